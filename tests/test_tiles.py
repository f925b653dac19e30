"""mergenet_amd.tiles -- the tile geometry of the reference and the numpy statement of Merger.tile_class_maps -- and
the C ABI of mn_tile_class_maps_device (no GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from mergenet_amd import tiles as mt
from tiles_util import CASES, make_case, tolerance, torch_composition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_starts_pinned_values():
    assert mt.tile_starts(1024, 713) == [0, 155, 311]
    assert mt.tile_starts(2048, 713) == [0, 445, 890, 1335]
    assert mt.tile_starts(24, 24) == [0, 0, 0]
    assert mt.tile_starts(37, 16) == [0, 7, 14, 21]
    assert mt.tile_starts(70, 24) == [0, 15, 30, 46]


def test_tile_starts_is_the_stated_formula():
    for size, side in ((1024, 713), (2048, 713), (53, 24), (200, 70), (33, 16)):
        n = int(size / float(side)) + 1
        stride = (size - side) / float(n)
        assert mt.tile_starts(size, side) == [int(i * stride) for i in range(n + 1)]
    with pytest.raises(ValueError):
        mt.tile_starts(10, 11)


def test_tile_starts_cover_every_pixel_and_end_at_the_border():
    for side in (8, 16, 33, 64, 100):
        for size in range(side, 4 * side + 50):
            starts = mt.tile_starts(size, side)
            assert starts[0] == 0 and starts == sorted(starts)
            assert starts[-1] + side == size, (size, side)
            cover = np.zeros(size, np.int64)
            for s in starts:
                assert 0 <= s and s + side <= size
                cover[s:s + side] += 1
            assert cover.min() >= 1, (size, side)


def test_cover_counts_of_the_cases():
    got = {}
    for name, (H, W, th, tw, *_rest) in CASES.items():
        cover = mt.tile_cover_count(mt.tile_starts(H, th), mt.tile_starts(W, tw), th, tw, H, W)
        got[name] = (int(cover.min()), int(cover.max()))
    assert got["a"] == (1, 9)             # ragged width; three row tiles times three column tiles in places
    assert got["c"] == (9, 9)             # nine tiles on one origin
    assert all(lo >= 1 for lo, _ in got.values())
    assert tolerance("a") == tolerance("e") == 40 * 2.0 ** -24         # 2.4e-6


def test_reference_on_a_hand_worked_case():
    """One row of 3 pixels, tiles 1 x 2 at columns 0 and 1, Cn = 3 -> C = 2.  Logits are logs of dyadic weights, so
    the softmax values are simple fractions."""
    w = np.array([[[[1.0, 2.0]], [[1.0, 1.0]], [[2.0, 1.0]]],          # tile 0: p = (1/4, 1/4, 1/2), (1/2, 1/4, 1/4)
                  [[[4.0, 1.0]], [[2.0, 1.0]], [[2.0, 2.0]]]])         # tile 1: p = (1/2, 1/4, 1/4), (1/4, 1/4, 1/2)
    tiles = np.log(w)
    out = mt.tile_class_maps_reference(tiles, None, [0], [0, 1], 1, 3, 2)
    assert out.shape == (2, 1, 3) and out.dtype == np.float64
    # pixel 0: tile 0 alone: q = (max(1/4, 1/4), 1/2) -> (1/3, 2/3) after the renormalisation
    # pixel 1: tiles 0 and 1: q = (1/2, 1/4) and (1/2, 1/4) -> s = (1/2, 1/4) -> (2/3, 1/3)
    # pixel 2: tile 1 alone: q = (1/4, 1/2) -> (1/3, 2/3)
    want = np.array([[[1 / 3, 2 / 3, 1 / 3]], [[2 / 3, 1 / 3, 2 / 3]]])
    assert np.abs(out - want).max() < 1e-15
    # the flipped pass is flipped back: tile t flipped = tile t's own columns reversed gives the same result
    out2 = mt.tile_class_maps_reference(tiles, tiles[:, :, :, ::-1], [0], [0, 1], 1, 3, 2)
    assert np.abs(out2 - want).max() < 1e-15
    # the maximum is taken AFTER the average: stuff classes (0.8, 0.1) and (0.1, 0.8) average to 0.45 each, not 0.8
    a = np.log(np.array([0.8, 0.1, 0.1])).reshape(1, 3, 1, 1)
    b = np.log(np.array([0.1, 0.8, 0.1])).reshape(1, 3, 1, 1)
    out3 = mt.tile_class_maps_reference(a, b, [0], [0], 1, 1, 2)
    assert np.abs(out3[:, 0, 0] - np.array([0.45, 0.1]) / 0.55).max() < 1e-15


def test_reference_refuses_bad_geometry():
    t = np.zeros((2, 3, 2, 2))
    with pytest.raises(ValueError):
        mt.tile_class_maps_reference(t, None, [0], [0, 3], 2, 4, 2)       # tile 1 leaves the image
    with pytest.raises(ValueError):
        mt.tile_class_maps_reference(t, None, [0], [0, 3], 2, 6, 2)       # column 2 uncovered
    with pytest.raises(ValueError):
        mt.tile_class_maps_reference(t, None, [0], [0, 2], 2, 4, 4)       # C > Cn
    with pytest.raises(ValueError):
        mt.tile_class_maps_reference(t, None, [0], [0, 1, 2], 2, 4, 2)    # 2 tiles for 3 starts


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_float32_composition_meets_the_bound(name):
    """The bound of the GPU tests is one that the reference's own float32 arithmetic meets."""
    tiles, flips, rows, cols, H, W, C = make_case(name)
    want = mt.tile_class_maps_reference(tiles, flips, rows, cols, H, W, C)
    got = torch_composition(tiles, flips, rows, cols, H, W, C)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("case %s: float32 torch composition off by %.3g (bound %.3g)" % (name, err, tolerance(name)))
    assert got.dtype == np.float32 and err <= tolerance(name)
    assert np.abs(want.sum(axis=0) - 1.0).max() < 1e-14


def test_entry_point_is_declared_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from mergenet_amd import segmenter as seg
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mn_tile_class_maps_device\s*\(([^)]*)\)\s*;", code)
    assert m, "include/mergenet_hip.h does not declare mn_tile_class_maps_device"
    assert len(m.group(1).split(",")) == 18
    assert "mn_tile_class_maps_device" in seg.EXPORTS
    fn = seg.load_library().mn_tile_class_maps_device
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 18
    assert fn.argtypes[3] is ctypes.c_int and fn.argtypes[15] is ctypes.c_int      # dtype, out_dtype
    assert "mn_kernels_tiles.h" in open(os.path.join(ROOT, "mergenet_amd", "csrc", "Makefile")).read()
    assert callable(seg.Merger.tile_class_maps)


def test_null_context_is_an_argument_error_without_a_gpu():
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    starts = (ctypes.c_int * 1)(0)
    p = ctypes.c_void_p(16)
    rc = lib.mn_tile_class_maps_device(None, p, None, 0, 3, 2, 2, starts, 1, starts, 1, 2, 2, 2, p, 0, 0, None)
    assert rc == -1
