"""The rule for the uniform 64-pixel groups of the sweep's lean form, on the host (labels.uniform_groups is the numpy
twin of what mn_cc_sign decides per group; tests/test_gpu_lean_sweep.py uses it to know what its cases exercise).

The positive masks are built here straight from a label map: bit k of pixel p is set iff p + offset k is inside the
image and carries p's label -- what the sweep leaves on maps with sameness 0.95 inside a label and 0.05 across."""
import numpy as np
import pytest

from lean_util import pos_bits_of, stripes
from mergenet_amd import labels, synth


def by_definition(bits, offs):
    """The rule, pixel by pixel."""
    flat = [int(b) for b in bits.reshape(-1)]
    n = len(flat)
    out = []
    for g in range((n + 63) // 64):
        ok = (0, 1) in offs and 64 * g + 64 <= n
        if ok:
            k = offs.index((0, 1))
            ok = all((flat[p] >> k) & 1 for p in range(64 * g, 64 * g + 63))
        out.append(ok)
    return np.asarray(out, bool)


OFFS = [(int(i), int(j)) for (i, j) in synth.generate_offsets(40, 10)]


@pytest.mark.parametrize("H,W", [(32, 256), (24, 192), (24, 100), (30, 66), (17, 64), (17, 68), (9, 13)])
def test_one_label_everywhere(H, W):
    """All links positive: a group is uniform iff it is whole and does not cross a row's end."""
    bits = pos_bits_of(np.zeros((H, W), np.int32), OFFS)
    flags = labels.uniform_groups(bits, OFFS)
    N = H * W
    assert flags.shape == ((N + 63) // 64,)
    for g, f in enumerate(flags):
        whole = 64 * g + 64 <= N
        one_row = (64 * g) // W == (64 * g + 63) // W
        assert bool(f) == (whole and one_row), (H, W, g)
    assert np.array_equal(flags, by_definition(bits, OFFS))


def test_shapes_where_no_group_may_be_uniform():
    """W < 64: every whole group crosses a row's end.  Stripes narrower than 63 columns: every run of links is broken
    (the label maps of the GPU test's "no group" cases)."""
    for H, W in [(40, 60), (17, 36)]:
        assert not labels.uniform_groups(pos_bits_of(np.zeros((H, W), np.int32), OFFS), OFFS).any()
    for H, W in [(24, 100), (30, 66), (17, 64)]:
        bits = pos_bits_of(stripes(H, W, 20), OFFS)
        flags = labels.uniform_groups(bits, OFFS)
        assert not flags.any()
        assert np.array_equal(flags, by_definition(bits, OFFS))


def test_last_partial_group_is_never_uniform():
    H, W = 1, 100                            # groups [0, 64) and the partial [64, 100)
    flags = labels.uniform_groups(pos_bits_of(np.zeros((H, W), np.int32), OFFS), OFFS)
    assert flags.tolist() == [True, False]


def test_no_unit_offset_no_group():
    offs = [(1, 0), (0, 2), (3, 3)]
    assert not labels.uniform_groups(pos_bits_of(np.zeros((8, 256), np.int32), offs), offs).any()


def test_a_broken_link_and_the_64th_pixel():
    lab = np.zeros((2, 256), np.int32)
    lab[0, 70:] = 1                          # link 69 -> 70 broken: group 1 of row 0
    lab[1, 64:] = 2                          # link 63 -> 64 broken: the 64th pixel's own link, group 0 stays uniform
    bits = pos_bits_of(lab, OFFS)
    flags = labels.uniform_groups(bits, OFFS)
    assert flags.tolist() == [True, False, True, True, True, True, True, True]
    assert np.array_equal(flags, by_definition(bits, OFFS))


def test_random_label_maps_against_the_definition():
    rng = np.random.default_rng(5)
    for H, W in [(16, 128), (12, 70), (5, 333)]:
        lab = (rng.random((H, W)) < 0.02).cumsum(axis=1).astype(np.int32)
        bits = pos_bits_of(lab, OFFS)
        assert np.array_equal(labels.uniform_groups(bits, OFFS), by_definition(bits, OFFS))
