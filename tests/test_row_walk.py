"""mn_row_walk.h -- the walk of the passes that stream a label mask row by row (instance table, overlap table, map
scores): pixels per lane, chunks per row and per wave, the grid, a wave's span of chunks and the pixel of
(chunk, lane) -- HOST build of the text the library launches and the kernels walk by (tests/tools/row_walk_check.cpp).
The expected values are worked out by hand from the rules; none comes from the function under test:

    V               4 bytes per element: 4 where W % 4 == 0 and the bases are 16-byte aligned, else 1;
                    2 bytes: 8 where W % 8 == 0 and 16-byte aligned, else 4 where W % 4 == 0 and 8-byte aligned, else 1
    chunks_per_row  ceil(W / (64 V)),  total = H * chunks_per_row
    aimed (tables)  4 waves per workgroup, 256 workgroups aimed at: chunks_per_wave = ceil(total / 1024),
                    blocks = ceil(total / (4 * chunks_per_wave))
    fixed (scores)  blocks given -- truth_pass_slots of mn_truth_pass.h, held to the same hand-made grids below --
                    and chunks_per_wave = ceil(total / (4 * blocks))

The host part of mn_truth_pass.h is in the same build: truth_pass_slots, the grid of the passes over the maps and a
truth mask, and truth_pass_offsets, the clamp of their offsets.  The check program has a main of its own: built with
the address and undefined-behaviour sanitizers it answers the same tables as a child process (that build is never
loaded into this one).

CPU only.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WAVES_PER_BLOCK = 4            # MN_INST_THREADS / 64 = MN_OVL_THREADS / 64 = MN_MS_WAVES
AIM = 256                      # MN_INST_WORKGROUPS = MN_OVL_WORKGROUPS
ALIGNED, OFF4, OFF8 = 0x7F0000001000, 0x7F0000001004, 0x7F0000001008

# (H, W), element size, OR of the bases, grid of the fixed rule or None for the aimed one
#   -> V, chunks per row, total chunks, chunks per wave, blocks
TABLE = [
    ((1, 1), 4, ALIGNED, None, (1, 1, 1, 1, 1)),
    ((3, 5), 4, ALIGNED, None, (1, 1, 3, 1, 1)),              # wave 3 of the one workgroup: an empty span
    ((48, 256), 4, ALIGNED, None, (4, 1, 48, 1, 12)),
    ((48, 256), 4, OFF4, None, (1, 4, 192, 1, 48)),
    ((32, 1028), 4, ALIGNED, None, (4, 5, 160, 1, 40)),
    ((64, 1030), 4, ALIGNED, None, (1, 17, 1088, 2, 136)),
    ((345, 516), 4, ALIGNED, None, (4, 3, 1035, 2, 130)),     # 16-byte loads AND two chunks per wave, across row ends
    ((256, 1040), 4, ALIGNED, 160, (4, 5, 1280, 2, 160)),
    ((256, 1040), 4, OFF4, 160, (1, 17, 4352, 7, 160)),       # the same grid: 7 * 640 waves >= 4352
    ((16, 520), 2, ALIGNED, 4, (8, 2, 32, 2, 4)),
    ((9, 260), 2, ALIGNED, 2, (4, 2, 18, 3, 2)),              # W % 8 == 4; grid: ceil(9 * 1 / 8) = 2
    # shapes chosen to stress the cover
    ((5, 1), 4, ALIGNED, None, (1, 1, 5, 1, 2)),
    ((3, 63), 4, ALIGNED, None, (1, 1, 3, 1, 1)),
    ((3, 64), 4, ALIGNED, None, (4, 1, 3, 1, 1)),             # a quarter of the chunk's lanes inside the row
    ((3, 64), 4, OFF8, None, (1, 1, 3, 1, 1)),                # exactly one chunk of single pixels
    ((3, 65), 4, ALIGNED, None, (1, 2, 6, 1, 2)),             # one pixel in the row's second chunk
    ((1, 300), 4, ALIGNED, None, (4, 2, 2, 1, 1)),
    ((1, 1000), 4, OFF4, None, (1, 16, 16, 1, 4)),
    ((1, 1000), 2, ALIGNED, 1, (8, 2, 2, 1, 1)),              # grid: ceil(1 * 2 / 8) = 1
    ((1024, 2048), 4, ALIGNED, None, (4, 8, 8192, 8, 256)),   # the timing tools' mask
    ((1024, 2048), 2, ALIGNED, 512, (8, 4, 4096, 2, 512)),    # grid: min(1024, ceil(1024 * 4 / 8)) = 512
    ((1024, 2048), 2, OFF8, 512, (4, 8, 8192, 4, 512)),       # the same grid at V = 4: 4 chunks per wave
]

# truth_pass_slots: the grids TABLE gives by hand, and one shape that meets the cap of 1024 workgroups
# (8 chunks per row at 4 float32 values per lane: 4096 * 8 / 8 = 4096)
SLOTS = sorted({(shape, elem, grid) for shape, elem, _, grid, _ in TABLE if grid is not None}) + [((4096, 2048), 4, 1024)]

# truth_pass_offsets at (H, W) = (3, 5): each offset held to -3..3 / -5..5
OFFSETS_HW = (3, 5)
OFFSETS_IN = [(0, 1), (-3, 2), (3, 0), (0, -5), (4, -6), (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)]
OFFSETS_OUT = [(0, 1), (-3, 2), (3, 0), (0, -5), (3, -5), (3, -5), (-3, 5)]

SRC = os.path.join(ROOT, "tests", "tools", "row_walk_check.cpp")


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("row_walk") / "librow_walk_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    i32p, i64p = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
    lib.row_walk_v_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong]
    lib.row_walk_v_check.restype = ctypes.c_int
    lib.row_walk_check.argtypes = [ctypes.c_int] * 6 + [i32p]
    lib.row_walk_check.restype = None
    lib.row_walk_span_check.argtypes = [i32p, ctypes.c_longlong, i64p]
    lib.row_walk_span_check.restype = None
    lib.row_walk_cover.argtypes = [ctypes.c_int, ctypes.c_int, i32p, ctypes.c_int, i32p]
    lib.row_walk_cover.restype = ctypes.c_longlong
    lib.truth_pass_slots_check.argtypes = [ctypes.c_int] * 4
    lib.truth_pass_slots_check.restype = ctypes.c_int
    lib.truth_pass_offsets_check.argtypes = [i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p]
    lib.truth_pass_offsets_check.restype = None
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def walk(lib, shape, elem, bases, grid):
    H, W = shape
    v = lib.row_walk_v_check(W, elem, bases)
    out = np.zeros(5, np.int32)
    lib.row_walk_check(H, W, v, int(grid is not None), AIM if grid is None else grid, WAVES_PER_BLOCK, ptr(out))
    return out


def span(lib, r, wave):
    out = np.zeros(2, np.int64)
    lib.row_walk_span_check(ptr(r), wave, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
    return int(out[0]), int(out[1])


def test_pixels_per_lane(host_lib):
    v = host_lib.row_walk_v_check
    assert [v(256, 4, ALIGNED), v(256, 4, OFF4), v(256, 4, OFF8), v(1030, 4, ALIGNED)] == [4, 1, 1, 1]
    assert [v(1040, 4, ALIGNED), v(1040, 4, OFF8)] == [4, 1]                  # float32 maps: no 8-byte form
    assert [v(520, 2, ALIGNED), v(520, 2, OFF8), v(520, 2, OFF4)] == [8, 4, 1]
    assert [v(260, 2, ALIGNED), v(260, 2, OFF8), v(260, 2, OFF4), v(262, 2, ALIGNED)] == [4, 4, 1, 1]


@pytest.mark.parametrize("shape,elem,bases,grid,want", TABLE)
def test_geometry(host_lib, shape, elem, bases, grid, want):
    assert tuple(walk(host_lib, shape, elem, bases, grid)) == want


@pytest.mark.parametrize("shape,elem,bases,grid,want", TABLE)
def test_every_pixel_once_and_no_lane_across_a_row_end(host_lib, shape, elem, bases, grid, want):
    """The property each pass relies on: the spans of the grid's waves visit every pixel exactly once, and a lane
    with x < W has all its V pixels inside the row."""
    H, W = shape
    r = np.array(want, np.int32)                   # (the hand-made values: test_geometry holds the function to them)
    visits = np.zeros(H * W, np.int32)
    assert host_lib.row_walk_cover(H, W, ptr(r), WAVES_PER_BLOCK, ptr(visits)) == 0
    assert visits.min() == 1 and visits.max() == 1


def test_spans_are_clamped_at_both_ends(host_lib):
    r = np.array([1, 1, 3, 1, 1], np.int32)                                   # (3, 5)
    assert [span(host_lib, r, w) for w in range(4)] == [(0, 1), (1, 2), (2, 3), (3, 3)]
    assert span(host_lib, r, 10 ** 6) == (3, 3)
    r = np.array([4, 3, 1035, 2, 130], np.int32)                              # (345, 516)
    assert span(host_lib, r, 1) == (2, 4)                                     # chunk 2 ends row 0, chunk 3 begins row 1
    assert span(host_lib, r, 517) == (1034, 1035)                             # the last wave with work: half a share
    assert span(host_lib, r, 518) == (1035, 1035) and span(host_lib, r, 519) == (1035, 1035)
    r = np.array([1, 2 ** 20, 2 ** 31 - 1, 2 ** 21, 256], np.int32)           # far waves: no overflow of the product
    assert span(host_lib, r, 2 ** 40) == (2 ** 31 - 1, 2 ** 31 - 1)


def test_slots_table_holds_the_five_hand_made_grids():
    assert SLOTS[:-1] == sorted([((256, 1040), 4, 160), ((16, 520), 2, 4), ((9, 260), 2, 2), ((1, 1000), 2, 1),
                                 ((1024, 2048), 2, 512)])


@pytest.mark.parametrize("shape,elem,grid", SLOTS)
def test_truth_pass_slots(host_lib, shape, elem, grid):
    assert host_lib.truth_pass_slots_check(shape[0], shape[1], elem, WAVES_PER_BLOCK) == grid


def test_truth_pass_offsets(host_lib):
    H, W = OFFSETS_HW
    off = np.array(OFFSETS_IN, np.int32)
    out = np.full_like(off, 99)
    host_lib.truth_pass_offsets_check(ptr(off), len(OFFSETS_IN), H, W, ptr(out))
    assert [tuple(int(x) for x in row) for row in out] == OFFSETS_OUT
    host_lib.truth_pass_offsets_check(None, 0, H, W, None)         # no offsets: nothing is read or written


def test_truth_pass_rules_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "row_walk_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover", SRC, "-o", exe], check=True)
    H, W = OFFSETS_HW
    args, want = [], []
    for shape, elem, grid in SLOTS:
        args += ["slots", shape[0], shape[1], elem, WAVES_PER_BLOCK]
        want.append(str(grid))
    args += ["offsets", H, W, len(OFFSETS_IN)] + [x for pair in OFFSETS_IN for x in pair]
    want.append(" ".join(str(x) for pair in OFFSETS_OUT for x in pair))
    args += ["offsets", H, W, 0]
    want.append("")
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.split("\n")[:-1] == want, res.stdout + res.stderr
