"""mn_sweep_form.h -- the form of a launch of the sweep (pixels per lane, class planes, lean outputs, where the group
records lie, how many partial sums come out), decided in one place from plain values -- HOST build of the text the
library launches by (tests/tools/sweep_form_check.cpp).  The expected values are the decision table worked out by
hand from the rules; none comes from the function under test.

CPU only.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mergenet_amd import segmenter as seg, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32, F16, BF16 = seg.MN_DTYPE_F32, seg.MN_DTYPE_F16, seg.MN_DTYPE_BF16
COMPONENTS, CORES, EXPORT, TIMING = 0, 1, 2, 3          # enum SweepAsker
A = [(0, 1), (1, 0), (1, 1)]
B = [tuple(int(x) for x in o) for o in synth.generate_offsets(40, 10)]
C = [(1, 1), (2, 0)]
NOT_LEAN = (-1, 0, 0, 0)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sweep_form") / "libsweep_form_host.so")
    src = os.path.join(ROOT, "tests", "tools", "sweep_form_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    i32p = ctypes.POINTER(ctypes.c_int)
    lib.sweep_form_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p]
    lib.sweep_form_check.restype = None
    return lib


def form(lib, H, W, offs, dtype=F32, logits=0, clip=0, sdb=0.0, aligned=1, flags=0, who=COMPONENTS):
    o = np.ascontiguousarray(np.asarray(offs, dtype=np.int32).reshape(-1, 2))
    out = np.zeros(14, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int)
    lib.sweep_form_check(H * W, W, len(offs), o.ctypes.data_as(i32p), dtype, logits, clip, sdb, aligned, flags, who,
                         out.ctypes.data_as(i32p))
    keys = ["px", "cls", "lean_cls", "lean_form", "plain", "kh", "packed", "rec0", "flag0", "blocks", "waves",
            "unit_kh", "unit_kv", "unit_dv"]
    f = {k: int(v) for k, v in zip(keys, out)}
    f["LO"] = (f["kh"], f["packed"], f["rec0"], f["flag0"])
    assert f["waves"] == 4 * f["blocks"]
    return f


def test_benchmark_shape_float32(host_lib):                                   # case 1
    assert B[1] == (0, 1)
    f = form(host_lib, 1024, 2048, B)
    assert (f["px"], f["cls"], f["lean_cls"], f["lean_form"]) == (4, 1, 1, 1)
    assert f["LO"] == (1, 1, 524288, 589824)
    assert f["waves"] == 8192


def test_sixteen_bit_maps_take_eight_pixels_where_they_can(host_lib):
    f = form(host_lib, 1024, 2048, B, dtype=BF16)                             # case 2
    assert (f["px"], f["waves"], f["LO"]) == (8, 4096, (1, 1, 524288, 589824))
    assert (f["cls"], f["lean_cls"], f["lean_form"]) == (1, 1, 1)
    assert form(host_lib, 1024, 2048, B, dtype=F16)["px"] == 8
    assert form(host_lib, 1024, 2048, B, dtype=BF16, flags=seg.MN_DEBUG_SWEEP16_4PX)["px"] == 4      # case 3
    assert form(host_lib, 1024, 2048, B, dtype=BF16, aligned=0)["px"] == 4                             # case 4
    assert form(host_lib, 24, 100, B, dtype=BF16)["px"] == 4                  # case 5: N % 8 == 0, W % 8 == 4


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_one_pixel_per_lane(host_lib, dtype):
    f = form(host_lib, 5, 7, B, dtype=dtype)                                  # case 6: N % 4 != 0
    assert (f["px"], f["cls"], f["lean_cls"], f["lean_form"]) == (1, 0, 0, 0)
    assert f["LO"] == NOT_LEAN and f["waves"] == 4
    f = form(host_lib, 64, 3, B, dtype=dtype)                                 # case 7: W < 4, N % 4 == 0
    assert (f["px"], f["cls"], f["lean_cls"], f["lean_form"], f["LO"]) == (1, 0, 0, 0, NOT_LEAN)


def test_lean_form_and_where_its_records_lie(host_lib):
    f = form(host_lib, 61, 100, A)                                            # case 8
    assert (f["px"], f["lean_form"], f["LO"], f["waves"]) == (4, 1, (0, 1, 1526, 1718), 24)
    f = form(host_lib, 4, 8, A)                                               # case 9: N = 32 < 64
    assert (f["px"], f["cls"], f["lean_cls"], f["lean_form"], f["LO"]) == (4, 1, 1, 0, NOT_LEAN)
    f = form(host_lib, 61, 100, A, flags=seg.MN_DEBUG_SWEEP_FULL_FORM)        # case 10
    assert (f["lean_cls"], f["lean_form"], f["LO"]) == (1, 0, NOT_LEAN)


def test_packing_limit_and_the_unit_step(host_lib):
    rest = [(i, j) for i in range(1, 5) for j in range(-4, 5) if (i, j) != (1, 0)]
    for O, packed in ((16, 1), (17, 0)):                                      # case 11
        offs = ([(1, 0), (0, 1)] + rest)[:O]
        f = form(host_lib, 61, 100, offs)
        assert len(offs) == O and (f["lean_form"], f["kh"], f["packed"]) == (1, 1, packed)
    f = form(host_lib, 61, 100, C)                                            # case 12: no (0, +1) in the list
    assert (f["lean_form"], f["kh"], f["packed"]) == (1, -1, 1)


@pytest.mark.parametrize("who", [CORES, EXPORT])
def test_cores_and_export_keep_the_full_form(host_lib, who):                  # case 13
    f = form(host_lib, 61, 100, A, who=who)
    assert (f["px"], f["cls"], f["lean_cls"], f["lean_form"], f["LO"], f["waves"]) == (4, 1, 0, 0, NOT_LEAN, 24)


def test_timing_loop_launches_the_product_form(host_lib):
    assert form(host_lib, 61, 100, A, who=TIMING) == form(host_lib, 61, 100, A, who=COMPONENTS)
    assert form(host_lib, 5, 7, A, who=TIMING) == form(host_lib, 5, 7, A, who=COMPONENTS)


def test_plain(host_lib):
    assert form(host_lib, 61, 100, A, dtype=F32, clip=0, sdb=0.0)["plain"] == 1                  # case 14
    assert form(host_lib, 61, 100, A, dtype=F32, clip=1)["plain"] == 0                           # case 15
    assert form(host_lib, 61, 100, A, dtype=BF16, clip=1)["plain"] == 1                          # case 16
    assert form(host_lib, 61, 100, A, dtype=F32, logits=1, clip=1)["plain"] == 1                 # case 17
    for dtype in (F32, F16, BF16):                                                               # case 18
        assert form(host_lib, 61, 100, A, dtype=dtype, clip=int(dtype != F32), sdb=0.5)["plain"] == 0


def test_unit_offsets(host_lib):
    """The first (0, +1) and the first (+-1, 0) of the list, with the latter's direction; -1 where there is none."""
    f = form(host_lib, 61, 100, A)
    assert (f["unit_kh"], f["unit_kv"], f["unit_dv"]) == (0, 1, 1)
    f = form(host_lib, 61, 100, [(2, 1), (-1, 0), (0, 1), (1, 0), (0, -1)])
    assert (f["unit_kh"], f["unit_kv"], f["unit_dv"]) == (2, 1, -1)
    f = form(host_lib, 61, 100, C)
    assert (f["unit_kh"], f["unit_kv"], f["unit_dv"]) == (-1, -1, 0)
