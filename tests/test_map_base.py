"""The case table of map_base_util (test_gpu_map_base.py runs it on the device), held on the host:

* the pixels per lane the table states for every (shape, dtype, pair of bases) are what mn_sweep_form.h decides when
  it is told `aligned16 = both bases % 16 == 0` -- HOST build of the header the library launches by, as in
  test_sweep_form.py.  The table's values are literals written out from the rule, none comes from the function;
* the project's oracle, run on the float32 values the kernels see (the widened 16-bit maps, clipped), gives the
  union-find labelling on every shape in every dtype, so both references of the GPU tests agree before they are used;
* every case but the two of random labels has at most 1024 records between its components: the `tail` attempt of the
  GPU tests is the speculative one (mn_cc_tail) and not a redo of it.  The random labels' count is pinned.

CPU only.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import map_base_util as mb
import topology_util as tu
from mergenet_amd import segmenter as seg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPE_CODE = {"float32": seg.MN_DTYPE_F32, "float16": seg.MN_DTYPE_F16, "bfloat16": seg.MN_DTYPE_BF16}
COMPONENTS, EXPORT = 0, 2          # enum SweepAsker


@pytest.fixture(scope="module")
def form_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("map_base") / "libsweep_form_host.so")
    src = os.path.join(ROOT, "tests", "tools", "sweep_form_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    i32p = ctypes.POINTER(ctypes.c_int)
    lib.sweep_form_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, i32p]
    lib.sweep_form_check.restype = None
    return lib


def _form(lib, H, W, offs, dtype, aligned, flags, who):
    o = np.ascontiguousarray(np.asarray(offs, dtype=np.int32).reshape(-1, 2))
    out = np.zeros(14, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int)
    lib.sweep_form_check(H * W, W, len(offs), o.ctypes.data_as(i32p), DTYPE_CODE[dtype], 0, 1, 0.0, int(aligned), flags,
                         who, out.ctypes.data_as(i32p))
    return dict(px=int(out[0]), cls=int(out[1]), lean_form=int(out[3]))


def test_the_table_is_complete():
    assert set(mb.PX) == set(mb.SHAPES) == set(mb.HW)
    for shape, make in mb.SHAPES.items():
        assert make().shape == mb.HW[shape], shape
    assert len(mb.CASES) == 17 and set(mb.CASE_SHAPE.values()) == set(mb.SHAPES)
    assert [len(mb.pairs(d)) for d in mb.DTYPES] == [10, 13, 13]
    for dtype in mb.DTYPES:
        size = 4 if dtype == "float32" else 2
        for (a, b) in mb.pairs(dtype):
            assert a % size == 0 and b % size == 0 and 0 <= a < 16 and 0 <= b < 16
            assert (a, b) == (0, 0) or a != b
        assert set(mb.edge_pairs(dtype)) <= set(mb.pairs(dtype))


@pytest.mark.parametrize("who", [COMPONENTS, EXPORT])
@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("case", mb.CASES, ids=repr)
def test_table_states_the_form_the_header_decides(form_lib, case, dtype, who):
    H, W = case.lab.shape
    for pair in mb.pairs(dtype):
        aligned = pair[0] % 16 == 0 and pair[1] % 16 == 0
        f = _form(form_lib, H, W, case.offs, dtype, aligned, 0, who)
        assert f["px"] == mb.expected_px(mb.shape_of(case), dtype, pair), (case.name, dtype, pair, f)
        assert f["cls"] == int(f["px"] >= 4)
        # (the lean form: the components path of every shape of the table that takes four pixels or more)
        assert f["lean_form"] == int(who == COMPONENTS and f["px"] >= 4), (case.name, dtype, pair, f)
        f = _form(form_lib, H, W, case.offs, dtype, aligned, seg.MN_DEBUG_SWEEP_FULL_FORM, who)
        assert (f["px"], f["lean_form"]) == (mb.expected_px(mb.shape_of(case), dtype, pair), 0)
        if mb.shape_of(case) in mb.PX_16_4PX:
            f = _form(form_lib, H, W, case.offs, dtype, aligned, seg.MN_DEBUG_SWEEP16_4PX, who)
            assert f["px"] == mb.expected_px(mb.shape_of(case), dtype, pair, sweep16_4px=True), (case.name, dtype, pair, f)


def test_every_form_of_the_table_is_reached():
    """Float32 and 16-bit rows of 4 pixels, 16-bit rows of 8 that a misaligned base turns into 4, rows of 1."""
    rows = {(shape, dtype, pair): mb.expected_px(shape, dtype, pair)
            for shape in mb.SHAPES for dtype in mb.DTYPES for pair in mb.pairs(dtype)}
    assert set(rows.values()) == {1, 4, 8}
    eights = [k for k, v in rows.items() if v == 8]
    assert {k[0] for k in eights} == {"comb3-32x136", "serpentine-1-1-18x8"}
    assert all(k[1] != "float32" and k[2] == (0, 0) for k in eights)
    assert rows[("comb3-32x136", "bfloat16", (8, 0))] == 4 and rows[("comb3-32x136", "float16", (0, 2))] == 4
    # 17x68 in 16 bits: N % 8 == 4, so plane k of an aligned map starts 8 * (k % 2) bytes behind a 16-byte boundary
    H, W = mb.HW["serpentine-1-1-17x68"]
    assert [(k * H * W * 2) % 16 for k in range(4)] == [0, 8, 0, 8]


@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("case", mb.CASES, ids=repr)
def test_oracle_on_the_widened_maps_gives_the_union_find_labelling(oracle, case, dtype):
    cp, sp, _, _ = mb.host_maps(case.name, dtype)
    ref = oracle.run_csegment(cp, sp, tu.C, case.offs, *mb.OPTS)
    mask, classes, objects = mb.reference(case.name)
    assert oracle.same_partition(ref.partition, case.comp), (case.name, dtype)
    assert oracle.masks_equivalent(ref.mask, ref.object_class, mask, classes), (case.name, dtype)
    assert int(ref.stats["n_objects"]) == objects


@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("shape", ["comb3-32x136", "serpentine-1-1-17x68"])
def test_logits_keep_the_sign_of_every_edge(oracle, shape, dtype):
    """The logits of the GPU tests, rounded to the dtype, still give the union-find labelling through the oracle."""
    case = mb.FIRST_OF_SHAPE[shape]
    cx, sx, _, _ = mb.host_logits(case.name, dtype)
    assert np.isposinf(sx).any() and np.isfinite(cx).all()
    ref = oracle.run_csegment(mb.probabilities_of_logits(cx), mb.probabilities_of_logits(sx), tu.C, case.offs, *mb.OPTS)
    assert oracle.same_partition(ref.partition, case.comp), (shape, dtype)


# Three random labels per pixel and the unit offsets alone leave 1778 components with 4046 records between them: no
# 35x131 image of random labels stays below 1024.  On this shape -- the one-pixel-per-lane control -- the library redoes
# the `tail` attempt on the waited one after its labelling ran speculatively, as it does for three cases of
# test_gpu_topology.py; it stays in components mode (4046 is below the default finish_limit of 4096), which the GPU
# tests assert.
MORE_THAN_THE_TAIL_TAKES = {"random3-35x131-unit": 4046, "random3-35x131-up": 4046}


@pytest.mark.parametrize("case", mb.CASES, ids=repr)
def test_the_tail_attempt_is_the_speculative_one(case):
    if case.name in MORE_THAN_THE_TAIL_TAKES:
        assert 1024 < case.records == MORE_THAN_THE_TAIL_TAKES[case.name] <= 4096, case.name
    else:
        assert case.records <= 1024, case.name


def test_percolation_has_many_negative_edges():
    assert mb.BY_NAME["percolation-35x68-unit"].records == 468
