"""mn_cc_tiles4 -- the tile stage of the labelling with four pixels per lane -- on tiles4_util's cases: winding shapes
at widths divisible by 4, where the library takes it (W % 4 == 0, 16-byte aligned arrays, MN_DEBUG_TILES_1PX off).

The checks are test_gpu_topology.py's own (_check_components: the partition must be EXACTLY topology_util.components
of the label map, the mask and classes the reference's, the certificate clean, total_logprob within 1e-5 relative of
the oracle's, two calls on one Merger bit-equal), on both attempts and -- serpentines, combs, percolation -- under the
sweep's full form.  On one Merger per case a call with MN_DEBUG_TILES_1PX (mn_cc_tiles, one pixel per lane) must
return mask, table and partition equal bit for bit to the default call's: parent[] is a function of the masks alone.
The cores run as test_gpu_topology.py::test_cores_on_winding_centre_lines runs them.
"""
import numpy as np
import pytest

import test_gpu_topology as tgt
import tiles4_util as t4
import topology_util as tu
from mergenet_amd import segmenter as seg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("attempt", list(tgt.ATTEMPTS))
@pytest.mark.parametrize("case", t4.CASES, ids=repr)
def test_labelling_is_the_union_find_partition(oracle, case, attempt):
    tgt._check_components(case, oracle, **tgt.ATTEMPTS[attempt])


@pytest.mark.parametrize("attempt", list(tgt.ATTEMPTS))
@pytest.mark.parametrize("case", t4.FORM_CASES, ids=repr)
def test_labelling_under_the_full_sweep_form(oracle, case, attempt):
    tgt._check_components(case, oracle, debug_flags=seg.MN_DEBUG_SWEEP_FULL_FORM, **tgt.ATTEMPTS[attempt])


@pytest.mark.parametrize("case", t4.CASES, ids=repr)
def test_one_pixel_kernel_gives_the_same_bits(oracle, case):
    e = tgt._expect(case, oracle)
    H, W = case.lab.shape
    merger = seg.Merger(H, W, tu.C, len(case.offs))
    try:
        got = []
        for flags in (0, seg.MN_DEBUG_TILES_1PX):
            o = seg.default_options(same_different_bias=tgt.OPTS[0], object_merge_factor=tgt.OPTS[1],
                                    merge_logprob_bias=tgt.OPTS[2], mode=seg.MN_MODE_COMPONENTS, clip_inputs=1,
                                    compute_logprob=1, debug_flags=flags)
            got.append(tgt._call(merger, e, case, o))
    finally:
        merger.close()
    for mask, table, part, st in got:
        assert st["status"] == 0 and st["mode_used"] == seg.MN_MODE_COMPONENTS, (case.name, st)
    assert oracle.same_partition(got[0][2], case.comp), case.name
    for name, a, b in zip(("mask", "table", "partition"), got[0], got[1]):
        assert np.array_equal(a, b), (name, case.name)


@pytest.mark.parametrize("case", t4.CORE_CASES, ids=repr)
def test_cores_on_winding_centre_lines(oracle, case):
    tgt.test_cores_on_winding_centre_lines(oracle, case)
