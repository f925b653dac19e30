"""The labelling chain of components mode -- mn_cc_tiles, mn_cc_borders, mn_cc_flatten, mn_cc_hook and what reads
parent[] behind them -- on winding shapes, against a union-find reference that is not the project's oracle.

Inputs are label maps of topology_util (serpentines, spirals, combs, staircases through a tile corner, chains of blobs
joined by one long offset, percolation clusters, random labels) turned into maps by lean_util.maps_from_labels.  With
the options (0, 1, 0) nothing merges after the first phase, so the partition a call returns must be EXACTLY
topology_util.components(label map, offsets): integer comparisons, no tolerance but the 1e-5 relative on
total_logprob that test_gpu_parity.py uses (there the reference is the csegment oracle; test_topology.py holds the
oracle's partition to the same union-find on every case, on the CPU).

Every case asserts status == 0 and mode_used == MN_MODE_COMPONENTS (MN_MODE_ROUNDS for the cores): a call that fell
back would prove nothing about the labelling.  No shape of the table had to be shrunk or left out for that.  Every
case is run twice on one Merger and the two results must be bit-equal: the order in which the lock-free stages hook
is racy, their result must not be.

Forms.  `tail`: default options, the speculative attempt that ends in mn_cc_tail.  It takes at most 1024 records
between components; three cases have more (test_topology.py::test_which_cases_leave_the_fused_tail:
percolation-48x130-unit and -up with 1314, random3-35x131-diag with 1159) and are redone by the library on the waited
attempt after their labelling ran speculatively -- still COMPONENTS.  `waited`: finish_limit above MN_FIN2_MAXR, the
ordinary attempt (mn_cc_certificate + mn_verify_records), on every case.  MN_DEBUG_SWEEP_FULL_FORM: the full form of
the sweep's outputs (mn_cc_sums instead of mn_cc_sums_lean) on the serpentine, comb and chain cases; of these the
shapes with N % 4 == 0 (32x128, 16x64, 34x66, 32x132, 40x136) are the ones where the two forms differ, the others
take one pixel per lane and mn_cc_class_sums either way.
"""
import numpy as np
import pytest
import torch

import lean_util
import topology_util as tu
from mergenet_amd import segmenter as seg

pytestmark = pytest.mark.gpu

WAITED = 8193        # finish_limit above MN_FIN2_MAXR = 8192: the ordinary (waited) components attempt
ATTEMPTS = {"tail": {}, "waited": dict(finish_limit=WAITED)}
OPTS = (0.0, 1.0, 0.0)

_expected = {}


def _expect(case, oracle):
    """Per case, computed once and left alone: the maps on the device, the reference labelling with its mask and
    classes, the oracle's total_logprob."""
    e = _expected.get(case.name)
    if e is None:
        cp, sp = lean_util.maps_from_labels(case.lab, tu.CLASS_OF_LABEL, tu.C, case.offs)
        mask, classes = tu.reference_mask(case.comp, case.lab, tu.CLASS_OF_LABEL)
        ref = oracle.run_csegment(cp, sp, tu.C, case.offs, *OPTS)
        e = _expected[case.name] = dict(cp=torch.from_numpy(cp).cuda(), sp=torch.from_numpy(sp).cuda(), mask=mask,
                                        classes=classes, objects=tu.count(case.comp), logprob=ref.total_logprob)
    return e


def _call(merger, e, case, opts):
    mask, table, part, st = merger.segment(e["cp"], e["sp"], case.offs, opts, want_partition=True)
    torch.cuda.synchronize()
    return mask.cpu().numpy(), table.cpu().numpy(), part.cpu().numpy(), st


def _segment_twice(case, oracle, mode, **kw):
    e = _expect(case, oracle)
    H, W = case.lab.shape
    merger = seg.Merger(H, W, tu.C, len(case.offs))
    try:
        o = seg.default_options(same_different_bias=OPTS[0], object_merge_factor=OPTS[1], merge_logprob_bias=OPTS[2],
                                mode=mode, clip_inputs=1, compute_logprob=1, **kw)
        return e, _call(merger, e, case, o), _call(merger, e, case, o)
    finally:
        merger.close()


def _check_components(case, oracle, **kw):
    e, first, second = _segment_twice(case, oracle, seg.MN_MODE_COMPONENTS, **kw)
    mask, table, part, st = first
    ctx = (case.name, kw, st)
    print("TOPOLOGY %s %s records %d objects %d (reference %d) logprob %.9g (oracle %.9g)" %
          (case.name, kw, case.records, st["num_objects"], e["objects"], st["total_logprob"], e["logprob"]))
    assert st["status"] == 0 and st["mode_used"] == seg.MN_MODE_COMPONENTS, ctx
    assert oracle.same_partition(part, case.comp), ctx
    assert st["num_objects"] == e["objects"], ctx
    got_classes = [int(c) for c in table[:st["num_instances"]]]
    assert oracle.masks_equivalent(mask, got_classes, e["mask"], e["classes"]), ctx
    assert st["certified"] == 1, ctx
    assert (st["cert_edge_violations"], st["cert_class_violations"], st["cert_record_violations"]) == (0, 0, 0), ctx
    assert abs(st["total_logprob"] - e["logprob"]) <= 1e-5 * abs(e["logprob"]), ctx
    for name, a, b in zip(("mask", "table", "partition"), first, second):
        assert np.array_equal(a, b), (name, ctx)
    assert second[3]["status"] == 0 and second[3]["mode_used"] == seg.MN_MODE_COMPONENTS, ctx


@pytest.mark.parametrize("attempt", list(ATTEMPTS))
@pytest.mark.parametrize("case", tu.CASES, ids=repr)
def test_labelling_is_the_union_find_partition(oracle, case, attempt):
    """Every case of the table on both attempts, in the lean form wherever the shape has one."""
    _check_components(case, oracle, **ATTEMPTS[attempt])


FORM_CASES = [c for c in tu.CASES if c.name.startswith(("serpentine", "comb", "chain"))]


@pytest.mark.parametrize("attempt", list(ATTEMPTS))
@pytest.mark.parametrize("case", FORM_CASES, ids=repr)
def test_labelling_under_the_full_sweep_form(oracle, case, attempt):
    """MN_DEBUG_SWEEP_FULL_FORM: mn_cc_sums reads parent[] where the default call's mn_cc_sums_lean did."""
    _check_components(case, oracle, debug_flags=seg.MN_DEBUG_SWEEP_FULL_FORM, **ATTEMPTS[attempt])


@pytest.mark.parametrize("case", tu.CORE_CASES, ids=repr)
def test_cores_on_winding_centre_lines(oracle, case):
    """MN_MODE_ROUNDS with core_radius = 1: the same four labelling kernels on the mn_core_bits masks, as the first
    step of the rounds.  The clean pixels are the centre lines of arms, teeth and blobs three pixels wide, so the cores
    wind as the shapes do (test_topology.py::test_core_cases_are_three_pixels_wide).  mn_kernels_cc.h claims the rounds
    from the cores are exact on sign-separable maps: the partition must be the reference's, and no core condemned."""
    e, first, _ = _segment_twice(case, oracle, seg.MN_MODE_ROUNDS, core_radius=1)
    mask, table, part, st = first
    ctx = (case.name, st)
    assert st["status"] == 0 and st["mode_used"] == seg.MN_MODE_ROUNDS, ctx
    assert oracle.same_partition(part, case.comp), ctx
    got_classes = [int(c) for c in table[:st["num_instances"]]]
    assert oracle.masks_equivalent(mask, got_classes, e["mask"], e["classes"]), ctx
    assert st["cores_condemned"] == 0, ctx
