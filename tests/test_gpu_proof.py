"""mn_stats.proof -- the CLAIM that goes with a mask -- held to the reference's own order on the GPU box.

proof 2 says: the reference's sequential order, nothing left to a tie rule.  MN_MODE_AUTO, require_proof and
tie_order = MN_TIES_DEFAULT all act on it: an image the exact engine calls proof 2 is never redone in the reference's
order.  Reference: RunSegmentation + Merge, utils/csegment/segment.cc:539-573, 602-727; its order among bit-equal
priorities is its std::priority_queue's (segment.h:270-275), restated by the CPU oracle (oracle/csegment_oracle.cpp)
that judges every fresh input here.  tests/tools/exact_model.cpp is the CPU model of the engine's own rule (lowest
record id among equals) and of its tie-conflict criterion.  Counts, partitions and proof: no tolerance.
"""
import os
import sys

import numpy as np
import pytest

import golden_util as gu
import test_exact_model as tm
from mergenet_amd import segmenter as seg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import exact_model  # noqa: E402

pytestmark = pytest.mark.gpu

EXPECTED_NO_CONFLICT = tm.EXPECTED_NO_CONFLICT      # (pinned in tests/test_exact_model.py, where the CPU suite asserts it too)
EXPECTED_CONFLICT = tm.EXPECTED_CONFLICT


def _options(opts, **kw):
    sdb, omf, bias = opts
    return seg.default_options(same_different_bias=sdb, object_merge_factor=omf, merge_logprob_bias=bias,
                               clip_inputs=1, **kw)


# ---- 1. fresh tied inputs: the claim against the reference's own order -----------------------------------------
@pytest.mark.parametrize("H,W,seed", tm.FRESH_TIED)
def test_proof_claim_on_fresh_tied_inputs(oracle, H, W, seed):
    """Inputs the engine was not tuned on, all with tied pops; on about half of them the tied choices provably commute.
    The reference-order loop must pop what the reference pops; the exact engine under its own rule must be the CPU
    model, event for event and verdict for verdict; and wherever it says proof == 2 the partition, the mask and the
    merge count ARE the reference's (on seed 8100 the lowest-id rule ends elsewhere: proof must be 3 there).  Default
    options: proven on every input, redone in the reference's order exactly where the verdict is "conflict"."""
    s, offs = tm.fresh_tied_input(H, W, seed)
    cp, sp = s.class_probs, s.sameness_probs
    sdb, omf, bias = tm.FRESH_OPTS
    ref = oracle.run_csegment(cp, sp, 9, offs, sdb, omf, bias)
    mpart, mcls, m = exact_model.run(cp, sp, offs, omf, bias)
    conflict = tm.expected_conflict(H, W, seed)
    assert m["tied_steps"] > 0 and (m["tied_conflicts"] > 0) == conflict, m      # (the pinned table still holds)
    ctx = seg.HostContext(H, W, 9, len(offs))
    try:
        r_ref = ctx.segment(cp, sp, offs, _options(tm.FRESH_OPTS, mode=seg.MN_MODE_EXACT, tie_order=seg.MN_TIES_REFERENCE))
        r_low = ctx.segment(cp, sp, offs, _options(tm.FRESH_OPTS, mode=seg.MN_MODE_EXACT, tie_order=seg.MN_TIES_LOWEST_ID))
        r_def = ctx.segment(cp, sp, offs, _options(tm.FRESH_OPTS))
    finally:
        ctx.close()

    # MN_TIES_REFERENCE: the reference's loop itself, stale queue entries included
    mask, classes, part, st = r_ref
    assert oracle.same_partition(part, ref.partition), st
    assert st["finisher_steps"] == ref.stats["n_pops"], (st["finisher_steps"], ref.stats["n_pops"])
    assert st["merges"] == ref.stats["n_merges"], (st["merges"], ref.stats["n_merges"])
    assert st["proof"] == seg.MN_PROOF_SEQUENTIAL and st["tie_order_used"] == seg.MN_TIES_REFERENCE, st
    assert abs(st["total_logprob"] - ref.total_logprob) <= 1e-5 * abs(ref.total_logprob)

    # MN_TIES_LOWEST_ID.  The claim first: proof == 2 => the reference's result
    mask, classes, part, st = r_low
    assert st["tie_order_used"] == seg.MN_TIES_LOWEST_ID, st
    assert st["proof"] in (seg.MN_PROOF_SEQUENTIAL, seg.MN_PROOF_SEQUENTIAL_TIES), st
    if st["proof"] == seg.MN_PROOF_SEQUENTIAL:
        assert oracle.same_partition(part, ref.partition), ("proof 2 on a partition that is not the reference's", st)
        assert oracle.masks_equivalent(mask, classes, ref.mask, ref.object_class), st
        assert st["merges"] == ref.stats["n_merges"], (st["merges"], ref.stats["n_merges"])
    # ... then the engine against the CPU model of its own rule
    assert (st["finisher_steps"], st["merges"], st["tied_steps"]) == (m["steps"], m["merges"], m["tied_steps"]), (st, m)
    assert (st["tied_conflicts"] > 0) == (m["tied_conflicts"] > 0), (st, m)
    assert oracle.same_partition(part, mpart), st
    if conflict:
        assert st["proof"] == seg.MN_PROOF_SEQUENTIAL_TIES, st
    else:
        assert st["proof"] == seg.MN_PROOF_SEQUENTIAL and st["tied_conflicts"] == 0, st
    if seed == tm.WITNESS_SEED:
        assert not oracle.same_partition(part, ref.partition)      # (the 3 is not idle caution)

    # default options (MN_MODE_AUTO): within MN_TIE_LIMIT_RECORDS, so proven either way
    mask, classes, part, st = r_def
    if st["certified"]:        # (blurred maps are not sign-separable: not expected, but a certificate would be right too)
        assert st["proof"] == seg.MN_PROOF_CERTIFICATE, st
    else:
        assert st["proof"] == seg.MN_PROOF_SEQUENTIAL and st["mode_used"] == seg.MN_MODE_EXACT, st
        assert st["tie_order_used"] == (seg.MN_TIES_REFERENCE if conflict else seg.MN_TIES_LOWEST_ID), st
    assert oracle.same_partition(part, ref.partition), st
    assert oracle.masks_equivalent(mask, classes, ref.mask, ref.object_class), st


# ---- 2. the conservative fall-back: ties that cannot be followed count as a conflict ---------------------------
def _fallback_inputs(oracle, which):
    if which == "fresh_8103":
        s, offs = tm.fresh_tied_input(64, 128, 8103)
        ref = oracle.run_csegment(s.class_probs, s.sameness_probs, 9, offs, *tm.FRESH_OPTS)
        return s.class_probs, s.sameness_probs, offs, tm.FRESH_OPTS, ref.mask, ref.object_class
    g = gu.load(which)
    return g["class_probs"], g["sameness_probs"], g["offsets"], tuple(g["spec"]["opts"]), g["mask"], g["object_class"]


@pytest.mark.parametrize("which", ["fresh_8103", "cseg_blur_64x128_r2_s8001"])
def test_untracked_ties_are_reported_as_a_conflict(oracle, monkeypatch, which):
    """When the engine cannot follow the ties (here: tracking switched off by MN_X_NO_TIE_TRACKING, read per run) a
    tied pop must count as a conflict: tied_conflicts >= 1 and proof 3 under the engine's own rule, and the default
    policy redoes the image in the reference's order.  With tracking, the same two inputs have tied pops that
    provably commute: proof 2, no conflict, nothing redone.
    The other two ways into that branch -- nesting stack full (tdepth >= MN_X_TSTACK = 1024) and the event counter
    near 2^31 -- are not reached: the stack holds one entry per pop of a run of non-decreasing priorities, an input
    that nests 1024 of them would have to be constructed against the float32 priority formula, and 2^31 pops take
    hours; the product build has no knob for either, and none was added for this test."""
    cp, sp, offs, opts, ref_mask, ref_classes = _fallback_inputs(oracle, which)
    H, W = cp.shape[1:]
    ctx = seg.HostContext(H, W, cp.shape[0], len(offs))
    try:
        monkeypatch.delenv("MN_X_NO_TIE_TRACKING", raising=False)
        t_low = ctx.segment(cp, sp, offs, _options(opts, mode=seg.MN_MODE_EXACT, tie_order=seg.MN_TIES_LOWEST_ID))
        t_def = ctx.segment(cp, sp, offs, _options(opts))
        monkeypatch.setenv("MN_X_NO_TIE_TRACKING", "1")
        u_low = ctx.segment(cp, sp, offs, _options(opts, mode=seg.MN_MODE_EXACT, tie_order=seg.MN_TIES_LOWEST_ID))
        u_def = ctx.segment(cp, sp, offs, _options(opts))
    finally:
        ctx.close()
    # tracked: proven under the engine's own rule
    for mask, classes, part, st in (t_low, t_def):
        assert st["tied_steps"] > 0 and st["tied_conflicts"] == 0 and st["proof"] == seg.MN_PROOF_SEQUENTIAL, st
        assert st["tie_order_used"] == seg.MN_TIES_LOWEST_ID, st
        assert oracle.masks_equivalent(mask, classes, ref_mask, ref_classes), st
    # untracked: the same pops, called a conflict
    mask, classes, part, st = u_low
    assert st["tied_steps"] == t_low[3]["tied_steps"] and st["finisher_steps"] == t_low[3]["finisher_steps"], st
    assert st["tied_conflicts"] >= 1 and st["proof"] == seg.MN_PROOF_SEQUENTIAL_TIES, st
    assert st["tie_order_used"] == seg.MN_TIES_LOWEST_ID
    assert np.array_equal(part, t_low[2])                # (the verdict changes the claim, not the result)
    # ... and the default policy acts on it
    mask, classes, part, st = u_def
    assert st["tie_order_used"] == seg.MN_TIES_REFERENCE and st["proof"] == seg.MN_PROOF_SEQUENTIAL, st
    assert st["tied_steps"] > 0 and st["tied_conflicts"] >= 1, st       # (what the exact engine met)
    assert oracle.masks_equivalent(mask, classes, ref_mask, ref_classes), st


# ---- 3. require_proof in a batch ---------------------------------------------------------------------------------
BATCH_128 = ["cseg_blur4_128x256_s5100", "cseg_blur4_128x256_s5103", "cseg_synth_128x256"]


def _batch_setup(names):
    import torch
    gs = [gu.load(n) for n in names]
    g0 = gs[0]
    H, W, C = g0["spec"]["H"], g0["spec"]["W"], g0["spec"]["C"]
    for g in gs:
        assert (g["spec"]["H"], g["spec"]["W"], g["spec"]["C"], g["spec"]["opts"]) == (H, W, C, g0["spec"]["opts"])
        assert np.array_equal(np.asarray(g["offsets"]), np.asarray(g0["offsets"]))
    cps = [torch.from_numpy(np.ascontiguousarray(g["class_probs"], dtype=np.float32)).cuda() for g in gs]
    sps = [torch.from_numpy(np.ascontiguousarray(g["sameness_probs"], dtype=np.float32)).cuda() for g in gs]
    return gs, (H, W, C, len(g0["offsets"])), cps, sps


def _to_host(res):
    return [(mask.cpu().numpy(), seg._class_list(table.cpu().numpy()), part.cpu().numpy(), st)
            for mask, table, part, st in res]


def test_a_batch_honours_require_proof(oracle, monkeypatch):
    """mn_segment_exact_batch with require_proof = 1: results are those of separate require_proof = 1 calls.
    MN_TIE_LIMIT = 1000 keeps the tie policy from redoing anything (the stand-in for an image above
    MN_TIE_LIMIT_BATCH_RECORDS): without require_proof the tie-decided images come back proof 3 under the engine's own
    rule; with it every result is proven -- those images redone in the reference's order and equal to the reference,
    still reporting the tied pops the exact engine met, an image that was proven already left alone -- and the same
    as three single calls."""
    monkeypatch.setenv("MN_TIE_LIMIT", "1000")
    gs, (H, W, C, O), cps, sps = _batch_setup(BATCH_128)
    opts = gs[0]["spec"]["opts"]
    offs = gs[0]["offsets"]
    batch = seg.ExactBatch(H, W, C, O, len(gs))
    try:
        res0 = _to_host(batch.segment(cps, sps, offs, _options(opts, mode=seg.MN_MODE_EXACT, require_proof=0),
                                      want_partition=True))
        res1 = _to_host(batch.segment(cps, sps, offs, _options(opts, mode=seg.MN_MODE_EXACT,
                                                               require_proof=seg.MN_PROVE_ALWAYS), want_partition=True))
    finally:
        batch.close()
    one = seg.Merger(H, W, C, O)
    try:
        single = _to_host([one.segment(cps[i], sps[i], offs, _options(opts, mode=seg.MN_MODE_EXACT,
                                                                      require_proof=seg.MN_PROVE_ALWAYS),
                                       want_partition=True) for i in range(len(gs))])
    finally:
        one.close()
    redone = 0
    for n, g, r0, r1, r2 in zip(BATCH_128, gs, res0, res1, single):
        st0, st1, st2 = r0[3], r1[3], r2[3]
        assert st0["status"] == 0 and st1["status"] == 0
        if "blur4" in n:                      # require_proof = 0: today's behaviour, kept
            assert st0["proof"] == seg.MN_PROOF_SEQUENTIAL_TIES and st0["tie_order_used"] == seg.MN_TIES_LOWEST_ID, (n, st0)
            assert st0["tied_steps"] > 0 and st0["tied_conflicts"] > 0, (n, st0)
        assert st1["proof"] in (seg.MN_PROOF_CERTIFICATE, seg.MN_PROOF_SEQUENTIAL), (n, st1)
        if st0["proof"] == seg.MN_PROOF_SEQUENTIAL_TIES:
            redone += 1
            assert st1["tie_order_used"] == seg.MN_TIES_REFERENCE and st1["proof"] == seg.MN_PROOF_SEQUENTIAL, (n, st1)
            assert (st1["tied_steps"], st1["tied_conflicts"]) == (st0["tied_steps"], st0["tied_conflicts"]), (n, st0, st1)
        else:                                 # proven already: not redone
            assert (st1["proof"], st1["tie_order_used"]) == (st0["proof"], st0["tie_order_used"]), (n, st0, st1)
            assert np.array_equal(r1[2], r0[2])
        assert oracle.masks_equivalent(r1[0], r1[1], g["mask"], g["object_class"]), (n, st1)
        # "Results are those of `count` separate MN_MODE_EXACT calls"
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[2], r2[2]) and r1[1] == r2[1], n
        for k in ("proof", "tie_order_used", "merges", "num_instances", "num_objects"):
            assert st1[k] == st2[k], (n, k, st1[k], st2[k])
    assert redone >= 2


PY_TIE_CONFLICT = "py_synth_64x128_n60_raw"       # (synth-v1's clipped plateaus: tied choices conflict within the first steps)
PY_BATCH = ["py_synth_64x128_n15_raw", PY_TIE_CONFLICT]      # (one shape, one option set)
PY_NO_CONFLICT = "py_adv_40x40_o1_raw"


def _py_options(g, **kw):
    sdb, omf, bias = g["spec"]["opts"]
    return seg.default_options(same_different_bias=sdb, object_merge_factor=omf, merge_logprob_bias=bias, clip_inputs=1,
                               variant=seg.MN_VARIANT_PYSEGMENTER, mode=seg.MN_MODE_EXACT,
                               prune_threshold=200.0 if g["spec"]["prune"] else float("-inf"), **kw)


def test_python_variant_with_conflicting_ties_is_unproven_under_require_proof(oracle):
    """The Python variant's heapq / dict order among equals is not restated, so a result whose tied choices conflict
    cannot be redone in the reference's order: require_proof = 1 answers MN_ERR_UNPROVEN; without require_proof the
    same call succeeds and says proof 3.  A vector without a tie conflict passes with proof 2."""
    g = gu.load(PY_TIE_CONFLICT)
    H, W, C = g["spec"]["H"], g["spec"]["W"], g["spec"]["C"]
    ctx = seg.HostContext(H, W, C, len(g["offsets"]))
    try:
        mask, classes, part, st = ctx.segment(g["class_probs"], g["sameness_probs"], g["offsets"], _py_options(g))
        assert st["tied_conflicts"] > 0 and st["proof"] == seg.MN_PROOF_SEQUENTIAL_TIES, st
        assert oracle.masks_equivalent(mask, classes, g["mask"], g["object_class"]), st
        with pytest.raises(seg.MergeNetError) as e:
            ctx.segment(g["class_probs"], g["sameness_probs"], g["offsets"],
                        _py_options(g, require_proof=seg.MN_PROVE_ALWAYS))
        assert e.value.status == seg.MN_ERR_UNPROVEN
    finally:
        ctx.close()
    g = gu.load(PY_NO_CONFLICT)
    H, W, C = g["spec"]["H"], g["spec"]["W"], g["spec"]["C"]
    ctx = seg.HostContext(H, W, C, len(g["offsets"]))
    try:
        mask, classes, part, st = ctx.segment(g["class_probs"], g["sameness_probs"], g["offsets"],
                                              _py_options(g, require_proof=seg.MN_PROVE_ALWAYS))
    finally:
        ctx.close()
    assert st["proof"] == seg.MN_PROOF_SEQUENTIAL and st["tied_conflicts"] == 0, st
    assert oracle.masks_equivalent(mask, classes, g["mask"], g["object_class"]), st


def test_a_batch_marks_the_unproven_python_variant_image_only(oracle):
    """A Python-variant batch under require_proof = 1 that holds an image whose tied choices conflict returns
    MN_ERR_UNPROVEN, with stats[i].status == MN_ERR_UNPROVEN on that image only and valid output for every image:
    proof 3 and the golden mask for the unproven one, a proven result for its companion.  ExactBatch.segment hands the
    results over on the exception."""
    gs, (H, W, C, O), cps, sps = _batch_setup(PY_BATCH)
    batch = seg.ExactBatch(H, W, C, O, len(gs))
    try:
        with pytest.raises(seg.MergeNetError) as e:
            batch.segment(cps, sps, gs[0]["offsets"], _py_options(gs[0], require_proof=seg.MN_PROVE_ALWAYS),
                          want_partition=True)
        assert e.value.status == seg.MN_ERR_UNPROVEN
        res = _to_host(e.value.results)
    finally:
        batch.close()
    for n, g, (mask, classes, part, st) in zip(PY_BATCH, gs, res):
        if n == PY_TIE_CONFLICT:
            assert st["status"] == seg.MN_ERR_UNPROVEN and st["proof"] == seg.MN_PROOF_SEQUENTIAL_TIES, (n, st)
            assert st["tied_conflicts"] > 0, (n, st)
        else:
            assert st["status"] == 0 and st["proof"] in (seg.MN_PROOF_CERTIFICATE, seg.MN_PROOF_SEQUENTIAL), (n, st)
        assert oracle.masks_equivalent(mask, classes, g["mask"], g["object_class"]), (n, st)
