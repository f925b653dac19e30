"""tests/tools/exact_model.cpp -- the CPU model of the exact engine's semantics (the reference's lazy greedy with ties
going to the lowest record id) and of its tie-conflict criterion -- against vectors taken from the reference
(utils/csegment/segment.cc:539-727).  CPU only.  The GPU suite then compares the engine with this model
(tests/test_gpu_exact.py::test_tie_conflict_verdict_equals_the_cpu_models)."""
import os
import sys

import numpy as np
import pytest

import golden_util as gu
from mergenet_amd import labels

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import exact_model  # noqa: E402


def _run(name):
    g = gu.load(name)
    sdb, omf, bias = g["spec"]["opts"]
    assert sdb == 0.0
    part, ocls, st = exact_model.run(g["class_probs"], g["sameness_probs"], g["offsets"], omf, bias)
    # the reference's mask: label 0 for class-0 objects, one label per other object (segment.cc:491-517)
    mask = np.where(ocls == 0, 0, part + 1).astype(np.int64)
    _, inv = np.unique(mask, return_inverse=True)
    mask = inv.reshape(mask.shape)
    if (ocls == 0).sum() == 0:
        mask = mask + 1
    classes = [int(ocls.reshape(-1)[np.argmax(mask.reshape(-1) == k)]) for k in range(1, int(mask.max()) + 1)]
    return g, mask, classes, st


@pytest.mark.parametrize("name", ["cseg_adv_32x32_o0", "cseg_adv_48x48_o0", "cseg_adv_48x48_o1", "cseg_adv_64x64_o1",
                                  "cseg_blur_64x128_r2_s8001"])
def test_no_tie_conflict_means_the_references_partition(name):
    """Vectors with no tied pop, or with tied pops that the criterion calls harmless (cseg_blur_64x128_r2_s8001 has
    86): the model -- whose order among equals is NOT the reference's -- must reproduce the reference's result."""
    g, mask, classes, st = _run(name)
    assert st["tied_conflicts"] == 0, st
    assert labels.masks_equivalent(mask, classes, g["mask"], g["object_class"]), st


def test_a_tie_decided_vector_is_reported_as_conflicting():
    """cseg_blur4_128x256_s5100: the lowest-id rule ends elsewhere than the reference (115 199 pops against the
    oracle's 115 297) -- and the criterion must have said so."""
    g, mask, classes, st = _run("cseg_blur4_128x256_s5100")
    assert st["steps"] == 115199 and st["tied_steps"] > 0 and st["tied_conflicts"] > 0, st
    assert not labels.masks_equivalent(mask, classes, g["mask"], g["object_class"])


# ---- fresh tied inputs: the verdict table that tests/test_gpu_proof.py holds the engine's proof claim to ----------
# synth.blurred_v1(H, W, 9, generate_offsets(40, 10), seed, radius=2, noise=0.05) with options (0.0, 1.0, 0.03): every
# one of these maps has tied pops (86-123 of ~26 k at 64x128, ~400 of ~52 k at 96x160, ~2 000 of ~117 k at 128x256).
# The table is what the model said when it was written; the test below and the GPU module assert it per input, so
# that neither can go vacuous if the generator or the model drifts.
FRESH_OPTS = (0.0, 1.0, 0.03)
EXPECTED_NO_CONFLICT = {(64, 128): (8102, 8103, 8106, 8107, 8111, 8112, 8113, 8114, 8115),
                        (96, 160): (8504, 8507),
                        (128, 256): (8701,)}
EXPECTED_CONFLICT = {(64, 128): (8100, 8101, 8104, 8105, 8108, 8109, 8110),
                     (96, 160): (8500,),
                     (128, 256): (8700,)}
# the lowest-id rule ends in a partition that is NOT the reference's on this one (on the other conflict seeds the two
# rules happen to end in the same partition)
WITNESS_SEED = 8100
FRESH_TIED = sorted((H, W, seed) for table in (EXPECTED_NO_CONFLICT, EXPECTED_CONFLICT)
                    for (H, W), seeds in table.items() for seed in seeds)


def fresh_tied_input(H, W, seed):
    from mergenet_amd import synth
    offs = synth.generate_offsets(40, 10)
    return synth.blurred_v1(H, W, 9, offs, seed, radius=2, noise=0.05), offs


def expected_conflict(H, W, seed):
    assert (seed in EXPECTED_CONFLICT[(H, W)]) != (seed in EXPECTED_NO_CONFLICT[(H, W)])
    return seed in EXPECTED_CONFLICT[(H, W)]


@pytest.mark.parametrize("H,W,seed", FRESH_TIED)
def test_verdict_table_of_the_fresh_tied_inputs(oracle, H, W, seed):
    """The model's yes / no on every fresh input equals the pinned table; no conflict => the model's partition (lowest
    record id among equals) is the partition of the oracle's run of the reference's loop (its heap's order among
    equals); and on seed 8100 -- a conflict -- it is not: there the verdict is not idle caution."""
    s, offs = fresh_tied_input(H, W, seed)
    sdb, omf, bias = FRESH_OPTS
    ref = oracle.run_csegment(s.class_probs, s.sameness_probs, 9, offs, sdb, omf, bias)
    part, ocls, st = exact_model.run(s.class_probs, s.sameness_probs, offs, omf, bias)
    assert st["tied_steps"] > 0, st
    assert (st["tied_conflicts"] > 0) == expected_conflict(H, W, seed), st
    if st["tied_conflicts"] == 0:
        assert oracle.same_partition(part, ref.partition), st
        assert st["merges"] == ref.stats["n_merges"]
    if seed == WITNESS_SEED:
        assert st["tied_conflicts"] > 0 and not oracle.same_partition(part, ref.partition), st


@pytest.mark.parametrize("window", [3, 16, 64])
@pytest.mark.parametrize("name", ["cseg_adv_32x32_o0", "cseg_adv_48x48_o1", "cseg_synth_32x64_n60", "cseg_blur_64x128_r2",
                                  "cseg_checker_96x128_b015"])
def test_prefix_executor_reproduces_the_sequential_order(name, window, monkeypatch):
    """The side-by-side executor sketched in DESIGN.md section 9 (XM_EXECUTOR=K in the model): per round the K best
    queue entries are planned from the state at the START of the round, and the longest prefix is committed in which
    no committed pop produced a queue key ahead of the next entry and no pop writes an object that an earlier one
    read or wrote (or reads one it wrote).  Claim: the state after every round is the sequential one -- same
    partition, same classes, same number of pops and merges as the sequential model."""
    g = gu.load(name)
    sdb, omf, bias = g["spec"]["opts"]
    monkeypatch.delenv("XM_EXECUTOR", raising=False)
    p0, c0, s0 = exact_model.run(g["class_probs"], g["sameness_probs"], g["offsets"], omf, bias, track=False)
    monkeypatch.setenv("XM_EXECUTOR", str(window))
    p1, c1, s1 = exact_model.run(g["class_probs"], g["sameness_probs"], g["offsets"], omf, bias, track=False)
    assert np.array_equal(p0, p1) and np.array_equal(c0, c1)
    assert (s0["steps"], s0["merges"]) == (s1["steps"], s1["merges"])


@pytest.mark.parametrize("name", ["cseg_adv_48x48_o0", "cseg_synth_32x64_n60", "cseg_blur_64x128_r2"])
def test_sorted_front_hands_out_the_queues_best_entries(name, monkeypatch):
    """The queue the executor would use on the GPU (XM_FRONT=M): a sorted front of the M best entries with the invariant
    "every entry outside is behind the front's last", rebuilt when fewer than K are left.  Every round's window must
    be the K best entries of the whole queue (checked inside the model), and the result the sequential one."""
    g = gu.load(name)
    sdb, omf, bias = g["spec"]["opts"]
    monkeypatch.delenv("XM_EXECUTOR", raising=False)
    monkeypatch.delenv("XM_FRONT", raising=False)
    p0, c0, s0 = exact_model.run(g["class_probs"], g["sameness_probs"], g["offsets"], omf, bias, track=False)
    monkeypatch.setenv("XM_EXECUTOR", "16")
    monkeypatch.setenv("XM_FRONT", "48")
    p1, c1, s1 = exact_model.run(g["class_probs"], g["sameness_probs"], g["offsets"], omf, bias, track=False)
    assert s1["front_errors"] == 0 and s1["front_rebuilds"] > 0
    assert np.array_equal(p0, p1) and (s0["steps"], s0["merges"]) == (s1["steps"], s1["merges"])
