"""Merger.instance_scores (mn_instance_scores, mn_kernels_prepare.h) against labels.instance_scores, the float64
statement, on every engine that leaves the state the kernel reads -- and the rule for when that state may be read.

The kernel computes nothing from the maps: at every root with a label it takes lpsum[class] - lpsum[0] of the object
(for an object that never merged, lpvalid == 0, logf of the caller's class planes).  So every case below runs a
segmentation, asserts the path it took (stats["mode_used"], and proof / tie_order_used where those select the path),
and compares the scores with the statement evaluated on the mask and the class table THAT CALL RETURNED: the test is
about the scores, the partition is held by other modules.

The bound, per instance
-----------------------
u = 2^-24 (unit roundoff of float32), n = pixels of the instance, A = sum over its pixels of |log p[cls]| + |log p[0]|
(every log p is <= 0, so A is also |sum_cls| + |sum_0|), want = the statement's score.

leaf    one term per pixel and class.  logf is taken to be within 3 units in the last place (the OpenCL accuracy the
        device library is built to; the exact engine's mn_ref_logf restates glibc's, under 1): 3 ulp <= 6 u |log p|,
        summed 6 u A.  With logits the loader's float32 sigmoid 1 / (1 + expf(-x)) comes first: expf within 3 ulp
        (6 u, damped by e^-x / (1 + e^-x) <= 1), one addition, one division: p (1 + d) with |d| <= 8 u; the
        statement's own p is the float64 value rounded once (u): |delta log p| <= 9 u per term, 18 u n for the two
        classes.  The clip is monotone and does not widen a difference.
fixed   the components path (mn_cc_sums / mn_cc_sums_lean / mn_cc_class_sums -> mn_cc_finish): a term is logf of one
        value or of the product (v.x * v.y) * (v.z * v.w) of a lane's four (three roundings: 3 u on the log of four
        pixels, under u per pixel), times MN_LP_FIX = 2^24 (exact) rounded to an integer: half a quantum, 2^-25 = u / 2
        per term, at most one term per pixel.  The integer sums are exact.  1.5 u per pixel and class: 3 u n.
        mn_cc_finish converts the sum to float: u |sum| per class, u A.
float   the float32 paths (mn_kernels_merge.h, mn_kernels_finish.h, the exact engine and the reference-order loop on
        X.lp): a sum of n terms in the order the merges happened, whatever that is: gamma(n - 1) * A with
        gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability, 4.2).  Where such a path starts from components
        or cores (fixed-point sums as leaves, converted once) the conversions and the additions together are still at
        most n - 1 roundings per sum, and the quanta add: `mixed` = float + 3 u n.
last    the kernel's one subtraction: u |want|.
All of it times (1 + 2^-20) for the second-order terms.

    components = leaf + 3 u n + u A + u |want|
    float      = leaf + gamma(n - 1) A + u |want|
    mixed      = float + 3 u n

Nothing in it was fitted to what the device returns.  Every case prints its greatest error as a share of its bound
("SHARE <case> <path> K share ..."; run with -s).  Greatest share per path on gfx950:
    components  speculative 0.19 (bfloat16; float32 0.13-0.16, logits 0.06-0.09), tail and waited 0.13-0.16,
                four calls through fixed buffers with the replay flags 0.21, async (the three images that stay on
                the path) 0.12-0.17
    mixed       fallback inside one call 0.005, rounds from the cores 0.010, async (the image that falls back) 0.005
    float       rounds from single pixels 0.007, exact engine 0.030 (chosen by AUTO: 0.082), Python variant with
                pruning 0.007, reference order among equals 0.007 (both ways), exact batch 0.030
The components bound is about 6e-7 of a score, the float bound grows with the instance (n u).

What overwrites the state (read from mergenet_hip.hip; the flag last_valid is cleared by all of them)
------------------------------------------------------------------------------------------------------
    mn_score_device_t          run_phase_a(components=false): lpvalid and matched zeroed, mn_init_objects writes osize,
                               parent, mate, mn_class_pass writes ocls, then cls0, ball.  label stays: every pixel
                               would be a root and race on scores[label - 1]            -> refuses
    mn_sweep_device_t          launch_sweep: cc_bits, cc_negbits, scalars, partial, cls0; with a form that carries the
                               classes also lpsum (as the int group sums gsum) and, in the full form, ocls and lpvalid
                                                                                         -> refuses (any form)
    mn_sweep_time_device_t     the same launches, `reps` times                           -> refuses
    mn_exact_phase_a_device_t  exact_setup: the exact workspace, cls0, and parent (X.parent = c->parent, set to the
                               identity by mn_x_init_objects)                            -> refuses
    mn_segment_exact_batch_t   exact_setup of every context (parent) long before the hand-over (segment_attempt with
                               xk.prerun) writes label, ocls, lpsum, lpvalid and sets the flag again
                                                                       -> the scores of the batch's image, or refuses
    everything else            (prepare, upsample, RLE, tables, filter, matching, evaluation, map scores, criteria,
                               wires, tiles) writes none of parent, label, ocls, lpvalid, lpsum -> same bits as before
"""
import ctypes

import numpy as np
import pytest
import torch

import golden_util as gu
import lean_util
import lowp_util
from mergenet_amd import labels, segmenter as seg, synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -12345.0
GUARD = 8
OFFS10 = [tuple(int(x) for x in o) for o in synth.generate_offsets(40, 10)]
OFFS6 = [tuple(int(x) for x in o) for o in synth.generate_offsets(12, 6)]
WAITED = 8193        # finish_limit above MN_FIN2_MAXR: the ordinary (waited) components attempt, as test_gpu_topology.py
CMP, RND, XCT, AUTO = seg.MN_MODE_COMPONENTS, seg.MN_MODE_ROUNDS, seg.MN_MODE_EXACT, seg.MN_MODE_AUTO


# ---- the bound -------------------------------------------------------------------------------------------------------

def gamma(k):
    return k * U / (1.0 - k * U)


def bound(path, n, A, want, logits):
    leaf = 6.0 * U * A + (18.0 * U * n if logits else 0.0)
    if path == "components":
        acc = 3.0 * U * n + U * A
    elif path == "float":
        acc = gamma(n - 1) * A
    else:
        assert path == "mixed"
        acc = gamma(n - 1) * A + 3.0 * U * n
    return (leaf + acc + U * abs(want)) * (1.0 + 2.0 ** -20)


def statement(values, mask, table, K, path, logits=False, clip=False):
    """(want float64 [K], bound float64 [K]) on the float32 values the device holds."""
    want = labels.instance_scores(values, mask, table, K, logits=logits, clip=clip)
    p = labels.loaded_class_probs(values, logits, clip).astype(np.float64)
    b = np.zeros(K)
    for k in range(1, K + 1):
        sel = mask == k
        A = float(np.abs(np.log(p[int(table[k - 1])][sel])).sum() + np.abs(np.log(p[0][sel])).sum())
        b[k - 1] = bound(path, int(sel.sum()), A, want[k - 1], logits)
    return want, b


# ---- the call --------------------------------------------------------------------------------------------------------

def raw_scores(m, K, guard=GUARD):
    """(status, float32 [K + guard] as the raw entry point left a sentinel-filled buffer)."""
    dev = torch.device("cuda", m.device)
    buf = torch.full((K + guard,), SENTINEL, dtype=torch.float32, device=dev)
    rc = m.lib.mn_instance_scores_device(m.handle, buf.data_ptr(), seg._stream(dev))
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy()


def check_scores(name, path, m, values, out, logits=False, clip=False):
    """The scores of the segmentation `out` that just finished on `m`, against the statement on out's own mask and
    table; the guard words; the Python call gives the raw call's bits.  Returns the greatest share of the bound."""
    mask, table, _, st = out
    K = st["num_instances"]
    assert st["status"] == 0, (name, st)
    mk, tb = mask.cpu().numpy(), table.cpu().numpy()[:K]
    rc, buf = raw_scores(m, K)
    assert rc == 0, (name, rc)
    assert np.all(buf[K:] == np.float32(SENTINEL)), (name, "wrote behind the K scores", buf[K:])
    assert np.all(buf[:K] != np.float32(SENTINEL)), (name, "left a score unwritten", buf[:K])
    assert np.array_equal(m.instance_scores(K).cpu().numpy().view(np.uint32), buf[:K].view(np.uint32)), name
    want, b = statement(values, mk, tb, K, path, logits, clip)
    err = np.abs(buf[:K].astype(np.float64) - want)
    share = float((err / b).max()) if K else 0.0
    worst = int(np.argmax(err / b)) if K else -1
    print("SHARE %s %s K=%d share %.4f (label %d: got %.9g want %.9g bound %.3g)" %
          (name, path, K, share, worst + 1, buf[worst] if K else 0.0, want[worst] if K else 0.0, b[worst] if K else 0.0))
    assert share <= 1.0, (name, path, share, worst + 1, float(buf[worst]), float(want[worst]), float(b[worst]))
    return share


# ---- inputs ----------------------------------------------------------------------------------------------------------

def label_map(H, W):
    """Background and: two instances that are wide enough for uniform 64-pixel groups where W allows; one single-pixel
    instance; at W >= 128 one instance that is exactly one aligned 64-pixel group of a row."""
    lab = np.zeros((H, W), np.int32)
    lab[1:H // 2, 1:W // 2 - 1] = 1
    lab[H // 3:H - 1, W // 2 + 1:W - 1] = 2
    lab[H - 2, 2] = 3
    if W >= 128:
        assert (W % 64) == 0
        lab[H - 3, 64:128] = 4
    return lab


def class_of_label(C):
    return {0: 0, **{l: (1 + (2 * l) % (C - 1)) if C > 2 else 1 for l in (1, 2, 3, 4)}}


def label_maps(H, W, C, offs=OFFS10, seed=0):
    """lean_util.maps_from_labels of label_map, the class planes scaled per pixel by a factor in [0.7, 1) so that no two
    instances, and no two pixels, share their terms (the arg-max stays: 0.63 against at most 0.0125)."""
    lab = label_map(H, W)
    cp, sp = lean_util.maps_from_labels(lab, class_of_label(C), C, offs)
    rng = np.random.default_rng(1000 * H + W + 7 * C + seed)
    cp = (cp * (0.7 + 0.3 * rng.random(cp.shape, dtype=np.float32))).astype(np.float32)
    return lab, cp, sp


def logits_of(p):
    p = p.astype(np.float64)
    with np.errstate(divide="ignore"):
        return (np.log(p) - np.log1p(-p)).astype(np.float32)


def device_maps(cp, sp, dtype):
    """((class tensor, sameness tensor), the float32 class values the device holds)."""
    if dtype == "float32":
        cp = np.ascontiguousarray(cp, np.float32)
        return (torch.from_numpy(cp).cuda(), torch.from_numpy(np.ascontiguousarray(sp, np.float32)).cuda()), cp
    cb, cw = lowp_util.quantize(cp, dtype)
    sb, _ = lowp_util.quantize(sp, dtype)
    return (lowp_util.to_torch(cb, dtype, "cuda"), lowp_util.to_torch(sb, dtype, "cuda")), cw


def synth_maps(H, W, C, offs, seed, **kw):
    s = synth.synth_v1(H, W, C, offs, seed, **kw)
    return s.class_probs, s.sameness_probs


# ---- B: the scores on every path -----------------------------------------------------------------------------------

# The label-map cases run with the options (0, 1, 0) of test_gpu_topology.py: with a bias the single-pixel instance
# would be merged into the background (the bias is added after the division by the pixel count).
PLAIN = dict(same_different_bias=0.0, object_merge_factor=1.0, merge_logprob_bias=0.0)
SPEC = dict(PLAIN, mode=CMP, require_proof=-1)          # the speculative components attempt
FULL, PX4 = seg.MN_DEBUG_SWEEP_FULL_FORM, seg.MN_DEBUG_SWEEP16_4PX

# name -> (maker of (class maps, sameness maps, offsets), dtype, logits, options, path of the bound, mode expected,
#          pixels per lane of the sweep or None)
CASES = {
    # components, lean form, 4 pixels per lane; the same in the full form
    "lean-32x256":       (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "float32", False, dict(SPEC), "components", CMP, 4),
    "full-32x256":       (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "float32", False, dict(SPEC, debug_flags=FULL), "components", CMP, 4),
    # one pixel per lane (N % 4 != 0); lanes that straddle rows (N % 4 == 0, W % 4 != 0); a last partial group
    "px1-33x67":         (lambda: label_maps(33, 67, 9)[1:] + (OFFS10,), "float32", False, dict(SPEC), "components", CMP, 1),
    "straddle-30x66":    (lambda: label_maps(30, 66, 9)[1:] + (OFFS10,), "float32", False, dict(SPEC), "components", CMP, 4),
    "partial-17x68":     (lambda: label_maps(17, 68, 9)[1:] + (OFFS10,), "float32", False, dict(SPEC), "components", CMP, 4),
    # class counts: 2; 17, the second round of the class loop; 81 at the shape of cseg_synth_48x80_c81
    "c2-32x256":         (lambda: label_maps(32, 256, 2)[1:] + (OFFS10,), "float32", False, dict(SPEC), "components", CMP, 4),
    "c17-32x256":        (lambda: label_maps(32, 256, 17)[1:] + (OFFS10,), "float32", False, dict(SPEC), "components", CMP, 4),
    "c81-48x80":         (lambda: label_maps(48, 80, 81)[1:] + (OFFS10,), "float32", False, dict(SPEC), "components", CMP, 4),
    # element types and forms
    "bf16-32x256":       (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "bfloat16", False, dict(SPEC), "components", CMP, 8),
    "f16-4px-32x256":    (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "float16", False, dict(SPEC, debug_flags=PX4), "components", CMP, 4),
    "logits-f32-32x256": (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "float32", True, dict(SPEC), "components", CMP, 4),
    "logits-bf16-32x256": (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "bfloat16", True, dict(SPEC), "components", CMP, 8),
    "clip0-32x256":      (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "float32", False, dict(SPEC, clip_inputs=0), "components", CMP, 4),
    "clip1-32x256":      (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "float32", False, dict(SPEC, clip_inputs=1), "components", CMP, 4),
    # the suite's two attempts (test_gpu_topology.ATTEMPTS) under the default require_proof.  With an explicit
    # mode = COMPONENTS, require_proof 0 asks for no more proof than -1: "tail" is the speculative fused attempt of
    # "lean-32x256" again (mn_cc_tail and its certificate), under the options the suite's tables use; the "waited"
    # cases are the ones that leave it, for the ordinary attempt (mn_cc_certificate, mn_verify_records).
    "tail-32x256":       (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "float32", False, dict(PLAIN, mode=CMP), "components", CMP, 4),
    "waited-32x256":     (lambda: label_maps(32, 256, 9)[1:] + (OFFS10,), "float32", False, dict(PLAIN, mode=CMP, finish_limit=WAITED), "components", CMP, 4),
    "waited-33x67":      (lambda: label_maps(33, 67, 9)[1:] + (OFFS10,), "float32", False, dict(PLAIN, mode=CMP, finish_limit=WAITED), "components", CMP, 1),
    # a map that leaves the speculative attempt inside one call (the 0.45 image of
    # test_segment_async_two_contexts_one_stream_equals_segment): redone on the ordinary path, which ends in the rounds
    "fallback-96x160":   (lambda: synth_maps(96, 160, 4, OFFS6, 701, noise=0.45) + (OFFS6,), "float32", False, dict(mode=CMP, clip_inputs=1), "mixed", RND, None),
    # the rounds, from the cores and from single pixels
    "rounds-n15":        (lambda: synth_maps(96, 160, 4, OFFS6, 700, noise=0.15) + (OFFS6,), "float32", False, dict(mode=RND, clip_inputs=1), "mixed", RND, None),
    "rounds-n45":        (lambda: synth_maps(96, 160, 4, OFFS6, 701, noise=0.45) + (OFFS6,), "float32", False, dict(mode=RND, clip_inputs=1), "mixed", RND, None),
    "rounds-n15-nocores": (lambda: synth_maps(96, 160, 4, OFFS6, 700, noise=0.15) + (OFFS6,), "float32", False, dict(mode=RND, clip_inputs=1, debug_flags=seg.MN_DEBUG_NO_CORES), "float", RND, None),
    "rounds-n45-nocores": (lambda: synth_maps(96, 160, 4, OFFS6, 701, noise=0.45) + (OFFS6,), "float32", False, dict(mode=RND, clip_inputs=1, debug_flags=seg.MN_DEBUG_NO_CORES), "float", RND, None),
    # the exact engine: asked for; chosen by AUTO itself (24 x 40 x 6 records <= 32768)
    "exact-64x128":      (lambda: synth_maps(64, 128, 9, OFFS10, 1001, num_instances=4) + (OFFS10,), "float32", False, dict(mode=XCT, clip_inputs=1), "float", XCT, None),
    "auto-24x40":        (lambda: synth_maps(24, 40, 4, OFFS6, 77, noise=0.45, num_instances=3) + (OFFS6,), "float32", False, dict(mode=AUTO, clip_inputs=1), "float", XCT, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_scores_meet_the_statement(name):
    """One segmentation per case on a fresh Merger, the path asserted, the scores against the statement within the
    bound of that path (module docstring), the guard words, and -- in a call of its own -- the form of the sweep."""
    make, dtype, logits, okw, path, mode, px = CASES[name]
    cp, sp, offs = make()
    C, H, W = cp.shape
    if logits:
        cp, sp = logits_of(cp), logits_of(sp)
    d, values = device_maps(cp, sp, dtype)
    opts = seg.default_options(**okw)
    m = seg.Merger(H, W, C, len(offs))
    try:
        out = m.segment(d[0], d[1], offs, opts, logits=logits)
        st = out[3]
        assert st["mode_used"] == mode, (name, st)
        if mode == CMP:
            assert st["num_instances"] == (4 if W >= 128 else 3), (name, st["num_instances"], st)
        assert st["num_instances"] > 0
        clip = bool(okw.get("clip_inputs", 0)) or dtype != "float32"
        check_scores(name, path, m, values, out, logits=logits, clip=clip)
    finally:
        m.close()
    if px is not None:
        # the form of the sweep this shape and element type take (a call of its own: it overwrites the state)
        m = seg.Merger(H, W, C, len(offs))
        try:
            so = seg.default_options(debug_flags=okw.get("debug_flags", 0), clip_inputs=okw.get("clip_inputs", 0))
            sw = m.sweep(d[0], d[1], offs, so, logits=logits)
            assert sw["pixels_per_lane"] == px, (name, sw["pixels_per_lane"])
            if name in ("lean-32x256", "full-32x256"):
                assert labels.uniform_groups(sw["bits"].cpu().numpy().view(np.uint32), offs).any()
        finally:
            m.close()


def test_python_variant_with_pruning():
    """MN_VARIANT_PYSEGMENTER on a py_* vector with the prune step (the vector keeps three of the four instances its
    unpruned twin py_synth_64x128_n15_raw has): pruned objects are background and get no score."""
    g = gu.load("py_synth_64x128_n15_prune")
    H, W, C = g["spec"]["H"], g["spec"]["W"], g["spec"]["C"]
    sdb, omf, bias = g["spec"]["opts"]
    o = seg.default_options(same_different_bias=sdb, object_merge_factor=omf, merge_logprob_bias=bias, clip_inputs=1,
                            variant=seg.MN_VARIANT_PYSEGMENTER, mode=XCT, prune_threshold=200.0)
    d, values = device_maps(g["class_probs"], g["sameness_probs"], "float32")
    m = seg.Merger(H, W, C, len(g["offsets"]))
    try:
        out = m.segment(d[0], d[1], g["offsets"], o)
        assert out[3]["mode_used"] == XCT and out[3]["num_instances"] == len(g["object_class"]) == 3, out[3]
        check_scores("py-prune-64x128", "float", m, values, out, clip=True)
    finally:
        m.close()


TIE_DECIDED = [n for n in gu.names("cseg_blur4_") if "128x256" in n][0]


@pytest.mark.parametrize("how", ["default", "reference"])
def test_reference_order_among_equals(how):
    """A vector whose instance borders the order among bit-equal priorities decides.  Default options: the exact engine
    runs, meets tied pops, and the image is redone by the reference-order loop; tie_order = MN_TIES_REFERENCE: that
    loop alone.  Either way exact_export hands the exact engine's X over, and the scores must be those of the
    partition the REDO ended in."""
    g = gu.load(TIE_DECIDED)
    H, W, C = g["spec"]["H"], g["spec"]["W"], g["spec"]["C"]
    sdb, omf, bias = g["spec"]["opts"]
    kw = dict(tie_order=seg.MN_TIES_REFERENCE) if how == "reference" else {}
    o = seg.default_options(same_different_bias=sdb, object_merge_factor=omf, merge_logprob_bias=bias, clip_inputs=1,
                            mode=XCT, **kw)
    d, values = device_maps(g["class_probs"], g["sameness_probs"], "float32")
    m = seg.Merger(H, W, C, len(g["offsets"]))
    try:
        out = m.segment(d[0], d[1], g["offsets"], o)
        st = out[3]
        assert st["mode_used"] == XCT and st["tie_order_used"] == seg.MN_TIES_REFERENCE, st
        assert st["proof"] == seg.MN_PROOF_SEQUENTIAL, st
        if how == "default":
            assert st["tied_steps"] > 0, st
        check_scores("ties-%s" % how, "float", m, values, out, clip=True)
    finally:
        m.close()


def test_exact_batch_of_two_images():
    """mn_segment_exact_batch: each context answers for ITS image of the batch (or refuses) -- never for the image it
    segmented before, and never for its neighbour's."""
    H, W, C = 64, 128, 9
    images = [device_maps(*synth_maps(H, W, C, OFFS10, seed, num_instances=4), "float32") for seed in (1001, 1003, 1005)]
    o = seg.default_options(clip_inputs=1)
    batch = seg.ExactBatch(H, W, C, len(OFFS10), 2)
    try:
        # the first context segments another image first
        (d0, v0) = images[2]
        before = batch.mergers[0].segment(d0[0], d0[1], OFFS10, seg.default_options(mode=XCT, clip_inputs=1))
        check_scores("batch-before", "float", batch.mergers[0], v0, before, clip=True)
        outs = batch.segment([images[0][0][0], images[1][0][0]], [images[0][0][1], images[1][0][1]], OFFS10, o)
        for i, out in enumerate(outs):
            assert out[3]["mode_used"] == XCT and out[3]["num_instances"] > 0, out[3]
            rc, _ = raw_scores(batch.mergers[i], out[3]["num_instances"])
            assert rc in (0, seg.MN_ERR_ARGUMENT)
            if rc == 0:
                check_scores("batch-%d" % i, "float", batch.mergers[i], images[i][1], out, clip=True)
            print("BATCH context %d: %s" % (i, "scores of its image" if rc == 0 else "refuses"))
    finally:
        batch.close()


def test_async_two_mergers_alternating():
    """Two Mergers alternating on one stream, the launch of image i + 1 ahead of the read-back of image i (as
    test_segment_async_two_contexts_one_stream_equals_segment): the scores taken after each .result() are that image's.
    The three noise-0.15 images stay on the speculative components path and are held to its bound; the 0.45 image is
    redone by the rounds inside .result() (the mixed bound).  Between launch and result a Merger refuses."""
    H, W, C = 96, 160, 4
    cases = [device_maps(*synth_maps(H, W, C, OFFS6, seed, noise=noise), "float32")
             for seed, noise in [(700, 0.15), (701, 0.45), (702, 0.15), (703, 0.15)]]
    ended = [(CMP, "components"), (RND, "mixed"), (CMP, "components"), (CMP, "components")]

    def finish(pm, pvalues, pend, j):
        out = pend.result()
        assert out[3]["mode_used"] == ended[j][0], (j, out[3])
        check_scores("async-%d" % j, ended[j][1], pm, pvalues, out, clip=True)

    opts = seg.default_options(mode=CMP, clip_inputs=1)
    a, b = seg.Merger(H, W, C, len(OFFS6)), seg.Merger(H, W, C, len(OFFS6))
    try:
        prev = None
        for i, (d, values) in enumerate(cases):
            m = (a, b)[i % 2]
            cur = m.segment_async(d[0], d[1], OFFS6, opts)
            if i == 0:
                rc, buf = raw_scores(m, 0)
                assert rc == seg.MN_ERR_ARGUMENT and np.all(buf == np.float32(SENTINEL))     # busy: launches nothing
            if prev is not None:
                finish(*prev)
            prev = (m, values, cur, i)
        finish(*prev)
    finally:
        a.close(); b.close()


def test_replay_with_the_inputs_rewritten_in_place():
    """MN_DEBUG_REPLAY | MN_DEBUG_LEAN_EVENTS through fixed buffers (first, clean, recording, replaying call), a
    DIFFERENT image at the same addresses each time -- which the replay key allows.  The replay branch sets
    last_params itself; the scores after each call are those of that call's image.  mn_stats has no field that says
    a call was replayed: the four calls meet every condition of the branch (same key, cc_clean), but if one of them
    failed silently they would pass on the ordinary fused path, and "replay-3" would be a fourth speculative call."""
    H, W, C = 32, 256, 9
    imgs = [synth_maps(H, W, C, OFFS10, seed, num_instances=4) for seed in (1011, 1012, 1013, 1014)]
    flags = seg.MN_DEBUG_REPLAY | seg.MN_DEBUG_LEAN_EVENTS
    o = seg.default_options(mode=CMP, require_proof=-1, clip_inputs=1, debug_flags=flags)
    buf = (torch.empty((C, H, W), dtype=torch.float32, device="cuda"),
           torch.empty((len(OFFS10), H, W), dtype=torch.float32, device="cuda"))
    out_buf = (torch.empty((H, W), dtype=torch.int32, device="cuda"), torch.empty((H * W,), dtype=torch.int32, device="cuda"))
    m = seg.Merger(H, W, C, len(OFFS10))
    try:
        for i, (cp, sp) in enumerate(imgs):
            buf[0].copy_(torch.from_numpy(cp)); buf[1].copy_(torch.from_numpy(sp))
            out = m.segment_async(buf[0], buf[1], OFFS10, o, out=out_buf).result()
            assert out[3]["mode_used"] == CMP and out[3]["num_instances"] > 0, (i, out[3])
            check_scores("replay-%d" % i, "components", m, cp, out, clip=True)
    finally:
        m.close()


def test_no_instances_writes_nothing():
    """K = 0: an all-background image.  The Python call returns an empty tensor; the raw entry point leaves a
    sentinel-filled buffer of 8 floats as it was."""
    H, W, C = 32, 256, 9
    cp, sp = lean_util.maps_from_labels(np.zeros((H, W), np.int32), {0: 0}, C, OFFS10)
    d, _ = device_maps(cp, sp, "float32")
    m = seg.Merger(H, W, C, len(OFFS10))
    try:
        out = m.segment(d[0], d[1], OFFS10, seg.default_options(**SPEC))
        assert out[3]["num_instances"] == 0 and out[3]["mode_used"] == CMP, out[3]
        assert m.instance_scores(0).shape == (0,)
        rc, buf = raw_scores(m, 0, guard=8)
        assert rc == 0 and buf.shape == (8,) and np.all(buf == np.float32(SENTINEL))
    finally:
        m.close()


# ---- C: when the state may be read -----------------------------------------------------------------------------------

class Scene:
    """One 32x256 image on a Merger, its segmentation and its scores s0."""

    def __init__(self):
        self.H, self.W, self.C = 32, 256, 9
        self.lab, cp, sp = label_maps(self.H, self.W, self.C)
        self.d, self.values = device_maps(cp, sp, "float32")
        self.x = (torch.from_numpy(logits_of(cp)).cuda(), torch.from_numpy(logits_of(np.minimum(sp, 0.999))).cuda())
        self.m = seg.Merger(self.H, self.W, self.C, len(OFFS10))
        self.opts = seg.default_options(**SPEC)
        self.out = self.m.segment(self.d[0], self.d[1], OFFS10, self.opts)
        self.K = self.out[3]["num_instances"]
        assert self.K == 4 and self.out[3]["mode_used"] == CMP
        rc, buf = raw_scores(self.m, self.K)
        assert rc == 0
        self.s0 = buf[:self.K].copy()
        want, b = statement(self.values, self.out[0].cpu().numpy(), self.out[1].cpu().numpy()[:self.K], self.K, "components")
        assert np.all(np.abs(self.s0.astype(np.float64) - want) <= b)

    def same_bits(self):
        rc, buf = raw_scores(self.m, self.K)
        return rc == 0 and np.array_equal(buf[:self.K].view(np.uint32), self.s0.view(np.uint32)) and \
            bool(np.all(buf[self.K:] == np.float32(SENTINEL)))

    def refuses(self):
        rc, buf = raw_scores(self.m, self.K)
        with pytest.raises(seg.MergeNetError) as e:
            self.m.instance_scores(self.K)
        return rc == seg.MN_ERR_ARGUMENT and e.value.status == seg.MN_ERR_ARGUMENT and \
            bool(np.all(buf == np.float32(SENTINEL)))

    def close(self):
        self.m.close()


@pytest.fixture
def scene():
    s = Scene()
    yield s
    s.close()


def _recipe(s):
    m, (mask, table, _, st), K = s.m, s.out, s.K
    full = m.upsample_mask(mask, s.H - 3, s.W - 5)          # (encode_rle holds the mask to the Merger's capacity)
    m.encode_rle(full, K, drop_zero_area=True)
    scores = m.instance_scores(K)
    tab = m.instance_table(full, K)
    m.filter_instances(full, table, K, min_area=50, scores=scores, table=tab)
    m.coco_results(full, table, K, 7, list(range(100, 100 + s.C)), scores=scores)


def _truth(s):
    truth = torch.from_numpy(s.lab).cuda()
    classes = torch.tensor([class_of_label(s.C)[l] for l in (1, 2, 3, 4)], dtype=torch.int32, device="cuda")
    return truth, classes


def _ground_truth(s):
    m, (mask, table, _, st), K = s.m, s.out, s.K
    truth, classes = _truth(s)
    m.sameness_targets(truth, OFFS10)
    t = m.overlap_table(mask, truth, K, 4)
    m.match_instances(t, table, classes, scores=m.instance_scores(K))


def _criteria(s):
    m = s.m
    truth, classes = _truth(s)
    m.map_scores(s.d[0], s.d[1], OFFS10, truth, classes)
    m.mask_bce(s.x[0], s.x[1], OFFS10, truth, classes)
    for part, x in (("class", s.x[0]), ("offset", s.x[1])):
        sums = m.plane_sums(x, part, OFFS10, truth, classes, terms=True)
        co = m.plane_coeffs("mbce", sums, pixels=float(s.H * s.W))
        m.plane_grad(x, part, OFFS10, truth, classes, co["coeffs"])
        m.mask_ce(x, part, OFFS10, truth, classes)


def _producers(s):
    m, (mask, table, _, st), K = s.m, s.out, s.K
    rles = m.encode_rle(mask, K)
    m.decode_rle(rles, s.H, s.W)
    cap = 2048
    wire = torch.zeros(seg.runs_wire_words(cap, 64), dtype=torch.int32, device="cuda")
    seg.pack_runs(m, mask, table, K, wire, cap, 64, -1.5)
    m.prepare(s.x[0], s.H // 2, s.W // 2, apply_sigmoid=True, clip=True)
    tiles = s.x[0][None].contiguous()
    m.tile_class_maps(tiles, None, [0], [0], s.H, s.W, s.C)


@pytest.mark.parametrize("calls", [_recipe, _ground_truth, _criteria, _producers], ids=lambda f: f.__name__.strip("_"))
def test_the_documented_calls_leave_the_scores_available(scene, calls):
    """INTEGRATION.md's recipe calls upsample_mask and encode_rle between segment and instance_scores; every other
    call that takes the Merger may come in between as well.  None of them writes an array the score kernel reads: the
    scores afterwards are bit-equal to those taken right after segment."""
    calls(scene)
    torch.cuda.synchronize()
    assert scene.same_bits()


def test_score_makes_the_scores_stale(scene):
    """segment, score, instance_scores.  mn_score_device re-initialises parent, ocls and lpvalid and leaves label: on
    the parent commit every pixel was a root racing on scores[label - 1], status 0."""
    scene.m.score(scene.d[0], scene.d[1], OFFS10, scene.opts)
    rc, buf = raw_scores(scene.m, scene.K)
    print("AFTER score: status %d, scores %s (s0 %s)" % (rc, buf[:scene.K], scene.s0))
    assert scene.refuses()
    # ... and the next segmentation makes them available again
    out = scene.m.segment(scene.d[0], scene.d[1], OFFS10, scene.opts)
    assert out[3]["num_instances"] == scene.K and scene.same_bits()


@pytest.mark.parametrize("which", ["sweep", "sweep_time", "exact_phase_a"])
def test_the_diagnostic_entries_make_the_scores_stale(scene, which):
    """By the table in the module's docstring each of them overwrites an array the score kernel reads (the sweep
    depending on its form: refused in every form).  Never silently different."""
    m = scene.m
    if which == "sweep":
        m.sweep(scene.d[0], scene.d[1], OFFS10, seg.default_options())
    elif which == "sweep_time":
        m.sweep_time([scene.d], OFFS10, seg.default_options(), reps=2)
    else:
        m.exact_phase_a(scene.d[0], scene.d[1], OFFS10, seg.default_options())
    rc, buf = raw_scores(m, scene.K)
    print("AFTER %s: status %d, scores %s (s0 %s)" % (which, rc, buf[:scene.K], scene.s0))
    assert scene.refuses() or scene.same_bits()
    assert scene.refuses()          # (what the table says for all three)


def test_a_call_refused_for_its_arguments_leaves_the_scores(scene):
    """begin_call rejects a wrong channel count (class_dim below num_classes cannot be said through Merger.segment:
    the raw entry point) and an offset list with an offset and its negation before anything runs."""
    m = scene.m
    with pytest.raises(seg.MergeNetError):
        m.segment(scene.d[0], scene.d[1], [(0, 1), (0, -1)] + OFFS10[2:], scene.opts)
    assert scene.same_bits()
    mask = torch.empty((scene.H, scene.W), dtype=torch.int32, device="cuda")
    table = torch.empty((scene.H * scene.W,), dtype=torch.int32, device="cuda")
    off = np.ascontiguousarray(np.asarray(OFFS10, np.int32))
    stats = seg.MnStats()
    fn, dt = m._typed("mn_segment_device", seg.MN_DTYPE_F32)
    rc = fn(m.handle, scene.d[0].data_ptr(), scene.C - 1, scene.d[1].data_ptr(), len(OFFS10), *dt, scene.W, scene.H,
            scene.C, off.ctypes.data_as(seg._i32p), mask.data_ptr(), table.data_ptr(), None,
            ctypes.byref(scene.opts), seg._stream(mask.device), ctypes.byref(stats))
    assert rc == seg.MN_ERR_ARGUMENT
    assert scene.same_bits()


def test_a_fresh_context_refuses():
    m = seg.Merger(32, 256, 9, len(OFFS10))
    try:
        rc, buf = raw_scores(m, 4)
        assert rc == seg.MN_ERR_ARGUMENT and np.all(buf == np.float32(SENTINEL))
        with pytest.raises(seg.MergeNetError):
            m.instance_scores(4)
    finally:
        m.close()
