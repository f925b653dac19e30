"""A call gives the same answer whatever ran before it on the context.

The context carries state from one call to the next: cc_clean (a fused attempt skips its fills when the image before
queued its own clean-up), the replay key and its recorded graphs, ms_partials (shared by map_scores, mask_bce,
plane_sums and mask_ce), block_count and scalars (the output stage and mn_rle_points_device), wire_counts,
match_work, the record lists (regrown by ensure_general), the exact workspace, debug_flags / ext_events /
core_radius.  test_gpu_memory.py walks one context through the allocating paths for byte counts; here every entry of
a list of PROBES is held to: its bytes on a Merger that just ran something else are its bytes on a fresh Merger.

A probe is a function of (Merger, inputs) that returns everything its call hands back, as bytes per item: tensors,
and the stats without their ms_* timing fields.

    determinism   each probe on two fresh Mergers: equal bytes.  (All probes are deterministic to the bit; none needed
                  the looser equivalence of its own test.)
    ordered pairs for every (A, B): B after A equals B fresh -- at 32x256 (C = 9, ten offsets: four pixels per lane,
                  the lean form, replay possible: 18 probes) and at the ragged 30x66 (W % 4 != 0: all 19).  The
                  probe that asks for the exact engine runs at 30x66 only (EXACT_ENGINE below says why).
    steady state  B five times on one Merger: every call equals B fresh.  The fused path's first, clean, recording and
                  replaying calls are four different code paths.
    other shape   a Merger created for 32x256 runs A at 30x66 with four offsets and C = 3 (another offset table,
                  another record capacity, another form of the sweep), then B at 32x256, for B among the segment probes
                  (without the exact engine's) and map_scores.
    error         speculative segment, a call refused for its arguments, speculative segment.

Every segment probe asserts the engine it ended on (MODE_OF): "auto-fallback" is the one sequence in which a
speculative fused attempt is redone inside one call -- by the rounds, after ensure_general has regrown the record lists
and dropped cc_clean and the replay graphs.

What the module cannot see: mn_stats has no field that says a call was REPLAYED.  "spec-replay" meets every condition
of the replay branch (same key, fixed buffers, cc_clean) from its third run on, and its runs of the steady-state test
are meant to be the first, clean, recording and replaying calls; should the key or the cc_clean condition fail
silently, the same calls would pass on the ordinary fused path.

One Merger per sequence, closed at the end; everything on the current stream; no threads, nothing timed.
"""
import functools

import numpy as np
import pytest
import torch

import lowp_util
from mergenet_amd import segmenter as seg, synth

pytestmark = pytest.mark.gpu

CMP, RND, XCT, AUTO = seg.MN_MODE_COMPONENTS, seg.MN_MODE_ROUNDS, seg.MN_MODE_EXACT, seg.MN_MODE_AUTO
WAITED = 8193          # finish_limit above MN_FIN2_MAXR: the ordinary components attempt (test_gpu_topology.ATTEMPTS)
LEAN, REPLAY = seg.MN_DEBUG_LEAN_EVENTS, seg.MN_DEBUG_REPLAY
OFFS10 = [tuple(int(x) for x in o) for o in synth.generate_offsets(40, 10)]
OFFS4 = [tuple(int(x) for x in o) for o in synth.generate_offsets(8, 4)]
SHAPES = {"32x256": (32, 256, 9, OFFS10), "30x66": (30, 66, 9, OFFS10), "small": (30, 66, 3, OFFS4)}


class Inputs:
    """The tensors of one shape, made once and left alone: the probes of every sequence read the same addresses
    (which is what lets the replay probe replay)."""

    def __init__(self, name):
        self.name = name
        self.H, self.W, self.C, self.offs = SHAPES[name]
        H, W, C, offs = self.H, self.W, self.C, self.offs
        s = synth.synth_v1(H, W, C, offs, 1011, num_instances=4)
        noisy = synth.synth_v1(H, W, C, offs, 701, noise=0.45, num_instances=4)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.probs = (dev(s.class_probs), dev(s.sameness_probs))
        self.noisy = (dev(noisy.class_probs), dev(noisy.sameness_probs))
        self.bf16 = tuple(lowp_util.to_torch(lowp_util.quantize(a, "bfloat16")[0], "bfloat16", "cuda")
                          for a in (s.class_probs, s.sameness_probs))
        logit = lambda p: np.log(p.astype(np.float64) / (1.0 - np.minimum(p, 0.999).astype(np.float64))).astype(np.float32)
        self.logits = (dev(logit(s.class_probs)), dev(logit(s.sameness_probs)))
        self.truth = dev(s.instances.astype(np.int32))
        self.truth_classes = torch.tensor(s.instance_class[1:], dtype=torch.int32, device="cuda")
        other = synth.synth_v1(H, W, C, offs, 1012, num_instances=4)
        self.pred = dev(other.instances.astype(np.int32))
        self.pred_classes = torch.tensor(other.instance_class[1:], dtype=torch.int32, device="cuda")
        self.pred_table = torch.full((H * W,), -1, dtype=torch.int32, device="cuda")
        self.pred_table[:4] = self.pred_classes
        self.out = (torch.empty((H, W), dtype=torch.int32, device="cuda"),
                    torch.empty((H * W,), dtype=torch.int32, device="cuda"))

    def merger(self, like=None):
        e = like or self
        return seg.Merger(e.H, e.W, e.C, len(e.offs))


@functools.lru_cache(maxsize=None)
def inputs(name):
    return Inputs(name)


# ---- probes ----------------------------------------------------------------------------------------------------------

def _b(t):
    return b"" if t is None else t.detach().cpu().contiguous().numpy().tobytes()


def _stats(st):
    return repr(sorted((k, v) for k, v in st.items() if not k.startswith("ms_"))).encode()


def _segment(m, e, maps, logits=False, replay=False, **okw):
    o = seg.default_options(**okw)
    if replay:
        e.out[0].fill_(-7)
        e.out[1].fill_(-7)
        mask, table, part, st = m.segment_async(maps[0], maps[1], e.offs, o, out=e.out, logits=logits).result()
    else:
        mask, table, part, st = m.segment(maps[0], maps[1], e.offs, o, want_partition=True, logits=logits)
    torch.cuda.synchronize()
    return {"mask": _b(mask), "table": _b(table), "part": _b(part), "stats": _stats(st)}


SPEC = dict(mode=CMP, require_proof=-1, clip_inputs=1)


def p_spec(m, e):
    return _segment(m, e, e.probs, **SPEC)


def p_spec_lean_events(m, e):
    return _segment(m, e, e.probs, debug_flags=LEAN, **SPEC)


def p_spec_replay(m, e):
    return _segment(m, e, e.probs, replay=True, debug_flags=LEAN | REPLAY, **SPEC)


def p_ordinary(m, e):
    return _segment(m, e, e.probs, mode=CMP, clip_inputs=1, finish_limit=WAITED)


def p_rounds(m, e):
    return _segment(m, e, e.probs, mode=RND, clip_inputs=1)


def p_exact(m, e):
    return _segment(m, e, e.probs, mode=XCT, clip_inputs=1)


def p_auto_fallback(m, e):
    """AUTO on the noise-0.45 map, whose sameness values cross 0.5: the speculative fused attempt runs, does not hold
    (not sign-separable), and the image is redone by the rounds inside the same call.  require_proof = -1 keeps the
    rounds' answer (by default AUTO would redo it a second time, in the exact engine); exact_limit = 1024 keeps AUTO
    from choosing the exact engine at once, which it does up to 32768 records (30 x 66 x 10 = 19800)."""
    return _segment(m, e, e.noisy, mode=AUTO, clip_inputs=1, require_proof=-1, exact_limit=1024)


def p_bf16(m, e):
    return _segment(m, e, e.bf16, **SPEC)


def p_logits(m, e):
    return _segment(m, e, e.logits, logits=True, **SPEC)


def p_sweep(m, e):
    sw = m.sweep(e.probs[0], e.probs[1], e.offs, seg.default_options(clip_inputs=1))
    torch.cuda.synchronize()
    return {"bits": _b(sw["bits"]), "neg": _b(sw["neg"]), "cls": _b(sw["cls"]), "gsum": _b(sw["gsum"]),
            "rest": repr((sw["logsum"], sw["pixels_per_lane"], sw["fused_class"], sw["margin_edges"])).encode()}


def p_score(m, e):
    _, _, cls, best = m.score(e.probs[0], e.probs[1], e.offs, seg.default_options(clip_inputs=1), want_arrays=True)
    torch.cuda.synchronize()
    return {"cls": _b(cls), "best": _b(best)}


def p_map_scores(m, e):
    r = m.map_scores(e.probs[0], e.probs[1], e.offs, e.truth, e.truth_classes)
    return {"confusion": _b(r["confusion"]), "sums": _b(r["sums"])}


def p_mask_bce(m, e):
    r = m.mask_bce(e.logits[0], e.logits[1], e.offs, e.truth, e.truth_classes)
    return {"sums": _b(r["sums"]), "grad_class": _b(r["grad_class"]), "grad_same": _b(r["grad_same"])}


def p_plane_sums(m, e):
    return {"class": _b(m.plane_sums(e.logits[0], "class", e.offs, e.truth, e.truth_classes, terms=True)),
            "offset": _b(m.plane_sums(e.logits[1], "offset", e.offs, e.truth, e.truth_classes, complement=True))}


def p_mask_ce(m, e):
    r = m.mask_ce(e.logits[0], "class", e.offs, e.truth, e.truth_classes)
    q = m.mask_ce(e.logits[1], "offset", e.offs, e.truth, e.truth_classes, grad=False)
    return {"sums": _b(r["sums"]), "grad": _b(r["grad"]), "offset_sums": _b(q["sums"])}


def p_encode_rle(m, e):
    return {"rles": repr(m.encode_rle(e.pred, 4)).encode()}


def p_runs(m, e):
    cap = 2048
    wire = torch.zeros(seg.runs_wire_words(cap, 64), dtype=torch.int32, device="cuda")
    seg.pack_runs(m, e.pred, e.pred_table, 4, wire, cap, 64, -4321.125)
    mask, table = seg.unpack_runs(wire, e.H, e.W, cap, 64)
    return {"wire": _b(wire), "mask": _b(mask), "table": _b(table)}


def p_match(m, e):
    t = m.overlap_table(e.pred, e.truth, 4, 4)
    r = m.match_instances(t, e.pred_classes, e.truth_classes, return_iou=True)
    return dict({"overlap": _b(t)}, **{k: _b(v) for k, v in r.items()})


def p_segment_scores(m, e):
    o = seg.default_options(**SPEC)
    mask, table, _, st = m.segment(e.probs[0], e.probs[1], e.offs, o)
    scores = m.instance_scores(st["num_instances"])
    torch.cuda.synchronize()
    return {"mask": _b(mask), "table": _b(table), "scores": _b(scores), "stats": _stats(st)}


SEGMENT_PROBES = {"spec": p_spec, "spec-lean-events": p_spec_lean_events, "spec-replay": p_spec_replay,
                  "ordinary": p_ordinary, "rounds": p_rounds, "exact": p_exact, "auto-fallback": p_auto_fallback,
                  "bf16": p_bf16, "logits": p_logits}
PROBES = dict(SEGMENT_PROBES, **{"sweep": p_sweep, "score": p_score, "map_scores": p_map_scores, "mask_bce": p_mask_bce,
                                 "plane_sums": p_plane_sums, "mask_ce": p_mask_ce, "encode_rle": p_encode_rle,
                                 "runs": p_runs, "match": p_match, "segment+scores": p_segment_scores})
PAIR_SHAPES = ["32x256", "30x66"]
# The exact engine takes about a second per call at 32x256 (one wave pops its 80 000 records) and a fifth of that at
# 30x66: the probe that asks for it runs at the ragged shape only -- the probe list is cut, not the pair rule.
EXACT_ENGINE = ("exact",)
# Where every segment probe must end (stats["mode_used"], with status 0): a probe that slipped onto another engine
# would hold another transition than its name says.
MODE_OF = {"spec": CMP, "spec-lean-events": CMP, "spec-replay": CMP, "ordinary": CMP, "rounds": RND, "exact": XCT,
           "auto-fallback": RND, "bf16": CMP, "logits": CMP, "segment+scores": CMP}


def ended_where_named(probe, res, what):
    if probe in MODE_OF:
        assert b"('status', 0)" in res["stats"], (what, probe, res["stats"])
        assert b"('mode_used', %d)" % MODE_OF[probe] in res["stats"], (what, probe, res["stats"])


def probes_at(shape):
    return [p for p in PROBES if not (shape == "32x256" and p in EXACT_ENGINE)]


def _cases():
    return [(shape, p) for shape in PAIR_SHAPES for p in probes_at(shape)]


def _differs(got, want):
    return sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


@functools.lru_cache(maxsize=None)
def fresh(shape, probe):
    """The probe's bytes on a fresh Merger -- twice, on two Mergers: determinism first."""
    e = inputs(shape)
    res = []
    for _ in range(2):
        m = e.merger()
        try:
            res.append(PROBES[probe](m, e))
        finally:
            m.close()
    assert not _differs(res[0], res[1]), ("not deterministic", shape, probe, _differs(res[0], res[1]))
    ended_where_named(probe, res[0], shape)
    return res[0]


def _held(shape, b, got, what):
    d = _differs(got, fresh(shape, b))
    assert not d, (what, "differs from a fresh Merger's in", d)


# ---- checks ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,probe", _cases(), ids=lambda v: v)
def test_each_probe_is_deterministic(shape, probe):
    """... and every segment probe ends on the engine its name says, with status 0 (fresh() asserts both)."""
    fresh(shape, probe)


@pytest.mark.parametrize("shape,a", _cases(), ids=lambda v: v)
def test_ordered_pairs(shape, a):
    """For every B: B on a Merger that just ran A equals B on a fresh Merger."""
    e = inputs(shape)
    bad = []
    for b in probes_at(shape):
        want = fresh(shape, b)
        m = e.merger()
        try:
            PROBES[a](m, e)
            got = PROBES[b](m, e)
        finally:
            m.close()
        d = _differs(got, want)
        if d:
            bad.append((a, b, d))
    assert not bad, bad


@pytest.mark.parametrize("shape,probe", _cases(), ids=lambda v: v)
def test_steady_state(shape, probe):
    """The same probe five times on one Merger (B after 1, 2, 3 and 4 runs of itself)."""
    e = inputs(shape)
    m = e.merger()
    try:
        for i in range(5):
            _held(shape, probe, PROBES[probe](m, e), (shape, probe, "call %d" % i))
    finally:
        m.close()


@pytest.mark.parametrize("a", list(SEGMENT_PROBES))
def test_another_shape_in_between(a):
    """A at 30x66 with four offsets and C = 3 on a Merger created for 32x256, then B at 32x256."""
    big, small = inputs("32x256"), inputs("small")
    bad = []
    for b in [p for p in SEGMENT_PROBES if p not in EXACT_ENGINE] + ["map_scores"]:
        want = fresh("32x256", b)
        m = big.merger()
        try:
            ended_where_named(a, PROBES[a](m, small), "small")
            got = PROBES[b](m, big)
        finally:
            m.close()
        d = _differs(got, want)
        if d:
            bad.append((a, b, d))
    assert not bad, bad


def test_an_argument_error_in_between():
    e = inputs("32x256")
    m = e.merger()
    try:
        _held("32x256", "spec", p_spec(m, e), "first")
        with pytest.raises(seg.MergeNetError):
            m.segment(e.probs[0], e.probs[1], [(0, 1), (0, -1)] + e.offs[2:], seg.default_options(**SPEC))
        _held("32x256", "spec", p_spec(m, e), "after the refused call")
    finally:
        m.close()
