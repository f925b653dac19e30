"""The certificate's counters and log-likelihood on the GPU against oracle/certificate.py (float64, numpy).

Every test segments with compute_logprob = 1, hands the partition and the classes THE GPU RETURNED to the
reference and asserts the three violation counts, `certified`, `proof` and `total_logprob`.  Whatever partition the
engine ends in, its certificate is checked as a function of that partition (other tests hold the partition to
the oracle's).  Each docstring names which of the five device forms the input reaches -- mn_verify_edges,
mn_verify_edges4, mn_cc_certificate, mn_cc_tail, mn_verify_records / mn_x_verify_records -- and the route
(`mode_used`, `rounds`) is asserted, so a change of routing fails the test instead of testing something else.

Out-of-image entries of every sameness plane are set to 0.5 here: the merger must never read them, and a form
that did would count them on either side.
"""
import numpy as np
import pytest

from mergenet_amd import segmenter as seg
from mergenet_amd import synth
from oracle import certificate as cert

pytestmark = pytest.mark.gpu

F = np.float32

# ---- the band for record violations ---------------------------------------------------------------------------
# The device scores a record in float32 from fixed-point sums, the reference in float64.  Measured: the same
# priorities evaluated in numpy float32 in mn_score's order of operations (`_priorities_f32`), over all records
# of all inputs of this file on the partitions the GPU returned: largest |f32 - f64| =
F32_GAP_MEASURED = 1.9e-7      # (1.86e-7, on a record of priority -0.34 between two objects of different classes)
# B = four times that: numpy does not reproduce the order in which the device accumulates the float32 class sums
# across merges.  A record whose float64 priority lies within B of -margin is "undecided".  Every check below
# also asserts that the gap on ITS records stays within the measured one, so the constant cannot go stale.
BAND = 4 * F32_GAP_MEASURED

OFFS = synth.generate_offsets(6, 4)                    # (1,0), (0,2), (-3,-1), (3,-6)
OFFS_NO_UNIT = [(-2, 3), (2, -1), (0, 2), (3, 1)]      # a negative-row offset, no unit offset
SHAPES = [(48, 64), (47, 66), (33, 67), (16, 130)]     # W % 4 = 0, 2, 3, 2; 16x130: two labelling tiles across
C = 3
WAITED = 8193    # finish_limit above what the fused tail takes: the ordinary (waited) components attempt


def _wxh(shape):
    return "%dx%d" % shape


def _valid(H, W, offs):
    """[O, H, W] bool: the edge (offset k, pixel) stays inside the image."""
    out = np.zeros((len(offs), H, W), bool)
    for k, (di, dj) in enumerate(offs):
        out[k, max(0, -di):min(H, H - di), max(0, -dj):min(W, W - dj)] = True
    return out


def _base(H, W, offs, seed, classes=C, noise=0.1, num_instances=None):
    s = synth.synth_v1(H, W, classes, offs, seed, noise=noise, num_instances=num_instances)
    sp = s.sameness_probs.copy()
    sp[~_valid(H, W, offs)] = 0.5
    return s.class_probs.copy(), sp, s.instances


def _segment(cp, sp, offs, mode, opts=(0.0, 1.0, 0.03), **kw):
    ctx = seg.HostContext(cp.shape[1], cp.shape[2], cp.shape[0], len(offs))
    try:
        o = seg.default_options(same_different_bias=opts[0], object_merge_factor=opts[1], merge_logprob_bias=opts[2],
                                mode=mode, clip_inputs=1, compute_logprob=1, **kw)
        return ctx.segment(cp, sp, offs, o)
    finally:
        ctx.close()


def _priorities_f32(res, omf, bias):
    """The records' priorities in float32, in mn_score's order: a + b per class, first maximum, (best - lu) - lv,
    oml * omf + cdl, / (n_u + n_v), + bias."""
    r = res.records
    a, b = r["lp_u"].astype(F), r["lp_v"].astype(F)
    R = a.shape[0]
    if R == 0:
        return np.zeros(0)
    joint = a + b
    best = joint.max(axis=1)
    lu = np.take_along_axis(a, r["cls_u"][:, None], axis=1)[:, 0]
    lv = np.take_along_axis(b, r["cls_v"][:, None], axis=1)[:, 0]
    cdl = np.where(r["cls_u"] != r["cls_v"], (best - lu) - lv, F(0))
    num = r["logodds"].astype(F) * F(omf) + cdl
    return (num / (r["n_u"] + r["n_v"]).astype(F) + F(bias)).astype(np.float64)


def reference_of(cp, sp, offs, mask, classes, part, opts):
    ocls = cert.object_class_of_root(mask, classes, part)
    return cert.certificate(cp, sp, offs, part, ocls, same_different_bias=opts[0], object_merge_factor=opts[1],
                            merge_logprob_bias=opts[2], clip=True)


def record_bounds(res):
    """(decided violators, undecided) of the reference's records under BAND."""
    d = res.priorities + res.margin                  # > 0: violates
    undecided = np.abs(d) <= BAND
    return int((~undecided & (d >= 0)).sum()), int(undecided.sum())


def check(cp, sp, offs, out, opts, what, *, route, exact=False, max_undecided=0):
    """The assertions of this file on one run.  `route` = (mode_used, rounds)."""
    mask, classes, part, st = out
    res = reference_of(cp, sp, offs, mask, classes, part, opts)
    lo, und = record_bounds(res)
    gap = float(np.abs(_priorities_f32(res, opts[1], opts[2]) - res.priorities).max()) if res.priorities.size else 0.0
    print("CERT %s | route mode %d rounds %d | gpu e %d c %d r %d cert %d proof %d lp %.9g | ref e %d c %d r %d(+%d) "
          "lp %.9g | records %d gap %.3g objects %d" %
          (what, st["mode_used"], st["rounds"], st["cert_edge_violations"], st["cert_class_violations"],
           st["cert_record_violations"], st["certified"], st["proof"], st["total_logprob"], res.edge_violations,
           res.class_violations, lo, und, res.total_logprob, res.priorities.size, gap, np.unique(part).size))
    ctx = (what, st)
    # the comparisons are integer ones on values away from ties
    vals = res.values[np.isfinite(res.values)]
    assert np.abs(vals - 0.5).min() > (0.0 if opts[0] == 0.0 else 1e-4), ctx
    assert res.class_gap > 1e-3, ctx
    assert (st["mode_used"], st["rounds"]) == route, ctx
    assert st["cert_edge_violations"] == res.edge_violations, ctx
    assert st["cert_class_violations"] == res.class_violations, ctx
    assert gap <= F32_GAP_MEASURED, ctx
    assert und <= max_undecided, ctx
    assert lo <= st["cert_record_violations"] <= lo + und, ctx
    allowed = cert.options_allow_certificate(opts[1], opts[2])
    zero = st["cert_edge_violations"] == 0 and st["cert_class_violations"] == 0 and st["cert_record_violations"] == 0
    assert st["certified"] == (1 if zero and allowed else 0), ctx
    if st["certified"]:
        assert st["proof"] == seg.MN_PROOF_CERTIFICATE, ctx
    elif exact:
        assert st["proof"] in (seg.MN_PROOF_SEQUENTIAL, seg.MN_PROOF_SEQUENTIAL_TIES), ctx
    else:
        assert st["proof"] == seg.MN_PROOF_NONE, ctx
    assert abs(st["total_logprob"] - res.total_logprob) <= 1e-5 * abs(res.total_logprob), ctx
    return res, st, und


# ---- inputs ---------------------------------------------------------------------------------------------------------

# seeds at which, on the CPU, the clean map has no violation under bias 0.03 (no instance is swallowed) and the
# reference swallows every planted lone pixel
CLEAN_SEED = {(48, 64): 101, (47, 66): 101, (33, 67): 101, (16, 130): 107}


def clean_input(shape, offs=OFFS):
    H, W = shape
    return _base(H, W, offs, CLEAN_SEED[shape])


def edge_input(shape, offs, E, F_):
    """E values of edges well inside an object set to 0.3, F_ values of edges across a boundary to 0.7, both ends in
    bounds; the first planted pixels sit in the last column, the last row and (W % 4 != 0) the last partial group
    of four."""
    H, W = shape
    cp, sp, inst = clean_input(shape, offs)
    valid = _valid(H, W, offs)
    same = np.zeros_like(valid)
    for k, (di, dj) in enumerate(offs):
        r0, r1, c0, c1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
        same[k, r0:r1, c0:c1] = inst[r0:r1, c0:c1] == inst[r0 + di:r1 + di, c0 + dj:c1 + dj]
    inside = [tuple(x) for x in np.argwhere(valid & same)]
    across = [tuple(x) for x in np.argwhere(valid & ~same)]
    # in order of preference: last column, last row, the last partial group of four, then spread over the image
    firsts = [lambda x: x[2] == W - 1, lambda x: x[1] == H - 1, lambda x: W % 4 != 0 and x[2] >= W - W % 4 and x[2] < W - 1]
    chosen = []
    for want in firsts:
        hit = [x for x in inside if want(x) and x not in chosen]
        if hit:
            chosen.append(hit[len(hit) // 2])
    step = max(1, len(inside) // 7)
    chosen += [x for x in inside[step // 2::step] if x not in chosen]
    plan_in = chosen[:E]
    plan_x = across[len(across) // 3::max(1, len(across) // 7)][:F_]
    assert len(plan_in) == E and len(plan_x) == F_
    cols = [x[2] for x in plan_in]
    rows = [x[1] for x in plan_in]
    if E >= 3:
        assert W - 1 in cols and H - 1 in rows and (W % 4 == 0 or any(W - W % 4 <= c < W - 1 for c in cols))
    else:
        assert W - 1 in cols
    for x in plan_in:
        sp[x] = 0.3
    for x in plan_x:
        sp[x] = 0.7
    return cp, sp, inst


def class_input(shape, k):
    """At k pixels the class map's two largest values are swapped; the sameness planes are as they were."""
    H, W = shape
    cp, sp, inst = clean_input(shape)
    inner = np.argwhere(inst > 0)
    picks = [tuple(x) for x in inner[len(inner) // 5::max(1, len(inner) // 5)][:k]]
    assert len(picks) == k
    for (r, c) in picks:
        order = np.argsort(cp[:, r, c])
        a, b = order[-1], order[-2]
        cp[a, r, c], cp[b, r, c] = cp[b, r, c], cp[a, r, c]
    return cp, sp, inst, picks


def lone_pixels(shape, offs, count, odd_class):
    """`count` single pixels inside the background, each with all its in-bounds edges (as source and as target) at
    0.1 and the background's class; with `odd_class` one more whose class is 1.  Returns the pixel list too."""
    H, W = shape
    cp, sp, inst = clean_input(shape, offs)
    assert int((inst == 0).sum()) >= 1500
    reach = max(max(abs(i), abs(j)) for (i, j) in offs)
    bg = inst == 0
    # pixels whose whole neighbourhood (every offset, both directions, and then some) is background
    ok = np.zeros((H, W), bool)
    m = reach + 1
    for r in range(m, H - m):
        for c in range(m, W - m):
            ok[r, c] = bg[r - m:r + m + 1, c - m:c + m + 1].all()
    cand = [tuple(x) for x in np.argwhere(ok)]
    picks = []
    for x in cand[::max(1, len(cand) // 40)]:
        if all(max(abs(x[0] - y[0]), abs(x[1] - y[1])) > 2 * reach + 1 for y in picks):
            picks.append(x)
        if len(picks) == count + (1 if odd_class else 0):
            break
    assert len(picks) == count + (1 if odd_class else 0), (shape, len(cand), picks)
    for (r, c) in picks:
        for k, (di, dj) in enumerate(offs):
            if 0 <= r + di < H and 0 <= c + dj < W:
                sp[k, r, c] = 0.1
            if 0 <= r - di < H and 0 <= c - dj < W:
                sp[k, r - di, c - dj] = 0.1
    if odd_class:
        r, c = picks[-1]
        cp[0, r, c], cp[1, r, c] = cp[1, r, c], cp[0, r, c]
    return cp, sp, inst, picks


def half_planes(shape, offs, v):
    """Two half-planes of class 1, every edge inside a half at 0.9, every edge across at `v`."""
    H, W = shape
    left = np.zeros((H, W), bool)
    left[:, :W // 2] = True
    cp = np.empty((2, H, W), F)
    cp[0], cp[1] = 0.1, 0.9
    sp = np.full((len(offs), H, W), 0.5, F)
    k_across = 0
    for k, (di, dj) in enumerate(offs):
        r0, r1, c0, c1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
        eq = left[r0:r1, c0:c1] == left[r0 + di:r1 + di, c0 + dj:c1 + dj]
        sp[k, r0:r1, c0:c1] = np.where(eq, F(0.9), F(v))
        k_across += int((~eq).sum())
    return cp, sp, left, k_across


def margin_bias(shape, offs, v, factor):
    """bias >= 0 (a float32) for which the one record's float64 priority k*logit(v)*omf/N + bias is
    -factor * margin, margin = 1e-6 + 1e-5 * bias."""
    H, W = shape
    _, _, _, k = half_planes(shape, offs, v)
    vv = float(F(v))
    x = -k * (np.log(vv) - np.log1p(-vv)) / (H * W)               # -priority without the bias, > 0
    bias = (x - factor * 1e-6) / (1.0 + factor * 1e-5)
    assert bias >= 0
    return float(F(bias))


# ---- the tests -------------------------------------------------------------------------------------------------------

# `stats.rounds` of the general path.  From the cores (the default) these images need ONE round before the finisher
# takes the list; where the rounds start from single pixels (MN_DEBUG_NO_CORES, or a merge factor below what the
# cores accept) it is what the matching needs on that image -- deterministic, as measured on the device:
ROUNDS_OF = {("clean", (48, 64), "rounds-no-cores"): 6, ("clean", (47, 66), "rounds-no-cores"): 6,
             ("clean", (33, 67), "rounds-no-cores"): 5, ("clean", (16, 130), "rounds-no-cores"): 5,
             ("omf", (48, 64), 0): 6, ("omf", (48, 64), 1): 6, ("omf", (47, 66), 0): 6, ("omf", (47, 66), 1): 6}


def _route_rounds(key, default=1):
    return ROUNDS_OF.get(key, default)


@pytest.mark.parametrize("shape", SHAPES, ids=_wxh)
def test_clean_maps_are_certified_on_every_route(shape):
    """Nothing planted: all counters zero, certified = 1.  Forced COMPONENTS: the speculative attempt, mn_cc_tail;
    with finish_limit above the tail's the ordinary attempt, mn_cc_certificate + mn_verify_records.  ROUNDS (from
    the cores and from single pixels) and EXACT: mn_verify_edges4 at 48x64, mn_verify_edges at the other shapes,
    with mn_verify_records resp. mn_x_verify_records."""
    cp, sp, _ = clean_input(shape)
    runs = [("components", seg.MN_MODE_COMPONENTS, {}, (seg.MN_MODE_COMPONENTS, 0)),
            ("components-waited", seg.MN_MODE_COMPONENTS, dict(finish_limit=WAITED), (seg.MN_MODE_COMPONENTS, 0)),
            ("rounds", seg.MN_MODE_ROUNDS, {}, (seg.MN_MODE_ROUNDS, _route_rounds(("clean", shape, "rounds")))),
            ("rounds-no-cores", seg.MN_MODE_ROUNDS, dict(debug_flags=seg.MN_DEBUG_NO_CORES),
             (seg.MN_MODE_ROUNDS, _route_rounds(("clean", shape, "rounds-no-cores")))),
            ("exact", seg.MN_MODE_EXACT, {}, (seg.MN_MODE_EXACT, 0))]
    for name, mode, kw, route in runs:
        out = _segment(cp, sp, OFFS, mode, **kw)
        res, st, _ = check(cp, sp, OFFS, out, (0.0, 1.0, 0.03), "clean %dx%d %s" % (shape + (name,)), route=route,
                           exact=mode == seg.MN_MODE_EXACT)
        assert st["certified"] == 1 and res.all_zero, (name, st)
        assert res.priorities.size > 0          # (there ARE records for the record checks to pass)


def test_clean_map_in_bfloat16_through_the_typed_entry():
    """48x64 as bfloat16 maps through mn_segment_device_t: three routes (mn_cc_tail, mn_verify_edges4 with
    mn_verify_records from the rounds, mn_verify_edges4 with mn_x_verify_records), the reference on the widened
    values."""
    import torch
    shape = (48, 64)
    cp, sp, _ = clean_input(shape)
    tc = torch.from_numpy(cp).cuda().to(torch.bfloat16)
    ts = torch.from_numpy(sp).cuda().to(torch.bfloat16)
    cp16, sp16 = tc.float().cpu().numpy(), ts.float().cpu().numpy()
    merger = seg.Merger(shape[0], shape[1], C, len(OFFS))
    try:
        for name, mode, rounds in (("components", seg.MN_MODE_COMPONENTS, 0),
                                   ("rounds", seg.MN_MODE_ROUNDS, _route_rounds(("clean16", "rounds"))),
                                   ("exact", seg.MN_MODE_EXACT, 0)):
            o = seg.default_options(mode=mode, clip_inputs=1, compute_logprob=1)
            mask, table, part, st = merger.segment(tc, ts, OFFS, o, want_partition=True)
            torch.cuda.synchronize()
            classes = [int(x) for x in table.cpu().numpy()[:st["num_instances"]]]
            out = (mask.cpu().numpy(), classes, part.cpu().numpy(), st)
            res, st, _ = check(cp16, sp16, OFFS, out, (0.0, 1.0, 0.03), "clean bfloat16 %s" % name, route=(mode, rounds),
                               exact=mode == seg.MN_MODE_EXACT)
            assert st["certified"] == 1, (name, st)
    finally:
        merger.close()


@pytest.mark.parametrize("offs", [OFFS, OFFS_NO_UNIT], ids=["spiral", "no-unit"])
@pytest.mark.parametrize("shape", SHAPES, ids=_wxh)
def test_planted_edge_violations_are_counted_by_the_sweeps(shape, offs):
    """E edges inside objects at 0.3 and F edges across boundaries at 0.7 (planted in the last column, the last row and
    the last partial group of four): the map is no longer separable, forced COMPONENTS falls back to the rounds, and
    the per-pixel sweep counts -- mn_verify_edges4 at 48x64 (W % 4 == 0), mn_verify_edges at 47x66, 33x67, 16x130 --
    with mn_verify_records on what the finisher left.  The count expected is the reference's on the returned
    partition, not E + F."""
    which = 0 if offs is OFFS else 1
    for (E, F_) in ((1, 1), (5, 1), (1, 5), (5, 5)):
        cp, sp, _ = edge_input(shape, offs, E, F_)
        out = _segment(cp, sp, offs, seg.MN_MODE_COMPONENTS)
        route = (seg.MN_MODE_ROUNDS, _route_rounds(("edges", shape, which, E, F_)))
        res, st, _ = check(cp, sp, offs, out, (0.0, 1.0, 0.03), "edges %dx%d offs %d E %d F %d" % (shape + (which, E, F_)),
                           route=route)
        assert res.edge_violations > 0 and st["certified"] == 0, st


@pytest.mark.parametrize("shape", SHAPES, ids=_wxh)
def test_planted_class_violations(shape):
    """k pixels inside instances whose two largest class values are swapped, sameness untouched: the pixels stay in
    their objects and are counted by mn_verify_edges4 (48x64) / mn_verify_edges (other shapes), from the rounds and
    from the exact engine (with mn_x_verify_records)."""
    for k in (1, 4):
        cp, sp, _, picks = class_input(shape, k)
        for name, mode in (("rounds", seg.MN_MODE_ROUNDS), ("exact", seg.MN_MODE_EXACT)):
            out = _segment(cp, sp, OFFS, mode)
            rounds = 0 if mode == seg.MN_MODE_EXACT else _route_rounds(("class", shape, k))
            res, st, _ = check(cp, sp, OFFS, out, (0.0, 1.0, 0.03), "class %dx%d k %d %s" % (shape + (k, name)),
                               route=(mode, rounds), exact=mode == seg.MN_MODE_EXACT)
            assert res.class_violations >= k and st["certified"] == 0, st


@pytest.mark.parametrize("waited", [False, True], ids=["mn_cc_tail", "mn_cc_certificate"])
@pytest.mark.parametrize("shape", SHAPES, ids=_wxh)
def test_second_phase_merges_on_the_components_forms(oracle, shape, waited):
    """Single pixels inside the background with every edge at 0.1: own components, sign-separable, and with bias
    0.03 the record sum / (1 + n) + 0.03 is positive, so the second phase swallows them and each of their edges
    becomes a violation: merged_E, merged_S and the compsize count of the components forms.  One pixel, three, and
    three plus one of class 1 (still swallowed: one class violation, a non-zero class delta).  The speculative
    attempt keeps such an image: mn_cc_tail; with finish_limit above the tail's the ordinary attempt runs:
    mn_cc_certificate + mn_verify_records.  Both are COMPONENTS with 0 rounds; what tells them apart is
    finish_limit (make_plan: speculate needs finish_limit <= MN_FIN2_MAXR)."""
    H, W = shape
    for count, odd in ((1, False), (3, False), (3, True)):
        cp, sp, inst, picks = lone_pixels(shape, OFFS, count, odd)
        ref = oracle.run_csegment(cp, sp, C, OFFS, 0.0, 1.0, 0.03)
        bg_root = np.bincount(ref.partition.reshape(-1)).argmax()
        for p in picks:                                              # precondition: the reference swallows them
            assert ref.partition[p] == bg_root, (shape, count, odd, p)
        kw = dict(finish_limit=WAITED) if waited else {}
        out = _segment(cp, sp, OFFS, seg.MN_MODE_COMPONENTS, **kw)
        res, st, _ = check(cp, sp, OFFS, out, (0.0, 1.0, 0.03),
                           "lone %dx%d n %d odd %d waited %d" % (shape + (count, odd, waited)),
                           route=(seg.MN_MODE_COMPONENTS, 0))
        part = out[2]
        n_edges = 0
        for p in picks:
            assert part[p] == part[0, 0] == np.bincount(part.reshape(-1)).argmax(), (st, p)
            n_edges += sum(0 <= p[0] + s * di < H and 0 <= p[1] + s * dj < W for (di, dj) in OFFS for s in (1, -1))
        assert st["cert_edge_violations"] >= n_edges > 0, st            # (other swallowed instances may add theirs)
        assert st["cert_class_violations"] >= (1 if odd else 0), st
        assert st["certified"] == 0


MARGIN_V = 0.02      # logit -3.9: the bias that balances it is ~0.5, the margin 6e-6, half of it well above BAND


@pytest.mark.parametrize("shape", [(48, 64), (33, 67)], ids=_wxh)
def test_one_record_on_either_side_of_the_margin(oracle, shape):
    """Two half-planes, one record of k edges at 0.02 between them; bias chosen so that its float64 priority is
    -0.5 * margin (negative, but inside the margin: ONE record violation, not certified, no merge) and -2 * margin
    (none, certified).  Each engine has its own record check: forced COMPONENTS -> mn_cc_tail; COMPONENTS with
    finish_limit above the tail's -> mn_verify_records behind mn_cc_certificate; ROUNDS -> mn_verify_records behind
    the sweep; EXACT -> mn_x_verify_records."""
    cp, sp, left, k = half_planes(shape, OFFS, MARGIN_V)
    for factor, want in ((0.5, 1), (2.0, 0)):
        bias = margin_bias(shape, OFFS, MARGIN_V, factor)
        opts = (0.0, 1.0, bias)
        ref = oracle.run_csegment(cp, sp, 2, OFFS, *opts)
        assert np.unique(ref.partition).size == 2
        for name, mode, kw in (("components", seg.MN_MODE_COMPONENTS, {}),
                               ("components-waited", seg.MN_MODE_COMPONENTS, dict(finish_limit=WAITED)),
                               ("rounds", seg.MN_MODE_ROUNDS, {}), ("exact", seg.MN_MODE_EXACT, {})):
            out = _segment(cp, sp, OFFS, mode, opts, **kw)
            rounds = _route_rounds(("margin", shape)) if mode == seg.MN_MODE_ROUNDS else 0
            res, st, _ = check(cp, sp, OFFS, out, opts, "margin %dx%d x%.1f %s" % (shape + (factor, name)),
                               route=(mode, rounds), exact=mode == seg.MN_MODE_EXACT)
            ctx = (name, factor, bias, st)
            assert res.priorities.size == 1 and res.records["edges"][0] == k, ctx
            assert res.priorities[0] == pytest.approx(-factor * res.margin, rel=2e-2), ctx
            assert abs(res.priorities[0] + res.margin) > BAND, ctx                  # decided
            assert st["cert_record_violations"] == want and st["certified"] == 1 - want, ctx
            assert st["cert_edge_violations"] == 0 and st["cert_class_violations"] == 0, ctx
            assert oracle.masks_equivalent(out[0], out[1], ref.mask, ref.object_class), ctx
            assert oracle.same_partition(out[2], ref.partition), ctx


@pytest.mark.parametrize("shape", [(48, 64), (47, 66)], ids=_wxh)
def test_tiny_merge_factor_takes_the_sign_from_the_float_gain(shape):
    """object_merge_factor = 1e-25 makes `by_value` false in mn_verify_edges4 (48x64) and mn_verify_edges (47x66): the
    sign of an edge is that of the float32 gain (log v - log(1 - v)) * omf.  ROUNDS only (components mode refuses this
    factor); a clean map with bias 0 (certified), and the planted edges."""
    opts = (0.0, 1e-25, 0.0)
    cp, sp, _ = clean_input(shape)
    out = _segment(cp, sp, OFFS, seg.MN_MODE_ROUNDS, opts)
    res, st, _ = check(cp, sp, OFFS, out, opts, "omf clean %dx%d" % shape,
                       route=(seg.MN_MODE_ROUNDS, _route_rounds(("omf", shape, 0))))
    assert st["certified"] == 1, st
    cp, sp, _ = edge_input(shape, OFFS, 5, 5)
    out = _segment(cp, sp, OFFS, seg.MN_MODE_ROUNDS, opts)
    res, st, _ = check(cp, sp, OFFS, out, opts, "omf edges %dx%d" % shape,
                       route=(seg.MN_MODE_ROUNDS, _route_rounds(("omf", shape, 1))))
    assert res.edge_violations > 0 and st["certified"] == 0, st
    # forced COMPONENTS with this factor is routed to the rounds before anything runs (make_plan: contractible)
    out = _segment(cp, sp, OFFS, seg.MN_MODE_COMPONENTS, opts)
    assert out[3]["mode_used"] == seg.MN_MODE_ROUNDS


@pytest.mark.parametrize("shape", [(48, 64), (33, 67)], ids=_wxh)
def test_same_different_bias_and_the_clip(shape):
    """same_different_bias = 0.3 (the value is logit, add, sigmoid in every form) on the planted edges, and
    clip_inputs = 1 on a map holding exact 0.0 and 1.0.  Forced COMPONENTS: the planted edges go to the rounds
    (mn_verify_edges4 / mn_verify_edges + mn_verify_records), the clipped map stays (mn_cc_tail)."""
    opts = (0.3, 1.0, 0.03)
    cp, sp, _ = edge_input(shape, OFFS, 5, 5)
    out = _segment(cp, sp, OFFS, seg.MN_MODE_COMPONENTS, opts)
    res, st, _ = check(cp, sp, OFFS, out, opts, "sdb %dx%d" % shape,
                       route=(seg.MN_MODE_ROUNDS, _route_rounds(("sdb", shape))))
    assert res.edge_violations > 0, st
    cp, sp, _ = clean_input(shape)
    valid = _valid(shape[0], shape[1], OFFS)
    sp[valid & (sp > 0.95)] = 1.0
    sp[valid & (sp < 0.05)] = 0.0
    assert (sp[valid] == 1.0).sum() > 10 and (sp[valid] == 0.0).sum() > 10
    for mode, rounds in ((seg.MN_MODE_COMPONENTS, 0), (seg.MN_MODE_ROUNDS, _route_rounds(("clip", shape)))):
        out = _segment(cp, sp, OFFS, mode)
        res, st, _ = check(cp, sp, OFFS, out, (0.0, 1.0, 0.03), "clip %dx%d mode %d" % (shape + (mode,)),
                           route=(mode, rounds))
        assert st["certified"] == 1, st


FUZZ_SEED = 20261018


def fuzz_trials():
    rng = np.random.default_rng(FUZZ_SEED)
    for trial in range(16):
        H, W = int(rng.integers(8, 41)), int(rng.integers(8, 141))
        classes = int(rng.integers(2, 7))
        offs = synth.generate_offsets(int(rng.integers(3, 8)), int(rng.integers(3, 9)))
        noise = [0.1, 0.3, 0.45][trial % 3]
        bias = [0.0, 0.03, 0.1][int(rng.integers(0, 3))]
        cp, sp, _ = _base(H, W, offs, 7000 + trial, classes=classes, noise=noise)
        yield trial, cp, sp, offs, (0.0, 1.0, bias), noise


def test_fuzz_of_sixteen_trials():
    """Random shapes 8..40 x 8..140, 2..6 classes, 3..8 offsets, noise 0.1 / 0.3 / 0.45, bias 0 / 0.03 / 0.1, forced
    COMPONENTS: whatever route a trial takes -- mn_cc_tail when it stays, mn_verify_edges / mn_verify_edges4 with
    mn_verify_records when it falls back -- the same assertions hold.  At noise 0.45 values cross 0.5, so those
    trials are the ones that fall back."""
    used = {seg.MN_MODE_COMPONENTS: 0, seg.MN_MODE_ROUNDS: 0}
    all_decided = 0
    for trial, cp, sp, offs, opts, noise in fuzz_trials():
        out = _segment(cp, sp, offs, seg.MN_MODE_COMPONENTS, opts)
        st = out[3]
        assert st["mode_used"] in used, st
        assert (st["rounds"] == 0) == (st["mode_used"] == seg.MN_MODE_COMPONENTS), st
        assert (st["mode_used"] == seg.MN_MODE_ROUNDS) == (noise == 0.45), st       # the route is the noise's
        res, st, und = check(cp, sp, offs, out, opts, "fuzz %d %dx%d C %d O %d noise %.2f bias %.2f" %
                             (trial, cp.shape[1], cp.shape[2], cp.shape[0], len(offs), noise, opts[2]),
                             route=(st["mode_used"], st["rounds"]), max_undecided=1 << 30)
        used[st["mode_used"]] += 1
        all_decided += und == 0
    assert used[seg.MN_MODE_COMPONENTS] >= 5 and used[seg.MN_MODE_ROUNDS] >= 4, used
    assert all_decided >= 14, all_decided
