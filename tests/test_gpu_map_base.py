"""The readers of the class and sameness maps -- the sweep (mn_cc_sign), its class part, mn_cc_cross, the
log-probability pass, the score kernels, the rounds, the exact engine's phase A -- and the output stage, with the
caller's buffers at every base address an element type allows, against references that know nothing of addresses.

The table is map_base_util's (test_map_base.py holds it on the host): the smallest shapes at which each form of the
sweep exists, float32 / float16 / bfloat16, and the class and sameness maps 0 .. 14 bytes behind a 16-byte boundary,
one at a time and both.  The kernels read through 8- and 16-byte loads whose C++ type promises more alignment than
such a caller gives; the tests hold that the result does not depend on it.

Every test first asserts that Merger.sweep reports the pixels per lane the table states for the very views it is about
to use, so a case that silently took another form fails instead of passing for the wrong reason.

References.  The partition is topology_util.components (a union-find that is not the project's oracle), the mask and
classes topology_util.reference_mask, total_logprob the csegment oracle's on the float32 values the kernels see, within
the 1e-5 relative of test_gpu_topology.py and test_gpu_parity.py.  "An address is not an input": everything a call
returns must be bit-equal to the same call on aligned copies on the same Merger; total_logprob and the counts are
compared as numbers where both calls ran in the same form (nothing but the addresses differs then), and within the
1e-5 of the oracle where a misaligned 16-bit base turned 8 pixels per lane into 4.

total_logprob of two aligned calls on one Merger (two copies of the maps at different 16-byte aligned addresses) is
asserted bit-equal as well: test_two_aligned_calls_agree_bit_for_bit.
"""
import numpy as np
import pytest
import torch

import lean_util
import map_base_util as mb
import topology_util as tu
from mergenet_amd import segmenter as seg, synth

pytestmark = pytest.mark.gpu

WAITED = 8193        # finish_limit above MN_FIN2_MAXR = 8192: the ordinary (waited) components attempt
# `tail`: default options, the speculative attempt that ends in mn_cc_tail, which takes at most 1024 records between
# components.  Every case has fewer (test_map_base.py) but the two of random3-35x131, the one-pixel-per-lane control,
# with 4046: there the library redoes the attempt on the waited one, so both attempts of those two cases end in the
# waited finish; serpentine-1-1-35x131 is the one-pixel-per-lane shape whose `tail` attempt is the speculative one.
ATTEMPTS = {"tail": {}, "waited": dict(finish_limit=WAITED)}
FULL, PX4_16 = seg.MN_DEBUG_SWEEP_FULL_FORM, seg.MN_DEBUG_SWEEP16_4PX
LOWP = ("float16", "bfloat16")


@pytest.fixture(scope="module")
def mergers(request):
    """One Merger per shape, made at its first use, with room for the longest offset list of the table."""
    made = {}

    def get(shape):
        if shape not in made:
            H, W = mb.HW[shape]
            made[shape] = seg.Merger(H, W, tu.C, max(len(c.offs) for c in mb.CASES if mb.shape_of(c) == shape))
        return made[shape]

    def close():
        for m in made.values():
            m.close()

    request.addfinalizer(close)
    return get


_device_maps = {}        # per (case, dtype, logits): the aligned maps on the device; emptied with the module's Mergers
_oracle_logprob = {}


@pytest.fixture(scope="module", autouse=True)
def _release_caches():
    yield
    _device_maps.clear()
    _oracle_logprob.clear()


def _aligned_maps(case, dtype, logits):
    key = (case.name, dtype, logits)
    if key not in _device_maps:
        cv, sv, cb, sb = (mb.host_logits if logits else mb.host_maps)(case.name, dtype)
        _device_maps[key] = (mb.to_device(cv, cb, dtype), mb.to_device(sv, sb, dtype))
    return _device_maps[key]


def _views(case, dtype, pair, logits=False):
    """Fresh copies of the case's maps, the class maps pair[0] and the sameness maps pair[1] bytes behind a 16-byte
    boundary."""
    cp, sp = _aligned_maps(case, dtype, logits)
    return mb.at_base(cp, pair[0]), mb.at_base(sp, pair[1])


def _logprob(oracle, case, dtype, logits=False):
    key = (case.name, dtype, logits)
    if key not in _oracle_logprob:
        if logits:
            cx, sx, _, _ = mb.host_logits(case.name, dtype)
            cp, sp = mb.probabilities_of_logits(cx), mb.probabilities_of_logits(sx)
        else:
            cp, sp, _, _ = mb.host_maps(case.name, dtype)
        _oracle_logprob[key] = oracle.run_csegment(cp, sp, tu.C, case.offs, *mb.OPTS).total_logprob
    return _oracle_logprob[key]


def _opts(mode=seg.MN_MODE_COMPONENTS, **kw):
    return seg.default_options(same_different_bias=mb.OPTS[0], object_merge_factor=mb.OPTS[1],
                               merge_logprob_bias=mb.OPTS[2], mode=mode, clip_inputs=1, compute_logprob=1, **kw)


def _assert_form(merger, views, case, dtype, pair, opts, logits=False):
    """The sweep of these very views runs in the form the table states."""
    px = merger.sweep(views[0], views[1], case.offs, opts, logits=logits)["pixels_per_lane"]
    want = mb.expected_px(mb.shape_of(case), dtype, pair, sweep16_4px=bool(opts.debug_flags & PX4_16))
    assert px == want, (case.name, dtype, pair, px, want)
    return px


def _segment(merger, views, case, opts, logits=False):
    mask, table, part, st = merger.segment(views[0], views[1], case.offs, opts, want_partition=True, logits=logits)
    torch.cuda.synchronize()
    return dict(mask=mask.cpu().numpy(), table=table.cpu().numpy(), part=part.cpu().numpy(), st=st)


def _check_against_references(res, oracle, case, dtype, ctx, logits=False, mode=seg.MN_MODE_COMPONENTS):
    st = res["st"]
    ctx = (ctx, st)
    mask, classes, objects = mb.reference(case.name)
    assert st["status"] == 0 and st["mode_used"] == mode, ctx
    assert oracle.same_partition(res["part"], case.comp), ctx
    got_classes = [int(c) for c in res["table"][:st["num_instances"]]]
    assert oracle.masks_equivalent(res["mask"], got_classes, mask, classes), ctx
    # (with the options (0, 1, 0) the partition is the union-find's in every mode, so the oracle's total_logprob and
    #  a clean certificate hold for the rounds and the exact engine as they do for components mode: there the
    #  certificate is the log-probability pass over the sameness maps, mn_verify_edges4 / mn_verify_edges)
    assert st["num_objects"] == objects, ctx
    assert st["certified"] == 1, ctx
    assert (st["cert_edge_violations"], st["cert_class_violations"], st["cert_record_violations"]) == (0, 0, 0), ctx
    want = _logprob(oracle, case, dtype, logits)
    assert abs(st["total_logprob"] - want) <= 1e-5 * abs(want), (ctx, want)


def _assert_outputs_equal(got, want, ctx):
    for name in ("mask", "table", "part"):
        assert got[name].tobytes() == want[name].tobytes(), (name, ctx)
    assert got["st"]["status"] == want["st"]["status"] == 0, ctx
    assert got["st"]["mode_used"] == want["st"]["mode_used"], ctx
    assert got["st"]["num_instances"] == want["st"]["num_instances"], ctx


def _assert_address_is_no_input(got, px, want, want_px, oracle, case, dtype, ctx, logits=False):
    """Check 2: bit-equal arrays; the numbers too where the form is the same, else the oracle's tolerance."""
    _assert_outputs_equal(got, want, ctx)
    a, b = got["st"], want["st"]
    if px == want_px:
        assert a["total_logprob"] == b["total_logprob"], (ctx, a["total_logprob"], b["total_logprob"])
        assert a["num_objects"] == b["num_objects"], ctx
    else:
        assert dtype in LOWP and (want_px, px) == (8, 4), ctx
        ref = _logprob(oracle, case, dtype, logits)
        assert abs(a["total_logprob"] - ref) <= 1e-5 * abs(ref), (ctx, a["total_logprob"], ref)
        assert a["num_objects"] == b["num_objects"], ctx


def _components_on_every_pair(mergers, oracle, case, dtype, attempt, flags=0, logits=False):
    """Checks 1 and 2 of one (case, dtype, attempt): every pair of bases against the references, and every
    misaligned pair against the aligned call on the same Merger."""
    merger = mergers(mb.shape_of(case))
    opts = _opts(debug_flags=flags, **ATTEMPTS[attempt])
    want = want_px = None
    for pair in mb.pairs(dtype):
        ctx = (case.name, dtype, pair, attempt, flags, logits)
        views = _views(case, dtype, pair, logits)
        px = _assert_form(merger, views, case, dtype, pair, opts, logits)
        got = _segment(merger, views, case, opts, logits)
        _check_against_references(got, oracle, case, dtype, ctx, logits)
        if pair == (0, 0):
            want, want_px = got, px
        else:
            _assert_address_is_no_input(got, px, want, want_px, oracle, case, dtype, ctx, logits)


# ---- 1, 2: components mode against the references, and against the aligned call -------------------------------------

@pytest.mark.parametrize("attempt", list(ATTEMPTS))
@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("case", mb.CASES, ids=repr)
def test_components_at_every_base(mergers, oracle, case, dtype, attempt):
    """Every (shape, dtype, pair) on both attempts: status, mode, partition == union-find, mask and classes,
    certificate, total_logprob within 1e-5 of the oracle; and every misaligned pair bit-equal to the aligned call
    (mask, table, partition; total_logprob and num_objects as numbers where pixels_per_lane agrees)."""
    _components_on_every_pair(mergers, oracle, case, dtype, attempt)


@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("case", mb.CASES, ids=repr)
def test_two_aligned_calls_agree_bit_for_bit(mergers, case, dtype):
    """Two copies of the maps at different 16-byte aligned addresses: total_logprob is reproducible on one Merger,
    which is what lets check 2 compare it as a number."""
    merger = mergers(mb.shape_of(case))
    for attempt, kw in ATTEMPTS.items():
        opts = _opts(**kw)
        first = _views(case, dtype, (0, 0))
        second = _views(case, dtype, (0, 0))
        assert first[0].data_ptr() != second[0].data_ptr() and first[1].data_ptr() != second[1].data_ptr()
        a, b = _segment(merger, first, case, opts), _segment(merger, second, case, opts)
        _assert_outputs_equal(a, b, (case.name, dtype, attempt))
        assert a["st"]["total_logprob"] == b["st"]["total_logprob"], (case.name, dtype, attempt)
        assert a["st"]["num_objects"] == b["st"]["num_objects"]


# ---- 3: the full form, and the 4-pixel form of 16-bit maps ------------------------------------------------------------------

FULL_FORM_CASES = [c for c in mb.CASES if mb.shape_of(c) in ("comb3-32x136", "serpentine-1-1-17x68", "serpentine-2-2-34x66")]


@pytest.mark.parametrize("attempt", list(ATTEMPTS))
@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("case", FULL_FORM_CASES, ids=repr)
def test_components_under_the_full_sweep_form(mergers, oracle, case, dtype, attempt):
    """MN_DEBUG_SWEEP_FULL_FORM: mn_cc_sums and mn_cc_class_sums read what the lean form's readers did not."""
    _components_on_every_pair(mergers, oracle, case, dtype, attempt, flags=FULL)


@pytest.mark.parametrize("attempt", list(ATTEMPTS))
@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("case", [c for c in mb.CASES if mb.shape_of(c) == "comb3-32x136"], ids=repr)
def test_components_under_the_4_pixel_16_bit_form(mergers, oracle, case, dtype, attempt):
    """MN_DEBUG_SWEEP16_4PX at N % 8 == 0: 8-byte loads from an aligned base, then from 8, 4, 2 and 14 mod 16."""
    _components_on_every_pair(mergers, oracle, case, dtype, attempt, flags=PX4_16)


# ---- 4: the sweep's own outputs -----------------------------------------------------------------------------------------------

def _sweep(merger, views, case, opts):
    sw = merger.sweep(views[0], views[1], case.offs, opts)
    torch.cuda.synchronize()
    out = dict(px=sw["pixels_per_lane"], logsum=sw["logsum"], fused=sw["fused_class"],
               bits=sw["bits"].cpu().numpy().view(np.uint32), neg=sw["neg"].cpu().numpy().view(np.uint32))
    out["cls"] = sw["cls"].cpu().numpy() if sw["cls"] is not None else None
    out["gsum"] = sw["gsum"].cpu().numpy() if sw["gsum"] is not None else None
    return out


@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("case", mb.CASES, ids=repr)
def test_sweep_outputs_at_every_base(mergers, case, dtype):
    """bits == the label map's positive masks at every base; bits, neg (its NaN pattern included), cls, gsum and
    logsum bit-equal to the aligned call's wherever both ran with the same pixels per lane."""
    merger = mergers(mb.shape_of(case))
    opts = _opts()
    O = len(case.offs)
    pos = lean_util.pos_bits_of(case.lab, case.offs)
    want = None
    for pair in mb.pairs(dtype):
        ctx = (case.name, dtype, pair)
        views = _views(case, dtype, pair)
        got = _sweep(merger, views, case, opts)
        assert got["px"] == mb.expected_px(mb.shape_of(case), dtype, pair), ctx
        assert got["fused"] == (got["px"] >= 4), ctx
        assert np.array_equal(got["bits"] & np.uint32((1 << O) - 1), pos), ctx
        # the negative edges are the complement inside the image: their values are listed, everything else is NaN
        listed = ~np.isnan(got["neg"].view(np.float32))
        for k, (di, dj) in enumerate(case.offs):
            H, W = case.lab.shape
            inside = np.zeros((H, W), bool)
            inside[max(0, -di):min(H, H - di), max(0, -dj):min(W, W - dj)] = True
            assert np.array_equal(listed[k], inside & ((pos >> np.uint32(k)) & 1 == 0)), (ctx, k)
        if pair == (0, 0):
            want = got
            continue
        if got["px"] != want["px"]:
            assert dtype in LOWP and (want["px"], got["px"]) == (8, 4), ctx
            assert np.array_equal(got["bits"], want["bits"]) and np.array_equal(got["neg"], want["neg"]), ctx
            assert np.array_equal(got["cls"], want["cls"]), ctx
            continue
        for name in ("bits", "neg", "cls", "gsum"):
            assert (got[name] is None) == (want[name] is None), (name, ctx)
            if got[name] is not None:
                assert got[name].tobytes() == want[name].tobytes(), (name, ctx)
        assert got["logsum"] == want["logsum"], (ctx, got["logsum"], want["logsum"])


# ---- 5: logits ------------------------------------------------------------------------------------------------------------------

LOGIT_CASES = [c for c in mb.CASES if mb.shape_of(c) in ("comb3-32x136", "serpentine-1-1-17x68")]


@pytest.mark.parametrize("attempt", list(ATTEMPTS))
@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("case", LOGIT_CASES, ids=repr)
def test_logits_at_every_base(mergers, oracle, case, dtype, attempt):
    """The same maps as logits (logits=True): the sigmoid on load behind the same wide loads."""
    _components_on_every_pair(mergers, oracle, case, dtype, attempt, logits=True)


# ---- 6: the other readers -----------------------------------------------------------------------------------------------------

OTHER_CASES = [c for c in mb.CASES if mb.shape_of(c) == "serpentine-1-1-17x68"]


def _bit_equal_nan_aware(a, b):
    """float32 arrays: NaN in the same places, and the same bit patterns (the sign of a zero included) elsewhere."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.mark.parametrize("dtype", mb.DTYPES)
@pytest.mark.parametrize("case", OTHER_CASES, ids=repr)
def test_rounds_exact_score_and_phase_a_at_the_edge_bases(mergers, oracle, case, dtype):
    """MN_MODE_ROUNDS with core_radius = 1, MN_MODE_EXACT, score(want_arrays=True) and exact_phase_a: bit-equal to
    the aligned call on the same Merger; the two modes give the union-find partition.  In these modes the certificate
    and total_logprob come from the log-probability pass over the sameness maps (mn_verify_edges4 at W % 4 == 0, four
    values per lane through mn_ld_map4): certified, no violation, total_logprob within 1e-5 of the oracle and equal
    as a number to the aligned call's."""
    merger = mergers(mb.shape_of(case))
    modes = {seg.MN_MODE_ROUNDS: _opts(seg.MN_MODE_ROUNDS, core_radius=1), seg.MN_MODE_EXACT: _opts(seg.MN_MODE_EXACT)}
    plain = _opts()

    def run(pair):
        ctx = (case.name, dtype, pair)
        views = _views(case, dtype, pair)
        _assert_form(merger, views, case, dtype, pair, plain)
        out = {}
        for mode, o in modes.items():
            out[mode] = _segment(merger, views, case, o)
            _check_against_references(out[mode], oracle, case, dtype, (ctx, mode), mode=mode)
        _, _, cls, best = merger.score(views[0], views[1], case.offs, plain, want_arrays=True)
        a_cls, oml, prio = merger.exact_phase_a(views[0], views[1], case.offs, plain)
        torch.cuda.synchronize()
        out["score"] = (cls.cpu().numpy(), best.cpu().numpy())
        out["phase_a"] = (a_cls.cpu().numpy(), oml.cpu().numpy(), prio.cpu().numpy())
        return out

    want = run((0, 0))
    assert np.isnan(want["phase_a"][1]).any() and np.isfinite(want["phase_a"][1]).any()
    for pair in [(0, 0)] + mb.edge_pairs(dtype):         # (first a second aligned copy: the numbers are reproducible)
        ctx = (case.name, dtype, pair)
        got = run(pair)
        for mode in modes:
            _assert_outputs_equal(got[mode], want[mode], (ctx, mode))
            a, b = got[mode]["st"], want[mode]["st"]
            assert a["num_objects"] == b["num_objects"], (ctx, mode)
            # every row of 17x68 takes four pixels per lane: nothing but the addresses differs, and what the
            # log-probability pass read through mn_ld_same4 must come out as the same number
            assert a["total_logprob"] == b["total_logprob"], (ctx, mode, a["total_logprob"], b["total_logprob"])
            assert a["certified"] == b["certified"] == 1, (ctx, mode)
        for a, b in zip(got["score"], want["score"]):
            assert a.tobytes() == b.tobytes(), ctx
        assert got["phase_a"][0].tobytes() == want["phase_a"][0].tobytes(), ctx
        assert _bit_equal_nan_aware(got["phase_a"][1], want["phase_a"][1]), ctx
        assert _bit_equal_nan_aware(got["phase_a"][2], want["phase_a"][2]), ctx


# ---- 7: caller-owned outputs ----------------------------------------------------------------------------------------------

SENTINEL = -7


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("shape", ["comb3-32x136", "serpentine-1-1-17x68"])
def test_callers_mask_and_table_at_every_base(mergers, oracle, shape, dtype):
    """segment_async(out=(mask, table)) with the caller's buffers 4, 8 and 12 bytes behind a 16-byte boundary (the
    aligned call takes the four-pixel output kernel: N % 4 == 0): the same mask and table, and not one element
    written outside them."""
    case = mb.FIRST_OF_SHAPE[shape]
    merger = mergers(shape)
    H, W = case.lab.shape
    N = H * W
    assert N % 4 == 0
    opts = _opts()
    views = _views(case, dtype, (0, 0))
    _assert_form(merger, views, case, dtype, (0, 0), opts)
    ref_mask, ref_classes, _ = mb.reference(case.name)

    def run(mask_base, table_base):
        ctx = (shape, dtype, mask_base, table_base)
        mask, mbuf, m0 = mb.at_base_guarded(torch.full((H, W), SENTINEL, dtype=torch.int32, device="cuda"), mask_base,
                                            fill=SENTINEL)
        table, tbuf, t0 = mb.at_base_guarded(torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda"), table_base,
                                             fill=SENTINEL)
        assert mask.data_ptr() % 16 == mask_base and table.data_ptr() % 16 == table_base, ctx
        assert mask.is_contiguous() and table.is_contiguous()
        out_mask, out_table, _, st = merger.segment_async(views[0], views[1], case.offs, opts, out=(mask, table)).result()
        torch.cuda.synchronize()
        assert out_mask.data_ptr() == mask.data_ptr() and out_table.data_ptr() == table.data_ptr()
        assert st["status"] == 0 and st["mode_used"] == seg.MN_MODE_COMPONENTS, (ctx, st)
        assert mb.guards_hold(mbuf, m0, N, SENTINEL), ("mask guards", ctx)
        assert mb.guards_hold(tbuf, t0, N, SENTINEL), ("table guards", ctx)
        return mask.cpu().numpy(), table.cpu().numpy(), st["num_instances"]

    want_mask, want_table, K = run(0, 0)
    assert oracle.masks_equivalent(want_mask, [int(c) for c in want_table[:K]], ref_mask, ref_classes)
    for b in (4, 8, 12):
        for mask_base, table_base in ((b, b), (b, 0), (0, b)):
            mask, table, k = run(mask_base, table_base)
            assert k == K
            assert mask.tobytes() == want_mask.tobytes(), (shape, dtype, mask_base, table_base)
            assert table[:K].tobytes() == want_table[:K].tobytes(), (shape, dtype, mask_base, table_base)


# ---- 8: the pipeline that produces such bases -----------------------------------------------------------------------------

@pytest.mark.parametrize("out_dtype", [torch.float16, torch.bfloat16])
def test_prepare_then_segment_on_slices_of_its_result(oracle, out_dtype):
    """prepare(out_dtype = 16 bits) returns ONE [C + O, H, W] tensor; with C = 3 at 17x68 (N % 8 == 4) the sameness
    maps maps[C:] start 8 bytes behind a 16-byte boundary.  The call on the slices against the oracle on the same
    values, and bit-equal to the call on aligned copies."""
    H, W, C = 17, 68, 3
    offs = [tuple(int(x) for x in o) for o in synth.generate_offsets(8, 6)]
    O = len(offs)
    s = synth.synth_v1(2 * H, 2 * W, C, offs, 77, num_instances=3)
    probs = np.concatenate([s.class_probs, s.sameness_probs]).clip(1e-4, 1 - 1e-4)
    logits = torch.from_numpy(np.log(probs / (1 - probs)).astype(np.float32)).cuda()
    m = seg.Merger(2 * H, 2 * W, C, O)
    try:
        maps = m.prepare(logits, H, W, apply_sigmoid=True, out_dtype=out_dtype)
        cp, sp = maps[:C], maps[C:]
        assert maps.data_ptr() % 16 == 0 and cp.data_ptr() % 16 == 0 and sp.data_ptr() % 16 == 8
        assert cp.is_contiguous() and sp.is_contiguous()
        bias = (0.0, 1.0, 0.03)
        # the halved maps no longer match the offsets' geometry -> order-dependent input: EXACT mode
        o = seg.default_options(same_different_bias=bias[0], object_merge_factor=bias[1], merge_logprob_bias=bias[2],
                                mode=seg.MN_MODE_EXACT, compute_logprob=1)
        assert m.sweep(cp, sp, offs, o)["pixels_per_lane"] == 4          # (16 bits, N % 8 == 4: four whatever the base)

        def run(a, b):
            mask, table, part, st = m.segment(a, b, offs, o, want_partition=True)
            torch.cuda.synchronize()
            return dict(mask=mask.cpu().numpy(), table=table.cpu().numpy(), part=part.cpu().numpy(), st=st)

        got = run(cp, sp)
        host = maps.float().cpu().numpy()
        ref = oracle.run_csegment(host[:C], host[C:], C, offs, *bias)
        got_classes = [int(c) for c in got["table"][:got["st"]["num_instances"]]]
        assert got["st"]["status"] == 0 and got["st"]["mode_used"] == seg.MN_MODE_EXACT, got["st"]
        assert oracle.masks_equivalent(got["mask"], got_classes, ref.mask, ref.object_class), got["st"]
        # the exact engine's total_logprob is the log-probability pass over maps[C:]: the oracle's, within the 1e-5
        # relative of test_gpu_parity.py
        lp = got["st"]["total_logprob"]
        assert abs(lp - ref.total_logprob) <= 1e-5 * abs(ref.total_logprob), (lp, ref.total_logprob)
        a, b = cp.clone(), sp.clone()
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        clones = run(a, b)
        _assert_outputs_equal(clones, got, ("clones", out_dtype))
        for key in ("total_logprob", "certified", "cert_edge_violations", "cert_class_violations",
                    "cert_record_violations", "num_objects"):
            assert clones["st"][key] == got["st"][key], (key, clones["st"], got["st"])
    finally:
        m.close()
