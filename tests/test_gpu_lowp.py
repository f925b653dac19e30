"""float16 / bfloat16 probability maps read in their own width (the *_t entry points).

The contract is an identity: a call on 16-bit maps gives what the float32 path gives on ``maps.float()`` with
``clip_inputs = 1`` (widening is exact, every kernel computes in float32 after the load, a 16-bit map is always
clipped on load).  Everything is compared bit for bit except the two sums a lane of 8 pixels regroups
(``total_logprob``, the sweep's ``logsum``): 1e-5 relative, the bound of tests/test_gpu_phase_a.py; where the
4-pixel form ran they are bit-equal too.
"""
import ctypes

import numpy as np
import pytest

import lowp_util
from mergenet_amd import segmenter as seg, synth

pytestmark = pytest.mark.gpu

MODES = {"components": dict(mode=seg.MN_MODE_COMPONENTS, require_proof=-1), "rounds": dict(mode=seg.MN_MODE_ROUNDS),
         "exact": dict(mode=seg.MN_MODE_EXACT), "auto": dict(mode=seg.MN_MODE_AUTO)}
STATS = ["mode_used", "proof", "certified", "num_instances", "num_objects", "merges", "finisher_steps", "tied_steps",
         "tied_merges", "tied_conflicts", "cert_edge_violations", "cert_class_violations", "cert_record_violations"]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _maps(v):
    """(16-bit class / sameness tensors, their float32 widening) of a vector on the GPU."""
    lo = (lowp_util.to_torch(v["class_bits"], v["dtype"], "cuda"), lowp_util.to_torch(v["same_bits"], v["dtype"], "cuda"))
    hi = (lo[0].float().contiguous(), lo[1].float().contiguous())
    assert np.array_equal(hi[0].cpu().numpy().view(np.uint32), v["class_probs"].view(np.uint32))   # torch widens as numpy
    return lo, hi


def _result(out):
    mask, table, part, st = out
    return dict(mask=mask.cpu().numpy(), table=table.cpu().numpy(), part=part.cpu().numpy() if part is not None else None,
                stats=st)


def _assert_same(got, want, exact_logprob, what):
    assert np.array_equal(got["mask"], want["mask"]), what
    assert np.array_equal(got["table"], want["table"]), what
    if got["part"] is not None and want["part"] is not None:
        assert np.array_equal(got["part"], want["part"]), what
    for k in STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])
    a, b = got["stats"]["total_logprob"], want["stats"]["total_logprob"]
    print("%s: total_logprob %.17g (16 bit) %.17g (float32)" % (what, a, b))
    if np.isnan(a) or np.isnan(b):
        assert np.isnan(a) and np.isnan(b), what
    elif exact_logprob:
        assert a == b, (what, a, b)
    else:
        assert abs(a - b) <= 1e-5 * abs(b), (what, a, b)


_quantised = {}


def _synth_vector(H, W, dtype, seed=1000):
    key = (H, W, dtype, seed)
    if key not in _quantised:
        offs = synth.generate_offsets(40, 10)
        s = synth.synth_v1(H, W, 9, offs, seed)
        cb, cw = lowp_util.quantize(s.class_probs, dtype)
        sb, sw = lowp_util.quantize(s.sameness_probs, dtype)
        _quantised[key] = dict(class_bits=cb, same_bits=sb, class_probs=cw, sameness_probs=sw, offsets=offs, dtype=dtype,
                               spec=dict(H=H, W=W, C=9))
        if len(_quantised) > 2:                       # (a 1024x2048 vector is 320 MB on the host)
            _quantised.pop(next(iter(_quantised)))
    return _quantised[key]


_float_results = {}


def _float_result(name, v, hi, mode):
    """The float32 path's result on the widened maps (fresh context), kept for the tests that compare with it."""
    key = (name, mode)
    if key not in _float_results:
        m = seg.Merger(v["spec"]["H"], v["spec"]["W"], v["spec"]["C"], len(v["offsets"]))
        try:
            o = seg.default_options(clip_inputs=1, **MODES[mode])
            _float_results[key] = _result(m.segment(hi[0], hi[1], v["offsets"], o, want_partition=True))
        finally:
            m.close()
    return _float_results[key]


# ---- 1. widening is exact ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", lowp_util.DTYPES)
def test_widening_is_exact_on_every_pattern_of_the_unit_interval(dtype):
    pat = lowp_util.unit_interval_patterns(dtype)
    assert pat.size == (15361 if dtype == "float16" else 16257)
    rows = (pat.size + 127) // 128
    padded = np.zeros(rows * 128, np.uint16)
    padded[:pat.size] = pat
    x = lowp_util.to_torch(padded.reshape(1, rows, 128), dtype, "cuda")
    m = seg.Merger(rows, 128, 4, 4)
    try:
        got = m.prepare(x, rows, 128, apply_sigmoid=False, clip=False)
    finally:
        m.close()
    import torch
    assert got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), x.float().cpu().numpy().view(np.uint32))
    assert np.array_equal(got.cpu().numpy().reshape(-1)[:pat.size].view(np.uint32),
                          lowp_util.widen(pat, dtype).view(np.uint32))


# ---- 2. identity with the float32 path ----------------------------------------------------------------------

def _identity(name, v, modes):
    lo, hi = _maps(v)
    H, W = v["spec"]["H"], v["spec"]["W"]
    m = seg.Merger(H, W, v["spec"]["C"], len(v["offsets"]))
    try:
        for mode in modes:
            o = seg.default_options(**MODES[mode])            # clip_inputs = 0: a 16-bit map is clipped all the same
            got = _result(m.segment(lo[0], lo[1], v["offsets"], o, want_partition=True))
            want = _float_result(name, v, hi, mode)
            _assert_same(got, want, exact_logprob=(H * W) % 8 != 0 or W % 8 != 0, what="%s/%s" % (name, mode))
    finally:
        m.close()


@pytest.mark.parametrize("name", lowp_util.names())
def test_identity_with_the_float_path_on_the_vectors(name):
    _identity(name, lowp_util.load(name), list(MODES))


@pytest.mark.parametrize("dtype", lowp_util.DTYPES)
def test_identity_with_the_float_path_256x512(dtype):
    _identity("synth_256x512_" + dtype, _synth_vector(256, 512, dtype), list(MODES))


@pytest.mark.parametrize("dtype", lowp_util.DTYPES)
def test_identity_with_the_float_path_1024x2048(dtype):
    # (COMPONENTS only: the exact engine takes half a minute per call at this size)
    _identity("synth_1024x2048_" + dtype, _synth_vector(1024, 2048, dtype), ["components"])
    _float_results.pop(("synth_1024x2048_" + dtype, "components"), None)


# ---- 3. the reference's result ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", lowp_util.names())
def test_default_options_give_the_references_result(name):
    v = lowp_util.load(name)
    lo, _ = _maps(v)
    m = seg.Merger(v["spec"]["H"], v["spec"]["W"], v["spec"]["C"], len(v["offsets"]))
    try:
        o = seg.default_options(same_different_bias=v["opts"][0], object_merge_factor=v["opts"][1],
                                merge_logprob_bias=v["opts"][2])
        mask, table, _, st = m.segment(lo[0], lo[1], v["offsets"], o)
    finally:
        m.close()
    print("%s: mode_used %d proof %d tied_steps %d tied_conflicts %d tie_order_used %d" %
          (name, st["mode_used"], st["proof"], st["tied_steps"], st["tied_conflicts"], st["tie_order_used"]))
    classes = [int(c) for c in table.cpu().numpy()[:st["num_instances"]]]
    from mergenet_amd.labels import masks_equivalent
    assert masks_equivalent(mask.cpu().numpy(), classes, v["mask"], v["object_class"])
    assert st["proof"] in (seg.MN_PROOF_CERTIFICATE, seg.MN_PROOF_SEQUENTIAL)


# ---- 4. sweep and phase A ---------------------------------------------------------------------------------

def _bits(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("dtype", lowp_util.DTYPES)
@pytest.mark.parametrize("shape", [(256, 512, 0, 8), (256, 512, seg.MN_DEBUG_SWEEP16_4PX, 4),
                                   (96, 100, 0, 4),      # W % 8 != 0: 4 pixels per lane, 8-byte loads
                                   (50, 102, 0, 4),      # W % 4 != 0, N % 4 == 0: lanes that run over a row's end
                                   (33, 47, 0, 1)])      # N % 4 != 0: one pixel per lane
def test_sweep_and_phase_a_equal_the_float_path(dtype, shape):
    H, W, flags, px = shape
    v = _synth_vector(H, W, dtype, seed=1000 + H)
    lo, hi = _maps(v)
    offs = v["offsets"]
    m = seg.Merger(H, W, 9, len(offs))
    try:
        got = m.sweep(lo[0], lo[1], offs, seg.default_options(debug_flags=flags))
        want = m.sweep(hi[0], hi[1], offs, seg.default_options(clip_inputs=1))
        assert got["pixels_per_lane"] == px and want["pixels_per_lane"] == min(px, 4)
        assert got["fused_class"] == want["fused_class"] == (px >= 4)
        assert got["margin_edges"] == want["margin_edges"]
        assert np.array_equal(_bits(got["bits"]), _bits(want["bits"]))
        assert np.array_equal(_bits(got["neg"]), _bits(want["neg"]))          # NaN pattern included
        if px >= 4:
            assert np.array_equal(_bits(got["cls"]), _bits(want["cls"]))
            assert np.array_equal(_bits(got["gsum"]), _bits(want["gsum"]))
        print("%dx%d %s px %d: logsum %.17g (16 bit) %.17g (float32)" % (H, W, dtype, px, got["logsum"], want["logsum"]))
        if px == 8:
            assert abs(got["logsum"] - want["logsum"]) <= 1e-5 * abs(want["logsum"])
        else:
            assert got["logsum"] == want["logsum"]
        a = m.exact_phase_a(lo[0], lo[1], offs, seg.default_options())
        b = m.exact_phase_a(hi[0], hi[1], offs, seg.default_options(clip_inputs=1))
        for x, y, what in zip(a, b, ("cls", "oml", "prio")):
            assert np.array_equal(_bits(x), _bits(y)), what
        if flags == 0:
            s1 = m.score(lo[0], lo[1], offs, seg.default_options(), want_arrays=True)
            s2 = m.score(hi[0], hi[1], offs, seg.default_options(clip_inputs=1), want_arrays=True)
            assert np.array_equal(s1[2].cpu().numpy(), s2[2].cpu().numpy())
            assert np.array_equal(s1[3].cpu().numpy(), s2[3].cpu().numpy())
    finally:
        m.close()


# ---- 5. batch ---------------------------------------------------------------------------------------------

def test_exact_batch_in_bfloat16_equals_the_single_calls():
    names = ["lowp_synth_s1001_bf16", "lowp_blur_s8001_bf16", "lowp_confident_s1003_bf16"]
    vs = [lowp_util.load(n) for n in names]
    maps = [_maps(v)[0] for v in vs]
    offs = vs[0]["offsets"]
    batch = seg.ExactBatch(64, 128, 9, len(offs), 3)
    try:
        for proof in (0, 1):
            o = seg.default_options(mode=seg.MN_MODE_EXACT, require_proof=proof)
            res = batch.segment([a for a, _ in maps], [b for _, b in maps], offs, o, want_partition=True)
            for i, (v, r) in enumerate(zip(vs, res)):
                single = seg.Merger(64, 128, 9, len(offs))
                try:
                    want = _result(single.segment(maps[i][0], maps[i][1], offs, o, want_partition=True))
                finally:
                    single.close()
                got = _result(r)
                _assert_same(got, want, exact_logprob=True, what="batch/%s/require_proof=%d" % (names[i], proof))
                if proof == 1:
                    assert got["stats"]["proof"] in (seg.MN_PROOF_CERTIFICATE, seg.MN_PROOF_SEQUENTIAL)
    finally:
        batch.close()


# ---- 6. prepare -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", lowp_util.DTYPES)
@pytest.mark.parametrize("shape", [((19, 64, 96), (32, 48)), ((5, 50, 70), (25, 35)),
                                   ((3, 33, 47), (64, 90)), ((2, 17, 9), (17, 9))])
@pytest.mark.parametrize("sigmoid", [False, True])
def test_prepare_with_16_bit_ends(dtype, shape, sigmoid):
    import torch
    (K, Hin, Win), (Ho, Wo) = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randn((K, Hin, Win), generator=g) * 3 if sigmoid else torch.rand((K, Hin, Win), generator=g)
    td = lowp_util.torch_dtype(dtype)
    x = x.to(td).cuda().contiguous()
    m = seg.Merger(max(Hin, Ho), max(Win, Wo), 4, 4)
    try:
        want = m.prepare(x.float().contiguous(), Ho, Wo, apply_sigmoid=sigmoid, clip=True)
        got = m.prepare(x, Ho, Wo, apply_sigmoid=sigmoid, clip=True)
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
        low = m.prepare(x, Ho, Wo, apply_sigmoid=sigmoid, clip=True, out_dtype=td)
        assert low.dtype == td and torch.equal(low.view(torch.int16), want.to(td).view(torch.int16))
        low32 = m.prepare(x.float().contiguous(), Ho, Wo, apply_sigmoid=sigmoid, clip=True, out_dtype=td)
        assert torch.equal(low32.view(torch.int16), want.to(td).view(torch.int16))
    finally:
        m.close()


# ---- 7. no float32 copy -----------------------------------------------------------------------------------

def test_workspace_is_the_same_after_bfloat16_and_float32_calls():
    v = lowp_util.load("lowp_blur_s8001_bf16")
    lo, hi = _maps(v)
    offs = v["offsets"]
    a, b = seg.Merger(64, 128, 9, len(offs)), seg.Merger(64, 128, 9, len(offs))
    try:
        assert a.workspace_bytes() == b.workspace_bytes()
        for mode in MODES:
            a.segment(hi[0], hi[1], offs, seg.default_options(clip_inputs=1, **MODES[mode]))
            b.segment(lo[0], lo[1], offs, seg.default_options(**MODES[mode]))
            assert a.workspace_bytes() == b.workspace_bytes(), mode
    finally:
        a.close()
        b.close()


# ---- 8. one context, changing dtype -----------------------------------------------------------------------

def test_one_context_alternating_dtypes():
    import torch
    vf, vb = lowp_util.load("lowp_synth_s1001_f16"), lowp_util.load("lowp_blur_s8001_bf16")
    (lf, hf), (lb, hb) = _maps(vf), _maps(vb)
    offs = vf["offsets"]
    # (name of the float result, vector, maps, options): a float32, a float16 and a bfloat16 call of one shape
    calls = [("lowp_synth_s1001_f16", vf, hf, dict(clip_inputs=1)), ("lowp_synth_s1001_f16", vf, lf, {}),
             ("lowp_blur_s8001_bf16", vb, lb, {})]
    m = seg.Merger(64, 128, 9, len(offs))
    try:
        for mode in MODES:
            for name, v, maps, extra in calls + calls:
                o = seg.default_options(**dict(MODES[mode], **extra))
                want = _float_result(name, v, _maps(v)[1], mode)
                exact = maps[0].dtype == torch.float32
                _assert_same(_result(m.segment(maps[0], maps[1], offs, o, want_partition=True)), want, exact,
                             "blocking/%s/%s/%s" % (name, mode, maps[0].dtype))
                pend = m.segment_async(maps[0], maps[1], offs, o, want_partition=True)
                _assert_same(_result(pend.result()), want, exact, "async/%s/%s/%s" % (name, mode, maps[0].dtype))
        # the serving loop: fixed buffers per dtype, graphs recorded at the second and replayed from the third call
        flags = seg.MN_DEBUG_LEAN_EVENTS | seg.MN_DEBUG_REPLAY
        outs = [(torch.empty((64, 128), dtype=torch.int32, device="cuda"),
                 torch.empty((64 * 128,), dtype=torch.int32, device="cuda")) for _ in calls]
        for rounds, order in ((2, [0, 1, 2]), (1, [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 0, 1, 2])):
            for _ in range(rounds):
                for i in order:
                    name, v, maps, extra = calls[i]
                    o = seg.default_options(debug_flags=flags, **extra)
                    want = _float_result(name, v, _maps(v)[1], "auto")
                    mask, table, _, st = m.segment_async(maps[0], maps[1], offs, o, out=outs[i]).result()
                    got = dict(mask=mask.cpu().numpy(), table=table.cpu().numpy(), part=None, stats=st)
                    _assert_same(got, want, maps[0].dtype == torch.float32, "replay/%s/%s" % (name, maps[0].dtype))
    finally:
        m.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------

def test_refusals():
    import torch
    v = lowp_util.load("lowp_synth_s1001_f16")
    lo, hi = _maps(v)
    offs = v["offsets"]
    m = seg.Merger(64, 128, 9, len(offs))
    try:
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            m.segment(lo[0], hi[1], offs)                              # mixed dtypes
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            m.segment(hi[0].double(), hi[1].double(), offs)
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            m.prepare(hi[0].double(), 64, 128)
        with pytest.raises(ValueError):
            m.segment_async(lo[0], lo[1].to(torch.bfloat16), offs)
        off = np.ascontiguousarray(np.asarray(offs, dtype=np.int32).reshape(-1, 2))
        mask = torch.empty((64, 128), dtype=torch.int32, device="cuda")
        table = torch.empty((64 * 128,), dtype=torch.int32, device="cuda")
        o = seg.default_options()
        st = seg.MnStats()
        rc = m.lib.mn_segment_device_t(m.handle, lo[0].data_ptr(), 9, lo[1].data_ptr(), len(offs), 7, 128, 64, 9,
                                       off.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), mask.data_ptr(),
                                       table.data_ptr(), None, ctypes.byref(o), None, ctypes.byref(st))
        assert rc == seg.MN_ERR_ARGUMENT and st.status == seg.MN_ERR_ARGUMENT
        rc = m.lib.mn_prepare_device_t(m.handle, lo[0].data_ptr(), 7, 9, 64, 128, hi[0].data_ptr(), 0, 64, 128, 0, 1, None)
        assert rc == seg.MN_ERR_ARGUMENT
        # the context is still good
        got = _result(m.segment(lo[0], lo[1], offs, seg.default_options(**MODES["auto"]), want_partition=True))
        _assert_same(got, _float_result("lowp_synth_s1001_f16", v, hi, "auto"), False, "after the refusals")
    finally:
        m.close()
