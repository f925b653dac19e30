"""Logits as maps (MN_MAPS_LOGITS, ``logits=True``): the sigmoid is taken where an element is loaded.

The contract is an identity.  A call on logits ``x`` gives what the float32 path gives on
``p = Merger.prepare(x, H, W, apply_sigmoid=True, clip=False)`` with ``clip_inputs = 1``: that kernel writes
``1.0f / (1.0f + expf(-(float)x))`` as float32 (its interpolation at unchanged size returns the tap itself), and logits
are always clipped on load.  Everything is compared bit for bit except the two sums that a lane of 8 pixels regroups
(``total_logprob``, the sweep's ``logsum``) where 16-bit logits take 8 pixels per lane and the float32 yardstick 4:
1e-5 relative, the bound of tests/test_gpu_lowp.py and tests/test_gpu_phase_a.py.  The code under test is never its
own reference: every yardstick is the probability path, in float32.

Inputs: ``x = log(p) - log1p(-p)`` in float64 of synth-v1 / blurred-v1 probabilities, rounded to the element type,
with the extremes of ``PLANT`` over the first two rows of every plane.
"""
import ctypes

import numpy as np
import pytest

import lowp_util
from mergenet_amd import segmenter as seg, synth
from test_gpu_lowp import STATS

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float16", "bfloat16")
MODES = {"components": dict(mode=seg.MN_MODE_COMPONENTS, require_proof=-1), "rounds": dict(mode=seg.MN_MODE_ROUNDS),
         "exact": dict(mode=seg.MN_MODE_EXACT), "auto": dict(mode=seg.MN_MODE_AUTO)}
# the float32 sigmoid is exactly 1.0 from about 17 up and exactly 0 below about -104; 3e4 is near binary16's largest
PLANT = [17.0, -17.0, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0, 3e4, -3e4, -0.0]
PLANT_WIDE = [1e30, -1e30, np.inf, -np.inf]          # float32 / bfloat16 only (binary16 ends at 65504)

# name -> (H, W, C, arguments of generate_offsets)
SHAPES = {"64x128": (64, 128, 9, (40, 10)),      # float32: 4 pixels per lane, fused class planes; 16-bit: 8 per lane
          "30x50": (30, 50, 9, (40, 10)),        # N % 4 == 0, W % 4 == 2, N % 8 != 0: straddling lanes, 16-bit at 4
          "33x35": (33, 35, 9, (40, 10)),        # N odd: one pixel per lane, separate class pass
          "24x40c81": (24, 40, 81, (20, 16))}    # more classes than lanes of a chunk, two offset groups past 10


def _planted(dtype):
    return PLANT + (PLANT_WIDE if dtype != "float16" else [])


def _plant(x, dtype, whole=False):
    """The extremes over the first two rows of every plane (`whole`: over all of it), rotated from plane to plane."""
    K, H, W = x.shape
    vals = np.asarray(_planted(dtype), np.float64)
    n = H * W if whole else 2 * W
    for k in range(K):
        x[k].reshape(-1)[:n] = np.resize(np.roll(vals, k), n)
    return x


def _to_device(x64, dtype):
    x32 = np.ascontiguousarray(x64, dtype=np.float32)
    if dtype == "float32":
        import torch
        return torch.from_numpy(x32).cuda()
    bits, _ = lowp_util.quantize(x32, dtype)
    return lowp_util.to_torch(bits, dtype, "cuda")


def _logit64(p):
    p = p.astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.log(p) - np.log1p(-p)            # (+inf where synth writes 1.0: an edge that leaves the image)


_cases = {}


def _case(kind, shape, dtype, seed=3000):
    """dict: x = (class, sameness) logits of `dtype` on the GPU, p = their float32 probabilities by Merger.prepare
    (the yardstick's input), offs, H, W, C.  Made once per key and left unchanged."""
    key = (kind, shape, dtype, seed)
    if key not in _cases:
        H, W, C, oa = SHAPES[shape]
        offs = synth.generate_offsets(*oa)
        if kind == "saturated":
            xc = _plant(np.zeros((C, H, W)), dtype, whole=True)
            xs = _plant(np.zeros((len(offs), H, W)), dtype, whole=True)
        else:
            s = (synth.blurred_v1(H, W, C, offs, seed, radius=2) if kind == "blur" else synth.synth_v1(H, W, C, offs, seed))
            xc = _plant(_logit64(s.class_probs), dtype)
            xs = _plant(_logit64(s.sameness_probs), dtype)
        x = (_to_device(xc, dtype), _to_device(xs, dtype))
        m = seg.Merger(H, W, C, len(offs))
        try:
            p = tuple(m.prepare(t, H, W, apply_sigmoid=True, clip=False) for t in x)
        finally:
            m.close()
        import torch
        assert p[0].dtype == torch.float32 and p[0].shape == x[0].shape
        _cases[key] = dict(x=x, p=p, offs=offs, H=H, W=W, C=C, dtype=dtype, key=key)
    return _cases[key]


def _px(v):
    """Pixels per lane of the sweep: (the logits form's, the float32 yardstick's)."""
    N, W = v["H"] * v["W"], v["W"]
    if N % 4 != 0 or W < 4:
        return 1, 1
    return (8 if v["dtype"] != "float32" and N % 8 == 0 and W % 8 == 0 else 4), 4


def _result(out):
    mask, table, part, st = out
    return dict(mask=mask.cpu().numpy(), table=table.cpu().numpy(), part=part.cpu().numpy() if part is not None else None,
                stats=st)


def _assert_same(got, want, exact_logprob, what):
    assert got["stats"]["status"] == want["stats"]["status"] == 0, what
    assert np.array_equal(got["mask"], want["mask"]), what
    assert np.array_equal(got["table"], want["table"]), what
    if got["part"] is not None and want["part"] is not None:
        assert np.array_equal(got["part"], want["part"]), what
    for k in STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])
    a, b = got["stats"]["total_logprob"], want["stats"]["total_logprob"]
    print("%s: total_logprob %.17g (logits) %.17g (float32 probabilities)" % (what, a, b))
    if np.isnan(a) or np.isnan(b):
        assert np.isnan(a) and np.isnan(b), what
    elif exact_logprob:
        assert a == b, (what, a, b)
    else:
        assert abs(a - b) <= 1e-5 * abs(b), (what, a, b)


_yardsticks = {}


def _yardstick(v, maps=None, **opts):
    """The float32 probability path's result on the case's probabilities (`maps`: on these instead), in a fresh context
    with clip_inputs = 1; kept for the tests that share it."""
    key = (v["key"], maps is not None, tuple(sorted(opts.items())))
    maps = v["p"] if maps is None else maps
    if key not in _yardsticks:
        m = seg.Merger(v["H"], v["W"], v["C"], len(v["offs"]))
        try:
            o = seg.default_options(clip_inputs=1, **opts)
            _yardsticks[key] = _result(m.segment(maps[0], maps[1], v["offs"], o, want_partition=True))
        finally:
            m.close()
    return _yardsticks[key]


def _bits(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


# ---- 1. the sweep -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,bias", [("64x128", 0.0), ("30x50", 0.0), ("33x35", 0.0), ("24x40c81", 0.0),
                                        ("64x128", 0.1)])      # (a bias: the non-plain instantiation)
def test_sweep_equals_the_probability_path(dtype, shape, bias):
    v = _case("synth", shape, dtype)
    px, px32 = _px(v)
    m = seg.Merger(v["H"], v["W"], v["C"], len(v["offs"]))
    try:
        got = m.sweep(v["x"][0], v["x"][1], v["offs"], seg.default_options(same_different_bias=bias), logits=True)
        want = m.sweep(v["p"][0], v["p"][1], v["offs"], seg.default_options(same_different_bias=bias, clip_inputs=1))
    finally:
        m.close()
    assert got["pixels_per_lane"] == px and want["pixels_per_lane"] == px32
    if dtype != "float32" and shape in ("64x128", "24x40c81"):
        assert got["pixels_per_lane"] == 8
    assert got["fused_class"] == want["fused_class"] == (px >= 4)
    assert got["margin_edges"] == want["margin_edges"]
    assert np.array_equal(_bits(got["bits"]), _bits(want["bits"]))
    assert np.array_equal(_bits(got["neg"]), _bits(want["neg"]))          # NaN pattern included
    if px >= 4:
        assert np.array_equal(_bits(got["cls"]), _bits(want["cls"]))
        assert np.array_equal(_bits(got["gsum"]), _bits(want["gsum"]))
    print("%s %s bias %g px %d: logsum %.17g (logits) %.17g (float32 probabilities)" %
          (shape, dtype, bias, px, got["logsum"], want["logsum"]))
    if px == px32:
        assert got["logsum"] == want["logsum"]
    else:
        assert abs(got["logsum"] - want["logsum"]) <= 1e-5 * abs(want["logsum"])


# ---- 2. phase A of the exact engine, the score kernels ----------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["64x128", "33x35"])
def test_phase_a_and_score_equal_the_probability_path(dtype, shape):
    v = _case("synth", shape, dtype)
    m = seg.Merger(v["H"], v["W"], v["C"], len(v["offs"]))
    try:
        a = m.exact_phase_a(v["x"][0], v["x"][1], v["offs"], seg.default_options(), logits=True)
        b = m.exact_phase_a(v["p"][0], v["p"][1], v["offs"], seg.default_options(clip_inputs=1))
        for x, y, what in zip(a, b, ("cls", "oml", "prio")):
            assert np.array_equal(_bits(x), _bits(y)), what
        s1 = m.score(v["x"][0], v["x"][1], v["offs"], seg.default_options(), want_arrays=True, logits=True)
        s2 = m.score(v["p"][0], v["p"][1], v["offs"], seg.default_options(clip_inputs=1), want_arrays=True)
        assert np.array_equal(s1[2].cpu().numpy(), s2[2].cpu().numpy())
        assert np.array_equal(s1[3].cpu().numpy(), s2[3].cpu().numpy())
    finally:
        m.close()


# ---- 3. segmentation --------------------------------------------------------------------------------------

def _identity(kind, shape, dtype, modes, **extra):
    v = _case(kind, shape, dtype)
    px, px32 = _px(v)
    m = seg.Merger(v["H"], v["W"], v["C"], len(v["offs"]))
    try:
        for mode in modes:
            opts = dict(MODES[mode], **extra)
            o = seg.default_options(**opts)                   # clip_inputs = 0: logits are clipped all the same
            got = _result(m.segment(v["x"][0], v["x"][1], v["offs"], o, want_partition=True, logits=True))
            want = _yardstick(v, **opts)
            _assert_same(got, want, px == px32, "%s/%s/%s/%s%s" % (kind, shape, dtype, mode, extra or ""))
    finally:
        m.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["synth", "blur"])
def test_segmentation_equals_the_probability_path_64x128(dtype, kind):
    _identity(kind, "64x128", dtype, list(MODES))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["30x50", "33x35", "24x40c81"])
def test_segmentation_equals_the_probability_path_other_shapes(dtype, shape):
    _identity("synth", shape, dtype, ["exact", "auto"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_segmentation_pysegmenter_variant(dtype):
    _identity("synth", "64x128", dtype, ["exact", "auto"], variant=seg.MN_VARIANT_PYSEGMENTER)


@pytest.mark.parametrize("dtype", DTYPES)
def test_segmentation_with_same_different_bias(dtype):
    _identity("blur", "64x128", dtype, ["exact", "auto"], same_different_bias=0.1)


def test_exact_mode_on_logits_gives_the_cpu_oracles_result():
    from oracle import checker as ck
    v = _case("synth", "64x128", "bfloat16")
    m = seg.Merger(v["H"], v["W"], v["C"], len(v["offs"]))
    try:
        o = seg.default_options(mode=seg.MN_MODE_EXACT, require_proof=1)
        mask, table, _, st = m.segment(v["x"][0], v["x"][1], v["offs"], o, logits=True)
    finally:
        m.close()
    # (the oracle clips as the binding does: the probabilities travel unclipped, as the logits did)
    ref = ck.run_csegment(v["p"][0].cpu().numpy(), v["p"][1].cpu().numpy(), v["C"], v["offs"],
                          o.same_different_bias, o.object_merge_factor, o.merge_logprob_bias)
    classes = [int(c) for c in table.cpu().numpy()[:st["num_instances"]]]
    print("proof %d tied_steps %d tied_conflicts %d; total_logprob %.17g (logits) %.17g (oracle)" %
          (st["proof"], st["tied_steps"], st["tied_conflicts"], st["total_logprob"], ref.total_logprob))
    assert ck.masks_equivalent(mask.cpu().numpy(), classes, ref.mask, ref.object_class)
    assert abs(st["total_logprob"] - ref.total_logprob) <= 1e-5 * abs(ref.total_logprob)


# ---- 4. saturation ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_a_map_of_nothing_but_extremes(dtype):
    v = _case("saturated", "64x128", dtype)
    px, px32 = _px(v)
    m = seg.Merger(v["H"], v["W"], v["C"], len(v["offs"]))
    try:
        for mode in ("components", "auto"):
            o = seg.default_options(clip_inputs=0, **MODES[mode])      # clip_inputs = 0: the clip is on regardless
            got = _result(m.segment(v["x"][0], v["x"][1], v["offs"], o, want_partition=True, logits=True))
            assert got["stats"]["status"] == 0
            assert got["mask"].min() >= 0 and got["mask"].max() <= got["stats"]["num_instances"]
            assert np.isfinite(got["stats"]["total_logprob"])
            want = _yardstick(v, **MODES[mode])
            _assert_same(got, want, px == px32, "saturated/%s/%s" % (dtype, mode))
    finally:
        m.close()


# ---- 5. async and replay ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_async_and_replay_never_cross_the_flag(dtype):
    import torch
    vs = [_case("synth", "64x128", dtype, seed=3000 + i) for i in range(4)]
    v0 = vs[0]
    px, px32 = _px(v0)
    H, W, C, offs = v0["H"], v0["W"], v0["C"], v0["offs"]
    a, b = seg.Merger(H, W, C, len(offs)), seg.Merger(H, W, C, len(offs))
    try:
        # two contexts alternating: the launch of image i + 1 precedes the read-back of image i
        # (components mode, unproven results kept: the speculative path, which is what the replay records)
        fast = MODES["components"]
        o = seg.default_options(**fast)
        pend = None
        for i, v in enumerate(vs):
            nxt = (a, b)[i & 1].segment_async(v["x"][0], v["x"][1], offs, o, want_partition=True, logits=True)
            if pend is not None:
                _assert_same(_result(pend.result()), _yardstick(vs[i - 1], **fast), px == px32,
                             "async/%s/%d" % (dtype, i - 1))
            pend = nxt
        _assert_same(_result(pend.result()), _yardstick(vs[3], **fast), px == px32, "async/%s/3" % dtype)
        # the serving loop on fixed buffers: recorded at the second call, replayed from the third
        flags = seg.MN_DEBUG_LEAN_EVENTS | seg.MN_DEBUG_REPLAY
        o = seg.default_options(debug_flags=flags, **fast)
        buf = (v0["x"][0].clone(), v0["x"][1].clone())
        out = (torch.empty((H, W), dtype=torch.int32, device="cuda"), torch.empty((H * W,), dtype=torch.int32, device="cuda"))
        want = _yardstick(v0, **fast)
        for i in range(3):
            mask, table, _, st = a.segment_async(buf[0], buf[1], offs, o, out=out, logits=True).result()
            _assert_same(dict(mask=mask.cpu().numpy(), table=table.cpu().numpy(), part=None, stats=st), want, px == px32,
                         "replay/%s/logits call %d" % (dtype, i))
        # the same addresses, options and shape, now holding probabilities of the same element type
        probs = tuple(a.prepare(t, H, W, apply_sigmoid=True, clip=True, out_dtype=t.dtype) for t in v0["x"])
        ptrs = (buf[0].data_ptr(), buf[1].data_ptr())
        buf[0].copy_(probs[0])
        buf[1].copy_(probs[1])
        torch.cuda.synchronize()
        assert ptrs == (buf[0].data_ptr(), buf[1].data_ptr())
        wide = (probs[0].float().contiguous(), probs[1].float().contiguous())
        want = _yardstick(v0, maps=wide, **fast)
        mask, table, _, st = a.segment_async(buf[0], buf[1], offs, o, out=out, logits=False).result()
        _assert_same(dict(mask=mask.cpu().numpy(), table=table.cpu().numpy(), part=None, stats=st), want, px == px32,
                     "replay/%s/probabilities after logits" % dtype)
    finally:
        a.close()
        b.close()


# ---- 6. batch ---------------------------------------------------------------------------------------------

def test_exact_batch_on_logits_equals_the_single_calls():
    vs = [_case("synth", "64x128", "bfloat16", seed=3000), _case("blur", "64x128", "bfloat16"),
          _case("synth", "64x128", "bfloat16", seed=3002)]
    offs = vs[0]["offs"]
    px, px32 = _px(vs[0])
    batch = seg.ExactBatch(64, 128, 9, len(offs), 3)
    try:
        o = seg.default_options(mode=seg.MN_MODE_EXACT)
        res = batch.segment([v["x"][0] for v in vs], [v["x"][1] for v in vs], offs, o, want_partition=True, logits=True)
        for v, r in zip(vs, res):
            _assert_same(_result(r), _yardstick(v, mode=seg.MN_MODE_EXACT), px == px32, "batch/%s" % (v["key"],))
    finally:
        batch.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------

def test_refusals():
    import torch
    v = _case("synth", "64x128", "float16")
    x, p, offs = v["x"], v["p"], v["offs"]
    m = seg.Merger(64, 128, 9, len(offs))
    try:
        with pytest.raises(ValueError):
            m.segment(x[0], x[1].to(torch.bfloat16), offs, logits=True)          # mixed dtypes
        with pytest.raises(ValueError):
            m.segment_async(x[0].float(), x[1], offs, logits=True)
        off = np.ascontiguousarray(np.asarray(offs, dtype=np.int32).reshape(-1, 2))
        mask = torch.empty((64, 128), dtype=torch.int32, device="cuda")
        table = torch.empty((64 * 128,), dtype=torch.int32, device="cuda")
        o = seg.default_options()
        st = seg.MnStats()
        for bad in (seg.MN_MAPS_LOGITS | 7, 7, seg.MN_MAPS_LOGITS << 1, seg.MN_MAPS_LOGITS | 0x80):
            rc = m.lib.mn_segment_device_t(m.handle, x[0].data_ptr(), 9, x[1].data_ptr(), len(offs), bad, 128, 64, 9,
                                           off.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), mask.data_ptr(),
                                           table.data_ptr(), None, ctypes.byref(o), None, ctypes.byref(st))
            assert rc == seg.MN_ERR_ARGUMENT and st.status == seg.MN_ERR_ARGUMENT, bad
        out = torch.empty_like(p[0])
        for in_dt, out_dt in ((seg.MN_DTYPE_F16 | seg.MN_MAPS_LOGITS, seg.MN_DTYPE_F32),
                              (seg.MN_DTYPE_F16, seg.MN_DTYPE_F32 | seg.MN_MAPS_LOGITS)):
            rc = m.lib.mn_prepare_device_t(m.handle, x[0].data_ptr(), in_dt, 9, 64, 128, out.data_ptr(), out_dt, 64, 128,
                                           1, 0, None)
            assert rc == seg.MN_ERR_ARGUMENT, (in_dt, out_dt)
        # the context is still good
        got = _result(m.segment(x[0], x[1], offs, seg.default_options(**MODES["auto"]), want_partition=True, logits=True))
        _assert_same(got, _yardstick(v, **MODES["auto"]), False, "after the refusals")
    finally:
        m.close()
