"""Merger.mask_bce and losses.MaskBCELoss on the device against the numpy statement labels.mask_bce on the same arrays.

Bounds (none of them comes from what the kernel gives; every test prints its greatest figures before it asserts).

Sums.  sums[1 + O], the number of kept pixels, is exact.  Every other sum is within relative 2^-21 + n * 2^-53 of the
statement, n its number of terms.  Per term softplus(z) = fmaxf(z, 0) + log1pf(expf(-|z|)) in float32: expf within
1 ulp; log1pf within 2 ulp, plus the ulp of its argument carried through (log1p is a contraction in relative terms on
(0, 1]); one rounding of the final addition, half an ulp; both summands are non-negative, so the term is within
3.5 ulp <= 3.5 * 2^-23 < 2^-21 of the true term, relative, and a sum of non-negative terms inherits the relative bound
of its terms.  The terms are then added in float64 in some order: n * 2^-53 relative to the correctly rounded sum the
statement gives.  (1 ulp for expf and 2 ulp for log1pf are taken as OCML's bounds, as the feature request assumed them:
a ROCm installation ships no document that states them, so they are an assumption of this derivation, and the bound
was not adjusted to any measured value; the greatest error measured on an MI355X is 3.3e-8, relative, on the
one-pixel image.)  A sum whose statement is 0 must be 0.  The logits lie in -12..12 with a band of columns at +-80, where expf(-80) is still a normal
float32; beyond about +-87 it underflows, outside this bound (mergenet_hip.h).

Gradient.  float32: |g - g_ref| <= 2^-21 * |scale|: the sigmoid is expf, an addition and a division, within 2.5 ulp
absolute of a value <= 1, then one subtraction and one multiplication.  16-bit types: the same plus half an ulp of the
type AT |g_ref|, the rounding to nearest of the store.  That half ulp is taken exactly here: 2^(e - 8) for bfloat16
and 2^(max(e, -14) - 11) for float16 with e = floor(log2 |g_ref|), i.e. 2^-25 in float16's subnormal range and at
zero.  (The feature request glosses it as 2^-9 and 2^-12 relative.  Those are the half ulp at the TOP of a binade; at
the bottom it is 2^-8 and 2^-11 relative, so a correctly rounded store would miss the gloss.  The test holds the kernel to what
the request's words say, half an ulp at |g_ref|, which is never wider than 2^-8 / 2^-11 relative.)
"""
import functools
import math

import numpy as np
import pytest

from mergenet_amd import labels, synth

pytestmark = pytest.mark.gpu

C, G_TRUTH = 9, 7
TRUTH_CLASSES = (3, 1, 8, 255, 2, 1, 5)          # label 4 has class 255: outside 0..C-1, an ignore class
SHAPES = [(1, 1),
          (3, 5),
          (7, 64),       # single elements, one chunk per row
          (33, 257),     # single elements, the last chunk of a row reaches past W
          (48, 256),     # 16-byte accesses: one chunk per row in float32, half a chunk in 16 bits
          (32, 1028),    # W % 8 == 4: four elements per lane in every dtype (8-byte accesses in 16 bits), the last
                         # chunk of a row partly past W
          (64, 1032)]    # eight per lane in 16 bits, four in float32; several chunks per row, more than one per wave
DTYPES = ["float32", "bfloat16", "float16"]
SENTINEL = 77.0                                  # (a value of all three dtypes)
TAIL = 64


def offsets_for(shape):
    H, W = shape
    return synth.generate_offsets(40, 10) + [(-3, 2), (0, -1), (H, 0), (0, W)]      # 14: three groups of offsets


def truth_mask(shape, seed=5):
    """The blobs of test_gpu_map_scores.image: 7 truth labels, a label out of range and a negative one."""
    H, W = shape
    rng = np.random.default_rng(seed + 1000 * H + W)
    truth = np.zeros((H, W), np.int32)
    for k in range(1, G_TRUTH + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        truth[max(0, y - H // 6):y + H // 6 + 1, max(0, x - W // 6):x + W // 6 + 1] = k
    if W > 70:
        truth[H // 2, 60:70] = 5                     # across lanes and across the 64-pixel mark
        truth[H - 1, W - 3:] = G_TRUTH + 4           # out of range: class 0, a label of its own for the offsets
        truth[0, 2] = -7
    truth[H - 1, W - 1] = 1
    return truth


def to_dtype(a, dtype):
    """float32 array holding the values of `a` rounded to `dtype` (what the device tensor of that dtype widens to)."""
    import torch
    return torch.from_numpy(a).to(getattr(torch, dtype)).float().numpy()


@functools.lru_cache(maxsize=None)
def image(shape, dtype="float32", seed=5, num_classes=C):
    """(class logits [C,H,W], offset logits [O,H,W], truth): logits uniform in -12..12, a band of columns at +-80."""
    H, W = shape
    rng = np.random.default_rng(seed + 7 * H + 13 * W)
    cl = (rng.random((num_classes, H, W), dtype=np.float32) * 24 - 12).astype(np.float32)
    sl = (rng.random((len(offsets_for(shape)), H, W), dtype=np.float32) * 24 - 12).astype(np.float32)
    b0, b1 = W // 3, W // 3 + max(1, W // 8)
    for a in (cl, sl):
        a[:, :, b0:b1] = np.where(rng.random(a[:, :, b0:b1].shape) < 0.5, -80.0, 80.0)
    cl, sl = to_dtype(cl, dtype), to_dtype(sl, dtype)
    truth = truth_mask(shape, seed)
    for a in (cl, sl, truth):
        a.setflags(write=False)
    return cl, sl, truth


@functools.lru_cache(maxsize=None)
def statement(shape, dtype="float32", seed=5):
    """labels.mask_bce of image(shape, dtype) with both scales 1 (the gradient of another scale is that times it)."""
    cl, sl, truth = image(shape, dtype, seed)
    res = labels.mask_bce(cl, sl, offsets_for(shape), truth, TRUTH_CLASSES, G_TRUTH)
    for a in res:
        a.setflags(write=False)
    return res


@pytest.fixture(scope="module")
def merger():
    from mergenet_amd import segmenter as seg
    m = seg.Merger(64, 128, 9, 10)
    yield m
    m.close()


def dev(a, dtype=None, shift=0):
    """The array on the device (in `dtype`), `shift` elements behind a 16-byte boundary."""
    import torch
    t = torch.from_numpy(np.array(a, order="C"))
    if dtype is not None:
        t = t.to(getattr(torch, dtype))
    buf = torch.zeros((t.numel() + 16,), dtype=t.dtype, device="cuda")
    view = buf[shift:shift + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (shift * t.element_size()) % 16 and view.is_contiguous()
    return view


def classes(values=TRUTH_CLASSES):
    import torch
    return torch.tensor(values, dtype=torch.int32, device="cuda")


class GradBuffer:
    """A gradient buffer full of NaN, `shift` elements behind a 16-byte boundary, between two runs of a sentinel."""

    def __init__(self, shape, dtype, shift=0):
        import torch
        n = int(np.prod(shape))
        self.lead = 8 + shift if dtype != "float32" else 4 + shift
        self.buf = torch.full((self.lead + n + TAIL,), SENTINEL, dtype=getattr(torch, dtype), device="cuda")
        self.view = self.buf[self.lead:self.lead + n].view(shape)
        self.view.fill_(float("nan"))
        assert self.view.data_ptr() % 16 == (shift * self.buf.element_size()) % 16

    def check_surroundings(self):
        n = self.view.numel()
        assert (self.buf[:self.lead] == SENTINEL).all().item(), "written before the buffer"
        assert (self.buf[self.lead + n:] == SENTINEL).all().item() and self.buf.numel() - self.lead - n == TAIL, \
            "the tail behind the buffer was touched"


def half_ulp(g_ref, dtype):
    """Half an ulp of `dtype` at |g_ref| (float64 array): the rounding to nearest of the store."""
    if dtype == "float32":
        return np.zeros_like(g_ref)                  # (the float32 bound has its rounding inside 2^-21)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(g_ref)))         # (-inf at 0)
    if dtype == "bfloat16":
        return np.where(np.isfinite(e), 2.0 ** (np.maximum(e, -126.0) - 8), 2.0 ** -134)
    return 2.0 ** (np.maximum(e, -14.0) - 11)        # float16: 2^-25 below 2^-14


def check_sums(sums, want, n_class_terms, n_pixels, what):
    assert sums.dtype == np.float64 and sums.shape == want.shape, what
    assert sums[-1] == want[-1], what                                    # the kept pixels: exact
    n = np.full(want.shape[0] - 1, float(n_pixels))
    n[0] = float(n_class_terms)
    bound = 2.0 ** -21 + n * 2.0 ** -53
    err = np.abs(sums[:-1] - want[:-1])
    pos = want[:-1] > 0
    rel = err[pos] / want[:-1][pos]
    print("%s: greatest relative error of a sum %.3g (bound %.3g)" % (what, rel.max() if rel.size else 0.0, bound.min()))
    assert (err <= bound * want[:-1]).all(), what                        # (a sum that is 0 must be exactly 0)


def check_grad(got, g_ref, scale, dtype, what, extra=0.0):
    """`got`: device tensor; `g_ref`: the statement's gradient at this scale (float64)."""
    g = got.float().cpu().numpy().astype(np.float64)
    assert g.shape == g_ref.shape, what
    assert not np.isnan(g).any(), what + ": an element was not written"
    bound = 2.0 ** -21 * abs(scale) + half_ulp(g_ref, dtype) + extra
    err = np.abs(g - g_ref)
    print("%s: greatest gradient error %.3g of its bound" % (what, (err / bound).max() if err.size else 0.0))
    assert (err <= bound).all(), what


def run(merger, shape, dtype, scale_c=1.0, scale_s=1.0, shifts=(0, 0, 0, 0), grad=True, seed=5):
    """One call on image(shape, dtype); shifts: elements behind a 16-byte boundary of the class logits, the offset
    logits, the class gradient and the offset gradient.  Returns (result, the two gradient buffers)."""
    cl, sl, truth = image(shape, dtype, seed)
    bufs = (GradBuffer(cl.shape, dtype, shifts[2]), GradBuffer(sl.shape, dtype, shifts[3])) if grad else None
    res = merger.mask_bce(dev(cl, dtype, shifts[0]), dev(sl, dtype, shifts[1]), offsets_for(shape), dev(truth),
                          classes(), scale_c, scale_s, grad=grad, out=(bufs[0].view, bufs[1].view) if grad else None)
    return res, bufs


def check_run(res, bufs, shape, dtype, scale_c, scale_s, what, seed=5):
    want_sums, gc, gs = statement(shape, dtype, seed)
    truth = image(shape, dtype, seed)[2]
    ignored = truth == 4
    kept = truth.size - int(ignored.sum())
    assert want_sums[-1] == kept
    check_sums(res["sums"].cpu().numpy(), want_sums, kept * C, truth.size, what)
    if bufs is None:
        assert res["grad_class"] is None and res["grad_same"] is None
        return
    assert res["grad_class"] is bufs[0].view and res["grad_same"] is bufs[1].view
    check_grad(bufs[0].view, gc * scale_c, scale_c, dtype, what + ", class gradient")
    check_grad(bufs[1].view, gs * scale_s, scale_s, dtype, what + ", offset gradient")
    if ignored.any():
        assert (bufs[0].view.float().cpu().numpy()[:, ignored] == 0).all(), what + ": ignored pixels hold 0"
    for b in bufs:
        b.check_surroundings()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_and_gradients_equal_the_statement(merger, shape, dtype):
    if shape[0] >= 32:
        assert (image(shape)[2] == 4).any()                              # the ignore class occurs
    for scale_c, scale_s in ((1.0, 1.0 / 64), (1.0 / 64, 1.0)):
        res, bufs = run(merger, shape, dtype, scale_c, scale_s)
        check_run(res, bufs, shape, dtype, scale_c, scale_s, "%s %s" % (shape, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(32, 1028), (64, 1032)])
def test_each_base_off_the_boundary_gives_the_same_sums_bit_for_bit(merger, shape, dtype):
    aligned, bufs = run(merger, shape, dtype, 1.0, 1.0 / 64)
    check_run(aligned, bufs, shape, dtype, 1.0, 1.0 / 64, "aligned")
    want = aligned["sums"].cpu().numpy().tobytes()
    for which in range(4):
        shifts = tuple(1 if i == which else 0 for i in range(4))
        res, bufs = run(merger, shape, dtype, 1.0, 1.0 / 64, shifts=shifts)
        assert res["sums"].cpu().numpy().tobytes() == want, "base %d one element off: other sums" % which
        check_run(res, bufs, shape, dtype, 1.0, 1.0 / 64, "base %d one element off" % which)


@pytest.mark.parametrize("shape,dtype", [((3, 5), "float32"),          # single elements
                                         ((9, 260), "bfloat16")])       # W % 8 == 4: four pixels per lane
def test_offsets_beyond_the_image_have_target_one_everywhere(merger, shape, dtype):
    """(0, 1), then five offsets that leave the image whatever the pixel: by exactly H rows or W columns, by one more,
    and by the ends of the int32 range (the entry point holds each to -H..H / -W..W)."""
    H, W = shape
    offs = [(0, 1), (H, 0), (0, -W), (H + 1, 0), (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)]
    cl, sl, truth = image(shape, dtype)
    sl = sl[:len(offs)]
    want_sums, gc, gs = labels.mask_bce(cl, sl, offs, truth, TRUTH_CLASSES, G_TRUTH)
    different = [labels._different(truth.astype(np.int64), di, dj) for di, dj in offs]
    assert different[0].any() and not any(d.any() for d in different[1:])
    bufs = (GradBuffer(cl.shape, dtype), GradBuffer(sl.shape, dtype))
    res = merger.mask_bce(dev(cl, dtype), dev(sl, dtype), offs, dev(truth), classes(), 1.0, 1.0,
                          out=(bufs[0].view, bufs[1].view))
    what = "%s %s" % (shape, dtype)
    check_sums(res["sums"].cpu().numpy(), want_sums, int(want_sums[-1]) * C, truth.size, what)
    check_grad(bufs[0].view, gc, 1.0, dtype, what + ", class gradient")
    check_grad(bufs[1].view, gs, 1.0, dtype, what + ", offset gradient")
    # target 1 everywhere: the gradient sigmoid(x) - 1 is never above 0 (a target of 0 gives sigmoid(x) > 0, also at
    # x = -80), and the term is softplus(-x)
    g = bufs[1].view.float().cpu().numpy()
    assert (g[1:] <= 0).all() and (g[0][different[0]] > 0).all()
    for b in bufs:
        b.check_surroundings()


@pytest.mark.parametrize("dtype", DTYPES)
def test_parts_may_be_absent(merger, dtype):
    import torch
    shape = (33, 257) if dtype == "float32" else (32, 1028)
    cl, sl, truth = image(shape, dtype)
    offs = offsets_for(shape)
    want_sums, gc, gs = statement(shape, dtype)
    O, n = len(offs), truth.size
    kept = int(want_sums[-1])
    d_cl, d_sl, d_truth = dev(cl, dtype), dev(sl, dtype), dev(truth)
    # no class planes (offset-only training): None, or a tensor without planes
    for none in (None, torch.empty((0,) + shape, dtype=d_sl.dtype, device="cuda")):
        res = merger.mask_bce(none, d_sl, offs, d_truth, classes(), 1.0, 1.0)
        want = labels.mask_bce(None, sl, offs, truth, TRUTH_CLASSES, G_TRUTH)[0]
        assert want[0] == 0.0 and want[-1] == 0.0 and np.array_equal(want[1:-1], want_sums[1:-1])
        check_sums(res["sums"].cpu().numpy(), want, 0, n, "C == 0")
        assert res["grad_class"] is None
        check_grad(res["grad_same"], gs, 1.0, dtype, "C == 0, offset gradient")
    # no offset planes (class-only training)
    res = merger.mask_bce(d_cl, None, [], d_truth, classes(), 1.0 / 64, 1.0)
    want = np.array([want_sums[0], want_sums[-1]])
    check_sums(res["sums"].cpu().numpy(), want, kept * C, n, "O == 0")
    assert res["grad_same"] is None and tuple(res["sums"].shape) == (2,)
    check_grad(res["grad_class"], gc / 64, 1.0 / 64, dtype, "O == 0, class gradient")
    # no truth instances: every pixel is class 0, the offsets look at the labels as they stand
    res = merger.mask_bce(d_cl, d_sl, offs, d_truth, None, 1.0, 1.0)
    want, gc0, gs0 = labels.mask_bce(cl, sl, offs, truth, None, 0)
    assert want[-1] == n and np.array_equal(gs0, gs)
    check_sums(res["sums"].cpu().numpy(), want, n * C, n, "G == 0")
    check_grad(res["grad_class"], gc0, 1.0, dtype, "G == 0, class gradient")
    check_grad(res["grad_same"], gs0, 1.0, dtype, "G == 0, offset gradient")


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_gradient_the_sums_are_the_same_bits(merger, dtype):
    shape = (64, 1032)
    with_grad, bufs = run(merger, shape, dtype)
    without, none = run(merger, shape, dtype, grad=False)
    check_run(without, none, shape, dtype, 1.0, 1.0, "no gradient")
    assert without["sums"].cpu().numpy().tobytes() == with_grad["sums"].cpu().numpy().tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_give_byte_identical_results(merger, dtype):
    shape = (64, 1032)
    a, bufs_a = run(merger, shape, dtype, 1.0 / 64, 1.0)
    b, bufs_b = run(merger, shape, dtype, 1.0 / 64, 1.0)
    assert a["sums"].cpu().numpy().tobytes() == b["sums"].cpu().numpy().tobytes()
    import torch
    for x, y in zip(bufs_a, bufs_b):
        assert torch.equal(x.view.view(torch.int16 if dtype != "float32" else torch.int32),
                           y.view.view(torch.int16 if dtype != "float32" else torch.int32))


def test_into_accumulates_the_totals(merger):
    import torch
    shape = (32, 1028)
    a, _ = run(merger, shape, "float32")
    b, _ = run(merger, shape, "float32", seed=6)
    assert not torch.equal(a["sums"], b["sums"])
    total = {"sums": a["sums"].clone()}
    cl, sl, truth = image(shape, "float32", 6)
    back = merger.mask_bce(dev(cl), dev(sl), offsets_for(shape), dev(truth), classes(), grad=False, into=total)
    assert back["sums"] is total["sums"]
    assert torch.equal(total["sums"], a["sums"] + b["sums"])             # one IEEE addition per total
    plain = a["sums"].clone()                                            # the tensor itself is accepted as well
    merger.mask_bce(dev(cl), dev(sl), offsets_for(shape), dev(truth), classes(), grad=False, into=plain)
    assert torch.equal(plain, total["sums"])


def test_bad_arguments_raise_and_launch_nothing(merger):
    import ctypes
    import torch
    from mergenet_amd import segmenter as seg
    shape = (7, 64)
    H, W = shape
    cl, sl, truth = image(shape)
    offs = offsets_for(shape)
    O = len(offs)
    d_cl, d_sl, d_truth, d_classes = dev(cl), dev(sl), dev(truth), classes()
    sums = torch.full((2 + O,), SENTINEL, dtype=torch.float64, device="cuda")
    gbufs = (GradBuffer(cl.shape, "float32"), GradBuffer(sl.shape, "float32"))
    off = np.ascontiguousarray(np.asarray(offs, np.int32))
    stream = torch.cuda.current_stream().cuda_stream

    def raw(**over):
        """The entry point itself on a good call with some arguments replaced: its status."""
        a = dict(ctx=merger.handle, cls=d_cl.data_ptr(), same=d_sl.data_ptr(), dtype=seg.MN_DTYPE_F32, width=W, height=H,
                 num_classes=C, offset_dim=O, offsets=off.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                 truth=d_truth.data_ptr(), num_truth=G_TRUTH, truth_classes=d_classes.data_ptr(),
                 gcls=gbufs[0].view.data_ptr(), gsame=gbufs[1].view.data_ptr(), scale_class=1.0, scale_same=1.0,
                 sums=sums.data_ptr(), accumulate=0, stream=ctypes.c_void_p(stream))
        assert set(over) <= set(a)
        a.update(over)
        return merger.lib.mn_mask_bce_device(*a.values())

    bad = [dict(ctx=None), dict(cls=None), dict(same=None), dict(offsets=None), dict(truth=None),
           dict(truth_classes=None), dict(sums=None),                                         # pointers that are needed
           dict(width=0), dict(height=-1), dict(num_classes=-1), dict(num_classes=128), dict(offset_dim=-1),
           dict(offset_dim=33), dict(num_truth=-1), dict(num_classes=0, offset_dim=0),        # sizes and counts
           dict(height=1 << 16, width=1 << 15),                                               # height * width = 2^31
           dict(height=1, width=(1 << 30) + 8),                                               # width > 2^30
           dict(dtype=3), dict(dtype=-1), dict(dtype=seg.MN_DTYPE_F32 | seg.MN_MAPS_LOGITS),  # dtypes
           dict(scale_class=float("nan")), dict(scale_same=float("inf")), dict(scale_class=float("-inf"))]
    for over in bad:
        assert raw(**over) == seg.MN_ERR_ARGUMENT, over
        assert merger.lib.mn_last_status() == seg.MN_ERR_ARGUMENT
    # through the wrapper: what it hands on to the entry point comes back as MergeNetError
    for kwargs in (dict(scale_class=float("nan")), dict(scale_same=float("inf"))):
        with pytest.raises(seg.MergeNetError):
            merger.mask_bce(d_cl, d_sl, offs, d_truth, d_classes, out=(gbufs[0].view, gbufs[1].view), into=sums, **kwargs)
    with pytest.raises(seg.MergeNetError):
        merger.mask_bce(torch.zeros((128, H, W), device="cuda"), d_sl, offs, d_truth, d_classes, grad=False, into=sums)
    with pytest.raises(seg.MergeNetError):
        merger.mask_bce(None, None, [], d_truth, d_classes, grad=False)
    # what the wrapper refuses itself
    with pytest.raises(ValueError):
        merger.mask_bce(d_cl.cpu(), d_sl, offs, d_truth, d_classes)
    with pytest.raises(ValueError):
        merger.mask_bce(d_cl, d_sl.half(), offs, d_truth, d_classes)
    with pytest.raises(ValueError):
        merger.mask_bce(d_cl.double(), d_sl.double(), offs, d_truth, d_classes)
    with pytest.raises(ValueError):
        merger.mask_bce(d_cl, d_sl, offs[:3], d_truth, d_classes)
    with pytest.raises(ValueError):
        merger.mask_bce(d_cl, d_sl, offs, d_truth.long(), d_classes)
    with pytest.raises(ValueError):
        merger.mask_bce(d_cl, d_sl, offs, d_truth, d_classes, out=(gbufs[0].view, gbufs[1].view.half()))
    with pytest.raises(ValueError):
        merger.mask_bce(d_cl, d_sl, offs, d_truth, d_classes, into=sums[:3])
    torch.cuda.synchronize()
    assert (sums == SENTINEL).all().item()                               # nothing ran
    for b in gbufs:
        assert torch.isnan(b.view).all().item()
        b.check_surroundings()
    assert raw() == 0                                                    # and the good call still does
    res = {"sums": sums, "grad_class": gbufs[0].view, "grad_same": gbufs[1].view}
    check_run(res, gbufs, shape, "float32", 1.0, 1.0, "after the refusals")


# ---- the module --------------------------------------------------------------------------------------------------

MOD_SHAPE, MOD_O, ALPHA = (24, 136), 10, 0.5


@functools.lru_cache(maxsize=None)
def batch(dtype):
    """prediction [2, 9 + 10, 24, 136] (values of `dtype`), truth [2, 24, 136], the statement of each image at the
    mean's scales, and the loss they give."""
    H, W = MOD_SHAPE
    offs = synth.generate_offsets(40, MOD_O)
    rng = np.random.default_rng(11)
    pred = to_dtype((rng.random((2, C + MOD_O, H, W), dtype=np.float32) * 24 - 12).astype(np.float32), dtype)
    truth = np.stack([truth_mask(MOD_SHAPE, 5), truth_mask(MOD_SHAPE, 6)])
    assert not np.array_equal(truth[0], truth[1])
    tcs = [TRUTH_CLASSES, (1, 2, 3, 4, 5, 6, 7)]
    sc, ss = 1.0 / (2 * C * H * W), ALPHA / (2 * MOD_O * H * W)
    parts = [labels.mask_bce(pred[b, :C], pred[b, C:], offs, truth[b], tcs[b], G_TRUTH, sc, ss) for b in range(2)]
    sums = parts[0][0] + parts[1][0]
    grad = np.stack([np.concatenate([p[1], p[2]]) for p in parts])
    loss_cls, loss_ofs = sums[0] * sc, sums[1:1 + MOD_O].sum() * ss
    return pred, truth, tcs, offs, sums, grad, (loss_cls, loss_ofs), (sc, ss)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_module_loss_and_backward(merger, dtype):
    import torch
    from mergenet_amd import losses
    pred, truth, tcs, offs, want_sums, want_grad, (loss_cls, loss_ofs), (sc, ss) = batch(dtype)
    H, W = MOD_SHAPE
    crit = losses.MaskBCELoss(merger, C, offs, alpha=ALPHA)
    d_truth = dev(truth)
    d_tcs = [classes(t) for t in tcs]
    want_loss = loss_cls + loss_ofs
    n_terms = 2 * C * H * W
    loss_bound = (2.0 ** -21 + n_terms * 2.0 ** -53) * want_loss + 2.0 ** -24 * want_loss
    scale = np.concatenate([np.full(C, sc), np.full(MOD_O, ss)])[None, :, None, None]
    values = []
    for factor in (1.0, 3.0):
        x = dev(pred, dtype).requires_grad_()
        loss = crit(x, d_truth, d_tcs)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad and loss.is_cuda
        assert crit.last_sums.dtype == torch.float64 and tuple(crit.last_sums.shape) == (2 + MOD_O,)
        assert crit.last_sums[-1].item() == want_sums[-1]
        (factor * loss).backward()
        print("%s: loss %.9g, statement %.17g (bound %.3g)" % (dtype, loss.item(), want_loss, loss_bound))
        assert abs(float(loss.item()) - want_loss) <= loss_bound
        values.append(loss.item())
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
        g = x.grad.float().cpu().numpy().astype(np.float64)
        ref = want_grad * factor
        # the pass's gradient within its bound (times the factor), then ONE rounding of the multiplication
        first = 2.0 ** -21 * scale + half_ulp(want_grad, dtype)
        bound = factor * first + (half_ulp(ref, dtype) if dtype != "float32" else 2.0 ** -24 * np.abs(ref))
        err = np.abs(g - ref)
        print("%s, times %g: greatest gradient error %.3g of its bound" % (dtype, factor, (err / bound).max()))
        assert (err <= bound).all()
    assert values[0] == values[1]

    # forward only: no gradient buffer, the same value
    calls = []
    inner = merger.mask_bce

    def spy(*args, **kwargs):
        calls.append(kwargs)
        return inner(*args, **kwargs)

    merger.mask_bce = spy
    try:
        with torch.no_grad():
            quiet = crit(dev(pred, dtype).requires_grad_(), d_truth, d_tcs)
        plain = crit(dev(pred, dtype), d_truth, d_tcs)               # requires_grad=False
    finally:
        del merger.mask_bce
    assert len(calls) == 4 and all(k["grad"] is False and k["out"] is None for k in calls)
    assert not quiet.requires_grad and not plain.requires_grad
    assert quiet.item() == values[0] and plain.item() == values[0]
    assert np.array_equal(crit.last_sums.cpu().numpy()[1:1 + MOD_O] > 0, np.ones(MOD_O, bool))


def test_module_equals_torch_bce_with_logits(merger):
    """The module against the criterion it replaces, on the device in float64 (no ignore class: the two are the
    same function).  Both carry float32 / float64 rounding only: the loss bound above, and the gradient bound."""
    import torch
    from mergenet_amd import losses
    pred, truth, tcs, offs, *_ = batch("float32")
    H, W = MOD_SHAPE
    tc = (1, 2, 3, 4, 5, 6, 7)
    crit = losses.MaskBCELoss(merger, C, offs, alpha=ALPHA)
    x = dev(pred).requires_grad_()
    d_truth = dev(truth)
    loss = crit(x, d_truth, [classes(tc), classes(tc)])
    loss.backward()
    y = dev(pred).double().requires_grad_()
    by_label = torch.tensor((0,) + tc, device="cuda")
    cls_t = torch.stack([(by_label[d_truth.long().clamp(0, G_TRUTH) * ((d_truth >= 0) & (d_truth <= G_TRUTH))] == q)
                         for q in range(C)], 1).double()
    ofs_t = torch.stack([merger.sameness_targets(d_truth[b], offs) for b in range(2)]).double()
    bce = torch.nn.BCEWithLogitsLoss()
    want = bce(y[:, :C], cls_t) + ALPHA * bce(y[:, C:], ofs_t)
    want.backward()
    n_terms = 2 * C * H * W
    bound = (2.0 ** -21 + n_terms * 2.0 ** -53 + 2.0 ** -24) * want.item()
    print("module %.9g, torch float64 %.17g (bound %.3g)" % (loss.item(), want.item(), bound))
    assert abs(loss.item() - want.item()) <= bound
    sc, ss = 1.0 / (2 * C * H * W), ALPHA / (2 * MOD_O * H * W)
    scale = torch.tensor([sc] * C + [ss] * MOD_O, device="cuda", dtype=torch.float64)[None, :, None, None]
    assert ((x.grad.double() - y.grad).abs() <= 2.0 ** -21 * scale).all().item()
