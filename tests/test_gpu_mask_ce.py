"""Merger.mask_ce and losses.MaskCELoss on the device against the numpy statement labels.mask_ce on the same arrays.

The float32 arithmetic of a pixel (mn_kernels_celoss.h), P planes, each operation rounded:
    m = max_q x_q, a = the first q with x_q == m;  e_q = expf(x_q - m) for q != a, e_a = 1;
    r = sum of e_q, q != a, ascending q;  term = log1pf(r) + (m - x_target);
    p_q = e_q * (1 / (1 + r));  g_q = (p_q - [q == target]) * scale.

Bounds (none of them comes from what the kernel gives; every check prints its greatest figures before it asserts).
u = 2^-24, half an ulp of float32 relative; OCML's expf is taken within 1 ulp = 2 u and log1pf within 2 ulp = 4 u, the
assumption tests/test_gpu_mask_bce.py states.  D is the greatest m - x_q of the input, capped at 88: beyond that
e_q < 2^-126.

Sum.  sums[1], the number of kept pixels, is exact.  sums[0] is within relative (D + P + 5) u + n 2^-53 of the
statement, n its number of terms, plus an absolute n P 2^-126.  Per term, to first order in u: the rounding of
x_q - m is at most D u absolute, which expf turns into D u relative; expf adds 2 u: e_q is within (D + 2) u.  The
P - 2 additions of r add one u each, relative to a partial sum of non-negative values that is at most r: r is within
(D + P) u.  log1p is a contraction in relative terms for r >= 0 (r / ((1 + r) log1p(r)) <= 1), log1pf adds 4 u: the
first summand is within (D + P + 4) u.  The second summand m - x_target is one rounding, u.  Both are >= 0, so their
sum is within the greater of the two, and the final addition adds u: (D + P + 5) u.  An e_q below the normal range
(0 or a subnormal, whichever expf returns) is off by at most 2^-126 absolute, P of them per term at most, and log1p
does not stretch an absolute error: n P 2^-126.  A sum of non-negative terms inherits the relative bound of its
terms; adding them in float64 in some order costs n 2^-53 relative to the correctly rounded sum of the statement.
A sum whose statement is 0 (one plane) must be 0 up to that allowance.

Gradient.  |g - g_ref| <= (2 D + P + 12) u |scale| + half an ulp of the store's dtype at |g_ref| (half_ulp of the BCE
test; float32 stores exactly) + P 2^-126 |scale|.  e_q is within (D + 2) u; 1 + r within (D + P) u for r and one more
for the addition, relative to 1 + r; a division, or a reciprocal and a product, within 2.5 ulp = 5 u: p_q <= 1 is
within (2 D + P + 8) u absolute.  The subtraction of the one-hot and the product with the scale are one rounding each
of a value of at most 1: (2 D + P + 10) u, inside the (2 D + P + 12) u of the feature request.  An ignored pixel holds
exactly 0 on every plane.
"""
import functools

import numpy as np
import pytest

import test_gpu_mask_bce as bce
from mergenet_amd import labels
from test_gpu_mask_bce import (G_TRUTH, SENTINEL, SHAPES, TRUTH_CLASSES, GradBuffer, classes, dev, half_ulp, merger,  # noqa: F401
                               to_dtype)

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "bfloat16", "float16"]
SMALL = [s for s in SHAPES if s[0] * s[1] <= 33 * 257]
# class part: 1, 2, 9; the bounds 4, 10, 20 of the resident form's buckets and the counts just above them -- 21 is the
# first count of the streaming form --; COCO's 81; MN_MAX_CLASSES.  Offset part: 10, 14, MN_MAX_OFFSETS.
CLASS_COUNTS = [1, 2, 4, 5, 9, 10, 11, 20, 21, 81, 127]
OFFSET_COUNTS = [10, 14, 32]
PARTS = [("class", p) for p in CLASS_COUNTS] + [("offset", p) for p in OFFSET_COUNTS]
CASES = [(s, part, p) for s in SHAPES for part, p in PARTS if p <= 19 or s in SMALL]     # (the larger counts at the small shapes)
U = 2.0 ** -24


def offsets_for(shape, count):
    """14: the list of the BCE test, with offsets of H rows and W columns; 10: its first nine and (-3, 2), all short,
    so that a pixel can have NO plane with target 1; 32: eighteen more in front."""
    full = bce.offsets_for(shape)
    if count == 14:
        return full
    if count == 10:
        return full[:9] + [full[10]]
    assert count == 32
    return [(1 + i // 3, (i % 7) - 3) for i in range(18)] + full


def truth_mask(shape):
    """The blobs of the BCE test, and one pixel with a label of its own that has every short offset's neighbour inside
    the image."""
    H, W = shape
    truth = bce.truth_mask(shape).copy()
    if H >= 32:
        truth[H // 4, W // 2 + 3] = 6
    return truth


@functools.lru_cache(maxsize=6)
def image(shape, dtype, part, count, seed=5):
    """(logits [P,H,W] float32 holding values of `dtype`, truth, offsets or None): logits uniform in -12..12, a band of
    columns at +-80 -- ties for the maximum, and differences of 160, where expf underflows."""
    H, W = shape
    rng = np.random.default_rng(seed + 7 * H + 13 * W + 1009 * count)
    x = (rng.random((count, H, W), dtype=np.float32) * 24 - 12).astype(np.float32)
    b0, b1 = W // 3, W // 3 + max(1, W // 8)
    x[:, :, b0:b1] = np.where(rng.random(x[:, :, b0:b1].shape) < 0.5, -80.0, 80.0)
    x = to_dtype(x, dtype)
    truth = truth_mask(shape) if seed == 5 else bce.truth_mask(shape, seed)
    for a in (x, truth):
        a.setflags(write=False)
    return x, truth, (offsets_for(shape, count) if part == "offset" else None)


@functools.lru_cache(maxsize=6)
def statement(shape, dtype, part, count, seed=5):
    """labels.mask_ce of image(...) at scale 1, the kept pixels, and D."""
    x, truth, offs = image(shape, dtype, part, count, seed)
    sums, grad = labels.mask_ce(x, part, offs, truth, TRUTH_CLASSES, G_TRUTH)
    keep = labels.ce_targets(part, count, offs, truth, TRUTH_CLASSES, G_TRUTH)[1]
    D = min(88.0, float((x.max(axis=0) - x.min(axis=0)).max()))
    for a in (sums, grad, keep):
        a.setflags(write=False)
    return sums, grad, keep, D


def check_sums(sums, case, what):
    want, _, keep, D = statement(*case)
    P = case[3]
    assert sums.dtype == np.float64 and sums.shape == (2,), what
    assert sums[1] == want[1] == keep.sum(), what                        # the kept pixels: exact
    n = float(want[1])
    bound = ((D + P + 5) * U + n * 2.0 ** -53) * want[0] + n * P * 2.0 ** -126
    err = abs(sums[0] - want[0])
    print("%s: sum %.17g, statement %.17g, error %.3g of its bound %.3g" % (what, sums[0], want[0], err / bound if bound else err, bound))
    assert err <= bound, what


def check_grad(got, case, scale, what):
    """`got`: device tensor; the statement's gradient is linear in the scale."""
    _, g1, keep, D = statement(*case)
    dtype, P = case[1], case[3]
    g_ref = g1 * scale
    g = got.float().cpu().numpy().astype(np.float64)
    assert g.shape == g_ref.shape, what
    assert not np.isnan(g).any(), what + ": an element was not written"
    bound = (2 * D + P + 12) * U * abs(scale) + half_ulp(g_ref, dtype) + P * 2.0 ** -126 * abs(scale)
    err = np.abs(g - g_ref)
    print("%s: greatest gradient error %.3g of its bound" % (what, (err / bound).max() if err.size else 0.0))
    assert (err <= bound).all(), what
    assert (g[:, ~keep] == 0).all(), what + ": ignored pixels hold 0 on every plane"


def run(merger, case, scale=1.0, shifts=(0, 0), grad=True, into=None):
    """One call on image(*case); shifts: elements behind a 16-byte boundary of the logits and of the gradient."""
    shape, dtype, part, count = case[:4]
    x, truth, offs = image(*case)
    buf = GradBuffer(x.shape, dtype, shifts[1]) if grad else None
    res = merger.mask_ce(dev(x, dtype, shifts[0]), part, offs, dev(truth), classes(), scale, grad=grad, into=into,
                         out=buf.view if grad else None)
    return res, buf


def check_run(res, buf, case, scale, what):
    check_sums(res["sums"].cpu().numpy(), case, what)
    if buf is None:
        assert res["grad"] is None
        return
    assert res["grad"] is buf.view
    check_grad(buf.view, case, scale, what)
    buf.check_surroundings()


def bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,part,count", CASES)
def test_sums_and_gradients_equal_the_statement(merger, shape, part, count, dtype):
    case = (shape, dtype, part, count)
    x, truth, offs = image(*case)
    if part == "class" and shape[0] >= 32:
        assert not statement(*case)[2].all()                             # the ignore class occurs
    if part == "offset" and shape[0] >= 32:
        y = labels.plane_targets(part, count, offs, truth, None, 0)[0]
        assert (~y.any(axis=0)).any() == (count == 10)                   # a pixel without a target-1 plane
        assert len(np.unique(labels.ce_targets(part, count, offs, truth, None, 0)[0])) >= 3
    for scale in (1.0, 1.0 / 64):
        res, buf = run(merger, case, scale)
        check_run(res, buf, case, scale, "%s %s %s %d, scale %g" % (shape, dtype, part, count, scale))


ALIGN_CASES = [((32, 1028), "class", 9), ((64, 1032), "class", 10), ((64, 1032), "class", 11), ((32, 1028), "offset", 14),
               ((64, 1032), "offset", 10), ((7, 64), "class", 20), ((7, 64), "class", 21), ((7, 64), "class", 81),
               ((7, 64), "offset", 32)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,part,count", ALIGN_CASES)
def test_each_base_off_the_boundary_gives_the_same_sums_bit_for_bit(merger, shape, part, count, dtype):
    case = (shape, dtype, part, count)
    aligned, buf = run(merger, case, 1.0 / 64)
    check_run(aligned, buf, case, 1.0 / 64, "aligned")
    want = bits(aligned["sums"])
    for shifts in ((1, 0), (0, 1), (1, 1)):
        res, buf = run(merger, case, 1.0 / 64, shifts=shifts)
        assert bits(res["sums"]) == want, "bases %s elements off: other sums" % (shifts,)
        check_run(res, buf, case, 1.0 / 64, "bases %s elements off" % (shifts,))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,part,count", [((64, 1032), "class", 9), ((64, 1032), "offset", 10), ((33, 257), "class", 81),
                                              ((7, 64), "class", 21)])
def test_without_gradient_and_twice(merger, shape, part, count, dtype):
    """Without a gradient the sums are the same bits; two calls give byte-identical sums and gradients."""
    import torch
    case = (shape, dtype, part, count)
    a, buf_a = run(merger, case, 1.0 / 64)
    b, buf_b = run(merger, case, 1.0 / 64)
    without, none = run(merger, case, 1.0 / 64, grad=False)
    check_run(without, none, case, 1.0 / 64, "no gradient")
    assert bits(without["sums"]) == bits(a["sums"]) == bits(b["sums"])
    as_int = torch.int16 if dtype != "float32" else torch.int32
    assert torch.equal(buf_a.view.view(as_int), buf_b.view.view(as_int))


def test_into_accumulates_the_totals(merger):
    import torch
    for part, count in (("class", 9), ("offset", 10), ("class", 81)):
        shape = (32, 1028) if count < 20 else (33, 257)
        a, _ = run(merger, (shape, "float32", part, count), grad=False)
        b, _ = run(merger, (shape, "float32", part, count, 6), grad=False)
        assert not torch.equal(a["sums"], b["sums"])
        total = {"sums": a["sums"].clone()}
        back, _ = run(merger, (shape, "float32", part, count, 6), grad=False, into=total)
        assert back["sums"] is total["sums"]
        assert torch.equal(total["sums"], a["sums"] + b["sums"])         # one IEEE addition per total
        plain = a["sums"].clone()                                        # the tensor itself is accepted as well
        run(merger, (shape, "float32", part, count, 6), into=plain)
        assert torch.equal(plain, total["sums"])


def test_bad_arguments_raise_and_launch_nothing(merger):
    import ctypes
    import torch
    from mergenet_amd import segmenter as seg
    shape, P = (7, 64), 14
    H, W = shape
    case = (shape, "float32", "offset", P)
    x, truth, offs = image(*case)
    d_x, d_truth, d_classes = dev(x), dev(truth), classes()
    sums = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
    gbuf = GradBuffer(x.shape, "float32")
    off = np.ascontiguousarray(np.asarray(offs, np.int32))
    stream = torch.cuda.current_stream().cuda_stream

    def raw(**over):
        """The entry point itself on a good call with some arguments replaced: its status."""
        a = dict(ctx=merger.handle, logits=d_x.data_ptr(), dtype=seg.MN_DTYPE_F32, width=W, height=H,
                 part=seg.MN_PART_OFFSET, planes=P, offsets=off.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                 truth=d_truth.data_ptr(), num_truth=G_TRUTH, truth_classes=d_classes.data_ptr(),
                 grad=gbuf.view.data_ptr(), scale=1.0, sums=sums.data_ptr(), accumulate=0, stream=ctypes.c_void_p(stream))
        assert set(over) <= set(a)
        a.update(over)
        return merger.lib.mn_mask_ce_device(*a.values())

    bad = [dict(ctx=None), dict(logits=None), dict(offsets=None), dict(truth=None), dict(sums=None),
           dict(part=seg.MN_PART_CLASS, truth_classes=None),                                  # pointers that are needed
           dict(width=0), dict(height=-1), dict(planes=0), dict(planes=-1), dict(planes=33),
           dict(part=seg.MN_PART_CLASS, planes=128), dict(num_truth=-1), dict(part=2), dict(part=-1),   # sizes, counts
           dict(height=1 << 16, width=1 << 15),                                               # height * width = 2^31
           dict(height=1, width=(1 << 30) + 8),                                               # width > 2^30
           dict(dtype=3), dict(dtype=-1), dict(dtype=seg.MN_DTYPE_F32 | seg.MN_MAPS_LOGITS),  # dtypes
           dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=float("-inf"))]
    for over in bad:
        assert raw(**over) == seg.MN_ERR_ARGUMENT, over
        assert merger.lib.mn_last_status() == seg.MN_ERR_ARGUMENT
    # through the wrapper: what it hands on to the entry point comes back as MergeNetError
    with pytest.raises(seg.MergeNetError):
        merger.mask_ce(d_x, "offset", offs, d_truth, None, scale=float("nan"), out=gbuf.view, into=sums)
    with pytest.raises(seg.MergeNetError):
        merger.mask_ce(torch.zeros((128, H, W), device="cuda"), "class", None, d_truth, d_classes, grad=False, into=sums)
    with pytest.raises(seg.MergeNetError):
        merger.mask_ce(torch.zeros((33, H, W), device="cuda"), "offset", [(0, 1)] * 33, d_truth, None, grad=False, into=sums)
    # what the wrapper refuses itself: device, dtype, rank, strides, the offsets, the truth, out and into
    for call in (lambda: merger.mask_ce(d_x.cpu(), "offset", offs, d_truth, None),
                 lambda: merger.mask_ce(d_x.double(), "offset", offs, d_truth, None),
                 lambda: merger.mask_ce(d_x[None], "offset", offs, d_truth, None),
                 lambda: merger.mask_ce(d_x.transpose(1, 2), "offset", offs, d_truth.t(), None),
                 lambda: merger.mask_ce(d_x[:, :, ::2], "offset", offs, d_truth[:, ::2].contiguous(), None),
                 lambda: merger.mask_ce(d_x, "offset", offs[:3], d_truth, None),
                 lambda: merger.mask_ce(d_x, "both", offs, d_truth, None),
                 lambda: merger.mask_ce(d_x, "class", None, d_truth.long(), d_classes),
                 lambda: merger.mask_ce(d_x, "class", None, d_truth, d_classes.long()),
                 lambda: merger.mask_ce(d_x, "offset", offs, d_truth, None, out=gbuf.view.half()),
                 lambda: merger.mask_ce(d_x, "offset", offs, d_truth, None, out=gbuf.view[:3]),
                 lambda: merger.mask_ce(d_x, "offset", offs, d_truth, None, grad=False, out=gbuf.view),
                 lambda: merger.mask_ce(d_x, "offset", offs, d_truth, None, into=sums[:1]),
                 lambda: merger.mask_ce(d_x, "offset", offs, d_truth, None, into=sums.float())):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert (sums == SENTINEL).all().item()                               # nothing ran
    assert torch.isnan(gbuf.view).all().item()
    gbuf.check_surroundings()
    assert raw() == 0                                                    # and the good call still does
    check_run({"sums": sums, "grad": gbuf.view}, gbuf, case, 1.0, "after the refusals")


# ---- the module --------------------------------------------------------------------------------------------------

MOD_SHAPE, MOD_C, MOD_O = (24, 136), 9, 10


@functools.lru_cache(maxsize=None)
def batch(dtype, part, in_range=False):
    """prediction [2, P, 24, 136] (values of `dtype`), truth [2, 24, 136], the classes of each image's labels, the
    statement's sums and gradient at the mean's scale, D."""
    from mergenet_amd import synth
    H, W = MOD_SHAPE
    P = MOD_C if part == "class" else MOD_O
    offs = synth.generate_offsets(40, MOD_O)[:9] + [(-3, 2)] if part == "offset" else None
    rng = np.random.default_rng(11 + P)
    pred = to_dtype((rng.random((2, P, H, W), dtype=np.float32) * 24 - 12).astype(np.float32), dtype)
    truth = np.stack([bce.truth_mask(MOD_SHAPE, 5), bce.truth_mask(MOD_SHAPE, 6)])
    assert not np.array_equal(truth[0], truth[1])
    tcs = [(3, 1, 8, 4, 2, 1, 5) if in_range else TRUTH_CLASSES, (1, 2, 3, 4, 5, 6, 7)]
    scale = 1.0 / (2 * H * W)
    parts = [labels.mask_ce(pred[b], part, offs, truth[b], tcs[b], G_TRUTH, scale) for b in range(2)]
    D = min(88.0, float((pred.max(axis=1) - pred.min(axis=1)).max()))
    return pred, truth, tcs, offs, parts[0][0] + parts[1][0], np.stack([p[1] for p in parts]), scale, D


@pytest.mark.parametrize("part", ["class", "offset"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_module_loss_and_backward(merger, dtype, part):
    import torch
    from mergenet_amd import losses
    pred, truth, tcs, offs, want_sums, want_grad, scale, D = batch(dtype, part)
    P = pred.shape[1]
    crit = losses.MaskCELoss(merger, part, offs)
    d_truth = dev(truth)
    d_tcs = [classes(t) for t in tcs]
    if part == "class":
        assert want_sums[1] < truth.size                                 # the ignore class occurs
    want_loss = want_sums[0] * scale
    n = float(want_sums[1])
    # the sum's bound, times the scale, then one rounding to float32
    loss_bound = (((D + P + 5) * U + n * 2.0 ** -53) * want_sums[0] + n * P * 2.0 ** -126) * scale + U * want_loss
    values = []
    for factor in (1.0, 3.0):
        x = dev(pred, dtype).requires_grad_()
        loss = crit(x, d_truth, d_tcs)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad and loss.is_cuda
        assert crit.last_sums.dtype == torch.float64 and tuple(crit.last_sums.shape) == (2,)
        assert crit.last_sums[1].item() == want_sums[1]
        (factor * loss).backward()
        print("%s %s: loss %.9g, statement %.17g (bound %.3g)" % (dtype, part, loss.item(), want_loss, loss_bound))
        assert abs(float(loss.item()) - want_loss) <= loss_bound
        values.append(loss.item())
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
        g = x.grad.float().cpu().numpy().astype(np.float64)
        ref = want_grad * factor
        # the pass's gradient within its bound (times the factor), then ONE rounding of the multiplication
        first = (2 * D + P + 12) * U * scale + half_ulp(want_grad, dtype) + P * 2.0 ** -126 * scale
        bound = factor * first + (half_ulp(ref, dtype) if dtype != "float32" else U * np.abs(ref))
        err = np.abs(g - ref)
        print("%s %s, times %g: greatest gradient error %.3g of its bound" % (dtype, part, factor, (err / bound).max()))
        assert (err <= bound).all()
    assert values[0] == values[1]

    # forward only: no gradient buffer, the same value
    calls = []
    inner = merger.mask_ce

    def spy(*args, **kwargs):
        calls.append(kwargs)
        return inner(*args, **kwargs)

    merger.mask_ce = spy
    try:
        with torch.no_grad():
            quiet = crit(dev(pred, dtype).requires_grad_(), d_truth, d_tcs)
        plain = crit(dev(pred, dtype), d_truth, d_tcs)                   # requires_grad=False
    finally:
        del merger.mask_ce
    assert len(calls) == 4 and all(k["grad"] is False and k["out"] is None for k in calls)
    assert not quiet.requires_grad and not plain.requires_grad
    assert quiet.item() == values[0] and plain.item() == values[0]


@pytest.mark.parametrize("part", ["class", "offset"])
def test_module_equals_torch_cross_entropy(merger, part):
    """The module against the criterion it replaces, on the device in float64, with every class in range (the two are
    the same function then): F.cross_entropy(x.double(), planes.max(1)[1]) on the one-hot class planes / the planes of
    Merger.sameness_targets.  Several planes of a pixel may hold 1, so max(1)[1] meets ties; where the device's
    choice is not the first maximal plane the test says so and lets the statement's rule decide."""
    import torch
    import torch.nn.functional as F
    from mergenet_amd import losses
    pred, truth, tcs, offs, want_sums, _, scale, D = batch("float32", part, True)
    H, W = MOD_SHAPE
    P = pred.shape[1]
    assert want_sums[1] == truth.size
    crit = losses.MaskCELoss(merger, part, offs)
    x = dev(pred).requires_grad_()
    d_truth = dev(truth)
    loss = crit(x, d_truth, [classes(t) for t in tcs])
    loss.backward()
    if part == "class":
        by_label = [torch.tensor((0,) + t, device="cuda") for t in tcs]
        inside = (d_truth >= 0) & (d_truth <= G_TRUTH)
        planes = torch.stack([torch.stack([by_label[b][d_truth[b].long().clamp(0, G_TRUTH) * inside[b]] == q
                                           for q in range(P)]) for b in range(2)]).double()
    else:
        planes = torch.stack([merger.sameness_targets(d_truth[b], offs) for b in range(2)]).double()
    elected = planes.max(1)[1]
    first = torch.from_numpy(np.stack([labels.ce_targets(part, P, offs, truth[b], tcs[b], G_TRUTH)[0]
                                       for b in range(2)])).cuda()
    other = elected != first
    if other.any().item():
        print("%s part: max(1)[1] on the device elects another plane than the first maximal one at %d pixels (ties); "
              "the statement's rule decides" % (part, int(other.sum().item())))
        assert (planes.gather(1, elected[:, None]) == planes.gather(1, first[:, None])).all().item()      # ties indeed
    y = dev(pred).double().requires_grad_()
    want = F.cross_entropy(y, first)
    want.backward()
    n = float(truth.size)
    bound = (((D + P + 5) * U + n * 2.0 ** -53) * want_sums[0] + n * P * 2.0 ** -126) * scale + U * want.item()
    print("%s part: module %.9g, torch float64 %.17g (bound %.3g)" % (part, loss.item(), want.item(), bound))
    assert abs(loss.item() - want.item()) <= bound + 1e-12 * want.item()
    g_bound = (2 * D + P + 12) * U * scale + 2.0 ** -52 * scale         # (torch's own softmax - 1 in float64)
    worst = ((x.grad.double() - y.grad).abs().max() / g_bound).item()
    print("%s part: greatest gradient difference %.3g of its bound" % (part, worst))
    assert worst <= 1.0
