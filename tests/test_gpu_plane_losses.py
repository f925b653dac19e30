"""Merger.plane_sums / plane_coeffs / plane_grad and losses.MaskDiceLoss / MaskMultiBCELoss on the device against the
numpy statements (labels.plane_sums, plane_coeffs, plane_grad, dice_loss, multi_bce_loss) on the same arrays.

Bounds (none of them comes from what the kernels give; every test prints its greatest figures before it asserts).
u32 = 2^-24 is half an ulp of float32 relative, "ulp" below means 2^-23 relative.

Sums.  Z (row 2) and the number of pixels are exact.  Every other sum is within relative EPS = 2^-21 + n * 2^-53 of the
statement, n the number of pixels.  q = 1.0f / (1.0f + expf(-x)): expf within 1 ulp, and e/(1 + e) <= 1, so that ulp
reaches q no larger; the addition half an ulp; the division, correctly rounded, half an ulp: q is within 2 ulp =
2^-22 relative.  term = fmaxf(z, 0) + log1pf(expf(-|z|)), the derivation of tests/test_gpu_mask_bce.py restated: expf
within 1 ulp; log1pf within 2 ulp, plus the ulp of its argument carried through (log1p is a contraction in relative
terms on (0, 1]); the final addition half an ulp; both summands are non-negative: 3.5 ulp < 2^-21.  A sum of
non-negative values inherits the relative bound of its values; added in float64 in some order it is within n * 2^-53
of the correctly rounded sum the statement gives.  (1 ulp for expf and 2 ulp for log1pf are taken as OCML's bounds: a
ROCm installation ships no document that states them, so they are an ASSUMPTION of this derivation, the same one the
BCE test rests on.)  A sum whose statement is 0 must be 0; rows 3 and 4 are 0 without the terms flag.  The logits lie
in -12..12 with a band of columns at +-80, where expf(80) and expf(-80) are normal float32.

Coefficients and loss (coeff_bounds), from EPS through the formulas; U = 2^-50 covers the float64 operations.
  Dice.  D = Q + Z + smooth and top = 2I + smooth are sums of non-negative parts: within EPS relative.  top <= D, so
  value = 1 - top/D is within 2*EPS absolute (a ratio <= 1 carries at most twice the relative error of its parts);
  the loss, scale times P values: |scale| * P * 2*EPS.  c1 = sigma*scale*top/D^2: three relative errors, 3*EPS*|c1|.
  c0 = c1 - sigma*scale*2/D: that plus EPS * |scale|*2/D.  Each is then rounded once to float32: u32 * |c|.
  MBCE.  w = (n - S + 1)/(S + 1): the numerator (>= 1) moves by the absolute error of S: EW = EPS*S/(n - S + 1) + EPS
  relative.  value = w*L1 + L0 within (EW + EPS)*w*L1 + EPS*L0; the loss |scale| times the sum of those.
  c0 = c1 = scale*L1*(n + 2)/(S + 1)^2: 3*EPS relative; c2 = scale*w: EW relative; c3 = scale: exact.  Then u32 * |c|.

Gradient, judged alone (the statement's coefficients, rounded to float32, go to the device pass).  With a = the
greater of |c0|, |c1| and b = the greater of |c2|, |c3| of the plane:
  q is within 2 ulp of a value <= 1: 2^-22 absolute; 1 - q rounds once more, 2^-24; their product (<= 1/4) is within
  2^-22 * |1 - 2q| + 2^-24 * q + 2^-26 (its rounding); times c, one rounding of a value <= a/4:
  (2^-22 + 2^-24 + 2^-26 + 2^-26) * a = 0.6875 * 2^-21 * a.
  (s - y): s within 2^-22, the subtraction 2^-25 (|s - y| <= 1), times c one rounding u32 * b: 0.6875 * 2^-21 * b.
  The addition of the two parts and the multiplication by f round once each on a magnitude <= a/4 + b:
  2 * u32 * (a/4 + b) = 0.0625 * 2^-21 * a + 0.25 * 2^-21 * b.
  Together |f| * 2^-21 * (a + b) -- float32 arithmetic on magnitudes |c|/4 and |c|, then |f| -- and for the 16-bit
  types half an ulp of the type AT the reference value (half_ulp, as in the BCE test), the rounding of the store.
Modules: the device's coefficients are within coeff_bounds of the statement's, which moves an element by at most
|f| * (dc01/4 + dc23); the gradient pass adds its own bound above.
"""
import ctypes
import functools

import numpy as np
import pytest

from mergenet_amd import labels

pytestmark = pytest.mark.gpu

C, G_TRUTH = 9, 7
TRUTH_CLASSES = (3, 1, 8, 255, 2, 1, 5)          # label 4 has class 255: outside 0..C-1, an ignore class
SHAPES = [(1, 1),
          (3, 5),
          (7, 64),       # single elements, one chunk per row
          (33, 257),     # single elements, the last chunk of a row reaches past W
          (48, 256),     # 16-byte accesses: one chunk per row in float32, half a chunk in 16 bits
          (32, 1028),    # W % 8 == 4: four elements per lane in every dtype, the last chunk of a row partly past W
          (64, 1032)]    # eight per lane in 16 bits, four in float32; several chunks per row, more than one per wave
DTYPES = ["float32", "bfloat16", "float16"]
SENTINEL = 77.0
TAIL = 64
U = 2.0 ** -50
PARTS = ("class", "offset")


def offsets_for(shape):
    H, W = shape
    return [(0, 1), (1, 0), (-3, 2), (0, -1), (H, 0), (5, -7)]          # 6 planes: a full group and a partial one


def truth_mask(shape, seed=5):
    """Blobs of 7 truth labels (label 4 is the ignore class), a label out of range and a negative one."""
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
    import torch
    return torch.from_numpy(a).to(getattr(torch, dtype)).float().numpy()


@functools.lru_cache(maxsize=None)
def image(shape, dtype="float32", seed=5):
    """({part: logits [P,H,W]}, truth): logits uniform in -12..12, a band of columns at +-80; values of `dtype`."""
    H, W = shape
    rng = np.random.default_rng(seed + 7 * H + 13 * W)
    maps = {"class": (rng.random((C, H, W), dtype=np.float32) * 24 - 12).astype(np.float32),
            "offset": (rng.random((len(offsets_for(shape)), H, W), dtype=np.float32) * 24 - 12).astype(np.float32)}
    b0, b1 = W // 3, W // 3 + max(1, W // 8)
    for k in maps:
        a = maps[k]
        a[:, :, b0:b1] = np.where(rng.random(a[:, :, b0:b1].shape) < 0.5, -80.0, 80.0)
        maps[k] = to_dtype(a, dtype)
        maps[k].setflags(write=False)
    truth = truth_mask(shape, seed)
    truth.setflags(write=False)
    return maps, truth


def part_args(shape, part):
    return (offsets_for(shape) if part == "offset" else None), (TRUTH_CLASSES if part == "class" else None), \
        (G_TRUTH if part == "class" else 0)


@functools.lru_cache(maxsize=None)
def statement_sums(shape, dtype, part, comp, seed=5):
    maps, truth = image(shape, dtype, seed)
    offs, tcs, G = part_args(shape, part)
    s = labels.plane_sums(maps[part], part, offs, truth, tcs, G, complement=comp, terms=True)
    s.setflags(write=False)
    return s


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


def eps_of(n):
    return 2.0 ** -21 + n * 2.0 ** -53


def device_sums(merger, shape, dtype, part, comp=False, terms=True, shift=0, seed=5, **kw):
    maps, truth = image(shape, dtype, seed)
    return merger.plane_sums(dev(maps[part], dtype, shift), part, offsets_for(shape), dev(truth),
                             classes() if part == "class" else None, complement=comp, terms=terms, **kw)


def check_sums(got, want, terms, n_pixels, what):
    P = (want.size - 1) // 5
    assert got.dtype == np.float64 and got.shape == want.shape, what
    want = want.copy()
    if not terms:
        want[3 * P:5 * P] = 0.0
    assert np.array_equal(got[2 * P:3 * P], want[2 * P:3 * P]) and got[-1] == want[-1], what + ": the counts are exact"
    err = np.abs(got[:-1] - want[:-1])
    pos = want[:-1] > 0
    rel = err[pos] / want[:-1][pos]
    print("%s: greatest relative error of a sum %.3g (bound %.3g)" % (what, rel.max() if rel.size else 0.0, eps_of(n_pixels)))
    assert (err <= eps_of(n_pixels) * want[:-1]).all(), what             # (a sum that is 0 must be exactly 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_equal_the_statement(merger, shape, dtype):
    truth = image(shape, dtype)[1]
    ignored = int((truth == 4).sum())
    if shape[0] >= 32:
        assert ignored > 0                                               # the ignore class occurs
    for part in PARTS:
        for comp in (False, True):
            want = statement_sums(shape, dtype, part, comp)
            assert want[-1] == truth.size - (ignored if part == "class" else 0)
            for terms in (True, False):
                got = device_sums(merger, shape, dtype, part, comp, terms).cpu().numpy()
                check_sums(got, want, terms, truth.size, "%s %s %s complement=%s terms=%s" % (shape, dtype, part, comp, terms))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(32, 1028), (64, 1032)])
def test_sums_are_the_same_bits_again_and_off_the_boundary(merger, shape, dtype):
    for part in PARTS:
        for terms in (True, False):
            a = device_sums(merger, shape, dtype, part, True, terms).cpu().numpy()
            b = device_sums(merger, shape, dtype, part, True, terms).cpu().numpy()
            off = device_sums(merger, shape, dtype, part, True, terms, shift=1).cpu().numpy()
            assert a.tobytes() == b.tobytes(), "two runs differ"
            assert a.tobytes() == off.tobytes(), "the map one element off the boundary: other sums"
            check_sums(off, statement_sums(shape, dtype, part, True), terms, shape[0] * shape[1], "one element off")


def test_into_is_one_ieee_addition_and_out_stores(merger):
    import torch
    shape = (32, 1028)
    for part in PARTS:
        a = device_sums(merger, shape, "float32", part)
        b = device_sums(merger, shape, "float32", part, seed=6)
        assert not torch.equal(a, b)
        total = a.clone()
        back = device_sums(merger, shape, "float32", part, seed=6, into=total)
        assert back is total and torch.equal(total, a + b)
        table = torch.full((2, a.numel()), SENTINEL, dtype=torch.float64, device="cuda")
        device_sums(merger, shape, "float32", part, seed=6, out=table[1])
        assert torch.equal(table[1], b) and (table[0] == SENTINEL).all().item()


# ---- coefficients and loss ----------------------------------------------------------------------------------------

def coeff_bounds(criterion, sums, eps, pixels=0.0, smooth=1.0, scale=1.0):
    """(bound of each coefficient [4,P], bound of the loss) for device sums within `eps` relative of `sums` -- the
    derivation of the module docstring."""
    s = np.asarray(sums, np.float64)
    P = (s.size - 1) // 5
    Q, I, Z, L1, L0 = (s[r * P:(r + 1) * P] for r in range(5))
    sc = abs(scale)
    u32 = 2.0 ** -24
    if criterion == "dice":
        D, top = Q + Z + smooth, 2 * I + smooth
        c1 = sc * top / D ** 2
        d1 = 3 * eps * c1
        d0 = d1 + eps * sc * 2 / D
        c0 = np.abs(c1 - sc * 2 / D)
        dc = np.stack([d0 + (u32 + U) * c0 + U * sc * 2 / D, d1 + (u32 + U) * c1, np.zeros(P), np.zeros(P)])
        return dc, sc * P * (2 * eps + U)
    S = Q
    w = (pixels - S + 1) / (S + 1)
    ew = eps * S / (pixels - S + 1) + eps
    c0 = sc * L1 * (pixels + 2) / (S + 1) ** 2
    dvalue = (ew + eps + U) * w * L1 + (eps + U) * L0
    dc = np.stack([(3 * eps + u32 + U) * c0] * 2 + [(ew + u32 + U) * sc * w, np.full(P, u32 * sc)])
    return dc, sc * dvalue.sum()


COEFF_CASES = [("dice", False, 1.0, 1.0), ("dice", True, 0.25, 2.0), ("mbce", False, 1.0, None)]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("shape", [(3, 5), (33, 257), (64, 1032)])
def test_coefficients_and_loss_equal_the_statement(merger, shape, dtype):
    import torch
    n = shape[0] * shape[1]
    for part in PARTS:
        P = C if part == "class" else len(offsets_for(shape))
        for crit, comp, smooth, scale in COEFF_CASES:
            scale = 1.0 / (P * n) if scale is None else scale
            want_sums = statement_sums(shape, dtype, part, comp)
            want_c, want_loss = labels.plane_coeffs(crit, want_sums, pixels=n, smooth=smooth, scale=scale, complement=comp)
            dc, dloss = coeff_bounds(crit, want_sums, eps_of(n), n, smooth, scale)
            sums = device_sums(merger, shape, dtype, part, comp, crit == "mbce")
            res = merger.plane_coeffs(crit, sums, pixels=n, smooth=smooth, scale=scale, complement=comp)
            got_c, got_loss = res["coeffs"].cpu().numpy().astype(np.float64), res["loss"].item()
            assert res["coeffs"].dtype == torch.float32 and tuple(res["coeffs"].shape) == (4, P)
            err = np.abs(got_c - want_c)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = np.nanmax(np.where(dc > 0, err / dc, 0.0))
            print("%s %s %s %s: greatest coefficient error %.3g of its bound; loss %.17g against %.17g, error %.3g (bound %.3g)"
                  % (shape, dtype, part, crit, worst, got_loss, want_loss, abs(got_loss - want_loss), dloss))
            assert (err <= dc).all() and abs(got_loss - want_loss) <= dloss
            if crit == "dice":
                assert (got_c[2:] == 0).all()
            # accumulate: one IEEE addition; out: the caller's buffer
            acc = res["loss"].clone()
            buf = torch.empty((4, P), dtype=torch.float32, device="cuda")
            again = merger.plane_coeffs(crit, sums, pixels=n, smooth=smooth, scale=scale, complement=comp, into=acc, out=buf)
            assert again["coeffs"] is buf and torch.equal(buf, res["coeffs"]) and again["loss"] is acc
            assert acc.item() == got_loss + got_loss


# ---- the gradient pass, judged alone ------------------------------------------------------------------------------

def grad_cases(shape, dtype, part):
    """(name, float32 coefficients, complement, factor): Dice in both modes (no (s - y) part), MBCE, and MBCE's
    coefficients under the complement flag (both parts of the formula with q != s)."""
    n = shape[0] * shape[1]
    dice1 = labels.plane_coeffs("dice", statement_sums(shape, dtype, part, False), smooth=1.0)[0]
    dice0 = labels.plane_coeffs("dice", statement_sums(shape, dtype, part, True), smooth=1.0, complement=True)[0]
    mbce = labels.plane_coeffs("mbce", statement_sums(shape, dtype, part, False), pixels=n, scale=1.0 / 64)[0]
    return [("dice mode 1", dice1.astype(np.float32), False, None), ("dice mode 0", dice0.astype(np.float32), True, 3.0),
            ("mbce", mbce.astype(np.float32), False, 1.0), ("mbce coefficients, complement", mbce.astype(np.float32), True, 3.0)]


def run_grad(merger, shape, dtype, part, coeffs, comp, factor, shifts=(0, 0)):
    import torch
    maps, truth = image(shape, dtype)
    buf = GradBuffer(maps[part].shape, dtype, shifts[1])
    f = None if factor is None else torch.tensor(factor, dtype=torch.float32, device="cuda")
    out = merger.plane_grad(dev(maps[part], dtype, shifts[0]), part, offsets_for(shape), dev(truth),
                            classes() if part == "class" else None, dev(coeffs), factor=f, complement=comp, out=buf.view)
    assert out is buf.view
    return buf


def check_grad(buf, shape, dtype, part, coeffs, comp, factor, what):
    maps, truth = image(shape, dtype)
    offs, tcs, G = part_args(shape, part)
    f = 1.0 if factor is None else factor
    ref = labels.plane_grad(maps[part], part, offs, truth, tcs, G, coeffs.astype(np.float64), f, complement=comp)
    g = buf.view.float().cpu().numpy().astype(np.float64)
    assert g.shape == ref.shape and not np.isnan(g).any(), what + ": an element was not written"
    c = np.abs(coeffs.astype(np.float64))
    mag = (np.maximum(c[0], c[1]) + np.maximum(c[2], c[3]))[:, None, None]
    bound = abs(f) * 2.0 ** -21 * mag + half_ulp(ref, dtype)
    err = np.abs(g - ref)
    print("%s: greatest gradient error %.3g of its bound" % (what, (err / bound).max()))
    assert (err <= bound).all(), what
    if part == "class" and (truth == 4).any():
        assert (g[:, truth == 4] == 0).all() and np.abs(g[:, truth != 4]).max() > 0, what + ": ignored pixels hold 0"
    buf.check_surroundings()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_equals_the_statement(merger, shape, dtype):
    for part in PARTS:
        for name, coeffs, comp, factor in grad_cases(shape, dtype, part):
            buf = run_grad(merger, shape, dtype, part, coeffs, comp, factor)
            check_grad(buf, shape, dtype, part, coeffs, comp, factor, "%s %s %s %s" % (shape, dtype, part, name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(32, 1028), (64, 1032)])
def test_gradient_with_a_base_off_the_boundary(merger, shape, dtype):
    import torch
    bits = torch.int32 if dtype == "float32" else torch.int16
    for part in PARTS:
        name, coeffs, comp, factor = grad_cases(shape, dtype, part)[2]
        aligned = run_grad(merger, shape, dtype, part, coeffs, comp, factor)
        for shifts in ((1, 0), (0, 1)):
            buf = run_grad(merger, shape, dtype, part, coeffs, comp, factor, shifts)
            check_grad(buf, shape, dtype, part, coeffs, comp, factor, "%s %s %s shifts %s" % (shape, dtype, part, shifts))
            assert torch.equal(buf.view.contiguous().view(bits), aligned.view.contiguous().view(bits))


def test_skipping_the_second_part_gives_the_same_values(merger):
    """Dice's coefficients with c2 = c3 = 0 take the branch without (s - y); with a c3 that is not zero on ONE plane
    every plane takes the other branch: the planes whose c2 and c3 are 0 must hold the same values."""
    import torch
    shape, dtype = (33, 257), "float32"
    for part in PARTS:
        name, coeffs, comp, factor = grad_cases(shape, dtype, part)[1]
        a = run_grad(merger, shape, dtype, part, coeffs, comp, factor)
        other = coeffs.copy()
        other[3, 0] = 0.5
        b = run_grad(merger, shape, dtype, part, other, comp, factor)
        assert torch.equal(a.view[1:], b.view[1:]) and not torch.equal(a.view[0], b.view[0])


def test_bad_arguments_are_refused_and_launch_nothing(merger):
    import torch
    from mergenet_amd import segmenter as seg
    shape = (7, 64)
    H, W = shape
    maps, truth = image(shape)
    offs = np.ascontiguousarray(np.asarray(offsets_for(shape), np.int32))
    O = offs.shape[0]
    d_cl, d_sl, d_truth, d_classes = dev(maps["class"]), dev(maps["offset"]), dev(truth), classes()
    sums = torch.full((5 * C + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    coeffs = torch.full((4, C), SENTINEL, dtype=torch.float32, device="cuda")
    loss = torch.full((), SENTINEL, dtype=torch.float64, device="cuda")
    gbuf = GradBuffer(maps["class"].shape, "float32")
    good_sums = device_sums(merger, shape, "float32", "class", terms=True)
    good_coeffs = merger.plane_coeffs("mbce", good_sums, pixels=H * W)["coeffs"]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32p = ctypes.POINTER(ctypes.c_int)
    lib = merger.lib

    def plane(**over):
        a = dict(ctx=merger.handle, logits=d_cl.data_ptr(), dtype=seg.MN_DTYPE_F32, width=W, height=H,
                 part=seg.MN_PART_CLASS, planes=C, offsets=None, truth=d_truth.data_ptr(), num_truth=G_TRUTH,
                 truth_classes=d_classes.data_ptr(), flags=seg.MN_PLANE_TERMS)
        assert set(over) <= set(a)
        a.update(over)
        return list(a.values())

    def raw_sums(sums_ptr=sums.data_ptr(), **over):
        return lib.mn_plane_sums_device(*plane(**over), sums_ptr, 0, stream)

    def raw_grad(coeffs_ptr=good_coeffs.data_ptr(), grad_ptr=gbuf.view.data_ptr(), **over):
        return lib.mn_plane_grad_device(*plane(**over), coeffs_ptr, None, grad_ptr, stream)

    def raw_coeffs(**over):
        a = dict(ctx=merger.handle, criterion=seg.MN_CRIT_DICE, flags=0, sums=good_sums.data_ptr(), planes=C,
                 pixels=float(H * W), smooth=1.0, scale=1.0, coeffs=coeffs.data_ptr(), loss=loss.data_ptr(),
                 accumulate=0, stream=stream)
        assert set(over) <= set(a)
        a.update(over)
        return lib.mn_plane_coeffs_device(*a.values())

    offset_part = dict(part=seg.MN_PART_OFFSET, planes=O, logits=d_sl.data_ptr(), offsets=offs.ctypes.data_as(i32p))
    bad = [dict(ctx=None), dict(logits=None), dict(truth=None), dict(truth_classes=None),   # pointers that are needed
           dict(offset_part, offsets=None),
           dict(width=0), dict(height=-1), dict(planes=0), dict(planes=128), dict(offset_part, planes=33),
           dict(num_truth=-1), dict(height=1 << 16, width=1 << 15), dict(height=1, width=(1 << 30) + 8),
           dict(part=2), dict(part=-1), dict(flags=4), dict(flags=-1),
           dict(dtype=3), dict(dtype=-1), dict(dtype=seg.MN_DTYPE_F32 | seg.MN_MAPS_LOGITS)]
    for over in bad:
        assert raw_sums(**over) == seg.MN_ERR_ARGUMENT, over
        assert lib.mn_last_status() == seg.MN_ERR_ARGUMENT
        assert raw_grad(**over) == seg.MN_ERR_ARGUMENT, over
    assert raw_sums(sums_ptr=None) == seg.MN_ERR_ARGUMENT
    assert raw_grad(coeffs_ptr=None) == seg.MN_ERR_ARGUMENT and raw_grad(grad_ptr=None) == seg.MN_ERR_ARGUMENT
    nan, inf = float("nan"), float("inf")
    bad_coeffs = [dict(ctx=None), dict(sums=None), dict(coeffs=None), dict(loss=None), dict(planes=0), dict(planes=128),
                  dict(criterion=2), dict(criterion=-1), dict(flags=4),
                  dict(criterion=seg.MN_CRIT_MBCE, flags=seg.MN_PLANE_COMPLEMENT),
                  dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=nan), dict(smooth=inf), dict(scale=nan),
                  dict(scale=-inf), dict(pixels=nan), dict(pixels=inf), dict(pixels=-1.0)]
    for over in bad_coeffs:
        assert raw_coeffs(**over) == seg.MN_ERR_ARGUMENT, over
        assert lib.mn_last_status() == seg.MN_ERR_ARGUMENT
    # through the wrappers: what they hand on comes back as MergeNetError, what they refuse themselves as ValueError
    with pytest.raises(seg.MergeNetError):
        merger.plane_coeffs("dice", good_sums, smooth=0.0, out=coeffs, into=loss)
    with pytest.raises(seg.MergeNetError):
        merger.plane_sums(torch.zeros((33, H, W), device="cuda"), "offset", [(0, 1)] * 33, d_truth, None)
    with pytest.raises(ValueError):
        merger.plane_sums(d_cl, "both", None, d_truth, d_classes)
    with pytest.raises(ValueError):
        merger.plane_sums(d_cl.cpu(), "class", None, d_truth, d_classes)
    with pytest.raises(ValueError):
        merger.plane_sums(d_cl.double(), "class", None, d_truth, d_classes)
    with pytest.raises(ValueError):
        merger.plane_sums(d_sl, "offset", offsets_for(shape)[:3], d_truth, None)
    with pytest.raises(ValueError):
        merger.plane_sums(d_cl, "class", None, d_truth.long(), d_classes)
    with pytest.raises(ValueError):
        merger.plane_sums(d_cl, "class", None, d_truth, d_classes, into=sums[:3])
    with pytest.raises(ValueError):
        merger.plane_coeffs("ce", good_sums)
    with pytest.raises(ValueError):
        merger.plane_grad(d_cl, "class", None, d_truth, d_classes, good_coeffs[:, :3], out=gbuf.view)
    with pytest.raises(ValueError):
        merger.plane_grad(d_cl, "class", None, d_truth, d_classes, good_coeffs, out=gbuf.view.half())
    with pytest.raises(ValueError):
        merger.plane_grad(d_cl, "class", None, d_truth, d_classes, good_coeffs, factor=torch.ones((), device="cuda").double())
    torch.cuda.synchronize()
    assert (sums == SENTINEL).all().item() and (coeffs == SENTINEL).all().item() and loss.item() == SENTINEL
    assert torch.isnan(gbuf.view).all().item()                           # nothing ran
    gbuf.check_surroundings()
    assert raw_sums() == 0 and raw_coeffs() == 0 and raw_grad() == 0     # and the good calls still do
    assert torch.equal(sums, good_sums)
    check_grad(gbuf, shape, "float32", "class", good_coeffs.cpu().numpy(), False, None, "after the refusals")


# ---- the modules --------------------------------------------------------------------------------------------------

MOD_SHAPE, MOD_B = (24, 136), 2
MOD_OFFSETS = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (2, 2), (-2, 2), (0, 40), (40, 0)]
MOD_TCS = [TRUTH_CLASSES, (1, 2, 3, 4, 5, 6, 7)]
CRITERIA = [("dice", "1"), ("dice", "0"), ("mbce", None)]


@functools.lru_cache(maxsize=None)
def batch(dtype, part):
    """(prediction [2, P, 24, 136] holding values of `dtype`, truth [2, 24, 136])."""
    H, W = MOD_SHAPE
    P = C if part == "class" else len(MOD_OFFSETS)
    rng = np.random.default_rng(11 + P)
    pred = to_dtype((rng.random((MOD_B, P, H, W), dtype=np.float32) * 24 - 12).astype(np.float32), dtype)
    truth = np.stack([truth_mask(MOD_SHAPE, 5), truth_mask(MOD_SHAPE, 6)])
    assert not np.array_equal(truth[0], truth[1])
    return pred, truth


@functools.lru_cache(maxsize=None)
def batch_statement(dtype, part, crit, mode):
    """(loss, gradient, coefficient magnitudes a and b per image and plane, their bounds, the loss's bound)."""
    pred, truth = batch(dtype, part)
    B, P, H, W = pred.shape
    offs = MOD_OFFSETS if part == "offset" else None
    tcs = MOD_TCS if part == "class" else None
    G = [len(t) for t in MOD_TCS] if part == "class" else [0, 0]
    comp = mode == "0"
    per = [labels.plane_sums(pred[b], part, offs, truth[b], tcs[b] if tcs else None, G[b], complement=comp,
                             terms=crit == "mbce") for b in range(B)]
    if crit == "dice":
        loss, grad = labels.dice_loss(pred, part, offs, truth, tcs, mode=mode, smooth=1.0)
        sums = per[0] + per[1]
        c = labels.plane_coeffs("dice", sums, smooth=1.0, complement=comp)[0]
        dc, dloss = coeff_bounds("dice", sums, eps_of(B * H * W) + U)
        cs, dcs = [c] * B, [dc] * B
    else:
        loss, grad = labels.multi_bce_loss(pred, part, offs, truth, tcs)
        scale = 1.0 / (B * P * H * W)
        cs = [labels.plane_coeffs("mbce", s, pixels=H * W, scale=scale)[0] for s in per]
        bounds = [coeff_bounds("mbce", s, eps_of(H * W), H * W, 1.0, scale) for s in per]
        dcs, dloss = [b[0] for b in bounds], sum(b[1] for b in bounds)
    a = np.stack([np.maximum(np.abs(c[0]), np.abs(c[1])) for c in cs])[:, :, None, None]
    b = np.stack([np.maximum(np.abs(c[2]), np.abs(c[3])) for c in cs])[:, :, None, None]
    da = np.stack([np.maximum(d[0], d[1]) for d in dcs])[:, :, None, None]
    db = np.stack([np.maximum(d[2], d[3]) for d in dcs])[:, :, None, None]
    dloss = dloss + 2.0 ** -24 * abs(loss)                               # the float32 the module returns
    return loss, grad, (a, b, da, db), dloss


def make_criterion(merger, part, crit, mode):
    from mergenet_amd import losses
    offs = MOD_OFFSETS if part == "offset" else None
    if crit == "dice":
        return losses.MaskDiceLoss(merger, part, offs, mode=mode, smooth=1.0)
    return losses.MaskMultiBCELoss(merger, part, offs)


def module_grad_bound(dtype, part, crit, mode, factor):
    loss, grad, (a, b, da, db), dloss = batch_statement(dtype, part, crit, mode)
    ref = grad * factor
    return ref, abs(factor) * (da / 4 + db + 2.0 ** -21 * (a + da + b + db)) + half_ulp(ref, dtype)


@pytest.mark.parametrize("crit,mode", CRITERIA)
@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_module_loss_and_backward(merger, dtype, part, crit, mode):
    import torch
    pred, truth = batch(dtype, part)
    want_loss, _, _, dloss = batch_statement(dtype, part, crit, mode)
    criterion = make_criterion(merger, part, crit, mode)
    d_truth = dev(truth)
    d_tcs = [classes(t) for t in MOD_TCS] if part == "class" else None
    values = []
    for factor in (1.0, 3.0):
        x = dev(pred, dtype).requires_grad_()
        loss = criterion(x, d_truth, d_tcs)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad and loss.is_cuda
        assert criterion.last_sums.dtype == torch.float64
        (factor * loss).backward()
        print("%s %s %s %s: loss %.9g, statement %.17g (bound %.3g)" % (dtype, part, crit, mode, loss.item(), want_loss, dloss))
        assert abs(float(loss.item()) - want_loss) <= dloss
        values.append(loss.item())
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape and x.grad.is_contiguous()
        ref, bound = module_grad_bound(dtype, part, crit, mode, factor)
        err = np.abs(x.grad.float().cpu().numpy().astype(np.float64) - ref)
        print("times %g: greatest gradient error %.3g of its bound" % (factor, (err / bound).max()))
        assert (err <= bound).all()
        if part == "class":
            ignored = truth == 4
            ignored[1] = False                                           # (label 4 of the second image has class 4)
            assert ignored.any() and (x.grad.float().cpu().numpy().transpose(1, 0, 2, 3)[:, ignored] == 0).all()
    assert values[0] == values[1]


@pytest.mark.parametrize("crit,mode", CRITERIA)
@pytest.mark.parametrize("part", PARTS)
def test_module_equals_the_torch_composition(merger, part, crit, mode):
    """The module against the criterion it replaces, written as a float64 torch composition on the device with
    materialised target planes (no ignore class: the two are the same function).  The composition itself is float64:
    it is within 1e-12 relative of the statement, which the bounds of the module then absorb."""
    import torch
    pred, truth = batch("float32", part)
    B, P, H, W = pred.shape
    tc = MOD_TCS[1]
    d_truth = dev(truth)
    offs = MOD_OFFSETS if part == "offset" else None
    tcs = [tc, tc] if part == "class" else None
    if part == "class":
        by_label = torch.tensor((0,) + tc, device="cuda")
        inside = (d_truth >= 0) & (d_truth <= G_TRUTH)
        target = torch.stack([by_label[d_truth.long().clamp(0, G_TRUTH) * inside] == q for q in range(P)], 1).double()
    else:
        target = torch.stack([merger.sameness_targets(d_truth[b], offs) for b in range(B)]).double()
    y = dev(pred).double().requires_grad_()
    if crit == "dice":
        p, t = torch.sigmoid(y), target
        if mode == "0":
            p, t = torch.sigmoid(-y), 1 - target
        want = (1 - (2 * (p * t).sum((0, 2, 3)) + 1.0) / (p.sum((0, 2, 3)) + t.sum((0, 2, 3)) + 1.0)).sum()
        want_np, grad_np = labels.dice_loss(pred, part, offs, truth, tcs, mode=mode)
    else:
        s = torch.sigmoid(y).sum((2, 3))
        weight = ((H * W - s + 1) / (s + 1))[:, :, None, None] * target + (1 - target)
        want = (weight * torch.nn.functional.binary_cross_entropy_with_logits(y, target, reduction="none")).mean()
        want_np, grad_np = labels.multi_bce_loss(pred, part, offs, truth, tcs)
    want.backward()
    comp_grad = y.grad.cpu().numpy()
    assert abs(want.item() - want_np) <= 1e-12 * abs(want_np)
    assert np.abs(comp_grad - grad_np).max() <= 1e-12 * np.abs(grad_np).max()
    criterion = make_criterion(merger, part, crit, mode)
    x = dev(pred).requires_grad_()
    loss = criterion(x, d_truth, [classes(tc), classes(tc)] if part == "class" else None)
    loss.backward()
    # the bounds of the statement for THIS truth (class part: other classes than batch_statement's)
    per = [labels.plane_sums(pred[b], part, offs, truth[b], tc if part == "class" else None,
                             G_TRUTH if part == "class" else 0, complement=mode == "0", terms=crit == "mbce") for b in range(B)]
    if crit == "dice":
        dcs = [coeff_bounds("dice", per[0] + per[1], eps_of(B * H * W) + U)] * B
        cs = [labels.plane_coeffs("dice", per[0] + per[1], complement=mode == "0")[0]] * B
        dloss = dcs[0][1]
    else:
        scale = 1.0 / (B * P * H * W)
        dcs = [coeff_bounds("mbce", s, eps_of(H * W), H * W, 1.0, scale) for s in per]
        cs = [labels.plane_coeffs("mbce", s, pixels=H * W, scale=scale)[0] for s in per]
        dloss = sum(d[1] for d in dcs)
    dloss += (2.0 ** -24 + 1e-12) * abs(want.item())
    print("%s %s %s: module %.9g, torch float64 %.17g (bound %.3g)" % (part, crit, mode, loss.item(), want.item(), dloss))
    assert abs(loss.item() - want.item()) <= dloss
    a = np.stack([np.maximum(np.abs(c[0]), np.abs(c[1])) for c in cs])[:, :, None, None]
    b = np.stack([np.maximum(np.abs(c[2]), np.abs(c[3])) for c in cs])[:, :, None, None]
    da = np.stack([np.maximum(d[0][0], d[0][1]) for d in dcs])[:, :, None, None]
    db = np.stack([np.maximum(d[0][2], d[0][3]) for d in dcs])[:, :, None, None]
    bound = da / 4 + db + 2.0 ** -21 * (a + da + b + db) + 1e-12 * np.abs(grad_np).max()
    err = np.abs(x.grad.cpu().numpy().astype(np.float64) - comp_grad)
    print("greatest gradient error %.3g of its bound" % (err / bound).max())
    assert (err <= bound).all()


def test_module_backward_twice_channel_slice_and_no_grad(merger):
    import torch
    from mergenet_amd import losses
    dtype, part = "float32", "offset"
    pred, truth = batch(dtype, part)
    B, P, H, W = pred.shape
    d_truth = dev(truth)
    criterion = losses.MaskDiceLoss(merger, "offset", MOD_OFFSETS, mode="0")
    # backward twice on one forward
    x = dev(pred).requires_grad_()
    loss = criterion(x, d_truth)
    loss.backward(retain_graph=True)
    first = x.grad.clone()
    x.grad = None
    loss.backward()
    assert torch.equal(first, x.grad)
    # a channel slice of the network's output: 9 class planes in front
    rng = np.random.default_rng(3)
    full = np.concatenate([rng.random((B, C, H, W), dtype=np.float32), pred], axis=1)
    xs = dev(full).requires_grad_()
    assert not xs[:, C:].is_contiguous()
    sliced = criterion(xs[:, C:], d_truth)
    sliced.backward()
    assert sliced.item() == loss.item()
    assert (xs.grad[:, :C] == 0).all().item() and torch.equal(xs.grad[:, C:], first)
    ref, bound = module_grad_bound(dtype, part, "dice", "0", 1.0)
    assert (np.abs(xs.grad[:, C:].cpu().numpy().astype(np.float64) - ref) <= bound).all()
    with pytest.raises(ValueError):
        criterion(xs[:, :, ::2], d_truth[:, ::2])                        # an image that is no contiguous block
    # forward only: no gradient pass, the same value
    calls = []
    inner = merger.plane_grad

    def spy(*args, **kwargs):
        calls.append(kwargs)
        return inner(*args, **kwargs)

    merger.plane_grad = spy
    try:
        for crit in (criterion, losses.MaskMultiBCELoss(merger, "offset", MOD_OFFSETS)):
            with torch.no_grad():
                quiet = crit(dev(pred).requires_grad_(), d_truth)
            plain = crit(dev(pred), d_truth)                             # requires_grad=False
            assert not quiet.requires_grad and not plain.requires_grad and quiet.item() == plain.item()
        assert calls == []
        x2 = dev(pred).requires_grad_()
        criterion(x2, d_truth).backward()
        assert len(calls) == B and quiet.item() > 0
    finally:
        del merger.plane_grad
    assert torch.equal(x2.grad, first)
