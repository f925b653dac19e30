"""labels.dice_loss / multi_bce_loss and the three-step statements labels.plane_sums / plane_coeffs / plane_grad -- the
numpy statements of losses.MaskDiceLoss / MaskMultiBCELoss and of Merger.plane_sums / plane_coeffs / plane_grad --
against the reference's own criteria (tests/golden/plane_losses_v1.npz, written by make_golden_plane_losses.py), on
hand-computed cases and on the ignore class; the C ABI of the three entry points (no GPU).

Bounds against the fixture.  Both sides are float64 throughout; u = 2^-52.  A plane's sums have n = B*H*W = 480 terms
(Dice, over the batch) or n = H*W = 240 (MBCE, per image), all of one sign: the statement's are correctly rounded
(math.fsum) and torch's, added in some order, are within n*u relative of them; sigmoid and softplus per element are
within a few u, which the sum inherits, so every sum is within (n + 4)*u <= 2*n*u relative of the other side's.
  Dice loss.  Per plane 1 - top/D, top = 2I + smooth <= D: a ratio <= 1 of two such sums carries at most 4*n*u
  absolute, the subtraction from 1 half a u more; P planes: P * (4*n + 1) * u.
  Dice gradient.  sigma*q*(1 - q)*(top/D^2 - 2z/D): with M = top/D^2 + 2/D the bracket is within (3 * 2*n*u + 2u)*M of
  the other side's (three sums' relative errors in top/D^2, one in 2/D, one subtraction), q*(1 - q) <= 1/4 within 4u:
  8*n*u * M/4.
  MBCE loss.  scale * sum of (w*L1 + L0), all terms >= 0, w = (n - S + 1)/(S + 1).  The numerator n - S + 1 >= 1
  cancels: it moves by the absolute error of S, 2*n*u*S, so it is within 2*n*u*S/(n - S + 1) relative, the denominator
  within 2*n*u, the division u more (mbce_weight_bound, from the reference's S of the fixture's logits, the greatest
  over the planes).  L1 and L0 are sums as above and the products and the mean add a few u: the loss is within
  (mbce_weight_bound + 4*n*u) relative.
  MBCE gradient.  scale*[(s - y)*(w or 1) + L1*(-(n + 2)/(S + 1)^2)*s*(1 - s)]: magnitude at most M = scale*(max(w, 1)
  + L1*(n + 2)/(S + 1)^2/4); each product carries the relative errors of w or of L1 and S: (mbce_weight_bound +
  8*n*u) * M.
None of these comes from what the statement gives; the tests print the greatest figure before they assert."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from mergenet_amd import labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "plane_losses_v1.npz"))


def part_inputs(golden, part):
    offs = [tuple(int(v) for v in o) for o in golden["offsets"]]
    tcs = [golden["truth_classes"][b] for b in range(golden["truth"].shape[0])]
    return golden["%s_logits" % part], offs if part == "offset" else None, golden["truth"], tcs


def test_fixture_targets_are_the_statements(golden):
    for part in ("class", "offset"):
        x, offs, truth, tcs = part_inputs(golden, part)
        for b in range(x.shape[0]):
            y, keep = labels.plane_targets(part, x.shape[1], offs, truth[b], tcs[b], len(tcs[b]))
            assert keep.all() and np.array_equal(y, golden["%s_targets" % part][b].astype(bool))
    assert "composition" in str(golden["mbce_grad_is"])


@pytest.mark.parametrize("mode", ["1", "0"])
@pytest.mark.parametrize("part", ["class", "offset"])
def test_dice_loss_equals_the_reference(golden, part, mode):
    x, offs, truth, tcs = part_inputs(golden, part)
    B, P, H, W = x.shape
    n = B * H * W
    loss, grad = labels.dice_loss(x, part, offs, truth, tcs, mode=mode, smooth=1.0)
    want, want_grad = float(golden["%s_dice%s_loss" % (part, mode)]), golden["%s_dice%s_grad" % (part, mode)]
    bound = P * (4 * n + 1) * U
    print("%s mode %s: loss %.17g against %.17g, error %.3g (bound %.3g)" % (part, mode, loss, want, abs(loss - want), bound))
    assert abs(loss - want) <= bound
    t = golden["%s_targets" % part].astype(np.float64)
    q = 1.0 / (1.0 + np.exp(-x))
    if mode == "0":
        q, t = 1.0 - q, 1.0 - t
    top = 2.0 * (q * t).sum(axis=(0, 2, 3)) + 1.0
    D = q.sum(axis=(0, 2, 3)) + t.sum(axis=(0, 2, 3)) + 1.0
    M = (top / D ** 2 + 2.0 / D)[None, :, None, None]
    gbound = 8 * n * U * M / 4
    err = np.abs(grad - want_grad)
    print("%s mode %s: greatest gradient error %.3g of its bound" % (part, mode, (err / gbound).max()))
    assert grad.shape == want_grad.shape and (err <= gbound).all()
    assert np.abs(want_grad).max() > 1e-4                                # (the comparison is not of zeros)


def mbce_weight_bound(S, n):
    """Relative bound of w = (n - S + 1)/(S + 1) given S within 2*n*u relative: the numerator moves by 2*n*u*S."""
    return 2 * n * U * S / (n - S + 1.0) + 2 * n * U + 2 * U


@pytest.mark.parametrize("part", ["class", "offset"])
def test_multi_bce_loss_equals_the_reference(golden, part):
    x, offs, truth, tcs = part_inputs(golden, part)
    B, P, H, W = x.shape
    n = H * W
    loss, grad = labels.multi_bce_loss(x, part, offs, truth, tcs)
    want = float(golden["%s_mbce_loss" % part])
    assert float(golden["%s_mbce_loss_composition" % part]) == pytest.approx(want, rel=1e-14, abs=0)
    want_grad = golden["%s_mbce_grad_composition" % part]
    t = golden["%s_targets" % part].astype(bool)
    s = 1.0 / (1.0 + np.exp(-x))
    S = s.sum(axis=(2, 3))
    L1 = (np.logaddexp(0.0, -x) * t).sum(axis=(2, 3))
    w = (n - S + 1.0) / (S + 1.0)
    wb = mbce_weight_bound(S, n).max()
    bound = (wb + 4 * n * U) * want
    print("%s: loss %.17g against %.17g, error %.3g (bound %.3g)" % (part, loss, want, abs(loss - want), bound))
    assert abs(loss - want) <= bound
    scale = 1.0 / (B * P * H * W)
    M = scale * (np.maximum(w, 1.0) + L1 * (n + 2.0) / (S + 1.0) ** 2 / 4)[:, :, None, None]
    gbound = (wb + 8 * n * U) * M
    err = np.abs(grad - want_grad)
    print("%s: greatest gradient error %.3g of its bound" % (part, (err / gbound).max()))
    assert grad.shape == want_grad.shape and (err <= gbound).all()
    assert np.abs(want_grad).max() > 1e-6


def test_dice_by_hand_on_two_pixels():
    """1x2 image, one class-1 instance on the right pixel, logits 0 everywhere: p = 1/2.  Plane 1 (t = [0, 1]):
    I = 1/2, sum p = 1, sum t = 1, value 1 - (1 + 1)/(1 + 1 + 1) = 1/3; plane 0 (t = [1, 0]) the same.  Gradient of
    plane 1: p(1-p) * (-2t/D + 2/D^2) = 1/4 * (-2t/3 + 2/9) = [1/18, -1/9]."""
    truth = np.array([[[0, 1]]], np.int32)
    x = np.zeros((1, 2, 1, 2), np.float32)
    loss, grad = labels.dice_loss(x, "class", None, truth, [[1]], mode="1", smooth=1.0)
    assert abs(loss - 2.0 / 3.0) <= 2 * U
    np.testing.assert_allclose(grad[0, 1, 0], [1.0 / 18, -1.0 / 9], rtol=4 * U, atol=0)
    np.testing.assert_allclose(grad[0, 0, 0], [-1.0 / 9, 1.0 / 18], rtol=4 * U, atol=0)
    # mode '0' on plane 1: q = 1 - p = 1/2, z = 1 - t = [1, 0]: the same value; dq/dx = -q(1-q) flips the sign
    loss0, grad0 = labels.dice_loss(x, "class", None, truth, [[1]], mode="0", smooth=1.0)
    assert abs(loss0 - 2.0 / 3.0) <= 2 * U
    np.testing.assert_allclose(grad0[0, 1, 0], [1.0 / 9, -1.0 / 18], rtol=4 * U, atol=0)
    # the offset part with offset (0, 1): the left pixel's neighbour differs (t = 0), the right one's is outside (1)
    lo, go = labels.dice_loss(x[:, :1], "offset", [(0, 1)], truth, None, mode="1", smooth=1.0)
    assert abs(lo - 1.0 / 3.0) <= 2 * U
    np.testing.assert_allclose(go[0, 0, 0], [1.0 / 18, -1.0 / 9], rtol=4 * U, atol=0)


def test_multi_bce_by_hand_on_two_pixels():
    """The same image, one plane (offset (0, 1), t = [0, 1]), logits 0: S = 1, n = 2, w = (2 - 1 + 1)/(1 + 1) = 1, every
    term ln 2: loss = (1*ln2 + ln2)/2 = ln 2.  Gradient / scale: (s - y)*(w or 1) = [1/2, -1/2], plus
    L1*(-(n + 2)/(S + 1)^2)*s(1-s) = ln2 * (-1) * 1/4 on both."""
    truth = np.array([[[0, 1]]], np.int32)
    x = np.zeros((1, 1, 1, 2), np.float32)
    loss, grad = labels.multi_bce_loss(x, "offset", [(0, 1)], truth, None)
    ln2 = math.log(2.0)
    assert abs(loss - ln2) <= 2 * U
    np.testing.assert_allclose(grad[0, 0, 0], [0.5 * (0.5 - ln2 / 4), 0.5 * (-0.5 - ln2 / 4)], rtol=4 * U, atol=0)


def ignore_case():
    H, W = 4, 6
    rng = np.random.default_rng(3)
    x = (rng.random((1, 3, H, W)) * 8 - 4).astype(np.float32)
    truth = np.array([[[0, 0, 1, 1, 2, 2],
                       [0, 0, 1, 1, 2, 2],
                       [9, 9, 0, 0, -5, 0],
                       [0, 0, 0, 0, 0, 0]]], np.int32)
    return x, truth, [[2, 255]]


def test_ignore_class_is_absent_from_the_sums_and_has_gradient_zero():
    x, truth, tcs = ignore_case()
    ignored = truth[0] == 2
    for terms in (True, False):
        sums = labels.plane_sums(x[0], "class", None, truth[0], tcs[0], 2, terms=terms)
        assert sums.shape == (16,) and sums[-1] == 24 - ignored.sum() == 20
        # the same sums from the kept pixels alone, laid out as one row
        kept = labels.plane_sums(x[0][:, ~ignored].reshape(3, 1, -1), "class", None, truth[0][~ignored].reshape(1, -1),
                                 tcs[0], 2, terms=terms)
        assert np.array_equal(sums, kept)
        assert (sums[9:15] == 0).all() if not terms else (sums[9:15] > 0).any()
    assert sums[6:9].tolist() == [16.0, 0.0, 4.0]                        # Z: class 0, class 1 (nobody), class 2 (label 1)
    for loss_fn in (lambda: labels.dice_loss(x, "class", None, truth, tcs),
                    lambda: labels.dice_loss(x, "class", None, truth, tcs, mode="0"),
                    lambda: labels.multi_bce_loss(x, "class", None, truth, tcs)):
        loss, grad = loss_fn()
        assert (grad[0][:, ignored] == 0).all() and (grad[0][:, ~ignored] != 0).all()
    # the offset part knows no classes
    a = labels.plane_sums(x[0][:2], "offset", [(0, 1), (-1, 0)], truth[0], tcs[0], 2)
    b = labels.plane_sums(x[0][:2], "offset", [(0, 1), (-1, 0)], truth[0], None, 0)
    assert np.array_equal(a, b) and a[-1] == 24


@pytest.mark.parametrize("part", ["class", "offset"])
def test_three_steps_reproduce_the_direct_statements(golden, part):
    """plane_sums (added over the batch for Dice, per image for MBCE), plane_coeffs and plane_grad give the gradient of
    dice_loss / multi_bce_loss: two statements written independently of each other.  Both are float64 on the same sums
    (both sides use math.fsum), so they differ by the rounding of a handful of operations: 16 u of the magnitude."""
    x, offs, truth, tcs = part_inputs(golden, part)
    x = x.astype(np.float32)
    B, P, H, W = x.shape
    for mode in ("1", "0"):
        comp = mode == "0"
        loss, grad = labels.dice_loss(x, part, offs, truth, tcs, mode=mode, smooth=0.5)
        sums = sum(labels.plane_sums(x[b], part, offs, truth[b], tcs[b], len(tcs[b]), complement=comp, terms=False)
                   for b in range(B))
        coeffs, value = labels.plane_coeffs("dice", sums, smooth=0.5, complement=comp)
        assert (coeffs[2:] == 0).all() and abs(value - loss) <= 16 * U * P
        got = np.stack([labels.plane_grad(x[b], part, offs, truth[b], tcs[b], len(tcs[b]), coeffs, 3.0, complement=comp)
                        for b in range(B)])
        err = np.abs(got - 3.0 * grad).max() / np.abs(3.0 * grad).max()
        print("%s dice mode %s: three steps against the direct statement, relative to the greatest element %.3g" % (part, mode, err))
        assert err <= 16 * U
    loss, grad = labels.multi_bce_loss(x, part, offs, truth, tcs)
    total, got = 0.0, []
    for b in range(B):
        sums = labels.plane_sums(x[b], part, offs, truth[b], tcs[b], len(tcs[b]), terms=True)
        coeffs, value = labels.plane_coeffs("mbce", sums, pixels=H * W, scale=1.0 / (B * P * H * W))
        total += value
        got.append(labels.plane_grad(x[b], part, offs, truth[b], tcs[b], len(tcs[b]), coeffs))
    err = np.abs(np.stack(got) - grad).max() / np.abs(grad).max()
    print("%s mbce: three steps against the direct statement, relative %.3g; loss %.17g against %.17g" % (part, err, total, loss))
    assert err <= 16 * U and abs(total - loss) <= 16 * U * loss
    with pytest.raises(ValueError):
        labels.plane_coeffs("mbce", sums, pixels=H * W, complement=True)
    with pytest.raises(ValueError):
        labels.plane_coeffs("dice", sums, smooth=0.0)


PROTOTYPES = {"mn_plane_sums_device": 15, "mn_plane_coeffs_device": 12, "mn_plane_grad_device": 16}


def test_entry_points_are_declared_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from mergenet_amd import segmenter as seg
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = seg.load_library()
    for name, count in PROTOTYPES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, "include/mergenet_hip.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == count and name in seg.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == count
        for i, a in enumerate(args):                                     # int, double and pointer arguments line up
            want = ctypes.c_double if a.startswith("double ") else ctypes.c_int if a.startswith("int ") else None
            if want is not None:
                assert fn.argtypes[i] is want, (name, a)
            else:
                assert "*" in a and fn.argtypes[i] in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)), (name, a)
    for const in ("MN_PART_CLASS", "MN_PART_OFFSET", "MN_PLANE_COMPLEMENT", "MN_PLANE_TERMS", "MN_CRIT_DICE", "MN_CRIT_MBCE"):
        m = re.search(r"#define\s+%s\s+(\d+)" % const, code)
        assert m and int(m.group(1)) == getattr(seg, const), const
    assert (labels.PART_CLASS, labels.PART_OFFSET) == (seg.MN_PART_CLASS, seg.MN_PART_OFFSET)
    assert "mn_kernels_planeloss.h" in open(os.path.join(ROOT, "mergenet_amd", "csrc", "Makefile")).read()
    assert all(callable(getattr(seg.Merger, n)) for n in ("plane_sums", "plane_coeffs", "plane_grad"))
    from mergenet_amd import losses
    nn = __import__("torch").nn
    assert issubclass(losses.MaskDiceLoss, nn.Module) and issubclass(losses.MaskMultiBCELoss, nn.Module)
