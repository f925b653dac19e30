"""labels.mask_ce -- the numpy statement of Merger.mask_ce -- against the reference's own criterion
(CrossEntropyLossOneHot: F.cross_entropy(input, target.max(1)[1]) in float64 on one-hot target planes built the way
the reference's datasets build them), on hand-computed cases, on the ignore class and on the offset part's targets;
the C ABI of mn_mask_ce_device (no GPU)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from mergenet_amd import labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, G = 4, 3
TRUTH_CLASSES = (2, 1, 3)                          # no ignore class: every class lies in 0..C-1


def offsets_for(shape):
    H, W = shape
    return [(0, 1), (2, -1), (0, 0), (-1, -2), (H, 0), (0, W)]


def offset_targets(mask, offset_list):
    """The target planes of utils/dataset.py:259-277 (np.roll, then the rows and columns that rolled around set to 1)."""
    h, w = mask.shape
    target = np.ndarray(shape=(len(offset_list), h, w), dtype="bool")
    for n, (i, j) in enumerate(offset_list):
        rolled = np.roll(np.roll(mask, -i, axis=0), -j, axis=1)
        target[n] = rolled == mask
        if i < 0:
            target[n, :-i, :] = 1
        elif i > 0:
            target[n, -i:, :] = 1
        if j < 0:
            target[n, :, :-j] = 1
        elif j > 0:
            target[n, :, -j:] = 1
    return target


def class_targets(class_mask, num_classes):
    """utils/dataset.py:419-429: plane n is (mask == n)."""
    return np.stack([class_mask == n for n in range(num_classes)])


def image(shape):
    H, W = shape
    rng = np.random.default_rng(100 * H + W)
    truth = np.zeros((H, W), np.int32)
    for k in range(1, G + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        truth[max(0, y - H // 4):y + H // 4 + 1, max(0, x - W // 4):x + W // 4 + 1] = k
    cl = (rng.random((C, H, W)) * 16 - 8).astype(np.float32)
    sl = (rng.random((len(offsets_for(shape)), H, W)) * 16 - 8).astype(np.float32)
    return cl, sl, truth


def one_hot_criterion(logits, planes):
    """CrossEntropyLossOneHot of utils/loss.py:24-35 in float64: (loss, gradient) for one image."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(logits.astype(np.float64))[None].requires_grad_()
    target = torch.from_numpy(planes.astype(np.float64))[None]
    loss = F.cross_entropy(x, target.max(1)[1])
    loss.backward()
    return loss.item(), x.grad[0].numpy()


@pytest.mark.parametrize("shape", [(3, 5), (7, 64), (33, 70)])
def test_statement_equals_the_reference_criterion(shape):
    H, W = shape
    cl, sl, truth = image(shape)
    offs = offsets_for(shape)
    class_mask = np.concatenate([[0], TRUTH_CLASSES])[truth]
    parts = [("class", cl, None, class_targets(class_mask, C)),
             ("offset", sl, offs, offset_targets(truth, offs))]
    for part, x, off, planes in parts:
        want_loss, want_grad = one_hot_criterion(x, planes)
        sums, grad = labels.mask_ce(x, part, off, truth, TRUTH_CLASSES, G, 1.0 / (H * W))
        assert sums.dtype == np.float64 and sums.shape == (2,) and grad.shape == x.shape and grad.dtype == np.float64
        assert sums[1] == H * W
        mean = sums[0] / (H * W)
        worst = np.abs(grad - want_grad).max() / np.abs(want_grad).max()
        print("%s part: mean %.17g against %.17g; gradient within %.3g of its greatest element" %
              (part, mean, want_loss, worst))
        assert abs(mean - want_loss) <= 1e-12 * want_loss
        # 1e-12 relative, element by element, plus the reference's own rounding at the target plane: torch forms
        # softmax - 1 from a float64 softmax that is within half an ulp of 1 where the target dominates, an absolute
        # 2^-53 (times the scale of the mean, twice for the rounding of its logsumexp) on a difference that may be
        # 1e-7; the statement takes that element as -(sum of the other exponentials) / sum, where nothing cancels.
        err, bound = np.abs(grad - want_grad), 1e-12 * np.abs(want_grad) + 2.0 ** -52 / (H * W)
        print("  greatest gradient error %.3g of its bound" % (err / bound).max())
        assert (err <= bound).all()
        # and the target planes agree with the election of max(1)[1]
        target, keep = labels.ce_targets(part, x.shape[0], off, truth, TRUTH_CLASSES, G)
        import torch
        assert np.array_equal(target, torch.from_numpy(planes.astype(np.float64)).max(0)[1].numpy()) and keep.all()


def test_one_pixel_at_zero():
    for P, target_class in ((2, 1), (5, 3), (9, 0)):
        truth = np.array([[1]], np.int32)
        sums, grad = labels.mask_ce(np.zeros((P, 1, 1), np.float32), "class", None, truth, [target_class], 1, scale=0.25)
        assert abs(sums[0] - math.log(P)) <= 4e-16 and sums[1] == 1.0
        want = np.full(P, 1.0 / P)
        want[target_class] -= 1.0
        np.testing.assert_allclose(grad.reshape(-1), want * 0.25, rtol=4e-16, atol=0)
    # the offset part: the neighbour of (0, 1) is outside the image ("same"), so plane 0 is the target
    sums, grad = labels.mask_ce(np.zeros((2, 1, 1), np.float32), "offset", [(0, 1), (0, 0)], truth, None, 0)
    assert abs(sums[0] - math.log(2.0)) <= 2e-16 and sums[1] == 1.0 and grad.reshape(-1).tolist() == [-0.5, 0.5]


def test_one_plane_has_term_zero_and_gradient_zero():
    rng = np.random.default_rng(2)
    x = (rng.random((1, 4, 6)) * 16 - 8).astype(np.float32)
    truth = rng.integers(0, 3, (4, 6)).astype(np.int32)
    sums, grad = labels.mask_ce(x, "class", None, truth, [0, 0], 2, scale=3.0)
    assert sums.tolist() == [0.0, 24.0] and (grad == 0).all() and not np.signbit(grad).any()
    sums, grad = labels.mask_ce(x, "offset", [(0, 1)], truth, None, 0, scale=3.0)
    assert sums.tolist() == [0.0, 24.0] and (grad == 0).all()


def test_a_far_maximum_keeps_its_small_term():
    """Where the target is the maximum and the other planes lie far below, the term is about r = sum of the other
    exponentials: log(1 + r) would give 0 below 2^-53."""
    x = np.array([60.0, -20.0, -20.0], np.float32).reshape(3, 1, 1)
    sums, grad = labels.mask_ce(x, "class", None, np.zeros((1, 1), np.int32), None, 0)
    r = 2.0 * math.exp(-80.0)
    assert r < 2.0 ** -53 and abs(sums[0] - r) <= 1e-15 * r
    np.testing.assert_allclose(grad.reshape(-1), [-r, r / 2, r / 2], rtol=1e-15, atol=0)


def test_ignore_class_and_labels_out_of_range():
    H, W, P = 4, 6, 3
    rng = np.random.default_rng(3)
    x = (rng.random((P, H, W)) * 8 - 4).astype(np.float32)
    truth = np.array([[0, 0, 1, 1, 2, 2],
                      [0, 0, 1, 1, 2, 2],
                      [9, 9, 0, 0, -5, 0],
                      [0, 0, 0, 0, 0, 0]], np.int32)
    sums, grad = labels.mask_ce(x, "class", None, truth, [2, 255], 2)
    ignored = truth == 2
    assert sums[1] == H * W - ignored.sum() == 20
    assert (grad[:, ignored] == 0).all() and (grad[:, ~ignored] != 0).all()
    # the sum is the sum over the kept pixels alone
    keep_only = labels.mask_ce(x[:, ~ignored].reshape(P, 1, -1), "class", None, truth[~ignored].reshape(1, -1), [2, 255], 2)
    assert abs(sums[0] - keep_only[0][0]) <= 1e-13 * sums[0] and keep_only[0][1] == 20
    # with every class in range nothing is ignored
    other = labels.mask_ce(x, "class", None, truth, [2, 1], 2)
    assert other[0][1] == H * W and np.array_equal(other[1][:, ~ignored], grad[:, ~ignored])
    # labels 9 and -5 are outside 0..G: class 0
    as_zero = np.where((truth == 9) | (truth == -5), 0, truth)
    zero = labels.mask_ce(x, "class", None, as_zero, [2, 255], 2)
    assert np.array_equal(grad, zero[1]) and sums[0] == zero[0][0]
    target, keep = labels.ce_targets("class", P, None, truth, [2, 255], 2)
    assert (target[truth == 1] == 2).all() and (target[(truth != 1) & ~ignored] == 0).all()
    assert np.array_equal(keep, ~ignored)
    # a negative class is ignored like one that is too large
    neg = labels.mask_ce(x, "class", None, truth, [2, -1], 2)
    assert np.array_equal(neg[1], grad) and np.array_equal(neg[0], sums)
    # the offset part does not know about classes, and takes labels 9 and -5 as labels of their own
    offs = [(0, 1), (-1, 0), (0, 0)]
    a = labels.mask_ce(x, "offset", offs, truth, [2, 255], 2)
    b = labels.mask_ce(x, "offset", offs, truth, None, 0)
    assert a[0][1] == H * W and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[1], labels.mask_ce(x, "offset", offs, as_zero, None, 0)[1])
    # no instances at all: every pixel is class 0
    none = labels.mask_ce(x, "class", None, truth, None, 0)
    assert none[0][1] == H * W
    assert (none[1][0] < 0).all() and (none[1][1:] > 0).all()


def test_offset_part_targets():
    H, W = 12, 20
    truth = np.zeros((H, W), np.int32)
    truth[2:7, 3:9] = 1
    truth[5:11, 8:15] = 2
    truth[6, 8] = 3                                   # a single pixel: every neighbour carries another label
    offs = [(0, 1), (1, 0), (-1, -1), (0, -2), (2, 2)]
    y, keep = labels.plane_targets("offset", len(offs), offs, truth, None, 0)
    target, keep2 = labels.ce_targets("offset", len(offs), offs, truth, None, 0)
    assert keep.all() and keep2.all()
    none = ~y.any(axis=0)
    assert none.any() and none[6, 8], "some pixel has no plane with target 1"
    assert (target[none] == 0).all()
    first = np.argmax(y, axis=0)
    assert len(set(first[~none].tolist())) >= 3, "the first target-1 plane takes at least three values"
    assert np.array_equal(target, np.where(none, 0, first))
    for k in range(len(offs)):                        # ... and it is the FIRST: no earlier plane has target 1
        at = (target == k) & ~none
        assert y[k][at].all() and not y[:k][:, at].any()
    # the election of max(1)[1] on the dataset's planes
    import torch
    planes = torch.from_numpy(offset_targets(truth, offs).astype(np.float64))
    assert np.array_equal(target, planes.max(0)[1].numpy())
    # offsets of H rows / W columns leave the image from every pixel: target 1 on plane 0 everywhere
    far = [(H, 0), (0, W), (0, 1)]
    target, _ = labels.ce_targets("offset", 3, far, truth, None, 0)
    assert (target == 0).all()
    target, _ = labels.ce_targets("offset", 3, [(0, 1), (0, -W), (-H, 0)], truth, None, 0)
    assert set(np.unique(target).tolist()) == {0, 1}
    rng = np.random.default_rng(5)
    x = (rng.random((3, H, W)) * 16 - 8).astype(np.float32)
    sums, grad = labels.mask_ce(x, "offset", far, truth, None, 0)
    assert (grad[0] < 0).all() and (grad[1:] > 0).all() and sums[1] == H * W


def test_entry_point_is_declared_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from mergenet_amd import abi, segmenter as seg
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mn_mask_ce_device\s*\(([^)]*)\)\s*;", code)
    assert m, "include/mergenet_hip.h does not declare mn_mask_ce_device"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 16
    assert "mn_mask_ce_device" in abi.SIGNATURES and "mn_mask_ce_device" in seg.EXPORTS
    fn = seg.load_library().mn_mask_ce_device
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
    for i, a in enumerate(args):                                         # int, float and pointer arguments line up
        want = ctypes.c_float if a.startswith("float ") else ctypes.c_int if a.startswith("int ") else None
        if want is not None:
            assert fn.argtypes[i] is want, a
        else:
            assert "*" in a and fn.argtypes[i] in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)), a
    assert args[2].startswith("int dtype") and args[5].startswith("int part") and args[12] == "float scale"
    assert args[14] == "int accumulate"
    assert "mn_kernels_celoss.h" in open(os.path.join(ROOT, "mergenet_amd", "csrc", "Makefile")).read()
    assert callable(seg.Merger.mask_ce)
    from mergenet_amd import losses
    assert issubclass(losses.MaskCELoss, __import__("torch").nn.Module)
