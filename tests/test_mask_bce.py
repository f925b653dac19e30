"""labels.mask_bce -- the numpy statement of Merger.mask_bce -- against the reference's own criterion
(torch.nn.BCEWithLogitsLoss in float64 on target planes built the way the reference's datasets build them), on a
hand-computed case and on the ignore class; the C ABI of mn_mask_bce_device (no GPU)."""
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
    return [(0, 0), (0, 1), (2, -1), (-1, -2), (H, 0), (0, W)]


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


@pytest.mark.parametrize("shape", [(3, 5), (7, 64), (33, 70)])
def test_statement_equals_the_reference_criterion(shape):
    import torch
    H, W = shape
    cl, sl, truth = image(shape)
    offs = offsets_for(shape)
    O = len(offs)
    class_mask = np.concatenate([[0], TRUTH_CLASSES])[truth]
    t_cls = torch.from_numpy(class_targets(class_mask, C).astype(np.float64))
    t_ofs = torch.from_numpy(offset_targets(truth, offs).astype(np.float64))
    assert t_ofs[0].all() and t_ofs[4].all() and t_ofs[5].all() and not t_ofs[1].all()
    x_cls = torch.from_numpy(cl.astype(np.float64)).requires_grad_()
    x_ofs = torch.from_numpy(sl.astype(np.float64)).requires_grad_()
    crit = torch.nn.BCEWithLogitsLoss()
    cls_loss, ofs_loss = crit(x_cls, t_cls), crit(x_ofs, t_ofs)
    (cls_loss + ofs_loss).backward()

    sums, gc, gs = labels.mask_bce(cl, sl, offs, truth, TRUTH_CLASSES, G, 1.0 / (C * H * W), 1.0 / (O * H * W))
    assert sums.dtype == np.float64 and sums.shape == (2 + O,) and gc.shape == (C, H, W) and gs.shape == (O, H, W)
    assert sums[1 + O] == H * W
    mean_cls, mean_ofs = sums[0] / (C * H * W), sums[1:1 + O].sum() / (O * H * W)
    print("class mean %.17g against %.17g, offset mean %.17g against %.17g" %
          (mean_cls, cls_loss.item(), mean_ofs, ofs_loss.item()))
    assert abs(mean_cls - cls_loss.item()) <= 1e-12 * cls_loss.item()
    assert abs(mean_ofs - ofs_loss.item()) <= 1e-12 * ofs_loss.item()
    np.testing.assert_allclose(gc, x_cls.grad.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(gs, x_ofs.grad.numpy(), rtol=1e-12, atol=0)


def test_one_pixel_at_zero():
    truth = np.array([[1]], np.int32)
    cl = np.zeros((2, 1, 1), np.float32)
    sl = np.zeros((1, 1, 1), np.float32)
    sums, gc, gs = labels.mask_bce(cl, sl, [(0, 1)], truth, [1], 1, scale_class=0.25, scale_same=3.0)
    ln2 = math.log(2.0)
    assert abs(sums[0] - 2 * ln2) <= 4e-16 and abs(sums[1] - ln2) <= 2e-16 and sums[2] == 1.0
    assert gc.reshape(-1).tolist() == [0.5 * 0.25, -0.5 * 0.25]          # class 1 is the target: (0.5 - 1) * scale
    assert gs.reshape(-1).tolist() == [-0.5 * 3.0]                       # the neighbour is outside: "same", y = 1


def test_ignore_class_and_labels_out_of_range():
    H, W = 4, 6
    rng = np.random.default_rng(3)
    cl = (rng.random((3, H, W)) * 8 - 4).astype(np.float32)
    sl = (rng.random((2, H, W)) * 8 - 4).astype(np.float32)
    offs = [(0, 1), (-1, 0)]
    truth = np.array([[0, 0, 1, 1, 2, 2],
                      [0, 0, 1, 1, 2, 2],
                      [9, 9, 0, 0, -5, 0],
                      [0, 0, 0, 0, 0, 0]], np.int32)
    sums, gc, gs = labels.mask_bce(cl, sl, offs, truth, [2, 255], 2)
    ignored = truth == 2
    assert sums[-1] == H * W - ignored.sum() == 20
    assert (gc[:, ignored] == 0).all() and (gc[:, ~ignored] != 0).all()
    # the class sum is the sum over the kept pixels alone
    keep_only = labels.mask_bce(cl[:, ~ignored].reshape(3, 1, -1), None, [], truth[~ignored].reshape(1, -1), [2, 255], 2)
    assert abs(sums[0] - keep_only[0][0]) <= 1e-13 * sums[0]
    # the offset planes do not know about classes: the same with every label kept
    other = labels.mask_bce(cl, sl, offs, truth, [2, 1], 2)
    assert np.array_equal(sums[1:3], other[0][1:3]) and np.array_equal(gs, other[2])
    assert other[0][-1] == H * W
    # labels 9 and -5 are outside 0..G: class 0 for the class planes, labels of their own for the offsets
    as_zero = np.where((truth == 9) | (truth == -5), 0, truth)
    zero = labels.mask_bce(cl, sl, offs, as_zero, [2, 255], 2)
    assert np.array_equal(gc, zero[1]) and sums[0] == zero[0][0]
    assert not np.array_equal(gs, zero[2])
    want_same = np.ones((H, W), bool)
    want_same[2, 1] = want_same[2, 3] = want_same[2, 4] = False          # (0, 1): 9|0, 0|-5, -5|0
    want_same[0, 1] = want_same[0, 3] = want_same[1, 1] = want_same[1, 3] = False     # 0|1 and 1|2, twice
    assert want_same[:, 5].all()                                         # the neighbour is outside the image: "same"
    sig = 1.0 / (1.0 + np.exp(-sl[0].astype(np.float64)))
    np.testing.assert_allclose(gs[0], sig - want_same, rtol=1e-15, atol=1e-16)
    # no instances at all: every pixel is class 0
    none = labels.mask_bce(cl, sl, offs, truth, None, 0)
    assert none[0][-1] == H * W and np.array_equal(none[2], gs)


def test_parts_may_be_absent():
    cl, sl, truth = image((7, 64))
    offs = offsets_for((7, 64))
    both = labels.mask_bce(cl, sl, offs, truth, TRUTH_CLASSES, G)
    only_c = labels.mask_bce(cl, None, [], truth, TRUTH_CLASSES, G)
    only_o = labels.mask_bce(None, sl, offs, truth, TRUTH_CLASSES, G)
    assert only_c[0].shape == (2,) and only_c[0][0] == both[0][0] and only_c[0][1] == both[0][-1]
    assert np.array_equal(only_c[1], both[1]) and only_c[2].shape == (0, 7, 64)
    assert np.array_equal(only_o[0][1:-1], both[0][1:-1]) and only_o[0][0] == 0.0 and only_o[0][-1] == 0.0
    assert np.array_equal(only_o[2], both[2])


def test_entry_point_is_declared_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from mergenet_amd import segmenter as seg
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mn_mask_bce_device\s*\(([^)]*)\)\s*;", code)
    assert m, "include/mergenet_hip.h does not declare mn_mask_bce_device"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 19
    assert "mn_mask_bce_device" in seg.EXPORTS
    fn = seg.load_library().mn_mask_bce_device
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 19
    for i, a in enumerate(args):                                         # int, float and pointer arguments line up
        want = ctypes.c_float if a.startswith("float ") else ctypes.c_int if a.startswith("int ") else None
        if want is not None:
            assert fn.argtypes[i] is want, a
        else:
            assert "*" in a and fn.argtypes[i] in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)), a
    assert args[3].startswith("int dtype") and args[14] == "float scale_class" and args[17] == "int accumulate"
    assert "mn_kernels_loss.h" in open(os.path.join(ROOT, "mergenet_amd", "csrc", "Makefile")).read()
    assert callable(seg.Merger.mask_bce)
    from mergenet_amd import losses
    assert issubclass(losses.MaskBCELoss, __import__("torch").nn.Module)
