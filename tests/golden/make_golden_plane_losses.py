#!/usr/bin/env python
"""Generate tests/golden/plane_losses_v1.npz: the reference's SoftDiceLoss and MultiBCEWithLogitsLoss on a small batch.

    python tests/golden/make_golden_plane_losses.py --reference /path/to/the/reference/tree

At generation time only, this imports utils/loss.py from the reference tree and runs its criteria on CPU float64
tensors: B = 2 images of 12x20, a 4-plane class part (every truth class in range) and a 5-plane offset part, logits
uniform in -6..6, blob label masks that differ per image, target planes built by this file's own statement of
utils/dataset.py:259-277 (offsets) and :419-429 (classes).  Recorded for each part:
  dice1_loss / dice1_grad, dice0_loss / dice0_grad   SoftDiceLoss(mode='1') and (mode='0'): loss and autograd gradient
  mbce_loss                                          MultiBCEWithLogitsLoss under torch.no_grad()
  mbce_grad_composition                              NOT the reference's module: a current torch refuses to
      differentiate binary_cross_entropy_with_logits with respect to its weight, so the module raises under autograd.
      This is the autograd gradient of the GENERATOR'S composition (weight * bce_terms).mean() with the reference's
      weight expression (utils/loss.py:70-74) kept in the graph; mbce_loss_composition is its value.
The fixture holds DATA only.  tests/test_plane_losses.py holds labels.dice_loss / multi_bce_loss to it.  A GPU box never
runs this.
"""
import argparse
import importlib.util
import os
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
B, H, W, C = 2, 12, 20, 4
OFFSETS = [(0, 1), (1, 0), (2, 3), (30, 0), (-3, -2)]
TRUTH_CLASSES = [[1, 2, 3, 1, 0], [3, 3, 1, 2, 0]]


def inputs():
    rng = np.random.default_rng(20261)
    class_logits = rng.random((B, C, H, W)) * 12 - 6
    offset_logits = rng.random((B, len(OFFSETS), H, W)) * 12 - 6
    truth = np.zeros((B, H, W), np.int32)
    for b in range(B):
        for k in range(1, len(TRUTH_CLASSES[b]) + 1):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            truth[b, max(0, y - 2):y + 3, max(0, x - 3):x + 4] = k
    return class_logits, offset_logits, truth


def sameness_targets(truth):
    """utils/dataset.py:259-277: 1 where the neighbour carries the same label or lies outside the image."""
    out = np.ones((len(OFFSETS), H, W), np.float64)
    for k, (di, dj) in enumerate(OFFSETS):
        for r in range(H):
            for c in range(W):
                rr, cc = r + di, c + dj
                if 0 <= rr < H and 0 <= cc < W and truth[rr, cc] != truth[r, c]:
                    out[k, r, c] = 0.0
    return out


def class_targets(truth, truth_classes):
    """utils/dataset.py:419-429: plane n is (class mask == n)."""
    truth_class = np.concatenate([[0], truth_classes]).astype(np.int64)[truth]
    return (np.arange(C)[:, None, None] == truth_class[None]).astype(np.float64)


def composition(x, target):
    """(weight * bce_terms).mean() with the weight expression of utils/loss.py:70-74, the weight in the graph."""
    n = x.shape[2] * x.shape[3]
    s = torch.sigmoid(x).sum(dim=-1).sum(dim=-1)
    weight = ((n - s + 1) / (s + 1))[:, :, None, None].expand(target.size())
    weight = weight * target + (1 - target)
    terms = torch.nn.functional.binary_cross_entropy_with_logits(x, target, reduction="none")
    return (weight * terms).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds utils/loss.py)")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(args.reference, "utils", "loss.py"))
    loss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loss)

    class_logits, offset_logits, truth = inputs()
    targets = {"class": np.stack([class_targets(truth[b], TRUTH_CLASSES[b]) for b in range(B)]),
               "offset": np.stack([sameness_targets(truth[b]) for b in range(B)])}
    assert targets["class"].sum(1).min() == 1 and 0 < targets["offset"].mean() < 1
    out = dict(class_logits=class_logits, offset_logits=offset_logits, truth=truth,
               truth_classes=np.asarray(TRUTH_CLASSES, np.int32), offsets=np.asarray(OFFSETS, np.int32),
               mbce_grad_is="composition of the generator: (weight * bce_terms).mean(), weight in the graph")
    for part, logits in (("class", class_logits), ("offset", offset_logits)):
        t = torch.from_numpy(targets[part])
        for mode in ("1", "0"):
            x = torch.from_numpy(logits).requires_grad_()
            value = loss.SoftDiceLoss(mode=mode, smooth=1)(x, t)
            value.backward()
            out["%s_dice%s_loss" % (part, mode)] = np.float64(value.item())
            out["%s_dice%s_grad" % (part, mode)] = x.grad.numpy().copy()
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["%s_mbce_loss" % part] = np.float64(loss.MultiBCEWithLogitsLoss()(torch.from_numpy(logits), t).item())
        x = torch.from_numpy(logits).requires_grad_()
        value = composition(x, t)
        value.backward()
        out["%s_mbce_loss_composition" % part] = np.float64(value.item())
        out["%s_mbce_grad_composition" % part] = x.grad.numpy().copy()
        out["%s_targets" % part] = targets[part].astype(np.uint8)
    np.savez_compressed(os.path.join(HERE, "plane_losses_v1.npz"), **out)


if __name__ == "__main__":
    main()
