#!/usr/bin/env python
"""Generate tests/golden/map_scores_v1.npz: the reference's own scoring classes on one small image.

    python tests/golden/make_golden_scores.py --reference /path/to/the/reference/tree

At generation time only, this imports utils/score.py from the reference tree and runs runningScore.update and
offsetIoU.update on CPU torch tensors, the way utils/train_utils.py drives them: the prediction planes, the one-hot
class planes of the truth and the sameness targets built by the rule of utils/dataset.py:259-277.  The fixture holds
DATA only: the inputs (24x40, C = 4, O = 5 with an offset that leaves the image and a negative pair, random float32
maps, a blob label mask with 6 instances) and what the reference accumulated and reported.  tests/test_map_scores.py
holds labels.map_scores / class_scores / offset_iou to it.  A GPU box never runs this.
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, C = 24, 40, 4
OFFSETS = [(0, 1), (1, 0), (2, 3), (30, 0), (-3, -2)]
TRUTH_CLASSES = [1, 2, 3, 1, 0, 2]


def inputs():
    rng = np.random.default_rng(20260)
    class_probs = rng.random((C, H, W), dtype=np.float32)
    same_probs = rng.random((len(OFFSETS), H, W), dtype=np.float32)
    truth = np.zeros((H, W), np.int32)
    for k in range(1, len(TRUTH_CLASSES) + 1):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        truth[max(0, y - 4):y + 5, max(0, x - 6):x + 7] = k
    return class_probs, same_probs, truth


def sameness_targets(truth):
    """utils/dataset.py:259-277: 1 where the neighbour carries the same label or lies outside the image."""
    out = np.ones((len(OFFSETS), H, W), np.float32)
    for k, (di, dj) in enumerate(OFFSETS):
        for r in range(H):
            for c in range(W):
                rr, cc = r + di, c + dj
                if 0 <= rr < H and 0 <= cc < W and truth[rr, cc] != truth[r, c]:
                    out[k, r, c] = 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds utils/score.py)")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_score", os.path.join(args.reference, "utils", "score.py"))
    score = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(score)

    class_probs, same_probs, truth = inputs()
    truth_class = np.concatenate([[0], TRUTH_CLASSES]).astype(np.int64)[truth]
    one_hot = (np.arange(C)[:, None, None] == truth_class[None]).astype(np.float32)
    targets = sameness_targets(truth)

    running = score.runningScore(C, list(range(C)))
    running.update(torch.from_numpy(class_probs)[None], torch.from_numpy(one_hot)[None])
    offs = score.offsetIoU(OFFSETS)
    offs.update(torch.from_numpy(same_probs)[None], torch.from_numpy(targets)[None])
    class_summary, class_iou = running.get_scores()
    intersection, union = offs.intersection.copy(), offs.union.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        offset_iou, offset_mean = offs.get_scores()

    np.savez_compressed(
        os.path.join(HERE, "map_scores_v1.npz"),
        class_probs=class_probs, same_probs=same_probs, truth=truth,
        truth_classes=np.asarray(TRUTH_CLASSES, np.int32), offsets=np.asarray(OFFSETS, np.int32),
        confusion_matrix=running.confusion_matrix, intersection=intersection, union=union,
        class_summary=np.asarray([class_summary[k] for k in ("overall_acc", "mean_acc", "freq_acc", "mean_IU")]),
        class_iou=np.asarray([class_iou[c] for c in range(C)]),
        offset_iou=np.asarray(offset_iou, np.float64), offset_mean=np.float64(offset_mean))


if __name__ == "__main__":
    main()
