"""Seeded inputs of the matching tests (tests/test_match.py, tests/test_gpu_match.py): pairs of small block masks
with classes, quantised scores, crowd flags and an area range, and a replay of a matching result that counts the
events the tests want their inputs to contain."""
import functools

import numpy as np

from mergenet_amd import labels

THRESHOLDS = np.concatenate([[0.1, 0.25], labels.COCO_THRESHOLDS])     # ties among disjoint instances need IoU < 0.5
AREA_RANGES = [(0.0, 1e10), (3.0, 24.0)]


def expand(coarse, block, H, W):
    m = np.repeat(np.repeat(coarse, block[0], axis=0), block[1], axis=1)[:H, :W]
    return np.ascontiguousarray(m, np.int32)


def block_mask(rng, H, W, n_labels, background=0.3):
    """Cells of 1-2 x 1-2 pixels (blocks of 1-4 pixels), each with a label of 0..n_labels; returns (mask, cells,
    cell size)."""
    block = tuple(int(v) for v in rng.integers(1, 3, 2))
    shape = (-(-H // block[0]), -(-W // block[1]))
    coarse = rng.integers(1, n_labels + 1, shape) if n_labels else np.zeros(shape, np.int64)
    coarse = np.where(rng.random(shape) < background, 0, coarse)
    return expand(coarse, block, H, W), coarse, block


def make_case(seed, H, W, K, G, n_classes=3, nan_score=False, derived=None, area_range=None):
    """One image: truth and prediction masks (the prediction either a relabelled, partly redrawn copy of the truth,
    so that IoUs above 0.5 occur, or drawn on its own: by the seed's parity unless `derived` says), classes, scores
    with ties, crowd flags, an area range (by the seed unless given)."""
    rng = np.random.default_rng(seed)
    truth, cells, block = block_mask(rng, H, W, G)
    if (seed % 2 == 0 if derived is None else derived) and K and G:
        relabel = np.concatenate([[0], rng.integers(1, K + 1, G)])
        redraw = rng.random(cells.shape) < 0.25
        coarse = np.where(redraw, rng.integers(0, K + 1, cells.shape), relabel[cells])
        pred = expand(coarse, block, H, W)
    else:
        pred = block_mask(rng, H, W, K)[0]
    scores = (rng.integers(0, 4, K) / 4).astype(np.float32)               # quantised: equal scores occur
    if nan_score and K >= 3:
        scores[K // 2] = np.nan
    case = dict(pred=pred, truth=truth, K=K, G=G,
                pred_classes=rng.integers(1, n_classes + 1, K).astype(np.int32),
                truth_classes=rng.integers(1, n_classes + 1, G).astype(np.int32),
                scores=scores, crowd=(rng.random(G) < 0.2).astype(np.uint8),
                area_range=AREA_RANGES[(seed // 2) % 2] if area_range is None else area_range)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def small_case(seed):
    """The cases of the CPU test: 4-10 x 6-16 pixels, 2-6 instances on either side, 2 classes."""
    rng = np.random.default_rng(10_000 + seed)
    H, W = int(rng.integers(4, 11)), int(rng.integers(6, 17))
    K, G = int(rng.integers(2, 7)), int(rng.integers(2, 7))
    return make_case(seed, H, W, K, G, n_classes=2)


def want(case, form="closed", with_scores=True):
    table = labels.overlap_table(case["pred"], case["truth"], case["K"], case["G"])
    return table, labels.match_instances(table, case["pred_classes"], case["truth_classes"],
                                         scores=case["scores"] if with_scores else None, crowd=case["crowd"],
                                         thresholds=THRESHOLDS, area_range=case["area_range"], form=form)


def events(case, res, with_scores=True):
    """Replays a result in detection order and counts: detections whose best candidates tied in IoU, matches with
    iou == threshold, crowd instances matched more than once, detections matched to an ignored truth instance."""
    n = dict(tie=0, at_threshold=0, crowd_twice=0, to_ignored=0)
    iou, ign, pm = res["iou"], res["truth_ignore"], res["pred_match"]
    crowd = case["crowd"].astype(bool)
    order = labels.detection_order(case["scores"] if with_scores else None, case["K"])
    for ti, t in enumerate(THRESHOLDS):
        taken = np.zeros(case["G"], bool)
        for d in order:
            m = int(pm[ti, d]) - 1
            if m < 0:
                continue
            cand = ((case["truth_classes"] == case["pred_classes"][d]) & (~taken | crowd) &
                    (iou[d] >= min(t, 1 - 1e-10)) & (ign == ign[m]))
            n["tie"] += int((iou[d][cand] == iou[d, m]).sum() > 1)
            n["at_threshold"] += int(iou[d, m] == t)
            n["to_ignored"] += int(ign[m])
            taken[m] = True
        for j in np.flatnonzero(crowd):
            n["crowd_twice"] += int((pm[ti] == j + 1).sum() > 1)
    return n
