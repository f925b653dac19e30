"""Comparing label maps up to a permutation of the labels (plain numpy helpers).

Instance ids have no canonical numbering: the reference numbers instances in hash-map iteration
order (``utils/csegment/segment.cc:503``), this library in ascending surviving pixel id.  Results
are therefore compared as partitions plus per-instance class.

Also the numpy statements of the instance table and the small-instance filter (``instance_table``,
``filter_instances``), the checkers of ``Merger.instance_table`` / ``Merger.filter_instances``, of the per-instance
confidence (``instance_scores``, the checker of ``Merger.instance_scores``), and those of the
comparison with the ground truth (``overlap_table``, ``instance_iou``, ``match_instances``), the checkers of
``Merger.overlap_table`` / ``Merger.match_instances``, of the dataset-level evaluation (``eval_records``,
``coco_accumulate``, ``coco_summarize``: the checkers of ``Merger.dataset_eval``), and of the scores of the network's maps themselves
(``map_scores``, the checker of ``Merger.map_scores``, with the reference's summaries ``class_scores`` and
``offset_iou``), and of the sameness targets of a label mask (``sameness_targets``, the checker of
``Merger.sameness_targets``).
"""

from __future__ import annotations

import math

import numpy as np


def canonical(labels: np.ndarray) -> np.ndarray:
    """Relabel by first occurrence in row-major order (0, 1, 2, ...)."""
    flat = np.asarray(labels).reshape(-1)
    _, first, inv = np.unique(flat, return_index=True, return_inverse=True)
    order = np.argsort(np.argsort(first))
    return order[inv].reshape(np.asarray(labels).shape).astype(np.int64)


def same_partition(a: np.ndarray, b: np.ndarray) -> bool:
    return bool(np.array_equal(canonical(a), canonical(b)))


def partition_mismatch(a: np.ndarray, b: np.ndarray) -> int:
    """Number of pixels whose part in ``a`` is not matched 1:1 to a part of ``b``."""
    ca, cb = canonical(a).reshape(-1), canonical(b).reshape(-1)
    pairs, counts = np.unique(np.stack([ca, cb], 1), axis=0, return_counts=True)
    best_a = {}
    for (x, y), n in zip(pairs, counts):
        if n > best_a.get(x, (None, 0))[1]:
            best_a[x] = (y, n)
    used = {}
    good = 0
    for x, (y, n) in best_a.items():
        if y in used:
            continue
        size_a = int((ca == x).sum())
        size_b = int((cb == y).sum())
        if size_a == n and size_b == n:
            good += n
            used[y] = x
    return int(ca.size - good)


def masks_equivalent(mask_a, classes_a, mask_b, classes_b) -> bool:
    """Instance masks equal up to a permutation of labels 1..K, with equal per-label class."""
    ma, mb = np.asarray(mask_a), np.asarray(mask_b)
    if ma.shape != mb.shape or len(classes_a) != len(classes_b):
        return False
    if not np.array_equal(ma == 0, mb == 0):
        return False
    if not same_partition(ma, mb):
        return False
    flat_a, flat_b = ma.reshape(-1), mb.reshape(-1)
    _, idx = np.unique(flat_a, return_index=True)
    for i in idx:
        la, lb = int(flat_a[i]), int(flat_b[i])
        if la == 0:
            continue
        if classes_a[la - 1] != classes_b[lb - 1]:
            return False
    return True


def agreement(mask_a, mask_b) -> int:
    """Pixels on which two label maps agree under the best one-to-one matching of their labels by
    overlap (greedy on the contingency table, largest overlap first)."""
    a = np.asarray(mask_a).astype(np.int64).reshape(-1)
    b = np.asarray(mask_b).astype(np.int64).reshape(-1)
    cont = np.zeros((int(a.max()) + 1, int(b.max()) + 1), np.int64)
    np.add.at(cont, (a, b), 1)
    agree = 0
    for _ in range(min(cont.shape)):
        i, j = np.unravel_index(int(np.argmax(cont)), cont.shape)
        if cont[i, j] <= 0:
            break
        agree += int(cont[i, j])
        cont[i, :] = -1
        cont[:, j] = -1
    return agree


# ---- instance table and small-instance filter: the numpy checkers of the device path ----------------------
# (the role rle.binary_mask_counts plays for the RLE strings: written straight from the definitions)

def instance_table(mask: np.ndarray, num_instances: int) -> np.ndarray:
    """int32 [K,5]: row k-1 = {area, x_min, y_min, x_max, y_max} of the pixels with label k, maxima inclusive;
    {0, W, H, -1, -1} for a label without pixels.  Labels outside 1..K are ignored."""
    m = np.asarray(mask)
    H, W = m.shape
    table = np.empty((int(num_instances), 5), np.int32)
    for k in range(1, int(num_instances) + 1):
        ys, xs = np.nonzero(m == k)
        if ys.size == 0:
            table[k - 1] = (0, W, H, -1, -1)
        else:
            table[k - 1] = (ys.size, xs.min(), ys.min(), xs.max(), ys.max())
    return table


def filter_instances(mask: np.ndarray, class_table, num_instances: int, table: np.ndarray, min_area: int,
                     scores=None, min_score=None):
    """Keep label k iff table[k-1][0] >= min_area (and, where scores are given, scores[k-1] >= min_score, -inf
    when min_score is None: a NaN score fails the comparison and is dropped); the kept
    labels get 1..K' in ascending old label, every other pixel 0.  Returns (mask int32, class table int32 [K] with
    -1 from K' on, scores float32 [K'] or None, table int32 [K',5], K', remap int32 [K+1] old -> new, 0 = dropped)."""
    m = np.asarray(mask)
    K = int(num_instances)
    table = np.asarray(table)
    classes = np.asarray(class_table)
    remap = np.zeros(K + 1, np.int32)
    kept = []
    for k in range(1, K + 1):
        keep = table[k - 1][0] >= min_area
        if scores is not None:
            keep = keep and bool(scores[k - 1] >= (-np.inf if min_score is None else min_score))
        if keep:
            kept.append(k)
            remap[k] = len(kept)
    out = np.zeros(m.shape, np.int32)
    for k in kept:
        out[m == k] = remap[k]
    new_classes = np.full(K, -1, np.int32)
    new_table = np.empty((len(kept), 5), np.int32)
    for k in kept:
        new_classes[remap[k] - 1] = classes[k - 1]
        new_table[remap[k] - 1] = table[k - 1]
    new_scores = None
    if scores is not None:
        new_scores = np.asarray([scores[k - 1] for k in kept], np.float32)
    return out, new_classes, new_scores, new_table, len(kept), remap


# ---- per-instance confidence: the numpy statement of Merger.instance_scores --------------------------------------
# (Object::GetNoBackLogprob, segment.h:109, summed over the pixels the result mask gives the instance)

EPS32 = float(np.finfo(np.float32).eps)          # MN_EPS32: the clip of the loaders is [eps, 1 - eps] in float32


def loaded_class_probs(class_maps, logits: bool = False, clip: bool = False) -> np.ndarray:
    """float32 [C,H,W]: the probability every kernel sees when it loads an element of the class maps (``mn_ld_class``).

    The element is widened exactly to float32.  With ``logits`` it is a logit and the loader takes
    ``1 / (1 + exp(-x))``: here each operation in float64 and ONE rounding to float32 (the device takes it in
    float32, within a few units in the last place of this value).  The clip to ``[eps32, 1 - eps32]`` (float32
    min / max, ``mn_clip``) applies where the loader applies it: always for logits and for 16-bit maps, for float32
    probabilities only when the caller asks (``clip_inputs``).  numpy has no bfloat16: such maps come as their float32
    widening, with ``clip=True``; a ``numpy.float16`` array is clipped by its dtype."""
    x = np.asarray(class_maps)
    lowp = x.dtype == np.float16
    p = x.astype(np.float32)
    if logits:
        with np.errstate(over="ignore"):
            p = (1.0 / (1.0 + np.exp(-p.astype(np.float64)))).astype(np.float32)
    if clip or logits or lowp:
        one = np.float32(1.0)
        p = np.minimum(np.maximum(p, np.float32(EPS32)), one - np.float32(EPS32)).astype(np.float32)
    return p


def instance_scores(class_maps, mask, class_table, num_instances: int, logits: bool = False,
                    clip: bool = False) -> np.ndarray:
    """float64 [K]: ``score[k-1]`` = the sum over the pixels with ``mask == k`` of ``log p[class_table[k-1]] - log p[0]``,
    with p = :func:`loaded_class_probs` ``(class_maps, logits, clip)`` and the logarithms in float64 (each class's sum
    is the correctly rounded sum of its terms, ``math.fsum``, then ONE subtraction).  A label without pixels scores 0; labels outside
    1..K are ignored; K = 0 gives an empty array.  The class of instance k is the table's word, whatever the maps say."""
    p = loaded_class_probs(class_maps, logits, clip)
    C, H, W = p.shape
    m = np.asarray(mask).astype(np.int64)
    if m.shape != (H, W):
        raise ValueError("the class maps and the mask differ in size")
    K = int(num_instances)
    table = np.asarray(class_table).astype(np.int64).reshape(-1)[:K]
    if table.size != K or (K and (table.min() < 0 or table.max() >= C)):
        raise ValueError("class_table: K classes in 0..C-1 are needed")
    out = np.zeros(K, np.float64)

    def log_sum(values):         # (math.log: the C library's, one and the same on every host; log 0 = -inf)
        return math.fsum(math.log(v) if v > 0.0 else -math.inf for v in values.astype(np.float64).tolist())

    for k in range(1, K + 1):
        sel = m == k
        if sel.any():
            out[k - 1] = log_sum(p[table[k - 1]][sel]) - log_sum(p[0][sel])
    return out


# ---- overlap table, IoU and matching against the ground truth: the numpy statements of the device path ------
# (Merger.overlap_table / Merger.match_instances; COCOeval.computeIoU and evaluateImg with maxDets >= K, restated:
# pycocotools is not needed.  Arrays per instance are indexed label - 1, table rows and columns by the label.)

COCO_THRESHOLDS = np.linspace(0.5, 0.95, 10)


def overlap_table(pred: np.ndarray, truth: np.ndarray, num_pred: int, num_truth: int) -> np.ndarray:
    """int32 [K+1, G+1]: entry [p][g] = number of pixels with prediction label p and truth label g.  A label outside
    0..K (prediction) or 0..G (truth) counts as 0.  Row sums are the prediction areas, column sums the truth areas."""
    K, G = int(num_pred), int(num_truth)
    p = np.asarray(pred).astype(np.int64).reshape(-1)
    g = np.asarray(truth).astype(np.int64).reshape(-1)
    if p.shape != g.shape:
        raise ValueError("the two masks differ in size")
    p = np.where((p < 0) | (p > K), 0, p)
    g = np.where((g < 0) | (g > G), 0, g)
    table = np.zeros((K + 1, G + 1), np.int64)
    np.add.at(table, (p, g), 1)
    return table.astype(np.int32)


def _crowd_flags(crowd, G):
    return np.zeros(G, bool) if crowd is None else np.asarray(crowd).astype(bool).reshape(-1)[:G]


def instance_iou(table: np.ndarray, crowd=None) -> np.ndarray:
    """float64 [K, G]: iou[k-1][j-1] = inter / (area_p[k] + area_g[j] - inter) with inter = table[k][j], area_p the
    row sums and area_g the column sums; inter / area_p[k] for a crowd truth instance; 0 where the denominator is 0.
    One division of exact integers."""
    t = np.asarray(table).astype(np.int64)
    K, G = t.shape[0] - 1, t.shape[1] - 1
    area_p = t.sum(axis=1)[1:].astype(np.float64)
    area_g = t.sum(axis=0)[1:].astype(np.float64)
    inter = t[1:, 1:].astype(np.float64)
    den = area_p[:, None] + area_g[None, :] - inter
    den = np.where(_crowd_flags(crowd, G)[None, :], np.broadcast_to(area_p[:, None], (K, G)), den)
    out = np.zeros((K, G), np.float64)
    np.divide(inter, den, out=out, where=den != 0)
    return out


def detection_order(scores, K: int):
    """Labels - 1 of the detections in the order they are taken: descending score, equal scores in ascending label, a
    NaN score last; label order without scores."""
    if scores is None:
        return list(range(K))
    s = [float(v) for v in np.asarray(scores).reshape(-1)[:K]]
    return sorted(range(K), key=lambda k: (1, 0.0, k) if s[k] != s[k] else (0, -s[k], k))


def match_instances(table, pred_classes, truth_classes, scores=None, crowd=None, thresholds=None,
                    area_range=(0.0, 1e10), form: str = "closed") -> dict:
    """COCO's greedy matching of one image for every IoU threshold (``None``: the ten of COCO), from the overlap
    table.  Returns ``{"pred_match": int32 [T,K] (truth label or 0), "truth_match": int32 [T,G] (prediction label
    or 0), "pred_ignore": bool [T,K], "truth_ignore": bool [G], "iou": float64 [K,G]}``.

    ``form="loop"`` is COCOeval.evaluateImg's loop over the truth instances in truth order (non-ignored first, then
    ignored, each in ascending label; ``if iou < best: continue`` keeps the LAST of equals; it stops at the first
    ignored instance once a non-ignored one is held).  ``form="closed"`` states its outcome: of the candidates --
    d's class, unmatched at this threshold or crowd, IoU >= min(t, 1 - 1e-10) -- the non-ignored one of greatest IoU
    if there is any, else the ignored one of greatest IoU, the greatest label among equals.  With K == 0 or G == 0
    there is nothing to match and every output is zero."""
    t = np.asarray(table).astype(np.int64)
    K, G = t.shape[0] - 1, t.shape[1] - 1
    th = COCO_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64).reshape(-1)
    T = len(th)
    area_lo, area_hi = float(area_range[0]), float(area_range[1])
    res = {"pred_match": np.zeros((T, K), np.int32), "truth_match": np.zeros((T, G), np.int32),
           "pred_ignore": np.zeros((T, K), bool), "truth_ignore": np.zeros(G, bool),
           "iou": np.zeros((K, G), np.float64)}
    if K == 0 or G == 0:
        return res
    pc = np.asarray(pred_classes).reshape(-1)[:K]
    tc = np.asarray(truth_classes).reshape(-1)[:G]
    is_crowd = _crowd_flags(crowd, G)
    area_p = t.sum(axis=1)[1:].astype(np.float64)
    area_g = t.sum(axis=0)[1:].astype(np.float64)
    ign = is_crowd | (area_g < area_lo) | (area_g > area_hi)
    iou = instance_iou(t, is_crowd)
    order = detection_order(scores, K)
    pm, tm, pi = res["pred_match"], res["truth_match"], res["pred_ignore"]
    truth_order = [j for j in range(G) if not ign[j]] + [j for j in range(G) if ign[j]]
    for ti in range(T):
        lo = min(float(th[ti]), 1 - 1e-10)
        for d in order:
            m = -1
            if form == "loop":
                best = lo
                for j in truth_order:
                    if tc[j] != pc[d]:
                        continue
                    if tm[ti, j] > 0 and not is_crowd[j]:
                        continue
                    if m > -1 and not ign[m] and ign[j]:
                        break
                    if iou[d, j] < best:
                        continue
                    best = iou[d, j]
                    m = j
            elif form == "closed":
                cand = (tc == pc[d]) & ((tm[ti] == 0) | is_crowd) & (iou[d] >= lo)
                for group in (~ign, ign):
                    c = np.flatnonzero(cand & group)
                    if c.size:
                        m = int(c[iou[d, c] == iou[d, c].max()].max())
                        break
            else:
                raise ValueError("form: 'loop' or 'closed'")
            if m == -1:
                continue
            pm[ti, d] = m + 1
            tm[ti, m] = d + 1
            pi[ti, d] = ign[m]
    outside = (area_p < area_lo) | (area_p > area_hi)
    pi |= (pm == 0) & outside[None, :]
    res["truth_ignore"] = ign
    res["iou"] = iou
    return res


# ---- the dataset-level evaluation: the numpy statements of Merger.dataset_eval -------------------------------
# (COCOeval.evaluate's per-image cut to maxDets, accumulate and summarize, restated.  The contract is pinned to these
# statements and to hand-computed cases, not to pycocotools, which is not a dependency.)

COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))   # all, small, medium, large
COCO_MAX_DETS = (1, 10, 100)
COCO_REC_THRESHOLDS = np.linspace(0.0, 1.0, 101)


def _eval_params(thresholds, area_ranges, max_dets):
    th = COCO_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64).reshape(-1)
    ar = np.asarray(COCO_AREA_RANGES if area_ranges is None else area_ranges, np.float64).reshape(-1, 2)
    md = [int(m) for m in max_dets]
    if not 1 <= len(th) <= 16:
        raise ValueError("thresholds: 1 to 16 values")
    if not 1 <= len(ar) <= 4:
        raise ValueError("area_ranges: 1 to 4 (lo, hi) pairs")
    if not 1 <= len(md) <= 4 or md[0] < 1 or any(b <= a for a, b in zip(md, md[1:])):
        raise ValueError("max_dets: 1 to 4 ascending positive values")
    return th, ar, md


def eval_records(table, pred_classes, truth_classes, scores=None, crowd=None, thresholds=None, area_ranges=None,
                 max_det: int = 100, num_classes=None, image: int = 0) -> dict:
    """What one image adds to the evaluation log.  The detections are taken in ``detection_order``; ``rank[d]`` is the
    number of detections of d's class before d; a detection with ``rank >= max_det`` (the largest maxDets) takes no
    part in the matching -- it is given a class that no truth instance has, which is how it matches nothing and
    holds no truth instance (COCOeval cuts to ``dt[:maxDet]`` per image and category before it matches).  One
    ``match_instances`` per area range: a truth instance is ignored when it is crowd or its area is outside the
    range, a detection without a match when its own area is.
    Returns, per detection IN DETECTION ORDER: ``classes`` int32 [K], ``scores`` float32 [K] (1 without scores,
    egs/cityscape/local/segment.py:181), ``rank`` int32 [K], ``image`` int32 [K], ``matched`` and ``ignored`` bool
    [A,T,K]; and ``npig`` int64 [C,A]: the truth instances of each class in 0..C-1 that the range does not ignore
    (``None`` without ``num_classes``)."""
    t = np.asarray(table).astype(np.int64)
    K, G = t.shape[0] - 1, t.shape[1] - 1
    th, ar, _ = _eval_params(thresholds, area_ranges, (max_det,))
    T, A = len(th), len(ar)
    pc = np.asarray(pred_classes).reshape(-1)[:K].astype(np.int64)
    tc = np.asarray(truth_classes).reshape(-1)[:G].astype(np.int64)
    order = detection_order(scores, K)
    rank = np.zeros(K, np.int32)
    seen = {}
    for d in order:
        rank[d] = seen.get(int(pc[d]), 0)
        seen[int(pc[d])] = int(rank[d]) + 1
    unused = min([int(v) for v in pc] + [int(v) for v in tc] + [0]) - 1
    matching_classes = np.where(rank >= max_det, unused, pc)
    area_p = t.sum(axis=1)[1:].astype(np.float64)
    area_g = t.sum(axis=0)[1:].astype(np.float64)
    is_crowd = _crowd_flags(crowd, G)
    matched = np.zeros((A, T, K), bool)
    ignored = np.zeros((A, T, K), bool)
    npig = None if num_classes is None else np.zeros((int(num_classes), A), np.int64)
    for a, (lo, hi) in enumerate(ar):
        if K and G:
            res = match_instances(t, matching_classes, tc, scores=scores, crowd=crowd, thresholds=th,
                                  area_range=(lo, hi))
            matched[a] = res["pred_match"][:, order] > 0
            ignored[a] = res["pred_ignore"][:, order]
        else:
            ignored[a] = ((area_p < lo) | (area_p > hi))[order][None, :]
        if npig is not None:
            counted = ~(is_crowd | (area_g < lo) | (area_g > hi)) & (tc >= 0) & (tc < npig.shape[0])
            np.add.at(npig[:, a], tc[counted], 1)
    sc = np.ones(K, np.float32) if scores is None else np.asarray(scores, np.float32).reshape(-1)[:K]
    return {"classes": pc[order].astype(np.int32), "scores": sc[order], "rank": rank[order],
            "image": np.full(K, int(image), np.int32), "matched": matched, "ignored": ignored, "npig": npig}


def coco_accumulate(images, num_classes: int, rec_thresholds=None, max_dets=COCO_MAX_DETS, num_thresholds=None,
                    num_area_ranges=None, form: str = "closed") -> dict:
    """COCOeval.accumulate over the ``eval_records`` of the images, in the order they were added.  Returns
    ``{"precision": float64 [T,R,C,A,M], "recall": float64 [T,C,A,M], "scores": float64 [T,R,C,A,M], "npig": int64
    [C,A]}``.  T and A are those of the records (``num_thresholds`` / ``num_area_ranges`` say them for an empty list:
    10 and 4 by default).  Per class k, range a and ``max_dets[m]``: the records of class k with ``rank < max_dets[m]``,
    sorted stably by descending score, NaN last; ``tp = cumsum(matched & ~ignored)``, ``fp = cumsum(~matched &
    ~ignored)``, ``rc = tp / npig[k][a]``, ``pr = tp / (fp + tp + np.spacing(1))``, ``pr[i] = max(pr[i:])``; per recall
    threshold the ``pr`` and score at the first index with ``rc >= threshold``, 0 where there is none; ``recall`` is
    the last ``rc``, 0 without records; everything of (k, a) is -1 where ``npig[k][a] == 0``.

    ``form="loop"`` is written the way COCOeval.accumulate is: concatenate, ``argsort(-scores, kind="mergesort")``,
    cumsum, the envelope ``for``, ``searchsorted`` (whose index is taken per threshold: where pycocotools stops at
    the first threshold out of reach, every later one is out of reach too when the thresholds ascend).
    ``form="closed"`` states the outcome: suffix maximum, first index with ``rc >= threshold``."""
    if form not in ("loop", "closed"):
        raise ValueError("form: 'loop' or 'closed'")
    images = list(images)
    C = int(num_classes)
    rec = COCO_REC_THRESHOLDS if rec_thresholds is None else np.asarray(rec_thresholds, np.float64).reshape(-1)
    _, _, md = _eval_params(None, None, max_dets)
    if images:
        A, T = images[0]["matched"].shape[:2]
    else:
        T = 10 if num_thresholds is None else int(num_thresholds)
        A = 4 if num_area_ranges is None else int(num_area_ranges)
    if any(img["matched"].shape[:2] != (A, T) or img["npig"].shape != (C, A) for img in images):
        raise ValueError("the records differ in their thresholds, area ranges or classes")
    R, M = len(rec), len(md)
    npig = np.zeros((C, A), np.int64)
    for img in images:
        npig += img["npig"]
    precision = -np.ones((T, R, C, A, M))
    recall = -np.ones((T, C, A, M))
    scores = -np.ones((T, R, C, A, M))
    for k in range(C):
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for m, max_det in enumerate(md):
                sel = [(img["classes"] == k) & (img["rank"] < max_det) for img in images]
                sc = np.concatenate([img["scores"][s] for img, s in zip(images, sel)] + [np.zeros(0, np.float32)])
                dtm = np.concatenate([img["matched"][a][:, s] for img, s in zip(images, sel)] +
                                     [np.zeros((T, 0), bool)], axis=1)
                dtig = np.concatenate([img["ignored"][a][:, s] for img, s in zip(images, sel)] +
                                      [np.zeros((T, 0), bool)], axis=1)
                nd = len(sc)
                if form == "loop":
                    inds = np.argsort(-sc, kind="mergesort")
                else:
                    inds = np.asarray(sorted(range(nd), key=lambda i: (1, 0.0) if sc[i] != sc[i] else (0, -float(sc[i]))),
                                      np.int64)
                sc, dtm, dtig = sc[inds], dtm[:, inds], dtig[:, inds]
                tp_sum = np.cumsum(dtm & ~dtig, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~dtm & ~dtig, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    rc = tp / npig[k, a]
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    q, ss = np.zeros(R), np.zeros(R)
                    if form == "loop":
                        pr = pr.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        for ri, pi in enumerate(np.searchsorted(rc, rec, side="left")):
                            if pi < nd:
                                q[ri] = pr[pi]
                                ss[ri] = sc[pi]
                    else:
                        env = np.maximum.accumulate(pr[::-1])[::-1]
                        for ri, thr in enumerate(rec):
                            at = np.flatnonzero(rc >= thr)
                            if at.size:
                                q[ri] = env[at[0]]
                                ss[ri] = sc[at[0]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return {"precision": precision, "recall": recall, "scores": scores, "npig": npig}


def eval_summary_names(max_dets=COCO_MAX_DETS):
    """The keys of ``coco_summarize`` in COCOeval.summarize's order: twelve with three maxDets."""
    return (["AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large"] + ["AR@%d" % int(m) for m in max_dets] +
            ["AR_small", "AR_medium", "AR_large"])


def coco_summarize(result, thresholds=None, max_dets=COCO_MAX_DETS, classes=None) -> dict:
    """The numbers of COCOeval.summarize for iouType 'segm' from what ``coco_accumulate`` (or the device) gave: each
    the mean of the entries greater than -1 over ``classes`` (default 1..C-1: class 0 is the background), -1 where
    there is none.  AP, AP50, AP75, AP_small / _medium / _large: ``precision`` at the largest maxDets, for area range
    0 ("all") and ranges 1, 2, 3; AR@m for each of ``max_dets`` at range 0; AR_small / _medium / _large: ``recall`` at
    the largest maxDets.  AP50 / AP75 take the threshold EQUAL to 0.5 / 0.75 and are -1 without it; the small,
    medium and large entries are -1 with fewer than four area ranges."""
    precision, recall = np.asarray(result["precision"]), np.asarray(result["recall"])
    T, _, C, A, M = precision.shape
    th = COCO_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64).reshape(-1)
    md = [int(m) for m in max_dets]
    if len(th) != T or len(md) != M:
        raise ValueError("thresholds / max_dets: not those of the result")
    cls = np.arange(1, C) if classes is None else np.asarray(list(classes), np.int64).reshape(-1)
    if cls.size and (cls.min() < 0 or cls.max() >= C):
        raise ValueError("classes: within 0..%d" % (C - 1))

    def mean(s):
        s = s[s > -1]
        return float(s.mean()) if s.size else -1.0

    def ap(a, at=None):
        if a >= A or (at is not None and not (th == at).any()):
            return -1.0
        s = precision[:, :, cls, a, M - 1]
        return mean(s if at is None else s[th == at])

    def ar(a, m):
        return mean(recall[:, cls, a, m]) if a < A else -1.0

    values = ([ap(0), ap(0, 0.5), ap(0, 0.75), ap(1), ap(2), ap(3)] + [ar(0, m) for m in range(M)] +
              [ar(1, M - 1), ar(2, M - 1), ar(3, M - 1)])
    return dict(zip(eval_summary_names(md), values))


# ---- uniform groups of the sweep's lean form: the numpy twin of the rule in mn_cc_sign ----------------------

def uniform_groups(pos_bits: np.ndarray, offsets) -> np.ndarray:
    """bool [ceil(N / 64)]: group g is the pixels [64 g, 64 g + 64) of the image in linear order.  It is uniform iff
    the offset list holds (0, +1) -- as offset k -- and bit k of the positive mask is set for its first 63 pixels;
    a last group of fewer than 64 pixels never is.  `pos_bits`: [H, W] positive out-edge masks (bit k = offset k,
    only in-bounds edges set: the bit of a row's last column is never set, so no group across a row's end is
    uniform)."""
    bits = np.asarray(pos_bits).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    n = bits.size
    groups = (n + 63) // 64
    flags = np.zeros(groups, bool)
    offs = [(int(i), int(j)) for (i, j) in offsets]
    if (0, 1) not in offs:
        return flags
    k = offs.index((0, 1))
    link = ((bits >> k) & 1).astype(bool)
    full = n // 64
    flags[:full] = link[: full * 64].reshape(full, 64)[:, :63].all(axis=1)
    return flags


# ---- the network's maps against the ground truth: the numpy statement of Merger.map_scores ----------------------
# (what runningScore.update and offsetIoU.update of utils/score.py accumulate per image, from the label mask instead of
# target planes; class_scores and offset_iou are their get_scores)

def map_scores(class_probs, same_probs, offsets, truth, truth_classes, num_truth: int, logits: bool = False):
    """(confusion int64 [C,C], sums float64 [3,O]) of one image.

    p is the element widened exactly to float32; with ``logits`` the float32 sigmoid ``1 / (1 + exp(-x))`` of that.
    No clip, no same_different_bias.  Predicted class: ``argmax`` of p over the C class planes (the lowest index among
    the greatest; NaN in a map is outside the contract -- numpy takes the first NaN, the device never takes one).  Truth class: 0 for truth label 0 and for a label outside 0..num_truth, ``truth_classes[g - 1]``
    for label g; a pixel whose truth class lies outside 0..C-1 is left out of the confusion matrix
    (``runningScore._fast_hist``); ``confusion[t][q]`` counts the others by truth class t and predicted class q.
    Per offset k = (di, dj) a pixel is different when (r + di, c + dj) is inside the image and carries another truth
    label (the labels as they stand, utils/dataset.py:259-277; outside the image is "same"); with d = 1 - p in float32:
    ``sums[0][k]`` = sum of d over the different pixels, ``sums[1][k]`` = sum of d over all pixels, ``sums[2][k]`` =
    the number of different pixels.  The sums are float64: the correctly rounded sum of the terms (``math.fsum``),
    which any float64 summation of these n non-negative terms meets within n * 2^-53, relative."""
    cp = np.asarray(class_probs).astype(np.float32)
    sp = np.asarray(same_probs).astype(np.float32)
    if logits:
        with np.errstate(over="ignore"):
            one = np.float32(1.0)
            cp = (one / (one + np.exp(-cp, dtype=np.float32))).astype(np.float32)
            sp = (one / (one + np.exp(-sp, dtype=np.float32))).astype(np.float32)
    C, H, W = cp.shape
    offs = np.asarray(offsets, np.int64).reshape(-1, 2)
    O = offs.shape[0]
    t = np.asarray(truth).astype(np.int64)
    if t.shape != (H, W) or sp.shape != (O, H, W):
        raise ValueError("the maps, the offsets and the truth mask differ in size")
    G = int(num_truth)
    by_label = np.zeros(G + 1, np.int64)
    if G:
        by_label[1:] = np.asarray(truth_classes).astype(np.int64).reshape(-1)[:G]
    tcls = by_label[np.where((t < 0) | (t > G), 0, t)]
    pred = cp.argmax(axis=0)
    keep = (tcls >= 0) & (tcls < C)
    confusion = np.bincount(C * tcls[keep] + pred[keep], minlength=C * C).reshape(C, C).astype(np.int64)
    sums = np.zeros((3, O), np.float64)
    for k, (di, dj) in enumerate(offs.tolist()):
        d = (np.float32(1.0) - sp[k]).astype(np.float64)
        diff = np.zeros((H, W), bool)
        r0, r1 = max(0, -di), min(H, H - di)
        c0, c1 = max(0, -dj), min(W, W - dj)
        if r0 < r1 and c0 < c1:
            diff[r0:r1, c0:c1] = t[r0:r1, c0:c1] != t[r0 + di:r1 + di, c0 + dj:c1 + dj]
        sums[0, k] = math.fsum(d[diff].tolist())
        sums[1, k] = math.fsum(d.reshape(-1).tolist())
        sums[2, k] = float(diff.sum())
    return confusion, sums


def class_scores(confusion):
    """The summaries ``runningScore.get_scores`` reports (utils/score.py:34-55) from a confusion matrix whose rows are
    the truth classes: ``({"overall_acc", "mean_acc", "freq_acc", "mean_IU"}, per-class IoU float64 [C])``.

    With ``hit[c]`` the diagonal, ``truth[c]`` the row totals, ``pred[c]`` the column totals and ``n`` their total:
    recall[c] = hit / truth, IoU[c] = hit / (truth + pred - hit); ``overall_acc`` = sum(hit) / n, ``mean_acc`` and
    ``mean_IU`` average recall and IoU over the classes where they are defined (0 / 0 is NaN and left out),
    ``freq_acc`` weighs the IoU of every class that occurs in the truth by its share truth / n."""
    m = np.asarray(confusion).astype(np.float64)
    hit, truth, pred = m.diagonal(), m.sum(axis=1), m.sum(axis=0)
    n = truth.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        recall = hit / truth
        iou = hit / (truth + pred - hit)
        overall = hit.sum() / n
        share = truth / n
        occurs = share > 0
        summary = {"overall_acc": overall, "mean_acc": np.nanmean(recall),
                   "freq_acc": float(np.dot(share[occurs], iou[occurs])), "mean_IU": np.nanmean(iou)}
    return summary, iou


def offset_iou(sums):
    """``offsetIoU.get_scores`` (utils/score.py:93-96) of the totals: (iou float64 [O], their mean), with
    intersection = sums[0] and union = sums[1] + sums[2] - sums[0]; 0 / 0 is NaN, as the reference leaves it."""
    s = np.asarray(sums, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = s[0] / (s[1] + s[2] - s[0])
    return iou, iou.mean()


# ---- the training criterion from the label mask: the numpy statement of Merger.mask_bce ---------------------------
# (torch.nn.BCEWithLogitsLoss of the reference's recipes on the class planes and the offset planes, as sums, and its
# gradient; the targets are those of utils/dataset.py:259-277 and :419-429, looked up in the label mask)

def _truth_class_of(truth, truth_classes, num_truth: int):
    """Per pixel: 0 for label 0 and for a label outside 0..num_truth, ``truth_classes[g - 1]`` for label g."""
    t = np.asarray(truth).astype(np.int64)
    G = int(num_truth)
    by_label = np.zeros(G + 1, np.int64)
    if G:
        by_label[1:] = np.asarray(truth_classes).astype(np.int64).reshape(-1)[:G]
    return by_label[np.where((t < 0) | (t > G), 0, t)]


def sameness_targets(mask, offsets) -> np.ndarray:
    """float32 [O,H,W]: the sameness targets of an instance mask as utils/dataset.py:259-277 defines them, the
    statement of ``Merger.sameness_targets``: for offset (i, j) the mask rolled by (-i, -j) compared with itself --
    as plain integers, negative (ignore) labels included -- and the rows and columns whose neighbour the roll
    wrapped round forced to 1; an offset that reaches past the image gives all ones."""
    m = np.asarray(mask)
    out = np.zeros((len(offsets),) + m.shape, np.float32)
    for n, (i, j) in enumerate(offsets):
        i, j = int(i), int(j)
        rolled = np.roll(np.roll(m, -i, axis=0), -j, axis=1)
        t = (rolled == m)
        if i < 0:
            t[:-i, :] = 1
        elif i > 0:
            t[-i:, :] = 1
        if j < 0:
            t[:, :-j] = 1
        elif j > 0:
            t[:, -j:] = 1
        out[n] = t
    return out


def _different(t, di: int, dj: int):
    """bool [H,W]: (r + di, c + dj) is inside the image and carries another label than (r, c)."""
    H, W = t.shape
    diff = np.zeros((H, W), bool)
    r0, r1 = max(0, -di), min(H, H - di)
    c0, c1 = max(0, -dj), min(W, W - dj)
    if r0 < r1 and c0 < c1:
        diff[r0:r1, c0:c1] = t[r0:r1, c0:c1] != t[r0 + di:r1 + di, c0 + dj:c1 + dj]
    return diff


def mask_bce(class_logits, same_logits, offsets, truth, truth_classes, num_truth: int, scale_class: float = 1.0,
             scale_same: float = 1.0):
    """(sums float64 [2+O], grad_class float64 [C,H,W], grad_same float64 [O,H,W]) of one image.

    x is the element widened exactly to float32; everything after that is float64.  Truth class: as in
    :func:`map_scores`.  Target y of class plane q: 1 where the truth class is q; of offset plane k = (di, dj): 0
    where (r + di, c + dj) is inside the image and carries another truth label (the labels as they stand), else 1.
    Term: ``softplus(z) = logaddexp(0, z)`` with z = -x where y is 1 and x where it is 0 -- ``BCEWithLogitsLoss`` per
    element.  A pixel whose truth class lies outside 0..C-1 (an ignore class) has no class term and class gradient
    0; the offset planes take it as any other pixel.  ``sums[0]``: the class terms of the kept pixels over the C
    planes, ``sums[1 + k]``: the terms of offset plane k, ``sums[1 + O]``: the number of kept pixels; each the
    correctly rounded sum (``math.fsum``).  Gradient: ``(expit(x) - y) * scale``.  Either map may be None or have
    no planes."""
    t = np.asarray(truth).astype(np.int64)
    H, W = t.shape
    cl = np.zeros((0, H, W), np.float32) if class_logits is None else np.asarray(class_logits).astype(np.float32)
    sl = np.zeros((0, H, W), np.float32) if same_logits is None else np.asarray(same_logits).astype(np.float32)
    C, O = cl.shape[0], sl.shape[0]
    offs = np.asarray(offsets if O else [], np.int64).reshape(-1, 2)
    if cl.shape != (C, H, W) or sl.shape != (O, H, W) or offs.shape[0] != O:
        raise ValueError("the maps, the offsets and the truth mask differ in size")

    def expit(x):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))

    tcls = _truth_class_of(t, truth_classes, num_truth)
    keep = (tcls >= 0) & (tcls < C)
    sums = np.zeros(2 + O, np.float64)
    grad_class = np.zeros((C, H, W), np.float64)
    grad_same = np.zeros((O, H, W), np.float64)
    class_terms = []
    for q in range(C):
        x = cl[q].astype(np.float64)
        y = tcls == q
        class_terms.append(np.logaddexp(0.0, np.where(y, -x, x))[keep])
        grad_class[q] = np.where(keep, (expit(x) - y) * float(scale_class), 0.0)
    sums[0] = math.fsum(v for plane in class_terms for v in plane.tolist())      # (one plane's list at a time)
    for k, (di, dj) in enumerate(offs.tolist()):
        x = sl[k].astype(np.float64)
        y = ~_different(t, di, dj)
        sums[1 + k] = math.fsum(np.logaddexp(0.0, np.where(y, -x, x)).reshape(-1).tolist())
        grad_same[k] = (expit(x) - y) * float(scale_same)
    sums[1 + O] = float(keep.sum())
    return sums, grad_class, grad_same


# ---- Dice and weighted multi-BCE from the label mask: the numpy statements of Merger.plane_sums / plane_coeffs /
# plane_grad and of losses.MaskDiceLoss / MaskMultiBCELoss (SoftDiceLoss and MultiBCEWithLogitsLoss of utils/loss.py:
# 38-76 on the targets of utils/dataset.py:259-277 and :419-429, looked up in the label mask) -------------------------

PART_CLASS, PART_OFFSET = 0, 1


def _part_of(part) -> int:
    if part in (PART_CLASS, "class"):
        return PART_CLASS
    if part in (PART_OFFSET, "offset"):
        return PART_OFFSET
    raise ValueError("part: 'class' or 'offset'")


def _expit(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def plane_targets(part, num_planes: int, offsets, truth, truth_classes, num_truth: int):
    """(y bool [P,H,W], keep bool [H,W]): the targets of one part of the output and the pixels that take part.

    Class part: y of plane q is 1 where the truth class (:func:`map_scores`) is q; a pixel whose truth class lies
    outside 0..P-1 is ignored.  Offset part: y of plane k = (di, dj) is 0 where (r + di, c + dj) is inside the image
    and carries another truth label (the labels as they stand), else 1; every pixel takes part."""
    t = np.asarray(truth).astype(np.int64)
    H, W = t.shape
    P = int(num_planes)
    if _part_of(part) == PART_CLASS:
        tcls = _truth_class_of(t, truth_classes, num_truth)
        return np.stack([tcls == q for q in range(P)]), (tcls >= 0) & (tcls < P)
    offs = np.asarray(offsets, np.int64).reshape(-1, 2)
    if offs.shape[0] != P:
        raise ValueError("%d offsets for %d offset planes" % (offs.shape[0], P))
    return np.stack([~_different(t, di, dj) for di, dj in offs.tolist()]), np.ones((H, W), bool)


def plane_sums(logits, part, offsets, truth, truth_classes, num_truth: int, complement: bool = False,
               terms: bool = True):
    """float64 [5*P + 1] of one image: per plane p ``Q = sum q`` at [p], ``I = sum of q where z`` at [P + p], ``Z =
    number of z`` at [2P + p], ``L1 = sum of term where y`` at [3P + p], ``L0 = sum of term where !y`` at [4P + p]
    (both 0 without ``terms``), then the number of pixels that took part.

    x is the element widened exactly to float64 (float64 logits are taken as they are), and so is all else.  ``q = expit(x)``, ``z = y``;
    ``complement``: ``q = expit(-x)``, ``z = !y``.  ``term = logaddexp(0, -x where y else x)``.  Ignored pixels
    (:func:`plane_targets`) are left out of every sum.  Each sum is the correctly rounded one (``math.fsum``)."""
    x = np.asarray(logits).astype(np.float64)
    P = x.shape[0]
    y, keep = plane_targets(part, P, offsets, truth, truth_classes, num_truth)
    sums = np.zeros(5 * P + 1, np.float64)
    for p in range(P):
        xp, yp = x[p][keep], y[p][keep]
        q = _expit(-xp if complement else xp)
        z = ~yp if complement else yp
        sums[p] = math.fsum(q.tolist())
        sums[P + p] = math.fsum(q[z].tolist())
        sums[2 * P + p] = float(z.sum())
        if terms:
            term = np.logaddexp(0.0, np.where(yp, -xp, xp))
            sums[3 * P + p] = math.fsum(term[yp].tolist())
            sums[4 * P + p] = math.fsum(term[~yp].tolist())
    sums[5 * P] = float(keep.sum())
    return sums


def plane_coeffs(criterion: str, sums, pixels: float = 0.0, smooth: float = 1.0, scale: float = 1.0,
                 complement: bool = False):
    """(coeffs float64 [4,P], loss): per plane the coefficients of :func:`plane_grad` and ``scale`` times the sum of
    the planes' values, from the sums of :func:`plane_sums` (of one image or added over a batch).  The device rounds
    each coefficient once to float32; these are not rounded.

    ``'dice'``: ``D = Q + Z + smooth``, value ``1 - (2I + smooth)/D``, ``c1 = sigma*scale*(2I + smooth)/D^2``, ``c0 =
    c1 - sigma*scale*2/D``, ``c2 = c3 = 0``; sigma is -1 with ``complement`` (dq/dx = -q(1-q)), else 1.
    ``'mbce'``: ``w = (pixels - Q + 1)/(Q + 1)``, value ``w*L1 + L0``, ``c0 = c1 = scale*L1*(-(pixels + 2)/(Q + 1)^2)``
    -- the weight is a function of x, this is its derivative --, ``c2 = scale*w``, ``c3 = scale``."""
    s = np.asarray(sums, np.float64).reshape(-1)
    P = (s.size - 1) // 5
    if s.size != 5 * P + 1 or P < 1:
        raise ValueError("sums: 5*P + 1 values")
    Q, I, Z, L1, L0 = (s[r * P:(r + 1) * P] for r in range(5))
    scale = float(scale)
    if criterion == "dice":
        if not smooth > 0:
            raise ValueError("smooth must be > 0")
        sigma = -1.0 if complement else 1.0
        D, top = Q + Z + float(smooth), 2.0 * I + float(smooth)
        value = 1.0 - top / D
        c1 = sigma * scale * top / (D * D)
        c0 = c1 - sigma * scale * 2.0 / D
        c2 = c3 = np.zeros(P)
    elif criterion == "mbce":
        if complement:
            raise ValueError("mbce has no complement")
        S1 = Q + 1.0
        w = (float(pixels) - Q + 1.0) / S1
        value = w * L1 + L0
        c0 = c1 = scale * L1 * (-(float(pixels) + 2.0) / (S1 * S1))
        c2, c3 = scale * w, np.full(P, scale)
    else:
        raise ValueError("criterion: 'dice' or 'mbce'")
    total = 0.0
    for v in value.tolist():                       # (ascending planes, as the device adds them)
        total += v
    return np.stack([c0, c1, c2, c3]).astype(np.float64), total * scale


def plane_grad(logits, part, offsets, truth, truth_classes, num_truth: int, coeffs, factor: float = 1.0,
               complement: bool = False):
    """float64 [P,H,W]: ``factor * (q*(1-q)*(c0 where z else c1) + (s - y)*(c2 where y else c3))`` with ``s =
    expit(x)`` and q, z as in :func:`plane_sums`; 0 at an ignored pixel."""
    x = np.asarray(logits).astype(np.float64)
    P = x.shape[0]
    c = np.asarray(coeffs, np.float64).reshape(4, P)
    y, keep = plane_targets(part, P, offsets, truth, truth_classes, num_truth)
    s = _expit(x)
    q = _expit(-x) if complement else s
    z = ~y if complement else y
    pick = lambda m, a, b: np.where(m, a[:, None, None], b[:, None, None])
    g = float(factor) * (q * (1.0 - q) * pick(z, c[0], c[1]) + (s - y) * pick(y, c[2], c[3]))
    return np.where(keep[None], g, 0.0)


def _batch_targets(prediction, part, offsets, truth, truth_classes):
    x = np.asarray(prediction).astype(np.float64)
    B, P = x.shape[:2]
    if truth_classes is None:
        truth_classes = [None] * B
    y, keep = [], []
    for b in range(B):
        tc = truth_classes[b]
        yb, kb = plane_targets(part, P, offsets, truth[b], tc, 0 if tc is None else len(tc))
        y.append(yb)
        keep.append(np.broadcast_to(kb[None], yb.shape))
    return x, np.stack(y), np.stack(keep)


def dice_loss(prediction, part, offsets, truth, truth_classes=None, mode: str = "1", smooth: float = 1.0):
    """(loss, gradient float64 [B,P,H,W]) of ``SoftDiceLoss(mode, smooth)`` (utils/loss.py:38-58) on one part of a
    batch, written directly: per plane i over the WHOLE batch ``1 - (2*sum(p*t) + smooth)/(sum(p) + sum(t) + smooth)``
    with ``p = sigmoid(x)``, the planes added up; mode ``'0'`` takes ``1 - p`` (as ``sigmoid(-x)``) and ``1 - t``.
    ``prediction`` [B,P,H,W], ``truth`` [B,H,W], ``truth_classes``: per image the classes of its labels or None.
    Ignored pixels (class part) are left out of every sum and have gradient 0."""
    if mode not in ("0", "1"):
        raise ValueError("mode: '0' or '1'")
    x, y, keep = _batch_targets(prediction, part, offsets, truth, truth_classes)
    comp = mode == "0"
    q = np.where(keep, _expit(-x if comp else x), 0.0)
    z = np.where(keep, ~y if comp else y, False)
    sigma = -1.0 if comp else 1.0
    loss, grad = 0.0, np.zeros_like(x)
    for i in range(x.shape[1]):
        qi, zi = q[:, i], z[:, i]
        top = 2.0 * math.fsum(qi[zi].tolist()) + smooth
        D = math.fsum(qi.reshape(-1).tolist()) + float(zi.sum()) + smooth
        loss += 1.0 - top / D
        grad[:, i] = sigma * qi * (1.0 - qi) * (top / (D * D) - np.where(zi, 2.0 / D, 0.0))
    return loss, np.where(keep, grad, 0.0)


def multi_bce_loss(prediction, part, offsets, truth, truth_classes=None):
    """(loss, gradient float64 [B,P,H,W]) of ``MultiBCEWithLogitsLoss`` (utils/loss.py:63-76) on one part of a batch,
    written directly: per image and plane ``S = sum sigmoid(x)``, ``w = (n - S + 1)/(S + 1)`` with ``n = H*W``; the
    element weight is w where the target is 1, else 1; the loss is the mean over all B*P*H*W elements of weight times
    BCE term.  The gradient is that of this loss as a function of x, the weight INCLUDED (the reference's torch kept it
    in the graph): ``[(s - y)*(w where y else 1) + L1*(-(n + 2)/(S + 1)^2)*s*(1 - s)] / (B*P*H*W)`` with L1 the sum of
    the terms of the plane's target-1 elements.  Ignored pixels (class part) are left out of S and L1, contribute 0
    and have gradient 0; they still count in n and in the divisor."""
    x, y, keep = _batch_targets(prediction, part, offsets, truth, truth_classes)
    B, P, H, W = x.shape
    n, scale = float(H * W), 1.0 / (B * P * H * W)
    s = _expit(x)
    term = np.logaddexp(0.0, np.where(y, -x, x))
    grad = np.zeros_like(x)
    values = []
    for b in range(B):
        for p in range(P):
            k, yy = keep[b, p], y[b, p] & keep[b, p]
            S = math.fsum(s[b, p][k].tolist())
            L1 = math.fsum(term[b, p][yy].tolist())
            L0 = math.fsum(term[b, p][k & ~yy].tolist())
            w = (n - S + 1.0) / (S + 1.0)
            values.append(w * L1 + L0)
            sp = s[b, p]
            grad[b, p] = scale * ((sp - y[b, p]) * np.where(y[b, p], w, 1.0)
                                  + L1 * (-(n + 2.0) / ((S + 1.0) * (S + 1.0))) * sp * (1.0 - sp))
    return math.fsum(values) * scale, np.where(keep, grad, 0.0)


# ---- cross-entropy over the planes of one part, from the label mask: the numpy statement of Merger.mask_ce and of
# losses.MaskCELoss (CrossEntropyLossOneHot of utils/loss.py:24-35, F.cross_entropy(input, target.max(1)[1]), on the
# targets of utils/dataset.py:259-277 and :419-429, looked up in the label mask) ---------------------------------------

def ce_targets(part, num_planes: int, offsets, truth, truth_classes, num_truth: int):
    """(target int64 [H,W], keep bool [H,W]): the target plane of every pixel and the pixels that take part -- what
    ``target.max(1)[1]`` elects on the one-hot planes of :func:`plane_targets`: the FIRST plane whose target is 1,
    plane 0 where none is.  Class part: the truth class; a pixel whose truth class lies outside 0..P-1 is ignored
    (its target is given as 0).  Offset part: the least k whose offset target is 1, else 0; every pixel takes part."""
    y, keep = plane_targets(part, num_planes, offsets, truth, truth_classes, num_truth)
    return np.argmax(y, axis=0).astype(np.int64), keep          # (argmax: the first maximal index, 0 when all are 0)


def mask_ce(logits, part, offsets, truth, truth_classes, num_truth: int, scale: float = 1.0):
    """(sums float64 [2], grad float64 [P,H,W]) of one image: the cross-entropy of the softmax over the P planes of
    one part of the output against the pixel's target plane, and its gradient.

    x is the element widened exactly to float64 (float64 logits are taken as they are), and so is all else.  Target plane: :func:`ce_targets`.
    Term of a pixel: ``logsumexp_q(x_q) - x_target``; gradient: ``(softmax(x)_q - [q == target]) * scale``.  A pixel
    whose truth class lies outside 0..P-1 (class part) is an ignore class: term 0, gradient 0, not counted.  That is
    one difference from the reference, whose one-hot planes would be all zero at such a pixel and would elect class
    0; with every class in range the two agree.  ``sums[0]``: the correctly rounded sum (``math.fsum``) of the kept
    pixels' terms, ``sums[1]``: the number of kept pixels."""
    x = np.asarray(logits).astype(np.float64)
    P = x.shape[0]
    target, keep = ce_targets(part, P, offsets, truth, truth_classes, num_truth)
    if x.shape != (P,) + target.shape:
        raise ValueError("the logits and the truth mask differ in size")
    planes = np.arange(P)[:, None, None]
    m = x.max(axis=0)
    first = planes == np.argmax(x, axis=0)[None]                # the first maximal plane: its exponential is 1
    onehot = planes == target[None]
    e = np.exp(x - m[None])
    r = np.where(first, 0.0, e).sum(axis=0)                     # sum(exp) - 1, without forming 1 + r
    x_target = np.take_along_axis(x, target[None], axis=0)[0]
    term = np.log1p(r) + (m - x_target)                         # (log(1 + r) would lose a term that is about r)
    rest = np.where(onehot, 0.0, e).sum(axis=0)                 # 1 - softmax_target = rest / (1 + r): nothing cancels
    grad = np.where(onehot, -rest[None], e) / (1.0 + r)[None] * float(scale)
    grad = np.where(keep[None], grad, 0.0) + 0.0                # (+ 0.0: no negative zero at P = 1)
    sums = np.array([math.fsum(term[keep].tolist()), float(keep.sum())], np.float64)
    return sums, grad
