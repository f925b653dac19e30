"""Seeded inputs of the dataset-evaluation tests (tests/test_dataset_eval.py, tests/test_gpu_dataset_eval.py): small
datasets of overlap tables with classes, quantised scores (ties within and across images, NaN), crowd flags, and the
numpy statement run over them."""
import numpy as np

from mergenet_amd import labels

# areas of the generated instances lie between 5 and about 60 pixels: "all, small, medium, large" at that scale
AREA_RANGES = [(0.0, 1e10), (0.0, 20.0), (20.0, 40.0), (40.0, 1e10)]


def random_table(rng, K, G, paired=0.7):
    """int32 [K+1, G+1]: most detections share 5-39 pixels with one truth instance and 0-9 with the background, so
    IoUs on both sides of 0.5 occur; a few stray overlaps on top."""
    t = np.zeros((K + 1, G + 1), np.int64)
    t[0, 0] = 50
    for k in range(1, K + 1):
        t[k, 0] = rng.integers(0, 10)
        if G and rng.random() < paired:
            t[k, rng.integers(1, G + 1)] += rng.integers(5, 40)
        elif t[k, 0] == 0:
            t[k, 0] = 3
    for j in range(1, G + 1):
        t[0, j] = rng.integers(0, 10)
    if K and G:
        for _ in range((K + G) // 4):
            t[rng.integers(1, K + 1), rng.integers(1, G + 1)] += rng.integers(1, 6)
    return t.astype(np.int32)


def random_image(rng, C, K, G, levels=8, nan=0.1, classes=None, out_of_range=True):
    """One image.  Classes are drawn from `classes` (default 0..C-1) and, with `out_of_range`, now and then from -1
    and C, which no result counts."""
    pool = np.arange(C) if classes is None else np.asarray(classes)
    pc = rng.choice(pool, K).astype(np.int32)
    tc = rng.choice(pool, G).astype(np.int32)
    if out_of_range:
        pc[rng.random(K) < 0.08] = -1
        pc[rng.random(K) < 0.05] = C
        tc[rng.random(G) < 0.05] = C
    scores = (rng.integers(0, levels, K) / levels).astype(np.float32)
    scores[rng.random(K) < nan] = np.nan
    img = dict(table=random_table(rng, K, G), pred_classes=pc, truth_classes=tc, scores=scores,
               crowd=(rng.random(G) < 0.15).astype(np.uint8))
    for v in img.values():
        v.setflags(write=False)
    return img


def make_dataset(seed, kmax=20, gmax=20):
    """1-12 images, K and G in 0..kmax / 0..gmax, C in 2..5 -- some class usually has no truth, no detection, or
    only ignored truth -- and varying T, A, M and recall thresholds (COCO's 101, or a few unsorted ones with
    duplicates, values outside 0..1 and, rarely, a NaN)."""
    rng = np.random.default_rng(20_000 + seed)
    C = int(rng.integers(2, 6))
    T = int(rng.choice([1, 2, 10, 16]))
    A = int(rng.integers(1, 5))
    M = int(rng.integers(1, 5))
    thresholds = labels.COCO_THRESHOLDS if T == 10 else np.sort(rng.choice(np.arange(1, 20) / 20, T, replace=False))
    if rng.random() < 0.3:
        rec = None
    else:
        rec = rng.choice(np.concatenate([np.arange(0, 11) / 10, [-0.5, 0.25, 1.5]]), int(rng.integers(1, 9)))
        if rng.random() < 0.15:
            rec[rng.integers(0, len(rec))] = np.nan
    max_dets = tuple(sorted(int(v) for v in rng.choice(np.arange(1, 9), M, replace=False)))
    with_scores = rng.random() < 0.8
    pool = rng.choice(np.arange(C), int(rng.integers(1, C + 1)), replace=False)     # classes that occur at all
    images = []
    for _ in range(int(rng.integers(1, 13))):
        img = random_image(rng, C, int(rng.integers(0, kmax + 1)), int(rng.integers(0, gmax + 1)), classes=pool)
        if not with_scores:
            img["scores"] = None
        if rng.random() < 0.2:
            img["crowd"] = None
        images.append(img)
    return dict(C=C, thresholds=thresholds, rec_thresholds=rec, area_ranges=AREA_RANGES[:A], max_dets=max_dets,
                images=images)


def records(ds):
    """labels.eval_records of every image, in order."""
    return [labels.eval_records(im["table"], im["pred_classes"], im["truth_classes"], im["scores"], im["crowd"],
                                thresholds=ds["thresholds"], area_ranges=ds["area_ranges"], max_det=ds["max_dets"][-1],
                                num_classes=ds["C"], image=i) for i, im in enumerate(ds["images"])]


def statement(ds, form="closed", recs=None):
    return labels.coco_accumulate(records(ds) if recs is None else recs, ds["C"], rec_thresholds=ds["rec_thresholds"],
                                  max_dets=ds["max_dets"], num_thresholds=len(ds["thresholds"]),
                                  num_area_ranges=len(ds["area_ranges"]), form=form)


def same(a, b):
    """Bit for bit, a NaN (the score of a NaN detection) equal to a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
