"""labels.map_scores, class_scores and offset_iou -- the numpy statement of Merger.map_scores -- on a hand-worked case
and against what the reference's own runningScore / offsetIoU gave (tests/golden/map_scores_v1.npz, written by
tests/golden/make_golden_scores.py); the C ABI of mn_map_scores_device (no GPU)."""
import ctypes
import os
import re

import numpy as np

from mergenet_amd import labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_case():
    """2 x 4 pixels, C = 3, truth labels 1 (class 1) and 2 (class 7: outside 0..2, an ignore class); label 9 is out
    of range: class 0, but still a label of its own for the sameness rule.  Every value is dyadic, so every sum is
    exact."""
    truth = np.array([[0, 1, 1, 9],
                      [2, 2, 0, 0]], np.int32)
    per_pixel = [[(.5, .25, .25), (.25, .5, .5), (.75, .5, .25), (.25, .25, .5)],       # 0, tie 1|2 -> 1, 0, 2
                 [(.25, .5, .75), (.75, .25, .5), (.5, .5, .5), (.25, .75, .5)]]        # 2, 0, tie of all -> 0, 1
    class_probs = np.ascontiguousarray(np.array(per_pixel, np.float32).transpose(2, 0, 1))
    offsets = [(0, 1), (5, 0), (-1, -1)]
    same_probs = np.array([[[.25, .5, .75, 1.0], [.5, .25, 0.0, .5]],
                           [[.75] * 4, [.75] * 4],
                           [[.5] * 4, [.5, .25, .75, .5]]], np.float32)
    return class_probs, same_probs, offsets, truth, np.array([1, 7], np.int32)


def test_hand_worked_case():
    cp, sp, offsets, truth, classes = hand_case()
    confusion, sums = labels.map_scores(cp, sp, offsets, truth, classes, 2)
    assert confusion.dtype == np.int64 and sums.dtype == np.float64 and sums.shape == (3, 3)
    # truth class 0: (0,0) -> 0, (0,3) [label 9] -> 2, (1,2) -> 0 [tie of all three], (1,3) -> 1
    # truth class 1: (0,1) -> 1 [tie of 1 and 2], (0,2) -> 0;  the two pixels of label 2 (class 7) are left out
    assert confusion.tolist() == [[2, 1, 1], [1, 1, 0], [0, 0, 0]]
    assert confusion.sum() == truth.size - 2
    # (0, 1): different at (0,0) 0|1, (0,2) 1|9, (1,1) 2|0 -- the excluded pixel (1,1) counts here
    assert sums[:, 0].tolist() == [.75 + .25 + .75, 4.25, 3.0]
    # (5, 0) leaves the image everywhere
    assert sums[:, 1].tolist() == [0.0, 2.0, 0.0]
    # (-1, -1): row 1 looks up and to the left: (1,1) 2|0, (1,2) 0|1, (1,3) 0|1
    assert sums[:, 2].tolist() == [.75 + .25 + .5, 4.0, 3.0]


def test_no_truth_instances_and_out_of_range_labels():
    cp, sp, offsets, truth, _ = hand_case()
    confusion, sums = labels.map_scores(cp, sp, offsets, truth, None, 0)
    assert confusion[0].tolist() == [4, 2, 2] and confusion[1:].sum() == 0          # every label reads as class 0
    assert sums.tolist() == labels.map_scores(cp, sp, offsets, truth, [1, 7], 2)[1].tolist()   # labels as they stand


def test_logits_are_scored_as_their_float32_probabilities():
    cp, sp, offsets, truth, classes = hand_case()
    lc = np.log(cp.astype(np.float64) / (1 - cp.astype(np.float64))).astype(np.float32)
    lc[:, 0, 0] = (-1.0, 25.0, 18.0)             # the float32 sigmoid is exactly 1.0 from about 17: a tie on p
    lc[:, 1, 3] = (20.0, 18.0, 25.0)
    ls = np.zeros_like(sp)
    confusion, sums = labels.map_scores(lc, ls, offsets, truth, classes, 2, logits=True)
    one = np.float32(1)
    p = one / (one + np.exp(-lc))
    assert p.dtype == np.float32 and p[1, 0, 0] == p[2, 0, 0] == 1.0 and (p[:, 1, 3] == 1.0).all()
    want, _ = labels.map_scores(p, sp, offsets, truth, classes, 2)
    assert np.array_equal(confusion, want)
    assert confusion[0].tolist() == [2, 1, 1]                        # pixel (0,0) -> class 1, pixel (1,3) -> class 0
    assert sums[1].tolist() == [4.0, 4.0, 4.0]                       # 1 - sigmoid(0) = 0.5 at 8 pixels


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "map_scores_v1.npz"), allow_pickle=False)


def test_against_the_reference_classes():
    z = golden()
    cp, sp, truth = z["class_probs"], z["same_probs"], z["truth"]
    assert cp.shape == (4, 24, 40) and sp.shape == (5, 24, 40) and cp.dtype == np.float32
    offsets = [tuple(int(v) for v in o) for o in z["offsets"]]
    assert (30, 0) in offsets and any(di < 0 and dj < 0 for di, dj in offsets)
    assert set(np.unique(truth)) == set(range(7))
    confusion, sums = labels.map_scores(cp, sp, offsets, truth, z["truth_classes"], 6)
    assert np.array_equal(confusion, z["confusion_matrix"].astype(np.int64))
    assert np.array_equal(z["confusion_matrix"], z["confusion_matrix"].astype(np.int64))
    # The reference sums in float32: any float32 summation of n non-negative terms is within n * 2^-24 of the true
    # sum, relative; n = 960 pixels.  (Measured: 2e-8 to 8e-8 relative.)
    n = truth.size
    assert n == 960
    eps = n * 2.0 ** -24
    union = sums[1] + sums[2] - sums[0]
    for k in range(len(offsets)):
        err_i = abs(sums[0, k] - z["intersection"][k])
        err_u = abs(union[k] - z["union"][k])
        print("offset %s: intersection off by %.3g (bound %.3g), union by %.3g (bound %.3g)"
              % (offsets[k], err_i, eps * sums[0, k], err_u, eps * sums[:, k].sum()))
        assert err_i <= eps * sums[0, k]
        assert err_u <= eps * (sums[0, k] + sums[1, k] + sums[2, k])
    k = offsets.index((30, 0))
    assert sums[0, k] == 0.0 and sums[2, k] == 0.0 and z["intersection"][k] == 0.0


def test_summaries_equal_the_reference_get_scores():
    z = golden()
    summary, iou = labels.class_scores(z["confusion_matrix"].astype(np.int64))
    want = dict(zip(("overall_acc", "mean_acc", "freq_acc", "mean_IU"), z["class_summary"]))
    assert set(summary) == set(want)
    for key in want:
        assert abs(summary[key] - want[key]) <= 1e-12, key
    assert np.abs(iou - z["class_iou"]).max() <= 1e-12
    # the reference's intersection and union as totals: sums[1] + sums[2] - sums[0] = union
    sums = np.stack([z["intersection"], z["union"] + z["intersection"], np.zeros_like(z["union"])])
    got, mean = labels.offset_iou(sums)
    assert np.abs(got - z["offset_iou"]).max() <= 1e-12 and abs(mean - z["offset_mean"]) <= 1e-12


def test_summaries_keep_the_reference_nans():
    summary, iou = labels.class_scores(np.array([[3, 1, 0], [0, 2, 0], [0, 0, 0]]))       # class 2 never occurs
    assert np.isnan(iou[2]) and abs(summary["mean_IU"] - (3 / 4 + 2 / 3) / 2) <= 1e-15
    assert abs(summary["overall_acc"] - 5 / 6) <= 1e-15 and abs(summary["mean_acc"] - (3 / 4 + 1) / 2) <= 1e-15
    iou, mean = labels.offset_iou(np.array([[0.0, 1.0], [0.0, 3.0], [0.0, 2.0]]))
    assert np.isnan(iou[0]) and iou[1] == 0.25 and np.isnan(mean)                         # 0 / 0 stays


def test_entry_point_is_declared_exported_and_listed():
    import __graft_entry__ as g
    g.build()
    from mergenet_amd import segmenter as seg
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mn_map_scores_device\s*\(([^)]*)\)\s*;", code)
    assert m, "include/mergenet_hip.h does not declare mn_map_scores_device"
    assert len(m.group(1).split(",")) == 17
    assert "mn_map_scores_device" in seg.EXPORTS
    fn = seg.load_library().mn_map_scores_device
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 17
    assert fn.argtypes[5] is ctypes.c_int and fn.argtypes[15] is ctypes.c_int      # dtype, accumulate
    assert "mn_kernels_mapscore.h" in open(os.path.join(ROOT, "mergenet_amd", "csrc", "Makefile")).read()
    assert callable(seg.Merger.map_scores)
