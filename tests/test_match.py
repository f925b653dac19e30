"""Overlap table, IoU and COCO matching: the numpy statements of mergenet_amd/labels.py on hand-worked cases, the
loop form of the matching against its closed form on random block masks, and the ABI of the two entry points
(no GPU).  Every comparison is exact."""
import ctypes
import os
import re

import numpy as np

import match_util as mu
from mergenet_amd import labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("loop", "closed")


def match(pred, truth, K, G, pc, tc, form, **kw):
    table = labels.overlap_table(np.asarray(pred, np.int32), np.asarray(truth, np.int32), K, G)
    return labels.match_instances(table, np.asarray(pc, np.int32), np.asarray(tc, np.int32), form=form, **kw)


def test_overlap_table_by_hand():
    pred = np.array([[1, 1, 0, 2], [1, 9, -3, 2]], np.int32)       # 9 and -3: outside 0..2, count as 0
    truth = np.array([[1, 2, 2, 0], [1, 1, 3, 4]], np.int32)       # 4: outside 0..3
    t = labels.overlap_table(pred, truth, 2, 3)
    assert t.dtype == np.int32 and t.tolist() == [[0, 1, 1, 1], [0, 2, 1, 0], [2, 0, 0, 0]]
    assert t.sum() == pred.size
    assert t.sum(axis=1)[1:].tolist() == [3, 2] and t.sum(axis=0)[1:].tolist() == [3, 2, 1]
    assert labels.overlap_table(pred, truth, 0, 0).tolist() == [[8]]
    assert labels.overlap_table(pred, truth, 0, 3).tolist() == [[2, 3, 2, 1]]
    iou = labels.instance_iou(t)
    assert iou.dtype == np.float64 and iou.tolist() == [[2 / 4, 1 / 4, 0.0], [0.0, 0.0, 0.0]]
    # a crowd truth instance: intersection over the detection's area
    assert labels.instance_iou(t, crowd=[1, 0, 0])[0].tolist() == [2 / 3, 1 / 4, 0.0]
    # a label without pixels on either side: the denominator is 0, the IoU 0
    assert labels.instance_iou(np.array([[4, 0], [0, 0]], np.int32)).tolist() == [[0.0]]


def test_a_single_pixel():
    for form in FORMS:
        r = match([[1]], [[1]], 1, 1, [3], [3], form)
        assert r["iou"].tolist() == [[1.0]]
        assert r["pred_match"].tolist() == [[1]] * 10 and r["truth_match"].tolist() == [[1]] * 10
        assert not r["pred_ignore"].any() and not r["truth_ignore"].any()
        assert r["pred_match"].dtype == np.int32 and r["pred_ignore"].dtype == bool
        r = match([[1]], [[1]], 1, 1, [3], [4], form)                         # another class: no candidate
        assert not r["pred_match"].any() and not r["truth_match"].any() and r["iou"].tolist() == [[1.0]]
        r = match([[1]], [[0]], 1, 1, [3], [3], form, area_range=(2.0, 1e10))   # no overlap; both areas outside
        assert r["iou"].tolist() == [[0.0]] and not r["pred_match"].any()
        assert r["pred_ignore"].all() and r["truth_ignore"].all()
        # nothing to match: every output is zero
        r = match([[1]], [[0]], 1, 0, [3], [], form, area_range=(2.0, 1e10))
        assert r["pred_match"].shape == (10, 1) and r["truth_match"].shape == (10, 0) and r["iou"].shape == (1, 0)
        assert not r["pred_match"].any() and not r["pred_ignore"].any()
        r = match([[0]], [[1]], 0, 1, [], [3], form, area_range=(2.0, 1e10))
        assert r["truth_match"].shape == (10, 1) and not r["truth_match"].any() and not r["truth_ignore"].any()


def test_masks_equal_up_to_a_permutation_match_with_iou_1_at_all_ten_thresholds():
    rng = np.random.default_rng(4)
    G = 7
    truth = mu.block_mask(rng, 12, 20, G)[0]
    perm = np.concatenate([[0], rng.permutation(G) + 1])             # truth label -> prediction label
    pred = perm[truth].astype(np.int32)
    tc = rng.integers(1, 4, G).astype(np.int32)
    pc = np.zeros(G, np.int32)
    pc[perm[1:] - 1] = tc
    present = np.array([(truth == j).any() for j in range(1, G + 1)])
    assert present.sum() >= 5
    for form in FORMS:
        r = match(pred, truth, G, G, pc, tc, form, scores=rng.random(G).astype(np.float32))
        assert r["pred_match"].shape == (10, G)
        for t in range(10):
            assert np.array_equal(r["truth_match"][t], np.where(present, perm[1:], 0))
            for j in np.flatnonzero(present):
                assert r["pred_match"][t, perm[j + 1] - 1] == j + 1 and r["iou"][perm[j + 1] - 1, j] == 1.0
        assert not r["pred_ignore"].any()


def test_two_equal_candidates_the_larger_truth_label_wins():
    for form in FORMS:
        r = match([[1, 1, 1, 1]], [[1, 1, 2, 2]], 1, 2, [5], [5, 5], form, thresholds=[0.5, 0.55])
        assert r["iou"].tolist() == [[0.5, 0.5]]
        assert r["pred_match"].tolist() == [[2], [0]]                 # iou == threshold is a match; the LAST of equals
        assert r["truth_match"].tolist() == [[0, 1], [0, 0]]
        assert not r["pred_ignore"].any()


def test_a_crowd_instance_is_matched_by_two_detections():
    for form in FORMS:
        kw = dict(crowd=[1], thresholds=[0.5, 0.95])
        r = match([[1, 1, 2, 2]], [[1, 1, 1, 1]], 2, 1, [5, 5], [5], form, **kw)
        assert r["iou"].tolist() == [[1.0], [1.0]]                    # intersection over the detection's area
        assert r["pred_match"].tolist() == [[1, 1]] * 2
        assert r["truth_match"].tolist() == [[2]] * 2                 # the last detection in order
        assert r["pred_ignore"].all() and r["truth_ignore"].tolist() == [True]
        r = match([[1, 1, 2, 2]], [[1, 1, 1, 1]], 2, 1, [5, 5], [5], form, scores=[0.1, 0.9], **kw)
        assert r["pred_match"].tolist() == [[1, 1]] * 2 and r["truth_match"].tolist() == [[1]] * 2
        # without the flag the instance is taken once, and the IoU is the plain one
        r = match([[1, 1, 2, 2]], [[1, 1, 1, 1]], 2, 1, [5, 5], [5], form, thresholds=[0.5])
        assert r["iou"].tolist() == [[0.5], [0.5]] and r["pred_match"].tolist() == [[1, 0]]


def test_an_ignored_truth_instance_is_taken_only_while_no_other_passes_the_threshold():
    pred = [[1] * 6 + [0] * 6]
    truth = [[2] + [1] * 11]                                          # truth 1: 11 pixels, above the range: ignored
    for form in FORMS:
        r = match(pred, truth, 1, 2, [5], [5, 5], form, thresholds=[0.1, 0.25, 0.5], area_range=(0.0, 10.0))
        assert r["iou"].tolist() == [[5 / 12, 1 / 6]]
        assert r["truth_ignore"].tolist() == [True, False]
        # t = 0.1: truth 2 is a candidate and not ignored, so it is taken although truth 1 overlaps more;
        # t = 0.25: only the ignored truth 1 passes; t = 0.5: nothing does
        assert r["pred_match"].tolist() == [[2], [1], [0]]
        assert r["pred_ignore"].tolist() == [[False], [True], [False]]
        assert r["truth_match"].tolist() == [[0, 1], [1, 0], [0, 0]]


def test_equal_scores_are_taken_in_label_order_and_a_nan_score_last():
    pred, truth = [[1, 2]], [[1, 1]]                                  # both detections: IoU 1/2 with the one truth
    for form in FORMS:
        for scores, winner in (([0.5, 0.5], 1), (None, 1), ([0.1, 0.5], 2), ([np.nan, -1.0], 2),
                               ([np.nan, np.nan], 1), ([0.0, -0.0], 1)):
            r = match(pred, truth, 2, 1, [5, 5], [5], form, thresholds=[0.5],
                      scores=None if scores is None else np.asarray(scores, np.float32))
            assert r["truth_match"].tolist() == [[winner]], scores
            assert r["pred_match"].tolist() == [[1, 0] if winner == 1 else [0, 1]]
    assert labels.detection_order(np.array([0.5, np.nan, 0.75, 0.5, np.inf], np.float32), 5) == [4, 2, 0, 3, 1]


def test_loop_form_equals_closed_form_on_random_block_masks():
    total = dict(tie=0, at_threshold=0, crowd_twice=0, to_ignored=0)
    ranges = set()
    for seed in range(300):
        case = mu.small_case(seed)
        for with_scores in ((True, False) if seed % 5 == 0 else (True,)):
            table, closed = mu.want(case, "closed", with_scores)
            _, loop = mu.want(case, "loop", with_scores)
            assert sorted(closed) == sorted(loop) == ["iou", "pred_ignore", "pred_match", "truth_ignore", "truth_match"]
            for key in closed:
                assert closed[key].dtype == loop[key].dtype and np.array_equal(closed[key], loop[key]), (seed, key)
            assert closed["iou"].tobytes() == labels.instance_iou(table, case["crowd"]).tobytes()
            for key, n in mu.events(case, closed, with_scores).items():
                total[key] += n
        ranges.add(case["area_range"])
        assert table.sum() == case["pred"].size
    # the inputs hold what makes the two forms differ if either is wrong
    assert total["tie"] >= 1 and total["at_threshold"] >= 1 and total["crowd_twice"] >= 1 and total["to_ignored"] >= 1
    assert len(ranges) == 2 and len(mu.THRESHOLDS) == 12 and 0.1 in mu.THRESHOLDS and 0.25 in mu.THRESHOLDS


def test_library_exports_both_entry_points():
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    for name in ("mn_overlap_table_device", "mn_match_overlaps_device"):
        assert name in seg.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
    assert len(lib.mn_overlap_table_device.argtypes) == 9
    assert len(lib.mn_match_overlaps_device.argtypes) == 18
    assert seg.MN_MATCH_MAX_INSTANCES == 4096 and seg.MN_ERR_CAPACITY == -4


def test_null_context_is_an_argument_error_without_a_device():
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.mn_overlap_table_device(None, p, p, 2, 2, 3, 3, p, None)
    assert rc == seg.MN_ERR_ARGUMENT and lib.mn_last_status() == seg.MN_ERR_ARGUMENT
    th = (ctypes.c_double * 2)(0.5, 0.75)
    rc = lib.mn_match_overlaps_device(None, p, 3, 3, p, None, p, None, th, 2, 0.0, 1e10, None, p, p, p, None, None)
    assert rc == seg.MN_ERR_ARGUMENT and lib.mn_last_status() == seg.MN_ERR_ARGUMENT


def test_header_declares_both_prototypes():
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int mn_overlap_table_device(mn_context* ctx, const int* d_pred, const int* d_truth, int height, "
            "int width, int num_pred, int num_truth, int* d_table, void* stream);") in flat
    assert ("int mn_match_overlaps_device(mn_context* ctx, const int* d_table, int num_pred, int num_truth, "
            "const int* d_pred_class, const float* d_pred_score, const int* d_truth_class, "
            "const unsigned char* d_truth_crowd, const double* thresholds, int num_thresholds, double area_lo, "
            "double area_hi, double* d_iou, int* d_pred_match, int* d_truth_match, unsigned char* d_pred_ignore, "
            "unsigned char* d_truth_ignore, void* stream);") in flat
    assert "#define MN_MATCH_MAX_INSTANCES 4096" in flat
    # the reference lines the two stand in for are cited next to them
    assert "egs/cityscape/local/evaluate.py:67-73" in flat and "utils/dataset.py:486-506" in flat
    makefile = open(os.path.join(ROOT, "mergenet_amd", "csrc", "Makefile")).read()
    assert "mn_kernels_match.h" in makefile
    assert os.path.exists(os.path.join(ROOT, "mergenet_amd", "csrc", "mn_kernels_match.h"))


def test_binding_has_both_methods():
    import inspect
    from mergenet_amd import segmenter as seg
    p = inspect.signature(seg.Merger.overlap_table).parameters
    assert list(p) == ["self", "pred", "truth", "num_pred", "num_truth"]
    p = inspect.signature(seg.Merger.match_instances).parameters
    assert list(p) == ["self", "table", "pred_classes", "truth_classes", "scores", "crowd", "thresholds", "area_range",
                       "return_iou"]
    assert p["scores"].default is None and p["crowd"].default is None and p["thresholds"].default is None
    assert p["area_range"].default == (0.0, 1e10) and p["return_iou"].default is False
    assert np.array_equal(labels.COCO_THRESHOLDS, np.linspace(0.5, 0.95, 10))
