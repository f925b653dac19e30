"""The numpy statements of the dataset-level evaluation (labels.eval_records, labels.coco_accumulate,
labels.coco_summarize): hand-computed cases, the two forms of the accumulate against each other bit for bit, and the
rules the device path is held to (tests/test_gpu_dataset_eval.py).  pycocotools is not needed anywhere."""
import ctypes
import os
import re

import numpy as np
import pytest

import eval_util as eu
from mergenet_amd import labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table_of(pairs, K, G):
    """[K+1, G+1] with the given {(p, g): pixels}."""
    t = np.zeros((K + 1, G + 1), np.int32)
    for (p, g), n in pairs.items():
        t[p, g] = n
    return t


def one(table, pc, tc, scores=None, crowd=None, image=0, C=2, thresholds=(0.5,), area_ranges=((0.0, 1e10),),
        max_det=100):
    return labels.eval_records(table, np.asarray(pc, np.int32), np.asarray(tc, np.int32),
                               None if scores is None else np.asarray(scores, np.float32), crowd,
                               thresholds=thresholds, area_ranges=area_ranges, max_det=max_det, num_classes=C,
                               image=image)


@pytest.mark.parametrize("form", ["loop", "closed"])
def test_hand_case_tp_fp_tp(form):
    """Two truth instances; detections TP (0.9), FP (0.8), TP (0.7) at one threshold: rc = [1/2, 1/2, 1],
    pr = [1, 1/2, 2/3], the envelope [1, 2/3, 2/3]; searchsorted gives index 0 for the 51 recall thresholds up to
    0.5 and index 2 for the other 50: AP = (51 * 1 + 50 * 2/3) / 101."""
    table = table_of({(0, 0): 100, (1, 1): 10, (2, 0): 10, (3, 2): 10}, 3, 2)
    rec = one(table, [1, 1, 1], [1, 1], [0.9, 0.8, 0.7])
    assert rec["matched"][0, 0].tolist() == [True, False, True] and not rec["ignored"].any()
    assert rec["rank"].tolist() == [0, 1, 2] and rec["npig"].tolist() == [[0], [2]]
    res = labels.coco_accumulate([rec], 2, max_dets=(100,), form=form)
    p = res["precision"][0, :, 1, 0, 0]
    assert p.shape == (101,)
    assert (np.abs(p[:51] - 1.0) < 1e-12).all() and (np.abs(p[51:] - 2.0 / 3.0) < 1e-12).all()
    assert abs(p.mean() - (51 * 1 + 50 * 2 / 3) / 101) < 1e-12 and abs(p.mean() - 0.834983498349835) < 1e-12
    assert res["recall"][0, 1, 0, 0] == 1.0
    s = res["scores"][0, :, 1, 0, 0]
    assert (s[:51] == np.float64(np.float32(0.9))).all() and (s[51:] == np.float64(np.float32(0.7))).all()
    assert (res["precision"][:, :, 0] == -1).all() and (res["recall"][:, 0] == -1).all()      # class 0: no truth
    summary = labels.coco_summarize(res, thresholds=(0.5,), max_dets=(100,))
    assert abs(summary["AP"] - 0.834983498349835) < 1e-12 and summary["AP50"] == summary["AP"]
    assert summary["AP75"] == -1.0 and summary["AP_small"] == -1.0 and summary["AR@100"] == 1.0


@pytest.mark.parametrize("form", ["loop", "closed"])
def test_the_envelope_lifts_a_precision_that_is_sampled(form):
    """FP (0.9) then TP (0.8), one truth instance: pr = [0, 1/2]; recall threshold 0 samples index 0, whose
    precision the envelope lifts from 0 to 1/2; the score sampled is still that of index 0."""
    table = table_of({(0, 0): 100, (1, 0): 10, (2, 1): 10}, 2, 1)
    rec = one(table, [1, 1], [1], [0.9, 0.8])
    res = labels.coco_accumulate([rec], 2, rec_thresholds=[0.0, 0.5, 1.0], max_dets=(100,), form=form)
    assert np.allclose(res["precision"][0, :, 1, 0, 0], 0.5, atol=1e-12)
    assert res["scores"][0, :, 1, 0, 0].tolist() == [np.float64(np.float32(0.9))] + [np.float64(np.float32(0.8))] * 2


@pytest.mark.parametrize("form", ["loop", "closed"])
def test_hand_case_recall_thresholds_out_of_reach(form):
    """Four truth instances, one TP: rc = [1/4]; the 26 thresholds up to 0.25 give precision 1, the 75 above it 0."""
    table = table_of({(0, 0): 100, (1, 1): 10, (0, 2): 10, (0, 3): 10, (0, 4): 10}, 1, 4)
    rec = one(table, [1], [1, 1, 1, 1], [0.6])
    res = labels.coco_accumulate([rec], 2, max_dets=(100,), form=form)
    p, s = res["precision"][0, :, 1, 0, 0], res["scores"][0, :, 1, 0, 0]
    assert (np.abs(p[:26] - 1.0) < 1e-12).all() and (p[26:] == 0).all() and (s[26:] == 0).all() and (s[:26] > 0).all()
    assert res["recall"][0, 1, 0, 0] == 0.25 and res["npig"][1, 0] == 4


@pytest.mark.parametrize("seed", range(300))
def test_loop_and_closed_forms_are_bit_equal(seed):
    ds = eu.make_dataset(seed)
    recs = eu.records(ds)
    a, b = eu.statement(ds, "loop", recs), eu.statement(ds, "closed", recs)
    T, A, M = len(ds["thresholds"]), len(ds["area_ranges"]), len(ds["max_dets"])
    R = 101 if ds["rec_thresholds"] is None else len(ds["rec_thresholds"])
    assert a["precision"].shape == (T, R, ds["C"], A, M) and a["recall"].shape == (T, ds["C"], A, M)
    for key in ("precision", "recall", "scores", "npig"):
        assert eu.same(a[key], b[key]), key
    assert ((a["precision"] == -1) == (a["scores"] == -1)).all()
    assert ((a["npig"] == 0)[None, :, :, None] == (a["recall"] == -1)).all()


def test_the_random_datasets_hold_what_they_are_meant_to():
    seen = dict(tie=0, nan=0, crowd=0, no_truth=0, no_det=0, ignored_only=0, out_of_reach=0, unscored=0, empty=0)
    for seed in range(300):
        ds = eu.make_dataset(seed)
        recs = eu.records(ds)
        res = eu.statement(ds, "closed", recs)
        sc = np.concatenate([r["scores"] for r in recs])
        cls = np.concatenate([r["classes"] for r in recs])
        tcs = np.concatenate([im["truth_classes"] for im in ds["images"]])
        seen["nan"] += int(np.isnan(sc).any())
        seen["tie"] += int(len(np.unique(sc[~np.isnan(sc)])) < (~np.isnan(sc)).sum())
        seen["crowd"] += int(any(im["crowd"] is not None and im["crowd"].any() for im in ds["images"]))
        seen["unscored"] += int(ds["images"][0]["scores"] is None)
        seen["empty"] += int(any(im["table"].shape == (1, 1) for im in ds["images"]))
        for k in range(ds["C"]):
            seen["no_truth"] += int((cls == k).any() and not (tcs == k).any())
            seen["no_det"] += int(not (cls == k).any() and res["npig"][k, 0] > 0)
            seen["ignored_only"] += int((tcs == k).any() and (res["npig"][k] == 0).any())
        seen["out_of_reach"] += int(((res["precision"] == 0) & (res["scores"] == 0)).any())
    assert min(seen.values()) >= 5, seen


def test_a_detection_beyond_the_cut_neither_matches_nor_holds_a_truth_instance():
    """Class 1: detection 1 (0.9) and detection 2 (0.8) both cover truth 1, detection 1 better.  Class 2 is there so
    that ranks are per class.  With max_det 1 detection 2 is beyond the cut: it stays unmatched -- in a matching of all
    detections at threshold 0.1 it would take truth 1's neighbour, truth 2."""
    table = table_of({(0, 0): 100, (1, 1): 20, (2, 1): 4, (2, 2): 8, (0, 2): 8, (3, 3): 10}, 3, 3)
    pc, tc, sc = [1, 1, 2], [1, 1, 2], [0.9, 0.8, 0.7]
    full = one(table, pc, tc, sc, C=3, thresholds=(0.1,), max_det=2)
    cut = one(table, pc, tc, sc, C=3, thresholds=(0.1,), max_det=1)
    assert full["rank"].tolist() == cut["rank"].tolist() == [0, 1, 0]
    assert full["matched"][0, 0].tolist() == [True, True, True]
    assert cut["matched"][0, 0].tolist() == [True, False, True] and not cut["ignored"].any()
    assert np.array_equal(full["npig"], cut["npig"])
    # and it does not hold a truth instance either: a NaN-free reordering in which the cut detection comes FIRST
    # (detection 2 of class 1 with the top score is rank 0; detection 1 is now beyond the cut)
    swapped = one(table, pc, tc, [0.8, 0.9, 0.7], C=3, thresholds=(0.1,), max_det=1)
    assert swapped["classes"].tolist() == [1, 1, 2] and swapped["rank"].tolist() == [0, 1, 0]
    assert swapped["matched"][0, 0].tolist() == [True, False, True]
    res_full = labels.coco_accumulate([full], 3, max_dets=(1, 2))
    res_cut = labels.coco_accumulate([cut], 3, max_dets=(1,))
    assert res_full["recall"][0, 1, 0].tolist() == [0.5, 1.0] and res_cut["recall"][0, 1, 0].tolist() == [0.5]


def test_a_truth_instance_that_only_a_cut_detection_covers_counts_as_missed():
    """TP (0.9), FP (0.8), TP (0.7) of one class with max_det 2: the third detection is cut, so the truth instance it
    alone covers is missed -- recall 1/2, where matching all detections gives 1.  (Ranks ascend within a class, so a
    cut detection never comes before a kept one of its class: what the cut changes is what is seen here and above.)"""
    table = table_of({(0, 0): 100, (1, 1): 10, (2, 0): 10, (3, 2): 10}, 3, 2)
    kept_all = labels.coco_accumulate([one(table, [1, 1, 1], [1, 1], [0.9, 0.8, 0.7], max_det=3)], 2, max_dets=(3,))
    cut = labels.coco_accumulate([one(table, [1, 1, 1], [1, 1], [0.9, 0.8, 0.7], max_det=2)], 2, max_dets=(2,))
    assert kept_all["recall"][0, 1, 0, 0] == 1.0 and cut["recall"][0, 1, 0, 0] == 0.5


def test_equal_scores_across_images_keep_the_order_of_add():
    tp = one(table_of({(0, 0): 100, (1, 1): 10}, 1, 1), [1], [1], [0.5], image=0)
    fp = one(table_of({(0, 0): 100, (1, 0): 10}, 1, 0), [1], [], [0.5], image=1)
    first_tp = labels.coco_accumulate([tp, fp], 2, rec_thresholds=[0.0], max_dets=(100,))
    first_fp = labels.coco_accumulate([fp, tp], 2, rec_thresholds=[0.0], max_dets=(100,))
    assert abs(first_tp["precision"][0, 0, 1, 0, 0] - 1.0) < 1e-12        # pr = [1, 1/2]
    assert abs(first_fp["precision"][0, 0, 1, 0, 0] - 0.5) < 1e-12        # pr = [0, 1/2], lifted to 1/2
    for form in ("loop", "closed"):
        again = labels.coco_accumulate([fp, tp], 2, rec_thresholds=[0.0], max_dets=(100,), form=form)
        assert eu.same(again["precision"], first_fp["precision"])


@pytest.mark.parametrize("seed", range(20))
def test_the_order_of_the_images_changes_nothing_without_ties_across_images(seed):
    ds = eu.make_dataset(1000 + seed)
    rng = np.random.default_rng(seed)
    total = sum(len(im["pred_classes"]) for im in ds["images"])
    distinct = iter(rng.permutation(total).astype(np.float32) / np.float32(total))
    for im in ds["images"]:
        im["scores"] = np.asarray([next(distinct) for _ in im["pred_classes"]], np.float32)
    want = eu.statement(ds)
    ds["images"] = [ds["images"][i] for i in rng.permutation(len(ds["images"]))]
    got = eu.statement(ds)
    for key in ("precision", "recall", "scores", "npig"):
        assert eu.same(got[key], want[key]), key


def near(a, b):
    """Means are compared within 1e-12: the order in which a mean sums its entries is no part of the contract."""
    return abs(float(a) - float(b)) < 1e-12


def test_summarize():
    T, R, C, A, M = 10, 3, 4, 4, 3
    rng = np.random.default_rng(5)
    res = {"precision": rng.random((T, R, C, A, M)), "recall": rng.random((T, C, A, M))}
    res["precision"][:, :, 2] = -1                       # class 2: no truth anywhere
    res["recall"][:, 2] = -1
    res["precision"][:, :, :, 1] = -1                    # nothing small
    res["recall"][:, :, 1] = -1
    s = labels.coco_summarize(res)
    assert list(s) == labels.eval_summary_names() == ["AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large",
                                                     "AR@1", "AR@10", "AR@100", "AR_small", "AR_medium", "AR_large"]
    p, r = res["precision"], res["recall"]
    assert near(s["AP"], p[:, :, [1, 3], 0, 2].mean()) and near(s["AP50"], p[0, :, [1, 3], 0, 2].mean())
    assert near(s["AP75"], p[5, :, [1, 3], 0, 2].mean()) and labels.COCO_THRESHOLDS[5] == 0.75
    assert s["AP_small"] == -1.0 and s["AR_small"] == -1.0
    assert near(s["AP_medium"], p[:, :, [1, 3], 2, 2].mean()) and near(s["AP_large"], p[:, :, [1, 3], 3, 2].mean())
    assert all(near(s[k], r[:, [1, 3], 0, m].mean()) for m, k in enumerate(("AR@1", "AR@10", "AR@100")))
    assert near(s["AR_medium"], r[:, [1, 3], 2, 2].mean()) and near(s["AR_large"], r[:, [1, 3], 3, 2].mean())
    # the classes argument: a subset, the background included on request, a class without entries alone
    assert near(labels.coco_summarize(res, classes=[3])["AP"], p[:, :, 3, 0, 2].mean())
    assert near(labels.coco_summarize(res, classes=[0, 1])["AR@10"], r[:, [0, 1], 0, 1].mean())
    assert set(labels.coco_summarize(res, classes=[2]).values()) == {-1.0}
    assert set(labels.coco_summarize(res, classes=[]).values()) == {-1.0}
    with pytest.raises(ValueError):
        labels.coco_summarize(res, classes=[4])
    # thresholds without 0.5 / 0.75: AP50 / AP75 are -1, AP is not; fewer than four ranges: small .. large are -1
    th = np.asarray([0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95, 0.99])
    s = labels.coco_summarize(res, thresholds=th)
    assert s["AP50"] == -1.0 and near(s["AP75"], p[4, :, [1, 3], 0, 2].mean()) and th[4] == 0.75 and s["AP"] > 0
    two = {"precision": res["precision"][:, :, :, :1, :2].copy(), "recall": res["recall"][:, :, :1, :2].copy()}
    s = labels.coco_summarize(two, max_dets=(1, 10))
    assert list(s) == ["AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR@1", "AR@10", "AR_small",
                       "AR_medium", "AR_large"]
    assert near(s["AP"], two["precision"][:, :, [1, 3], 0, 1].mean()) and near(s["AR@10"], two["recall"][:, [1, 3], 0, 1].mean())
    assert [s[k] for k in ("AP_small", "AP_medium", "AP_large", "AR_small", "AR_medium", "AR_large")] == [-1.0] * 6
    with pytest.raises(ValueError):
        labels.coco_summarize(res, max_dets=(1, 10))


def test_an_evaluation_without_images_is_all_minus_one():
    res = labels.coco_accumulate([], 3, num_thresholds=2, num_area_ranges=1, max_dets=(1, 5))
    assert res["precision"].shape == (2, 101, 3, 1, 2) and (res["precision"] == -1).all()
    assert (res["recall"] == -1).all() and (res["scores"] == -1).all() and not res["npig"].any()


def test_parameter_errors():
    table = table_of({(0, 0): 1}, 0, 0)
    for kw in (dict(thresholds=[]), dict(thresholds=np.linspace(0, 1, 17)), dict(area_ranges=[]),
               dict(area_ranges=[(0, 1)] * 5)):
        with pytest.raises(ValueError):
            labels.eval_records(table, [], [], num_classes=2, **kw)
    for md in ((), (1, 2, 3, 4, 5), (0, 1), (2, 2), (3, 1)):
        with pytest.raises(ValueError):
            labels.coco_accumulate([], 2, max_dets=md)
    with pytest.raises(ValueError):
        labels.coco_accumulate([], 2, form="other")


def test_library_exports_the_entry_points_and_the_constants_agree():
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    for name, n in (("mn_eval_append_device", 18), ("mn_eval_keys_device", 6), ("mn_eval_accumulate_device", 17)):
        assert name in seg.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mergenet_hip.h")).read())
    for name in ("MN_EVAL_RECORD_BYTES", "MN_EVAL_MAX_AREAS", "MN_EVAL_MAX_DETS", "MN_EVAL_CHUNK"):
        assert "#define %s %d " % (name, getattr(seg, name)) in flat
    assert "mn_kernels_eval.h" in open(os.path.join(ROOT, "mergenet_amd", "csrc", "Makefile")).read()
    assert hasattr(seg.Merger, "dataset_eval") and hasattr(seg.DatasetEval, "summarize")


def test_null_context_is_an_argument_error_without_a_device():
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    th = (ctypes.c_double * 2)(0.5, 0.75)
    md = (ctypes.c_int * 2)(1, 10)
    assert lib.mn_eval_append_device(None, p, 1, 1, p, None, p, None, th, 2, th, 1, 10, 2, 0, p, p, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_eval_keys_device(None, p, 1, 2, p, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_eval_accumulate_device(None, p, 1, p, p, p, 2, 2, p, 2, 1, md, 2, p, p, p, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_last_status() == seg.MN_ERR_ARGUMENT
