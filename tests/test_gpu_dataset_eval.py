"""Merger.dataset_eval on the device against the numpy statements of mergenet_amd/labels.py (eval_records,
coco_accumulate, coco_summarize).  Every comparison is exact: the records hold integers and bits, and every value of
precision, recall and scores is one IEEE division of exact integers or a float32 score widened -- so there are no
tolerances (a NaN score equals a NaN score)."""
import functools

import numpy as np
import pytest

import eval_util as eu
from mergenet_amd import labels

pytestmark = pytest.mark.gpu

KEYS = ("precision", "recall", "scores", "npig")
RECORD_KEYS = ("classes", "scores", "rank", "image", "matched", "ignored")


@pytest.fixture(scope="module")
def merger():
    from mergenet_amd import segmenter as seg
    m = seg.Merger(64, 128, 9, 10)
    yield m
    m.close()


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def evaluator(merger, ds, **kw):
    return merger.dataset_eval(ds["C"], thresholds=ds["thresholds"], rec_thresholds=ds["rec_thresholds"],
                               area_ranges=ds["area_ranges"], max_dets=ds["max_dets"], **kw)


def add_all(ev, ds):
    for im in ds["images"]:
        ev.add(dev(im["table"]), dev(im["pred_classes"]), dev(im["truth_classes"]), dev(im["scores"]), dev(im["crowd"]))


def check_records(ev, recs):
    got = ev.records()
    for key in RECORD_KEYS:
        want = np.concatenate([r[key] for r in recs], axis=-1) if recs else got[key][..., :0]
        assert eu.same(got[key], want), key


def check_result(got, want):
    assert sorted(got) == sorted(KEYS)
    for key in KEYS:
        assert eu.same(got[key].cpu().numpy(), want[key]), key


@functools.lru_cache(maxsize=None)
def small(seed, T=None, A=None, M=None):
    """A dataset of eval_util with T, A or M forced, its records and the statement's result (shared, read-only)."""
    ds = eu.make_dataset(seed)
    if T is not None:
        ds["thresholds"] = np.asarray([0.2]) if T == 1 else np.arange(1, T + 1) / 20
    if A is not None:
        ds["area_ranges"] = eu.AREA_RANGES[:A]
    if M is not None:
        ds["max_dets"] = (1, 2, 4, 7)[:M]
    recs = eu.records(ds)
    return ds, recs, eu.statement(ds, "closed", recs)


@pytest.mark.parametrize("seed", [0, 14, 15, 23])
def test_random_datasets_equal_the_statement(merger, seed):
    ds, recs, want = small(seed)
    ev = evaluator(merger, ds)
    add_all(ev, ds)
    assert ev.num_images == len(ds["images"]) and ev.num_records == sum(len(r["rank"]) for r in recs)
    check_records(ev, recs)
    check_result(ev.accumulate(), want)


@pytest.mark.parametrize("T,A,M", [(1, 1, 1), (16, 4, 4), (1, 4, 1), (16, 1, 4)])
def test_the_least_and_the_most_thresholds_ranges_and_max_dets(merger, T, A, M):
    """T = 16 with A = 4 uses all 64 bits of a record's two masks."""
    ds, recs, want = small(14, T, A, M)
    assert want["precision"].shape[0] == T and want["precision"].shape[3:] == (A, M)
    ev = evaluator(merger, ds)
    add_all(ev, ds)
    check_records(ev, recs)
    check_result(ev.accumulate(), want)
    if (T, A) == (16, 4):
        got = ev.records()
        assert got["matched"][3, 15].any() and got["ignored"][3, 15].any() and got["matched"][0, 0].any()


@functools.lru_cache(maxsize=None)
def chunk_case():
    """Class segments of 0, 1, CHUNK - 1, CHUNK, CHUNK + 1 and 2 * CHUNK + 1 records (classes 1..6; class 1 has truth
    instances and no detection: recall 0, precision 0; class 7 has detections and no truth instance: -1; class 0
    has neither), over four images of more than 256 detections each, so that every kernel of add runs several
    workgroups.  max_dets (3, 1000): the first selects a few records of every segment, the second all of them."""
    from mergenet_amd import segmenter as seg
    chunk = seg.MN_EVAL_CHUNK
    lengths = {1: 0, 2: 1, 3: chunk - 1, 4: chunk, 5: chunk + 1, 6: 2 * chunk + 1, 7: 9}
    rng = np.random.default_rng(99)
    classes = rng.permutation(np.concatenate([np.full(n, c, np.int32) for c, n in lengths.items()]))
    images = []
    for part in np.array_split(classes, 4):
        K, G = len(part), 90
        im = dict(eu.random_image(rng, 8, K, G, levels=16, nan=0.02, out_of_range=False))
        im["pred_classes"] = np.ascontiguousarray(part)
        # a truth instance has the class of the detection that covers it best (6 for 7), the first five class 1
        best = part[np.argmax(im["table"][1:, 1:], axis=0)]
        im["truth_classes"] = np.where(np.arange(G) < 5, 1, np.minimum(best, 6)).astype(np.int32)
        images.append(im)
    ds = dict(C=8, thresholds=np.asarray([0.3]), rec_thresholds=None, area_ranges=eu.AREA_RANGES[:1],
              max_dets=(3, 1000), images=images)
    recs = eu.records(ds)
    return ds, recs, eu.statement(ds, "closed", recs), lengths


def test_segment_lengths_around_the_scan_chunk(merger):
    ds, recs, want, lengths = chunk_case()
    got_lengths = np.bincount(np.concatenate([r["classes"] for r in recs]), minlength=8)
    assert got_lengths.tolist() == [0] + [lengths[c] for c in range(1, 8)] and min(len(r["rank"]) for r in recs) > 256
    assert (want["recall"][:, 1] == 0).all() and (want["precision"][:, :, 1] == 0).all() and want["npig"][1, 0] > 0
    assert (want["precision"][:, :, 7] == -1).all() and want["npig"][7, 0] == 0
    assert (want["precision"][:, :, 6, 0, 1] > 0).any() and (want["recall"][0, 3:7, 0, 1] > 0.1).all()
    ev = evaluator(merger, ds, capacity=300)                  # grows 300 -> 642 -> 1284: two doublings on the way
    add_all(ev, ds)
    assert ev.num_records == sum(lengths.values()) and ev.capacity >= ev.num_records > 4 * 300
    check_records(ev, recs)
    first = ev.accumulate()
    check_result(first, want)
    second = ev.accumulate()                                  # the log is left as it was
    for key in KEYS:
        assert eu.same(second[key].cpu().numpy(), first[key].cpu().numpy()), key
    summary = ev.summarize(first)
    assert summary == labels.coco_summarize(want, ds["thresholds"], ds["max_dets"])
    assert summary["AP"] > 0 and summary["AR@1000"] > summary["AR@3"] > 0 and summary["AP_small"] == -1.0
    assert ev.summarize(classes=[7]) == labels.coco_summarize(want, ds["thresholds"], ds["max_dets"], classes=[7])


def test_log_growth_across_a_doubling_keeps_the_records(merger):
    ds, recs, want = small(0)
    ev = evaluator(merger, ds, capacity=1)
    add_all(ev, ds)
    assert ev.capacity >= ev.num_records > 1
    check_records(ev, recs)
    check_result(ev.accumulate(), want)


def test_reset_then_reuse(merger):
    ds, recs, want = small(23)
    other = small(0)[0]
    ev = evaluator(merger, ds)
    add_all(ev, dict(ds, images=other["images"][:2]))
    ev.accumulate()
    ev.reset()
    assert ev.num_images == 0 and ev.num_records == 0
    empty = ev.accumulate()
    assert all((empty[k] == -1).all().item() for k in ("precision", "recall", "scores")) and not empty["npig"].any().item()
    add_all(ev, ds)
    check_records(ev, recs)
    check_result(ev.accumulate(), want)


def test_an_evaluator_without_images_and_images_without_instances(merger):
    ev = merger.dataset_eval(3, thresholds=[0.5, 0.75], max_dets=(1, 5), area_ranges=eu.AREA_RANGES[:2])
    want = labels.coco_accumulate([], 3, num_thresholds=2, num_area_ranges=2, max_dets=(1, 5))
    check_result(ev.accumulate(), want)
    assert set(ev.summarize().values()) == {-1.0}
    rng = np.random.default_rng(1)
    images = [eu.random_image(rng, 3, 0, 6), eu.random_image(rng, 3, 7, 0), eu.random_image(rng, 3, 0, 0),
              eu.random_image(rng, 3, 5, 4)]
    ds = dict(C=3, thresholds=np.asarray([0.5, 0.75]), rec_thresholds=None, area_ranges=eu.AREA_RANGES[:2],
              max_dets=(1, 5), images=images)
    recs = eu.records(ds)
    add_all(ev, ds)
    assert ev.num_images == 4 and ev.num_records == 12
    check_records(ev, recs)
    check_result(ev.accumulate(), eu.statement(ds, "closed", recs))


def test_every_detection_ignored(merger):
    """Five truth instances of one pixel each, inside the area range (0, 2); twelve detections of 3 pixels or more
    that touch none of them: every detection is unmatched and outside the range, so ignored -- tp = fp = 0 at every
    position, pr = 0 / eps = 0, and recall 0 with npig 5."""
    rng = np.random.default_rng(2)
    table = np.zeros((13, 6), np.int32)
    table[0, 1:] = 1
    table[1:, 0] = rng.integers(3, 30, 12)
    im = dict(table=table, pred_classes=np.ones(12, np.int32), truth_classes=np.ones(5, np.int32),
              scores=(rng.integers(1, 9, 12) / 8).astype(np.float32), crowd=None)
    ds = dict(C=2, thresholds=np.asarray([0.5, 1.0]), rec_thresholds=None, area_ranges=[(0.0, 2.0)], max_dets=(100,),
              images=[im])
    recs = eu.records(ds)
    assert recs[0]["ignored"].all() and not recs[0]["matched"].any()
    want = eu.statement(ds, "closed", recs)
    assert want["npig"][1, 0] == 5 and (want["recall"][:, 1] == 0).all() and (want["precision"][:, :, 1] == 0).all()
    assert want["scores"][0, 0, 1, 0, 0] > 0                   # recall threshold 0 is answered by the first record
    ev = evaluator(merger, ds)
    add_all(ev, ds)
    check_records(ev, recs)
    check_result(ev.accumulate(), want)


def test_tied_and_nan_scores_keep_the_order_of_add(merger):
    """Three scores only and many NaN over six images: most records tie across images."""
    rng = np.random.default_rng(7)
    images = [eu.random_image(rng, 3, 25, 12, levels=3, nan=0.3, classes=[1, 2], out_of_range=False) for _ in range(6)]
    ds = dict(C=3, thresholds=labels.COCO_THRESHOLDS, rec_thresholds=None, area_ranges=eu.AREA_RANGES,
              max_dets=(1, 10, 100), images=images)
    recs = eu.records(ds)
    want = eu.statement(ds, "closed", recs)
    assert np.isnan(want["scores"]).any()
    ev = evaluator(merger, ds)
    add_all(ev, ds)
    check_records(ev, recs)
    check_result(ev.accumulate(), want)
    rev = dict(ds, images=images[::-1])
    want_rev = eu.statement(rev)
    assert not eu.same(want_rev["precision"], want["precision"])          # the order of add matters among ties
    ev.reset()
    add_all(ev, rev)
    check_result(ev.accumulate(), want_rev)


def test_the_rank_cut(merger):
    """max_dets (1, 2) over images with a dozen detections per class: most detections lie beyond the cut, and would
    have matched."""
    rng = np.random.default_rng(13)
    images = [eu.random_image(rng, 3, 24, 10, classes=[1, 2], out_of_range=False) for _ in range(3)]
    ds = dict(C=3, thresholds=np.asarray([0.3, 0.5]), rec_thresholds=None, area_ranges=eu.AREA_RANGES[:2],
              max_dets=(1, 2), images=images)
    recs = eu.records(ds)
    uncut = [labels.eval_records(im["table"], im["pred_classes"], im["truth_classes"], im["scores"], im["crowd"],
                                 thresholds=ds["thresholds"], area_ranges=ds["area_ranges"], max_det=100, num_classes=3)
             for im in images]
    assert all((r["rank"] >= 2).sum() > 10 and not r["matched"][:, :, r["rank"] >= 2].any() for r in recs)
    assert any(u["matched"][:, :, u["rank"] >= 2].any() for u in uncut)
    ev = evaluator(merger, ds)
    add_all(ev, ds)
    check_records(ev, recs)
    check_result(ev.accumulate(), eu.statement(ds, "closed", recs))


def test_segment_to_summary_on_synthetic_images(merger):
    """Three synth images at 64x128: segment -> overlap_table -> add against the generator's ground truth (shifted by
    two columns in the last image, so that not every IoU is 1); the statement is fed from the same tables."""
    import torch
    from mergenet_amd import segmenter as seg
    from mergenet_amd import synth
    offs = synth.generate_offsets(40, 10)
    ev = merger.dataset_eval(9)
    recs = []
    for i, seed in enumerate((1001, 1002, 1003)):
        s = synth.synth_v1(64, 128, 9, offs, seed, num_instances=4 + i)
        mask, classes, _, st = merger.segment(torch.from_numpy(s.class_probs).cuda(),
                                              torch.from_numpy(s.sameness_probs).cuda(), offs,
                                              seg.default_options(clip_inputs=1))
        K, G = st["num_instances"], len(s.instance_class) - 1
        truth = np.ascontiguousarray(s.instances, np.int32)
        if i == 2:
            truth = np.ascontiguousarray(np.roll(truth, 2, axis=1))
        truth_classes = np.asarray(s.instance_class[1:], np.int32)
        scores = (np.random.default_rng(seed).integers(1, 5, K) / 4).astype(np.float32)
        table = merger.overlap_table(mask, dev(truth), K, G)
        ev.add(table, classes, dev(truth_classes), dev(scores))
        recs.append(labels.eval_records(table.cpu().numpy(), classes.cpu().numpy()[:K], truth_classes, scores,
                                        num_classes=9, image=i))
    assert ev.num_images == 3 and ev.num_records == sum(len(r["rank"]) for r in recs) > 0
    check_records(ev, recs)
    want = labels.coco_accumulate(recs, 9)
    result = ev.accumulate()
    check_result(result, want)
    summary = ev.summarize(result)
    assert summary == labels.coco_summarize(want) and list(summary) == labels.eval_summary_names()
    assert 0.0 < summary["AP"] <= 1.0 and summary["AP50"] >= summary["AP75"] > 0.0


def test_argument_errors_come_before_any_launch(merger):
    import torch
    from mergenet_amd import segmenter as seg
    for kw in (dict(thresholds=[]), dict(thresholds=np.linspace(0, 1, 17)), dict(area_ranges=[]),
               dict(area_ranges=[(0, 1)] * 5), dict(max_dets=()), dict(max_dets=(1, 2, 3, 4, 5)), dict(max_dets=(0, 1)),
               dict(max_dets=(2, 2)), dict(max_dets=(10, 1)), dict(capacity=0)):
        with pytest.raises(ValueError):
            merger.dataset_eval(3, **kw)
    with pytest.raises(ValueError):
        merger.dataset_eval(0)
    ev = merger.dataset_eval(3)
    table = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    pc = torch.ones((3,), dtype=torch.int32, device="cuda")
    tc = torch.ones((2,), dtype=torch.int32, device="cuda")
    sc = torch.ones((3,), dtype=torch.float32, device="cuda")
    cr = torch.zeros((2,), dtype=torch.uint8, device="cuda")
    big = torch.zeros((seg.MN_MATCH_MAX_INSTANCES + 2, 2), dtype=torch.int32, device="cuda")
    many = torch.ones((seg.MN_MATCH_MAX_INSTANCES + 1,), dtype=torch.int32, device="cuda")
    bad = [(table.long(), pc, tc, None, None), (table.cpu(), pc, tc, None, None), (table.t(), pc, tc, None, None),
           (table.view(-1), pc, tc, None, None), (table, None, tc, None, None), (table, pc, None, None, None),
           (table, pc.long(), tc, None, None), (table, pc[:2], tc, None, None), (table, pc, tc[:1], None, None),
           (table, pc, tc.cpu(), None, None), (table, pc, tc, sc.double(), None), (table, pc, tc, sc[:2], None),
           (table, pc, tc, sc, cr.int()), (table, pc, tc, sc, cr[:1]), (table, torch.ones(6, dtype=torch.int32,
                                                                                           device="cuda")[::2], tc, None, None),
           (big, many, tc, None, None), (big.t().contiguous(), pc, many, None, None)]
    for args in bad:
        with pytest.raises(ValueError):
            ev.add(*args)
    assert ev.num_images == 0 and ev.num_records == 0 and not ev._npig.any().item()
    ev.add(table, pc, tc, sc, cr.bool())                     # and the good call goes through
    assert ev.num_images == 1 and ev.num_records == 3
    # the C entry points refuse what the Python side cannot pass
    lib, h = merger.lib, merger.handle
    import ctypes
    th = (ctypes.c_double * 2)(0.5, 0.75)
    md = (ctypes.c_int * 2)(10, 1)
    p = table.data_ptr()
    out = torch.zeros((64,), dtype=torch.float64, device="cuda")
    o = out.data_ptr()
    assert lib.mn_eval_append_device(h, p, 3, 2, p, None, p, None, th, 17, th, 1, 10, 2, 0, o, o, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_eval_append_device(h, p, 3, 2, p, None, p, None, th, 2, th, 5, 10, 2, 0, o, o, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_eval_append_device(h, p, 3, 2, p, None, p, None, th, 2, th, 1, 0, 2, 0, o, o, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_eval_append_device(h, p, 3, 2, p, None, p, None, th, 2, th, 1, 10, 2, 0, o + 4, o, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_eval_append_device(h, p, 5000, 2, p, None, p, None, th, 2, th, 1, 10, 2, 0, o, o, None) == seg.MN_ERR_CAPACITY
    assert lib.mn_eval_keys_device(h, o, -1, 2, o, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_eval_accumulate_device(h, o, 1, o, o, o, 2, 2, o, 2, 1, md, 2, o, o, o, None) == seg.MN_ERR_ARGUMENT
    assert lib.mn_eval_accumulate_device(h, o, 1, o, o, o, 2, 2, o, 2, 1, md, 5, o, o, o, None) == seg.MN_ERR_ARGUMENT
    assert not out.any().item()
