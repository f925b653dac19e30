"""Overlap table, IoU and COCO matching on the device against the numpy statements of mergenet_amd/labels.py.
Every comparison is exact: the table holds integers, the IoU is one IEEE division of exact integers (compared bit
for bit as float64), the matching compares those IoUs -- so there are no tolerances."""
import ctypes
import functools

import numpy as np
import pytest

import golden_util as gu
import match_util as mu
from mergenet_amd import labels

pytestmark = pytest.mark.gpu

K_PRED, G_TRUTH = 9, 6
SHAPES = [(1, 1),
          (3, 5),
          (7, 64),       # exactly one chunk of 4-byte loads per row (taken with an unaligned mask: W % 4 == 0)
          (33, 257),     # 4-byte loads, the last chunk of a row reaches past W
          (48, 256),     # 16-byte loads, one chunk per row
          (32, 1028),    # 16-byte loads, the last chunk of a row partly past W
          (64, 1030),    # 4-byte loads, several chunks per row
          (345, 516)]    # 16-byte loads AND two chunks per wave (three per row: a wave's pair straddles a row end)
KINDS = ["blobs", "noise", "pred_rows", "truth_rows"]


def blobs(shape, n, seed):
    H, W = shape
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.int32)
    for k in range(1, n + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        m[max(0, y - H // 6):y + H // 6 + 1, max(0, x - W // 6):x + W // 6 + 1] = k
    return m


@functools.lru_cache(maxsize=None)
def masks(kind, shape):
    """(prediction, truth).  blobs: a few labels, runs of realistic length, plus runs placed where the walk changes
    path; noise: every pixel a head; pred_rows / truth_rows: one mask constant over each row while the other
    changes within it -- a head test that looks at one mask only counts whole rows for the wrong pair."""
    H, W = shape
    rng = np.random.default_rng(17)
    if kind == "blobs":
        pred, truth = blobs(shape, K_PRED, 3), blobs(shape, G_TRUTH, 4)
        if W > 70:
            pred[H // 2, 60:70] = 5                   # across lanes 63 | 64 or inside one lane's pixels
            truth[H // 2, 62:66] = 2
        pred[H - 1, W - 1], truth[H - 1, W - 1] = 1, 1          # the last pixel of the image
        if W >= 256:
            truth[1, 250:W] = 3                       # across the 256-pixel mark, up to the last column
            pred[2, :] = 4                            # a whole row: no later head in the wave
    elif kind == "noise":
        pred = rng.integers(0, K_PRED + 1, shape).astype(np.int32)
        truth = rng.integers(0, G_TRUTH + 1, shape).astype(np.int32)
    else:
        rows = np.repeat(rng.integers(0, K_PRED + 1, (H, 1)), W, axis=1).astype(np.int32)
        other = blobs(shape, G_TRUTH, 4) if kind == "pred_rows" else blobs(shape, K_PRED, 3)
        rows_max = G_TRUTH if kind == "truth_rows" else K_PRED
        rows = np.minimum(rows, rows_max)
        pred, truth = (rows, other) if kind == "pred_rows" else (other, rows)
    for a in (pred, truth):
        a.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def checker_table(kind, shape):
    t = labels.overlap_table(*masks(kind, shape), K_PRED, G_TRUTH)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def merger():
    from mergenet_amd import segmenter as seg
    m = seg.Merger(64, 128, 9, 10)
    yield m
    m.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the shared arrays are read-only)


def unaligned(a):
    """The mask on the device one int into a larger buffer: 4 bytes off a 16-byte boundary."""
    import torch
    buf = torch.zeros((a.size + 4,), dtype=torch.int32, device="cuda")
    view = buf[1:1 + a.size].view(a.shape)
    view.copy_(dev(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_table_equals_the_checker(merger, shape, kind):
    pred, truth = masks(kind, shape)
    d_pred = dev(pred)
    got = merger.overlap_table(d_pred, dev(truth), K_PRED, G_TRUTH).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (K_PRED + 1, G_TRUTH + 1)
    assert np.array_equal(got, checker_table(kind, shape))
    assert got.sum() == shape[0] * shape[1]
    areas = merger.instance_table(d_pred, K_PRED).cpu().numpy()[:, 0]
    assert np.array_equal(got.sum(axis=1)[1:], areas)
    if shape[1] % 4 == 0:                                # the same shape through the 4-byte loads
        got = merger.overlap_table(unaligned(pred), dev(truth), K_PRED, G_TRUTH).cpu().numpy()
        assert np.array_equal(got, checker_table(kind, shape))
    if kind in ("pred_rows", "truth_rows") and shape[1] >= 64:
        changing = truth if kind == "pred_rows" else pred
        assert (changing[:, 1:] != changing[:, :-1]).any()


def test_table_with_no_instances_on_either_side(merger):
    pred, truth = masks("blobs", (33, 257))
    n = pred.size
    got = merger.overlap_table(dev(pred), dev(truth), 0, G_TRUTH).cpu().numpy()
    assert got.shape == (1, G_TRUTH + 1) and np.array_equal(got, labels.overlap_table(pred, truth, 0, G_TRUTH))
    got = merger.overlap_table(dev(pred), dev(truth), K_PRED, 0).cpu().numpy()
    assert got.shape == (K_PRED + 1, 1) and np.array_equal(got, labels.overlap_table(pred, truth, K_PRED, 0))
    got = merger.overlap_table(dev(pred), dev(truth), 0, 0).cpu().numpy()
    assert got.tolist() == [[n]]


@pytest.mark.parametrize("shape", [(33, 257), (48, 256)])
def test_out_of_range_labels_count_as_0_and_write_nothing_outside_the_table(merger, shape):
    import torch
    K, G = K_PRED, G_TRUTH
    pred, truth = (np.array(m) for m in masks("noise", shape))
    pred[pred == 2] = -3
    pred[pred == 3] = K + 7
    truth[truth == 1] = G + 1
    assert (pred == -3).any() and (pred == K + 7).any() and (truth == G + 1).any()
    entries = (K + 1) * (G + 1)
    pad = 16 * (G + 1)                                   # room for the rows K + 1 .. K + 16 an unguarded kernel would hit
    buf = torch.full((pad + entries + pad,), -777, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    d_pred, d_truth = dev(pred), dev(truth)              # (held: a temporary's memory is handed out again at once)
    rc = merger.lib.mn_overlap_table_device(merger.handle, d_pred.data_ptr(), d_truth.data_ptr(), shape[0],
                                            shape[1], K, G, buf[pad:].data_ptr(), ctypes.c_void_p(stream))
    assert rc == 0
    got = buf.cpu().numpy()
    assert (got[:pad] == -777).all() and (got[pad + entries:] == -777).all()
    table = got[pad:pad + entries].reshape(K + 1, G + 1)
    assert np.array_equal(table, labels.overlap_table(pred, truth, K, G))
    zeroed_p = np.where((pred < 0) | (pred > K), 0, pred)
    zeroed_t = np.where(truth > G, 0, truth)
    assert np.array_equal(table, labels.overlap_table(zeroed_p, zeroed_t, K, G)) and table.sum() == pred.size


@pytest.mark.parametrize("which", ["pred", "truth"])
def test_an_unaligned_mask_on_a_16_byte_shape(merger, which):
    shape = (48, 256)
    pred, truth = masks("blobs", shape)
    d_pred, d_truth = (unaligned(pred), dev(truth)) if which == "pred" else (dev(pred), unaligned(truth))
    got = merger.overlap_table(d_pred, d_truth, K_PRED, G_TRUTH).cpu().numpy()
    assert np.array_equal(got, checker_table("blobs", shape))


def test_every_pixel_its_own_prediction_label(merger):
    H, W = 32, 64
    pred = (np.random.default_rng(8).permutation(H * W) + 1).astype(np.int32).reshape(H, W)
    truth = blobs((H, W), 9, 4)
    got = merger.overlap_table(dev(pred), dev(truth), H * W, 9).cpu().numpy()
    assert np.array_equal(got, labels.overlap_table(pred, truth, H * W, 9))
    assert (got[1:].sum(axis=1) == 1).all() and got[0].sum() == 0


def test_argument_errors(merger):
    import torch
    from mergenet_amd import segmenter as seg
    m = dev(np.zeros((4, 4), np.int32))
    table = torch.zeros((16,), dtype=torch.int32, device="cuda")
    fn, h = merger.lib.mn_overlap_table_device, merger.handle
    for args in ((None, m.data_ptr(), 4, 4, 1, 1, table.data_ptr()), (m.data_ptr(), None, 4, 4, 1, 1, table.data_ptr()),
                 (m.data_ptr(), m.data_ptr(), 4, 4, 1, 1, None), (m.data_ptr(), m.data_ptr(), 0, 4, 1, 1, table.data_ptr()),
                 (m.data_ptr(), m.data_ptr(), 4, -1, 1, 1, table.data_ptr()),
                 (m.data_ptr(), m.data_ptr(), 4, 4, -1, 1, table.data_ptr()),
                 (m.data_ptr(), m.data_ptr(), 4, 4, 1, -1, table.data_ptr()),
                 (m.data_ptr(), m.data_ptr(), 65536, 32768, 1, 1, table.data_ptr()),       # H * W > INT_MAX
                 (m.data_ptr(), m.data_ptr(), 4, 4, 2 ** 14, 2 ** 14, table.data_ptr())):  # (K + 1) * (G + 1) > 2^28
        assert fn(h, *args, None) == seg.MN_ERR_ARGUMENT and merger.lib.mn_last_status() == seg.MN_ERR_ARGUMENT
    assert not table.any().item()


# ---- matching ---------------------------------------------------------------------------------------------------

SIZES = [(0, 3), (3, 0), (1, 1), (5, 7), (70, 65), (300, 257)]


@functools.lru_cache(maxsize=None)
def match_case(size, variant):
    """Tables from masks of at most 64x128 with blocks of 1-4 pixels, the prediction a redrawn copy of the truth.
    variant 0 / 1: the two area ranges, two / three classes."""
    K, G = size
    H, W = (8, 16) if max(K, G) <= 7 else (64, 128)
    return mu.make_case(100 + 2 * (K + G) + variant, H, W, K, G, n_classes=2 + variant, nan_score=True, derived=True,
                        area_range=mu.AREA_RANGES[variant])


@functools.lru_cache(maxsize=None)
def match_want(size, variant, with_scores):
    return mu.want(match_case(size, variant), "closed", with_scores)


def run_match(merger, case, table, with_scores, **kw):
    return merger.match_instances(dev(table), dev(case["pred_classes"]), dev(case["truth_classes"]),
                                  scores=dev(case["scores"]) if with_scores else None, crowd=dev(case["crowd"]),
                                  thresholds=mu.THRESHOLDS, area_range=case["area_range"], return_iou=True, **kw)


@pytest.mark.parametrize("with_scores", [True, False])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("size", SIZES)
def test_matching_equals_the_checker(merger, size, variant, with_scores):
    import torch
    case = match_case(size, variant)
    K, G = size
    table, want = match_want(size, variant, with_scores)
    got_table = merger.overlap_table(dev(case["pred"]), dev(case["truth"]), K, G)
    assert np.array_equal(got_table.cpu().numpy(), table)
    got = run_match(merger, case, table, with_scores)
    assert sorted(got) == sorted(want)
    T = len(mu.THRESHOLDS)
    assert tuple(got["pred_match"].shape) == (T, K) and tuple(got["truth_match"].shape) == (T, G)
    assert got["pred_ignore"].dtype == torch.bool and got["truth_ignore"].dtype == torch.bool
    assert got["iou"].dtype == torch.float64
    assert got["iou"].cpu().numpy().tobytes() == want["iou"].tobytes()
    for key in ("pred_match", "truth_match", "pred_ignore", "truth_ignore"):
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key
    if K >= 70:                                          # the inputs exercise the rules (counted on the checker's result)
        n = mu.events(case, want, with_scores)
        assert n["to_ignored"] >= 1 and want["pred_match"].any() and np.isnan(case["scores"]).sum() == 1
        assert len(np.unique(case["scores"][~np.isnan(case["scores"])])) < K


def test_matching_events_are_present_in_the_device_cases():
    """Ties, iou == threshold and a crowd instance taken twice occur somewhere in the cases above."""
    total = dict(tie=0, at_threshold=0, crowd_twice=0, to_ignored=0)
    for size in SIZES:
        for variant in (0, 1):
            for with_scores in (True, False):
                if size[0] and size[1]:
                    for key, n in mu.events(match_case(size, variant), match_want(size, variant, with_scores)[1],
                                            with_scores).items():
                        total[key] += n
    assert min(total.values()) >= 1, total


def test_matching_without_optional_arguments_and_with_the_default_thresholds(merger):
    case = match_case((70, 65), 0)
    table = labels.overlap_table(case["pred"], case["truth"], 70, 65)
    want = labels.match_instances(table, case["pred_classes"], case["truth_classes"])
    got = merger.match_instances(dev(table), dev(case["pred_classes"]), dev(case["truth_classes"]))
    assert sorted(got) == ["pred_ignore", "pred_match", "truth_ignore", "truth_match"]
    assert tuple(got["pred_match"].shape) == (10, 70)
    for key in got:
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key
    assert want["pred_match"].any()


def test_more_instances_than_the_matching_holds(merger):
    import torch
    from mergenet_amd import segmenter as seg
    K = seg.MN_MATCH_MAX_INSTANCES + 1
    table = torch.zeros((K + 1, 2), dtype=torch.int32, device="cuda")
    classes = torch.ones((K,), dtype=torch.int32, device="cuda")
    with pytest.raises(seg.MergeNetError) as e:
        merger.match_instances(table, classes, classes)
    assert e.value.status == seg.MN_ERR_CAPACITY and merger.lib.mn_last_status() == seg.MN_ERR_CAPACITY
    with pytest.raises(seg.MergeNetError) as e:
        merger.match_instances(table.t().contiguous(), classes, classes)
    assert e.value.status == seg.MN_ERR_CAPACITY


def test_segment_then_match_against_the_golden_mask(merger, oracle):
    import torch
    from mergenet_amd import segmenter as seg
    g = gu.load("cseg_synth_64x128_n15")
    sdb, omf, bias = g["spec"]["opts"]
    opts = seg.default_options(same_different_bias=sdb, object_merge_factor=omf, merge_logprob_bias=bias, clip_inputs=1)
    mask, classes, _, st = merger.segment(torch.from_numpy(g["class_probs"]).cuda(),
                                          torch.from_numpy(g["sameness_probs"]).cuda(), g["offsets"], opts)
    K, G = st["num_instances"], len(g["object_class"])
    mask_np, classes_np = mask.cpu().numpy(), [int(c) for c in classes.cpu().numpy()[:K]]
    assert oracle.masks_equivalent(mask_np, classes_np, g["mask"], g["object_class"]) and K == G > 0
    truth = np.ascontiguousarray(g["mask"], np.int32)
    truth_classes = np.asarray(g["object_class"], np.int32)
    table = merger.overlap_table(mask, dev(truth), K, G)
    got = merger.match_instances(table, classes, dev(truth_classes), return_iou=True)
    pm, tm, iou = got["pred_match"].cpu().numpy(), got["truth_match"].cpu().numpy(), got["iou"].cpu().numpy()
    # every detection is matched at all ten thresholds with IoU 1, by the permutation the checker accepts
    assert (pm > 0).all() and (pm == pm[0]).all() and sorted(pm[0]) == list(range(1, G + 1))
    assert (iou[np.arange(K), pm[0] - 1] == 1.0).all() and not got["pred_ignore"].any().item()
    assert np.array_equal(np.concatenate([[0], pm[0]])[mask_np], truth)
    assert all(classes_np[k] == truth_classes[pm[0, k] - 1] for k in range(K))
    assert all(tm[t, pm[t, k] - 1] == k + 1 for t in range(10) for k in range(K))
    # the truth two columns to the right: whatever now matches, it is what the checker says
    shifted = np.zeros_like(truth)
    shifted[:, 2:] = truth[:, :-2]
    table = merger.overlap_table(mask, dev(shifted), K, G)
    want_table = labels.overlap_table(mask_np, shifted, K, G)
    assert np.array_equal(table.cpu().numpy(), want_table)
    want = labels.match_instances(want_table, classes_np, truth_classes)
    got = merger.match_instances(table, classes, dev(truth_classes), return_iou=True)
    assert got["iou"].cpu().numpy().tobytes() == want["iou"].tobytes()
    for key in ("pred_match", "truth_match", "pred_ignore", "truth_ignore"):
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key
    assert 0 < (want["pred_match"][0] > 0).sum() and (want["iou"] < 1.0).all()
