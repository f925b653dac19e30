"""Instance table, small-instance filter and COCO results on the device against the numpy checkers of
mergenet_amd/labels.py.  Every comparison is integer-exact (scores are copied), so there are no tolerances."""
import ctypes
import functools

import numpy as np
import pytest

from mergenet_amd import labels, rle

pytestmark = pytest.mark.gpu

K_BLOBS = 9
SHAPES = [(1, 1),        # one pixel
          (1, 70),       # one row, longer than a wave
          (3, 5),
          (7, 67),       # odd W: 4-byte loads, a run across the wave boundary
          (33, 257),
          (64, 1030),    # W % 4 != 0 and wider than one workgroup's share of a row
          (48, 256),     # W % 4 == 0: 16-byte loads
          (345, 516)]    # 16-byte loads AND two chunks per wave (three per row: a wave's pair straddles a row end)


@functools.lru_cache(maxsize=None)
def blob_mask(shape):
    """The blob masks of tests/test_rle.py (realistic run lengths), plus runs placed where the walk changes path."""
    H, W = shape
    rng = np.random.default_rng(3)
    m = np.zeros((H, W), np.int32)
    for k in range(1, K_BLOBS + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        m[max(0, y - H // 6):y + H // 6 + 1, max(0, x - W // 6):x + W // 6 + 1] = k
    if shape == (7, 67):
        m[3, 60:67] = 5                       # across lanes 63 | 64 and up to the last column
    if shape == (64, 1030):
        m[5, 250:300] = 2                     # across the 256-pixel mark
        m[6, 1020:1030] = 3                   # up to the last column, in the last, partly filled load of the row
        m[7, :] = 4                           # a whole row
    if shape == (48, 256):
        m[7, 5:7] = 1                         # inside one lane's four pixels
        m[8, 3:9] = 2                         # over three lanes
        m[9, 255] = 3                         # the last pixel of a row alone
        m[10, :] = 4                          # a whole row: no later head in the wave
        m[11, 0:4] = 5
        m[11, 4:8] = 6                        # heads on lane boundaries
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def noise_mask(shape):
    m = np.random.default_rng(5).integers(0, K_BLOBS + 1, shape).astype(np.int32)     # runs of length ~1
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def checker_table(kind, shape):
    t = labels.instance_table({"blobs": blob_mask, "noise": noise_mask}[kind](shape), K_BLOBS)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def own_label_mask():
    """Every pixel its own instance: K = H * W, labels a random permutation."""
    H, W = 96, 131
    m = (np.random.default_rng(8).permutation(H * W) + 1).astype(np.int32).reshape(H, W)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def own_label_table():
    m = own_label_mask()
    t = labels.instance_table(m, m.size)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def merger():
    from mergenet_amd import segmenter as seg
    m = seg.Merger(150, 301, 9, 10)
    yield m
    m.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the shared arrays are read-only)


@pytest.mark.parametrize("kind", ["blobs", "noise"])
@pytest.mark.parametrize("shape", SHAPES)
def test_table_equals_the_checker(merger, shape, kind):
    m = {"blobs": blob_mask, "noise": noise_mask}[kind](shape)
    got = merger.instance_table(dev(m), K_BLOBS).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (K_BLOBS, 5)
    assert np.array_equal(got, checker_table(kind, shape))


def test_table_of_special_masks(merger):
    H, W = 33, 257
    empty = [0, W, H, -1, -1]
    got = merger.instance_table(dev(np.zeros((H, W), np.int32)), 3).cpu().numpy()       # all background, K = 3
    assert got.tolist() == [empty] * 3
    got = merger.instance_table(dev(blob_mask((H, W))), 0)                                # K = 0
    assert tuple(got.shape) == (0, 5)
    for shape in ((33, 257), (48, 256)):
        h, w = shape
        got = merger.instance_table(dev(np.ones(shape, np.int32)), 1).cpu().numpy()       # one instance, the whole image
        assert got.tolist() == [[h * w, 0, 0, w - 1, h - 1]]
        m = np.zeros(shape, np.int32)
        m[h - 1, w - 1] = 2                                                               # one pixel, last row and column
        got = merger.instance_table(dev(m), 2).cpu().numpy()
        assert got.tolist() == [[0, w, h, -1, -1], [1, w - 1, h - 1, w - 1, h - 1]]


def test_table_of_an_unaligned_mask_on_a_16_byte_shape(merger):
    import torch
    m = blob_mask((48, 256))
    buf = torch.zeros((48 * 256 + 4,), dtype=torch.int32, device="cuda")
    view = buf[1:1 + 48 * 256].view(48, 256)
    view.copy_(dev(m))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = merger.instance_table(view, K_BLOBS).cpu().numpy()
    assert np.array_equal(got, checker_table("blobs", (48, 256)))


def test_every_pixel_its_own_instance(merger):
    m = own_label_mask()
    got = merger.instance_table(dev(m), m.size).cpu().numpy()
    assert np.array_equal(got, own_label_table())
    assert (got[:, 0] == 1).all() and np.array_equal(got[:, 1], got[:, 3]) and np.array_equal(got[:, 2], got[:, 4])


@pytest.mark.parametrize("shape", [(33, 257), (48, 256)])
def test_out_of_range_labels_are_ignored(merger, shape):
    import torch
    K = K_BLOBS - 3
    m = np.array(blob_mask(shape))                      # holds labels K+1 .. K+3 = 7..9
    assert all((m == k).any() for k in (K + 1, K + 2, K + 3))
    table = torch.full((K + 8, 5), -777, dtype=torch.int32, device="cuda")    # 8 spare rows: an unguarded
    stream = torch.cuda.current_stream().cuda_stream                          # kernel would still write inside
    rc = merger.lib.mn_instance_table_device(merger.handle, dev(m).data_ptr(), shape[0], shape[1], K,
                                             table.data_ptr(), ctypes.c_void_p(stream))
    assert rc == 0
    got = table.cpu().numpy()
    zeroed = np.where(m > K, 0, m)
    assert np.array_equal(got[:K], labels.instance_table(zeroed, K))
    assert (got[K:] == -777).all()


K_FILTER = 12


@functools.lru_cache(maxsize=None)
def filter_case(shape):
    """Blobs 1..9, label 10 one pixel, label 11 two pixels, label 12 absent; classes and scores per label."""
    m = np.array(blob_mask(shape))
    H, W = shape
    m[H - 1, W - 1] = 10
    m[0, 0:2] = 11
    rng = np.random.default_rng(21)
    classes = rng.integers(1, 9, K_FILTER).astype(np.int32)
    scores = rng.normal(size=K_FILTER).astype(np.float32)
    table = labels.instance_table(m, K_FILTER)
    for a in (m, classes, scores, table):
        a.setflags(write=False)
    return m, classes, scores, table


@pytest.mark.parametrize("with_scores", [False, True])
@pytest.mark.parametrize("which", ["1", "2", "median", "N+1"])
@pytest.mark.parametrize("shape", [(33, 257), (64, 1030)])
def test_filter_equals_the_checker(merger, shape, which, with_scores):
    m, classes, scores, table = filter_case(shape)
    areas = table[:, 0]
    min_area = {"1": 1, "2": 2, "median": int(np.median(areas[areas > 0])), "N+1": m.size + 1}[which]
    min_score = float(np.median(scores)) if with_scores else None
    want = labels.filter_instances(m, classes, K_FILTER, table, min_area, scores if with_scores else None, min_score)
    w_mask, w_cls, w_scores, w_table, w_k, w_remap = want
    d_scores = dev(scores) if with_scores else None
    got = merger.filter_instances(dev(m), dev(classes), K_FILTER, min_area=min_area, scores=d_scores,
                                  min_score=min_score, return_remap=True)
    g_mask, g_cls, g_scores, g_table, g_k, g_remap = got
    assert isinstance(g_k, int) and g_k == w_k                 # read from the device int
    assert np.array_equal(g_remap.cpu().numpy(), w_remap)
    assert np.array_equal(g_mask.cpu().numpy(), w_mask)
    assert np.array_equal(g_cls.cpu().numpy(), w_cls)
    assert np.array_equal(g_table.cpu().numpy(), w_table) and tuple(g_table.shape) == (w_k, 5)
    if with_scores:
        assert g_scores.cpu().numpy().tobytes() == w_scores.tobytes()
    else:
        assert g_scores is None
    if which == "N+1":
        assert g_k == 0 and not g_mask.any().item()
    # in place: the same mask, written over the input; with the table handed in
    mine = dev(m)
    again = merger.filter_instances(mine, dev(classes), K_FILTER, min_area=min_area, scores=d_scores,
                                    min_score=min_score, inplace=True, table=dev(table))
    assert again[0].data_ptr() == mine.data_ptr() and again[4] == w_k
    assert np.array_equal(mine.cpu().numpy(), w_mask)
    assert np.array_equal(again[3].cpu().numpy(), w_table)


def test_filter_of_an_unaligned_mask_and_of_no_instances(merger):
    import torch
    m, classes, scores, table = filter_case((33, 257))
    want = labels.filter_instances(m, classes, K_FILTER, table, 2)
    buf = torch.zeros((m.size + 4,), dtype=torch.int32, device="cuda")       # 33 * 257 is odd: 4-byte form anyway;
    view = buf[1:1 + m.size].view(m.shape)                                    # the (48, 256) mask below is not
    view.copy_(dev(m))
    got = merger.filter_instances(view, dev(classes), K_FILTER, min_area=2)
    assert got[4] == want[4] and np.array_equal(got[0].cpu().numpy(), want[0])
    m2 = np.array(blob_mask((48, 256)))
    t2 = labels.instance_table(m2, K_BLOBS)
    want = labels.filter_instances(m2, classes[:K_BLOBS], K_BLOBS, t2, 40)
    buf = torch.zeros((m2.size + 4,), dtype=torch.int32, device="cuda")
    view = buf[1:1 + m2.size].view(m2.shape)
    view.copy_(dev(m2))
    got = merger.filter_instances(view, dev(classes[:K_BLOBS]), K_BLOBS, min_area=40, inplace=True)
    assert got[4] == want[4] and np.array_equal(view.cpu().numpy(), want[0])
    # K = 0: everything becomes background
    got = merger.filter_instances(dev(m2), dev(classes), 0)
    assert got[4] == 0 and not got[0].any().item() and tuple(got[3].shape) == (0, 5)


def test_filter_drops_a_nan_score_and_refuses_outputs_that_are_its_inputs(merger):
    import torch
    m, classes, scores, table = filter_case((33, 257))
    with_nan = np.array(scores)
    with_nan[4] = np.nan
    want = labels.filter_instances(m, classes, K_FILTER, table, 1, with_nan)
    got = merger.filter_instances(dev(m), dev(classes), K_FILTER, min_area=1, scores=dev(with_nan), return_remap=True)
    assert got[4] == want[4] and got[5].cpu().numpy()[5] == 0
    assert np.array_equal(got[5].cpu().numpy(), want[5]) and np.array_equal(got[0].cpu().numpy(), want[0])
    assert got[2].cpu().numpy().tobytes() == want[2].tobytes()
    # in-place compaction would race: an output that is its input is an argument error, nothing is queued
    d_m, d_t, d_c = dev(m), dev(table), dev(classes)
    remap = torch.empty((K_FILTER + 1,), dtype=torch.int32, device="cuda")
    spare_t, spare_c = torch.empty_like(d_t), torch.empty_like(d_c)
    count = torch.empty((1,), dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for t_out, c_out in ((d_t, spare_c), (spare_t, d_c)):
        rc = merger.lib.mn_filter_instances_device(merger.handle, d_m.data_ptr(), 33, 257, K_FILTER, d_t.data_ptr(),
                                                   d_c.data_ptr(), None, 1, 0.0, d_m.data_ptr(), remap.data_ptr(),
                                                   t_out.data_ptr(), c_out.data_ptr(), None, count.data_ptr(), stream)
        assert rc == -1 and merger.lib.mn_last_status() == -1
    assert np.array_equal(d_m.cpu().numpy(), m) and np.array_equal(d_t.cpu().numpy(), table)


def test_filter_with_more_labels_than_one_block_holds(merger):
    m = own_label_mask()
    K = m.size
    table = own_label_table()
    classes = (np.arange(K) % 7 + 1).astype(np.int32)
    # min_area = 2 drops every single-pixel instance
    got = merger.filter_instances(dev(m), dev(classes), K, min_area=2, table=dev(table))
    assert got[4] == 0 and not got[0].any().item() and (got[1].cpu().numpy() == -1).all()
    # min_score drops every second label: the survivors are renumbered densely, in order
    scores = (np.arange(1, K + 1) % 2).astype(np.float32)          # label k scores k % 2
    want = labels.filter_instances(m, classes, K, table, 1, scores, 0.5)
    got = merger.filter_instances(dev(m), dev(classes), K, min_area=1, scores=dev(scores), min_score=0.5,
                                  return_remap=True)
    assert got[4] == K // 2 == want[4]
    remap = got[5].cpu().numpy()
    assert np.array_equal(remap, want[5])
    odd = np.arange(1, K + 1, 2)
    assert np.array_equal(remap[odd], np.arange(1, K // 2 + 1)) and not remap[0::2].any()
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(got[3].cpu().numpy(), want[3])
    assert got[2].cpu().numpy().tobytes() == want[2].tobytes()


def test_segment_upsample_table_filter_coco_results(merger):
    import torch
    from mergenet_amd import segmenter as seg, synth
    offs = synth.generate_offsets(40, 10)
    s = synth.synth_v1(64, 128, 9, offs, 1001, num_instances=4)
    cp, sp = torch.from_numpy(s.class_probs).cuda(), torch.from_numpy(s.sameness_probs).cuda()
    mask, classes, _, st = merger.segment(cp, sp, offs, seg.default_options(clip_inputs=1))
    K = st["num_instances"]
    assert K > 0
    scores = merger.instance_scores(K)
    H, W = 150, 301
    big = merger.upsample_mask(mask, H, W)
    table = merger.instance_table(big, K)
    big_np, table_np = big.cpu().numpy(), table.cpu().numpy()
    assert np.array_equal(table_np, labels.instance_table(big_np, K))
    fmask, fcls, fscores, ftable, k2 = merger.filter_instances(big, classes, K, min_area=1, scores=scores, table=table)
    kept = [k for k in range(1, K + 1) if (big_np == k).any()]
    assert k2 == len(kept)
    fmask_np = fmask.cpu().numpy()
    assert all((fmask_np == k).any() for k in range(1, k2 + 1))           # no label of the filtered mask is empty
    assert fmask_np.max() == k2
    assert fscores.cpu().numpy().tobytes() == scores.cpu().numpy()[[k - 1 for k in kept]].tobytes()
    cat_ids = [0, 24, 25, 26, 27, 28, 31, 32, 33]
    res = merger.coco_results(big, classes, K, image_id=17, cat_ids=cat_ids, scores=scores, min_area=1)
    assert len(res) == k2
    want_table = labels.instance_table(fmask_np, k2)
    fcls_np, fscores_np = fcls.cpu().numpy(), fscores.cpu().numpy()
    for k, r in enumerate(res, start=1):
        assert sorted(r) == ["area", "bbox", "category_id", "image_id", "score", "segmentation"]
        assert r["image_id"] == 17 and r["segmentation"]["size"] == [H, W]
        own = fmask_np == k
        assert np.array_equal(rle.decode(rle.string_to_counts(r["segmentation"]["counts"]), H, W), own)
        assert r["area"] == int(own.sum())
        a, x0, y0, x1, y1 = (int(v) for v in want_table[k - 1])
        assert r["bbox"] == [float(x0), float(y0), float(x1 - x0 + 1), float(y1 - y0 + 1)]
        assert all(isinstance(v, float) for v in r["bbox"])
        assert r["category_id"] == cat_ids[int(fcls_np[k - 1])]
        assert r["score"] == float(fscores_np[k - 1])
    # without scores the results carry the reference's constant score 1 (segment.py:181)
    plain = merger.coco_results(big, classes, K, image_id=17, cat_ids=cat_ids)
    assert [r["score"] for r in plain] == [1] * k2
    assert [r["bbox"] for r in plain] == [r["bbox"] for r in res]
