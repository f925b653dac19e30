"""The resize, RLE and wire kernels (mn_kernels_prepare.h, mn_pack_wire) against plain statements, at their edges.

References: the float64 / integer statements of mergenet_amd/resize.py (cv2's INTER_NEAREST and INTER_LINEAR, from
OpenCV's published source -- cv2 is not installed, nothing here was compared with a run of it), rle.binary_mask_counts /
counts_to_string, distributed.pack_runs_cpu / unpack_runs_cpu and labels.sameness_targets.  Everything is compared for
integer or bit equality, except Merger.prepare, which is held to the per-element bound derived in resize_util.py.
Shapes are the smallest at which each kernel takes another path: sizes below, at and one past a block of 256 lanes
or of 1024 items, one pixel, one row, one column, a capacity met exactly and missed by one.
"""
import functools
import struct

import numpy as np
import pytest

from mergenet_amd import distributed as mnd
from mergenet_amd import labels, resize, rle

pytestmark = pytest.mark.gpu

MAX_OFFSETS = 32          # MN_MAX_OFFSETS


@pytest.fixture(scope="module")
def merger():
    """A context for the calls that are not held to its capacity (prepare, upsample_mask, sameness_targets) and, with
    its 4096 pixels, for the small RLE and run-length cases."""
    from mergenet_amd import segmenter as seg
    m = seg.Merger(64, 64, 2, 2)
    yield m
    m.close()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 2. upsample_mask: cv2's INTER_NEAREST index, in double ---------------------------------------------------------

NEAREST_PAIRS = [(8, 82), (8, 98), (8, 196), (24, 34), (24, 260), (33, 27), (39, 15), (1, 7), (7, 1), (5, 5),
                 (1000, 1040)]


@pytest.mark.parametrize("axis", ["columns", "rows"])
@pytest.mark.parametrize("pair", NEAREST_PAIRS, ids=lambda p: "%dto%d" % p)
def test_upsample_mask_is_cv2_nearest(merger, pair, axis):
    """Every pixel of the source distinct (arange), the pair on one axis and 3 -> 4 on the other, so a wrong or a
    swapped index shows; equality with resize.upsample_mask.  24 -> 260 and 1000 -> 1040 cross the 256-lane block.
    A float32 index (torch's mode="nearest") fails here at, for instance, 8 -> 82 index 41 (3 for 4), 8 -> 98 index
    49 (4 for 3), 8 -> 196 indices 49, 98, 147 and at 30 indices of 1000 -> 1040."""
    src, dst = pair
    (Hin, Ho), (Win, Wo) = ((3, 4), (src, dst)) if axis == "columns" else ((src, dst), (3, 4))
    mask = np.arange(Hin * Win, dtype=np.int32).reshape(Hin, Win)
    want = resize.upsample_mask(mask, Ho, Wo)
    got = merger.upsample_mask(cuda(mask), Ho, Wo).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.int32
    if not np.array_equal(got, want):
        ys, xs = np.nonzero(got != want)
        bad = sorted(set((xs if axis == "columns" else ys).tolist()))
        line = (lambda a: a[0, bad] % Win) if axis == "columns" else (lambda a: a[bad, 0] // Win)
        raise AssertionError("%d -> %d on the %s: %d wrong, at destination indices %s: source index %s, cv2 takes %s"
                             % (src, dst, axis, len(ys), bad, line(got).tolist(), line(want).tolist()))


# ---- 3. prepare: cv2's INTER_LINEAR blend in float64, derived bound --------------------------------------------------

PREPARE_SHAPES = [((2, 5, 2048), (7, 1333)), ((2, 6, 667), (9, 1333)), ((1, 8, 2047), (3, 1000)), ((3, 1, 9), (4, 9)),
                  ((3, 9, 1), (9, 5)), ((1, 17, 9), (1, 1)), ((2, 33, 47), (64, 257))]
DTYPES = ["float32", "float16", "bfloat16"]


def torch_dtype(name):
    import torch
    return getattr(torch, name)


@functools.lru_cache(maxsize=None)
def prepare_case(shape, in_dtype, sigmoid):
    """(input tensor on the GPU in `in_dtype`, the values the statement blends as float64 [K,H,W]).  The 16-bit
    input is rounded first and widened exactly, so statement and kernel see the same values."""
    import torch
    (K, H, W), _ = shape
    rng = np.random.default_rng(K * 1000003 + H * 1009 + W)
    x = (rng.standard_normal((K, H, W)) * 3 if sigmoid else rng.random((K, H, W))).astype(np.float32)
    t = torch.from_numpy(x).to(torch_dtype(in_dtype))
    seen = t.to(torch.float64).numpy()
    return t.cuda().contiguous(), (resize.sigmoid(seen) if sigmoid else seen), seen


@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("in_dtype", DTYPES)
@pytest.mark.parametrize("shape", PREPARE_SHAPES, ids=lambda s: "%dx%dx%d-%dx%d" % (s[0] + s[1]))
def test_prepare_within_the_derived_bound_of_the_float64_statement(merger, shape, in_dtype, out_dtype):
    """Merger.prepare against resize.prepare_maps, sigmoid and clip on and off, every element within the bound of
    resize_util.prepare_bound -- derived there from the statement: the coordinate error (4 * 2^-24 of the
    coordinate's magnitude) times the difference of the blended neighbours (and of the adjacent segments, for a
    coordinate that straddles a pixel), 4 * eps32 of the blended magnitude for the two blends, 3 * eps32 of it for
    mn_sigmoid's expf, sum and division, 2^-126, and half an ulp of a 16-bit output.  A fixed 2e-6 holds only for
    narrow maps: at 2048 -> 1333 the float32 coordinate is off by up to 1e-4 of a pixel times the local slope.
    Measured on an MI355X, greatest error as a share of its bound: float32 out 0.493 (2048 -> 1333, bfloat16 in,
    1.19e-4 absolute); float16 out 0.998 and bfloat16 out 1.000 to three places (the half ulp of the
    store is nearly all of the bound there, and a value halfway between two 16-bit neighbours uses all of it)."""
    import resize_util as ru
    (K, H, W), (Ho, Wo) = shape
    worst = 0.0
    for sigmoid in (False, True):
        x, p, seen = prepare_case(shape, in_dtype, sigmoid)
        for clip in (False, True):
            ref = resize.prepare_maps(seen, Ho, Wo, sigmoid, clip)
            bound = ru.prepare_bound(p, Ho, Wo, sigmoid, out_dtype, ref)
            got = merger.prepare(x, Ho, Wo, apply_sigmoid=sigmoid, clip=clip, out_dtype=torch_dtype(out_dtype))
            assert got.dtype == torch_dtype(out_dtype) and tuple(got.shape) == (K, Ho, Wo)
            err = np.abs(got.double().cpu().numpy() - ref)
            share = float((err / bound).max())
            worst = max(worst, share)
            print("prepare %s %s->%s sigmoid=%d clip=%d: max error %.3e, max bound %.3e, greatest share %.3f"
                  % (shape, in_dtype, out_dtype, sigmoid, clip, err.max(), bound.max(), share))
            assert share <= 1.0, (sigmoid, clip, float(err.max()))
    print("prepare worst share of the bound %s %s->%s: %.3f" % (shape, in_dtype, out_dtype, worst))


def test_prepare_saturated_logits_give_exactly_the_clip_values(merger):
    """Sigmoid and clip on, float32 out: logits 30, 100, +inf give exactly 1 - eps32 and -30, -100, -inf exactly eps32
    -- constant planes and planes that mix the three of one sign, growing, shrinking and at the input's size."""
    eps = np.float32(np.finfo(np.float32).eps)
    rng = np.random.default_rng(12)
    high = [np.full((5, 9), v) for v in (30.0, 100.0, np.inf)] + [rng.choice([30.0, 100.0, np.inf], (5, 9))]
    low = [-a for a in high]
    x = np.stack(high + low).astype(np.float32)
    for Ho, Wo in [(7, 13), (5, 9), (3, 4), (11, 300)]:
        got = merger.prepare(cuda(x), Ho, Wo, apply_sigmoid=True, clip=True).cpu().numpy()
        want = np.empty((8, Ho, Wo), np.float32)
        want[:4], want[4:] = np.float32(1) - eps, eps
        assert got.dtype == np.float32 and np.array_equal(got, want), (Ho, Wo)
        assert np.array_equal(resize.prepare_maps(x, Ho, Wo, True, True), want.astype(np.float64))


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_prepare_nan_logit_gives_nan(merger, out_dtype):
    """Clip off: a NaN logit makes NaN of every output that blends it (weight 0 included: NaN * 0 is NaN) and of no
    other, in all three output types, with and without the sigmoid -- at the input's size and at exactly twice it,
    where float32 and double coordinates are the same numbers, so the set is the statement's."""
    rng = np.random.default_rng(13)
    x = rng.standard_normal((2, 5, 9)).astype(np.float32)
    x[0, 2, 4] = x[1, 0, 0] = x[1, 4, 8] = np.nan
    for Ho, Wo in [(5, 9), (10, 18)]:
        for sigmoid in (False, True):
            want = np.isnan(resize.prepare_maps(x, Ho, Wo, sigmoid, clip=False))
            got = merger.prepare(cuda(x), Ho, Wo, apply_sigmoid=sigmoid, clip=False, out_dtype=torch_dtype(out_dtype))
            got = np.isnan(got.double().cpu().numpy())
            assert want.any() and not want.all() and np.array_equal(got, want), (Ho, Wo, sigmoid)


# ---- 4. encode_rle at its edges ---------------------------------------------------------------------------------------

def rle_reference(mask, K):
    return [(rle.counts_to_string(rle.binary_mask_counts(mask == k)), int((mask == k).sum())) for k in range(1, K + 1)]


def check_rle(m, mask, K):
    """encode_rle of `mask` on Merger `m` against the per-label host encoding: strings, areas, labels, sizes."""
    H, W = mask.shape
    res = m.encode_rle(cuda(mask.astype(np.int32)), K)
    want = rle_reference(mask, K)
    assert [e["label"] for e in res] == list(range(1, K + 1))
    assert [(e["counts"], e["area"]) for e in res] == want
    assert all(e["size"] == [H, W] for e in res)
    kept = m.encode_rle(cuda(mask.astype(np.int32)), K, drop_zero_area=True)
    assert [(e["label"], e["counts"]) for e in kept] == [(k + 1, want[k][0]) for k in range(K) if want[k][1] > 0]
    return res


def column_major(flat, H, W):
    """The [H,W] mask whose column-major scan (the order of COCO's RLE and of mn_rle_count) is `flat`."""
    return np.ascontiguousarray(np.asarray(flat, np.int32).reshape(W, H).T)


def blobs(H, W, K, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.int32)
    for k in range(1, K + 1):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[max(0, y - H // 6):y + H // 6 + 1, max(0, x - W // 6):x + W // 6 + 1] = k
    return m


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1)])
def test_encode_rle_one_pixel_one_row_one_column(merger, shape):
    H, W = shape
    n = H * W
    for flat in (np.ones(n), np.zeros(n), np.arange(n) % 3, (np.arange(n) // 5) % 3, 2 - (np.arange(n) % 3)):
        check_rle(merger, column_major(flat, H, W), 2)


@pytest.mark.parametrize("shape", [(33, 31), (32, 32), (41, 25)], ids=["1023", "1024", "1025"])
def test_encode_rle_round_the_first_block_of_1024_items(merger, shape):
    """H * W = 1023, 1024, 1025: a block of mn_rle_count holds 1024 scan positions.  A non-zero label at position 0
    (the change point whose predecessor is the implicit 0), a change at position 1023 (the last item of block 0) and
    one exactly at position 1024 (the first item of block 1, whose predecessor lies in block 0) -- each where the
    image has that position, else at its last one."""
    H, W = shape
    n = H * W
    assert n in (1023, 1024, 1025)
    flat = np.zeros(n, np.int32)
    flat[0] = 2
    flat[5:700] = 1
    flat[900:] = 3
    flat[min(1023, n - 1):] = 1
    flat[min(1024, n - 1):] = 2
    check_rle(merger, column_major(flat, H, W), 3)
    flat[:] = 3                             # and no change but the one at position 0
    flat[min(1024, n - 1):] = 1
    check_rle(merger, column_major(flat, H, W), 3)


def test_encode_rle_column_longer_than_a_block():
    """1100 x 3: one column spans two blocks of 1024 scan positions, and a block two columns."""
    from mergenet_amd import segmenter as seg
    m = seg.Merger(1100, 3, 2, 2)
    try:
        mask = np.zeros((1100, 3), np.int32)
        mask[10:1030, 0] = 1
        mask[1024:, 1] = 2
        mask[:924, 2] = 2
        mask[1000:1099, 2] = 3
        check_rle(m, mask, 3)
        check_rle(m, (np.arange(3300).reshape(1100, 3) // 7 % 4).astype(np.int32), 3)
    finally:
        m.close()


def test_encode_rle_empty_and_full_masks(merger):
    """All background with K = 3: three zero-area entries (the string of an empty mask is its pixel count), and
    nothing with drop_zero_area.  One label filling the image: [0, H * W]."""
    zero = np.zeros((20, 30), np.int32)
    res = check_rle(merger, zero, 3)
    assert [e["area"] for e in res] == [0, 0, 0] and res[0]["counts"] == rle.counts_to_string([600])
    assert merger.encode_rle(cuda(zero), 3, drop_zero_area=True) == []
    assert merger.encode_rle(cuda(zero), 0) == []
    res = check_rle(merger, np.full((20, 30), 2, np.int32), 2)
    assert res[1]["counts"] == rle.counts_to_string([0, 600]) and res[1]["area"] == 600 and res[0]["area"] == 0


def test_encode_rle_retries_past_its_capacity_and_stays_right():
    """A 40 x 40 checkerboard of two labels changes label at 1561 of its 1600 scan positions (all but the 39 column
    starts after the first), the first buffer of a Merger holds 1024: mn_rle_points_device reports the count,
    encode_rle allocates and runs again.  The strings must be right, and so must those of a blob mask encoded next on
    the same Merger (with the grown buffer)."""
    from mergenet_amd import segmenter as seg
    H = W = 40
    m = seg.Merger(H, W, 2, 2)
    try:
        board = (1 + (np.add.outer(np.arange(H), np.arange(W)) % 2)).astype(np.int32)
        scan = board.reshape(-1, order="F")
        assert int(np.count_nonzero(scan != np.concatenate([[0], scan[:-1]]))) == 1561 > max(1024, H * W // 16) == 1024
        check_rle(m, board, 2)
        assert m._rle_cap == 1561
        check_rle(m, blobs(H, W, 4, 5), 4)
        check_rle(m, board.T.copy() * (np.arange(W) % 3 > 0), 2)
    finally:
        m.close()


def test_encode_rle_ignores_labels_outside_its_range(merger):
    """A label above num_instances and a negative (ignore) label in the mask: mn_rle_encode_host ignores them -- they
    get no string, and in the strings of the others they count as zeros, as `mask == k` does (the promise of the
    header, include/mergenet_hip.h)."""
    mask = blobs(33, 47, 4, 8)
    mask[0:3, 0:5] = 9
    mask[30:, 40:] = -1
    mask[10:14, 10:30] = -7
    mask[5, :] = 6
    assert set(np.unique(mask)) >= {-7, -1, 6, 9} and (mask == 2).any()
    check_rle(merger, mask, 4)
    check_rle(merger, mask, 2)              # labels 3 and 4 are now above the count too


def test_encode_rle_more_than_1024_blocks():
    """1030 x 1100 with 5 instances: 1107 blocks of 1024 scan positions, so mn_rank_scan goes round its loop a second
    time (blocks 1024..1106) and carries the sum of the first pass."""
    from mergenet_amd import segmenter as seg
    H, W = 1030, 1100
    m = seg.Merger(H, W, 2, 2)
    try:
        mask = blobs(H, W, 5, 21)
        mask[:, 1060:1090] = 5              # (runs in the blocks of the second pass, whatever the blobs did)
        mask[100:900, 1075] = 3
        assert -(-H * W // 1024) == 1107
        check_rle(m, mask, 5)
    finally:
        m.close()


# ---- 5. run-length wire and int16 wire at their edges ------------------------------------------------------------------

GUARD = 8


def check_pack_runs(m, mask, classes, cap, max_instances, logprob):
    """pack_runs of `mask` on Merger `m` against pack_runs_cpu, word for word over the sections the header defines as
    written -- header, min(count, cap) positions, as many int16 labels, max_instances int8 classes -- with guard words
    behind the wire; then unpack_runs against the mask (zeros for a wire that reports overflow).  Returns the count."""
    import torch
    from mergenet_amd import segmenter as seg
    mask = np.ascontiguousarray(mask, np.int32)
    H, W = mask.shape
    K = len(classes)
    words = seg.runs_wire_words(cap, max_instances)
    assert words == 4 + cap + (cap + 1) // 2 + (max_instances + 3) // 4
    table = torch.full((max(H * W, max_instances),), -1, dtype=torch.int32)
    table[:K] = torch.tensor(classes, dtype=torch.int32)
    buf = torch.full((words + GUARD,), 777, dtype=torch.int32, device="cuda")
    wire = buf[:words]
    seg.pack_runs(m, cuda(mask), table.cuda(), K, wire, cap, max_instances, logprob)
    got = buf.cpu()
    ref = mnd.pack_runs_cpu(torch.from_numpy(mask), table, K, logprob, cap, max_instances)
    flat = mask.reshape(-1)
    count = int(np.count_nonzero(flat != np.concatenate([[0], flat[:-1]])))
    assert int(ref[0]) == (count if count <= cap else -1)
    assert got[:4].tolist() == ref[:4].tolist()                    # count or -1, K, the float64's two words
    n = min(count, cap)
    assert torch.equal(got[4:4 + n], ref[4:4 + n])
    lab = slice(4 + cap, 4 + cap + (cap + 1) // 2)
    assert torch.equal(got[lab].view(torch.int16)[:n], ref[lab].view(torch.int16)[:n])
    assert torch.equal(got[lab.stop:words].view(torch.int8)[:max_instances],
                       ref[lab.stop:].view(torch.int8)[:max_instances])
    assert bool((got[words:] == 777).all())
    m2, t2 = seg.unpack_runs(wire, H, W, cap, max_instances)
    assert torch.equal(m2.cpu(), torch.from_numpy(mask if count <= cap else np.zeros_like(mask)))
    assert t2.cpu().tolist() == list(classes) + [-1] * (max_instances - K)
    if count <= cap:
        cm, ct, ck, cl = mnd.unpack_runs_cpu(got[:words], H, W, cap, max_instances)
        assert torch.equal(cm, torch.from_numpy(mask)) and ck == K and struct.pack("<d", cl) == struct.pack("<d", logprob)
    return count


def alternating(changes, n):
    """A flat mask of n pixels whose change points are exactly the positions 0 .. changes - 1."""
    flat = np.zeros(n, np.int32)
    flat[:changes] = (np.arange(changes) + 1) % 2
    flat[changes:] = flat[changes - 1]
    return flat


def test_pack_runs_capacity_met_exactly_and_missed_by_one(merger):
    """cap change points fit (header cap, every slot of the positions and labels used); cap + 1 do not: header -1,
    nothing behind the wire touched, unpack gives zeros.  An odd capacity too (the labels end in half a word)."""
    for cap in (64, 65):
        for shape in ((10, 20), (1, 200)):
            n = shape[0] * shape[1]
            assert check_pack_runs(merger, alternating(cap, n).reshape(shape), [5, 6], cap, 16, -1.5) == cap
            assert check_pack_runs(merger, alternating(cap + 1, n).reshape(shape), [5, 6], cap, 16, -1.5) == cap + 1
            assert check_pack_runs(merger, alternating(cap - 1, n).reshape(shape), [5, 6], cap, 16, -1.5) == cap - 1


def test_pack_runs_empty_mask_first_pixel_and_class_range(merger):
    """All zeros: header 0, unpacks to zeros.  mask[0] != 0: the first change point is position 0.  num_instances ==
    max_instances: no -1 padding left.  Classes 0 and 127, the ends of the int8 range the wire carries."""
    assert check_pack_runs(merger, np.zeros((7, 9), np.int32), [], 64, 16, 0.0) == 0
    assert check_pack_runs(merger, np.zeros((7, 9), np.int32), [3], 64, 16, float("inf")) == 0
    first = np.zeros((7, 9), np.int32)
    first[0, 0] = 3
    assert check_pack_runs(merger, first, [1, 2, 3], 64, 16, -0.0) == 2
    assert check_pack_runs(merger, np.full((7, 9), 2, np.int32), [1, 2], 64, 16, 5e-324) == 1
    rng = np.random.default_rng(31)
    full = np.repeat(rng.integers(0, 17, (6, 4)), 5, axis=1).astype(np.int32)
    classes = [0, 127] + [int(c) for c in rng.integers(0, 128, 14)]
    check_pack_runs(merger, full, classes, 128, 16, -4321.125)       # K = max_instances = 16, label 16 in the mask
    check_pack_runs(merger, full % 3, [127, 0], 128, 2, 1.0)          # ... and = 2
    check_pack_runs(merger, full % 2, [0], 128, 1, 1.0)               # one class byte in a word of its own


@pytest.mark.parametrize("shape", [(1, 1), (33, 31), (32, 32), (41, 25)], ids=["1", "1023", "1024", "1025"])
def test_pack_runs_round_a_block_of_1024_pixels(merger, shape):
    """n_pixels = 1, 1023, 1024, 1025 (a block of mn_runs_count holds 1024): run masks, one with a change at the last
    pixel, one with changes at pixels 1023 and 1024 where they exist."""
    H, W = shape
    n = H * W
    rng = np.random.default_rng(n)
    runs = np.repeat(rng.integers(0, 4, n // 5 + 1), 5)[:n].astype(np.int32)
    check_pack_runs(merger, runs.reshape(H, W), [1, 2, 3], 1100, 16, -2.0)
    edge = np.ones(n, np.int32)
    edge[n - 1:] = 2
    check_pack_runs(merger, edge.reshape(H, W), [1, 2], 64, 16, -2.0)
    edge[min(1023, n - 1):] = 3
    edge[min(1024, n - 1):] = 1
    check_pack_runs(merger, edge.reshape(H, W), [1, 2, 3], 64, 16, -2.0)
    check_pack_runs(merger, np.zeros((H, W), np.int32), [], 64, 16, -2.0)


def test_unpack_runs_batch_with_an_overflowed_wire(merger):
    """unpack_runs_batch, count = 3, the middle wire with header -1 (its mask had more change points than the
    capacity): zeros for that mask, its class table and the other two masks intact."""
    import torch
    from mergenet_amd import segmenter as seg
    H, W, cap, mi = 20, 30, 64, 16
    words = seg.runs_wire_words(cap, mi)
    rng = np.random.default_rng(41)
    masks = [np.repeat(rng.integers(0, 4, (20, 3)), 10, axis=1).astype(np.int32),
             rng.integers(0, 4, (H, W)).astype(np.int32),
             np.repeat(rng.integers(0, 4, (20, 2)), 15, axis=1).astype(np.int32)]
    wires = torch.zeros((3, words), dtype=torch.int32, device="cuda")
    for r, mk in enumerate(masks):
        table = torch.full((H * W,), -1, dtype=torch.int32)
        table[:3] = torch.tensor([1 + r, 2 + r, 3 + r], dtype=torch.int32)
        seg.pack_runs(merger, cuda(mk), table.cuda(), 3, wires[r], cap, mi, -1.0 * r)
    assert wires[:, 0].tolist()[1] == -1 and 0 < int(wires[0, 0]) <= cap and 0 < int(wires[2, 0]) <= cap
    got_m, got_t = seg.unpack_runs_batch(wires, H, W, cap, mi)
    for r in range(3):
        assert np.array_equal(got_m[r].cpu().numpy(), masks[r] if r != 1 else np.zeros((H, W), np.int32))
        assert got_t[r].cpu().tolist() == [1 + r, 2 + r, 3 + r] + [-1] * (mi - 3)


def wire16_reference(flat, classes, max_instances, logprob):
    """The int16 wire as distributed.py lays it out: labels, K, classes padded with -1, the float64 as four 16-bit
    words, low word first."""
    K = len(classes)
    tail = np.frombuffer(struct.pack("<d", logprob), dtype="<i2")
    return np.concatenate([np.asarray(flat, np.int16), [K], np.asarray(classes, np.int16).reshape(-1),
                           np.full(max_instances - K, -1, np.int16), tail]).astype(np.int16)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1027])
def test_pack_wire_small_pixel_counts_and_any_base(n):
    """mn_pack_wire packs four pixels per lane and the rest one by one: n_pixels below, at and past 4, and 1027 (four
    blocks of 256 lanes, three left over).  num_instances 0 and max_instances; the float64 words bit for bit for -0.0,
    inf, NaN and a denormal; guard words on both sides of the wire.  The wire starts at an 8-byte boundary, 2 bytes
    past one and 4 past (as the second wire of a batch buffer does): the vector store is taken only at the first."""
    import torch
    from mergenet_amd import segmenter as seg
    mi = 16
    words = n + 1 + mi + 4
    rng = np.random.default_rng(n)
    specials = [-0.0, float("inf"), float("nan"), 5e-324]
    case = 0
    for K in (0, mi):
        for lead in (8, 9, 10):
            flat = rng.integers(0, K + 1, n).astype(np.int32)
            classes = [int(c) for c in rng.integers(0, 128, K)]
            logprob = specials[case % 4]
            case += 1
            table = torch.full((max(n, mi),), -1, dtype=torch.int32)
            table[:K] = torch.tensor(classes, dtype=torch.int32)
            buf = torch.full((lead + words + GUARD,), 12345, dtype=torch.int16, device="cuda")
            seg.pack_wire(cuda(flat.reshape(1, n)), table.cuda(), K, buf[lead:lead + words], mi, logprob)
            got = buf.cpu().numpy()
            assert (got[:lead] == 12345).all() and (got[lead + words:] == 12345).all(), (K, lead)
            assert np.array_equal(got[lead:lead + words], wire16_reference(flat, classes, mi, logprob)), (K, lead)


def test_pack_wire_mask_that_is_a_plane_of_a_larger_tensor():
    """The mask may be plane 1 of a [2, 3, 5] tensor, 60 bytes in: no 16-byte load fits that base."""
    import torch
    from mergenet_amd import segmenter as seg
    rng = np.random.default_rng(3)
    planes = rng.integers(0, 5, (2, 3, 5)).astype(np.int32)
    table = torch.tensor([7, 8, 9, 10], dtype=torch.int32).cuda()
    buf = torch.full((15 + 1 + 4 + 4 + GUARD,), 12345, dtype=torch.int16, device="cuda")
    seg.pack_wire(cuda(planes)[1], table, 4, buf[:24], 4, -3.25)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:24], wire16_reference(planes[1].reshape(-1), [7, 8, 9, 10], 4, -3.25))
    assert (got[24:] == 12345).all()


@pytest.mark.parametrize("shape", [(33, 47), (32, 48)])
def test_mask_exchange_batch_of_two_with_an_overflowing_mask(shape):
    """MaskExchange on one GPU, no process group, fmt="runs", batch=2: the path of the library's own caller.  Each
    batch carries a mask that fits the run-length wire and a noisy one that does not (header -1), in both orders;
    both come back equal -- the noisy one through _int16_fallback, from the int16 copy staged at submit time -- with
    their class tables, counts and log-likelihoods.  The staged copy of the second submit starts
    n_pixels + 1 + 4096 + 4 int16 elements into its buffer: 5652 for 33 x 47 (an 8-byte boundary), 5637 for 32 x 48
    (an odd element: mn_pack_wire must not take its 8-byte stores there)."""
    import torch
    from mergenet_amd import segmenter as seg
    H, W = shape
    n = H * W
    assert (n + 1 + mnd.MAX_INSTANCES + 4) % 2 == (0 if shape == (33, 47) else 1)
    rng = np.random.default_rng(n)
    fit = np.zeros((H, W), np.int32)
    fit[3:8, 5:30] = 2
    fit[10:20, 25:47] = 5
    fit[0, 0] = 1
    noisy = rng.integers(0, 6, (H, W)).astype(np.int32)
    cap = mnd.runs_capacity(n)
    changes = lambda a: int(np.count_nonzero(a.reshape(-1) != np.concatenate([[0], a.reshape(-1)[:-1]])))
    assert changes(fit) <= cap < changes(noisy)
    items = {"fit": (fit, [3, 1, 4, 1, 5], -77.125), "noisy": (noisy, [9, 0, 127, 2, 6], -3.5)}
    merger = seg.Merger(H, W, 3, 2)
    try:
        ex = mnd.MaskExchange(H, W, torch.device("cuda", 0), fmt="runs", merger=merger, batch=2)
        for order in (("fit", "noisy"), ("noisy", "fit")):
            handles = []
            for name in order:
                mask, classes, lp = items[name]
                table = torch.full((n,), -1, dtype=torch.int32)
                table[:5] = torch.tensor(classes, dtype=torch.int32)
                handles.append(ex.submit(cuda(mask), table.cuda(), 5, lp))
            for name, h in zip(order, handles):
                mask, classes, lp = items[name]
                masks, tabs, counts = ex.result(h)
                assert tuple(masks.shape) == (1, H, W) and masks.dtype == torch.int32 and tabs.dtype == torch.int32
                assert np.array_equal(masks[0].cpu().numpy(), mask), (order, name)
                assert tabs[0].cpu().tolist() == classes + [-1] * (mnd.MAX_INSTANCES - 5)
                assert counts.cpu().tolist() == [5] and ex.logprobs(h).cpu().tolist() == [lp]
                slot, pos = divmod(h, 2)
                assert ((slot, pos) in ex.fallback) == (name == "noisy")
        ex.drain()
    finally:
        merger.close()


# ---- 6. sameness_targets -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (37, 53)])
def test_sameness_targets_equal_the_roll_definition_at_the_edges(merger, shape):
    """Merger.sameness_targets against labels.sameness_targets (the np.roll definition, utils/dataset.py:259-277),
    bit for bit: offset (0, 0) and offsets that reach past the image (all ones), negative and mixed-sign offsets, and
    a full list of MN_MAX_OFFSETS offsets; masks with negative (ignore) labels, compared as plain integers."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    edge = [(0, 0), (H, 0), (0, W), (-H, 0), (0, -W), (H + 5, -W - 5), (-1, 0), (0, -1), (-1, -1), (1, -1), (-1, 1),
            (2, 3), (-3, 2), (H - 1, 0), (0, W - 1), (-(H - 1), -(W - 1)), (H - 1, -(W - 1))]
    full = [(int(i), int(j)) for i, j in zip(rng.integers(-H - 1, H + 2, MAX_OFFSETS),
                                             rng.integers(-W - 1, W + 2, MAX_OFFSETS))]
    for low in (0, -2):
        mask = np.repeat(rng.integers(low, 4, (H, (W + 2) // 3)), 3, axis=1)[:, :W].astype(np.int32)
        assert low == 0 or (mask < 0).any() or H * W == 1
        for offs in (edge, full):
            want = labels.sameness_targets(mask, offs)
            got = merger.sameness_targets(cuda(mask), offs).cpu().numpy()
            assert got.dtype == np.float32 and np.array_equal(got, want)
            if offs is edge:
                assert want[:6].all() and (H * W == 1 or not want.all())
