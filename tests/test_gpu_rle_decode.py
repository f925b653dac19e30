"""Merger.decode_rle / mn_rle_decode_device against the numpy statement rle.label_mask.  Every comparison is
integer-exact."""
import ctypes
import functools

import numpy as np
import pytest

from mergenet_amd import labels, rle

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (5, 7),   # a segment shorter than a wave; a tile wider or taller than the image
          (64, 64),                           # one full segment per column
          (65, 130), (67, 129),               # segments and tiles that end past the image on both axes
          (130, 261)]                         # several tiles each way
KINDS = ["none", "empty", "full", "column_end", "long_run", "last_pixel", "labels", "rects2", "rects65", "rects300",
         "checker", "zeros_even", "zeros_odd"]


def rectangles(shape, n, seed):
    """n overlapping rectangles as binary masks; the second lies inside the first, which hides it entirely."""
    H, W = shape
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        b = np.zeros((H, W), np.uint8)
        if i == 1:
            ys, xs = np.nonzero(out[0])
            b[ys.min():(ys.min() + ys.max()) // 2 + 1, xs.min():(xs.min() + xs.max()) // 2 + 1] = 1
        else:
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            h, w = int(rng.integers(1, max(2, H // 3 + 1))), int(rng.integers(1, max(2, W // 3 + 1)))
            b[y:y + h, x:x + w] = 1
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def annotation_counts(kind, shape):
    """The counts lists of one annotation set."""
    H, W = shape
    N = H * W
    if kind == "none":
        return ()
    if kind == "empty":
        return ((N,),)
    if kind == "full":
        return ((0, N),)
    if kind == "column_end":                   # a run that ends exactly at a column's end, one that ends exactly at N
        s = H - min(H, 3)
        t = max(0, N - 5)
        return ((s, H - s, N - H), (t, N - t))
    if kind == "long_run":                     # one run longer than several columns
        s = H // 2
        length = min(N - s, 3 * H + 5)
        return ((s, length, N - s - length),)
    if kind == "last_pixel":
        return ((N - 1, 1),)
    if kind == "labels":                       # non-overlapping labels, encoded per label
        K = 300 if shape == SHAPES[-1] else 7
        rng = np.random.default_rng(11)
        if K == 300:
            lab = (np.arange(H)[:, None] // 9) * 21 + np.arange(W)[None, :] // 13 + 1
            lab = np.where(lab <= K, lab, 0)
        else:
            lab = np.kron(rng.integers(0, K + 1, ((H + 2) // 3, (W + 3) // 4)), np.ones((3, 4), np.int64))[:H, :W]
        return tuple(tuple(rle.binary_mask_counts(lab == k)) for k in range(1, K + 1))
    if kind.startswith("rects"):
        return tuple(tuple(rle.binary_mask_counts(b)) for b in rectangles(shape, int(kind[5:]), 5))
    if kind == "checker":                      # a run end at every position; the complement goes to annotation 2
        board = (np.arange(H)[:, None] + np.arange(W)[None, :]) % 2
        return (tuple(rle.binary_mask_counts(board)), (0, N))
    zeros = 200 if kind == "zeros_even" else 201           # in the middle of a column
    q = min(W - 1, 1) * H + H // 2
    u = min(5, N - q)
    return ((q // 2, q - q // 2) + (0,) * zeros + (u, N - q - u), (0, N))


@functools.lru_cache(maxsize=None)
def checker(kind, shape):
    H, W = shape
    mask, area = rle.label_mask([list(c) for c in annotation_counts(kind, shape)], H, W, return_area=True)
    mask.setflags(write=False)
    area.setflags(write=False)
    return mask, area


@pytest.fixture(scope="module")
def merger():
    from mergenet_amd import segmenter as seg
    m = seg.Merger(80, 160, 9, 10)
    yield m
    m.close()


def test_the_sets_hold_what_they_are_for():
    """(no device work) the properties the cases are chosen for."""
    assert len(annotation_counts("checker", (67, 129))[0]) > 1024          # more counts than one scan chunk
    # an end at every position but the first of a column (H even: the runs join there): 63 inside every segment
    assert len(annotation_counts("checker", (64, 64))[0]) == 64 * 64 - 63
    assert len(annotation_counts("checker", (65, 130))[0]) == 65 * 130      # (H odd: an end at every position)
    assert len(annotation_counts("labels", SHAPES[-1])) == 300
    hidden = rle.decode(list(annotation_counts("rects65", (65, 130))[1]), 65, 130)
    assert hidden.any() and not (checker("rects65", (65, 130))[0] == 2).any()
    assert checker("zeros_even", (65, 130))[0].tobytes() != checker("zeros_odd", (65, 130))[0].tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_decode_rle_is_label_mask(merger, kind, shape):
    H, W = shape
    want, want_area = checker(kind, shape)
    got, area = merger.decode_rle([list(c) for c in annotation_counts(kind, shape)], H, W, return_area=True)
    assert got.dtype == merger.torch.int32 and tuple(got.shape) == shape and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert area.dtype == merger.torch.int32 and np.array_equal(area.cpu().numpy(), want_area)   # hidden ones too


def test_values_class_ids_zeros_and_repeats(merger):
    shape = (65, 130)
    counts = [list(c) for c in annotation_counts("rects65", shape)]
    values = [int(v) for v in np.random.default_rng(3).integers(0, 4, len(counts))]
    values[0], values[1] = 0, 3                # a hidden annotation with value 0 in front of a visible one
    want = rle.label_mask(counts, *shape, values=values)
    assert (want == 3).any()
    got = merger.decode_rle(counts, *shape, values=values)
    assert np.array_equal(got.cpu().numpy(), want)
    same = [counts[0], counts[0]]              # the same pixels twice: value 0 claims nothing
    got = merger.decode_rle(same, *shape, values=[0, 5])
    assert np.array_equal(got.cpu().numpy(), rle.label_mask(same, *shape, values=[0, 5]))
    assert (got == 5).any()


def test_input_forms_give_the_same_mask(merger):
    shape = (67, 129)
    H, W = shape
    counts = [list(c) for c in annotation_counts("rects65", shape)]
    want = checker("rects65", shape)[0]
    strings = [rle.counts_to_string(c) for c in counts]
    forms = {"bytes": strings, "str": [s.decode("ascii") for s in strings], "lists": counts,
             "dicts": [{"size": [H, W], "counts": s} for s in strings],
             "dicts of lists": [{"size": [H, W], "counts": c} for c in counts],
             "mixed": [s if i % 2 else c for i, (s, c) in enumerate(zip(strings, counts))]}
    for name, items in forms.items():
        assert np.array_equal(merger.decode_rle(items, H, W).cpu().numpy(), want), name


def raw_decode(merger, counts, shape, mask, area=None):
    """mn_rle_decode_device itself, into the caller's `mask`."""
    torch = merger.torch
    H, W = shape
    flat = np.concatenate([np.asarray(c, np.int64) for c in counts]).astype(np.uint32).view(np.int32)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in counts])]).astype(np.int32)
    d_counts, d_starts = torch.from_numpy(flat).cuda(), torch.from_numpy(starts).cuda()
    ends = torch.empty((flat.size,), dtype=torch.int32, device="cuda")
    records = torch.empty((len(counts), 4), dtype=torch.int32, device="cuda")
    rc = merger.lib.mn_rle_decode_device(merger.handle, d_counts.data_ptr(), d_starts.data_ptr(), len(counts),
                                         int(flat.size), None, H, W, ends.data_ptr(), records.data_ptr(),
                                         mask.data_ptr(), area.data_ptr() if area is not None else None,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()


def test_mask_is_written_completely_and_twice_the_same(merger):
    torch = merger.torch
    for shape in ((5, 7), (67, 129)):
        counts = [list(c) for c in annotation_counts("rects65", shape)]
        first = torch.full(shape, -7, dtype=torch.int32, device="cuda")
        raw_decode(merger, counts, shape, first)
        assert np.array_equal(first.cpu().numpy(), checker("rects65", shape)[0])
        second = torch.full(shape, 12345, dtype=torch.int32, device="cuda")
        raw_decode(merger, counts, shape, second)
        assert torch.equal(first, second)
    none = torch.full((67, 129), -7, dtype=torch.int32, device="cuda")      # A == 0 writes zeros
    rc = merger.lib.mn_rle_decode_device(merger.handle, None, None, 0, 0, None, 67, 129, None, None, none.data_ptr(),
                                         None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and int(none.abs().sum().item()) == 0


def test_round_trip_through_encode_rle(merger):
    torch = merger.torch
    H, W, K = 67, 129, 9
    rng = np.random.default_rng(21)
    mask = np.kron(rng.integers(0, K + 1, ((H + 4) // 5, (W + 6) // 7)), np.ones((5, 7), np.int64))[:H, :W]
    mask = np.ascontiguousarray(mask, np.int32)
    res = merger.encode_rle(torch.from_numpy(mask).cuda(), K)
    assert len(res) == K
    back, area = merger.decode_rle(res, H, W, values=[r["label"] for r in res], return_area=True)
    assert np.array_equal(back.cpu().numpy(), mask)
    assert area.cpu().numpy().tolist() == [r["area"] for r in res]


def test_overlap_table_takes_a_decoded_truth(merger):
    torch = merger.torch
    shape = (65, 130)
    counts = [list(c) for c in annotation_counts("labels", shape)]
    G, K = len(counts), 65
    pred = checker("rects65", shape)[0]
    truth = merger.decode_rle([rle.counts_to_string(c) for c in counts], *shape)
    got = merger.overlap_table(torch.from_numpy(np.array(pred)).cuda(), truth, K, G)
    assert np.array_equal(got.cpu().numpy(), labels.overlap_table(pred, checker("labels", shape)[0], K, G))


def test_refusals_come_before_any_launch(merger):
    torch = merger.torch
    H, W = 5, 7
    good = [4, 2, 29]
    merger.decode_rle([good], H, W)                          # (the scratch exists from here on)
    merger._rld_rec.fill_(-7)                                # the scan kernel writes a record per annotation
    truncated = rle.counts_to_string([100000, 5])[:2]
    bad_calls = {
        "size": lambda: merger.decode_rle([{"size": [W, H], "counts": good}], H, W),
        "sum": lambda: merger.decode_rle([[4, 2, 28]], H, W),
        "sum of a string": lambda: merger.decode_rle([rle.counts_to_string([4, 2, 30])], H, W),
        "negative count": lambda: merger.decode_rle([[6, -2, 31]], H, W),
        "negative count in a string": lambda: merger.decode_rle([rle.counts_to_string([6, -2, 31])], H, W),
        "negative value": lambda: merger.decode_rle([good], H, W, values=[-1]),
        "values length": lambda: merger.decode_rle([good, good], H, W, values=[1]),
        "too many": lambda: merger.decode_rle([[1]] * 65536, 1, 1),
        "malformed string": lambda: merger.decode_rle([truncated], H, W),
        "count beyond 31 bits": lambda: merger.decode_rle([rle.counts_to_string([2 ** 31, 0])], H, W),
    }
    for name, call in bad_calls.items():
        with pytest.raises(ValueError):
            call()
        assert int((merger._rld_rec != -7).sum().item()) == 0, name
