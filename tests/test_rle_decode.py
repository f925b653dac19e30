"""The decoding half of the RLE path without a GPU: rle.label_mask against the reference's arithmetic, the native
string parser mn_rle_counts_host against rle.string_to_counts, the exports and Merger.decode_rle's signature."""
import ctypes
import inspect

import numpy as np
import pytest

from mergenet_amd import rle


def random_counts(rng, N, zero_runs=True):
    """Counts of a random binary mask over N scan positions, with zero-length runs put in when asked."""
    k = int(rng.integers(0, min(N, 12) + 1))
    cuts = np.sort(rng.integers(0, N + 1, k))
    counts = np.diff(np.concatenate([[0], cuts, [N]])).tolist()      # (equal cuts give zero-length runs already)
    if zero_runs and rng.random() < 0.5:
        at = int(rng.integers(0, len(counts) + 1))
        counts = counts[:at] + [0] * int(rng.integers(1, 6)) + counts[at:]
    return [int(c) for c in counts]


def reference_mask(all_counts, H, W, values):
    """The reference's statement, literally (utils/dataset.py:486-506 over maskUtils.decode)."""
    mask = np.zeros((H, W), np.uint16)
    for counts, v in zip(all_counts, values):
        m = rle.decode(counts, H, W).astype(np.uint16) * np.uint16(v)
        mask = m * (mask == 0) + mask
    return mask


def as_form(counts, H, W, form):
    if form == 0:
        return list(counts)
    s = rle.counts_to_string(counts)
    if form == 1:
        return s
    if form == 2:
        return s.decode("ascii")
    return {"size": [H, W], "counts": s if form == 3 else list(counts)}


def test_label_mask_is_the_reference_arithmetic():
    rng = np.random.default_rng(2024)
    for case in range(200):
        H, W = (1, 1) if case == 0 else (40, 53) if case == 1 else (int(rng.integers(1, 41)), int(rng.integers(1, 54)))
        A = 0 if case == 2 else 30 if case == 3 else int(rng.integers(0, 31))
        all_counts = [random_counts(rng, H * W) for _ in range(A)]
        items = [as_form(c, H, W, int(rng.integers(0, 5))) for c in all_counts]
        if case % 2:
            values = [int(v) for v in rng.integers(0, 5, A)]         # zeros and repeats
            got, area = rle.label_mask(items, H, W, values=values, return_area=True)
        else:
            values = list(range(1, A + 1))
            got, area = rle.label_mask(items, H, W, return_area=True)
        assert got.dtype == np.int32 and got.shape == (H, W) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, reference_mask(all_counts, H, W, values)), case
        assert area.dtype == np.int32 and area.tolist() == [sum(c[1::2]) for c in all_counts], case


def test_label_mask_refuses_what_decode_rle_refuses():
    good = [4, 2]
    with pytest.raises(ValueError):
        rle.label_mask([{"size": [3, 2], "counts": good}], 2, 3)
    with pytest.raises(ValueError):
        rle.label_mask([[4, 1]], 2, 3)
    with pytest.raises(ValueError):
        rle.label_mask([[7, -1]], 2, 3)
    with pytest.raises(ValueError):
        rle.label_mask([good], 2, 3, values=[-1])
    with pytest.raises(ValueError):
        rle.label_mask([good], 2, 3, values=[1, 2])
    with pytest.raises(ValueError):
        rle.label_mask([[1]] * 65536, 1, 1)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mergenet_amd import segmenter as seg
    return seg.load_library()


def native_counts(lib, s, capacity=None, guard=3):
    """(return value, the counts written, total, the words behind `capacity`)."""
    cap = len(s) if capacity is None else capacity
    buf = np.full(cap + guard, 0xDEADBEEF, np.uint32)
    total = ctypes.c_longlong(-1)
    n = lib.mn_rle_counts_host(s, len(s), buf.ctypes.data, cap, ctypes.byref(total))
    return n, buf[:cap], total.value, buf[cap:]


def test_native_parser_is_string_to_counts(lib):
    rng = np.random.default_rng(7)
    big = 2 ** 31 - 1
    lists = [[0], [5], [big], [3, 4], [0, big], [big, 0, big, 0, big], [1, big, big, 1, 0, 0, 17],
             [10, 20, 9, 21, 10, 1, 500000, 2, 1]]                                       # deltas of both signs
    for _ in range(60):
        n = int(rng.integers(1, 40))
        scale = [3, 40, 5000, 2 ** 20, big][int(rng.integers(0, 5))]
        lists.append([int(v) for v in rng.integers(0, scale + 1, n)])
    for counts in lists:
        s = rle.counts_to_string(counts)
        assert rle.string_to_counts(s) == counts
        n, got, total, behind = native_counts(lib, s)
        assert n == len(counts) and got[:n].tolist() == counts and total == sum(counts)
        assert (behind == 0xDEADBEEF).all()
        small = len(counts) // 2
        n, got, total, behind = native_counts(lib, s, capacity=small)     # too little room: the full number still
        assert n == len(counts) and got.tolist() == counts[:small] and total == sum(counts)
        assert (behind == 0xDEADBEEF).all()
    n, _, total, _ = native_counts(lib, b"")
    assert n == 0 and total == 0


def test_native_parser_refusals(lib):
    whole = rle.counts_to_string([100000, 5])
    assert native_counts(lib, whole)[0] == 2
    assert native_counts(lib, whole[:2])[0] < 0                       # ends inside the first count's groups
    assert native_counts(lib, rle.counts_to_string([-3]))[0] < 0      # a negative count
    assert native_counts(lib, rle.counts_to_string([5, 1, 2, -3]))[0] < 0          # a delta below minus the count two back
    assert native_counts(lib, rle.counts_to_string([2 ** 31]))[0] < 0                # does not fit 31 bits
    assert native_counts(lib, rle.counts_to_string([1, 2 ** 31 - 1, 1, 2 ** 31 + 4]))[0] < 0   # overflows by its delta
    assert native_counts(lib, rle.counts_to_string([2 ** 70]))[0] < 0
    assert native_counts(lib, b"\x05")[0] < 0                        # a byte below the alphabet


def test_exports_and_signature(lib):
    from mergenet_amd import segmenter as seg
    for name in ("mn_rle_counts_host", "mn_rle_decode_device"):
        assert name in seg.EXPORTS and hasattr(lib, name)
    assert lib.mn_rle_counts_host.restype is ctypes.c_longlong and len(lib.mn_rle_counts_host.argtypes) == 5
    assert lib.mn_rle_decode_device.restype is ctypes.c_int and len(lib.mn_rle_decode_device.argtypes) == 13
    sig = inspect.signature(seg.Merger.decode_rle)
    assert list(sig.parameters) == ["self", "rles", "height", "width", "values", "return_area"]
    assert sig.parameters["values"].default is None and sig.parameters["return_area"].default is False
    sig = inspect.signature(rle.label_mask)
    assert list(sig.parameters) == ["rles", "height", "width", "values", "return_area"]
    assert sig.parameters["values"].default is None and sig.parameters["return_area"].default is False
