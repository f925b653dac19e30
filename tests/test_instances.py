"""Instance table and small-instance filter: the numpy checkers (mergenet_amd/labels.py) on known answers, their
areas against the native RLE encoder's, and the two new entry points of the C ABI (no GPU)."""
import ctypes
import os
import re

import numpy as np

from mergenet_amd import labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_of_a_single_pixel():
    assert labels.instance_table(np.array([[1]], np.int32), 1).tolist() == [[1, 0, 0, 0, 0]]
    assert labels.instance_table(np.array([[0]], np.int32), 1).tolist() == [[0, 1, 1, -1, -1]]
    assert labels.instance_table(np.array([[0]], np.int32), 0).shape == (0, 5)


def test_table_of_two_instances_and_a_label_that_never_occurs():
    m = np.array([[1, 1, 0, 3],
                  [0, 1, 0, 3],
                  [0, 0, 0, 3]], np.int32)
    t = labels.instance_table(m, 3)
    assert t.dtype == np.int32
    assert t.tolist() == [[3, 0, 0, 1, 1],       # {area, x_min, y_min, x_max, y_max}, maxima inclusive
                          [0, 4, 3, -1, -1],     # label 2 has no pixel: {0, W, H, -1, -1}
                          [3, 3, 0, 3, 2]]
    # labels beyond K are not counted
    assert labels.instance_table(m, 2).tolist() == t[:2].tolist()


def test_table_of_an_instance_touching_all_four_borders():
    m = np.zeros((5, 7), np.int32)
    m[0, 3] = m[4, 2] = m[2, 0] = m[1, 6] = 2
    m[2, 2:5] = 1
    t = labels.instance_table(m, 2)
    assert t.tolist() == [[3, 2, 2, 4, 2], [4, 0, 0, 6, 4]]


def _random_case(rng, K=7):
    H, W = (int(x) for x in rng.integers(1, 14, 2))
    m = rng.integers(0, K + 1, (H, W)).astype(np.int32)
    for k in rng.choice(np.arange(1, K + 1), 2, replace=False):
        m[m == k] = 0                                          # two labels without pixels
    classes = np.concatenate([rng.integers(1, 9, K), np.full(H * W, -1)]).astype(np.int32)[:max(K, H * W)]
    return m, classes, K


def test_filter_min_area_1_removes_exactly_the_empty_labels():
    rng = np.random.default_rng(11)
    for _ in range(40):
        m, classes, K = _random_case(rng)
        t = labels.instance_table(m, K)
        out, cls, sc, t2, k2, remap = labels.filter_instances(m, classes, K, t, 1)
        present = [k for k in range(1, K + 1) if (m == k).any()]
        assert k2 == len(present) and sc is None
        assert remap[0] == 0 and remap.shape == (K + 1,)
        # survivors keep their order and are numbered densely
        assert [int(remap[k]) for k in present] == list(range(1, k2 + 1))
        assert all(remap[k] == 0 for k in range(1, K + 1) if k not in present)
        for k in present:
            assert np.array_equal(out == remap[k], m == k)
        assert np.array_equal(out == 0, m == 0)
        assert cls[:k2].tolist() == [int(classes[k - 1]) for k in present]
        assert (cls[k2:] == -1).all() and cls.shape == (K,)
        assert t2.tolist() == [t[k - 1].tolist() for k in present]
        assert np.array_equal(t2, labels.instance_table(out, k2))


def test_filter_by_area_and_score_drops_pixels_to_background():
    m = np.array([[1, 1, 2, 0],
                  [1, 3, 3, 0],
                  [4, 4, 4, 4]], np.int32)
    classes = np.array([5, 6, 7, 8, -1, -1], np.int32)
    t = labels.instance_table(m, 4)
    out, cls, sc, t2, k2, remap = labels.filter_instances(m, classes, 4, t, 2)
    assert k2 == 3 and remap.tolist() == [0, 1, 0, 2, 3]
    assert out.tolist() == [[1, 1, 0, 0], [1, 2, 2, 0], [3, 3, 3, 3]]
    assert cls.tolist() == [5, 7, 8, -1]
    assert t2.tolist() == [[3, 0, 0, 1, 1], [2, 1, 1, 2, 1], [4, 0, 2, 3, 2]]
    scores = np.array([0.5, 9.0, 2.0, 1.0], np.float32)
    out, cls, sc, t2, k2, remap = labels.filter_instances(m, classes, 4, t, 2, scores, 1.0)
    assert k2 == 2 and remap.tolist() == [0, 0, 0, 1, 2]
    assert sc.dtype == np.float32 and sc.tolist() == [2.0, 1.0]
    assert cls.tolist() == [7, 8, -1, -1]
    assert out.tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [2, 2, 2, 2]]
    # scores without a threshold are carried along
    out, cls, sc, t2, k2, remap = labels.filter_instances(m, classes, 4, t, 1, scores)
    assert k2 == 4 and sc.tolist() == scores.tolist()
    # ... except a NaN score, which fails every comparison (as on the device)
    with_nan = np.array([0.5, np.nan, 2.0, 1.0], np.float32)
    out, cls, sc, t2, k2, remap = labels.filter_instances(m, classes, 4, t, 1, with_nan)
    assert k2 == 3 and remap.tolist() == [0, 1, 0, 2, 3] and sc.tolist() == [0.5, 2.0, 1.0]
    # a threshold beyond every area drops everything
    out, cls, sc, t2, k2, remap = labels.filter_instances(m, classes, 4, t, 13)
    assert k2 == 0 and not out.any() and (cls == -1).all() and t2.shape == (0, 5) and not remap.any()


def test_filtering_twice_changes_nothing():
    rng = np.random.default_rng(12)
    for _ in range(40):
        m, classes, K = _random_case(rng)
        t = labels.instance_table(m, K)
        min_area = int(rng.integers(1, 6))
        out, cls, _, t2, k2, _ = labels.filter_instances(m, classes, K, t, min_area)
        out2, cls2, _, t3, k3, remap2 = labels.filter_instances(out, cls, k2, t2, min_area)
        assert k3 == k2 and np.array_equal(out2, out) and np.array_equal(t3, t2)
        assert np.array_equal(cls2, cls[:k2])
        assert remap2.tolist() == list(range(k2 + 1))


def test_checker_areas_equal_the_native_rle_encoder_areas():
    """mn_rle_encode_host counts the pixels of every instance from the change points of the column-major scan:
    an independent route to the areas (needs no GPU)."""
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    rng = np.random.default_rng(13)
    for it in range(60):
        H, W = (int(x) for x in rng.integers(1, 16, 2))
        K = 6
        m = rng.integers(0, K + 1, (H, W)).astype(np.int32)
        if it % 3 == 0:
            m[m == 4] = 0
        flat = m.reshape(-1, order="F")
        prev = np.concatenate([[0], flat[:-1]])
        j = np.flatnonzero(flat != prev)
        n, cap = len(j), len(j) + 3
        pts = np.zeros((3, cap), np.int32)
        pts[0, :n], pts[1, :n], pts[2, :n] = j, prev[j], flat[j]
        offs = (ctypes.c_longlong * (K + 1))()
        areas = (ctypes.c_int * K)()
        out = ctypes.create_string_buffer(8 * n + 16 * K + 64)
        need = lib.mn_rle_encode_host(pts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), cap, n, H, W, K,
                                      ctypes.cast(out, ctypes.c_void_p), len(out), offs, areas)
        assert 0 < need <= len(out)
        assert labels.instance_table(m, K)[:, 0].tolist() == list(areas)


def test_library_exports_both_entry_points():
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    for name in ("mn_instance_table_device", "mn_filter_instances_device"):
        assert name in seg.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
    assert len(lib.mn_instance_table_device.argtypes) == 7
    assert len(lib.mn_filter_instances_device.argtypes) == 17
    assert not [n for n in seg.EXPORTS if "instance" in n and n not in (
        "mn_instance_scores_device", "mn_instance_table_device", "mn_filter_instances_device")]


def test_null_context_is_an_argument_error_without_a_device():
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.mn_instance_table_device(None, p, 2, 2, 3, p, None)
    assert rc == seg.MN_ERR_ARGUMENT and lib.mn_last_status() == seg.MN_ERR_ARGUMENT
    rc = lib.mn_filter_instances_device(None, p, 2, 2, 3, p, p, None, 1, 0.0, p, p, p, p, None, p, None)
    assert rc == seg.MN_ERR_ARGUMENT and lib.mn_last_status() == seg.MN_ERR_ARGUMENT


def test_header_declares_both_prototypes():
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("int mn_instance_table_device(mn_context* ctx, const int* d_mask, int height, int width, "
            "int num_instances, int* d_table, void* stream);") in flat
    assert ("int mn_filter_instances_device(mn_context* ctx, const int* d_mask, int height, int width, "
            "int num_instances, const int* d_table, const int* d_object_class, const float* d_scores, "
            "int min_area, float min_score, int* d_mask_out, int* d_remap, int* d_table_out, "
            "int* d_object_class_out, float* d_scores_out, int* d_new_count, void* stream);") in flat
    # the reference lines the two stand in for are cited next to them
    assert "segment.py:165-186" in flat and "egs/cityscape/local/evaluate.py:52-54" in flat


def test_binding_has_the_three_methods():
    import inspect
    from mergenet_amd import segmenter as seg
    p = inspect.signature(seg.Merger.filter_instances).parameters
    assert list(p)[:8] == ["self", "mask", "class_table", "num_instances", "min_area", "scores", "min_score", "inplace"]
    assert p["min_area"].default == 1 and p["scores"].default is None and p["min_score"].default is None
    assert p["inplace"].default is False and p["table"].default is None
    assert list(inspect.signature(seg.Merger.instance_table).parameters)[:3] == ["self", "mask", "num_instances"]
    p = inspect.signature(seg.Merger.coco_results).parameters
    assert list(p) == ["self", "mask", "class_table", "num_instances", "image_id", "cat_ids", "scores", "min_area"]
    assert p["scores"].default is None and p["min_area"].default == 1
