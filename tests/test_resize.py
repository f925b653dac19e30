"""The numpy statements of the two resizes (mergenet_amd/resize.py) and of the sameness targets
(labels.sameness_targets), on the CPU: the properties any resize has, and the pinned indices at which cv2's
double-precision INTER_NEAREST index parts from the float32 one and from the rational floor.

cv2 is not installed here: the pinned values come from evaluating the formulas of OpenCV's published source, not from
a run of cv2 (see the module docstring of resize.py).
"""
import numpy as np
import pytest

from mergenet_amd import labels, resize


def float32_index(src, dst):
    """The index the kernel took before it followed cv2 (and torch's mode="nearest" takes): all in float32."""
    f32 = np.float32
    x = np.arange(dst, dtype=f32)
    return np.minimum(np.floor(x * (f32(src) / f32(dst))).astype(np.int64), src - 1)


def rational_index(src, dst):
    return np.minimum((np.arange(dst, dtype=np.int64) * src) // dst, src - 1)


@pytest.mark.parametrize("n", [1, 2, 5, 37, 1000])
def test_identity_when_the_sizes_are_equal(n):
    assert np.array_equal(resize.nearest_index(n, n), np.arange(n))
    s0, s1, f = resize.linear_coords(n, n)
    assert np.array_equal(s0, np.arange(n)) and np.array_equal(s1, np.minimum(np.arange(n) + 1, n - 1))
    assert not f.any()
    x = np.random.default_rng(n).random((2, 3, n))
    assert np.array_equal(resize.prepare_maps(x, 3, n, clip=False), x)
    m = np.arange(3 * n).reshape(3, n)
    assert np.array_equal(resize.upsample_mask(m, 3, n), m)


@pytest.mark.parametrize("n", [1, 4, 33, 512])
def test_exact_factor_two_in_both_directions(n):
    assert np.array_equal(resize.nearest_index(n, 2 * n), np.arange(2 * n) // 2)
    assert np.array_equal(resize.nearest_index(2 * n, n), 2 * np.arange(n))
    # growing: coordinate x / 2 - 1/4 -> weights 3/4 and 1/4 in turn, clamped at both ends
    s0, s1, f = resize.linear_coords(n, 2 * n)
    x = np.arange(2 * n)
    want0 = np.clip((x - 1) // 2, 0, n - 1)
    wantf = np.where(x % 2 == 1, 0.25, 0.75)
    wantf[(x == 0) | (want0 >= n - 1)] = 0.0
    assert np.array_equal(s0, want0) and np.array_equal(s1, np.minimum(want0 + 1, n - 1)) and np.array_equal(f, wantf)
    # shrinking: coordinate 2 x + 1/2 -> the mean of the pair
    s0, s1, f = resize.linear_coords(2 * n, n)
    assert np.array_equal(s0, 2 * np.arange(n)) and np.array_equal(s1, s0 + 1) and np.array_equal(f, np.full(n, 0.5))
    img = np.random.default_rng(n).random((1, 2, 2 * n))
    got = resize.prepare_maps(img, 1, n, clip=False)
    assert np.allclose(got[0, 0], img[0].reshape(2, n, 2).mean(axis=(0, 2)), rtol=0, atol=1e-15)


def test_one_pixel_sources_and_destinations():
    assert np.array_equal(resize.nearest_index(1, 7), np.zeros(7, np.int64))
    assert np.array_equal(resize.nearest_index(7, 1), [0])
    s0, s1, f = resize.linear_coords(1, 7)
    assert not s0.any() and not s1.any() and not f.any()
    s0, s1, f = resize.linear_coords(7, 1)              # coordinate 0.5 * 7 - 0.5 = 3
    assert (s0.tolist(), s1.tolist(), f.tolist()) == ([3], [4], [0.0])
    s0, s1, f = resize.linear_coords(8, 1)              # 3.5: the mean of the two middle pixels
    assert (s0.tolist(), s1.tolist(), f.tolist()) == ([3], [4], [0.5])
    x = np.random.default_rng(0).random((2, 1, 1))
    assert np.array_equal(resize.prepare_maps(x, 4, 5, clip=False), np.broadcast_to(x, (2, 4, 5)))
    with pytest.raises(ValueError):
        resize.nearest_index(0, 4)
    with pytest.raises(ValueError):
        resize.linear_coords(4, 0)


# (src, dst, positions, float32 index there, cv2 index there)
PINNED = [(8, 82, [41], [3], [4]), (8, 98, [49], [4], [3]), (8, 196, [49, 98, 147], [2, 4, 6], [1, 3, 5])]


@pytest.mark.parametrize("src,dst,pos,f32_values,cv2_values", PINNED)
def test_pinned_indices_where_double_and_float32_part(src, dst, pos, f32_values, cv2_values):
    got = resize.nearest_index(src, dst)
    old = float32_index(src, dst)
    assert got[pos].tolist() == cv2_values and old[pos].tolist() == f32_values
    assert np.flatnonzero(got != old).tolist() == pos           # ... and nowhere else
    assert got.min() == 0 and got.max() == src - 1 and (np.diff(got) >= 0).all()


def test_cv2_index_is_not_the_rational_floor_in_general():
    """On 25 -> 50, 40 -> 37 and 37 -> 53 cv2's index is the integer floor (x * src) // dst at every x.  The two
    need not agree: ``1. / (dst / src)`` is rounded twice, and where x * src / dst is an integer the product can fall
    just below it -- 8 -> 98 at x = 49 takes 3, the quotient being exactly 4 (and the same at 98 and 147 of
    8 -> 196).  cv2's value is the one to match: the reference's masks carry it."""
    for src, dst in [(25, 50), (40, 37), (37, 53)]:
        assert np.array_equal(resize.nearest_index(src, dst), rational_index(src, dst))
    assert np.flatnonzero(resize.nearest_index(8, 98) != rational_index(8, 98)).tolist() == [49]
    assert np.flatnonzero(resize.nearest_index(8, 196) != rational_index(8, 196)).tolist() == [49, 98, 147]


def test_where_the_float32_index_agrees_and_where_it_does_not():
    """The size pairs of test_gpu_prepare.py::test_upsample_mask_matches_torch_nearest and of test_gpu_e2e.py are
    ones where float32 and double give the same index everywhere, which is why torch can be their reference; the
    pairs test_gpu_edges.py adds are ones where they do not."""
    for src, dst in [(32, 64), (48, 96), (25, 50), (35, 70), (40, 37), (56, 129), (512, 1024), (1024, 2048)]:
        assert np.array_equal(resize.nearest_index(src, dst), float32_index(src, dst)), (src, dst)
    for src, dst in [(8, 82), (8, 98), (8, 196), (24, 34), (24, 260), (33, 27), (39, 15), (1000, 1040)]:
        assert (resize.nearest_index(src, dst) != float32_index(src, dst)).any(), (src, dst)
    assert int((resize.nearest_index(1000, 1040) != float32_index(1000, 1040)).sum()) == 30


def test_upsample_mask_picks_rows_and_columns_independently():
    m = np.arange(8 * 24).reshape(8, 24)
    got = resize.upsample_mask(m, 82, 34)
    iy, ix = resize.nearest_index(8, 82), resize.nearest_index(24, 34)
    assert got.shape == (82, 34)
    for y in (0, 41, 81):
        for x in (0, 17, 33):
            assert got[y, x] == m[iy[y], ix[x]]


def test_prepare_maps_blend_sigmoid_clip_and_nan():
    eps = float(np.finfo(np.float32).eps)
    # a constant stays the constant, a horizontal ramp stays linear between the clamped borders
    c = np.full((1, 5, 7), 0.375)
    assert np.array_equal(resize.prepare_maps(c, 9, 13, clip=False), np.full((1, 9, 13), 0.375))
    ramp = np.broadcast_to(np.arange(9.0), (1, 4, 9)) / 16
    got = resize.prepare_maps(ramp, 4, 18, clip=False)[0, 0]
    s0, s1, f = resize.linear_coords(9, 18)
    assert np.allclose(got, (s0 * (1 - f) + s1 * f) / 16, rtol=0, atol=1e-15)
    # sigmoid in float64, saturating without overflow; the clip comes last
    z = np.array([[[-np.inf, -100.0, -30.0, 0.0, 30.0, 100.0, np.inf]]])
    p = resize.prepare_maps(z, 1, 7, apply_sigmoid=True, clip=False)[0, 0]
    assert p[0] == 0.0 and 0 < p[1] < 1e-43 and p[3] == 0.5 and p[5] == 1.0 and p[6] == 1.0
    q = resize.prepare_maps(z, 1, 7, apply_sigmoid=True, clip=True)[0, 0]
    assert q.tolist() == [eps, eps, eps, 0.5, 1 - eps, 1 - eps, 1 - eps]
    # a NaN spreads to every output that blends it, weight 0 included, and through the clip
    n = np.zeros((1, 3, 3))
    n[0, 1, 1] = np.nan
    out = resize.prepare_maps(n, 3, 3, apply_sigmoid=True, clip=True)
    want = np.zeros((3, 3), bool)
    want[0:2, 0:2] = True                  # (s0, s1) = (0,1), (1,2), (2,2): outputs 0 and 1 of each axis read index 1
    assert np.array_equal(np.isnan(out[0]), want)
    with pytest.raises(ValueError):
        resize.prepare_maps(np.zeros((3, 3)), 3, 3)


def test_sameness_targets_statement_equals_the_pixel_definition():
    """target[k][r][c] = (mask[r + di][c + dj] == mask[r][c]), 1 where the neighbour is outside the image: the loop
    form of the np.roll definition (utils/dataset.py:259-277), negative labels compared as plain integers."""
    rng = np.random.default_rng(11)
    for H, W in [(1, 1), (1, 9), (7, 1), (6, 8)]:
        mask = rng.integers(-1, 3, (H, W)).astype(np.int32)
        offs = [(0, 0), (1, 0), (0, -1), (-2, 3), (H, 0), (0, -W), (-H - 3, W + 2), (5, -5)]
        got = labels.sameness_targets(mask, offs)
        assert got.dtype == np.float32 and got.shape == (len(offs), H, W)
        for k, (di, dj) in enumerate(offs):
            for r in range(H):
                for c in range(W):
                    rr, cc = r + di, c + dj
                    inside = 0 <= rr < H and 0 <= cc < W
                    assert got[k, r, c] == (float(mask[rr, cc] == mask[r, c]) if inside else 1.0)
        assert got[0].all() and got[4].all() and got[5].all() and got[6].all()


PREPARE_SHAPES = [((2, 5, 2048), (7, 1333)), ((2, 6, 667), (9, 1333)), ((1, 8, 2047), (3, 1000)), ((3, 1, 9), (4, 9)),
                  ((3, 9, 1), (9, 5)), ((1, 17, 9), (1, 1)), ((2, 33, 47), (64, 257))]


@pytest.mark.parametrize("shape", PREPARE_SHAPES)
@pytest.mark.parametrize("sigmoid", [False, True])
def test_float32_form_of_the_bilinear_kernel_stays_within_the_derived_bound(shape, sigmoid):
    """resize_util.kernel_formula (mn_prepare_maps' arithmetic in numpy float32) against the float64 statement,
    under the bound test_gpu_edges.py holds the kernel to: the derivation covers the formula before any GPU is
    asked.  At 2048 -> 1333 the error reaches 1e-4 (float32 coordinates of magnitude 2048 on a map of slope ~1),
    fifty times the fixed 2e-6 that holds up to a width of 129 -- and about half of its bound."""
    import resize_util as ru
    (K, H, W), (Ho, Wo) = shape
    rng = np.random.default_rng(H * W + Wo)
    x = (rng.standard_normal((K, H, W)) * 3 if sigmoid else rng.random((K, H, W))).astype(np.float32)
    p = resize.sigmoid(x) if sigmoid else x.astype(np.float64)
    for clip in (False, True):
        ref = resize.prepare_maps(x, Ho, Wo, sigmoid, clip)
        bound = ru.prepare_bound(p, Ho, Wo, sigmoid, "float32", ref)
        got = ru.kernel_formula(x, Ho, Wo, sigmoid, clip).astype(np.float64)
        assert got.shape == ref.shape == bound.shape
        assert (np.abs(got - ref) <= bound).all()
        assert bound.max() <= 4 * 2.0 ** -24 * (max(H, W) + 1) * 2 + 8 * 2.0 ** -23   # (values in [0, 1]: slopes <= 1)


def test_half_ulp_of_the_16_bit_outputs():
    import resize_util as ru
    a = np.array([0.0, 2.0 ** -24, 2.0 ** -14, 0.75, 1.0])
    assert ru.half_ulp("float32", a).tolist() == [0, 0, 0, 0, 0]
    assert ru.half_ulp("float16", a).tolist() == [2.0 ** -25, 2.0 ** -25, 2.0 ** -25, 2.0 ** -12, 2.0 ** -11]
    assert ru.half_ulp("bfloat16", a).tolist() == [2.0 ** -134, 2.0 ** -32, 2.0 ** -22, 2.0 ** -9, 2.0 ** -8]
