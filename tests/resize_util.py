"""The per-element error bound of Merger.prepare against the float64 statement (mergenet_amd/resize.py), and a
float32 restatement of the kernel's own formula that the CPU suite holds to the same bound.

The bound (u = 2^-24, the unit roundoff of float32; eps32 = 2u).  With L the clamped piecewise-linear interpolant
of the source values, the statement is L at cv2's coordinates (cx, cy), the kernel L at its own (cx', cy'), plus
rounding:

 coordinate   The kernel forms the coordinate of destination d in float32: fl(src / dst) carries u relative, the
              product with d + 0.5 (exact) another u, the subtraction of 0.5 one more u of its result: at most
              3u * (d + 0.5) * scale.  cv2 forms it in double and casts to float32: u * |c|.  Together
                  delta = 4u * ((d + 0.5) * scale + 0.5),
              a few ulp of the coordinate's magnitude (about 5e-4 of a pixel at a width of 2048): far less than one
              pixel, so the two coordinates lie in the same segment of L or in adjacent ones, and L being continuous
                  |L(c') - L(c)| <= delta * max |v[j + 1] - v[j]| over the segments j = s0 - 1, s0, s0 + 1
              (those that exist; past a border L is constant).  This is the difference of the two blended
              neighbours, widened to the adjacent segments for the coordinate that straddles a pixel.  In two
              dimensions, by the triangle inequality through (cx, cy'):
                  delta_x * max of the horizontal differences over those three segments and the rows y0 - 1 .. y1 + 1
                + delta_y * max of the vertical differences, over those three segments, of the statement's
                            horizontally blended rows.
 blend        1 - f, two products and a sum, twice: at most 3u of the greatest blended magnitude M per stage, 6u and
              second-order terms in all: 4 * eps32 * M.
 sigmoid      mn_sigmoid(x) = 1.0f / (1.0f + expf(-x)): expf within 1 ulp (2u relative, and it enters s = 1 / (1 + e)
              with the factor e / (1 + e) < 1), the sum u, the correctly rounded division u: 4u = 2 * eps32 of s to
              first order; 3 * eps32 * M is taken.  It passes the blend with weights that sum to 1.
 tiny         2^-126 absolute: results below the normal range (sigmoid of a logit under -87: expf overflows and the
              kernel gives 0 where the statement gives 1e-38 or less).
 clip         a clamp moves two values no further apart: nothing added.
 16-bit out   half an ulp of the output type at the kernel's float32 value, taken at |reference| + the bound so far.
"""
import numpy as np

from mergenet_amd import resize

U = 2.0 ** -24
EPS32 = 2.0 ** -23
TINY = 2.0 ** -126


def half_ulp(dtype: str, a) -> np.ndarray:
    """Half an ulp of `dtype` ("float32" -> 0) at |a| (float64 array): the rounding to nearest of the store."""
    a = np.abs(np.asarray(a, np.float64))
    if dtype == "float32":
        return np.zeros_like(a)
    e = np.frexp(np.maximum(a, 2.0 ** -140))[1] - 1               # floor(log2 |a|)
    if dtype == "float16":
        return np.ldexp(1.0, np.maximum(e, -14) - 11)
    if dtype == "bfloat16":
        return np.ldexp(1.0, np.maximum(e, -126) - 8)
    raise ValueError(dtype)


def _axis(src: int, dst: int):
    s0, s1, _ = resize.linear_coords(src, dst)
    scale = 1.0 / (float(dst) / float(src))
    delta = 4.0 * U * ((np.arange(dst, dtype=np.float64) + 0.5) * scale + 0.5)
    return s0, s1, delta


def _segment_slope(a, s0):
    """a [..., n] -> [..., len(s0)]: the greatest |a[j + 1] - a[j]| over the existing segments j = s0 - 1, s0, s0 + 1."""
    n = a.shape[-1]
    if n == 1:
        return np.zeros(a.shape[:-1] + (len(s0),))
    d = np.abs(np.diff(a, axis=-1))
    out = np.zeros(a.shape[:-1] + (len(s0),))
    for o in (-1, 0, 1):
        out = np.maximum(out, d[..., np.clip(s0 + o, 0, n - 2)])
    return out


def prepare_bound(p, out_height: int, out_width: int, sigmoid: bool, out_dtype: str, ref) -> np.ndarray:
    """float64 [K, out_height, out_width]: the bound of the module docstring.  `p`: the values that are blended,
    float64 [K, H, W] (the statement's sigmoid already taken when `sigmoid`); `ref`: the statement's result."""
    p = np.asarray(p, np.float64)
    K, H, W = p.shape
    x0, x1, dx = _axis(W, out_width)
    y0, y1, dy = _axis(H, out_height)
    hx = _segment_slope(p, x0)                                     # [K, H, Wo]
    rows = [np.clip(y0 - 1, 0, H - 1), y0, y1, np.clip(y1 + 1, 0, H - 1)]
    hx = np.maximum.reduce([hx[:, r, :] for r in rows])            # [K, Ho, Wo]
    t = resize.blend_rows(p, out_width)                            # [K, H, Wo]
    vy = np.moveaxis(_segment_slope(np.moveaxis(t, 1, -1), y0), -1, 1)
    a = np.abs(p)
    m = np.maximum(a[..., x0], a[..., x1])
    m = np.maximum(m[:, y0, :], m[:, y1, :])
    bound = dx[None, None, :] * hx + dy[None, :, None] * vy + (4.0 + (3.0 if sigmoid else 0.0)) * EPS32 * m + TINY
    return bound + half_ulp(out_dtype, np.abs(np.asarray(ref, np.float64)) + bound)


def kernel_formula(x, out_height: int, out_width: int, sigmoid: bool, clip: bool) -> np.ndarray:
    """mn_prepare_maps' arithmetic restated in numpy float32 (the coordinate in float32 from fl(src / dst), blends in
    the kernel's order): what the bound must cover, without a GPU."""
    f32 = np.float32
    x = np.asarray(x, f32)

    def coords(src, dst):
        c = (np.arange(dst, dtype=f32) + f32(0.5)) * (f32(src) / f32(dst)) - f32(0.5)
        s = np.floor(c).astype(np.int64)
        f = (c - s.astype(f32)).astype(f32)
        f[s < 0] = 0
        s[s < 0] = 0
        f[s >= src - 1] = 0
        s[s >= src - 1] = src - 1
        return s, np.minimum(s + 1, src - 1), f

    with np.errstate(over="ignore"):
        p = (f32(1) / (f32(1) + np.exp(-x))).astype(f32) if sigmoid else x
    x0, x1, fx = coords(x.shape[2], out_width)
    y0, y1, fy = coords(x.shape[1], out_height)
    fy = fy[:, None]
    t = p[..., x0] * (f32(1) - fx) + p[..., x1] * fx
    v = t[:, y0, :] * (f32(1) - fy) + t[:, y1, :] * fy
    if clip:
        v = np.minimum(np.maximum(v, f32(EPS32)), f32(1) - f32(EPS32))
    assert v.dtype == f32
    return v
