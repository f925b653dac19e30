"""The numpy statements of the two resizes of the path, the checkers of ``Merger.upsample_mask`` and ``Merger.prepare``.

The reference resizes with OpenCV: the instance mask back to the image size with ``cv2.resize(mask, ...,
interpolation=cv2.INTER_NEAREST)`` (egs/cityscape/local/segment.py:146-149) and the network's maps to the segmentation
size with ``cv2.resize`` / INTER_LINEAR (segment.py:110-123).  cv2 is not installed where this project is built and
tested, so NOTHING below was compared with a run of cv2: the formulas are taken from OpenCV's published source
(modules/imgproc/src/resize.cpp: the portable ``resizeNN`` and, for INTER_LINEAR on float images, the coordinate
tables of ``resize`` feeding ``HResizeLinear`` / ``VResizeLinear``) and restated in float64.
"""

from __future__ import annotations

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def _inverse_scale(src: int, dst: int) -> float:
    """cv2's scale of one axis: ``fx = (double)dst / src`` and then ``1. / fx`` -- two roundings in double, which is
    not always ``src / dst`` rounded once."""
    if src <= 0 or dst <= 0:
        raise ValueError("sizes must be positive")
    fx = float(dst) / float(src)
    return 1.0 / fx


def nearest_index(src: int, dst: int) -> np.ndarray:
    """int64 [dst]: the source index INTER_NEAREST takes for every destination index of one axis, as resizeNN
    computes it, ``min(cvFloor(x * ifx), src - 1)`` with ``ifx = 1. / ((double)dst / src)``, all in double.

    Not the float32 index ``floorf(x * ((float)src / dst))`` (what torch's ``mode="nearest"`` computes): 8 -> 82
    gives 4 at x = 41 where float32 gives 3.  Not the rational floor ``(x * src) // dst`` either: 8 -> 98 gives 3 at
    x = 49, where the quotient is exactly 4 -- cv2's own rounding, which is what the reference's masks carry."""
    ifx = _inverse_scale(src, dst)
    x = np.arange(int(dst), dtype=np.float64)
    return np.minimum(np.floor(x * ifx).astype(np.int64), int(src) - 1)


def upsample_mask(mask, out_height: int, out_width: int) -> np.ndarray:
    """``cv2.resize(mask, (out_width, out_height), interpolation=cv2.INTER_NEAREST)`` of a 2-D array (growing or
    shrinking): rows and columns picked by :func:`nearest_index`."""
    m = np.asarray(mask)
    iy = nearest_index(m.shape[0], out_height)
    ix = nearest_index(m.shape[1], out_width)
    return m[iy][:, ix]


def linear_coords(src: int, dst: int):
    """(s0 int64 [dst], s1 int64 [dst], f float64 [dst]): the two source indices INTER_LINEAR blends for every
    destination index of one axis of a float image, and the weight of the second.

    The coordinate is ``(float)((x + 0.5) * scale - 0.5)`` with ``scale = 1. / ((double)dst / src)`` in double, the
    cast to float32 being cv2's; ``s0 = floor`` of it and ``f`` the rest (exact in float32).  At the borders both
    indices are the border pixel and the weight is 0: ``s0 < 0 -> s0 = 0, f = 0``; ``s0 >= src - 1 -> s0 = src - 1,
    f = 0``; ``s1 = min(s0 + 1, src - 1)``."""
    scale = _inverse_scale(src, dst)
    x = np.arange(int(dst), dtype=np.float64)
    c = ((x + 0.5) * scale - 0.5).astype(np.float32)
    s0 = np.floor(c).astype(np.int64)
    f = (c - s0.astype(np.float32)).astype(np.float64)
    low = s0 < 0
    s0[low] = 0
    f[low] = 0.0
    high = s0 >= int(src) - 1
    s0[high] = int(src) - 1
    f[high] = 0.0
    return s0, np.minimum(s0 + 1, int(src) - 1), f


def sigmoid(x) -> np.ndarray:
    """1 / (1 + exp(-x)) in float64 without overflow: 0 and 1 at -inf and +inf, NaN stays NaN."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def blend_rows(p, out_width: int) -> np.ndarray:
    """The horizontal half of :func:`prepare_maps`: float64 [..., W] -> [..., out_width]."""
    p = np.asarray(p, np.float64)
    x0, x1, fx = linear_coords(p.shape[-1], out_width)
    return p[..., x0] * (1.0 - fx) + p[..., x1] * fx


def prepare_maps(x, out_height: int, out_width: int, apply_sigmoid: bool = False, clip: bool = True) -> np.ndarray:
    """The statement of ``Merger.prepare``: float64 [K, out_height, out_width] from [K, H, W] maps -- the sigmoid of
    the elements (``apply_sigmoid``), cv2's INTER_LINEAR blend with the coordinates of :func:`linear_coords`,
    horizontal then vertical, in float64, and the merger's clip to ``[eps32, 1 - eps32]`` (``clip``).  A NaN element
    makes every output NaN that blends it, weight 0 included; the clip keeps NaN (the kernel's ``fminf`` / ``fmaxf``
    do not: with ``clip`` a NaN is undefined)."""
    p = np.asarray(x, np.float64)
    if p.ndim != 3:
        raise ValueError("maps are [K, H, W]")
    if apply_sigmoid:
        p = sigmoid(p)
    t = blend_rows(p, out_width)
    y0, y1, fy = linear_coords(p.shape[1], out_height)
    fy = fy[:, None]
    with np.errstate(invalid="ignore"):
        v = t[:, y0, :] * (1.0 - fy) + t[:, y1, :] * fy
    if clip:
        v = np.clip(v, EPS32, 1.0 - EPS32)
    return v
