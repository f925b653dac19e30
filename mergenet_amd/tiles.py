"""Class maps from a tiled semantic network: the geometry and the numpy statement of ``Merger.tile_class_maps``.

The production recipe's class maps come from a Cn-class semantic network run on overlapping tiles, plain and
horizontally flipped (``tile_predict``, models/pspnet_caffe.py:492-560 of the reference).  The
library assembles the image's C class planes from the tiles' logits in one kernel (``mn_tile_class_maps_device``);
this module holds what needs no GPU: where the tiles lie, and what the kernel computes, in float64."""
import numpy as np


def tile_starts(size: int, side: int):
    """Where the tiles of side ``side`` start along an axis of ``size`` pixels: the reference's geometry
    (pspnet_caffe.py:504-515).  n + 1 tiles with n = size // side + 1, a stride of (size - side) / n, every start
    truncated to an integer; an axis of exactly one tile gives [0, 0, 0]."""
    size, side = int(size), int(side)
    if side <= 0 or size < side:
        raise ValueError("tile side %d does not fit an axis of %d pixels" % (side, size))
    n = int(size / float(side)) + 1
    stride = (size - side) / float(n)
    return [int(i * stride) for i in range(n + 1)]


def tile_cover_count(row_starts, col_starts, tile_height: int, tile_width: int, height: int, width: int):
    """int64 [H, W]: how many tiles cover each pixel (the reference's ``count`` plane)."""
    rows = np.zeros(height, np.int64)
    cols = np.zeros(width, np.int64)
    for r in row_starts:
        rows[r:r + tile_height] += 1
    for c in col_starts:
        cols[c:c + tile_width] += 1
    return rows[:, None] * cols[None, :]


def _softmax64(x):
    x = x - x.max(axis=0, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=0, keepdims=True)


def tile_class_maps_reference(tiles, flip_tiles, row_starts, col_starts, height: int, width: int, num_classes: int):
    """float64 [C, H, W]: the class planes of an image from the logits of its tiles.

    ``tiles`` [T, Cn, th, tw]: the logits of tile t = i * len(col_starts) + j, whose top-left pixel is
    (row_starts[i], col_starts[j]); ``flip_tiles``: the same shape or None, the logits on the horizontally flipped
    slice as the network gave them.  Per tile: softmax over the Cn classes, the flipped pass flipped back and the two
    averaged, plane 0 = the maximum over the first Cn - C + 1 ("stuff") classes, planes 1..C-1 = the remaining
    classes.  Per image: the tiles summed in ascending t, divided by the cover count, renormalised over the C planes.
    No clip."""
    tiles = np.asarray(tiles, np.float64)
    T, Cn, th, tw = tiles.shape
    C = int(num_classes)
    if not 1 <= C <= Cn:
        raise ValueError("num_classes must lie in 1..%d" % Cn)
    if T != len(row_starts) * len(col_starts):
        raise ValueError("%d tiles for %d x %d starts" % (T, len(row_starts), len(col_starts)))
    if flip_tiles is not None:
        flip_tiles = np.asarray(flip_tiles, np.float64)
        if flip_tiles.shape != tiles.shape:
            raise ValueError("flip_tiles must have the shape of tiles")
    nstuff = Cn - C + 1
    acc = np.zeros((C, height, width), np.float64)
    t = 0
    for r in row_starts:
        for c in col_starts:
            if r < 0 or c < 0 or r + th > height or c + tw > width:
                raise ValueError("tile %d leaves the image" % t)
            p = _softmax64(tiles[t])
            if flip_tiles is not None:
                p = (p + _softmax64(flip_tiles[t])[:, :, ::-1]) * 0.5
            acc[0, r:r + th, c:c + tw] += p[:nstuff].max(axis=0)
            acc[1:, r:r + th, c:c + tw] += p[nstuff:]
            t += 1
    count = tile_cover_count(row_starts, col_starts, th, tw, height, width)
    if (count == 0).any():
        raise ValueError("a pixel is covered by no tile")
    s = acc / count[None].astype(np.float64)
    return s / s.sum(axis=0, keepdims=True)
