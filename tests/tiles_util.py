"""Shapes, inputs and bound shared by tests/test_tiles.py and tests/test_gpu_tiles.py."""
import numpy as np

from mergenet_amd import tiles as mt

# image H x W, tile th x tw, Cn -> C, logit scale, with flip, and the cover the bound is worked out for where that is
# less than the greatest cover of the shape (None: the greatest cover): the shapes of tests/test_gpu_tiles.py
CASES = {
    "a": (37, 53, 16, 24, 19, 9, 4.0, True, 4),
    "b": (40, 70, 16, 24, 19, 9, 12.0, True, None),
    "c": (24, 24, 24, 24, 5, 2, 4.0, True, None),
    "d": (50, 33, 16, 16, 7, 7, 30.0, True, None),
    "e": (37, 53, 16, 24, 19, 9, 4.0, False, 4),
    "f": (20, 200, 8, 70, 64, 3, 4.0, True, None),
    "g": (9, 300, 9, 130, 4, 2, 4.0, True, None),       # a row wider than one workgroup, an image one tile high
    "h": (12, 40, 8, 24, 21, 5, 4.0, True, None),       # 21 network classes: the kernel's form for 21..32
}


def make_case(name, seed=0):
    """(tiles, flip_tiles or None, row_starts, col_starts, H, W, C) of a case: float32 normal logits times the scale."""
    H, W, th, tw, Cn, C, scale, flip, _ = CASES[name]
    rows, cols = mt.tile_starts(H, th), mt.tile_starts(W, tw)
    rng = np.random.RandomState(1000 + seed + sum(ord(ch) for ch in name))
    shape = (len(rows) * len(cols), Cn, th, tw)
    tiles = (rng.standard_normal(shape) * scale).astype(np.float32)
    flips = (rng.standard_normal(shape) * scale).astype(np.float32) if flip else None
    return tiles, flips, rows, cols, H, W, C


def tolerance(name):
    """(Cn + cover_max + C + 8) * 2^-24.  Outputs lie in [0, 1]; a float32 evaluation errs by the softmax (Cn additions
    and a few ulp of expf and the division), the average, up to cover_max accumulations, two divisions and C
    additions, each at most 2^-24 of a value that is at most 1.  Shapes (a) and (e) were specified with the figure for
    a cover of 4, 40 * 2^-24 = 2.4e-6; their starts cover some pixels nine times, and the smaller figure is kept."""
    H, W, th, tw, Cn, C, _, _, stated_cover = CASES[name]
    cover = mt.tile_cover_count(mt.tile_starts(H, th), mt.tile_starts(W, tw), th, tw, H, W)
    cover_max = int(cover.max()) if stated_cover is None else min(int(cover.max()), stated_cover)
    return (Cn + cover_max + C + 8) * 2.0 ** -24


def torch_composition(tiles, flips, rows, cols, H, W, C):
    """The float32 composition a user writes in torch today, tile by tile: what tile_predict does, with the slice-add
    in place of its numpy one."""
    import torch
    import torch.nn.functional as F
    tiles = torch.from_numpy(tiles)
    flips = None if flips is None else torch.from_numpy(flips)
    T, Cn, th, tw = tiles.shape
    pred = torch.zeros((C, H, W), dtype=torch.float32)
    count = torch.zeros((H, W), dtype=torch.float32)
    t = 0
    for r in rows:
        for c in cols:
            p = F.softmax(tiles[t].float(), dim=0)
            if flips is not None:
                p = (p + F.softmax(flips[t].float(), dim=0).flip(-1)) / 2.0
            pred[0, r:r + th, c:c + tw] += p[:Cn - C + 1].max(dim=0)[0]
            pred[1:, r:r + th, c:c + tw] += p[Cn - C + 1:]
            count[r:r + th, c:c + tw] += 1.0
            t += 1
    score = pred / count[None]
    return (score / score.sum(0, keepdim=True)).numpy()
