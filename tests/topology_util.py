"""Winding label maps and a union-find reference for the component labelling (test_topology.py, test_gpu_topology.py).

On maps built by ``lean_util.maps_from_labels`` (sameness 0.95 inside a label, 0.05 across, class maps peaked on the
label's class) and with the options (same_different_bias, object_merge_factor, merge_logprob_bias) = (0, 1, 0) every
record between two components scores below 0, so nothing merges after the first phase: the final partition is the
connected components of the graph "p ~ p + o_k iff both pixels are inside the image and carry one label".
``components`` states that and nothing else.  It knows nothing of the project's oracle; test_topology.py holds the two
against each other.

Every generator returns an int32 [H, W] label map (0 = background) and is described by what makes it hard for a tiled
union-find (tiles of 16 rows x 64 columns: borders between rows 15 | 16, 31 | 32 and columns 63 | 64, 127 | 128), not
by how it is drawn.  ``CASES`` is the table of (label map, offset list) pairs both test files run.
"""
import functools

import numpy as np

from mergenet_amd import synth


# ---- the reference ---------------------------------------------------------------------------------------------------

def components(lab, offs):
    """int32 [H, W]: every pixel carries the lowest pixel id (r * W + c) of its component in the graph whose edges are
    the pairs (p, p + o), o in `offs`, with both ends inside the image and lab[p] == lab[p + o].  Plain union-find:
    the larger root goes under the smaller, so a root is the lowest id of its set."""
    H, W = lab.shape
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for r in range(H):
        for c in range(W):
            for (di, dj) in offs:
                rr, cc = r + di, c + dj
                if 0 <= rr < H and 0 <= cc < W and lab[r, c] == lab[rr, cc]:
                    a, b = find(r * W + c), find(rr * W + cc)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    return np.array([find(p) for p in range(H * W)], np.int32).reshape(H, W)


def records_between(comp, offs):
    """Number of distinct unordered pairs of components with at least one edge (p, p + o) between them: the records
    the second phase starts from."""
    H, W = comp.shape
    pairs = set()
    for (di, dj) in offs:
        r0, r1, c0, c1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
        if r0 >= r1 or c0 >= c1:
            continue
        a = comp[r0:r1, c0:c1].reshape(-1).astype(np.int64)
        b = comp[r0 + di:r1 + di, c0 + dj:c1 + dj].reshape(-1).astype(np.int64)
        d = a != b
        lo, hi = np.minimum(a[d], b[d]), np.maximum(a[d], b[d])
        pairs.update((lo * (H * W) + hi).tolist())
    return len(pairs)


def count(comp, where=None):
    """Number of components (of the pixels selected by the boolean map `where`)."""
    return int(np.unique(comp if where is None else comp[where]).size)


def reference_mask(comp, lab, class_of_label):
    """(mask int32 [H, W], class list): the labelling collapsed as the library's mask is -- every component of class 0
    is 0, the others are 1..K in ascending root -- with the class of label k at index k - 1."""
    mask = np.zeros(comp.shape, np.int32)
    classes = []
    for root in np.unique(comp):
        cls = class_of_label[int(lab.reshape(-1)[root])]
        if cls != 0:
            classes.append(cls)
            mask[comp == root] = len(classes)
    return mask, classes


# ---- generators ------------------------------------------------------------------------------------------------------

def serpentine(H, W, arm, gap, shift=0, vertical=False):
    """ONE foreground label that runs the full width in a band `arm` rows high, turns in the last (first) `arm`
    columns and runs back, `gap` rows further down, and so on.  With the unit offsets its graph diameter is about
    H * W / (arm + gap); every arm crosses every vertical tile border, every turn joins two arms that are far apart in
    pixel order, and a pixel's root (the top-left pixel) lies in the first tile.  The gaps are background components
    of their own, closed at alternating ends.  The first arm starts at row `shift` (modulo the period): arm = 1,
    gap = 1 puts arms on the even rows -- row 16, the first of a tile, with its turn in row 15, the last of the tile
    above; arm = gap = 2, shift = 3 makes rows 15 and 16 one arm.  `vertical`: the transpose (arms are columns, the
    turns in the first and last rows; shift = 3 with arm = gap = 2 makes columns 63 and 64 one arm)."""
    if vertical:
        return np.ascontiguousarray(serpentine(W, H, arm, gap, shift).T)
    lab = np.zeros((H, W), np.int32)
    period = arm + gap
    for r in range(H):
        k, phase = divmod(r - shift % period + 2 * period, period)
        if phase < arm:
            lab[r, :] = 1
        elif k % 2 == 0:
            lab[r, max(0, W - arm):] = 1
        else:
            lab[r, :arm] = 1
    return lab


def spiral(H, W):
    """Two interleaved one-pixel corridors, foreground and background, winding clockwise from the image's border to
    its centre (an even height leaves the background's innermost stretch two wide): each is ONE component with the
    unit offsets, a path about H * W / 2 long.  A pixel's root (pixel 0
    for the foreground) lies many tiles away, and the only path to it leaves the pixel's tile and re-enters it once
    per turn of the spiral -- inside a tile the corridor is dozens of separate pieces."""
    lab = np.zeros((H, W), np.int32)
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    r = c = d = 0
    lab[0, 0] = 1
    blocked = 0
    while blocked < 2:
        dr, dc = steps[d]
        r1, c1 = r + dr, c + dc
        free = 0 <= r1 < H and 0 <= c1 < W and lab[r1, c1] == 0
        # the next pixel may touch the corridor only where it comes from: one background pixel stays between laps
        touching = sum(int(lab[r1 + a, c1 + b]) for (a, b) in steps if 0 <= r1 + a < H and 0 <= c1 + b < W) if free else 0
        if free and touching == 1:
            r, c = r1, c1
            lab[r, c] = 1
            blocked = 0
        else:
            d = (d + 1) % 4
            blocked += 1
    return lab


def comb(H, W, up, teeth=1):
    """Teeth `teeth` columns wide with as wide a gap between them, joined by a spine `teeth` rows high in the LAST
    rows (`up` false) or the FIRST rows (`up` true).  With one-pixel teeth a tile row holds 32 runs, which are one
    component only through a row outside the tile: the tile stage sees 32 components per tile, the border stage has
    to join them all.  With the spine below, the root (pixel 0, the top of the first tooth) is at the far end of the
    last union; with the spine above it is on the spine."""
    lab = np.zeros((H, W), np.int32)
    for c in range(W):
        if (c // teeth) % 2 == 0:
            lab[:, c] = 1
    if up:
        lab[:teeth, :] = 1
    else:
        lab[H - teeth:, :] = 1
    return lab


def stairs(H, W, anti=False):
    """A one-pixel staircase through the corner where four tiles meet (rows 15 | 16, columns 63 | 64), from the
    image's first row to its last.  Right, down, right, down ...: (15, 63) -> (15, 64) -> (16, 64).  `anti`: up, right,
    up, right ...: (16, 63) -> (15, 63) -> (15, 64).  Every piece inside a tile row is two pixels, and at the corner the
    staircase is connected -- with the unit offsets -- through one edge across the vertical border followed at once
    by one across the horizontal border: only through border edges, and through both waves of the border stage."""
    assert H > 16 and W > 65
    lab = np.zeros((H, W), np.int32)
    for r in range(H):
        cols = (78 - r, 79 - r) if anti else (r + 48, r + 49)
        for c in cols:
            if 0 <= c < W:
                lab[r, c] = 1
    return lab


def chain(H, W, k, step, down, blob=(3, 3)):
    """`k` blobs of one label, blob i + 1 = blob i moved by `step` = (a, b) (`down`) or by (-a, b) (not `down`), far
    enough apart that only that one long offset joins a blob to the next.  The blobs' roots then arrive at the hook
    in ascending (`down`) or descending pixel order and it builds a chain of roots instead of a star: a pixel of the
    last blob can be as many steps from the final root as there are blobs.  The chain crosses tile borders in both
    directions."""
    a, b = step
    bh, bw = blob
    assert bh <= a and bw < b and (k - 1) * a + bh <= H and (k - 1) * b + bw <= W
    lab = np.zeros((H, W), np.int32)
    c0 = (W - ((k - 1) * b + bw)) // 2
    r0 = (H - ((k - 1) * a + bh)) // 2
    for i in range(k):
        r = r0 + i * a if down else r0 + (k - 1 - i) * a
        lab[r:r + bh, c0 + i * b:c0 + i * b + bw] = 1
    return lab


def percolation(H, W, p, seed):
    """Site percolation: label 1 with probability `p`, else 0.  At p = 0.6, near the threshold of the square lattice,
    both labels fall into ragged clusters of every size: hundreds of components per tile, unions that arrive in no
    order at all, and many lost races for the same root."""
    return (np.random.default_rng(seed).random((H, W)) < p).astype(np.int32)


def random_labels(H, W, n, seed):
    """Every pixel one of `n` labels, independently: tiny components that only lists with diagonal offsets join into
    anything larger."""
    return np.random.default_rng(seed).integers(0, n, (H, W)).astype(np.int32)


# ---- the table of cases ----------------------------------------------------------------------------------------------

CLASS_OF_LABEL = {0: 0, 1: 3, 2: 5}     # label 0 is background; 9 classes
C = 9

UNIT = [(0, 1), (1, 0)]
UNIT_UP = [(0, 1), (-1, 0)]             # the vertical unit offset points up: dv = -1 in the tile and border stages
NO_UNIT = [(0, 2), (2, 0), (1, 1), (1, -1)]    # no unit offset: every union is the hook's
REAL = [tuple(int(x) for x in o) for o in synth.generate_offsets(12, 6)]   # the realistic list: (1, 0), (0, 1), long ones


class Case:
    def __init__(self, name, make, offs):
        self.name, self.make, self.offs = name, make, [tuple(o) for o in offs]

    @functools.cached_property
    def lab(self):
        lab = self.make()
        lab.setflags(write=False)
        return lab

    @functools.cached_property
    def comp(self):
        comp = components(self.lab, self.offs)
        comp.setflags(write=False)
        return comp

    @functools.cached_property
    def records(self):
        return records_between(self.comp, self.offs)

    def __repr__(self):
        return self.name


def _cases():
    out = []

    def add(name, make, lists):
        for tag, offs in lists:
            out.append(Case("%s-%s" % (name, tag), make, offs))

    both = [("unit", UNIT), ("up", UNIT_UP)]
    for (H, W) in [(35, 130), (32, 128), (17, 65), (16, 64)]:
        add("serpentine-1-1-%dx%d" % (H, W), lambda H=H, W=W: serpentine(H, W, 1, 1), both)
    for (H, W) in [(35, 130), (34, 66), (32, 128)]:      # mn_cc_hook<1>, <1> with straddling lanes in the sweep, <4>
        add("serpentine-2-2-%dx%d" % (H, W), lambda H=H, W=W: serpentine(H, W, 2, 2), [("nounit", NO_UNIT)])
    add("serpentine-2-2-rows15+16-35x130", lambda: serpentine(35, 130, 2, 2, shift=3), both)
    add("serpentine-vertical-33x131", lambda: serpentine(33, 131, 1, 1, vertical=True),
        [("swapped", [(1, 0), (0, 1)]), ("v+0,3", [(1, 0), (0, 3)])])
    add("serpentine-vertical-cols63+64-33x131", lambda: serpentine(33, 131, 2, 2, shift=3, vertical=True), both)
    for (H, W) in [(35, 131), (48, 64)]:
        add("spiral-%dx%d" % (H, W), lambda H=H, W=W: spiral(H, W), both)
    for up in (False, True):
        add("comb-%s-33x130" % ("up" if up else "down"), lambda up=up: comb(33, 130, up),
            both + [("unit+long", UNIT + [(0, 9), (5, -3)])])
    add("comb-down-32x132", lambda: comb(32, 132, False), [("unit", UNIT)])          # N % 4 == 0: the lean form
    for anti in (False, True):
        add("stairs-%s33x130" % ("anti-" if anti else ""), lambda anti=anti: stairs(33, 130, anti), both)
    add("chain-down-40x136", lambda: chain(40, 136, 12, (3, 6), True), [("unit+3,6", UNIT + [(3, 6)]),
                                                                        ("nounit", [(3, 6), (0, 2), (2, 0)])])
    add("chain-up-40x136", lambda: chain(40, 136, 12, (3, 6), False), [("unit-3,6", UNIT + [(-3, 6)])])
    for (H, W) in [(48, 130), (35, 67)]:
        add("percolation-%dx%d" % (H, W), lambda H=H, W=W: percolation(H, W, 0.6, 7), both)
    add("random3-35x131", lambda: random_labels(35, 131, 3, 11), [("diag", UNIT + [(1, 1), (2, -1)])])
    add("serpentine-1-1-35x130", lambda: serpentine(35, 130, 1, 1), [("real", REAL)])
    add("spiral-35x131", lambda: spiral(35, 131), [("real", REAL)])
    add("percolation-48x130", lambda: percolation(48, 130, 0.6, 7), [("real", REAL)])
    # narrow images, and the last column on either side of a tile's last lane
    add("serpentine-1-1-40x3", lambda: serpentine(40, 3, 1, 1), both)
    add("serpentine-1-1-3x130", lambda: serpentine(3, 130, 1, 1), both)
    for W in (63, 65):
        add("serpentine-1-1-18x%d" % W, lambda W=W: serpentine(18, W, 1, 1), both)
        add("comb-down-18x%d" % W, lambda W=W: comb(18, W, False), both)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Cores: arms three pixels wide, so the clean pixels (core_radius = 1) are the centre lines and wind as the arms do.
CORE_CASES = [
    Case("core-serpentine-3-3-36x130", lambda: serpentine(36, 130, 3, 3), UNIT + [(0, 7)]),
    Case("core-comb-down-33x132", lambda: comb(33, 132, False, teeth=3), UNIT + [(5, -3)]),
    Case("core-comb-up-33x132", lambda: comb(33, 132, True, teeth=3), UNIT + [(0, 9)]),
    Case("core-chain-down-40x136", lambda: chain(40, 136, 12, (3, 6), True, blob=(3, 5)), UNIT + [(3, 6)]),
    Case("core-chain-up-40x136", lambda: chain(40, 136, 12, (3, 6), False, blob=(3, 5)), UNIT + [(-3, 6)]),
]
