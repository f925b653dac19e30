"""The case table of the four-pixel tile stage (mn_cc_tiles4): topology_util's generators at widths divisible by 4.

mn_cc_tiles4 runs where W % 4 == 0; nearly every case of topology_util.CASES has another width and keeps running the
one-pixel kernel.  These shapes put what the generators are hard for against a lane's four pixels and a DPP row's 64:
three live rows, then one, in the last tile row and a last tile column of 4 pixels (35x132, 17x68); rows 15 | 16 and
columns 63 | 64 as one arm; a 2-pixel run at every alignment against a lane's pixels (vertical serpentines, shift
0..3) and 3-pixel runs drifting through all lane positions (teeth of 3); offset lists with the horizontal unit offset
second, with the vertical one pointing up, with neither; narrow images and cut tile columns (widths 4, 8, 60, 64, 68).

``RECORDS`` states each case's number of records between components (topology_util.records_between), computed once on
the CPU; test_tiles4_cases.py holds the table to it.  Three cases exceed the 1024 records of the fused tail and are
redone by the library on the waited attempt, as three of topology_util.CASES are.
"""
import topology_util as tu
from topology_util import NO_UNIT, REAL, UNIT, UNIT_UP, Case

SWAPPED = [(1, 0), (0, 1)]            # kh = 1, kv = 0
DIAG = UNIT + [(1, 1), (2, -1)]
NARROW = (4, 8, 60, 64, 68)


def _cases():
    out = []

    def add(name, make, lists):
        for tag, offs in lists:
            out.append(Case("t4-%s-%s" % (name, tag), make, offs))

    both = [("unit", UNIT), ("up", UNIT_UP)]
    for (H, W) in [(35, 132), (17, 68)]:
        add("serpentine-1-1-%dx%d" % (H, W), lambda H=H, W=W: tu.serpentine(H, W, 1, 1), both)
    add("serpentine-2-2-rows15+16-35x132", lambda: tu.serpentine(35, 132, 2, 2, shift=3), both)
    for s in range(4):
        add("serpentine-vertical-2-2-shift%d-33x132" % s, lambda s=s: tu.serpentine(33, 132, 2, 2, shift=s, vertical=True),
            both if s == 3 else both[:1])
    add("serpentine-vertical-1-1-33x132", lambda: tu.serpentine(33, 132, 1, 1, vertical=True), [("swapped", SWAPPED)])
    add("serpentine-2-2-34x68", lambda: tu.serpentine(34, 68, 2, 2), [("nounit", NO_UNIT)])
    for up in (False, True):
        add("comb-%s-33x132" % ("up" if up else "down"), lambda up=up: tu.comb(33, 132, up), both)
    add("comb-down-teeth3-32x136", lambda: tu.comb(32, 136, False, teeth=3), both)
    for anti in (False, True):
        add("stairs-%s33x132" % ("anti-" if anti else ""), lambda anti=anti: tu.stairs(33, 132, anti), both)
    add("spiral-35x132", lambda: tu.spiral(35, 132), both + [("real", REAL)])
    add("spiral-48x64", lambda: tu.spiral(48, 64), both)
    add("percolation-48x132", lambda: tu.percolation(48, 132, 0.6, 7), both + [("real", REAL)])
    add("percolation-35x68", lambda: tu.percolation(35, 68, 0.6, 7), both)
    add("random3-35x132", lambda: tu.random_labels(35, 132, 3, 11), [("diag", DIAG)])
    for W in NARROW:
        add("serpentine-1-1-18x%d" % W, lambda W=W: tu.serpentine(18, W, 1, 1), both)
        add("comb-down-18x%d" % W, lambda W=W: tu.comb(18, W, False), both)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) == 54

# the sweep's full form is also run on these (test_gpu_tiles4.py)
FORM_CASES = [c for c in CASES if c.name.startswith(("t4-serpentine", "t4-comb", "t4-percolation"))]

# cores: the two shapes of topology_util.CORE_CASES that are 132 wide
CORE_CASES = [c for c in tu.CORE_CASES if c.name.endswith("x132")]
assert len(CORE_CASES) == 2

OVER_THE_TAIL = ["t4-percolation-48x132-unit", "t4-percolation-48x132-up", "t4-random3-35x132-diag"]

# records between components per case
RECORDS = {
    "t4-serpentine-1-1-35x132-unit": 17,
    "t4-serpentine-1-1-35x132-up": 17,
    "t4-serpentine-1-1-17x68-unit": 8,
    "t4-serpentine-1-1-17x68-up": 8,
    "t4-serpentine-2-2-rows15+16-35x132-unit": 9,
    "t4-serpentine-2-2-rows15+16-35x132-up": 9,
    "t4-serpentine-vertical-2-2-shift0-33x132-unit": 33,
    "t4-serpentine-vertical-2-2-shift1-33x132-unit": 34,
    "t4-serpentine-vertical-2-2-shift2-33x132-unit": 33,
    "t4-serpentine-vertical-2-2-shift3-33x132-unit": 33,
    "t4-serpentine-vertical-2-2-shift3-33x132-up": 33,
    "t4-serpentine-vertical-1-1-33x132-swapped": 66,
    "t4-serpentine-2-2-34x68-nounit": 16,
    "t4-comb-down-33x132-unit": 66,
    "t4-comb-down-33x132-up": 66,
    "t4-comb-up-33x132-unit": 66,
    "t4-comb-up-33x132-up": 66,
    "t4-comb-down-teeth3-32x136-unit": 23,
    "t4-comb-down-teeth3-32x136-up": 23,
    "t4-stairs-33x132-unit": 2,
    "t4-stairs-33x132-up": 2,
    "t4-stairs-anti-33x132-unit": 2,
    "t4-stairs-anti-33x132-up": 2,
    "t4-spiral-35x132-unit": 1,
    "t4-spiral-35x132-up": 1,
    "t4-spiral-35x132-real": 1,
    "t4-spiral-48x64-unit": 1,
    "t4-spiral-48x64-up": 1,
    "t4-percolation-48x132-unit": 1233,
    "t4-percolation-48x132-up": 1233,
    "t4-percolation-48x132-real": 9,
    "t4-percolation-35x68-unit": 468,
    "t4-percolation-35x68-up": 468,
    "t4-random3-35x132-diag": 1086,
    "t4-serpentine-1-1-18x4-unit": 9,
    "t4-serpentine-1-1-18x4-up": 9,
    "t4-comb-down-18x4-unit": 2,
    "t4-comb-down-18x4-up": 2,
    "t4-serpentine-1-1-18x8-unit": 9,
    "t4-serpentine-1-1-18x8-up": 9,
    "t4-comb-down-18x8-unit": 4,
    "t4-comb-down-18x8-up": 4,
    "t4-serpentine-1-1-18x60-unit": 9,
    "t4-serpentine-1-1-18x60-up": 9,
    "t4-comb-down-18x60-unit": 30,
    "t4-comb-down-18x60-up": 30,
    "t4-serpentine-1-1-18x64-unit": 9,
    "t4-serpentine-1-1-18x64-up": 9,
    "t4-comb-down-18x64-unit": 32,
    "t4-comb-down-18x64-up": 32,
    "t4-serpentine-1-1-18x68-unit": 9,
    "t4-serpentine-1-1-18x68-up": 9,
    "t4-comb-down-18x68-unit": 34,
    "t4-comb-down-18x68-up": 34,
}
