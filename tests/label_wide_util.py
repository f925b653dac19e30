"""Label maps five and more tiles wide for the component labelling (test_label_wide.py, test_gpu_label_wide.py).

The labelling works on tiles of 16 rows x 64 columns, and the table of topology_util stops at three tile columns: a
component there crosses at most two vertical tile borders, and a group of four horizontally adjacent tiles never
exists.  The cases here are topology_util's generators at widths of 6, 8, 9 and 10 tile columns (counts that are no
multiple of four, and one that is) over two or three rows of tiles, with the last tile column cut (322 = 5 * 64 + 2,
515 = 8 * 64 + 3 ...) or full (512).  `records` is the number of records between components, stated here and held to
topology_util.records_between by test_label_wide.py: all stay within the 1024 records of the speculative attempt's
fused tail.
"""
import topology_util as tu

TILE_COLUMNS = {322: 6, 324: 6, 328: 6, 512: 8, 515: 9, 579: 10}


def _table():
    rows = [
        ("wide-serpentine-1-1-35x322", lambda: tu.serpentine(35, 322, 1, 1), [("unit", tu.UNIT, 17), ("up", tu.UNIT_UP, 17)]),
        ("wide-serpentine-vertical-cols63+64-33x515", lambda: tu.serpentine(33, 515, 2, 2, shift=3, vertical=True),
         [("unit", tu.UNIT, 129)]),
        ("wide-spiral-35x579", lambda: tu.spiral(35, 579), [("real", tu.REAL, 1)]),
        ("wide-comb-down-32x512", lambda: tu.comb(32, 512, False), [("unit", tu.UNIT, 256)]),     # N % 4 == 0: the lean form
        ("wide-comb-up-33x322", lambda: tu.comb(33, 322, True), [("unit+long", tu.UNIT + [(0, 9), (5, -3)], 161)]),
        ("wide-stairs-33x322", lambda: tu.stairs(33, 322), [("up", tu.UNIT_UP, 2)]),
        ("wide-chain-down-40x328", lambda: tu.chain(40, 328, 12, (3, 6), True), [("unit+3,6", tu.UNIT + [(3, 6)], 1)]),
        ("wide-percolation-48x322", lambda: tu.percolation(48, 322, 0.6, 7), [("real", tu.REAL, 27)]),
        ("wide-serpentine-2-2-34x324", lambda: tu.serpentine(34, 324, 2, 2), [("nounit", tu.NO_UNIT, 16)]),
    ]
    cases, records = [], {}
    for name, make, lists in rows:
        for tag, offs, n in lists:
            case = tu.Case("%s-%s" % (name, tag), make, offs)
            cases.append(case)
            records[case.name] = n
    return cases, records


CASES, RECORDS = _table()
assert len(RECORDS) == len(CASES) and not set(RECORDS) & set(tu.BY_NAME)
