"""label_wide_util on the CPU: the csegment oracle's partition on every wide case is topology_util.components, as
test_topology.py holds it for topology_util's own table -- so that the reference of test_gpu_label_wide.py is itself held
to the oracle -- and the cases are as wide as they say: no tolerance anywhere in this file.
"""
import pytest

import label_wide_util as lw
import lean_util
import topology_util as tu


@pytest.mark.parametrize("case", lw.CASES, ids=repr)
def test_components_is_what_the_oracle_ends_in(oracle, case):
    cp, sp = lean_util.maps_from_labels(case.lab, tu.CLASS_OF_LABEL, tu.C, case.offs)
    ref = oracle.run_csegment(cp, sp, tu.C, case.offs, 0.0, 1.0, 0.0)
    assert oracle.same_partition(ref.partition, case.comp)
    assert int(ref.stats["n_objects"]) == tu.count(case.comp)
    mask, classes = tu.reference_mask(case.comp, case.lab, tu.CLASS_OF_LABEL)
    assert oracle.masks_equivalent(ref.mask, ref.object_class, mask, classes)


def test_every_case_stays_in_the_fused_tail():
    """At most 1024 records between components (and 2048 roots): a default call ends in mn_cc_tail, so the `tail`
    attempt of test_gpu_label_wide.py is the speculative one on every case."""
    assert {c.name: c.records for c in lw.CASES} == lw.RECORDS
    assert max(lw.RECORDS.values()) <= 1024
    assert max(tu.count(c.comp) for c in lw.CASES) <= 2048


def test_cases_are_as_wide_as_they_say():
    """Five or more tile columns on every case: counts that are no multiple of four (6, 9, 10) and one that is (8);
    two or more rows of tiles; a last tile column that is cut, and one that is full."""
    cols = set()
    for case in lw.CASES:
        H, W = case.lab.shape
        assert (W + 63) // 64 == lw.TILE_COLUMNS[W] >= 5 and (H + 15) // 16 >= 2, case
        cols.add(lw.TILE_COLUMNS[W])
    assert cols == {6, 8, 9, 10}
    assert {c.lab.shape[1] % 64 == 0 for c in lw.CASES} == {True, False}
    lean = [c for c in lw.CASES if c.lab.size % 4 == 0 and c.lab.shape[1] % 4 == 0]      # four pixels per lane
    assert "wide-comb-down-32x512-unit" in [c.name for c in lean]


def test_shapes_keep_their_properties_at_this_width():
    """What makes each shape hard holds at the wide sizes too (test_topology.py states it at two or three columns)."""
    by = {c.name: c for c in lw.CASES}

    def fg(case):
        return tu.count(case.comp, case.lab == 1)

    for name in ("wide-serpentine-1-1-35x322-unit", "wide-serpentine-1-1-35x322-up",
                 "wide-serpentine-vertical-cols63+64-33x515-unit", "wide-spiral-35x579-real",
                 "wide-comb-down-32x512-unit", "wide-comb-up-33x322-unit+long", "wide-stairs-33x322-up",
                 "wide-chain-down-40x328-unit+3,6"):
        assert fg(by[name]) == 1, name
    # the comb's 32 teeth per tile are one component only through the spine, outside all but one row of tiles
    lab = by["wide-comb-down-32x512-unit"].lab
    assert tu.count(tu.components(lab[:16], tu.UNIT), lab[:16] == 1) == 256
    # the chain's blobs are joined by the long offset alone
    case = by["wide-chain-down-40x328-unit+3,6"]
    assert tu.count(tu.components(case.lab, tu.UNIT), case.lab == 1) == 12
    # without a unit offset: one component per colour of the chessboard
    assert fg(by["wide-serpentine-2-2-34x324-nounit"]) == 2
