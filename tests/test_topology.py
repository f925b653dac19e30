"""topology_util on the CPU: its union-find reference against the csegment oracle (and scipy), and each generator's
stated property -- so that the reference of test_gpu_topology.py can be trusted and nobody can quietly simplify a shape.

With the options (0, 1, 0) nothing merges after the first phase on maps built by lean_util.maps_from_labels, so the
oracle's partition must be exactly topology_util.components of the label map: no tolerance anywhere in this file.
"""
import numpy as np
import pytest

import lean_util
import topology_util as tu

ALL = tu.CASES + tu.CORE_CASES


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_components_is_what_the_oracle_ends_in(oracle, case):
    cp, sp = lean_util.maps_from_labels(case.lab, tu.CLASS_OF_LABEL, tu.C, case.offs)
    ref = oracle.run_csegment(cp, sp, tu.C, case.offs, 0.0, 1.0, 0.0)
    assert oracle.same_partition(ref.partition, case.comp)
    assert int(ref.stats["n_objects"]) == tu.count(case.comp)
    mask, classes = tu.reference_mask(case.comp, case.lab, tu.CLASS_OF_LABEL)
    assert oracle.masks_equivalent(ref.mask, ref.object_class, mask, classes)


@pytest.mark.parametrize("name", ["percolation-48x130-unit", "percolation-35x67-unit", "spiral-35x131-unit",
                                  "spiral-48x64-unit"])
def test_components_against_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    case = tu.BY_NAME[name]
    theirs = np.zeros(case.lab.shape, np.int64)
    base = 0
    for value in np.unique(case.lab):
        lbl, n = ndimage.label(case.lab == value)          # (the default structure: 4-connectivity)
        theirs[lbl > 0] = lbl[lbl > 0] + base
        base += n
    assert base == tu.count(case.comp)
    from mergenet_amd.labels import same_partition
    assert same_partition(theirs, case.comp)


def test_components_roots_are_lowest_pixel_ids():
    for name in ("chain-up-40x136-unit-3,6", "comb-down-33x130-unit", "random3-35x131-diag"):
        comp = tu.BY_NAME[name].comp
        ids = np.arange(comp.size, dtype=np.int32).reshape(comp.shape)
        assert (comp <= ids).all()
        roots = np.unique(comp)
        assert (comp.reshape(-1)[roots] == roots).all()


def test_records_between_on_a_hand_made_map():
    lab = np.array([[0, 0, 1], [2, 0, 1], [2, 2, 1]], np.int32)
    comp = tu.components(lab, tu.UNIT)
    assert tu.count(comp) == 3
    assert tu.records_between(comp, tu.UNIT) == 3           # 0|1, 0|2, 2|1
    assert tu.records_between(comp, [(0, 2)]) == 2          # 0|1 (rows 0, 1), 2|1 (row 2)
    assert tu.records_between(comp, [(-2, 0)]) == 1         # 2|0 (column 0); columns 1, 2 stay inside a component


def test_which_cases_leave_the_fused_tail():
    """The speculative attempt's mn_cc_tail takes at most 1024 records; beyond that a default call is redone on the
    waited attempt.  test_gpu_topology.py runs both forms on every case and states which these are."""
    over = sorted(c.name for c in tu.CASES if c.records > 1024)
    assert over == ["percolation-48x130-unit", "percolation-48x130-up", "random3-35x131-diag"]
    assert tu.BY_NAME["percolation-48x130-unit"].records == tu.BY_NAME["percolation-48x130-up"].records == 1314
    assert tu.BY_NAME["random3-35x131-diag"].records == 1159
    assert max(tu.count(c.comp) for c in tu.CASES) <= 2048        # (the tail's other limit, component roots, is not met)


# ---- each generator's stated property ----------------------------------------------------------------------------------

def _fg(case_or_lab, offs=None):
    if offs is None:
        return tu.count(case_or_lab.comp, case_or_lab.lab == 1)
    return tu.count(tu.components(case_or_lab, offs), case_or_lab == 1)


@pytest.mark.parametrize("name", [c.name for c in tu.CASES if c.name.startswith("serpentine")
                                  and c.name.endswith(("-unit", "-up", "-swapped"))])
def test_serpentine_is_one_component_with_closed_gaps(name):
    case = tu.BY_NAME[name]
    assert _fg(case) == 1
    H, W = case.lab.shape
    if min(H, W) > 3:                    # every gap between two arms is a background component of its own
        assert tu.count(case.comp, case.lab == 0) >= (max(H, W) if "vertical" in name else H) // 4


def test_serpentine_arms_span_the_image_and_hug_the_borders():
    lab = tu.serpentine(35, 130, 1, 1)
    assert lab[0::2].all() and lab[16].all() and lab[15].sum() == 1 and lab[17].sum() == 1
    assert lab[1, 129] == 1 and lab[3, 0] == 1                         # turns at alternating ends
    lab = tu.serpentine(35, 130, 2, 2, shift=3)
    assert lab[15].all() and lab[16].all() and lab[14].sum() == 2 and lab[17].sum() == 2
    lab = tu.serpentine(33, 131, 2, 2, shift=3, vertical=True)
    assert lab[:, 63].all() and lab[:, 64].all() and lab[:, 62].sum() == 2 and lab[:, 65].sum() == 2
    # without a unit offset the arm-2 serpentine is connected through diagonals only, one component per colour of the
    # chessboard (every offset of NO_UNIT keeps r + c even or odd)
    assert _fg(tu.BY_NAME["serpentine-2-2-35x130-nounit"]) == 2


@pytest.mark.parametrize("shape", [(35, 131), (48, 64)])
def test_spiral_is_two_corridors(shape):
    lab = tu.spiral(*shape)
    comp = tu.components(lab, tu.UNIT)
    assert tu.count(comp, lab == 1) == 1 and tu.count(comp, lab == 0) == 1
    fg = lab == 1
    # one pixel wide: no 2 x 2 block of one label (but the background's innermost stretch where the height is even)
    for m, most in ((fg, 0), (~fg, 0 if shape[0] % 2 else shape[1])):
        assert (m[:-1, :-1] & m[1:, :-1] & m[:-1, 1:] & m[1:, 1:]).sum() <= most
    assert abs(int(fg.sum()) - lab.size // 2) < lab.size // 8
    # winding: inside the first tile the foreground corridor is many separate pieces
    assert tu.count(tu.components(lab[:16, :64], tu.UNIT), lab[:16, :64] == 1) >= 8


@pytest.mark.parametrize("up", [False, True])
def test_comb_is_one_component_only_through_its_spine(up):
    H, W = 33, 130
    lab = tu.comb(H, W, up)
    teeth = (W + 1) // 2
    assert _fg(lab, tu.UNIT) == 1 and _fg(lab, tu.UNIT_UP) == 1
    # (0, 1) alone: every row of teeth is `teeth` runs of one pixel -- 32 per tile row --, the spine is one run
    assert _fg(lab, [(0, 1)]) == (H - 1) * teeth + 1
    for r in (range(1, H) if up else range(H - 1)):
        assert tu.count(tu.components(lab[r:r + 1], [(0, 1)]), lab[r:r + 1] == 1) == teeth
    assert lab[:16, :64].sum(axis=1).tolist() == ([64] if up else [32]) + [32] * 15
    # without the spine's row the teeth are `teeth` components
    rest = lab[1:] if up else lab[:-1]
    assert _fg(rest, tu.UNIT) == teeth
    assert (lab[0] if up else lab[-1]).all()
    if not up:
        assert tu.components(lab, tu.UNIT)[H - 1, W - 1] == 0      # the root: the top of the first tooth


@pytest.mark.parametrize("anti", [False, True])
def test_stairs_pass_through_the_tile_corner(anti):
    lab = tu.stairs(33, 130, anti)
    corner = {(15, 63): 1, (15, 64): 1, (16, 64): 0 if anti else 1, (16, 63): 1 if anti else 0}
    for (r, c), v in corner.items():
        assert lab[r, c] == v, (r, c)
    assert (lab.sum(axis=1) == 2).all() and lab.sum() == 66          # one pixel wide, first row to last
    assert _fg(lab, tu.UNIT) == 1 and _fg(lab, tu.UNIT_UP) == 1
    assert _fg(lab, [(0, 1)]) == 33 and _fg(lab, [(1, 0)]) == 34     # each unit offset alone: pieces of two pixels
    # cut the two border edges at the corner and it falls apart: inside the four tiles it is four pieces
    tiles = [lab[:16, :64], lab[:16, 64:128], lab[16:32, :64], lab[16:32, 64:128]]
    assert [tu.count(tu.components(t, tu.UNIT), t == 1) if t.any() else 0 for t in tiles] == \
        ([1, 1, 1, 0] if anti else [1, 1, 0, 1])


@pytest.mark.parametrize("down", [True, False])
def test_chain_is_joined_by_its_long_offset_alone(down):
    step = (3, 6) if down else (-3, 6)
    for blob in ((3, 3), (3, 5)):
        lab = tu.chain(40, 136, 12, (3, 6), down, blob=blob)
        assert lab.sum() == 12 * blob[0] * blob[1]
        assert _fg(lab, tu.UNIT) == 12
        assert _fg(lab, tu.UNIT + [step]) == 1
        assert _fg(lab, tu.UNIT + [(-step[0], step[1])]) == 12      # the mirrored offset joins nothing
    comp = tu.components(lab, tu.UNIT)
    roots = [int(comp[r, c]) for r, c in zip(*np.nonzero(lab))]
    cols = [c for r, c in zip(*np.nonzero(lab))]
    # blob after blob along the columns, the roots ascend (down) or descend (up)
    by_col = [r for _, r in sorted(set(zip([(c - min(cols)) // 6 for c in cols], roots)))]
    assert by_col == sorted(by_col, reverse=not down) and len(set(by_col)) == 12
    # ... and the chain crosses a tile border in both directions
    rows = np.nonzero(lab.any(axis=1))[0]
    colsu = np.nonzero(lab.any(axis=0))[0]
    assert rows.min() < 15 and rows.max() > 32 and colsu.min() < 63 and colsu.max() > 64


def test_percolation_and_random_labels():
    lab = tu.percolation(48, 130, 0.6, 7)
    assert np.array_equal(lab, (np.random.default_rng(7).random((48, 130)) < 0.6).astype(np.int32))
    case = tu.BY_NAME["percolation-48x130-unit"]
    assert tu.count(case.comp) > 500 and case.records > 1024
    assert tu.count(tu.components(lab[:16, :64], tu.UNIT)) > 100       # hundreds of components per tile
    case = tu.BY_NAME["random3-35x131-diag"]
    assert sorted(np.unique(case.lab)) == [0, 1, 2] and tu.count(case.comp) > 200


def test_core_cases_are_three_pixels_wide():
    """Arms, teeth and blobs at least three wide and high: the pixels whose four unit neighbours carry their label --
    what core_radius = 1 leaves clean -- are the centre lines, and each label's centre lines are still one winding
    component with the case's offsets."""
    for case in tu.CORE_CASES:
        lab = case.lab
        pad = np.pad(lab, 1, mode="edge")
        clean = ((pad[1:-1, 1:-1] == pad[:-2, 1:-1]) & (pad[1:-1, 1:-1] == pad[2:, 1:-1]) &
                 (pad[1:-1, 1:-1] == pad[1:-1, :-2]) & (pad[1:-1, 1:-1] == pad[1:-1, 2:]))
        core = np.where(clean, lab, -1).astype(np.int32)              # fringe pixels: a label of their own
        fg = clean & (lab == 1)
        assert fg.any() and tu.count(tu.components(core, case.offs), fg) == 1, case
        assert tu.count(case.comp, lab == 1) == 1, case
        assert tu.count(tu.components(core, tu.UNIT), fg) == (12 if "chain" in case.name else 1), case
