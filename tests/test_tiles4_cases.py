"""tiles4_util on the CPU: the union-find reference of its cases against the csegment oracle, as test_topology.py holds
topology_util's, and each case's number of records between components against the table the util states.

With the options (0, 1, 0) nothing merges after the first phase on maps built by lean_util.maps_from_labels, so the
oracle's partition must be exactly topology_util.components of the label map: no tolerance anywhere in this file.
"""
import pytest

import lean_util
import tiles4_util as t4
import topology_util as tu


@pytest.mark.parametrize("case", t4.CASES, ids=repr)
def test_components_is_what_the_oracle_ends_in(oracle, case):
    cp, sp = lean_util.maps_from_labels(case.lab, tu.CLASS_OF_LABEL, tu.C, case.offs)
    ref = oracle.run_csegment(cp, sp, tu.C, case.offs, 0.0, 1.0, 0.0)
    assert oracle.same_partition(ref.partition, case.comp)
    assert int(ref.stats["n_objects"]) == tu.count(case.comp)
    mask, classes = tu.reference_mask(case.comp, case.lab, tu.CLASS_OF_LABEL)
    assert oracle.masks_equivalent(ref.mask, ref.object_class, mask, classes)


@pytest.mark.parametrize("case", t4.CASES, ids=repr)
def test_record_count_is_the_table_s(case):
    assert case.records == t4.RECORDS[case.name]


def test_table_and_cases_match():
    assert sorted(t4.RECORDS) == sorted(c.name for c in t4.CASES)
    assert all(c.lab.shape[1] % 4 == 0 for c in t4.CASES + t4.CORE_CASES)        # every case takes mn_cc_tiles4


def test_which_cases_leave_the_fused_tail():
    """mn_cc_tail takes at most 1024 records and 2048 component roots; beyond that a default call is redone on the
    waited attempt.  test_gpu_tiles4.py runs both attempts on every case."""
    assert sorted(n for n, r in t4.RECORDS.items() if r > 1024) == t4.OVER_THE_TAIL
    assert t4.RECORDS["t4-percolation-48x132-unit"] == t4.RECORDS["t4-percolation-48x132-up"] == 1233
    assert t4.RECORDS["t4-random3-35x132-diag"] == 1086
    assert max(tu.count(c.comp) for c in t4.CASES) <= 2048
