"""The labelling chain on images five and more tiles wide.  topology_util's table stops at three tile columns: a
component there crosses at most two vertical tile borders; here the chains of tile roots that the border stage builds
and chases (mn_cc_find2: both ends of an edge step together) run over up to nine borders of a row of tiles.

The cases are label_wide_util's (6, 8, 9 and 10 tile columns over two or three rows of tiles); the checks are
test_gpu_topology.py's own -- status 0, MN_MODE_COMPONENTS, the partition equal to topology_util.components, the
certificate, two runs on one Merger bit-equal -- on the `tail` and the `waited` attempt.  Every case has at most 1024
records between components (test_label_wide.py), so the `tail` attempt is the speculative one that ends in mn_cc_tail;
32x512 takes the lean form of the sweep.  test_label_wide.py holds the reference to the csegment oracle on the CPU.
"""
import pytest

import label_wide_util as lw
from test_gpu_topology import ATTEMPTS, _check_components

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("attempt", list(ATTEMPTS))
@pytest.mark.parametrize("case", lw.CASES, ids=repr)
def test_wide_labelling_is_the_union_find_partition(oracle, case, attempt):
    _check_components(case, oracle, **ATTEMPTS[attempt])
