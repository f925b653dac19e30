"""Which event the component contraction records between which kernels, seen through the timings of ``mn_stats``:
``ms_cc_edges`` (the sweep), ``ms_cc_label`` (tiles to hook), ``ms_cc_sums``, ``ms_cc_cross``, and the phases
``ms_merge`` / ``ms_output`` / ``ms_total`` around them.  An interval between two recorded events, in stream order, is
finite and positive; one whose events ``debug_flags`` switched off stays at the 0 the stats start from.

64 x 128, C = 9, the ten offsets of generate_offsets(40, 10), four instances: the smallest map on which every stage of
the contraction has work and the attempt stays on the speculative tail.
"""
import math

import pytest
import torch

from mergenet_amd import segmenter as seg, synth

pytestmark = pytest.mark.gpu

H, W, C = 64, 128, 9
OFFS = [tuple(int(x) for x in o) for o in synth.generate_offsets(40, 10)]
CC = ["ms_cc_edges", "ms_cc_label", "ms_cc_sums", "ms_cc_cross"]


@pytest.fixture(scope="module")
def maps():
    s = synth.synth_v1(H, W, C, OFFS, 1001, num_instances=4)
    return torch.from_numpy(s.class_probs).cuda(), torch.from_numpy(s.sameness_probs).cuda()


def _stats(maps, mode=seg.MN_MODE_COMPONENTS, flags=0):
    m = seg.Merger(H, W, C, len(OFFS))       # a fresh context: no event of an earlier call is left to read
    try:
        o = seg.default_options(mode=mode, require_proof=-1, debug_flags=flags)
        st = m.segment(maps[0], maps[1], OFFS, o)[3]
        torch.cuda.synchronize()
    finally:
        m.close()
    print({k: v for k, v in st.items() if k.startswith("ms_") or k == "mode_used"})
    assert st["status"] == 0
    return st


def test_every_interval_is_recorded(maps):
    st = _stats(maps)
    assert st["mode_used"] == seg.MN_MODE_COMPONENTS
    for k in CC + ["ms_merge", "ms_output", "ms_total"]:
        assert math.isfinite(st[k]) and st[k] > 0, (k, st[k])
    assert st["ms_total"] >= st["ms_cc_edges"]


def test_lean_events_time_the_sweep_alone(maps):
    st = _stats(maps, flags=seg.MN_DEBUG_LEAN_EVENTS)
    assert st["mode_used"] == seg.MN_MODE_COMPONENTS
    assert st["ms_cc_edges"] > 0
    for k in ["ms_cc_label", "ms_cc_sums", "ms_cc_cross", "ms_total"]:
        assert st[k] == 0, (k, st[k])


def test_no_events(maps):
    st = _stats(maps, flags=seg.MN_DEBUG_NO_EVENTS)
    for k in CC:
        assert st[k] == 0, (k, st[k])


def test_rounds_mode_times_the_cores_sweep(maps):
    st = _stats(maps, mode=seg.MN_MODE_ROUNDS)
    assert st["ms_edge_pass"] > 0
    assert st["ms_total"] > 0
