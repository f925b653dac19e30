"""MN_MAPS_LOGITS: a flag in the `int dtype` of the typed (*_t) entry points, a keyword in the binding; no struct
moved (no GPU)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_flag_and_python_agrees():
    from mergenet_amd import segmenter as seg
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    m = re.search(r"^#define\s+MN_MAPS_LOGITS\s+(\S+)\s*$", text, re.M)
    assert m, "include/mergenet_hip.h does not define MN_MAPS_LOGITS"
    assert m.group(1) == "0x100"
    assert seg.MN_MAPS_LOGITS == int(m.group(1), 16) == 0x100
    # the low byte stays the element type, whose enum did not move
    assert "enum mn_dtype { MN_DTYPE_F32 = 0, MN_DTYPE_F16 = 1, MN_DTYPE_BF16 = 2 }" in text
    assert seg.MN_MAPS_LOGITS & 0xFF == 0


def test_struct_sizes_did_not_move():
    from mergenet_amd import segmenter as seg
    assert ctypes.sizeof(seg.MnOptions) == 17 * 4
    assert ctypes.sizeof(seg.MnStats) == 10 * 4 + 2 * 8 + 8 + 10 * 4 + 6 * 4


def test_no_new_exported_function():
    from mergenet_amd import segmenter as seg
    assert not [n for n in seg.EXPORTS if "logit" in n.lower()]


def test_the_methods_that_take_maps_accept_logits():
    from mergenet_amd import segmenter as seg
    methods = [seg.Merger.segment, seg.Merger.segment_async, seg.Merger.score, seg.Merger.sweep, seg.Merger.sweep_time,
               seg.Merger.exact_phase_a, seg.ExactBatch.segment, seg.MergerPool.submit, seg.MergerPool.map]
    for fn in methods:
        p = inspect.signature(fn).parameters.get("logits")
        assert p is not None, fn.__qualname__
        assert p.default is False, fn.__qualname__
    # the host paths stay probabilities only
    for fn in (seg.run_segmentation, seg.HostContext.segment, seg.ObjectSegmenter.run_segmentation, seg.Merger.prepare):
        assert "logits" not in inspect.signature(fn).parameters, fn.__qualname__
