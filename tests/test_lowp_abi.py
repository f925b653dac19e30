"""The typed (*_t) entry points of the C ABI: listed, exported, and nothing else moved (no GPU)."""
import ctypes

TYPED = ["mn_segment_device_t", "mn_segment_launch_t", "mn_segment_exact_batch_t", "mn_score_device_t",
         "mn_sweep_device_t", "mn_sweep_time_device_t", "mn_exact_phase_a_device_t", "mn_prepare_device_t"]


def test_typed_entry_points_are_listed_and_exported():
    import __graft_entry__ as g
    g.build()
    from mergenet_amd import segmenter as seg
    lib = seg.load_library()
    for name in TYPED:
        assert name in seg.EXPORTS, name
        assert hasattr(lib, name), name
        assert hasattr(lib, name[:-2]), name[:-2]          # the float entry point is still there


def test_struct_sizes_did_not_move():
    from mergenet_amd import segmenter as seg
    assert ctypes.sizeof(seg.MnOptions) == 17 * 4
    assert ctypes.sizeof(seg.MnStats) == 10 * 4 + 2 * 8 + 8 + 10 * 4 + 6 * 4
    assert (seg.MN_DTYPE_F32, seg.MN_DTYPE_F16, seg.MN_DTYPE_BF16) == (0, 1, 2)


def test_header_declares_the_dtype_enum_and_the_typed_forms():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "mergenet_hip.h")).read()
    assert "enum mn_dtype { MN_DTYPE_F32 = 0, MN_DTYPE_F16 = 1, MN_DTYPE_BF16 = 2 }" in text
    for name in TYPED:
        assert name + "(" in text, name
