"""The C ABI of libmergenet_hip.so (include/mergenet_hip.h) as data: its constants, its two structs and the signature
of every exported function.  Imports only ctypes -- no library, no torch, no GPU -- so that
tests/test_abi_signatures.py can hold every line of it to the header on any machine.  ``segmenter.load_library``
applies ``SIGNATURES`` to the loaded library; ``segmenter`` re-exports every name of ``__all__``."""
import ctypes
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

MN_VARIANT_CSEGMENT = 0
MN_VARIANT_PYSEGMENTER = 1
MN_MODE_AUTO, MN_MODE_EXACT, MN_MODE_ROUNDS, MN_MODE_COMPONENTS = 0, 1, 2, 3
MN_ERR_NO_BACKGROUND = -10
MN_ERR_UNPROVEN = -30
MN_DEBUG_GENERIC_EDGE_PASS, MN_DEBUG_NO_EVENTS, MN_DEBUG_NO_CORES = 1, 2, 4
MN_DEBUG_LEAN_EVENTS, MN_DEBUG_REPLAY = 16, 32
MN_DEBUG_SWEEP_EVENT_PACKETS = 128   # the sweep is timed by an event packet before and behind it
MN_DEBUG_SWEEP16_4PX = 256    # a 16-bit map's sweep takes 4 pixels per lane (8-byte loads) where it would take 8
MN_DEBUG_SWEEP_FULL_FORM = 512   # the sweep of components mode leaves the full form of its outputs, not the lean one
MN_DEBUG_TILES_1PX = 1024   # the labelling's tile stage takes one pixel per lane (mn_cc_tiles) where it would take four
MN_DTYPE_F32, MN_DTYPE_F16, MN_DTYPE_BF16 = 0, 1, 2   # enum mn_dtype: element type of the maps (*_t entry points)
MN_MAPS_LOGITS = 0x100   # or-ed into that dtype: both maps hold logits, the kernels take the sigmoid on load
MN_PART_CLASS, MN_PART_OFFSET = 0, 1          # the part of the output a plane-loss call takes (Merger.plane_sums)
MN_PLANE_COMPLEMENT, MN_PLANE_TERMS = 1, 2    # its flags
MN_CRIT_DICE, MN_CRIT_MBCE = 0, 1             # the criteria of Merger.plane_coeffs
MN_ERR_ARGUMENT = -1
MN_ERR_CAPACITY = -4
MN_MATCH_MAX_INSTANCES = 4096   # most prediction / truth instances of Merger.match_instances
MN_EVAL_RECORD_BYTES = 32        # a record of the evaluation log (DatasetEval)
MN_EVAL_MAX_AREAS, MN_EVAL_MAX_DETS = 4, 4
MN_EVAL_CHUNK = 256              # records the accumulate pass scans per step
MN_PROVE_ALWAYS, MN_PROVE_BY_MODE, MN_PROVE_NEVER = 1, 0, -1   # mn_options.require_proof (the header says it in prose)
MN_TIES_DEFAULT, MN_TIES_REFERENCE, MN_TIES_LOWEST_ID = 0, 1, 2   # mn_options.tie_order
MN_PROOF_NONE, MN_PROOF_CERTIFICATE, MN_PROOF_SEQUENTIAL, MN_PROOF_SEQUENTIAL_TIES = 0, 1, 2, 3   # mn_stats.proof


class MnOptions(ctypes.Structure):
    _fields_ = [("same_different_bias", c_float), ("object_merge_factor", c_float),
                ("merge_logprob_bias", c_float), ("variant", c_int),
                ("mode", c_int), ("clip_inputs", c_int),
                ("exact_limit", c_int), ("finish_limit", c_int),
                ("subrounds", c_int), ("prune_threshold", c_float),
                ("compute_logprob", c_int), ("no_handover_refresh", c_int),
                ("band_permille", c_int), ("debug_flags", c_int),
                ("require_proof", c_int), ("core_radius", c_int),
                ("tie_order", c_int)]


class MnStats(ctypes.Structure):
    _fields_ = [("status", c_int), ("mode_used", c_int), ("certified", c_int),
                ("num_instances", c_int), ("num_objects", c_int),
                ("rounds", c_int), ("finisher_steps", c_int),
                ("cert_edge_violations", c_int),
                ("cert_class_violations", c_int), ("cert_record_violations", c_int),
                ("initial_records", c_longlong),
                ("merges", c_longlong), ("total_logprob", c_double),
                ("ms_score", c_float), ("ms_class_pass", c_float),
                ("ms_edge_pass", c_float), ("ms_merge", c_float),
                ("ms_output", c_float), ("ms_total", c_float),
                ("ms_cc_label", c_float), ("ms_cc_sums", c_float),
                ("ms_cc_edges", c_float), ("ms_cc_cross", c_float),
                ("proof", c_int), ("cores_condemned", c_int), ("tied_steps", c_int), ("tied_merges", c_int),
                ("tie_order_used", c_int), ("tied_conflicts", c_int)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


_f32p = POINTER(c_float)
_i32p = POINTER(c_int)


def _signatures() -> dict:
    P, I, L, F, D = c_void_p, c_int, c_longlong, c_float, c_double
    FP, IP, DP, LP, PP = _f32p, _i32p, POINTER(c_double), POINTER(c_longlong), POINTER(c_void_p)
    OPT, ST = POINTER(MnOptions), POINTER(MnStats)
    s = {
        "mn_default_options": (None, [OPT]),
        "mn_create": (P, [I, I, I, I, I]),
        "mn_destroy": (None, [P]),
        "mn_workspace_bytes": (c_size_t, [P]),
        "mn_segment_device": (I, [P, P, I, P, I, I, I, I, IP, P, P, P, OPT, P, ST]),
        "mn_segment_finish": (I, [P, ST]),
        "mn_segment_exact_batch": (I, [PP, I, PP, I, PP, I, I, I, I, IP, PP, PP, PP, OPT, P, ST]),
        "mn_score_device": (I, [P, P, I, P, I, I, I, I, IP, OPT, P, P, P, FP, FP]),
        "mn_exact_phase_a_device": (I, [P, P, I, P, I, I, I, I, IP, OPT, P, P, P, P]),
        "mn_sweep_device": (I, [P, P, I, P, I, I, I, I, IP, OPT, P, P, P, P, P, DP, IP]),
        "mn_sweep_time_device": (I, [P, PP, PP, I, I, I, I, I, I, IP, OPT, P, I, FP]),
        "mn_segment_host": (I, [P, FP, I, FP, I, I, I, I, IP, IP, IP, IP, OPT, ST]),
        "c_run_segmentation": (None, [FP, I, FP, I, I, I, I, IP, IP, IP, F, F, F]),
        "mn_prepare_device": (I, [P, P, I, I, I, P, I, I, I, I, P]),
        "mn_prepare_device_t": (I, [P, P, I, I, I, I, P, I, I, I, I, I, P]),
        "mn_upsample_mask_device": (I, [P, P, I, I, P, I, I, P]),
        "mn_rle_points_device": (I, [P, P, I, I, P, I, IP, P]),
        "mn_rle_encode_host": (L, [IP, I, I, I, I, I, P, L, LP, IP]),
        "mn_rle_counts_host": (L, [c_char_p, L, P, L, LP]),
        "mn_rle_decode_device": (I, [P, P, P, I, I, P, I, I, P, P, P, P, P]),
        "mn_sameness_targets_device": (I, [P, P, I, I, IP, I, P, P]),
        "mn_instance_scores_device": (I, [P, P, P]),
        "mn_instance_table_device": (I, [P, P, I, I, I, P, P]),
        "mn_filter_instances_device": (I, [P, P, I, I, I, P, P, P, I, F, P, P, P, P, P, P, P]),
        "mn_overlap_table_device": (I, [P, P, P, I, I, I, I, P, P]),
        "mn_match_overlaps_device": (I, [P, P, I, I, P, P, P, P, DP, I, D, D, P, P, P, P, P, P]),
        "mn_map_scores_device": (I, [P, P, I, P, I, I, I, I, I, IP, P, I, P, P, P, I, P]),
        "mn_mask_bce_device": (I, [P, P, P, I, I, I, I, I, IP, P, I, P, P, P, F, F, P, I, P]),
        "mn_plane_sums_device": (I, [P, P, I, I, I, I, I, IP, P, I, P, I, P, I, P]),
        "mn_plane_coeffs_device": (I, [P, I, I, P, I, D, D, D, P, P, I, P]),
        "mn_plane_grad_device": (I, [P, P, I, I, I, I, I, IP, P, I, P, I, P, P, P, P]),
        "mn_mask_ce_device": (I, [P, P, I, I, I, I, I, IP, P, I, P, P, F, P, I, P]),
        "mn_tile_class_maps_device": (I, [P, P, P, I, I, I, I, IP, I, IP, I, I, I, I, P, I, I, P]),
        "mn_eval_append_device": (I, [P, P, I, I, P, P, P, P, DP, I, DP, I, I, I, I, P, P, P]),
        "mn_eval_keys_device": (I, [P, P, L, I, P, P]),
        "mn_eval_accumulate_device": (I, [P, P, L, P, P, P, I, I, P, I, I, IP, I, P, P, P, P]),
        "mn_pack_wire_device": (I, [P, P, I, D, I, I, P, P]),
        "mn_runs_wire_words": (c_size_t, [I, I]),
        "mn_pack_runs_device": (I, [P, P, P, I, D, I, I, I, P, P]),
        "mn_unpack_runs_device": (I, [P, I, I, I, P, P, P]),
        "mn_unpack_runs_batch_device": (I, [P, L, I, I, I, I, P, P, P]),
        "mn_last_status": (I, []),
        "mn_status_string": (c_char_p, [I]),
        "mn_version": (c_char_p, []),
    }
    s["mn_segment_launch"] = (I, s["mn_segment_device"][1][:-1])      # the same call without the statistics
    # the typed forms: `int dtype` right after the group of the two map pointers
    for name, at in (("mn_segment_device", 5), ("mn_segment_launch", 5), ("mn_segment_exact_batch", 6),
                     ("mn_score_device", 5), ("mn_exact_phase_a_device", 5), ("mn_sweep_device", 5),
                     ("mn_sweep_time_device", 3)):
        argtypes = s[name][1]
        s[name + "_t"] = (I, argtypes[:at] + [I] + argtypes[at:])
    return s


SIGNATURES = _signatures()      # name -> (restype, argtypes) of every function the header declares
EXPORTS = list(SIGNATURES)

__all__ = [n for n in dir() if n.startswith("MN_")] + ["MnOptions", "MnStats", "_f32p", "_i32p", "SIGNATURES", "EXPORTS"]
