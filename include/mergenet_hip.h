/* mergenet_hip.h -- C ABI of libmergenet_hip.so (MI355X / gfx950 pixel merger).
 *
 * Drop-in boundary for the MergeNet post-processor (the greedy merger that folds pixels into
 * instances by log-likelihood gain).  Plain pointers and sizes only; no torch / C++ types.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   c_run_segmentation      utils/csegment/segment.cc:742-765 (declared to Cython at
 *                           utils/csegment/c_segment.pyx:16-25)  -- same symbol, same signature
 *   ObjectSegmenterOption   utils/csegment/segment.h:245-268     -- mn_options (3 floats + mode)
 *   ObjectSegmenter ctor    utils/csegment/segment.cc:153-232    -- phase A (affinity scoring)
 *   RunSegmentation/Merge   utils/csegment/segment.cc:539-727    -- phase B (merge)
 *   OutputMask              utils/csegment/segment.cc:491-517    -- label / class-table output
 *   ObjectSegmenter (py)    utils/segmenter.py:225-483           -- MN_VARIANT_PYSEGMENTER
 *
 * Error behaviour: the reference returns void and calls exit(1) on internal inconsistencies
 * (segment.cc:39-43,96-100,665-673).  Here every entry point except the ABI-compatible
 * c_run_segmentation returns an int status (0 = MN_OK) and never exits; c_run_segmentation
 * keeps the void signature, prints the failure to stderr and leaves mn_last_status() set.
 *
 * Threading: an mn_context owns one GPU workspace and is used by one thread at a time; separate
 * contexts are independent (one per GPU / per process in the multi-GPU driver).
 */
#ifndef MERGENET_HIP_H_
#define MERGENET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MN_MAX_OFFSETS 32
#define MN_MAX_CLASSES 127

enum mn_status {
  MN_OK = 0,
  MN_ERR_ARGUMENT = -1,     /* null pointer, non-positive size, class_dim < num_classes, ...  */
  MN_ERR_OFFSETS = -2,      /* (0,0), a duplicate, or an offset together with its negation    */
  MN_ERR_NO_DEVICE = -3,    /* no usable HIP device / HIP call failed (message on stderr)     */
  MN_ERR_CAPACITY = -4,     /* image larger than the context was created for                  */
  MN_ERR_NO_BACKGROUND = -10, /* pysegmenter prune: no class-0 object (reference: NameError)  */
  MN_ERR_INTERNAL = -20,
  MN_ERR_UNPROVEN = -30     /* a proven result was asked for (require_proof) and could not be had: no room for
                               the exact engine's or the reference-order loop's workspace, or a Python-variant
                               result whose tied choices conflict (the output then holds that proof 3 result) */
};

enum mn_variant {
  MN_VARIANT_CSEGMENT = 0,    /* utils/csegment semantics: den = n1+n2, bias outside, merge on == */
  MN_VARIANT_PYSEGMENTER = 1  /* utils/segmenter.py: den = n1*n2, bias inside, merge on >=, prune */
};

enum mn_mode {
  MN_MODE_AUTO = 0,      /* the reference's result, by the cheapest route that PROVES it: EXACT when the
                            image has <= exact_limit initial records; else COMPONENTS, kept when the
                            certificate holds (any order of the lazy greedy ends in this partition);
                            else EXACT (require_proof = -1: keep the fast path's unproven answer)   */
  MN_MODE_EXACT = 1,     /* the reference's sequential lazy-greedy order itself, any image size: the
                            exact engine (mn_kernels_exact.h) -- float32 state and operation order of
                            segment.cc, glibc's logf / expf restated bit for bit, pop = block-max queue in
                            LDS, per-object adjacency, pair table (seconds per image: DESIGN.md section 6) */
  MN_MODE_ROUNDS = 2,    /* parallel rounds + sequential finisher + certificate                  */
  MN_MODE_COMPONENTS = 3 /* sign-separable inputs: phase 1 of the merge (provably order-
                            independent there) by one union-find sweep over the positive edges,
                            then rounds/finisher on the records between components; falls back to
                            ROUNDS when the input is not sign-separable (mode_used tells)         */
};

/* Element type of the probability maps handed to the *_t entry points (both maps of a call share one). */
enum mn_dtype { MN_DTYPE_F32 = 0, MN_DTYPE_F16 = 1, MN_DTYPE_BF16 = 2 };   /* IEEE binary32 / binary16 / bfloat16 */

enum mn_tie_order { MN_TIES_DEFAULT = 0, MN_TIES_REFERENCE = 1, MN_TIES_LOWEST_ID = 2 };
/* mn_stats.proof */
enum mn_proof {
  MN_PROOF_NONE = 0,             /* measured only: an approximation of the sequential order on order-dependent inputs */
  MN_PROOF_CERTIFICATE = 1,      /* ANY order of the lazy greedy ends in this partition          */
  MN_PROOF_SEQUENTIAL = 2,       /* the reference's sequential order was run and no choice among bit-equal priorities
                                    was left to the engine: every pop was forced (tied_steps == 0), or the reference's
                                    own heap / hash-map order among equals was reproduced (tie_order_used ==
                                    MN_TIES_REFERENCE), or there were tied pops whose choices provably commute
                                    (tied_steps > 0, tied_conflicts == 0: no tied choice wrote what another read or
                                    wrote, so every order among equals ends in this state; mn_kernels_exact.h "ties") */
  MN_PROOF_SEQUENTIAL_TIES = 3   /* the sequential order was run, but some pops chose among bit-equal priorities by
                                    the engine's rule (lowest record id) where the reference's std::priority_queue
                                    chooses by heap position: equal to the reference on most vectors held at the
                                    benchmark's sizes, differing on the radius-4 blurred ones and on one blurred 1024x2048; require_proof = 1 redoes such an
                                    image in the reference's order                                                   */
};
#define MN_TIE_LIMIT_RECORDS 400000   /* MN_TIES_DEFAULT: largest image (initial records) redone in the reference's order */
#define MN_TIE_LIMIT_BATCH_RECORDS 1400000   /* ... inside mn_segment_exact_batch, where the images are redone together (256x512 at O = 10) */

/* mn_options.debug_flags.  (Round 4 removed the opt-in engines that were measured slower or known to deviate: bits 3,
   10-13; bit 9 was among them and now means the below.) */
enum mn_debug_flags {
  MN_DEBUG_GENERIC_EDGE_PASS = 1,      /* use the generic edge pass where the fast form would run (tests compare the two) */
  MN_DEBUG_NO_EVENTS = 2,              /* no per-kernel timestamps in components mode (ms_cc_* stay 0; each is an event
                                          on the caller's stream) */
  MN_DEBUG_NO_CORES = 4,               /* general rounds from single pixels instead of from the cores */
  MN_DEBUG_LEAN_EVENTS = 16,           /* only the sweep is timed (ms_cc_edges; the other ms_* stay 0) -- an event costs
                                          the host ~3.5 us to record and ~8 us to read */
  MN_DEBUG_REPLAY = 32,                /* (with MN_DEBUG_LEAN_EVENTS) replay -- when mn_segment_launch is called again with
                                          the same buffers, shape, options and stream, the launches after the sweep are
                                          recorded into two hipGraphs (second call) and replayed (from the third): a loop
                                          over images through fixed buffers */
  MN_DEBUG_SWEEP_EVENT_PACKETS = 128,  /* time the sweep with an event packet before and behind it instead of start/stop
                                          events on its own dispatch (round 2's first form: measures dispatch gap + kernel) */
  MN_DEBUG_SWEEP16_4PX = 256,          /* a 16-bit map's sweep takes 4 pixels per lane (8-byte loads) where it would take 8
                                          (16-byte loads) -- same results, for the measurement of the two forms */
  MN_DEBUG_TILES_1PX = 1024,           /* the tile stage of the labelling takes one pixel per lane (mn_cc_tiles) where it
                                          would take four (mn_cc_tiles4: W % 4 == 0, 16-byte aligned arrays) -- same
                                          parent[] bit for bit, the yardstick of the four-pixel kernel inside one build */
  MN_DEBUG_SWEEP_FULL_FORM = 512       /* the sweep of components mode leaves the FULL form of its outputs (two mask words
                                          per pixel, per-lane class log-products for every lane) where the default path
                                          takes the lean form (one packed word for up to 16 offsets, one record per uniform
                                          64-pixel run) -- same results bit for bit, the yardstick of the lean form inside
                                          one build; the replay key holds the options, so the two forms never share graphs */
};

typedef struct mn_options {
  float same_different_bias;   /* segment.h:246 */
  float object_merge_factor;   /* segment.h:247 */
  float merge_logprob_bias;    /* segment.h:248 */
  int variant;                 /* enum mn_variant */
  int mode;                    /* enum mn_mode */
  int clip_inputs;             /* 1: clip to [2^-23, 1-2^-23] on load (c_segment.pyx:53-55 fused).  For 16-bit
                                  maps (MN_DTYPE_F16 / MN_DTYPE_BF16) the clip on load is ALWAYS on, whatever
                                  this says: neither format holds 1 - 2^-23, and a saturated sigmoid is exactly
                                  1.0 in both (and 0.0 in binary16)                                  */
  int exact_limit;             /* AUTO: images with at most this many initial records go to EXACT right
                                  away (0 = default 32768)                                        */
  int finish_limit;            /* ROUNDS: hand over to the sequential finisher at <= this many
                                  live records (0 = default: 2048 in the rounds, 4096 records
                                  between components in components mode)                         */
  int subrounds;               /* ROUNDS: matching sub-rounds per round (0 = default 32)         */
  float prune_threshold;       /* pysegmenter prune threshold (segmenter.py:351; default 200)    */
  int compute_logprob;         /* 1: also evaluate the total log-likelihood (segment.cc:314-350) and
                                  the certificate; 0: skip both (total_logprob NaN, certified 0)  */
  int no_handover_refresh;     /* ROUNDS: 1 = keep stored priorities when the finisher takes over  */
  int band_permille;           /* ROUNDS: a round merges only records whose gain is >= this many
                                  thousandths of the round's best gain (0 = default 50, <0 = off;
                                  round 1, rounds from single pixels: parity with the reference lost at
                                  10, once in 65 runs at 25, never from 50 up; round 2, rounds from the
                                  cores: 100, 50 and 20 give the same verdict and pixel agreement on
                                  every reference vector, 50 is a fifth faster than 100)            */
  int debug_flags;             /* enum mn_debug_flags, or-ed */
  int require_proof;           /* what happens to a result that is not PROVEN equal to the reference's
                                  sequential order (stats.proof == 0): 1 = it is redone in MN_MODE_EXACT,
                                  whatever mode was asked for, and -- if that run chose among bit-equal
                                  priorities by its own rule (proof 3) -- once more in the reference's order
                                  among equals (tie_order MN_TIES_REFERENCE; MN_ERR_UNPROVEN for the Python
                                  variant, whose heapq order is not restated, with the proof 3 output left in
                                  place; mn_segment_exact_batch applies the same per image); -1 = it is handed back as it is (the
                                  speculative fast path: an approximation on order-dependent inputs,
                                  stats.proof tells); 0 (default) = by mode: AUTO redoes it, an explicit
                                  MN_MODE_ROUNDS / MN_MODE_COMPONENTS request is taken as a request for
                                  that engine's own answer                                          */
  int core_radius;             /* general rounds: an offset counts as SHORT when both its components
                                  are at most this many pixels; a pixel is clean -- and may join a core
                                  ahead of the rounds -- when all its short edges are positive and
                                  same-class (0 = default; < 0 = every offset
                                  is short: the widest fringe, the closest to the reference's order)   */
  int tie_order;               /* MN_MODE_EXACT (and what AUTO redoes by it): who goes first among records with
                                  bit-equal priorities.  MN_TIES_LOWEST_ID: the record created first -- the
                                  exact engine's own rule.  MN_TIES_REFERENCE: what the reference's
                                  std::priority_queue and std::unordered_map (libstdc++, GCC 11: the build the
                                  golden vectors come from) make of it -- binary-heap position and hash-map
                                  iteration order, restated on flat arrays (mn_reforder.h); the maps are worked
                                  by ONE lane, the heap by its wave: the reference's very partition also on
                                  maps with plateaus of equal values, at 20-40x the exact engine's time
                                  (csegment variant only).  MN_TIES_DEFAULT (0): the exact engine first; if it
                                  met tied pops whose choices conflict (stats.tied_conflicts > 0: only then can
                                  the two rules end in different states) and the image has at most
                                  MN_TIE_LIMIT_RECORDS initial records, it is redone in the reference's order;
                                  larger images keep the exact engine's answer and say so (stats.proof == 3,
                                  stats.tie_order_used, stats.tied_steps, stats.tied_conflicts)              */
} mn_options;

typedef struct mn_stats {
  int status;
  int mode_used;               /* MN_MODE_EXACT, MN_MODE_ROUNDS or MN_MODE_COMPONENTS */
  int certified;               /* 1: result proven equal to the sequential reference partition
                                  (sign-separable input, see DESIGN.md "certificate")           */
  int num_instances;           /* labels 1..K written to the mask */
  int num_objects;             /* surviving objects including class-0 ones */
  int rounds;                  /* parallel rounds executed */
  int finisher_steps;          /* sequential steps (pops) executed by the finisher */
  int cert_edge_violations;    /* pixel edges whose log-odds sign contradicts the partition   */
  int cert_class_violations;   /* pixels whose own arg-max class differs from their object's  */
  int cert_record_violations;  /* records between final objects that are still mergeable      */
  long long initial_records;   /* in-bounds (pixel, offset) pairs */
  long long merges;            /* objects absorbed */
  double total_logprob;        /* A.4: sum lp[cls] + omf*(sum log p | log(1-p)); NaN if not asked */
  float ms_score;              /* phase A kernels (class pass + edge pass), HIP events */
  float ms_class_pass;
  float ms_edge_pass;
  float ms_merge;              /* phase B */
  float ms_output;             /* labels, mask, class table, certificate, log-likelihood */
  float ms_total;
  /* components mode only (0 otherwise), HIP events on the launch stream: */
  float ms_cc_label;           /* mn_cc_tiles + borders + flatten + hook: union-find on the 4 B/pixel masks */
  float ms_cc_sums;            /* mn_cc_class_sums: reads the C class planes                            */
  float ms_cc_edges;           /* mn_cc_sign: THE read of the O sameness planes (masks, negative edges)  */
  float ms_cc_cross;           /* mn_cc_cross: negative-edge list -> records between components         */
  int proof;                   /* enum mn_proof: why (and whether) the partition equals the reference's     */
  int cores_condemned;         /* general rounds: 1 if a core held an edge that was not positive and
                                  fell apart again (mn_core_check); 0 otherwise                    */
  int tied_steps;              /* MN_MODE_EXACT: pops at which a second live record held the bit-equal stored
                                  priority (saturates at INT_MAX).  0 = every pop was forced: the result is
                                  the reference's whatever its heap does among equals.  > 0: the reference's
                                  std::priority_queue picks by heap position, the engine by lowest record id;
                                  the two orders usually commute, DESIGN.md section 5 has the inputs where
                                  they do not (radius-4 blurred, clipped maps)                             */
  int tied_merges;             /* ... of which were merges */
  int tie_order_used;          /* MN_MODE_EXACT: MN_TIES_LOWEST_ID or MN_TIES_REFERENCE (0 on the other paths) */
  int tied_conflicts;          /* MN_MODE_EXACT: 0 = no tied pop's choice WROTE an object's state that another tied
                                  choice read or wrote (a merge writes its two ends and reads their neighbours):
                                  the tied events commute and every order among equals ends in this state (then
                                  proof == 2 even with tied_steps > 0); > 0 = at least one did (the engine stops
                                  looking at the first: a yes / no, not a count).  mn_kernels_exact.h "ties"      */
} mn_stats;

typedef struct mn_context mn_context;

/* Fill `o` with the Cityscapes caller's options (egs/cityscape/local/segment.py:134-136):
 * same_different_bias 0, object_merge_factor 1, merge_logprob_bias 0.03, csegment, AUTO. */
void mn_default_options(mn_options* o);

/* Create a context on HIP device `device` able to hold images up to max_height x max_width with
 * up to max_classes class planes and max_offsets offsets.  All device memory is allocated here;
 * mn_segment_device allocates nothing.  Returns NULL on failure (see mn_last_status). */
mn_context* mn_create(int device, int max_height, int max_width, int max_classes, int max_offsets);
void mn_destroy(mn_context* ctx);
size_t mn_workspace_bytes(const mn_context* ctx);

/* Segment one image whose probability maps are ALREADY ON THE DEVICE.
 *   d_class_pred [class_dim][H][W] float32, d_adj_pred [offset_dim][H][W] float32 (C order)
 *   offset_list  HOST pointer, [offset_dim][2] = (d_row, d_col)   (segment.cc:166-169)
 *   d_mask       [H][W] int32 out: 0 = every class-0 object, 1..K instances (segment.cc:491-517)
 *   d_object_class [H*W] int32 out: class of label k at k-1, -1 from index K on
 *   d_partition  optional [H*W] int32 out: surviving object id per pixel before the class-0
 *                collapse (may be NULL)
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  The call enqueues work and
 * synchronises the stream before returning when `stats` is non-NULL or the mode needs host
 * decisions (ROUNDS does, per round).  Inputs are never modified (the reference rewrites
 * adj_pred in place when same_different_bias != 0; here the bias is applied on load). */
int mn_segment_device(mn_context* ctx, const float* d_class_pred, int class_dim,
                      const float* d_adj_pred, int offset_dim, int img_width, int img_height,
                      int num_classes, const int* offset_list, int* d_mask, int* d_object_class,
                      int* d_partition, const mn_options* opts, void* stream, mn_stats* stats);

/* The same in two halves, for callers that keep the GPU busy across images: mn_segment_launch
 * queues one image and returns -- in components mode (the default for large images) without
 * having waited for anything; mn_segment_finish waits, reads the verdict (redoing the image on the
 * ordinary path if the speculative attempt does not hold) and fills `stats`.  Between the two the
 * context is busy and inputs, outputs and stream must stay alive; with two contexts on one stream
 * the launch of image i+1 can precede the finish of image i, which hides the host round trip
 * without letting kernels of different images overlap.  A negative return of mn_segment_launch
 * leaves nothing pending. */
int mn_segment_launch(mn_context* ctx, const float* d_class_pred, int class_dim,
                      const float* d_adj_pred, int offset_dim, int img_width, int img_height,
                      int num_classes, const int* offset_list, int* d_mask, int* d_object_class,
                      int* d_partition, const mn_options* opts, void* stream);
int mn_segment_finish(mn_context* ctx, mn_stats* stats);

/* Tuning aid: the sweep alone, `reps` launches back to back over `n_inputs` input sets in rotation (more than
 * 256 MB of inputs in all keeps the Infinity Cache from serving them); average microseconds per launch. */
int mn_sweep_time_device(mn_context* ctx, const float* const* d_class_pred, const float* const* d_adj_pred,
                         int n_inputs, int class_dim, int offset_dim, int img_width, int img_height,
                         int num_classes, const int* offset_list, const mn_options* opts, void* stream, int reps,
                         float* us_per_launch);

/* `count` images of ONE shape through the exact engine (MN_MODE_EXACT) together: the engine's loop is one
 * wavefront per image, so a batch is ONE launch with a workgroup per image -- images in flight are how the
 * sequential order gets throughput (the reference scales the same way, by processes: --num-jobs).  One
 * context per image (each holds its image's workspace, ~1.5 GB at 512x1024, ~6 GB at 1024x2048); arrays of
 * `count` device pointers (host arrays); d_partition may be NULL; stats: `count` entries or NULL.  The call
 * returns when all images are done.  Results are those of `count` separate MN_MODE_EXACT calls; the images the
 * tie policy sends to the reference-order loop (opts->tie_order; stats.tied_conflicts > 0) are redone TOGETHER,
 * one workgroup per image in one launch of that loop, and up to MN_TIE_LIMIT_BATCH_RECORDS initial records
 * instead of MN_TIE_LIMIT_RECORDS (the loop is sequential: images in flight are its throughput).  With
 * opts->tie_order == MN_TIES_REFERENCE the exact engine is not run at all.
 * opts->require_proof = 1 holds per image as in a single call: after the hand-over, every image that is still
 * proof 3 (no certificate, tied choices that conflict, not redone by the tie policy) is redone in the reference's
 * order, together and whatever its size; stats keep the tied pops the exact engine met.  Where that is not possible
 * (Python variant; MN_ERR_CAPACITY from the loop's workspace) the image's output stays the exact engine's (proof 3),
 * its stats[i].status is MN_ERR_UNPROVEN, the other images are unaffected, and the call returns the first non-OK
 * status. */
int mn_segment_exact_batch(mn_context** ctxs, int count, const float* const* d_class_pred, int class_dim,
                           const float* const* d_adj_pred, int offset_dim, int img_width, int img_height,
                           int num_classes, const int* offset_list, int* const* d_mask,
                           int* const* d_object_class, int* const* d_partition, const mn_options* opts,
                           void* stream, mn_stats* stats);

/* Phase A alone (per-pixel class log-probs + argmax, per-edge log-odds and initial priorities,
 * best initial record per pixel).  Used by bench.py / profiles to time the affinity-scoring pass
 * against the HBM roofline, and by tests to compare phase-A arrays with the oracle.
 *   d_cls_out   [H*W] uint8  argmax class per pixel                     (segment.cc:18-20)
 *   d_best_out  [H*W] uint64 (priority bits << 32 | ~partner pixel id), 0 = no record >= 0 */
int mn_score_device(mn_context* ctx, const float* d_class_pred, int class_dim,
                    const float* d_adj_pred, int offset_dim, int img_width, int img_height,
                    int num_classes, const int* offset_list, const mn_options* opts, void* stream,
                    unsigned char* d_cls_out, unsigned long long* d_best_out, float* ms_class_pass,
                    float* ms_edge_pass);

/* The affinity-scoring sweep of the default path alone (mn_cc_sign: ONE read of the C class planes and the
 * O sameness planes) and what it leaves behind, for the parity test of the sweep itself against the
 * oracle's phase A (segment.cc:5-46):
 *   d_bits_out [H*W] uint32   bit k = out-edge of offset k is in bounds and positive (value >= sep_hi)
 *   d_neg_out  [O][H*W] f32   log-odds of every NEGATIVE in-bounds edge the sweep listed, NaN elsewhere
 *   d_cls_out  [H*W] uint8    per-pixel arg-max class            (only written in the fused-class form)
 *   d_gsum_out [C][H*W/4] i32 per lane and class the 2^-24 fixed-point log of the product of its four
 *                             pixels' class values             (only written in the fused-class form)
 *   logsum_out (host)         the certificate's sum over in-bounds edges of log max(v, 1 - v)
 *   info_out   (host) int[3]  {pixels per lane (4 | 1), fused-class form (1 | 0), edges inside the
 *                             float32 rounding margin of 0.5 (they fail the separability check)}
 * d_cls_out / d_gsum_out may be NULL.  Synchronises. */
int mn_sweep_device(mn_context* ctx, const float* d_class_pred, int class_dim, const float* d_adj_pred,
                    int offset_dim, int img_width, int img_height, int num_classes, const int* offset_list,
                    const mn_options* opts, void* stream, unsigned* d_bits_out, float* d_neg_out,
                    unsigned char* d_cls_out, int* d_gsum_out, double* logsum_out, int* info_out);

/* Phase A of the exact engine alone (tests pin it against the oracle, bit for bit): per record the
 * float32 log-odds obj_merge_logprob (segment.cc:33-36: logf and a double log, as glibc computes them)
 * and the initial merge priority (segment.cc:107-150), laid out [offset][source pixel] with NaN where
 * the edge leaves the image; d_cls_out [H*W] uint8 arg-max class (may be NULL).  Synchronises. */
int mn_exact_phase_a_device(mn_context* ctx, const float* d_class_pred, int class_dim,
                            const float* d_adj_pred, int offset_dim, int img_width, int img_height,
                            int num_classes, const int* offset_list, const mn_options* opts, void* stream,
                            unsigned char* d_cls_out, float* d_oml_out, float* d_prio_out);

/* ---- 16-bit probability maps -------------------------------------------------------------------------
 * The *_t entry points take the maps as untyped device pointers plus their element type, `int dtype` (enum
 * mn_dtype): float32, IEEE binary16 or bfloat16, the width the network wrote them in -- no float32 copy is
 * made anywhere.  ARGUMENT ORDER: that of the float entry point, with `int dtype` right after the group of the
 * two map pointers (d_class_pred, class_dim, d_adj_pred, offset_dim, DTYPE, img_width, ...; where the two
 * pointers are adjacent -- mn_sweep_time_device_t -- right after them); mn_prepare_device_t has one dtype
 * behind each of its two pointers.  Both maps of a call share the dtype.  An unknown dtype is MN_ERR_ARGUMENT.
 * Every kernel widens on load (exact) and computes in float32, so a call on 16-bit maps gives what the float
 * entry point gives on the same values widened to float32 with clip_inputs = 1 (see mn_options.clip_inputs:
 * a 16-bit map is always clipped on load; same_different_bias is applied after widening).  The sweep takes 8
 * pixels per lane where N % 8 == 0, W % 8 == 0 and the planes are 16-byte aligned (info_out[0] of
 * mn_sweep_device_t is then 8), which regroups the float products behind total_logprob / logsum_out: those
 * agree to rounding (1e-5 relative), everything else bit for bit.  The float entry points are one-line calls
 * of these with MN_DTYPE_F32; mn_segment_finish serves both.  c_run_segmentation and mn_segment_host stay
 * float32 only.
 *
 * LOGITS.  The reference's two networks emit logits and put a sigmoid behind them (utils/inference_utils.py:
 * 44,96).  MN_MAPS_LOGITS or-ed into `dtype` (the low byte stays the element type) says that BOTH maps of the
 * call hold logits: every kernel then takes p = 1.0f / (1.0f + expf(-(float)x)) where it loads an element, in
 * float32 after the exact widening, and no probability copy of the maps is made.  The call gives bit for bit
 * what it gives on those p as float32 maps with clip_inputs = 1 -- what mn_prepare_device_t(..., apply_sigmoid
 * = 1, clip = 0) writes at unchanged size -- with the one regrouping above where 16-bit logits take 8 pixels
 * per lane (the rule looks at the element type only).  Logits are ALWAYS clipped on load, whatever clip_inputs
 * says: the float32 sigmoid is exactly 1.0 from about 17 up and 0 below about -104.  +-inf are legal logits,
 * NaN is undefined as for probabilities.  same_different_bias is applied to the probability, as ever.  A
 * 16-bit logit keeps a distinct probability per distinct logit up to about 17, where a 16-bit probability
 * above 0.5 has 128 (bfloat16) values and is 1.0 from a logit of about 5.5.  The seven entry points below
 * this line and above mn_prepare_device_t take the flag; mn_prepare_device_t has apply_sigmoid of its own and
 * refuses it in either dtype (MN_ERR_ARGUMENT), the float entry points stay probabilities only. */
#define MN_MAPS_LOGITS 0x100
int mn_segment_device_t(mn_context* ctx, const void* d_class_pred, int class_dim, const void* d_adj_pred,
                        int offset_dim, int dtype, int img_width, int img_height, int num_classes,
                        const int* offset_list, int* d_mask, int* d_object_class, int* d_partition,
                        const mn_options* opts, void* stream, mn_stats* stats);
int mn_segment_launch_t(mn_context* ctx, const void* d_class_pred, int class_dim, const void* d_adj_pred,
                        int offset_dim, int dtype, int img_width, int img_height, int num_classes,
                        const int* offset_list, int* d_mask, int* d_object_class, int* d_partition,
                        const mn_options* opts, void* stream);
int mn_segment_exact_batch_t(mn_context** ctxs, int count, const void* const* d_class_pred, int class_dim,
                             const void* const* d_adj_pred, int offset_dim, int dtype, int img_width,
                             int img_height, int num_classes, const int* offset_list, int* const* d_mask,
                             int* const* d_object_class, int* const* d_partition, const mn_options* opts,
                             void* stream, mn_stats* stats);
int mn_score_device_t(mn_context* ctx, const void* d_class_pred, int class_dim, const void* d_adj_pred,
                      int offset_dim, int dtype, int img_width, int img_height, int num_classes,
                      const int* offset_list, const mn_options* opts, void* stream, unsigned char* d_cls_out,
                      unsigned long long* d_best_out, float* ms_class_pass, float* ms_edge_pass);
int mn_sweep_device_t(mn_context* ctx, const void* d_class_pred, int class_dim, const void* d_adj_pred,
                      int offset_dim, int dtype, int img_width, int img_height, int num_classes,
                      const int* offset_list, const mn_options* opts, void* stream, unsigned* d_bits_out,
                      float* d_neg_out, unsigned char* d_cls_out, int* d_gsum_out, double* logsum_out,
                      int* info_out);   /* info_out[0]: pixels per lane, 8 | 4 | 1 */
int mn_sweep_time_device_t(mn_context* ctx, const void* const* d_class_pred, const void* const* d_adj_pred,
                           int dtype, int n_inputs, int class_dim, int offset_dim, int img_width, int img_height,
                           int num_classes, const int* offset_list, const mn_options* opts, void* stream,
                           int reps, float* us_per_launch);
int mn_exact_phase_a_device_t(mn_context* ctx, const void* d_class_pred, int class_dim, const void* d_adj_pred,
                              int offset_dim, int dtype, int img_width, int img_height, int num_classes,
                              const int* offset_list, const mn_options* opts, void* stream,
                              unsigned char* d_cls_out, float* d_oml_out, float* d_prio_out);
/* mn_prepare_device with typed ends: d_in holds in_dtype elements, d_out out_dtype elements; the arithmetic is
 * float32 and a 16-bit output is that float32 value rounded to nearest even. */
int mn_prepare_device_t(mn_context* ctx, const void* d_in, int in_dtype, int channels, int in_height,
                        int in_width, void* d_out, int out_dtype, int out_height, int out_width,
                        int apply_sigmoid, int clip, void* stream);

/* Host-pointer convenience: copies in, runs mn_segment_device, copies out. */
int mn_segment_host(mn_context* ctx, const float* class_pred, int class_dim, const float* adj_pred,
                    int offset_dim, int img_width, int img_height, int num_classes,
                    const int* offset_list, int* mask, int* object_class, int* partition,
                    const mn_options* opts, mn_stats* stats);

/* ABI-compatible replacement of the reference entry point (utils/csegment/segment.cc:742-754).
 * Width precedes height.  Host pointers; inputs must already be clipped as the reference binding
 * does (c_segment.pyx:53-55).  Unlike the reference it does not rewrite adj_pred. */
void c_run_segmentation(float* class_pred, int class_dim, float* adj_pred, int offset_dim,
                        int img_width, int img_height, int num_classes, int* offset_list,
                        int* output, int* object_class, float same_different_bias,
                        float object_merge_factor, float merge_logprob_bias);

/* Producer hand-off on the device ("next" row 1 of the scope table): logits or probabilities
 * [channels][in_h][in_w] -> probabilities [channels][out_h][out_w] in ONE pass: optional sigmoid
 * (utils/inference_utils.py:44,96), bilinear resize with cv2.resize/INTER_LINEAR coordinates
 * (egs/cityscape/local/segment.py:115-123) and the binding's clip (c_segment.pyx:53-55).  Replaces
 * the .npy round trip between the network and the merger. */
int mn_prepare_device(mn_context* ctx, const float* d_in, int channels, int in_height, int in_width,
                      float* d_out, int out_height, int out_width, int apply_sigmoid, int clip,
                      void* stream);

/* Class maps from a TILED semantic network, assembled on the device.  The production recipe's class maps do not
 * come from a sigmoid network but from a Cn-class semantic network run by tile_predict (models/pspnet_caffe.py:
 * 492-560, switched on in egs/cityscape/local/class_infer.py:58-64): overlapping tiles, each run plain and
 * horizontally flipped, softmax, the two passes averaged, the "stuff" classes folded into one background plane by a
 * maximum, the tiles summed into the image, divided by a per-pixel cover count and renormalised -- in numpy on the
 * host, with a .cpu() and a .cuda() per tile.  Here ONE gather kernel reads every tile logit once and writes the C
 * planes of the image: no atomics, no scratch buffer, no second launch.
 *   d_tiles       [T][net_classes][tile_height][tile_width], contiguous, elements of `dtype` (MN_DTYPE_*, widened
 *                 exactly on load): the network's LOGITS for tile t = i * num_cols + j, whose top-left pixel is
 *                 (row_starts[i], col_starts[j]) -- the reference's loop order, rows outer
 *   d_flip_tiles  the same shape, or NULL: the network's logits on the horizontally flipped slice, as they come
 *                 out (not flipped back)
 *   row_starts [num_rows], col_starts [num_cols]   HOST arrays; duplicates are legal (the reference's geometry
 *                 gives {0, 0, 0} where the image is exactly one tile high); they travel as kernel arguments
 *   num_classes   C, the planes written, 1 <= C <= net_classes (Cn); the first Cn - C + 1 network classes are the
 *                 stuff classes
 * float32 arithmetic throughout.  Per tile pixel: p1 = softmax over the Cn logits, as expf(x - max) / sum; with a
 * flip tensor p2 the same at tile column tile_width - 1 - x and p = (p1 + p2) * 0.5f, else p = p1; q[0] = the maximum
 * of p over the stuff classes (taken AFTER the average: not simply the probability of the greatest logit), q[k] =
 * p[Cn - C + k] for k = 1..C-1.  Per image pixel: acc[k] = the sum of q[k] over the covering tiles in ascending t,
 * s[k] = acc[k] / (float)count, out[k] = s[k] / (s[0] + ... + s[C-1]) summed in ascending k; with clip != 0 the
 * merger's clip to [2^-23, 1 - 2^-23] comes last.  d_out is [C][img_height][img_width] of out_dtype, a 16-bit
 * output being the float32 value rounded to nearest even.  NaN and +-inf logits are undefined.
 * Any image size (not held to the context's capacity).  MN_ERR_ARGUMENT, with nothing launched: a null pointer other
 * than d_flip_tiles, a non-positive size, num_rows or num_cols > 32, net_classes > 64, num_classes outside 1..Cn, a
 * tile that leaves the image, a row or column of the image that no start covers, an unknown dtype, MN_MAPS_LOGITS in
 * either dtype (the tiles are logits by definition).  Enqueues only: no host synchronisation, no copies. */
int mn_tile_class_maps_device(mn_context* ctx, const void* d_tiles, const void* d_flip_tiles, int dtype,
                              int net_classes, int tile_height, int tile_width,
                              const int* row_starts, int num_rows, const int* col_starts, int num_cols,
                              int img_height, int img_width, int num_classes,
                              void* d_out, int out_dtype, int clip, void* stream);

/* Nearest-neighbour resize of the instance mask back to the image size, cv2 INTER_NEAREST
 * coordinates (egs/cityscape/local/segment.py:146-149), as OpenCV's portable resizeNN forms them, in double:
 * source index = min(floor(dst * (1. / ((double)dst_size / src_size))), src_size - 1), per axis.  That is neither
 * the float32 index of torch's mode="nearest" nor the rational floor (dst * src_size) / dst_size: 8 -> 82 differs
 * from the first at dst 41, 8 -> 98 from the second at dst 49.  mergenet_amd/labels.py::nearest_index is the numpy
 * statement.  Any sizes, growing or shrinking; out_height <= 65535. */
int mn_upsample_mask_device(mn_context* ctx, const int* d_mask, int in_height, int in_width,
                            int* d_out, int out_height, int out_width, void* stream);

/* Run boundaries of ALL instances in one pass, for COCO RLE (egs/cityscape/local/segment.py:
 * 165-186 encodes each instance with pycocotools over the Fortran-ordered binary mask).  The
 * label scan runs column-major; d_points gets [positions | label before | label at] with stride
 * `capacity`, *count the number of change points.  The host groups them per label. */
int mn_rle_points_device(mn_context* ctx, const int* d_mask, int height, int width, int* d_points,
                         int capacity, int* count, void* stream);

/* HOST helper of the RLE path: groups the change points of mn_rle_points_device per instance and
 * writes pycocotools' compressed counts strings (egs/cityscape/local/segment.py:165-186: one
 * maskUtils.encode per instance), in native code (the Python loop it replaces took 2.8 ms for 21
 * instances).  points = [positions | label before | label at] with stride `capacity` (host copy of
 * d_points), n of them.  Strings are concatenated into `out` (string k-1 = out[offsets[k-1] ..
 * offsets[k]) ), areas[k-1] = pixels of instance k (0 => the caller may drop it, as
 * egs/cityscape/local/evaluate.py:52-54 does).  A label outside 1..num_instances in the mask (a negative
 * ignore label, a label above the count) is ignored: it gets no string and counts as zeros in the strings of
 * the others, as `mask == k` does.  Returns the bytes needed; nothing is written past out_capacity.  Needs no GPU. */
long long mn_rle_encode_host(const int* points, int capacity, int n, int height, int width,
                             int num_instances, unsigned char* out, long long out_capacity,
                             long long* offsets, int* areas);

/* The decoding half of the RLE path: COCO run-length encodings back into ONE int32 label mask, what anns_to_mask
 * and anns_to_mask_class build on the host (utils/dataset.py:486-522: one maskUtils.decode per annotation, painted
 * in list order with mask = m * (mask == 0) + mask) and what mn_overlap_table_device, mn_map_scores_device and
 * mn_sameness_targets_device take as the ground truth.  mergenet_amd/rle.py::label_mask is the numpy statement.
 *
 * mn_rle_counts_host (HOST, needs no GPU): unpacks pycocotools' compressed counts string -- 5-bit groups, low
 * group first, 0x20 = more groups follow, 0x10 of the last group = sign, offset 48; from the fourth count on the
 * value is the difference to the count two places earlier.  Writes counts[0 .. min(n, capacity)) and returns n,
 * the number of counts in the string (nothing is written past `capacity`); *total (may be NULL) = their sum.
 * Negative returns: MN_ERR_ARGUMENT for a string that ends inside a group, a byte outside '0'..'o' or a count that
 * comes out negative; MN_ERR_CAPACITY for a count that does not fit 31 bits. */
long long mn_rle_counts_host(const unsigned char* s, long long len, unsigned* counts, long long capacity,
                             long long* total);

/* mn_rle_decode_device: all pointers are device memory.
 *   d_counts   uint32 [num_counts]: the counts of all annotations, concatenated; the counts of one annotation are
 *              the lengths of alternating runs of its binary mask in COLUMN-major order, the first run zeros;
 *   d_starts   int32 [A + 1], CSR: annotation a owns d_counts[d_starts[a] .. d_starts[a + 1]);
 *   d_values   int32 [A] or NULL: annotation a paints d_values[a], or a + 1; the value 0 paints nothing;
 *   d_mask     int32 [height][width], row-major, written completely (zeros included: it needs no clearing):
 *              a pixel holds the value of the first annotation in list order with a nonzero value that covers it;
 *   d_area     int32 [A] or NULL: the sum of a's odd-indexed counts (maskUtils.area), visible or not;
 *   scratch of the call, the caller's: d_scratch_ends uint32 [num_counts] (4 bytes per count) and
 *              d_scratch_records int32 [A][MN_RLE_RECORD_INTS] (16 bytes per annotation, 16-byte aligned).
 * Zero-length runs are legal anywhere.  The counts of an annotation should sum to height * width; whatever they
 * hold, every run end is clamped to height * width and no scan position forms an address (a d_starts entry is
 * held to 0..num_counts), and every loop is bounded by num_counts.  Two launches (one when A == 0, which writes
 * zeros); integer work only, bit-identical from run to run.  Any image size with height * width < 2^31 (not held
 * to the context's capacity); A <= MN_RLE_MAX_ANNOTATIONS (the reference's mask is uint16).  MN_ERR_ARGUMENT: a
 * null pointer that is needed, a non-positive size, a negative count, A above the limit.
 * Enqueues only: no allocation, no copy, no host synchronisation. */
#define MN_RLE_MAX_ANNOTATIONS 65535
#define MN_RLE_RECORD_INTS 4
int mn_rle_decode_device(mn_context* ctx, const unsigned* d_counts, const int* d_starts, int num_annotations,
                         int num_counts, const int* d_values, int height, int width, unsigned* d_scratch_ends,
                         int* d_scratch_records, int* d_mask, int* d_area, void* stream);

/* Sameness targets of an instance mask: out[k][r][c] = (mask[r+di][c+dj] == mask[r][c]), 1 outside
 * the image (utils/dataset.py:259-277).  d_out is float32 [offset_dim][H][W]. */
int mn_sameness_targets_device(mn_context* ctx, const int* d_mask, int height, int width,
                               const int* offset_list, int offset_dim, float* d_out, void* stream);

/* Confidence of the instances of the last segmentation on this context (mn_segment_device, mn_segment_finish, the
 * context's image of mn_segment_exact_batch): d_scores[k-1] = lp[cls] - lp[0] of label k (segment.h:109), for the
 * labels 1..num_instances of that call; words of d_scores behind them, and all of them when it found no instance,
 * are not written.  The reference's COCO results carry a constant score 1.
 *
 * Contract: the call gives the scores of the last segmentation on this context, or it refuses -- never a third
 * thing.  It computes nothing from the maps: it reads what that segmentation left in the context (the sums of the
 * objects; for a single-pixel instance the caller's class maps, which must still be alive and unchanged).  It
 * refuses with MN_ERR_ARGUMENT, launching nothing, on a context that has not segmented yet, whose last
 * segmentation failed after its first launch, that has an unfinished mn_segment_launch, or on which one of
 * mn_score_device, mn_sweep_device, mn_sweep_time_device or mn_exact_phase_a_device ran since: those overwrite the
 * state.  A call that is rejected for its arguments before anything ran, and every other entry point (resize, RLE,
 * tables, matching, evaluation, map scores, criteria, wires, tiles), leaves the scores available. */
int mn_instance_scores_device(mn_context* ctx, float* d_scores, void* stream);

/* Instance table of a label mask (labels 0..num_instances, 0 = background): what a detection result needs per
 * instance beside its RLE.  The reference's caller ends in convert_to_coco_result (egs/cityscape/local/
 * segment.py:165-186) and leaves area and box to COCO.loadRes, which derives them from every RLE on the host;
 * here ONE pass over the mask gives them for all instances.
 * d_table int32 [num_instances][5] = {area, x_min, y_min, x_max, y_max}, maxima inclusive; a label without
 * pixels keeps the empty row {0, W, H, -1, -1} (the identities of sum, min and max over the image).  Labels
 * outside 1..num_instances in the mask are ignored.  Any image size (not held to the context's capacity, as in
 * mn_upsample_mask_device: the table is most wanted on the upsampled mask); 16-byte loads where width % 4 == 0
 * and d_mask is 16-byte aligned, 4-byte loads otherwise.  num_instances == 0 is legal (nothing written).
 * Enqueues only: no host synchronisation, no copies. */
int mn_instance_table_device(mn_context* ctx, const int* d_mask, int height, int width,
                             int num_instances, int* d_table, void* stream);

/* Drop instances with area < min_area (or score < min_score when d_scores != NULL) and renumber the
 * survivors 1..K' in ascending old label: the evaluator's zero-area drop with a threshold
 * (egs/cityscape/local/evaluate.py:52-54; such instances arise when the mask is resized back with
 * nearest-neighbour), done so that mask, class table, scores and instance table still agree afterwards.
 * d_table: what mn_instance_table_device wrote for d_mask.  d_remap int32 [num_instances+1] out (old -> new,
 * 0 = dropped; d_remap[0] = 0); d_mask_out may equal d_mask (labels outside 0..num_instances become 0);
 * the *_out arrays have num_instances entries and must not be their inputs (MN_ERR_ARGUMENT): rows / entries 0..K'-1 are
 * the survivors', d_object_class_out is -1 from K' up to num_instances (the library's convention), the rest of
 * d_table_out and d_scores_out is not written; d_scores_out is needed only with d_scores; d_new_count: one
 * device int, K'.  A NaN score fails the comparison: with d_scores given it is dropped whatever min_score is
 * (-INFINITY keeps every other score).  Any image size, any num_instances >= 0.  Enqueues only. */
int mn_filter_instances_device(mn_context* ctx, const int* d_mask, int height, int width, int num_instances,
                               const int* d_table, const int* d_object_class, const float* d_scores,
                               int min_area, float min_score, int* d_mask_out, int* d_remap,
                               int* d_table_out, int* d_object_class_out, float* d_scores_out,
                               int* d_new_count, void* stream);

/* A label mask against the ground-truth label mask, on the device.  The reference's caller ends by handing its
 * results to COCOeval (egs/cityscape/local/evaluate.py:67-73), which computes per image the IoU of every detection
 * with every ground-truth instance and matches greedily once per IoU threshold; the ground truth is the label mask
 * anns_to_mask builds (utils/dataset.py:486-506), what mn_sameness_targets_device takes.  The two calls below are
 * that per-image part; the mn_eval_* calls behind them are the dataset-level part (accumulate); the annotation
 * files stay on the host, and summarize is a few means of the accumulated arrays, taken there too.
 *
 * mn_overlap_table_device: d_table int32 [num_pred + 1][num_truth + 1], row-major; table[p][g] = number of pixels
 * with prediction label p and truth label g (p in 0..K, g in 0..G).  A label outside its range (negative, above K
 * or above G) counts as 0 in either mask.  Row 0 and column 0 are kept: row sums are the prediction areas, column
 * sums the truth areas, all entries sum to height * width.  ONE pass over both masks: 16-byte loads where
 * width % 4 == 0 and BOTH masks are 16-byte aligned, 4-byte loads otherwise.  Any image size (not held to the
 * context's capacity); K == 0 and G == 0 are legal.  MN_ERR_ARGUMENT: a null pointer, a non-positive size,
 * height * width > INT_MAX, a negative count, (K + 1) * (G + 1) > 2^28.  The call clears the table on `stream`
 * and launches; it only enqueues: no host synchronisation, no copies. */
int mn_overlap_table_device(mn_context* ctx, const int* d_pred, const int* d_truth,
                            int height, int width, int num_pred, int num_truth,
                            int* d_table, void* stream);

/* IoU and matching from that table: COCOeval.evaluateImg with maxDets >= K, for all thresholds at once.
 * Arrays per instance are indexed label - 1.  With area_p[k] the sum of row k and area_g[j] the sum of column j:
 *   iou[k][j] = table[k][j] / (area_p[k] + area_g[j] - table[k][j]); for a crowd truth instance table[k][j] /
 *   area_p[k]; 0 where the denominator is 0.  float64, ONE IEEE division of exact integers.
 *   truth_ignore[j] = crowd[j] || area_g[j] < area_lo || area_g[j] > area_hi.
 *   Order: detections by descending score, equal scores in ascending label, a NaN score last; in label order
 *   without scores.  Truth instances: the non-ignored, then the ignored, each group in ascending label.
 *   Per threshold t and detection d in that order, with lo = min(t, 1 - 1e-10): the candidates are the truth
 *   instances of d's class that are unmatched at this t or crowd and have iou[d][j] >= lo.  d takes the
 *   non-ignored candidate of greatest IoU if there is one, else the ignored candidate of greatest IoU; among equal
 *   IoUs the LAST in truth order (the greatest label of the group).  On a match with m: pred_match[t][d] = m (a
 *   truth label 1..G), truth_match[t][m] = d (a prediction label; a crowd instance keeps the last d),
 *   pred_ignore[t][d] = truth_ignore[m].  A detection without a match is ignored iff area_p[d] < area_lo or
 *   area_p[d] > area_hi.  Unmatched entries are 0.
 * thresholds: HOST array of num_thresholds (1..16) values; they travel as kernel arguments.  d_pred_score and
 * d_truth_crowd may be NULL (label order; no crowd), d_iou ([K][G]) and d_truth_ignore ([G]) too (not wanted).
 * d_pred_match, d_pred_ignore: [T][K]; d_truth_match: [T][G].  K, G <= MN_MATCH_MAX_INSTANCES, else
 * MN_ERR_CAPACITY; with K == 0 or G == 0 there is nothing to match and every output is zero.  Calls on one context
 * share its scratch (allocated by the first call): keep them on one stream.  Enqueues only. */
#define MN_MATCH_MAX_INSTANCES 4096
int mn_match_overlaps_device(mn_context* ctx, const int* d_table, int num_pred, int num_truth,
                              const int* d_pred_class, const float* d_pred_score,
                              const int* d_truth_class, const unsigned char* d_truth_crowd,
                              const double* thresholds, int num_thresholds,
                              double area_lo, double area_hi,
                              double* d_iou, int* d_pred_match, int* d_truth_match,
                              unsigned char* d_pred_ignore, unsigned char* d_truth_ignore, void* stream);

/* The dataset-level half: COCOeval.accumulate over a log of detections that lives on the device.  The caller owns
 * the log -- num_records records of MN_EVAL_RECORD_BYTES, 16-byte aligned -- and its fill: an append of an image
 * writes exactly num_pred records, so the host knows where the next image goes without asking the device.  There is
 * no cursor on the device, no overflow state, and nothing here synchronises.  The contract is pinned to the numpy
 * statement (labels.eval_records, labels.coco_accumulate) and hand-computed cases; pycocotools is not a dependency.
 *
 * A record (eight 32-bit words): class, score (float32 bits; 1.0 without scores), rank, image ordinal, then two
 * 64-bit words, low half first: matched and ignored, bit a * T + t for area range a and threshold t.
 *
 * mn_eval_append_device, one image; the inputs are those of mn_match_overlaps_device:
 *   1. detection order: descending score, equal scores in ascending label, a NaN score last; label order without
 *      scores.  rank[d] = number of detections of d's class before d in that order.
 *   2. a detection with rank >= max_det (the largest maxDets) takes no part in the matching: it matches nothing and
 *      holds no truth instance (COCOeval cuts to dt[:maxDet] per image and category before it matches).
 *   3. per area range a (area_ranges: HOST array of num_areas {lo, hi} pairs, 1..MN_EVAL_MAX_AREAS): the matching of
 *      mn_match_overlaps_device over the remaining detections, truth_ignore_a[j] = crowd[j] || area_g[j] outside
 *      range a; a detection without a match -- those of 2 included -- is ignored iff its own area is outside range a.
 *   4. d_records receives num_pred records in detection order; a class outside 0..num_classes-1 (the library's -1
 *      included) is recorded as it is and never selected.
 *   5. d_npig (int64 [num_classes][num_areas], a running total the caller zeroes once): += the number of truth
 *      instances of each class in 0..num_classes-1 that range a does not ignore.
 *   num_thresholds * num_areas <= 64; K, G <= MN_MATCH_MAX_INSTANCES (MN_ERR_CAPACITY); K == 0 and G == 0 are legal.
 *   Shares the context's scratch with mn_match_overlaps_device: one stream for all of them.  Enqueues only.
 *
 * mn_eval_keys_device: d_keys int64 [num_records], class << 32 | a 32-bit key that ascends as the score DESCENDS,
 *   NaN last, equal scores equal keys; classes outside 0..num_classes-1 read as num_classes.  A STABLE ascending
 *   sort of the keys (any; the Python side takes torch's) gives d_sorted_keys and d_sorted_index (int64, the
 *   permutation) for:
 * mn_eval_accumulate_device: for every class k, range a, max_dets[m] (HOST array, 1..MN_EVAL_MAX_DETS ascending
 *   positive values) and threshold t, over the records of class k with rank < max_dets[m] in sorted order (nd of them):
 *     tp = cumsum(matched & ~ignored), fp = cumsum(~matched & ~ignored), rc = tp / npig[k][a],
 *     pr = tp / (fp + tp + DBL_EPSILON), pr[i] = max(pr[i:]); per recall threshold r (d_rec_thresholds: DEVICE
 *     float64 [R], compared as they are) pi = first i with rc[i] >= threshold: precision[t][r][k][a][m] = pr[pi],
 *     scores[...] = score[pi] if there is one, else both 0; recall[t][k][a][m] = rc[nd-1], 0 if nd == 0; where
 *     npig[k][a] == 0 every entry of (k, a) is -1.  All float64, each division ONE IEEE division of exact integers.
 *   Every entry of the three arrays is written exactly once per call.  num_records == 0 is legal (the three sorted
 *   pointers may then be NULL).  Enqueues only; the sort between the two calls is the caller's. */
#define MN_EVAL_RECORD_BYTES 32
#define MN_EVAL_MAX_AREAS 4
#define MN_EVAL_MAX_DETS 4
#define MN_EVAL_CHUNK 256          /* records the accumulate pass scans per step (tests place segment lengths around it) */
int mn_eval_append_device(mn_context* ctx, const int* d_table, int num_pred, int num_truth,
                          const int* d_pred_class, const float* d_pred_score,
                          const int* d_truth_class, const unsigned char* d_truth_crowd,
                          const double* thresholds, int num_thresholds,
                          const double* area_ranges, int num_areas, int max_det, int num_classes,
                          int image, void* d_records, long long* d_npig, void* stream);
int mn_eval_keys_device(mn_context* ctx, const void* d_records, long long num_records, int num_classes,
                        long long* d_keys, void* stream);
int mn_eval_accumulate_device(mn_context* ctx, const void* d_records, long long num_records,
                              const long long* d_sorted_keys, const long long* d_sorted_index,
                              const long long* d_npig, int num_classes, int num_thresholds,
                              const double* d_rec_thresholds, int num_rec_thresholds, int num_areas,
                              const int* max_dets, int num_max_dets,
                              double* d_precision, double* d_recall, double* d_scores, void* stream);

/* The network's maps themselves against the ground truth, on the device.  The reference scores both networks in
 * every validation pass (runningScore and offsetIoU of utils/score.py:20-32,77-86, driven from utils/train_utils.py:
 * 84-121,183-219 and utils/inference_utils.py:46-47,98-99): it argmaxes the class planes into a confusion matrix
 * and, per offset, forms the soft intersection and union of "different instance" between prediction and target --
 * after copying every plane of every image to the host, one `.cpu()` per offset, and after materialising the
 * targets of utils/dataset.py:259-277.  Here ONE pass reads each map element once, in the layout and element types
 * the sweep reads (`dtype`: MN_DTYPE_*, | MN_MAPS_LOGITS for logits), and looks the truth up in the label mask that
 * mn_sameness_targets_device and mn_overlap_table_device take; no target plane is written.
 *   p: the element widened exactly to float32; for logits 1.0f / (1.0f + expf(-x)) of that, in float32.  No clip and
 *   no same_different_bias: this scores the network, not the merger's view of it.
 *   Predicted class of a pixel: the LOWEST index among the greatest p over the num_classes class planes (numpy's
 *   argmax; it is taken on p, so logits of 18, 20 and 25 -- all exactly 1.0 as float32 probabilities -- tie).
 *   NaN in a map is undefined, as for every other entry point (the running maximum here never takes one, numpy's
 *   argmax takes the first).
 *   Truth class of a pixel: 0 for truth label 0, d_truth_classes[g - 1] for label g in 1..num_truth; a label outside
 *   0..num_truth reads as 0, as in mn_overlap_table_device.  A pixel whose truth class lies outside 0..C-1 is left
 *   out of the confusion matrix (the mask of runningScore._fast_hist: an ignore class for the caller).
 *   d_confusion int64 [C][C], row-major: confusion[t][q] = number of the remaining pixels with truth class t and
 *   predicted class q.
 *   Per offset k = (di, dj): a pixel (r, c) is DIFFERENT when (r + di, c + dj) is inside the image and carries another
 *   truth label -- the labels as they stand in the mask, the rule of mn_sameness_targets_device; a neighbour outside
 *   the image is "same".  With d = 1.0f - p of plane k, in float32 (the reference's 1 - pred):
 *     d_sums[0 * O + k] = sum of d over the different pixels     (the reference's intersection)
 *     d_sums[1 * O + k] = sum of d over all pixels
 *     d_sums[2 * O + k] = the number of different pixels
 *   each summed in float64; the reference's union is sums[1] + sums[2] - sums[0].  d_sums is float64 [3][O].
 * The sums of a call are bit-identical from run to run: no floating-point atomic is used, every workgroup writes its
 * partial sums to its own slot of a buffer of the context and a second launch adds the slots in a fixed order; the
 * grid follows (height, width, element type) only.  accumulate != 0: the counts and the image's three totals per
 * offset are ADDED to what d_confusion / d_sums hold (one IEEE addition per total) -- the running totals of a
 * validation loop, with no synchronisation between images; accumulate == 0: they are stored.
 * Loads: 4 pixels per lane and 16-byte load for float32, 8 for 16-bit maps, where the width is a multiple of that
 * and BOTH maps are 16-byte aligned; 4 per lane and 8-byte load for 16-bit maps of width % 4 == 0 aligned to 8;
 * single elements otherwise.  The truth mask is read through the cache, offset_dim + 1 times and more.
 * Any image size (not held to the context's capacity).  1 <= num_classes <= MN_MAX_CLASSES (class_dim >= num_classes
 * is accepted and not used: the planes are height * width apart), 1 <= offset_dim <= MN_MAX_OFFSETS, num_truth >= 0;
 * d_truth_classes may be NULL when num_truth == 0.  offset_list is a HOST array of (di, dj) pairs, any values, (0, 0)
 * and duplicates included.  MN_ERR_ARGUMENT: a null pointer, a non-positive size, height * width > INT_MAX, img_width
 * > 2^30, a count out of range, an unknown dtype; nothing is launched then.  Calls on one context share its partials buffer
 * (allocated by the first call): keep them on one stream.  Enqueues on `stream` only: no host synchronisation. */
int mn_map_scores_device(mn_context* ctx, const void* d_class_pred, int class_dim, const void* d_adj_pred,
                         int offset_dim, int dtype /* MN_DTYPE_* | MN_MAPS_LOGITS */, int img_width, int img_height,
                         int num_classes, const int* offset_list, const int* d_truth, int num_truth,
                         const int* d_truth_classes, long long* d_confusion /* [C*C] */,
                         double* d_sums /* [3*O] */, int accumulate, void* stream);

/* The training criterion from the label mask, on the device: loss and gradient in one pass.  Every recipe of the
 * reference trains both parts of the network's output with torch.nn.BCEWithLogitsLoss against target planes
 * (egs/cityscape/local/train.py:183-195, egs/coco/local/train.py:145,156; cls_loss + alpha * ofs_loss and its backward
 * pass in utils/train_utils.py:42-79,145-180; the targets of utils/dataset.py:259-277 and :419-429).  Here ONE pass
 * reads each logit once, looks its target up in the label mask that mn_map_scores_device takes, adds the terms up
 * and -- if asked -- stores each gradient element once; no target plane is written or read.  One image per call.
 *   d_class_logits [num_classes][height * width] and d_same_logits [offset_dim][height * width]: float32, float16 or
 *   bfloat16 (`dtype`: MN_DTYPE_*; the maps are logits by definition, MN_MAPS_LOGITS is not accepted).
 *   x: the element widened exactly to float32.
 *   Truth class of a pixel: 0 for truth label 0, d_truth_classes[g - 1] for label g in 1..num_truth; a label outside
 *   0..num_truth reads as 0.  The labels are compared as they stand in the mask for the offset planes.
 *   Target y of class plane q: 1 where the truth class is q, else 0.  Target y of offset plane k = (di, dj): 0 where
 *   (r + di, c + dj) is inside the image and carries another truth label ("different"), else 1 ("same": a neighbour
 *   outside the image counts as same).
 *   Term of an element: softplus(z) with z = y ? -x : x, computed in float32 as
 *     fmaxf(z, 0) + log1pf(expf(-fabsf(z)))
 *   -- PyTorch's stable form of BCEWithLogits; x - x * y is exact for y in {0, 1}, so it is the sign flip and
 *   nothing cancels.  expf(-|x|) is a normal float32 up to |x| of about 87; beyond that a term that should be tiny
 *   falls through the subnormals to 0 and is no longer accurate to a few ulp (a term near |x| still is).
 *   Ignore class: a pixel whose truth class lies outside 0..num_classes-1 is left out of the class loss and gets
 *   gradient 0 on all class planes (the store is made); it takes part in the offset planes as any other pixel.
 *   d_sums float64 [2 + O]:
 *     d_sums[0]     = sum of the class terms over the kept pixels and the num_classes planes
 *     d_sums[1 + k] = sum of the terms of offset plane k over all pixels
 *     d_sums[1 + O] = the number of kept pixels, an exact integer
 *   each term widened to float64 before it is added.
 *   Gradient: d_grad_class / d_grad_same have the element type and layout of the maps; either may be NULL (both NULL:
 *   the validation loss, nothing but the sums is written).  Element = (s - y) * scale in float32 with s =
 *   1.0f / (1.0f + expf(-x)) and scale = scale_class / scale_same, rounded to nearest even into the element type.  A
 *   gradient buffer must not overlap a map.  A float16 gradient scaled by 1 / (number of elements) underflows: scale
 *   it up (loss scaling) or use bfloat16.
 * The sums of a call are bit-identical from run to run, the same whether or not a gradient is written and wherever
 * the maps and gradients lie in memory: no floating-point atomic is used, which pixels a lane adds up follows
 * (height, width, element type) only, every workgroup writes its partial sums to its own slot of a buffer of the
 * context and a second launch adds the slots in a fixed order.  accumulate != 0: the image's 2 + O totals are ADDED to
 * what d_sums holds (one IEEE addition per total) -- the totals of a batch or of a validation loop, with no
 * synchronisation between images; accumulate == 0: they are stored.
 * Accesses: 4 elements per lane and 16-byte load and store for float32, 8 for 16-bit maps, where the width is a
 * multiple of that and ALL of the up to four map and gradient bases are 16-byte aligned; 4 per lane and 8-byte
 * accesses for 16-bit maps of width % 4 == 0 and width % 8 != 0 aligned to 8; otherwise single elements, any width
 * and any base.  The truth mask is read through the cache.
 * Any image size (not held to the context's capacity).  0 <= num_classes <= MN_MAX_CLASSES and 0 <= offset_dim <=
 * MN_MAX_OFFSETS, not both 0: num_classes == 0 (d_class_logits may be NULL) is offset-only training, offset_dim == 0
 * (d_same_logits and offset_list may be NULL) class-only.  num_truth >= 0; d_truth_classes may be NULL when num_truth
 * == 0.  offset_list is a HOST array of (di, dj) pairs, any values, (0, 0) and duplicates included.
 * MN_ERR_ARGUMENT: a null pointer that is needed, a non-positive size, height * width > INT_MAX, img_width > 2^30,
 * a count out of range, both counts 0, an unknown dtype or one with MN_MAPS_LOGITS, a scale that is not finite;
 * nothing is launched then.  The partials buffer is the one of mn_map_scores_device (allocated by the first call of
 * either): keep the calls of both on one context on one stream.  Enqueues on `stream` only: no host synchronisation. */
int mn_mask_bce_device(mn_context* ctx, const void* d_class_logits, const void* d_same_logits,
                       int dtype /* MN_DTYPE_* */, int img_width, int img_height, int num_classes, int offset_dim,
                       const int* offset_list, const int* d_truth, int num_truth, const int* d_truth_classes,
                       void* d_grad_class, void* d_grad_same, float scale_class, float scale_same,
                       double* d_sums /* [2+O] */, int accumulate, void* stream);

/* The criteria whose gradient needs totals over a whole plane, from the label mask: the reference's SoftDiceLoss and
 * MultiBCEWithLogitsLoss (utils/loss.py:38-76; --loss dice / --loss mbce of egs/cityscape/local/train.py:193-204 and
 * egs/coco/local/train.py:143-154).  The gradient of an element depends on sums over its plane, so there are three
 * steps -- the sums, a tiny launch for per-plane coefficients, the gradient -- and ONE part of the network's output
 * per call; no target plane is written or read.  One image per call. */
#define MN_PART_CLASS 0          /* the class planes of mn_mask_bce_device: their targets and their ignore class */
#define MN_PART_OFFSET 1         /* its offset planes */
#define MN_PLANE_COMPLEMENT 1    /* flag: q = sigmoid(-x), z = !y (SoftDiceLoss(mode='0')) */
#define MN_PLANE_TERMS 2         /* flag of the sums: rows 3 and 4, the BCE terms, are wanted */
#define MN_CRIT_DICE 0
#define MN_CRIT_MBCE 1

/* Step 1, the sums of one image.
 *   d_logits [num_planes][height * width]: float32, float16 or bfloat16 LOGITS (`dtype`: MN_DTYPE_*; MN_MAPS_LOGITS
 *   is not accepted).  x: the element widened exactly to float32.
 *   part == MN_PART_CLASS: num_planes = C class planes; truth class, target y (1 where the truth class is the plane)
 *   and ignore class (a truth class outside 0..C-1) as for mn_mask_bce_device.  part == MN_PART_OFFSET: num_planes = O
 *   offset planes, offset_list a HOST array of O (di, dj) pairs, any values; y = 0 where (r + di, c + dj) is inside
 *   the image and carries another truth label, else 1; num_truth and d_truth_classes are not used (num_truth >= 0).
 *   s = 1.0f / (1.0f + expf(-x)) in float32.  Without MN_PLANE_COMPLEMENT q = s and z = y; with it
 *   q = 1.0f / (1.0f + expf(x)) and z = !y -- not 1 - s, which cancels where z is rare.
 *   term = softplus(y ? -x : x) in float32, as for mn_mask_bce_device.
 *   d_sums float64 [5 * num_planes + 1], row r of plane p at d_sums[r * num_planes + p]:
 *     row 0  Q_p  = sum of q                      row 3  L1_p = sum of term where y
 *     row 1  I_p  = sum of q where z              row 4  L0_p = sum of term where !y
 *     row 2  Z_p  = the number of z, exact        last   the pixels that took part, exact: the kept pixels of the
 *                                                        class part, height * width of the offset part
 *   each value widened to float64 before it is added.  An ignored pixel is left out of every sum.  Rows 3 and 4 are
 *   computed only with MN_PLANE_TERMS; without it they are written as 0 and no log1pf is spent.
 * The sums of a call are bit-identical from run to run and wherever the map lies in memory: no floating-point atomic
 * is used, which pixels a lane adds up follows (height, width, element type) only, every workgroup writes its partial
 * sums to its own slot of a buffer of the context and a second launch adds the slots in a fixed order.  accumulate !=
 * 0: the image's totals are ADDED to what d_sums holds (one IEEE addition per total) -- the totals of a batch, with no
 * synchronisation between images; accumulate == 0: they are stored.
 * Accesses: as for mn_mask_bce_device (16-byte loads where the width is a multiple of 4 float32 / 8 16-bit elements
 * and the base is aligned, 8-byte loads for 16-bit maps of width % 8 == 4 aligned to 8, single elements otherwise).
 * Any image size (not held to the context's capacity).  1 <= num_planes <= MN_MAX_CLASSES (class part) or
 * MN_MAX_OFFSETS (offset part).  MN_ERR_ARGUMENT: a null pointer that is needed (d_truth_classes when num_truth > 0 in
 * the class part, offset_list in the offset part), a non-positive size, height * width > INT_MAX, img_width > 2^30, a
 * count out of range, an unknown part or flag bit, an unknown dtype or one with MN_MAPS_LOGITS; nothing is launched
 * then.  The partials buffer of this pass is its own (5 MiB, allocated by the first call, freed with the context);
 * keep the calls of one context on one stream.  Enqueues on `stream` only: no host synchronisation. */
int mn_plane_sums_device(mn_context* ctx, const void* d_logits, int dtype /* MN_DTYPE_* */, int img_width,
                         int img_height, int part, int num_planes, const int* offset_list, const int* d_truth,
                         int num_truth, const int* d_truth_classes, int flags, double* d_sums /* [5*P+1] */,
                         int accumulate, void* stream);

/* Step 2, per plane the value of the criterion and the four coefficients of the gradient, from d_sums of step 1 (of
 * one image, or accumulated over a batch).  One small launch, all in float64; each coefficient is rounded once to
 * float32.  d_coeffs float32 [4][num_planes]: c0 / c1 multiply q * (1 - q) where z / where !z, c2 / c3 multiply
 * (s - y) where y / where !y.  With Q, I, Z, L1, L0 the plane's sums:
 *   MN_CRIT_DICE  D = Q + Z + smooth; value = 1 - (2 I + smooth) / D; c1 = sigma scale (2 I + smooth) / D^2;
 *                 c0 = c1 - sigma scale 2 / D; c2 = c3 = 0; sigma = -1 with MN_PLANE_COMPLEMENT (dq/dx = -q (1 - q)),
 *                 else +1.  smooth must be > 0 (D cannot be 0 then).  `pixels` is not used.
 *   MN_CRIT_MBCE  w = (pixels - Q + 1) / (Q + 1); value = w L1 + L0; c0 = c1 = scale L1 (-(pixels + 2) / (Q + 1)^2)
 *                 -- the weight depends on x, this is its derivative --; c2 = scale w; c3 = scale.  The sums must come
 *                 from a call with MN_PLANE_TERMS and without MN_PLANE_COMPLEMENT; the flag is refused here.  `smooth`
 *                 is not used.
 * *d_loss gets scale * (the values added over the planes in ascending order): stored, or -- accumulate != 0 -- added
 * to what it holds in one IEEE addition.  `flags`: MN_PLANE_COMPLEMENT as in step 1 (MN_PLANE_TERMS is accepted and
 * means nothing here).  MN_ERR_ARGUMENT: a null pointer, num_planes outside 1..MN_MAX_CLASSES, an unknown criterion or
 * flag bit, the complement with MN_CRIT_MBCE, smooth, scale or pixels not finite, pixels < 0, smooth <= 0 with
 * MN_CRIT_DICE; nothing is launched then.  Enqueues on `stream` only. */
int mn_plane_coeffs_device(mn_context* ctx, int criterion, int flags, const double* d_sums, int num_planes,
                           double pixels, double smooth, double scale, float* d_coeffs /* [4*P] */, double* d_loss,
                           int accumulate, void* stream);

/* Step 3, the gradient of one image: the arguments of step 1, the coefficients of step 2.
 *   element = f * (q * (1 - q) * (z ? c0 : c1) + (s - y) * (y ? c2 : c3)) in float32, each operation rounded (no
 *   fused multiply-add), rounded to nearest even into the element type of the map; an ignored pixel (class part) gets
 *   0, the store is made.  f = *d_factor, a float32 on the device -- the incoming gradient of a backward pass, read by
 *   the kernel: no synchronisation, no multiply pass --, or 1 when d_factor is NULL.  When c2 and c3 are zero for
 *   every plane (MN_CRIT_DICE) the (s - y) part is skipped, by a branch that is uniform over the launch; the value
 *   is the same either way.
 *   d_grad [num_planes][height * width] has the element type of d_logits and must not overlap it.  Each logit is
 *   loaded once, each gradient element stored once; wide accesses where BOTH bases admit them.
 * `flags`: MN_PLANE_COMPLEMENT as in step 1.  MN_ERR_ARGUMENT: as for step 1, and a null d_coeffs or d_grad; nothing
 * is launched then.  Enqueues on `stream` only: no host synchronisation. */
int mn_plane_grad_device(mn_context* ctx, const void* d_logits, int dtype /* MN_DTYPE_* */, int img_width,
                         int img_height, int part, int num_planes, const int* offset_list, const int* d_truth,
                         int num_truth, const int* d_truth_classes, int flags, const float* d_coeffs /* [4*P] */,
                         const float* d_factor, void* d_grad, void* stream);

/* The cross-entropy criterion from the label mask: the reference's CrossEntropyLossOneHot (utils/loss.py:24-35,
 * F.cross_entropy(input, target.max(1)[1]); --loss ce of egs/coco/local/train.py:145-154 on the class planes and of
 * egs/cityscape/local/train.py:193-204 on the offset planes) on ONE part of the network's output, as a sum, and its
 * gradient, in ONE pass over one image: no target plane and no argmax plane is written or read.
 *   d_logits [num_planes][height * width]: float32, float16 or bfloat16 LOGITS (`dtype`: MN_DTYPE_*; MN_MAPS_LOGITS
 *   is not accepted).  x_q: the element of plane q widened exactly to float32.
 *   Target plane of a pixel -- what target.max(1)[1] elects on the reference's one-hot planes, the FIRST plane whose
 *   target is 1, plane 0 where none is:
 *     part == MN_PART_CLASS: the pixel's truth class (as for mn_mask_bce_device).  A truth class outside
 *     0..num_planes-1 is an ignore class: the pixel has no term, gets gradient 0 on every plane (the store is made)
 *     and is not counted.  (The reference has no ignore class: its one-hot planes would be all zero there and elect
 *     class 0.  With every class in range the two agree.)
 *     part == MN_PART_OFFSET: offset_list a HOST array of num_planes (di, dj) pairs, any values; the least k whose
 *     target is 1 -- (r + di_k, c + dj_k) is outside the image or carries the pixel's own truth label -- or plane 0 if
 *     every plane's target is 0; every pixel takes part; num_truth and d_truth_classes are not used (num_truth >= 0).
 *   Term of a pixel: logsumexp_q(x_q) - x_target, and its gradient softmax(x)_q - [q == target], in float32 as
 *     m    = max_q x_q                      a = the first q with x_q == m
 *     e_q  = expf(x_q - m) for q != a       (e_a is 1)
 *     r    = sum of e_q, q != a, in ascending q
 *     term = log1pf(r) + (m - x_target)     (both summands >= 0)
 *     p_q  = e_q * (1.0f / (1.0f + r));     g_q = (p_q - [q == target]) * scale
 *   each operation rounded (no fused multiply-add).  An x_q more than about 87 below the maximum has an e_q below
 *   2^-126: 0 or a subnormal.  num_planes == 1: term 0 and gradient 0.
 *   d_sums float64 [2]: d_sums[0] = the sum of the terms over the kept pixels, each term widened to float64 before it
 *   is added; d_sums[1] = the number of kept pixels, an exact integer (height * width in the offset part).
 *   Gradient: d_grad has the element type and layout of d_logits, or is NULL (the validation loss: nothing but the
 *   sums is written); element = g_q rounded to nearest even into the element type.  It must not overlap d_logits.  A
 *   float16 gradient scaled by 1 / (number of pixels) underflows: scale it up (loss scaling) or use bfloat16.
 * The sums of a call are bit-identical from run to run, the same whether or not a gradient is written and wherever
 * the map and the gradient lie in memory: no floating-point atomic is used, which pixels a lane adds up follows
 * (height, width, element type) only and the kernel's form num_planes only (up to 20 planes a lane keeps all planes
 * of its pixels in registers and reads every logit once; above that it reads them three times, twice without a
 * gradient, the repeats through the cache), every workgroup writes its partial sums to its own slot of a buffer of the
 * context and a second launch adds the slots in a fixed order.  accumulate != 0: the two totals are ADDED to what d_sums
 * holds (one IEEE addition each) -- the totals of a batch, with no synchronisation between images; accumulate == 0:
 * they are stored.
 * Accesses: as for mn_mask_bce_device (16-byte accesses where the width is a multiple of 4 float32 / 8 16-bit elements
 * and both bases are aligned, 8-byte ones for 16-bit maps of width % 8 == 4 aligned to 8, single elements otherwise).
 * Any image size (not held to the context's capacity).  1 <= num_planes <= MN_MAX_CLASSES (class part) or
 * MN_MAX_OFFSETS (offset part).  MN_ERR_ARGUMENT: a null pointer that is needed (d_truth_classes when num_truth > 0 in
 * the class part, offset_list in the offset part), a non-positive size, height * width > INT_MAX, img_width > 2^30, a
 * count out of range, an unknown part, an unknown dtype or one with MN_MAPS_LOGITS, a scale that is not finite; nothing
 * is launched then.  The partials buffer is the one of mn_map_scores_device (allocated by the first call of either):
 * keep the calls of one context on one stream.  Enqueues on `stream` only: no host synchronisation. */
int mn_mask_ce_device(mn_context* ctx, const void* d_logits, int dtype /* MN_DTYPE_* */, int img_width,
                      int img_height, int part /* MN_PART_* */, int num_planes, const int* offset_list,
                      const int* d_truth, int num_truth, const int* d_truth_classes, void* d_grad /* or null */,
                      float scale, double* d_sums /* [2] */, int accumulate, void* stream);

/* Wire format of the multi-GPU mask exchange (the all-gather of final instance masks the north
 * star asks for; the reference has no exchange, its jobs write files: segment.py:59-61).  d_wire is
 * int16 [n_pixels + 1 + max_instances + 4]: the labels (0..K), K, the classes of labels 1..K
 * padded with -1, then the float64 total log-likelihood as four 16-bit words, low word first
 * (the scalars ride the same gather).  Needs no context; max_instances <= 32767.  d_wire may start
 * at any int16 element and d_mask at any int32 element (a wire inside a batch buffer, a plane of a larger tensor):
 * the vector accesses are taken only where both bases have their natural alignment. */
int mn_pack_wire_device(const int* d_mask, const int* d_object_class, int num_instances,
                        double total_logprob, int n_pixels, int max_instances, short* d_wire,
                        void* stream);

/* Run-length wire format of the same exchange: the row-major label CHANGE POINTS instead of the
 * label of every pixel (the masks are piecewise constant).  d_wire is int32[mn_runs_wire_words(
 * capacity, max_instances)]: [0] change points (-1: more than `capacity`, the image does not fit)
 * [1] K [2..3] float64 log-likelihood, `capacity` ascending positions, `capacity` int16 labels,
 * max_instances int8 classes.  At capacity = n_pixels / 32 the wire is 10.6x smaller than the int16
 * map (397 KB per 1024x2048 image).  No host synchronisation.  mn_unpack_runs_device restores the
 * dense mask (and, if d_table is given, max_instances int32 classes, -1 padded). */
size_t mn_runs_wire_words(int capacity, int max_instances);
int mn_pack_runs_device(mn_context* ctx, const int* d_mask, const int* d_object_class, int num_instances,
                        double total_logprob, int n_pixels, int capacity, int max_instances,
                        int* d_wire, void* stream);
int mn_unpack_runs_device(const int* d_wire, int n_pixels, int capacity, int max_instances,
                          int* d_mask, int* d_table, void* stream);
/* The same for `count` wires in ONE launch (the gathered wires of all ranks): wire i starts at
 * d_wires + i * wire_stride_words, mask i at d_masks + i * n_pixels, table i at d_tables + i * max_instances. */
int mn_unpack_runs_batch_device(const int* d_wires, long long wire_stride_words, int count, int n_pixels,
                                int capacity, int max_instances, int* d_masks, int* d_tables, void* stream);

int mn_last_status(void);
const char* mn_status_string(int status);
const char* mn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MERGENET_HIP_H_ */
