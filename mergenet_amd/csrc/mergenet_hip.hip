// mergenet_hip.hip -- host side of libmergenet_hip.so: workspace, launch sequence, C ABI.
//
// gfx950 only.  Build: see mergenet_amd/csrc/Makefile (hipcc --offload-arch=gfx950
// -ffp-contract=off).  The entry points and the reference interfaces they replace are
// documented in include/mergenet_hip.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <type_traits>

#include "../../include/mergenet_hip.h"
#include "mn_device.h"
#include "mn_kernels_score.h"
#include "mn_kernels_merge.h"
#include "mn_kernels_finish.h"
#include "mn_kernels_output.h"
#include "mn_kernels_prepare.h"
#include "mn_kernels_instances.h"
#include "mn_kernels_match.h"
#include "mn_kernels_eval.h"
#include "mn_kernels_cc.h"
#include "mn_kernels_mapscore.h"
#include "mn_kernels_loss.h"
#include "mn_kernels_planeloss.h"
#include "mn_kernels_celoss.h"
#include "mn_kernels_rle.h"
#include "mn_kernels_tiles.h"
#include "mn_sweep_form.h"
#include "mn_memory.h"
#include "mn_kernels_tail.h"
#include "mn_kernels_exact.h"
#include "mn_kernels_reforder.h"

// The stat block (stat_layout): Counters | 16 int scalars | 4 doubles, each part 16-byte aligned
// scalars: [0] edge violations [1] instances [2] objects [3] class violations [4] record violations
//          [5] RLE change points [6] separability violations [7] table / list overflow
//          [8] component roots [9] negative edges (unsigned)
#define MN_NSCALARS 16

#define MN_MAX_SUBROUNDS 64

static thread_local int g_last_status = MN_OK;
// How an entry point leaves: the status is kept for mn_last_status() and returned.
static int done(int status) { return g_last_status = status; }

#define MN_HIP(expr)                                                                      \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      fprintf(stderr, "mergenet_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), \
              __FILE__, __LINE__);                                                        \
      return done(MN_ERR_NO_DEVICE);                                                      \
    }                                                                                     \
  } while (0)

// Host scratch of n zeroed plain elements that every return path frees; !ok(): no memory (MN_ERR_INTERNAL to the caller).
template <typename T>
struct HostBuf {
  T* p;
  explicit HostBuf(size_t n) : p(static_cast<T*>(calloc(n ? n : 1, sizeof(T)))) {}
  ~HostBuf() { free(p); }
  HostBuf(const HostBuf&) = delete;
  bool ok() const { return p != nullptr; }
  operator T*() const { return p; }
};

// One image call as an entry point received it.  The entry sets the maps, the shape and the outputs; image_call the rest.
struct ImageCall {
  const void *d_class, *d_adj;   // maps, elements of `dtype`
  int dtype;                     // enum mn_dtype, | MN_MAPS_LOGITS when the maps hold logits (fill_params splits it)
  int class_dim, offset_dim, W, H, num_classes;
  int *d_mask, *d_objcls, *d_part;
  hipStream_t stream;
  bool has_offsets;              // the caller gave an offset list (copied only when offset_dim is in range)
  int offs[2 * MN_MAX_OFFSETS];
  mn_options opts;               // resolved: the defaults when the caller gave none
};

struct Queued { int mode, rounds, finish_limit, N; long long R0; bool speculate, want_cert; };

struct mn_context {
  int device;
  int maxH, maxW, maxC, maxO;
  size_t N, Rmax, cap;    // cap: slots of the record table / entries of the record lists CURRENTLY allocated
  size_t cap_full;        // ... and what the general rounds need (allocated on their first use: ensure_general)
  int gen_ready;
  size_t cc_cap;          // table capacity used by the last component contraction
  int debug_flags;        // mn_options.debug_flags of the call in progress
  MnMemory mem;           // every buffer below, by group (mn_memory.h); mem.counted is mn_workspace_bytes
  // objects
  unsigned char *ocls, *cls0, *lpvalid, *matched, *pruned;
  int *osize, *parent, *mate, *root, *label, *mapbuf;
  float* lpsum;
  i64* lp_acc;            // [C][N] fixed-point class log-prob sums of the component contraction
  u64 *ball, *bsub;
  // records
  RecList LA, LB;
  int* touched_list;
  int* fin_lists;         // 3 * MN_FIN2_MAXR ints: scratch lists of the LDS finisher
  int fin_lds_ready, tail_lds_ready;
  int* wire_counts;       // block counts + total of mn_pack_runs_device (apart from the image's own scratch)
  int core_radius;        // short-offset radius of the cores (mn_options::core_radius resolved)
  int ext_events;         // the sweep carries its own start/stop events (hipExtLaunchKernel): no event packets around it
  int cores_used;         // the last attempt ran the general rounds from the cores (mn_core_clean)
  int cc_clean;           // 1: counters and the speculative record table were cleared at the end of the last image
  HashTab T;
  // output / scratch
  int* block_count;
  double* partial;
  Counters* cnt;          // device
  int* scalars;           // device: [0] violations, [1] total instances, [2] n_objects
  unsigned* gmax;         // device [64]: highest visible priority of the round
  unsigned* touch;        // device [64]: records of the round with a matched object at an end (mn_rec_apply)
  unsigned* h_touch;      // pinned mirror
  float* theta;           // device [1]: band threshold of the round
  int* progress;          // device [MN_MAX_SUBROUNDS]: did sub-round s pair anything
  u64* bg_key;            // device
  double* lp_out;         // device [4]
  Counters* h_cnt;        // pinned host mirror
  int* h_scalars;         // pinned
  double* h_lp;           // pinned
  size_t cc_sum_lds, oc_lds;
  // counters, scalars and log-likelihood outputs live in ONE device block mirrored by ONE pinned
  // host block, so that the statistics of an image come back in a single copy
  unsigned char* statblk;
  unsigned char* h_statblk;
  size_t stat_bytes;
  int *cc_tcount, *cc_lcount;   // pixel edges per record: parallel to the components-mode table / list
  unsigned* cc_bits;            // [N] positive out-edges of every pixel (mn_cc_sign)
  int* cc_roots;                // [N] component roots (mn_cc_finish)
  SweepForm cc_sweep;           // of the last contraction (its `waves` partial sums: the tail and the certificate add them up)
  unsigned* cc_negbits;         // per pixel: its negative out-edges (bit k = offset k), written by the sweep
  size_t cc_cap_max;
  hipEvent_t ev[12];   // 0-4 phases, 6-11 components-mode kernels
  // mn_segment_launch / mn_segment_finish: what the second half needs of the first
  struct Pending {
    int active;            // 0 none, 1 kernels queued and verdict unread, 2 finished in launch
    int rc;
    Queued queued;         // what the queued attempt leaves for segment_read_back
    ImageCall call;
    mn_stats stats;
  } pend;
  hipEvent_t ev_done;
  // Replay (MN_DEBUG_REPLAY): a loop that merges image after image through the same buffers issues
  // the same ~17 launches every time, ~3.5 us of host time each -- more than the kernels on the
  // caller's stream take.  The second identical call captures what follows the sweep into two
  // hipGraphs (labelling on the caller's stream, the tail on the side stream); later calls launch
  // the sweep between its two events and the two graphs.
  struct Replay {
    int state;             // 0 nothing, 1 key seen once, 2 graphs ready
    int capturing;         // this attempt records the graphs
    unsigned char key[256];
    size_t key_bytes;
    hipGraph_t gA, gB;
    hipGraphExec_t eA, eB;
    hipStream_t cap;       // capture happens here (the caller's stream may be the null stream, which cannot capture)
    hipStream_t behind;    // the stream an open recording stands for
    Queued queued;         // of the attempt that recorded the graphs
    SweepForm sweep;       // ... and the form of its sweep, whose outputs the graphs read
  } replay;
  hipStream_t side;       // the single-workgroup tail of an image runs here, beside the next image's sweeps
  hipEvent_t ev_fork;
  // What mn_instance_scores_device reads: parent, label, ocls, lpvalid and lpsum as the last segmentation left them,
  // and through last_params the caller's class planes (element type, logits flag and clip with them).  last_valid
  // says that all of it is still that segmentation's: set where an attempt has queued everything (and kept only
  // if its read-back succeeds), cleared by scores_stale() in every entry that overwrites one of those arrays.
  ImgParams last_params;
  int last_valid;
  MnMatchWork* match_work;  // scratch of mn_match_overlaps_device (mn_kernels_match.h): allocated on first use
  MnEvalWork* eval_work;    // scratch of mn_eval_append_device (mn_kernels_eval.h): allocated on first use
  double* ms_partials;      // [MN_MS_VALUES][MN_MS_WORKGROUPS] partial sums of mn_map_scores_device: allocated on first use
  double* pl_partials;      // [MN_PL_VALUES][MN_MS_WORKGROUPS] partial sums of mn_plane_sums_device: allocated on first use
  // workspace of the exact engine (mn_kernels_exact.h): allocated on first use, for the largest
  // image seen so far (group MN_MEM_EXACT; x_free drops it and resets this struct)
  struct XWork {
    XState X;
    size_t n_pix, n_rec, n_cls_floats, hcap, arena_cap, leaf_cap;   // capacities of what is allocated
    void* block;                  // the ONE allocation all arrays live in
    XCtl* h_ctl;                  // pinned
  } xw;
  // ... and what outlives a regrow of it: the sizing rules, the batch arrays, the state of the run
  struct XKeep {
    int lds_ready;
    int prerun;                   // set-up and loop of the image have run (as part of a batch)
    ImgParams* d_P;               // device copies of a batch's parameters (first context of the batch)
    XState* d_X;
    int batch_cap;
    int arena_extra;              // arena words per pixel beyond the initial arrays (doubled when a run fills it)
    int table_permille;           // pair table: load at the start, in thousandths (lowered when a run fills the table)
    int max_blocks;               // most queue blocks (0 = MN_X_MAXBLOCKS); smaller for the contexts of a large batch
  } xk;
  // the reference-order loop (mn_options.tie_order = MN_TIES_REFERENCE, mn_kernels_reforder.h): workspace
  // (group MN_MEM_REFORDER; r_free drops it and resets this struct) and what outlives a regrow
  struct RWork {
    RoState S;
    void* block;                  // one allocation for all arrays
    int n_pix; long long n_rec; int n_cls; long long arena_cap, heap_cap;
    long long* h_ctl;             // pinned
  } rw;
  struct RKeep {
    int arena_per_pixel, heap_per_record;     // (doubled when a run fills them)
    RoState* d_S;                 // device copies of a batch's states (first context of the batch)
    int batch_cap;
  } rk;
  int tie_ref;                    // this attempt: MN_TIES_* as asked for
  int tie_used;                   // ... and what the last exact attempt ran in the end
  // staging for the host-pointer entry points
  float *d_class, *d_same;
  int *d_mask, *d_objcls, *d_part;
};

#define MN_DEFAULT_CORE_RADIUS 6

// MN_TRACE_HOST=1: where the host's time goes in launch / wait / read-back (printed by mn_destroy)
static double g_host_us[4];
static long long g_host_n[2];
static inline double host_now_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3;
}

struct HostLaunchTimer {
  double t0;
  HostLaunchTimer() : t0(host_now_us()) {}
  ~HostLaunchTimer() { g_host_us[0] += host_now_us() - t0; g_host_n[0]++; }
};

static size_t next_pow2(size_t x) {
  size_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// ---- memory: every allocation is a registration with the context (mn_memory.h) --------------------------
static int hip_failed(const char* what, size_t bytes, hipError_t e) {
  if (e != hipSuccess) fprintf(stderr, "mergenet_hip: %s of %zu bytes failed: %s\n", what, bytes, hipGetErrorString(e));
  return e != hipSuccess;
}
static int hip_dev_alloc(void** p, size_t b) { return hip_failed("hipMalloc", b, hipMalloc(p, b)); }
static int hip_pin_alloc(void** p, size_t b) { return hip_failed("hipHostMalloc", b, hipHostMalloc(p, b)); }
static void hip_dev_free(void* p) { (void)hipFree(p); }
static void hip_pin_free(void* p) { (void)hipHostFree(p); }

// How a step leaves on a status that is not MN_OK (an allocation: MN_ERR_NO_DEVICE).
#define MN_TRY(expr) do { const int _rc = (expr); if (_rc != MN_OK) return done(_rc); } while (0)

// n elements on the device, rounded up to 256 bytes and counted toward mn_workspace_bytes
template <typename T>
static int dev_alloc(mn_context* c, int group, T** p, size_t n) { return c->mem.alloc(p, (n * sizeof(T) + 255) & ~(size_t)255, group, MN_MEM_DEVICE, true); }
// ... one that an entry point allocates where it first needs it
template <typename T>
static int ensure_scratch(mn_context* c, T** p, size_t n) { return *p ? MN_OK : dev_alloc(c, MN_MEM_SCRATCH, p, n); }

// ---- exact engine and reference-order loop: workspaces (block, pinned mirror, merge log; the arrays are the block's) ----
static void x_free(mn_context* c) { c->mem.free_group(MN_MEM_EXACT); c->xw = mn_context::XWork(); }
static void r_free(mn_context* c) { c->mem.free_group(MN_MEM_REFORDER); c->rw = mn_context::RWork(); }

// Sizes the workspace for an image of N pixels, O offsets, C classes.  Per pixel (C = 9, O = 10):
// records 20 B x O, pair table 32-64 B x O (load <= 0.5 at the start, falling: pairs only disappear), class
// vectors 4 B x C, objects 20 B, adjacency arena 4 B x (64 + 11 O + 8) (150 words per pixel are used at O = 10, 230 at O = 16;
// a run that fills the arena or the table is repeated with twice as much: exact_run): ~1.7 KB, 3.5 GB for
// 1024 x 2048 (of 288 GB) -- the workspace bounds the images in flight (mn_segment_exact_batch).
static int x_ensure(mn_context* c, int N, int O, int C) {
  mn_context::XWork& w = c->xw;
  mn_context::XKeep& keep = c->xk;
  const size_t NL = (size_t)N * O;
  if (NL >= 0xFFFFFFF0ull) return MN_ERR_CAPACITY;
  size_t B = 256;
  // blocks of the queue: at most 16 K (128 KB of LDS: one image per compute unit); a context that is one of MORE
  // images than the chip has compute units (xk.max_blocks, set by mn_segment_exact_batch) takes at most 6 K
  // (72 KB with the rest of the loop's LDS: two images per compute unit, at the price of longer block scans)
  const size_t max_blocks = keep.max_blocks > 0 ? (size_t)keep.max_blocks : (size_t)MN_X_MAXBLOCKS;
  while ((NL + B - 1) / B > max_blocks) B <<= 1;
  const size_t NB = (NL + B - 1) / B;
  const size_t leaf_cap = NB * B + 1024;             // (a round of the block scan may read past a short block)
  if (keep.arena_extra <= 0) {
    keep.arena_extra = 8 * O + 8;                        // (measured use: 6.4 entries per pixel and offset at O = 10: doubling reallocation, exact-size free lists)
    if (const char* e = getenv("MN_X_ARENA_EXTRA")) { const int v = atoi(e); if (v > 0) keep.arena_extra = v; }   // (tests)
    keep.table_permille = 600;
    if (const char* e = getenv("MN_X_TABLE_PERMILLE")) { const int v = atoi(e); if (v >= 50 && v <= 950) keep.table_permille = v; }   // (tests)
  }
  // pair table: 4-slot buckets for a load of table_permille / 1000 (0.6) at the start (pairs only disappear: it falls)
  const size_t nbuckets = (size_t)((double)NL * 1000.0 / (4.0 * (double)keep.table_permille)) + 64;
  if (nbuckets * 4 >= 0xFFFFFFF0ull) return MN_ERR_CAPACITY;
  // (single pixels keep no stored array: the arena only holds what merges allocate)
  const size_t arena_cap = (size_t)N * (size_t)keep.arena_extra + 65536;
  if (arena_cap >= 0xFFFFFFF0ull) return MN_ERR_CAPACITY;
  const size_t ovf_cap = NL / 256 + 4096;
  if (w.n_pix < (size_t)N || w.n_rec < NL || w.n_cls_floats < (size_t)N * C || w.hcap < nbuckets ||
      w.arena_cap < arena_cap || w.leaf_cap < leaf_cap) {
    x_free(c);
    XState& X = w.X;
    // ONE allocation for the whole workspace, the arrays at 2 MB-aligned offsets (the loop walks them at random)
    auto arrays = [&](void* block) {
      MnCarver k(block, ((size_t)N * O > (1u << 20)) ? ((size_t)2 << 20) : 4096);
      k.carve(X.hs, nbuckets * 4); k.carve(X.rec, NL); k.carve(X.arena, arena_cap); k.carve(X.leaf, leaf_cap);
      k.carve(X.lp, (size_t)N * C + 64); k.carve(X.obj, (size_t)N); k.carve(X.acap, (size_t)N);
      k.carve(X.ostamp, (size_t)N * 2); k.carve(X.overflow, ovf_cap); k.carve(X.l1g, (size_t)MN_X_MAXBLOCKS);
      k.carve(X.tstack, (size_t)MN_X_TSTACK); k.carve(X.freeheads, (size_t)MN_X_FREE_CLASSES); k.carve(X.ctl, 1);
      return k.off;
    };
    int rc = c->mem.alloc(&w.block, arrays(nullptr), MN_MEM_EXACT, MN_MEM_DEVICE, true);
    if (rc == MN_OK) rc = c->mem.alloc(&w.h_ctl, sizeof(XCtl), MN_MEM_EXACT, MN_MEM_PINNED, false);
    if (rc != MN_OK) { x_free(c); return done(rc); }
    arrays(w.block);
    w.n_pix = N; w.n_rec = NL; w.n_cls_floats = (size_t)N * C; w.hcap = nbuckets; w.arena_cap = arena_cap;
    w.leaf_cap = leaf_cap;
    X.overflow_cap = (int)ovf_cap;
  }
  XState& X = w.X;
  X.nb = (unsigned)nbuckets;
  X.arena_cap = arena_cap;
  X.Blog = 0;
  while (((size_t)1 << X.Blog) < B) X.Blog++;
  X.NB = (int)NB;
  X.NBpad = (int)((NB + 63) / 64 * 64);
  X.NG = X.NBpad / 64;
  X.NL = (unsigned)NL;
  X.parent = c->parent;
  X.dbg = getenv("MN_X_FORCE_RELOCATE") ? 1 : 0;                       // (tests)
  // diagnostic: MN_X_MERGELOG=<file> keeps the sequence of merges (survivor, absorbed, record, priority)
  if (getenv("MN_X_MERGELOG") && !X.mlog) {
    if (c->mem.alloc(&X.mlog, (size_t)N * 16, MN_MEM_EXACT, MN_MEM_DEVICE, false) == MN_OK) X.mlog_cap = N;
  }
  return MN_OK;
}

extern "C" void mn_default_options(mn_options* o) {
  memset(o, 0, sizeof(*o));
  o->same_different_bias = 0.0f;
  o->object_merge_factor = 1.0f;
  o->merge_logprob_bias = 0.03f;
  o->variant = MN_VARIANT_CSEGMENT;
  o->mode = MN_MODE_AUTO;
  o->clip_inputs = 0;
  o->exact_limit = 0;
  o->finish_limit = 0;
  o->subrounds = 0;
  o->prune_threshold = 200.0f;
  o->compute_logprob = 1;
}

extern "C" int mn_last_status(void) { return g_last_status; }

extern "C" const char* mn_status_string(int s) {
  switch (s) {
    case MN_OK: return "ok";
    case MN_ERR_ARGUMENT: return "invalid argument";
    case MN_ERR_OFFSETS: return "offset list holds (0,0), a duplicate, or an offset with its negation";
    case MN_ERR_NO_DEVICE: return "HIP device unavailable or HIP call failed";
    case MN_ERR_CAPACITY: return "image exceeds the context's capacity";
    case MN_ERR_NO_BACKGROUND: return "prune: no class-0 object to merge into";
    case MN_ERR_INTERNAL: return "internal error";
    case MN_ERR_UNPROVEN: return "result not proven equal to the reference's sequential order (require_proof)";
    default: return "unknown status";
  }
}

extern "C" const char* mn_version(void) { return "mergenet_hip 0.1 (gfx950)"; }

// record lists A / B, the record table and the finisher's scratch list, `cap` entries each
static int alloc_records(mn_context* c, size_t cap) {
  for (RecList* L : {&c->LA, &c->LB}) {
    MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &L->key, cap));
    MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &L->S, cap));
    MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &L->st, cap));
    MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &L->fr, cap));
    MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &L->aux, cap));
  }
  MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &c->touched_list, cap));
  MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &c->T.key, cap));
  MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &c->T.S, cap));
  MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &c->T.st, cap));
  MN_TRY(dev_alloc(c, MN_MEM_RECORDS, &c->T.touched, cap));
  return MN_OK;
}

// The lists and the table at `cap` entries in place of what there was; c->cap says what is there (0 after a failure).
static int set_records(mn_context* c, size_t cap) {
  c->mem.free_group(MN_MEM_RECORDS);
  c->cap = 0;
  const int rc = alloc_records(c, cap);
  if (rc != MN_OK) { c->mem.free_group(MN_MEM_RECORDS); return rc; }
  c->cap = cap;
  return MN_OK;
}

// Counters | MN_NSCALARS ints | 4 doubles of a stat block at `blk` (null: only its size, which is returned)
static size_t stat_layout(void* blk, Counters*& cnt, int*& scalars, double*& lp) {
  MnCarver k(blk, 16); k.carve(cnt, 1); k.carve(scalars, MN_NSCALARS); k.carve(lp, 4);
  return k.off;
}

static int ctx_alloc(mn_context* c) {
  const size_t N = c->N;
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->ocls, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->cls0, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->lpvalid, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->matched, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->pruned, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->osize, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->parent, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->mate, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->root, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->label, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->mapbuf, N));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->lpsum, N * (size_t)c->maxC));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->fin_lists, 3 * (size_t)MN_FIN2_MAXR));
  c->cc_cap_max = next_pow2(N / 8 + 8192);
  if (c->cc_cap_max > c->cap_full) c->cc_cap_max = c->cap_full;
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->cc_tcount, c->cc_cap_max));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->cc_lcount, c->cc_cap_max));
  // record lists and record table: sized for what the speculative components attempt can use (records
  // BETWEEN components: at most cc_cap_max); the general rounds, which hold a record per pixel edge,
  // get theirs at first use (ensure_general) -- 0.3 instead of 2.1 GB per 1024x2048 context, and a ring
  // of eight of them is what a throughput loop keeps
  MN_TRY(set_records(c, c->cc_cap_max));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->block_count, N / MN_SCAN_ITEMS + 2));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->wire_counts, N / MN_RLE_ITEMS + 4));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->partial, 3 * (N / 256 + 2) > 2 * (N / 64 + 8) ? 3 * (N / 256 + 2) : 2 * (N / 64 + 8)));   // (verify: 3 per block; sweep: 2 per wave)
  c->stat_bytes = stat_layout(nullptr, c->cnt, c->scalars, c->lp_out);
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->statblk, c->stat_bytes));
  stat_layout(c->statblk, c->cnt, c->scalars, c->lp_out);
  MN_TRY(c->mem.alloc(&c->h_statblk, c->stat_bytes, MN_MEM_BASE, MN_MEM_PINNED, false));
  stat_layout(c->h_statblk, c->h_cnt, c->h_scalars, c->h_lp);
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->gmax, 64));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->touch, 64));
  MN_TRY(c->mem.alloc(&c->h_touch, (64 + MN_MAX_SUBROUNDS) * sizeof(unsigned), MN_MEM_BASE, MN_MEM_PINNED, false));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->theta, 4));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->progress, MN_MAX_SUBROUNDS));
  MN_TRY(dev_alloc(c, MN_MEM_BASE, &c->bg_key, 1));
  for (int i = 0; i < 12; i++) MN_HIP(hipEventCreate(&c->ev[i]));
  MN_HIP(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  MN_HIP(hipEventCreate(&c->ev_fork));            // (timing enabled: it can be the stop event of a dispatch)
  {
    // The tail of an image runs beside the NEXT images' sweeps and should not take compute units from
    // them: its stream gets the lowest priority the device offers (sweep 53 instead of 57-60 us by
    // events in bench.py's ring).  How that plays out for a whole loop depends on the ring depth
    // (tests/tools/gpu_ring_sweep.sh, Gpixel/s low / default priority: 2 contexts 11.9 / 11.9, 3 contexts
    // 12.0 / 14.3, 4 contexts 13.6 / 12.3); MN_SIDE_PRIORITY=default in the environment switches it off.
    int lo = 0, hi = 0;
    const char* e = getenv("MN_SIDE_PRIORITY");
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = 0; (void)hipGetLastError(); }
    if (e && e[0] == 'd') lo = 0;
    if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, lo) != hipSuccess) {
      (void)hipGetLastError();
      MN_HIP(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    }
  }
  MN_HIP(hipStreamCreateWithFlags(&c->replay.cap, hipStreamNonBlocking));
  return MN_OK;
}

extern "C" mn_context* mn_create(int device, int max_height, int max_width, int max_classes,
                                 int max_offsets) {
  if (max_height <= 0 || max_width <= 0 || max_classes <= 0 || max_classes > MN_MAX_CLASSES ||
      max_offsets <= 0 || max_offsets > MN_MAX_OFFSETS ||
      (long long)max_height * max_width > (1LL << 28)) {
    g_last_status = MN_ERR_ARGUMENT;
    return NULL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    fprintf(stderr, "mergenet_hip: no HIP device %d (found %d)\n", device, ndev);
    g_last_status = MN_ERR_NO_DEVICE;
    return NULL;
  }
  if (hipSetDevice(device) != hipSuccess) { g_last_status = MN_ERR_NO_DEVICE; return NULL; }
  mn_context* c = static_cast<mn_context*>(calloc(1, sizeof(mn_context)));
  if (!c) { g_last_status = MN_ERR_INTERNAL; return NULL; }
  c->device = device;
  c->mem = MnMemory{{hip_dev_alloc, hip_pin_alloc}, {hip_dev_free, hip_pin_free}};      // (by MnMemKind)
  c->maxH = max_height; c->maxW = max_width; c->maxC = max_classes; c->maxO = max_offsets;
  c->N = (size_t)max_height * max_width;
  c->Rmax = c->N * (size_t)max_offsets;
  c->cap_full = next_pow2(c->Rmax + c->Rmax / 4 + 1024);
  if (ctx_alloc(c) != MN_OK) { mn_destroy(c); return NULL; }
  g_last_status = MN_OK;
  return c;
}

extern "C" void mn_destroy(mn_context* c) {
  if (!c) return;
  if (getenv("MN_TRACE_HOST") && g_host_n[1] > 0) {
    fprintf(stderr, "host: %lld launches %.1f us each; %lld read-backs: waiting for the image %.1f us, the rest %.1f us each\n",
            g_host_n[0], g_host_us[0] / (double)(g_host_n[0] ? g_host_n[0] : 1), g_host_n[1],
            g_host_us[1] / (double)g_host_n[1], g_host_us[2] / (double)g_host_n[1]);
    g_host_n[0] = g_host_n[1] = 0; g_host_us[0] = g_host_us[1] = g_host_us[2] = 0.0;
  }
  (void)hipSetDevice(c->device);
  c->mem.free_all();
  for (int i = 0; i < 12; i++)
    if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  if (c->ev_done) (void)hipEventDestroy(c->ev_done);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->side) (void)hipStreamDestroy(c->side);
  if (c->replay.eA) (void)hipGraphExecDestroy(c->replay.eA);
  if (c->replay.eB) (void)hipGraphExecDestroy(c->replay.eB);
  if (c->replay.gA) (void)hipGraphDestroy(c->replay.gA);
  if (c->replay.gB) (void)hipGraphDestroy(c->replay.gB);
  if (c->replay.cap) (void)hipStreamDestroy(c->replay.cap);
  free(c);
}

extern "C" size_t mn_workspace_bytes(const mn_context* c) { return c ? c->mem.counted : 0; }

// What only the fast paths use (fixed-point class sums, best-record slots, edge masks: 100 B per pixel at C = 9) is
// allocated at their first use: a context that only ever serves the exact engine -- the contexts of a batch
// (mn_segment_exact_batch), where memory per image bounds the images in flight -- never pays for it.
static int ensure_fast(mn_context* c) {
  if (c->cc_negbits) return MN_OK;         // (the last one allocated: the group is whole)
  c->mem.free_group(MN_MEM_FAST);          // (what an attempt that failed half-way left)
  const size_t N = c->N;
  MN_TRY(dev_alloc(c, MN_MEM_FAST, &c->lp_acc, N * (size_t)c->maxC));
  MN_TRY(dev_alloc(c, MN_MEM_FAST, &c->ball, N));
  MN_TRY(dev_alloc(c, MN_MEM_FAST, &c->bsub, N));
  MN_TRY(dev_alloc(c, MN_MEM_FAST, &c->cc_bits, N));
  MN_TRY(dev_alloc(c, MN_MEM_FAST, &c->cc_roots, N));
  MN_TRY(dev_alloc(c, MN_MEM_FAST, &c->cc_negbits, N + 16));
  return MN_OK;
}

// The entry in progress overwrites an array the score kernel reads (or may, depending on the form of its sweep):
// until the next segmentation has finished, mn_instance_scores_device refuses.
static inline void scores_stale(mn_context* c) { c->last_valid = 0; }

static void drop_replay_graphs(mn_context::Replay& rp) {
  if (rp.eA) { (void)hipGraphExecDestroy(rp.eA); rp.eA = nullptr; }
  if (rp.eB) { (void)hipGraphExecDestroy(rp.eB); rp.eB = nullptr; }
  if (rp.gA) { (void)hipGraphDestroy(rp.gA); rp.gA = nullptr; }
  if (rp.gB) { (void)hipGraphDestroy(rp.gB); rp.gB = nullptr; }
  rp.state = 0;
}

// The general rounds (and the small-list exact mode) hold a record per pixel edge: their lists and table
// are allocated when first needed.  Recorded replay graphs hold the old pointers and are dropped.  (The small lists
// go first, to make room.  Should the large ones fail, the small ones come back; a context left without any, c->cap
// = 0, takes no further image: check_args answers MN_ERR_CAPACITY to every size.)
static int ensure_general(mn_context* c) {
  if (c->gen_ready) return MN_OK;
  MN_HIP(hipDeviceSynchronize());
  c->cc_clean = 0;
  drop_replay_graphs(c->replay);
  const int rc = set_records(c, c->cap_full);
  if (rc != MN_OK && set_records(c, c->cc_cap_max) != MN_OK) c->N = 0;
  if (rc != MN_OK) return done(rc);
  c->gen_ready = 1;
  return MN_OK;
}

// ---- argument checking shared by the entry points ---------------------------------------------
static int check_args(const mn_context* c, const ImageCall& call) {
  const int W = call.W, H = call.H, num_classes = call.num_classes, offset_dim = call.offset_dim;
  const int* offs = call.offs;
  if (!c || !call.has_offsets) return MN_ERR_ARGUMENT;
  if (W <= 0 || H <= 0 || num_classes <= 0 || offset_dim <= 0 || call.class_dim < num_classes)
    return MN_ERR_ARGUMENT;
  if (num_classes > MN_MAX_CLASSES || offset_dim > MN_MAX_OFFSETS) return MN_ERR_ARGUMENT;
  if ((size_t)W * H > c->N || num_classes > c->maxC || offset_dim > c->maxO) return MN_ERR_CAPACITY;
  if (call.opts.variant != MN_VARIANT_CSEGMENT && call.opts.variant != MN_VARIANT_PYSEGMENTER)
    return MN_ERR_ARGUMENT;
  for (int a = 0; a < offset_dim; a++)
    for (int b = 0; b < offset_dim; b++) {
      const bool neg = offs[2 * a] == -offs[2 * b] && offs[2 * a + 1] == -offs[2 * b + 1];
      const bool dup = a != b && offs[2 * a] == offs[2 * b] && offs[2 * a + 1] == offs[2 * b + 1];
      if (neg || dup) return MN_ERR_OFFSETS;   // also rejects (0,0): it is its own negation
    }
  return MN_OK;
}

// `dtype` as an entry point takes it: the element type in the low byte, for the entries that read maps
// (`logits_allowed`) optionally MN_MAPS_LOGITS above it; any other bit is an unknown dtype.
static inline bool dtype_ok(int dtype, bool logits_allowed) {
  if (dtype & ~(0xFF | (logits_allowed ? MN_MAPS_LOGITS : 0))) return false;
  const int elem = dtype & 0xFF;
  return elem == MN_DTYPE_F32 || elem == MN_DTYPE_F16 || elem == MN_DTYPE_BF16;
}

// A null offset list is only noted (check_args rejects the call before `offs` is read), as is an offset_dim out of range.
static void image_call(ImageCall* call, const int* offset_list, const mn_options* opts, void* stream) {
  call->has_offsets = offset_list != nullptr;
  if (offset_list && call->offset_dim > 0 && call->offset_dim <= MN_MAX_OFFSETS)
    memcpy(call->offs, offset_list, sizeof(int) * 2 * (size_t)call->offset_dim);
  call->stream = static_cast<hipStream_t>(stream);
  if (opts) call->opts = *opts; else mn_default_options(&call->opts);
}

static void fill_params(ImgParams* P, const ImageCall& call) {
  const int dtype = call.dtype & 0xFF, logits = (call.dtype & MN_MAPS_LOGITS) ? 1 : 0;
  const int offset_dim = call.offset_dim, W = call.W, H = call.H;
  const mn_options* o = &call.opts;
  memset(P, 0, sizeof(*P));
  P->H = H; P->W = W; P->N = W * H; P->C = call.num_classes; P->O = offset_dim;
  P->sdb = o->same_different_bias; P->omf = o->object_merge_factor; P->bias = o->merge_logprob_bias;
  // a 16-bit map cannot hold 1 - 2^-23 and a saturated sigmoid is exactly 1.0 in it: always clipped on load;
  // so are logits: the float32 sigmoid taken on load is exactly 1.0 from about 17 up and 0 below about -104
  P->variant = o->variant; P->clip = (o->clip_inputs || dtype != MN_DTYPE_F32 || logits) ? 1 : 0;
  P->dtype = dtype; P->logits = logits;
  P->cls = call.d_class; P->same = call.d_adj;
  P->djmin = 0; P->djmax = 0;
  for (int k = 0; k < offset_dim; k++) {
    P->di[k] = call.offs[2 * k]; P->dj[k] = call.offs[2 * k + 1];
    if (P->dj[k] < P->djmin) P->djmin = P->dj[k];
    if (P->dj[k] > P->djmax) P->djmax = P->dj[k];
  }
  // pixel-level upper bound: priority <= (log-odds * omf) / den + bias with den = 2 (csegment) or
  // (log-odds * omf + bias) / 1 (pysegmenter); solve for the sameness value, keep a safety margin
  // a 256-pixel tile row of W = 2048*m pixels puts column band j on XCD j under the identity
  // block order already (measured 65 vs 74 us); other widths use the banded order
  P->banded = (W % 2048 == 0) ? 0 : 1;
  P->vmin_first = 0.0f;
  if (P->omf > 0.0f) {
    const double need = (o->variant == MN_VARIANT_CSEGMENT ? -2.0 : -1.0) * (double)P->bias / (double)P->omf;
    P->vmin_first = (float)(1.0 / (1.0 + exp(-need)) - 1e-3);
  }
  // Components mode argues "a record inside a component scores > bias, one between components
  // < bias".  In float32 that needs the quotient gain / (n1 + n2) to survive the addition of the
  // bias (and gain / (n1 * n2) not to underflow): |gain| of every single edge must be at least
  // tau = 2 N ulp(bias)  (resp. 1e-30 N^2), i.e. its sameness value outside (sep_lo, sep_hi).
  P->sep_hi = nextafterf(0.5f, 1.0f);
  P->sep_lo = nextafterf(0.5f, 0.0f);
  if (P->omf > 0.0f && P->bias >= 0.0f) {
    const double n = (double)P->N;
    const double ulp = (double)nextafterf(P->bias, INFINITY) - (double)P->bias;
    const double tau = fmax(2.0 * n * ulp, 1e-30 * n * n) / (double)P->omf;
    const double hi = 1.0 / (1.0 + exp(-tau)), lo = 1.0 / (1.0 + exp(tau));
    float fh = (float)hi, fl = (float)lo;
    if ((double)fh < hi) fh = nextafterf(fh, 1.0f);
    if ((double)fl > lo) fl = nextafterf(fl, 0.0f);
    if (fh > P->sep_hi) P->sep_hi = fh;
    if (fl < P->sep_lo) P->sep_lo = fl;
  }
}

// What the six entry points that take an image begin with: the call is checked (`entry_ok`: what the entry checks
// of its own arguments, reported after the shared checks as MN_ERR_ARGUMENT), the device selected and the kernel
// parameters filled.  `stats`, where the entry has some, is reset once the verdict of the checks is known.  (New for
// segment_attempt and the replay branch: the checks of the maps and the element type; their callers make them first.)
static int begin_call(mn_context* c, const ImageCall& call, bool entry_ok, mn_stats* stats, ImgParams* P) {
  int rc = check_args(c, call);
  if (rc == MN_OK && (!call.d_class || !call.d_adj || !dtype_ok(call.dtype, true) || !entry_ok)) rc = MN_ERR_ARGUMENT;
  if (stats) { memset(stats, 0, sizeof(*stats)); stats->status = rc; stats->total_logprob = NAN; }
  if (rc != MN_OK) return done(rc);
  MN_HIP(hipSetDevice(c->device));
  fill_params(P, call);
  return MN_OK;
}

static long long count_records(const ImageCall& call) {
  long long r = 0;
  for (int k = 0; k < call.offset_dim; k++) {
    const long long hh = call.H - abs(call.offs[2 * k]), ww = call.W - abs(call.offs[2 * k + 1]);
    if (hh > 0 && ww > 0) r += hh * ww;
  }
  return r;
}

static inline unsigned grid_for(size_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }
// blocks of lanes that take four pixels each
static inline unsigned quad_grid(int N, unsigned block) { return grid_for((size_t)(N >> 2) > 0 ? (size_t)(N >> 2) : 1, block); }
static inline unsigned all_offsets(int O) { return O >= 32 ? 0xFFFFFFFFu : ((1u << O) - 1u); }
template <int V> using Int = std::integral_constant<int, V>;
// Run-time values as compile-time ones, for generic lambdas: f(Int<DT>()) for the element type dt (what dtype_ok took,
// without the logits bit), and f(Int<V>()) for v pixels per lane -- 8 only for the 16-bit types, then 4, then 1.
template <typename F>
static void by_dtype(int dt, F f) {
  if (dt == MN_DTYPE_F32) f(Int<MN_DTYPE_F32>());
  else if (dt == MN_DTYPE_F16) f(Int<MN_DTYPE_F16>());
  else f(Int<MN_DTYPE_BF16>());
}
template <int DT, typename F>
static void by_pixels(Int<DT>, int v, F f) {
  if constexpr (DT != MN_DTYPE_F32) {
    if (v == 8) return f(Int<8>());
  }
  v == 4 ? f(Int<4>()) : f(Int<1>());
}

struct FillList {
  FillJobs j;
  size_t largest = 0;
  FillList() { j.count = 0; }
  void add(void* p, size_t bytes, unsigned char byte) {
    if (!bytes) return;
    j.ptr[j.count] = p;
    j.bytes[j.count] = bytes;
    j.pattern[j.count] = 0x01010101u * byte;
    j.count++;
    if (bytes > largest) largest = bytes;
  }
  bool full() const { return j.count == MN_FILL_JOBS; }
  void launch(hipStream_t st) {
    if (!j.count) return;
    unsigned blocks = grid_for(largest / 16 + 1, 256 * 4);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(mn_fill_many, dim3(blocks), dim3(256), 0, st, j);
    j.count = 0;
    largest = 0;
  }
};

// the record table at `cap` slots (a power of two)
static HashTab table_of(const mn_context* c, size_t cap) { HashTab T = c->T; T.mask = (unsigned)(cap - 1); return T; }

static ObjState obj_state(mn_context* c) {
  ObjState S;
  S.ocls = c->ocls; S.osize = c->osize; S.parent = c->parent; S.lpsum = c->lpsum;
  S.lpvalid = c->lpvalid;
  return S;
}

// edge pass dispatch: fast form for the common offset counts, generic form otherwise
template <bool FIRST>
static void launch_edge_pass(mn_context* c, const ImgParams& P, hipStream_t st, u64* out, int s) {
  const int* progress = c->progress;
  const dim3 g(grid_for(P.N, 256)), b(256);
  // XCD-banded tile order (mn_xcd_tile) unless a row is a whole number of 8-tile groups, in
  // which case the identity order already keeps every column band on one XCD (measured faster)
  const dim3 gx(8 * ((grid_for(P.N, 256) + 7) / 8));
  const unsigned char* cls0 = c->ocls;       // unchanged until mn_pix_apply
  const unsigned char* matched = c->matched;
  const bool fast = P.omf > 0.0f && P.sdb == 0.0f && !(c->debug_flags & MN_DEBUG_GENERIC_EDGE_PASS);
  if (fast && P.O == 10 && !P.clip)
    hipLaunchKernelGGL((mn_edge_pass_fast<10, FIRST, false>), gx, b, 0, st, P, cls0, matched, out,
                       progress, s);
  else if (fast && P.O == 10)
    hipLaunchKernelGGL((mn_edge_pass_fast<10, FIRST, true>), gx, b, 0, st, P, cls0, matched, out,
                       progress, s);
  else if (fast && P.O == 16 && !P.clip)
    hipLaunchKernelGGL((mn_edge_pass_fast<16, FIRST, false>), gx, b, 0, st, P, cls0, matched, out,
                       progress, s);
  else if (fast && P.O == 16)
    hipLaunchKernelGGL((mn_edge_pass_fast<16, FIRST, true>), gx, b, 0, st, P, cls0, matched, out,
                       progress, s);
  else
    hipLaunchKernelGGL(mn_edge_pass_generic<FIRST>, g, b, 0, st, P, obj_state(c), matched, out, progress, s);
}

// phase A prologue + class pass (+ first edge pass when `edge` is set)
// `components`: only the fills -- components mode labels first and takes the class planes in its
// own sweep (mn_cc_class_sums), which also sets every field mn_init_objects would
static int run_phase_a(mn_context* c, const ImgParams& P, hipStream_t st, bool edge,
                       FillList* fills = nullptr, bool components = false) {
  const int N = P.N;
  FillList own;
  if (!fills) fills = &own;
  if (!components) {                  // (components mode: mn_cc_class_sums writes lpvalid, nothing reads matched)
    fills->add(c->lpvalid, N, 0);
    fills->add(c->matched, N, 0);
  }
  fills->launch(st);
  if (components) {
    // one event for three timestamps: elapsed(ev[0], ev[0]) = 0 for the phases this mode does not have
    // (with ext_events the sweep's own dispatch sets it)
    if (!c->ext_events) MN_HIP(hipEventRecord(c->ev[0], st));
    return MN_OK;
  }
  hipLaunchKernelGGL(mn_init_objects, dim3(grid_for(N, 256)), dim3(256), 0, st, N, c->osize,
                     c->parent, c->mate);
  MN_HIP(hipEventRecord(c->ev[0], st));
  hipLaunchKernelGGL(mn_class_pass, dim3(quad_grid(N, 256)), dim3(256), 0, st, P, c->ocls);
  MN_HIP(hipEventRecord(c->ev[1], st));
  if (edge) {
    launch_edge_pass<true>(c, P, st, c->ball, 0);
  }
  MN_HIP(hipEventRecord(c->ev[2], st));
  // the per-pixel arg-max is kept apart: ocls is overwritten as objects merge
  MN_HIP(hipMemcpyAsync(c->cls0, c->ocls, N, hipMemcpyDeviceToDevice, st));
  MN_HIP(hipGetLastError());
  return MN_OK;
}

static int read_counters(mn_context* c, hipStream_t st) {
  MN_HIP(hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(Counters), hipMemcpyDeviceToHost, st));
  MN_HIP(hipStreamSynchronize(st));
  return MN_OK;
}

// `src`: the list of the round before (Rsrc records); null: the records come from the pixel graph
static int build_list(mn_context* c, const ImgParams& P, hipStream_t st, size_t cap, RecList L,
                      const RecList* src, int Rsrc, int* Rout) {
  ObjState S = obj_state(c);
  const HashTab T = table_of(c, cap);
  // the next list is appended to by both kernels below; they also fill the best-record slots and
  // the band maximum of the coming round.  ONE launch clears all of it (six memsets cost six
  // dispatch gaps, which is what a late round is made of)
  FillList f;
  f.add(T.key, cap * sizeof(u64), 0xFF);
  f.add(T.S, cap * sizeof(i64), 0);
  f.add(T.touched, cap, 0);
  f.add(&c->cnt->n_records, sizeof(int), 0);
  f.add(c->ball, (size_t)P.N * sizeof(u64), 0);
  f.add(c->gmax, 64 * sizeof(unsigned), 0);
  f.launch(st);
  if (!src)
    hipLaunchKernelGGL(mn_build_from_pixels, dim3(grid_for(P.N, 256)), dim3(256), 0, st, P, S, T);
  else
    hipLaunchKernelGGL(mn_rebuild, dim3(grid_for(Rsrc, MN_REBUILD_ITEMS)), dim3(256), 0, st, S, *src,
                       Rsrc, (const unsigned char*)c->matched, T, L, c->ball, c->gmax, c->cnt, /* fresh_all */ 0);
  if (cap <= (1u << 16))
    hipLaunchKernelGGL(mn_compact<1>, dim3(grid_for(cap, 256)), dim3(256), 0, st, P, S, T, L,
                       c->ball, c->gmax, c->cnt, (const int*)nullptr, (int*)nullptr);
  else
    hipLaunchKernelGGL(mn_compact<4>, dim3(grid_for(cap, MN_COMPACT_SLOTS)), dim3(256), 0, st, P, S, T, L,
                       c->ball, c->gmax, c->cnt, (const int*)nullptr, (int*)nullptr);
  MN_HIP(hipGetLastError());
  if (read_counters(c, st) != MN_OK) return MN_ERR_NO_DEVICE;
  *Rout = c->h_cnt->n_records;
  return MN_OK;
}

// The form of the sweep for the call in progress, as `who` asks for it (the rules: mn_sweep_form.h).
static SweepForm sweep_form_of(const mn_context* c, const ImgParams& P, SweepAsker who) {
  const bool aligned16 = ((reinterpret_cast<uintptr_t>(P.cls) | reinterpret_cast<uintptr_t>(P.same)) & 15) == 0;
  return sweep_form(P.N, P.W, P.O, P.di, P.dj, P.dtype, P.logits != 0, P.clip != 0, P.sdb, aligned16, c->debug_flags, who);
}

// The sweep (mn_cc_sign) in the form F.  It only dispatches: logits (the sigmoid on load) x element type x pixels
// per lane x (plain, cls, lean) are compile-time forms of the kernel.
static void launch_sweep(mn_context* c, const ImgParams& P, hipStream_t st, const SweepForm& F) {
  const dim3 g(F.blocks), b(MN_CC_SIGN_THREADS);
  ClsOut CO;
  CO.ocls = F.lean_cls ? nullptr : c->ocls; CO.cls0 = c->cls0; CO.lpvalid = F.lean_cls ? nullptr : c->lpvalid;
  CO.gsum = reinterpret_cast<int*>(c->lpsum);     // (the summed class log-probs are written later, at roots only)
  CO.gstride = (size_t)P.N;
  auto launch = [&](auto lg, auto dt, auto px, auto plain, auto cls, auto lean) {
    constexpr bool LG = decltype(lg)::value, PLAIN = decltype(plain)::value;
    constexpr int DT = decltype(dt)::value, PX = decltype(px)::value;
    constexpr bool CLS = decltype(cls)::value && PX >= 4, LEAN = decltype(lean)::value && PX >= 4;   // (one pixel per lane: neither)
    // Timed: the dispatch itself carries the two events (hipExtLaunchKernel: start and stop time of THIS kernel),
    // instead of an event packet in front of it and one behind -- each of those cost a ~6 us dispatch gap on the
    // stream, and the pair measured gap + kernel (54 us where rocprofv3 saw 46).
    if (c->ext_events)
      hipExtLaunchKernelGGL((mn_cc_sign<PX, PLAIN, CLS, DT, LG, LEAN>), g, b, 0, st, c->ev[0], c->ev[10], 0, P,
                            c->cc_bits, c->cc_negbits, c->scalars + 6, c->partial, CO, F.LO);
    else
      hipLaunchKernelGGL((mn_cc_sign<PX, PLAIN, CLS, DT, LG, LEAN>), g, b, 0, st, P, c->cc_bits, c->cc_negbits,
                         c->scalars + 6, c->partial, CO, F.LO);
  };
  const std::true_type yes; const std::false_type no;
  auto by_form = [&](auto lg, auto dt, auto px) {
    if (F.plain && F.lean_form) launch(lg, dt, px, yes, yes, yes);
    else if (F.lean_form) launch(lg, dt, px, no, yes, yes);
    else if (F.plain && F.cls) launch(lg, dt, px, yes, yes, no);
    else if (F.plain) launch(lg, dt, px, yes, no, no);
    else if (F.cls) launch(lg, dt, px, no, yes, no);
    else launch(lg, dt, px, no, no, no);
  };
  auto by_px = [&](auto lg) {
    by_dtype(P.dtype, [&](auto dt) { by_pixels(dt, F.px, [&](auto px) { by_form(lg, dt, px); }); });
  };
  P.logits ? by_px(yes) : by_px(no);
}

// the sweep over the positive masks that hooks the offsets the tile stages did not take
template <int PX>
static void launch_cc_hook(mn_context* c, const ImgParams& P, hipStream_t st, unsigned kmask, const unsigned* bits,
                           hipEvent_t hook_done) {
  const dim3 gx(8 * ((grid_for((P.N + PX - 1) / PX, 256) + 7) / 8));
  if (hook_done)                 // (its completion is the fork point of the image: no event packet behind it)
    hipExtLaunchKernelGGL(mn_cc_hook<PX>, gx, dim3(256), 0, st, nullptr, hook_done, 0, P, bits, c->parent, kmask);
  else
    hipLaunchKernelGGL(mn_cc_hook<PX>, gx, dim3(256), 0, st, P, bits, c->parent, kmask);
}

// Replay's recording (mn_context::Replay).  Begin: what is launched on `st` from here on goes into a graph, on the
// capture stream.  End: the graph is instantiated and launched on the stream the recording stood for, and `st` is
// that stream again.  Abandon: an attempt that did not get as far as the end of graph B leaves no recording open.
static int replay_begin(mn_context* c, hipStream_t& st) {
  MN_HIP(hipStreamBeginCapture(c->replay.cap, hipStreamCaptureModeThreadLocal));
  c->replay.behind = st;
  st = c->replay.cap;
  return MN_OK;
}
static int replay_end(mn_context* c, hipGraph_t* graph, hipGraphExec_t* exec, hipStream_t& st) {
  MN_HIP(hipStreamEndCapture(c->replay.cap, graph));
  MN_HIP(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
  MN_HIP(hipGraphLaunch(*exec, c->replay.behind));
  st = c->replay.behind;
  return MN_OK;
}
static void replay_abandon(mn_context::Replay& rp) {
  hipGraph_t open_graph = nullptr;
  if (hipStreamEndCapture(rp.cap, &open_graph) == hipSuccess && open_graph) (void)hipGraphDestroy(open_graph);
  (void)hipGetLastError();
  rp.capturing = 0;
  rp.state = 0;
}

enum CcUse {          // the four uses of the component contraction
  CC_WAITED,          // ordinary components attempt: compacted with the best-record slots, verdict waited for
  CC_QUEUED_COMPACT,  // speculative attempt that ends in the LDS finisher: compacted, nothing waited for
  CC_QUEUED_TAIL,     // speculative attempt that ends in mn_cc_tail: forks to the side stream before the sums
  CC_CORES            // first step of the general rounds, on the edges between clean pixels
};

struct CcPlan {            // everything a contraction decides before its first launch
  bool wait, with_ball;    // CC_WAITED: the verdict is waited for; the compaction fills the best-record slots
  bool with_compact;       // the table is compacted into the list here (mn_cc_tail takes the table itself)
  bool fork_before_sums, cores;   // CC_QUEUED_TAIL / CC_CORES
  SweepForm sweep;
  UnitOffsets unit;        // go to the tile and border stages; the sweep over the mask (the hook) takes the rest
  unsigned kshort, kmask;  // cores: the short offsets (core_radius) / the offsets left to the hook
  unsigned* core_bits;     // cores: the edges between clean pixels (mn_core_bits; `label` is free until the finisher)
  const unsigned* lbits;   // the masks the labelling reads: core_bits, or the sweep's
  int *clsmin, *clsmax;    // class range of the components: `root` and `mapbuf` are free until the output stage
  HashTab T;               // (table, violation counters and any best-record slots were cleared by the caller's fill)
  dim3 tiles;
  // Events.  MN_DEBUG_NO_EVENTS: no per-kernel timestamps on the caller's stream.  MN_DEBUG_LEAN_EVENTS: only the
  // sweep is timed (ev[0], ev[10]).  An event costs the host ~3.5 us to record and ~8 us to read: a dozen per image
  // made the HOST the bottleneck of a loop over images (0.18 ms per step against 0.12 ms of kernels on the stream).
  bool sweep_packet, timed;   // ev[10] is a packet behind the sweep (ext_events: its dispatch carries it) / later stages record theirs
  bool fork_by_hook;       // the last kernel on the caller's stream carries the fork event (hipExtLaunchKernel stop event)
};

static CcPlan make_cc_plan(mn_context* c, const ImgParams& P, CcUse use) {
  CcPlan pl;
  pl.wait = pl.with_ball = use == CC_WAITED;
  pl.with_compact = use == CC_WAITED || use == CC_QUEUED_COMPACT;
  pl.fork_before_sums = use == CC_QUEUED_TAIL; pl.cores = use == CC_CORES;
  pl.sweep = sweep_form_of(c, P, pl.cores ? SWEEP_CORES : SWEEP_COMPONENTS);
  pl.unit = unit_offsets(P.di, P.dj, P.O);
  pl.kmask = all_offsets(P.O);
  if (pl.unit.kh >= 0) pl.kmask &= ~(1u << pl.unit.kh);
  if (pl.unit.kv >= 0) pl.kmask &= ~(1u << pl.unit.kv);
  pl.kshort = 0u;          // short offsets: both components within core_radius pixels (default 6; < 0: every offset is short)
  for (int k = 0; pl.cores && k < P.O; k++)
    if (c->core_radius < 0 || (abs(P.di[k]) <= c->core_radius && abs(P.dj[k]) <= c->core_radius)) pl.kshort |= 1u << k;
  pl.core_bits = pl.cores ? reinterpret_cast<unsigned*>(c->label) : nullptr;
  pl.lbits = pl.cores ? pl.core_bits : c->cc_bits;
  pl.clsmin = c->root; pl.clsmax = c->mapbuf;
  pl.T = table_of(c, c->cc_cap);
  pl.tiles = dim3((P.W + 63) / 64, (P.H + MN_CC_TILE_ROWS - 1) / MN_CC_TILE_ROWS);
  const bool few_events = (c->debug_flags & MN_DEBUG_NO_EVENTS) != 0;
  pl.sweep_packet = !few_events && !c->ext_events;
  pl.timed = !few_events && !(c->debug_flags & MN_DEBUG_LEAN_EVENTS);
  pl.fork_by_hook = pl.fork_before_sums && c->ext_events && !c->replay.capturing && pl.kmask;
  return pl;
}

static int cc_event(mn_context* c, bool on, int ev, hipStream_t st) { if (on) MN_HIP(hipEventRecord(c->ev[ev], st)); return MN_OK; }

// (ev[0], recorded by run_phase_a right before, is its start: every event on the caller's stream costs a ~6 us dispatch gap)
static int cc_sweep(mn_context* c, const ImgParams& P, const CcPlan& pl, hipStream_t st) {
  c->cc_sweep = pl.sweep;
  if (c->replay.capturing) c->replay.sweep = pl.sweep;
  launch_sweep(c, P, st, pl.sweep);
  return cc_event(c, pl.sweep_packet, 10, st);
}

// Cores (first step of the general rounds): the labelling runs on the edges between clean pixels.
static void cc_core_masks(mn_context* c, const ImgParams& P, const CcPlan& pl, hipStream_t st) {
  const dim3 g(grid_for(P.N, 256)), b(256);
  if (!pl.sweep.cls)               // (one pixel per lane: the sweep did not take the class planes)
    hipLaunchKernelGGL(mn_class_pass, dim3(quad_grid(P.N, 256)), b, 0, st, P, c->cls0);
  hipLaunchKernelGGL(mn_core_clean, g, b, 0, st, P, (const unsigned*)c->cc_bits, (const unsigned char*)c->cls0,
                     c->pruned, pl.kshort);
  hipLaunchKernelGGL(mn_core_bits, g, b, 0, st, P, (const unsigned char*)c->pruned, (const unsigned*)c->cc_bits,
                     (const unsigned char*)c->cls0, pl.core_bits);
}

// Labelling: tiles, borders, flatten, hook.  (Labelling the tiles inside the sign sweep -- a block = a 16 x 64 tile --
// was tried: 40.6 us for the fused kernel against 27 + 15 apart; the LDS union-find and its barriers sit on every
// block's critical path and the tile layout reads 256-byte row segments.)
static void cc_label(mn_context* c, const ImgParams& P, const CcPlan& pl, hipStream_t st) {
  const int kh = pl.unit.kh, kv = pl.unit.kv, dv = pl.unit.dv;
  // Four pixels per lane (mn_cc_tiles4) wherever a lane's pixels are one 16-byte access of the masks, of parent[] and
  // of the candidates; MN_DEBUG_TILES_1PX keeps the one-pixel kernel (the yardstick inside one build).  (Replay: the
  // key holds the options and the width, and a recorded graph holds the context's arrays by address, so a graph is
  // never replayed for the other kernel.)
  const uintptr_t bases = reinterpret_cast<uintptr_t>(pl.lbits) | reinterpret_cast<uintptr_t>(c->parent) |
                          reinterpret_cast<uintptr_t>(c->matched);
  if (P.W % 4 == 0 && (bases & 15) == 0 && !(c->debug_flags & MN_DEBUG_TILES_1PX))
    hipLaunchKernelGGL(mn_cc_tiles4, pl.tiles, dim3(256), 0, st, P, pl.lbits, c->parent, kh, kv, dv,
                       c->osize, c->lp_acc, pl.clsmin, pl.clsmax, c->matched);
  else
  hipLaunchKernelGGL(mn_cc_tiles, pl.tiles, dim3(MN_CC_TILE_ROWS * 64), 0, st, P, pl.lbits, c->parent, kh, kv, dv,
                     c->osize, c->lp_acc, pl.clsmin, pl.clsmax, c->matched);   // `matched` is free in this mode
  if (kh >= 0 || kv >= 0)
    hipLaunchKernelGGL(mn_cc_borders, pl.tiles, dim3(128), 0, st, P, pl.lbits, c->parent, kh, kv, dv);
  hipLaunchKernelGGL(mn_cc_flatten, dim3(quad_grid(P.N, 256)), dim3(256), 0, st, P.N, c->parent);
  if (pl.kmask) {
    const hipEvent_t hook_done = pl.fork_by_hook ? c->ev_fork : nullptr;
    if (P.W % 4 == 0) launch_cc_hook<4>(c, P, st, pl.kmask, pl.lbits, hook_done);
    else launch_cc_hook<1>(c, P, st, pl.kmask, pl.lbits, hook_done);
  }
}

// From here on the image is latency-bound work of a few workgroups (and one pixel-wide mask write): it moves to the
// context's side stream, so that the sweeps of the NEXT image (another context, the caller's stream) run beside it
// instead of behind it.  mn_segment_finish waits for the side stream; nothing of this image is left on the caller's.
static int cc_fork(mn_context* c, const CcPlan& pl, hipStream_t& st) {
  if (!pl.fork_by_hook) MN_HIP(hipEventRecord(c->ev_fork, st));
  MN_HIP(hipStreamWaitEvent(c->side, c->ev_fork, 0));
  st = c->side;
  if (c->replay.capturing) return replay_begin(c, st);     // everything from here to the end of the image goes into graph B
  return MN_OK;
}

// Class sums of the components, between ev[11] and ev[8]: from the sweep's lean form, from its per-lane products,
// or (one pixel per lane) from the class planes themselves.
static int cc_sums(mn_context* c, const ImgParams& P, const CcPlan& pl, hipStream_t st) {
  const ObjState S = obj_state(c);
  const int* gsum = reinterpret_cast<const int*>(c->lpsum);
  if (cc_event(c, pl.timed, 11, st) != MN_OK) return MN_ERR_NO_DEVICE;
  const size_t lds = (size_t)MN_CC_SUM_SLOTS * (P.C + 1) * sizeof(u64);
  if (lds > c->cc_sum_lds) {
    for (const void* k : {reinterpret_cast<const void*>(mn_cc_class_sums), reinterpret_cast<const void*>(mn_cc_sums),
                          reinterpret_cast<const void*>(mn_cc_sums_lean)})
      MN_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    c->cc_sum_lds = lds;
  }
  const unsigned blocks = quad_grid(P.N, MN_CC_SUM_THREADS);
  if (pl.sweep.lean_form)
    hipLaunchKernelGGL(mn_cc_sums_lean, dim3(grid_for((size_t)(P.N + 63) / 64, MN_CC_LEAN_GROUPS)),
                       dim3(MN_CC_LEAN_THREADS), lds, st, P, S, (const unsigned char*)c->cls0, gsum, (size_t)P.N,
                       pl.sweep.LO, c->lp_acc, pl.clsmin, pl.clsmax);
  else if (pl.sweep.cls)
    hipLaunchKernelGGL(mn_cc_sums, dim3((blocks + MN_CC_SUMS_ITERS - 1) / MN_CC_SUMS_ITERS), dim3(MN_CC_SUM_THREADS), lds, st, P, S,
                       (const unsigned char*)c->cls0, gsum, (size_t)P.N, c->lp_acc, pl.clsmin, pl.clsmax,
                       pl.cores ? (const unsigned char*)c->pruned : (const unsigned char*)nullptr);
  else
    hipLaunchKernelGGL(mn_cc_class_sums, dim3(blocks), dim3(MN_CC_SUM_THREADS), lds, st, P, S, c->cls0,
                       c->lp_acc, pl.clsmin, pl.clsmax);
  return cc_event(c, pl.timed, 8, st);
}

// Records between components, then ev[9].  (Not for the cores: the rounds build theirs from the pixel graph, positive ones too.)
static int cc_cross(mn_context* c, const ImgParams& P, const CcPlan& pl, hipStream_t st) {
  if (!pl.cores) {
    // (lean form with packed masks: the negative ones are the upper half of the word the labelling read)
    const bool packed = pl.sweep.LO.packed != 0;
    const unsigned* negsrc = packed ? (const unsigned*)c->cc_bits : (const unsigned*)c->cc_negbits;
    const dim3 b(MN_CC_CROSS_THREADS);
    if (pl.sweep.px >= 4)
      hipLaunchKernelGGL(mn_cc_cross<4>, dim3(grid_for((size_t)P.N / 4, MN_CC_CROSS_THREADS)), b, 0, st, P,
                         (const int*)c->parent, pl.T, negsrc, packed ? 16 : 0, 0, c->scalars + 6, c->cc_tcount);
    else
      hipLaunchKernelGGL(mn_cc_cross<1>, dim3(grid_for((size_t)P.N, MN_CC_CROSS_THREADS)), b, 0, st, P,
                         (const int*)c->parent, pl.T, negsrc, 0, 0, c->scalars + 6, c->cc_tcount);
  }
  return cc_event(c, pl.timed, 9, st);
}

// Nothing waits for the verdict here: the object state and the record list are built right away and the violation
// count travels to the host with the record count.  A map that is not separable discards it all (run_phase_a again).
static int cc_finish(mn_context* c, const ImgParams& P, const CcPlan& pl, hipStream_t st) {
  const ObjState S = obj_state(c);
  const dim3 g(grid_for(P.N, 256)), b(256);
  // (`mate` is free in this mode: it keeps the component sizes; lean_cls: the roots' class and validity flag are set here)
  hipLaunchKernelGGL(mn_cc_finish, dim3(grid_for((size_t)(P.N >> 4) > 0 ? (size_t)(P.N >> 4) : 1, 256)), b, 0, st, P, S,
                     (const unsigned char*)c->matched, (const i64*)c->lp_acc,
                     (const int*)pl.clsmin, (const int*)pl.clsmax, c->mate, pl.cores ? (int*)nullptr : c->cc_roots,
                     c->scalars + 8, c->scalars + 6, pl.sweep.lean_cls ? (const unsigned char*)c->cls0 : (const unsigned char*)nullptr);
  if (pl.cores) {
    if (pl.kshort != all_offsets(P.O)) {           // a core with a non-positive edge inside falls apart again
      MN_HIP(hipMemsetAsync(c->matched, 0, (size_t)P.N, st));    // (the root candidates are done with)
      hipLaunchKernelGGL(mn_core_check, g, b, 0, st, P, (const int*)c->parent, pl.lbits, c->matched);
      hipLaunchKernelGGL(mn_core_dissolve, g, b, 0, st, P, S, (const unsigned char*)c->matched, c->scalars + 9);
    }
    // what mn_build_from_pixels will insert: sizes its table (c->touch was cleared by the caller's fill)
    hipLaunchKernelGGL(mn_count_cross_edges, g, b, 0, st, P, (const int*)c->parent, c->touch);
  }
  if (pl.with_compact)             // (mn_cc_tail takes the table itself)
    hipLaunchKernelGGL(mn_compact<4>, dim3(grid_for(c->cc_cap, MN_COMPACT_SLOTS)), dim3(256), 0, st, P, S,
                       pl.T, c->LA, pl.with_ball ? c->ball : (u64*)nullptr, c->gmax, c->cnt,
                       (const int*)c->cc_tcount, c->cc_lcount);
  MN_HIP(hipGetLastError());
  return MN_OK;
}

// 0 when the input is sign-separable, 1 when it is not, or the table filled up (the caller falls back)
static int cc_verdict(mn_context* c, hipStream_t st) {
  MN_HIP(hipMemcpyAsync(c->h_scalars, c->scalars, MN_NSCALARS * sizeof(int), hipMemcpyDeviceToHost, st));
  MN_HIP(hipMemcpyAsync(c->h_cnt, c->cnt, sizeof(Counters), hipMemcpyDeviceToHost, st));
  MN_HIP(hipStreamSynchronize(st));
  if (c->h_scalars[6] == 0 && c->h_scalars[7] == 0) return 0;
  MN_HIP(hipMemsetAsync(c->cnt, 0, sizeof(Counters), st));
  return 1;
}

// Component contraction (mn_kernels_cc.h).  CC_WAITED: returns 0 when the input is sign-separable (object state +
// list of records between components ready, count in h_cnt), 1 when it is not (caller falls back), < 0 on error.
// The others: everything is queued, 0 is returned and the verdict is read by the caller at the end.  `st` ends on
// the side stream where the image forked, and on replay's capture stream while graph B is being recorded.
static int run_components(mn_context* c, const ImgParams& P, hipStream_t& st, CcUse use) {
  const CcPlan pl = make_cc_plan(c, P, use);
  mn_context::Replay& rp = c->replay;
  int rc;
  if ((rc = cc_sweep(c, P, pl, st)) != MN_OK) return rc;
  if (pl.cores) cc_core_masks(c, P, pl, st);
  if (rp.capturing && (rc = replay_begin(c, st)) != MN_OK) return rc;       // the labelling stages go into graph A
  cc_label(c, P, pl, st);
  if (rp.capturing && (rc = replay_end(c, &rp.gA, &rp.eA, st)) != MN_OK) return rc;
  // end of the labelling stages, on the stream they ran on (the side stream starts when it gets the chip)
  if ((rc = cc_event(c, pl.timed, 7, st)) != MN_OK) return rc;
  if (pl.fork_before_sums && (rc = cc_fork(c, pl, st)) != MN_OK) return rc;
  if ((rc = cc_sums(c, P, pl, st)) != MN_OK) return rc;
  if ((rc = cc_cross(c, P, pl, st)) != MN_OK) return rc;
  if ((rc = cc_finish(c, P, pl, st)) != MN_OK) return rc;
  return pl.wait ? cc_verdict(c, st) : 0;             // speculative: the caller finds out at its final synchronisation
}

// ---- exact engine: set-up kernels, the loop, hand-over to the output stage ------------------------
// The loop kernel is ONE wavefront that runs until the queue is empty; it comes back early when its
// step budget is used up (MN_X_BUDGET: block maxima are rebuilt and it is launched again) or when the
// adjacency arena is full.  `ev[1]`, `ev[2]` bracket the two set-up kernels (class terms / records).
static int exact_setup(mn_context* c, const ImgParams& P, hipStream_t st) {
  int rc = x_ensure(c, P.N, P.O, P.C);
  if (rc != MN_OK) return rc;
  mn_context::XWork& w = c->xw;
  XState& X = w.X;
  const size_t N = (size_t)P.N;
  MN_HIP(hipMemsetAsync(X.hs, 0xFF, (size_t)X.nb * 4 * sizeof(XSlot), st));
  MN_HIP(hipMemsetAsync(X.leaf, 0, (((size_t)X.NB << X.Blog) + 1024) * sizeof(unsigned), st));
  MN_HIP(hipMemsetAsync(X.ostamp, 0, (size_t)N * 2 * sizeof(unsigned), st));
  MN_HIP(hipMemsetAsync(X.freeheads, 0xFF, MN_X_FREE_CLASSES * sizeof(unsigned), st));
  memset(w.h_ctl, 0, sizeof(XCtl));
  w.h_ctl->ttrack = getenv("MN_X_NO_TIE_TRACKING") ? 0 : 1;          // (timing comparisons)
  w.h_ctl->bump = 0ull;
  MN_HIP(hipMemcpyAsync(X.ctl, w.h_ctl, sizeof(XCtl), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(mn_x_init_objects, dim3(grid_for(N, 256)), dim3(256), 0, st, P, X, c->cls0);
  MN_HIP(hipEventRecord(c->ev[1], st));
  hipLaunchKernelGGL(mn_x_init_records, dim3(grid_for((size_t)X.NL, 256)), dim3(256), 0, st, P, X);
  MN_HIP(hipEventRecord(c->ev[2], st));
  MN_HIP(hipGetLastError());
  return MN_OK;
}

// The loop for a batch of images (contexts set up by exact_setup), ONE launch with a workgroup per image;
// device copies of the images' parameters live in the first context given.  `full[i]` is set for an image that ran
// out of arena or pair table (its workspace grows and exact_run repeats it; the others finish).
static int exact_loop(mn_context** cs, int n, const ImgParams* Ps, hipStream_t st, unsigned char* full) {
  mn_context::XKeep& w0 = cs[0]->xk;
  if (w0.batch_cap < n) {
    MnMemory& mem = cs[0]->mem;
    mem.free_group(MN_MEM_EXACT_BATCH);
    w0.batch_cap = 0;
    int rc = mem.alloc(&w0.d_P, (size_t)n * sizeof(ImgParams), MN_MEM_EXACT_BATCH, MN_MEM_DEVICE, false);
    if (rc == MN_OK) rc = mem.alloc(&w0.d_X, (size_t)n * sizeof(XState), MN_MEM_EXACT_BATCH, MN_MEM_DEVICE, false);
    if (rc != MN_OK) { mem.free_group(MN_MEM_EXACT_BATCH); return done(rc); }
    w0.batch_cap = n;
  }
  size_t lds = 0;
  long long max_total = 0;
  {
    HostBuf<XState> hx((size_t)n);
    if (!hx.ok()) return MN_ERR_INTERNAL;
    for (int i = 0; i < n; i++) {
      const XState& X = cs[i]->xw.X;
      hx[i] = X;
      const size_t l = MN_X_LDS_BYTES(X.NBpad);
      if (l > lds) lds = l;
      // every wave reaches the loop exit: the reference needs ~0.4 steps per initial record; 8 per
      // record (plus slack) is the hard stop of a run, whatever the input
      const long long mt = 8LL * (long long)X.NL + 65536;
      if (mt > max_total) max_total = mt;
    }
    hipError_t e1 = hipMemcpyAsync(w0.d_P, Ps, (size_t)n * sizeof(ImgParams), hipMemcpyHostToDevice, st);
    hipError_t e2 = hipMemcpyAsync(w0.d_X, hx, (size_t)n * sizeof(XState), hipMemcpyHostToDevice, st);
    hipError_t e3 = hipStreamSynchronize(st);     // (before any return: a copy queued ahead of a failed call still reads host scratch)
    MN_HIP(e1); MN_HIP(e2); MN_HIP(e3);
  }
  if (!w0.lds_ready) {
    MN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mn_x_run),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    w0.lds_ready = 1;
  }
  long long per_launch = 1LL << 24;                  // steps per launch (MN_X_BUDGET: tests of the relaunch)
  if (const char* e = getenv("MN_X_BUDGET")) { const long long v = atoll(e); if (v > 0) per_launch = v; }
  const long long max_launches = 1 << 20;
  for (long long it = 0; it < max_launches; it++) {
    long long most = 0;
    bool any = false;
    for (int i = 0; i < n; i++) {
      mn_context::XWork& w = cs[i]->xw;
      if (it > 0 && w.h_ctl->status != MN_X_BUDGET) continue;
      any = true;
      if (w.h_ctl->steps > most) most = w.h_ctl->steps;
      hipLaunchKernelGGL(mn_x_build_l1, dim3(w.X.NB), dim3(64), 0, st, w.X);
    }
    if (!any) break;
    const long long left = max_total - most;
    if (left <= 0) {
      fprintf(stderr, "mergenet_hip: exact engine exceeded %lld steps\n", max_total);
      return MN_ERR_INTERNAL;
    }
    const long long budget = left < per_launch ? left : per_launch;
    hipLaunchKernelGGL(mn_x_run, dim3((unsigned)n), dim3(64), lds, st, (const ImgParams*)w0.d_P, (const XState*)w0.d_X, budget);
    MN_HIP(hipGetLastError());
    for (int i = 0; i < n; i++)
      MN_HIP(hipMemcpyAsync(cs[i]->xw.h_ctl, cs[i]->xw.X.ctl, sizeof(XCtl), hipMemcpyDeviceToHost, st));
    MN_HIP(hipStreamSynchronize(st));
    bool all_done = true;
    for (int i = 0; i < n; i++) {
      const int status = cs[i]->xw.h_ctl->status;
      if (status == MN_X_DONE) continue;
      all_done = false;
      if (status == MN_X_BUDGET) continue;
      if (status == MN_X_ARENA_FULL || status == MN_X_HASH_FULL) {
        if (getenv("MN_TRACE_EXACT"))
          fprintf(stderr, "exact engine: out of %s after %lld steps (image %d of the batch): workspace grows, run repeated\n",
                  status == MN_X_ARENA_FULL ? "adjacency arena" : "pair table", cs[i]->xw.h_ctl->steps, i);
        full[i] = (unsigned char)status;
        continue;
      }
      fprintf(stderr, "mergenet_hip: exact engine stopped with status %d after %lld steps\n", status, cs[i]->xw.h_ctl->steps);
      return MN_ERR_INTERNAL;
    }
    if (all_done) break;
  }
  for (int i = 0; i < n; i++)
    if (cs[i]->xw.h_ctl->status != MN_X_DONE && !full[i]) return MN_ERR_INTERNAL;
  return MN_OK;
}

// Set-up and loop of a batch; an image whose workspace was too small is repeated with a larger one.
static int exact_run(mn_context** cs, int n, const ImgParams* Ps, hipStream_t st) {
  HostBuf<mn_context*> sub((size_t)n); HostBuf<ImgParams> subP((size_t)n); HostBuf<unsigned char> full((size_t)n);
  int rc = (sub.ok() && subP.ok() && full.ok()) ? MN_OK : MN_ERR_INTERNAL, m = n;
  for (int i = 0; i < n && rc == MN_OK; i++) { sub[i] = cs[i]; subP[i] = Ps[i]; }
  for (int attempt = 0; rc == MN_OK && m > 0; attempt++) {
    if (attempt == 8) { rc = MN_ERR_CAPACITY; break; }
    for (int i = 0; i < m && rc == MN_OK; i++) rc = exact_setup(sub[i], subP[i], st);
    if (rc != MN_OK) break;
    memset(full, 0, (size_t)m);
    rc = exact_loop(sub, m, subP, st, full);
    if (rc != MN_OK) break;
    int k = 0;
    for (int i = 0; i < m; i++) {
      if (!full[i]) continue;
      mn_context::XKeep& w = sub[i]->xk;
      if (full[i] == MN_X_ARENA_FULL) w.arena_extra *= 2;
      else if (w.table_permille > 100) w.table_permille = w.table_permille * 2 / 3;
      else { rc = MN_ERR_CAPACITY; break; }
      sub[k] = sub[i]; subP[k] = subP[i]; k++;
    }
    m = k;
  }
  return rc;
}

// what the output stage reads: sizes, classes and class sums of the survivors, step counters
static int exact_export(mn_context* c, const ImgParams& P, hipStream_t st) {
  mn_context::XWork& w = c->xw;
  XState& X = w.X;
  const size_t N = (size_t)P.N;
  if (getenv("MN_X_CHECK_SLOTS") && c->tie_used != MN_TIES_REFERENCE) {
    // tests: records and pair-table slots must point at each other at the end of a run
    const size_t n = (size_t)X.NL > (size_t)X.nb * 4 ? (size_t)X.NL : (size_t)X.nb * 4;
    hipLaunchKernelGGL(mn_x_check_slots, dim3(grid_for(n, 256)), dim3(256), 0, st, X);
    long long errs = -1;
    MN_HIP(hipMemcpyAsync(&errs, &X.ctl->slot_errors, sizeof(errs), hipMemcpyDeviceToHost, st));
    MN_HIP(hipStreamSynchronize(st));
    fprintf(stderr, "exact engine: pair-table check: %lld errors (slow inserts %lld)\n", errs, w.h_ctl->slow_inserts);
    if (errs != 0) return MN_ERR_INTERNAL;
  }
  if (getenv("MN_TRACE_EXACT"))
    fprintf(stderr, "exact engine: steps %lld merges %lld rescans %lld reallocs %lld folded %lld adopted %lld slow inserts %lld set-up overflow %d arena %llu of %llu\n",
            w.h_ctl->steps, w.h_ctl->merges, w.h_ctl->rescans, w.h_ctl->reallocs, w.h_ctl->folded,
            w.h_ctl->adopted, w.h_ctl->slow_inserts, abs(w.h_ctl->n_overflow), w.h_ctl->bump, X.arena_cap);
#ifdef MN_X_STAMPS
  if (getenv("MN_TRACE_EXACT")) {
    static const char* nm[12] = {"loop", "pop", "record+scan", "objects+score", "restale", "merge-state", "realloc",
                                 "walk-load", "probe+third", "fold/adopt", "rescore+queue", "rescan+groups"};
    long long tot = 0;
    for (int i = 0; i < 12; i++) tot += w.h_ctl->stamps[i];
    for (int i = 0; i < 12; i++)
      fprintf(stderr, "  stamp %-14s %12lld cycles %5.1f%%\n", nm[i], w.h_ctl->stamps[i], 100.0 * w.h_ctl->stamps[i] / (tot ? tot : 1));
  }
#endif
  if (const char* path = getenv("MN_X_MERGELOG")) {
    if (X.mlog && w.h_ctl->merges > 0) {
      const size_t n = (size_t)(w.h_ctl->merges < X.mlog_cap ? w.h_ctl->merges : X.mlog_cap);
      int* h = static_cast<int*>(malloc(n * 16));
      if (h && hipMemcpy(h, X.mlog, n * 16, hipMemcpyDeviceToHost) == hipSuccess) {
        if (FILE* f = fopen(path, "wb")) { fwrite(h, 16, n, f); fclose(f); }
      }
      free(h);
    }
  }
  hipLaunchKernelGGL(mn_x_export_objects, dim3(grid_for(N, 256)), dim3(256), 0, st, P, X, c->osize, c->ocls,
                     c->lpsum, c->lpvalid);
  const long long steps = w.h_ctl->steps, merges = w.h_ctl->merges;
  Counters hc;
  memset(&hc, 0, sizeof(hc));
  hc.finisher_steps = (int)(steps > 0x7FFFFFFF ? 0x7FFFFFFF : steps);
  hc.finisher_merges = (int)merges;
  hc.n_merged = (int)merges;
  *c->h_cnt = hc;
  MN_HIP(hipMemcpyAsync(c->cnt, c->h_cnt, sizeof(Counters), hipMemcpyHostToDevice, st));
  MN_HIP(hipGetLastError());
  return MN_OK;
}

// ---- the reference-order loop (tie_order = MN_TIES_REFERENCE): workspace, launches ---------------------
// Per record: two list nodes (12 B each), ends, log-odds, priority (16 B), queue entries (8 B x 3: the
// reference's queue holds up to 2.4 entries per record, stale ones included); per pixel: object state, map
// header, bucket arrays (13 + 29 + ... entries as the maps grow: 95-200 per pixel measured).
static int r_ensure(mn_context* c, int N, int O, int C) {
  mn_context::RWork& w = c->rw;
  mn_context::RKeep& keep = c->rk;
  if (keep.arena_per_pixel <= 0) {
    keep.arena_per_pixel = 16 * O + 64; keep.heap_per_record = 3;
    if (const char* e = getenv("MN_RO_ARENA_PER_PIXEL")) { const int v = atoi(e); if (v > 0) keep.arena_per_pixel = v; }   // (tests)
    if (const char* e = getenv("MN_RO_HEAP_PER_RECORD")) { const int v = atoi(e); if (v > 0) keep.heap_per_record = v; }
  }
  const long long NL = (long long)N * O;
  const long long arena_cap = (long long)N * keep.arena_per_pixel + 65536;
  const long long heap_cap = NL * keep.heap_per_record + 65536;
  if (NL > (1LL << 28)) return MN_ERR_CAPACITY;          // (node ids 2 * record + side are ints)
  if (!(w.block && w.n_pix >= N && w.n_rec >= NL && w.arena_cap >= arena_cap && w.heap_cap >= heap_cap)) {
    r_free(c);
    RoState& S = w.S;
    auto arrays = [&](void* block) {
      MnCarver k(block, 256);
      k.carve(S.osize, (size_t)N); k.carve(S.ocls, (size_t)N); k.carve(S.bcount, (size_t)N); k.carve(S.nelem, (size_t)N);
      k.carve(S.head, (size_t)N); k.carve(S.boff, (size_t)N); k.carve(S.single, (size_t)N);
      k.carve(S.barena, (size_t)arena_cap); k.carve(S.nnext, (size_t)NL * 2); k.carve(S.nkey, (size_t)NL * 2);
      k.carve(S.r1, (size_t)NL); k.carve(S.r2, (size_t)NL); k.carve(S.oml, (size_t)NL); k.carve(S.prio, (size_t)NL);
      k.carve(S.heap, (size_t)heap_cap); k.carve(S.ctl, 16);
      return k.off;
    };
    int rc = c->mem.alloc(&w.block, arrays(nullptr), MN_MEM_REFORDER, MN_MEM_DEVICE, true);
    if (rc == MN_OK) rc = c->mem.alloc(&w.h_ctl, 128, MN_MEM_REFORDER, MN_MEM_PINNED, false);
    if (rc != MN_OK) { r_free(c); return done(rc); }
    arrays(w.block);
    w.n_pix = N; w.n_rec = NL; w.n_cls = C; w.arena_cap = arena_cap; w.heap_cap = heap_cap;
  }
  w.S.N = N; w.S.C = C; w.S.NL = NL;
  w.S.barena_cap = w.arena_cap; w.S.hcap = w.heap_cap;
  return MN_OK;
}

// The exact engine's set-up (class vectors, records with the reference's log-odds), then ONE wave per image runs the
// reference's constructor loop and merge loop on its containers (mn_reforder.h); a run that fills the bucket
// arena or the queue is repeated with twice as much.  A batch of images is ONE launch of the loop with a
// workgroup per image (the loop is sequential in the reference's own data structures: images in flight are its
// throughput, as for the exact engine).
// set-up of one image; returns 1 when the parallel map construction ran out of bucket arena (grown, try again)
static int ro_setup(mn_context* c, const ImgParams& P, hipStream_t st) {
  if (P.variant != MN_VARIANT_CSEGMENT) return MN_ERR_ARGUMENT;
  int rc = exact_setup(c, P, st);
  if (rc != MN_OK) return rc;
  rc = r_ensure(c, P.N, P.O, P.C);
  if (rc != MN_OK) return rc;
  mn_context::RWork& w = c->rw;
  XState& X = c->xw.X;
  w.S.lp = X.lp; w.S.parent = X.parent; w.S.omf = P.omf; w.S.bias = P.bias;
  const RoState S = w.S;
  hipLaunchKernelGGL(mn_ro_prepare_objects, dim3(grid_for((size_t)P.N, 256)), dim3(256), 0, st, P, X, S);
  hipLaunchKernelGGL(mn_ro_prepare_records, dim3(grid_for((size_t)S.NL, 256)), dim3(256), 0, st, P, X, S);
  // (ctl[7]: lanes of the parallel map construction that found the bucket arena full)
  hipLaunchKernelGGL(mn_ro_build_maps, dim3(grid_for((size_t)P.N, 64)), dim3(64), 0, st, P, S,
                     reinterpret_cast<int*>(S.ctl + 7));
  MN_HIP(hipGetLastError());
  MN_HIP(hipMemcpyAsync(w.h_ctl, S.ctl, 128, hipMemcpyDeviceToHost, st));
  return MN_OK;
}

// The loop of a batch (contexts set up by ro_setup), relaunched while any image has used up its pop budget;
// device copies of the images' states live in the first context given.  full[i]: MN_RO_ARENA_FULL / MN_RO_HEAP_FULL
// for an image whose workspace was too small (it grows and the caller repeats that image).
static int ro_loop(mn_context** cs, int n, const ImgParams* Ps, hipStream_t st, unsigned char* full) {
  mn_context::RKeep& w0 = cs[0]->rk;
  if (w0.batch_cap < n) {
    cs[0]->mem.free_group(MN_MEM_REFORDER_BATCH);
    w0.batch_cap = 0;
    MN_TRY(cs[0]->mem.alloc(&w0.d_S, (size_t)n * sizeof(RoState), MN_MEM_REFORDER_BATCH, MN_MEM_DEVICE, false));
    w0.batch_cap = n;
  }
  HostBuf<RoState> hs((size_t)n);
  if (!hs.ok()) return MN_ERR_INTERNAL;
  long long max_pops = 0;
  for (int i = 0; i < n; i++) {
    hs[i] = cs[i]->rw.S;
    // every loop ends: the reference pops each queue entry once, and a record is pushed at most once per
    // re-score; 64 pops per initial record is far beyond what it does (4-5)
    const long long mp = 64LL * hs[i].NL + 65536;
    if (mp > max_pops) max_pops = mp;
  }
  MN_HIP(hipMemcpyAsync(w0.d_S, hs, (size_t)n * sizeof(RoState), hipMemcpyHostToDevice, st));
  MN_HIP(hipStreamSynchronize(st));
  long long per_launch = 1LL << 20;                  // pops per launch (MN_X_BUDGET: tests of the relaunch)
  if (const char* e = getenv("MN_X_BUDGET")) { const long long v = atoll(e); if (v > 0) per_launch = v; }
  for (long long it = 0; it < (1 << 20); it++) {
    hipLaunchKernelGGL(mn_ro_loop, dim3((unsigned)n), dim3(64), 0, st, (const RoState*)w0.d_S, Ps[0].O, per_launch);
    MN_HIP(hipGetLastError());
    for (int i = 0; i < n; i++)
      MN_HIP(hipMemcpyAsync(cs[i]->rw.h_ctl, cs[i]->rw.S.ctl, 128, hipMemcpyDeviceToHost, st));
    MN_HIP(hipStreamSynchronize(st));
    if ((it & 31) == 31 && getenv("MN_TRACE_EXACT"))     // (a 1024x2048 image takes ~100 launches: a sign of life)
      fprintf(stderr, "reference-order loop: launch %lld, image 0 at %lld pops\n", it + 1, cs[0]->rw.h_ctl[3]);
    bool again = false;
    for (int i = 0; i < n; i++) {
      const long long status = cs[i]->rw.h_ctl[0];
      if (status == MN_RO_BUDGET) {
        if (cs[i]->rw.h_ctl[3] > max_pops) {
          fprintf(stderr, "mergenet_hip: reference-order loop exceeded %lld pops\n", max_pops);
          return MN_ERR_INTERNAL;
        }
        again = true;
      }
    }
    if (!again) break;
  }
  for (int i = 0; i < n; i++) {
    mn_context::RWork& w = cs[i]->rw;
    const long long status = w.h_ctl[0];
    if (getenv("MN_TRACE_EXACT"))
      fprintf(stderr, "reference-order loop: status %lld pops %lld merges %lld bucket arena %lld of %lld largest queue %lld of %lld; "
              "seconds: constructor's loop %.2f, pops (and stores of fresh priorities) %.2f, merges %.2f\n",
              status, w.h_ctl[3], w.h_ctl[4], w.h_ctl[2], w.arena_cap, w.h_ctl[6], w.heap_cap,
              (double)w.h_ctl[8] * 1e-8, (double)w.h_ctl[9] * 1e-8, (double)w.h_ctl[10] * 1e-8);
    if (status == MN_RO_ARENA_FULL || status == MN_RO_HEAP_FULL) { full[i] = (unsigned char)status; continue; }
    if (status != MN_RO_DONE) {
      fprintf(stderr, "mergenet_hip: reference-order loop stopped with status %lld after %lld pops\n", status, w.h_ctl[3]);
      return MN_ERR_INTERNAL;
    }
  }
  return MN_OK;
}

static int ro_finish(mn_context* c, const ImgParams& P, hipStream_t st) {
  mn_context::RWork& w = c->rw;
  const RoState S = w.S;
  const size_t n = (size_t)S.NL > (size_t)P.N ? (size_t)S.NL : (size_t)P.N;
  hipLaunchKernelGGL(mn_ro_finish, dim3(grid_for(n, 256)), dim3(256), 0, st, P, c->xw.X, S);
  MN_HIP(hipGetLastError());
  XCtl* h = c->xw.h_ctl;
  h->steps = w.h_ctl[3]; h->merges = w.h_ctl[4];
  h->tied_steps = 0; h->tied_merges = 0;           // (ties are resolved as the reference resolves them)
  h->tied_conflicts = 0;
  return MN_OK;
}

// set-up, loop and hand-over of a batch; an image whose workspace was too small is repeated with a larger one
static int run_reforder_batch(mn_context** cs, int n, const ImgParams* Ps, hipStream_t st) {
  HostBuf<mn_context*> sub((size_t)n), run((size_t)n); HostBuf<ImgParams> subP((size_t)n), runP((size_t)n);
  HostBuf<unsigned char> full((size_t)n), f2((size_t)n); HostBuf<int> idx((size_t)n);
  int rc = (sub.ok() && subP.ok() && full.ok() && run.ok() && runP.ok() && f2.ok() && idx.ok()) ? MN_OK : MN_ERR_INTERNAL, m = n;
  for (int i = 0; i < n && rc == MN_OK; i++) { sub[i] = cs[i]; subP[i] = Ps[i]; }
  for (int attempt = 0; rc == MN_OK && m > 0; attempt++) {
    if (attempt == 8) { rc = MN_ERR_CAPACITY; break; }
    for (int i = 0; i < m && rc == MN_OK; i++) rc = ro_setup(sub[i], subP[i], st);
    if (rc != MN_OK) break;
    MN_HIP(hipStreamSynchronize(st));
    memset(full, 0, (size_t)m);
    int ready = 0;                 // images whose maps were built: they go through the loop now
    for (int i = 0; i < m; i++) {
      if (sub[i]->rw.h_ctl[7] != 0) { full[i] = MN_RO_ARENA_FULL; continue; }
      run[ready] = sub[i]; runP[ready] = subP[i]; idx[ready] = i; ready++;
    }
    if (ready > 0) {
      memset(f2, 0, (size_t)ready);
      rc = ro_loop(run, ready, runP, st, f2);
      for (int j = 0; j < ready && rc == MN_OK; j++) {
        if (f2[j]) full[idx[j]] = f2[j];
        else rc = ro_finish(run[j], runP[j], st);
      }
    }
    if (rc != MN_OK) break;
    int k = 0;
    for (int i = 0; i < m; i++) {
      if (!full[i]) continue;
      mn_context::RKeep& w = sub[i]->rk;
      if (full[i] == MN_RO_ARENA_FULL) w.arena_per_pixel *= 2; else w.heap_per_record *= 2;
      sub[k] = sub[i]; subP[k] = subP[i]; k++;
    }
    m = k;
  }
  return rc;
}

// Did the run leave anything to the engine's own rule among bit-equal priorities?  Tied pops whose choices touched
// disjoint parts of the image commute (mn_kernels_exact.h, "ties"): only a tie CONFLICT can make the reference's
// heap order end elsewhere.
static bool x_ties_unresolved(const XCtl* h) {
  return h->tied_steps > 0 && (h->ttrack == 0 || h->tied_conflicts > 0);
}

// Images redone in the reference's order among equals.  `keep_ties`: they have been through the exact engine, and on
// success its tie counters -- what the exact engine met -- are put back over the zeros that ro_finish leaves.
static int redo_in_reference_order(mn_context** cs, int n, const ImgParams* Ps, hipStream_t st, bool keep_ties) {
  HostBuf<XCtl> saved((size_t)n);
  if (!saved.ok()) return MN_ERR_INTERNAL;
  for (int i = 0; i < n && keep_ties; i++) saved[i] = *cs[i]->xw.h_ctl;
  const int rc = run_reforder_batch(cs, n, Ps, st);
  for (int i = 0; i < n && keep_ties && rc == MN_OK; i++) {
    XCtl* h = cs[i]->xw.h_ctl;
    h->tied_steps = saved[i].tied_steps; h->tied_merges = saved[i].tied_merges;
    h->tied_conflicts = saved[i].tied_conflicts; h->ttrack = saved[i].ttrack;
  }
  return rc;
}

// set-up, loop and hand-over of ONE image; in a batch (mn_segment_exact_batch) set-up and loop have run for
// all images together and only the hand-over is left (xk.prerun)
static int run_exact_engine(mn_context* c, const ImgParams& P, hipStream_t st) {
  int rc = MN_OK;
  mn_context* one[1] = {c};
  c->tie_used = MN_TIES_LOWEST_ID;
  const bool ref_possible = P.variant == MN_VARIANT_CSEGMENT;       // (the Python variant's heapq / dict order is not restated)
  if (c->tie_ref == MN_TIES_REFERENCE && !c->xk.prerun) {
    if (!ref_possible) return MN_ERR_ARGUMENT;
    if ((rc = redo_in_reference_order(one, 1, &P, st, false)) != MN_OK) return rc;
    c->tie_used = MN_TIES_REFERENCE;
    MN_HIP(hipEventRecord(c->ev[1], st));
    MN_HIP(hipEventRecord(c->ev[2], st));
  } else if (!c->xk.prerun) {
    if ((rc = exact_run(one, 1, &P, st)) != MN_OK) return rc;
    // MN_TIES_DEFAULT: tied pops are the only place where the engine's order and the reference's can part; a
    // small image that had some is redone the reference's way
    long long limit = MN_TIE_LIMIT_RECORDS;
    if (const char* e = getenv("MN_TIE_LIMIT")) limit = atoll(e);
    if (c->tie_ref == MN_TIES_DEFAULT && ref_possible && x_ties_unresolved(c->xw.h_ctl) &&
        (long long)P.N * P.O <= limit) {
      if ((rc = redo_in_reference_order(one, 1, &P, st, true)) != MN_OK) return rc;
      c->tie_used = MN_TIES_REFERENCE;
    }
  } else {
    // (set-up and loop have run as part of a batch; prerun == 2: the reference-order loop too)
    if (c->xk.prerun == 2) c->tie_used = MN_TIES_REFERENCE;
    MN_HIP(hipEventRecord(c->ev[1], st));
    MN_HIP(hipEventRecord(c->ev[2], st));
  }
  return exact_export(c, P, st);
}

// Internal verdicts of a speculative attempt (never returned to the caller).
#define MN_RETRY_ROUNDS 1001   /* not sign-separable: redo with the rounds            */
#define MN_RETRY_WAIT 1002     /* more records than the finisher takes: redo, waiting for the count */
#define MN_PENDING 1003        /* deferred: everything queued, mn_segment_finish reads the verdict   */

// The options under which "a record inside a component scores > bias, one between components < bias" can hold:
// gain = omf * log-odds with omf at least `min_omf`; bias >= 0 (csegment) so that intra-component records
// (> bias) are always visible and ahead of cross records (< bias); pysegmenter divides (gain + bias) by n1*n2,
// which only separates the two kinds when bias == 0.  The contraction (components mode, cores) asks for omf >= 1e-20,
// the certificate for any omf > 0 (it passes 0 and adds the strict test).  Why the two differ is not recorded: carry-over.
static bool separable_options(const mn_options& o, float min_omf) {
  return o.object_merge_factor >= min_omf &&
         (o.variant == MN_VARIANT_CSEGMENT ? o.merge_logprob_bias >= 0.0f : o.merge_logprob_bias == 0.0f);
}

// After the stream has drained: verdict of a speculative attempt, then the statistics.
static int segment_read_back(mn_context* c, const mn_options* opts, const Queued& q, mn_stats* stats) {
  const int mode = q.mode;
  if (q.speculate) {
    if (c->h_scalars[6] != 0) return MN_RETRY_ROUNDS;
    if (c->h_scalars[7] != 0 || c->h_cnt->n_records > q.finish_limit) return MN_RETRY_WAIT;
  }
  const long long merges = (long long)q.N - (long long)c->h_scalars[2];     // every merge removes one object
  if (getenv("MN_TRACE_LABEL"))
    fprintf(stderr, "labelling: unions asked for -- vertical borders %d, horizontal borders %d, other offsets %d\n",
            c->h_scalars[10], c->h_scalars[11], c->h_scalars[12]);
  const int rc = c->h_cnt->error != 0 ? c->h_cnt->error : MN_OK;
  if (stats) {
    stats->status = rc;
    stats->mode_used = mode;
    const bool cert_opts = opts->object_merge_factor > 0.0f && separable_options(*opts, 0.0f);
    stats->cert_edge_violations = c->h_scalars[0];
    stats->cert_class_violations = c->h_scalars[3];
    stats->cert_record_violations = c->h_scalars[4];
    stats->certified = (q.want_cert && c->h_scalars[0] == 0 && c->h_scalars[3] == 0 && c->h_scalars[4] == 0 && cert_opts) ? 1 : 0;
    // 2 only where the pop order was forced or the reference's own order among equals was run; an exact-engine
    // result that met tied pops under its own lowest-id rule says 3 (advisor r3 / verdict r3: a held vector
    // shows the two rules can part)
    stats->proof = MN_PROOF_NONE;
    if (stats->certified) stats->proof = MN_PROOF_CERTIFICATE;
    else if (mode == MN_MODE_EXACT && c->xw.h_ctl)
      stats->proof = (c->tie_used == MN_TIES_REFERENCE || c->xw.h_ctl->tied_steps == 0 ||
                      (c->xw.h_ctl->ttrack != 0 && c->xw.h_ctl->tied_conflicts == 0)) ? MN_PROOF_SEQUENTIAL
                                                                                       : MN_PROOF_SEQUENTIAL_TIES;
    stats->num_instances = c->h_scalars[1];
    stats->num_objects = c->h_scalars[2];
    stats->rounds = q.rounds;
    stats->cores_condemned = c->cores_used ? (c->h_scalars[9] != 0) : 0;
    stats->finisher_steps = c->h_cnt->finisher_steps;
    stats->tied_steps = stats->tied_merges = stats->tied_conflicts = 0;
    stats->tie_order_used = 0;
    if (mode == MN_MODE_EXACT && c->xw.h_ctl) {
      stats->tie_order_used = c->tie_used;
      const long long ts = c->xw.h_ctl->tied_steps, tm = c->xw.h_ctl->tied_merges;
      stats->tied_steps = (int)(ts > 0x7FFFFFFF ? 0x7FFFFFFF : ts);
      stats->tied_merges = (int)(tm > 0x7FFFFFFF ? 0x7FFFFFFF : tm);
      // (tracking switched off by the environment: unknown, reported as a conflict wherever a pop was tied)
      const long long tc = c->xw.h_ctl->tied_conflicts;
      stats->tied_conflicts = (c->xw.h_ctl->ttrack == 0 && tc == 0 && ts > 0) ? 1 : (int)(tc > 0x7FFFFFFF ? 0x7FFFFFFF : tc);
    }
    stats->initial_records = q.R0;
    stats->merges = merges;
    stats->total_logprob = q.want_cert ? c->h_lp[0] : NAN;
    float ms = 0;
    const bool cmode = mode == MN_MODE_COMPONENTS || c->cores_used;   // (no separate scoring phase: ev[1], ev[2] not recorded)
    if (c->cores_used && !(opts->debug_flags & MN_DEBUG_NO_EVENTS)) {
      (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[10]); stats->ms_edge_pass = ms;    // the sweep: class + sameness planes
    }
    if (!cmode) {
      (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]); stats->ms_class_pass = ms;
      (void)hipEventElapsedTime(&ms, c->ev[1], c->ev[2]); stats->ms_edge_pass = ms;
    }
    stats->ms_score = stats->ms_class_pass + stats->ms_edge_pass;
    const bool lean = (opts->debug_flags & MN_DEBUG_LEAN_EVENTS) != 0 && q.speculate && mode == MN_MODE_COMPONENTS &&
                      opts->variant == MN_VARIANT_CSEGMENT;      // (only ev[0], ev[10] were recorded)
    if (!lean) {
      (void)hipEventElapsedTime(&ms, c->ev[cmode ? 0 : 2], c->ev[3]); stats->ms_merge = ms;
      (void)hipEventElapsedTime(&ms, c->ev[3], c->ev[4]); stats->ms_output = ms;
      (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[4]); stats->ms_total = ms;
    }
    if (mode == MN_MODE_COMPONENTS && !(opts->debug_flags & MN_DEBUG_NO_EVENTS)) {
      (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[10]); stats->ms_cc_edges = ms;
      if (!(opts->debug_flags & MN_DEBUG_LEAN_EVENTS)) {
        (void)hipEventElapsedTime(&ms, c->ev[10], c->ev[7]); stats->ms_cc_label = ms;
        (void)hipEventElapsedTime(&ms, c->ev[11], c->ev[8]); stats->ms_cc_sums = ms;
        (void)hipEventElapsedTime(&ms, c->ev[8], c->ev[9]); stats->ms_cc_cross = ms;
      }
    }
  }
  return done(rc);
}

struct Plan {              // everything an attempt decides before its first launch
  int mode;                // MN_MODE_EXACT / ROUNDS / COMPONENTS, resolved (a waited contraction can still fall back)
  bool xengine;            // the sequential order at any size: the exact engine
  bool speculate;          // nothing is waited for before the one synchronisation at the end
  bool fused_tail;         // the speculative attempt of the C++ variant ends in mn_cc_tail
  bool cores_ok;           // the general rounds may start from the cores (mn_core_clean) instead of from single pixels
  bool want_cert, lean;    // lean: only the sweep is timed
  int finish_limit, rounds_limit, exact_limit, subrounds;
  float band_gamma; long long R0;     // R0: records of the pixel graph
};

static Plan make_plan(const ImageCall& call, int force_mode, bool speculate) {
  const mn_options* opts = &call.opts;
  Plan pl;
  pl.R0 = count_records(call);
  pl.exact_limit = opts->exact_limit > 0 ? opts->exact_limit : 32768;
  pl.finish_limit = opts->finish_limit > 0 ? opts->finish_limit : 4096;
  // hand-over of the general rounds: since the rounds start from the cores a late round is cheap, and
  // 2048 records beat 4096 (10.0 against 11.6 ms on a blurred 1024x2048 map; 1536: 9.7 ms)
  pl.rounds_limit = opts->finish_limit > 0 ? opts->finish_limit : 2048;
  pl.subrounds = opts->subrounds > 0 ? opts->subrounds : 32;
  if (pl.subrounds > MN_MAX_SUBROUNDS) pl.subrounds = MN_MAX_SUBROUNDS;
  pl.band_gamma = opts->band_permille > 0 ? opts->band_permille * 1e-3f
                                          : (opts->band_permille < 0 ? 0.0f : 0.05f);
  pl.mode = force_mode > 0 ? force_mode : opts->mode;
  if (pl.mode != MN_MODE_EXACT && pl.mode != MN_MODE_ROUNDS && pl.mode != MN_MODE_COMPONENTS)
    pl.mode = (pl.R0 <= pl.exact_limit) ? MN_MODE_EXACT : MN_MODE_COMPONENTS;
  // the component contraction needs separable_options
  // (and N <= 2^26: a component's class sums are 2^-32 fixed point in 64 bits, |log p| <= 16)
  const bool contractible = call.W * call.H <= (1 << 26) && separable_options(*opts, 1e-20f);
  if (pl.mode == MN_MODE_COMPONENTS && !contractible) pl.mode = MN_MODE_ROUNDS;
  pl.xengine = pl.mode == MN_MODE_EXACT;
  // the same conditions let the general rounds start from the cores (mn_core_clean) instead of from
  // single pixels; MN_DEBUG_NO_CORES keeps the round on the implicit pixel graph
  pl.cores_ok = contractible && !(opts->debug_flags & MN_DEBUG_NO_CORES);
  pl.speculate = speculate && pl.mode == MN_MODE_COMPONENTS && pl.finish_limit <= MN_FIN2_MAXR;
  pl.fused_tail = pl.speculate && opts->variant == MN_VARIANT_CSEGMENT;
  pl.want_cert = opts->compute_logprob != 0;
  pl.lean = (opts->debug_flags & MN_DEBUG_LEAN_EVENTS) != 0 && pl.fused_tail;
  return pl;
}

struct Attempt {           // what an attempt carries from one stage to the next
  hipStream_t st;          // where the next launch goes (run_components moves it to the side / capture stream)
  int mode;                // Plan::mode, or the rounds after a contraction that did not hold
  bool cores;              // the rounds start from the cores
  RecList cur, nxt;        // record list in use / the one the next round builds
  int rounds, R;           // R: records in `cur` (speculating: the most the finisher takes)
  FillList fills, post;    // what is cleared in ONE launch before the first kernel; the same again, for the end of a fused attempt
  // (mn_cc_certificate: from what the contraction and the LDS finisher left, not from a sweep)
  bool cc_certificate() const { return mode == MN_MODE_COMPONENTS && rounds == 0 && R <= MN_FIN2_MAXR; }
};

// What the attempt expects cleared before its first kernel, as ONE fill launch (A.fills).
static void build_clear_list(mn_context* c, const ImgParams& P, const Plan& pl, Attempt& A) {
  FillList& fills = A.fills;
  fills.add(c->cnt, sizeof(Counters), 0);
  fills.add(c->scalars, MN_NSCALARS * sizeof(int), 0);
  if (pl.mode != MN_MODE_COMPONENTS)
    fills.add(c->mapbuf, (size_t)P.N * sizeof(int), 0xFF);    // (object -> record) map of mn_finisher
  if (pl.mode == MN_MODE_COMPONENTS) {
    // everything the contraction and the compaction after it expect cleared, in the same launch.
    // Records between components are few: the speculative attempt, which only stands with at
    // most finish_limit of them, takes a table of 8x that many slots (less to clear, less for
    // mn_compact to scan); the ordinary attempt one of N/8.  A table that fills up fails the
    // bounded insert, counted apart from the separability violations (scalars[7]).
    // (the speculative attempt ends in mn_cc_tail, whose lanes hold MN_TAIL_TABLE_CAP / 1024 slots each)
    size_t cap = pl.fused_tail ? (size_t)MN_TAIL_TABLE_CAP
                               : (pl.speculate ? next_pow2((size_t)pl.finish_limit * 8) : next_pow2((size_t)P.N / 8 + 8192));
    if (cap > c->cc_cap_max) cap = c->cc_cap_max;
    c->cc_cap = cap;
    fills.add(c->T.key, cap * sizeof(u64), 0xFF);
    fills.add(c->T.S, cap * sizeof(i64), 0);
    fills.add(c->T.touched, cap, 0);
    fills.add(c->cc_tcount, cap * sizeof(int), 0);
    if (!pl.speculate) {
      // best-record slots: only if more records may be left than the finisher takes, so that the
      // rounds go on from this list and look at all N slots (the speculative attempt never does:
      // it is redone on this path instead)
      fills.add(c->ball, (size_t)P.N * sizeof(u64), 0);
      fills.add(c->gmax, 64 * sizeof(unsigned), 0);
    }
  }
  // A fused speculative attempt clears the same few kilobytes again at its END, on the side stream
  // (after the statistics have been copied out): the next one starts with its sweep over the
  // sameness planes instead of a fill kernel and the dispatch gap behind it.
  A.post = fills;
  if (pl.fused_tail && c->cc_clean) fills.j.count = 0;
  c->cc_clean = 0;                 // (set again only when this attempt has queued its own clean-up)
}

// Phase A: the exact engine from start to end, or the scoring passes / the contraction (with its fall-back to the rounds).
static int run_first_phase(mn_context* c, const ImgParams& P, const Plan& pl, Attempt& A) {
  FillList& fills = A.fills;
  int rc;
  if (A.cores) fills.add(c->touch, 64 * sizeof(unsigned), 0);        // (edges outside the cores: mn_core_bits)
  if (pl.xengine) {
    fills.launch(A.st);
    MN_HIP(hipEventRecord(c->ev[0], A.st));
    rc = run_exact_engine(c, P, A.st);
  } else {
    rc = run_phase_a(c, P, A.st, A.mode == MN_MODE_ROUNDS && !A.cores, &fills, A.mode == MN_MODE_COMPONENTS || A.cores);
  }
  if (rc != MN_OK) return rc;
  if (A.mode == MN_MODE_COMPONENTS) {
    rc = run_components(c, P, A.st, !pl.speculate ? CC_WAITED : (pl.fused_tail ? CC_QUEUED_TAIL : CC_QUEUED_COMPACT));
    if (rc < 0) return rc;
    if (rc == 1) {                 // not sign-separable: start over with the general rounds
      A.mode = MN_MODE_ROUNDS;
      A.cores = pl.cores_ok;
      FillList none;
      if (A.cores) none.add(c->touch, 64 * sizeof(unsigned), 0);
      if ((rc = run_phase_a(c, P, A.st, !A.cores, &none, A.cores)) != MN_OK) return rc;
    }
  }
  if (A.cores) {
    // sweep + labelling of the cores + their class sums and object state; nothing is waited for
    if ((rc = run_components(c, P, A.st, CC_CORES)) < 0) return rc;
    c->cores_used = 1;
  }
  return MN_OK;
}

// Round 0 of the general rounds (the contraction of the cores stands for it where they are used).
static int run_round0(mn_context* c, const ImgParams& P, const Plan& pl, Attempt& A) {
  if (A.mode != MN_MODE_ROUNDS) return MN_OK;
  const int N = P.N;
  if (!A.cores) {
    // round 0 on the implicit pixel graph: matching sub-rounds, then one apply
    MN_HIP(hipMemsetAsync(c->progress, 0, MN_MAX_SUBROUNDS * sizeof(int), A.st));
    hipLaunchKernelGGL(mn_pix_match, dim3(grid_for(N, 256)), dim3(256), 0, A.st, N,
                       (const u64*)c->ball, c->matched, c->mate, c->progress, 0, c->cnt);
    for (int s = 1; s < pl.subrounds; s++) {
      launch_edge_pass<false>(c, P, A.st, c->bsub, s);
      hipLaunchKernelGGL(mn_pix_match, dim3(grid_for(N, 256)), dim3(256), 0, A.st, N,
                         (const u64*)c->bsub, c->matched, c->mate, c->progress, s, c->cnt);
    }
    hipLaunchKernelGGL(mn_pix_apply, dim3(grid_for(N, 256)), dim3(256), 0, A.st, P, obj_state(c), (const int*)c->mate, c->cnt);
  }
  A.rounds = 1;
  return MN_OK;
}

// The first record list, then rounds until the finisher can take what is left: A.cur, A.R, A.rounds.
static int run_rounds(mn_context* c, const ImgParams& P, const Plan& pl, Attempt& A) {
  if (pl.xengine) return MN_OK;      // (the engine has no list: R stays 0)
  const int N = P.N;
  const hipStream_t st = A.st;
  int &R = A.R, rc;
  if (A.mode == MN_MODE_COMPONENTS) {
    // run_components already compacted the table into the list; speculating, the count is still
    // on the device: launches below are sized for the most the finisher takes
    R = pl.speculate ? pl.finish_limit : c->h_cnt->n_records;
  } else {
    size_t cap0 = next_pow2((size_t)pl.R0 + (size_t)pl.R0 / 4 + 1024);
    if (A.cores && pl.R0 > (1 << 18)) {   // only the edges outside the cores become records: worth a round trip
      MN_HIP(hipMemcpyAsync(c->h_touch, c->touch, 64 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
      MN_HIP(hipStreamSynchronize(st));
      size_t need = 0;
      for (int w = 0; w < 64; w++) need += c->h_touch[w];
      cap0 = next_pow2(need + need / 2 + 1024);
    }
    if ((rc = build_list(c, P, st, cap0 < c->cap ? cap0 : c->cap, A.cur, nullptr, 0, &R)) != MN_OK) return rc;
  }
  bool first_round = true;
  int productive = pl.subrounds;    // matching sub-rounds of the previous round that paired anything, + 1
  // (a list the finisher can take whole goes to it at once: the sequential order itself; the lower
  //  hand-over only applies once the rounds are running)
  int loop_limit = pl.finish_limit;
  while (!pl.speculate && R > loop_limit && A.rounds < 5000) {
    if (A.mode != MN_MODE_COMPONENTS || A.rounds > 0) loop_limit = pl.rounds_limit;
    {
      FillList f;                // one launch instead of five memsets
      f.add(c->matched, N, 0);
      f.add(c->mate, (size_t)N * sizeof(int), 0xFF);
      f.add(c->cnt, 4 * sizeof(int), 0);                       // n_records, any_selected, ...
      f.add(c->progress, MN_MAX_SUBROUNDS * sizeof(int), 0);
      f.add(c->touch, 64 * sizeof(unsigned), 0);
      if (first_round) f.add(c->bsub, (size_t)N * sizeof(u64), 0);   // (accept leaves it clean for the next round)
      f.launch(st);
      first_round = false;
    }
    const dim3 g(grid_for(R, 256)), b(256), go(grid_for(N, 256));
    hipLaunchKernelGGL(mn_band_threshold, dim3(1), dim3(64), 0, st, (const unsigned*)c->gmax,
                       P.bias, P.variant, pl.band_gamma, c->theta);
    hipLaunchKernelGGL(mn_obj_match_mutual, go, b, 0, st, N, (const u64*)c->ball,
                       (const float*)c->theta, c->matched, c->mate, c->progress, c->cnt);
    // late rounds are launch-bound: fewer matching sub-rounds once the list is small
    // ... and a sub-round is two launches that return at once when the one before paired nothing:
    // how far the previous round got (read back with its counters) bounds this one, plus a margin
    int sub_r = R > (1 << 20) ? pl.subrounds : (pl.subrounds > 8 ? pl.subrounds / 4 : pl.subrounds);
    if (sub_r > productive + 3) sub_r = productive + 3;
    for (int s = 1; s < sub_r; s++) {
      hipLaunchKernelGGL(mn_obj_propose, go, b, 0, st, N, (const u64*)c->ball, (const float*)c->theta,
                         (const unsigned char*)c->matched, c->bsub, (const int*)c->progress, s, c->cnt);
      hipLaunchKernelGGL(mn_obj_accept, go, b, 0, st, N, c->bsub, c->matched, c->mate, c->progress, s, c->cnt);
    }
    hipLaunchKernelGGL(mn_rec_apply, g, b, 0, st, P, obj_state(c), A.cur, R, (const int*)c->mate, c->cnt, c->touch);
    // the table only takes the records with a matched object at an end (the others go straight to
    // the next list): for a big list it is worth a host round trip to size it for those
    size_t need = (size_t)R;
    if (R > (1 << 18)) {
      MN_HIP(hipMemcpyAsync(c->h_touch, c->touch, 64 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
      MN_HIP(hipStreamSynchronize(st));
      need = 0;
      for (int w = 0; w < 64; w++) need += c->h_touch[w];
    }
    size_t cap = next_pow2(need + need / 2 + 1024);   // load <= 2/3
    if (cap > c->cap) cap = c->cap;
    int Rn = 0;
    MN_HIP(hipMemcpyAsync(c->h_touch + 64, c->progress, MN_MAX_SUBROUNDS * sizeof(int), hipMemcpyDeviceToHost, st));
    if ((rc = build_list(c, P, st, cap, A.nxt, &A.cur, R, &Rn)) != MN_OK) return rc;
    productive = 1;
    for (int w = 1; w < sub_r; w++)
      if (c->h_touch[64 + w]) productive = w + 1;
    if (getenv("MN_TRACE_ROUNDS"))
      fprintf(stderr, "round %d: R %d -> %d, sub-rounds used %d of %d\n", A.rounds, R, Rn, productive, sub_r);
    A.rounds++;
    const int selected = c->h_cnt->any_selected;
    RecList t = A.cur; A.cur = A.nxt; A.nxt = t;
    R = Rn;
    if (selected == 0) break;     // nothing visible any more: the queue is empty
  }
  return MN_OK;
}

// Sequential lazy-greedy on what is left: mn_cc_tail, mn_finisher_lds or mn_finisher by the attempt and its list's length.
static int launch_finisher(mn_context* c, const ImgParams& P, const Plan& pl, const Attempt& A, const ImageCall& call) {
  const ObjState S = obj_state(c);
  const long long max_steps = 64LL * (pl.R0 > 0 ? pl.R0 : 1) + 4096;
  if (pl.xengine) {
    // (the engine has run to the end of the queue)
  } else if (pl.fused_tail) {
    if (!c->tail_lds_ready) {
      MN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mn_cc_tail),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, MN_FIN2_MAXR * 12));
      c->tail_lds_ready = 1;
    }
    const HashTab T = table_of(c, c->cc_cap);
    const int nbe = c->cc_sweep.waves;
    hipLaunchKernelGGL(mn_cc_tail, dim3(1), dim3(MN_FIN2_THREADS), MN_FIN2_MAXR * 12, A.st, P, S, T, (const int*)c->cc_tcount,
                       A.cur, c->cc_lcount, c->label, c->fin_lists, c->cnt, max_steps, c->scalars, pl.finish_limit,
                       (const unsigned char*)c->cls0, (const int*)c->mate, (const int*)c->cc_roots, nbe,
                       (const double*)c->partial, c->lp_out, pl.want_cert ? 1 : 0, c->label, call.d_objcls);
  } else {
    // (records that come straight from the component contraction were scored a moment ago)
    if (A.mode != MN_MODE_EXACT && A.R > 0 && !call.opts.no_handover_refresh &&
        !(A.mode == MN_MODE_COMPONENTS && A.rounds == 0))
      hipLaunchKernelGGL(mn_rec_refresh, dim3(grid_for(A.R, 256)), dim3(256), 0, A.st, P, S, A.cur, A.R);
    if (A.R <= MN_FIN2_MAXR) {
      // record list resident in LDS (96 KiB dynamic); the (object -> record) map lives in `label`
      if (!c->fin_lds_ready) {
        MN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mn_finisher_lds),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, MN_FIN2_MAXR * 12));
        c->fin_lds_ready = 1;
      }
      hipLaunchKernelGGL(mn_finisher_lds, dim3(1), dim3(MN_FIN2_THREADS), MN_FIN2_MAXR * 12, A.st, P, S, A.cur, A.R, c->label,
                         c->fin_lists, c->cnt, max_steps, pl.speculate ? (const int*)&c->cnt->n_records : (const int*)nullptr,
                         (const int*)(c->scalars + 6), pl.finish_limit,
                         (A.mode == MN_MODE_COMPONENTS && A.rounds == 0) ? c->cc_lcount : (int*)nullptr);
    } else {
      if (A.mode == MN_MODE_COMPONENTS || A.cores)   // (the class range of the contraction lived there)
        MN_HIP(hipMemsetAsync(c->mapbuf, 0xFF, (size_t)P.N * sizeof(int), A.st));
      hipLaunchKernelGGL(mn_finisher, dim3(1), dim3(MN_FIN_THREADS), 0, A.st, P, S, A.cur, A.R, c->mapbuf,
                         c->touched_list, c->cnt, max_steps);
    }
  }
  if (!pl.lean) MN_HIP(hipEventRecord(c->ev[3], A.st));
  return MN_OK;
}

// Output stage: pruning (pysegmenter), instance ranks, mask / class table / partition.
static int launch_output(mn_context* c, const ImgParams& P, const Plan& pl, const Attempt& A, const ImageCall& call) {
  const int N = P.N;
  const ObjState S = obj_state(c);
  const unsigned char* pruned = NULL;
  if (call.opts.variant == MN_VARIANT_PYSEGMENTER) {
    MN_HIP(hipMemsetAsync(c->bg_key, 0, sizeof(u64), A.st));
    hipLaunchKernelGGL(mn_prune_find_background, dim3(grid_for(N, 256)), dim3(256), 0, A.st, P, S, c->bg_key);
    hipLaunchKernelGGL(mn_prune_mark, dim3(grid_for(N, 256)), dim3(256), 0, A.st, P, S,
                       call.opts.prune_threshold, (const u64*)c->bg_key, c->pruned, c->cnt);
    pruned = c->pruned;
  }
  if (!pl.fused_tail) {
    const int nblk = (int)grid_for(N, MN_SCAN_ITEMS);
    hipLaunchKernelGGL(mn_rank_count, dim3(nblk), dim3(256), 0, A.st, N, S, pruned, c->block_count, c->scalars + 2);
    hipLaunchKernelGGL(mn_rank_scan, dim3(1), dim3(1024), 0, A.st, nblk, c->block_count, c->scalars + 1);
    hipLaunchKernelGGL(mn_rank_assign, dim3(nblk), dim3(256), 0, A.st, N, S, pruned,
                       (const int*)c->block_count, c->label, call.d_objcls);
  }
  {
    // (the per-pixel roots are only read by the per-pixel certificate below)
    const bool need_root = pl.want_cert && !pl.fused_tail && !A.cc_certificate();
    int* root_out = need_root ? c->root : nullptr;
    const bool aligned = (N & 3) == 0 && ((reinterpret_cast<uintptr_t>(call.d_mask) | reinterpret_cast<uintptr_t>(call.d_objcls) |
                                           reinterpret_cast<uintptr_t>(call.d_part)) & 15) == 0;
    if (aligned)
      hipLaunchKernelGGL(mn_write_mask4, dim3(grid_for((size_t)N / 4, 256)), dim3(256), 0, A.st, N, (const int*)c->parent,
                         (const int*)c->label, (const int*)(c->scalars + 1), root_out, call.d_mask, call.d_part, call.d_objcls);
    else
      hipLaunchKernelGGL(mn_write_mask, dim3(grid_for(N, 256)), dim3(256), 0, A.st, N, (const int*)c->parent,
                         (const int*)c->label, (const int*)(c->scalars + 1), root_out, call.d_mask, call.d_part, call.d_objcls);
  }
  return MN_OK;
}

// certificate + log-likelihood (skipped on request: compute_logprob = 0, the drop-in entry's
// setting -- the reference's c_run_segmentation returns neither)
static int launch_certificate(mn_context* c, const ImgParams& P, const Plan& pl, const Attempt& A) {
  const int N = P.N, R = A.R;
  const ObjState S = obj_state(c);
  if (!pl.want_cert || pl.fused_tail) {
  } else if (A.cc_certificate()) {
    // no further sweep over the sameness planes: the edge sweep of the contraction left the sums
    // for the components and the finisher what the merged records moved (mn_cc_certificate)
    const int nbe = c->cc_sweep.waves;
    hipLaunchKernelGGL(mn_cc_certificate, dim3(1), dim3(MN_CC_CERT_THREADS), 0, A.st, P, S, (const unsigned char*)c->cls0,
                       (const int*)c->mate, (const int*)c->cc_roots, (const int*)(c->scalars + 8), nbe,
                       (const double*)c->partial, (const Counters*)c->cnt, c->lp_out, c->scalars);
  } else {
    const bool four = P.W % 4 == 0;              // 4 pixels of one row per lane
    const int vb = (int)grid_for(four ? (size_t)N / 4 : (size_t)N, four ? MN_VERIFY4_THREADS : 256);
    if (four)
      hipLaunchKernelGGL(mn_verify_edges4, dim3(vb), dim3(MN_VERIFY4_THREADS), 0, A.st, P, S,
                         (const unsigned char*)c->cls0, (const int*)c->root, c->partial, c->scalars);
    else
      hipLaunchKernelGGL(mn_verify_edges, dim3(vb), dim3(256), 0, A.st, P, S,
                         (const unsigned char*)c->cls0, (const int*)c->root, c->partial, c->scalars);
    hipLaunchKernelGGL(mn_verify_reduce, dim3(1), dim3(256), 0, A.st, vb, (const double*)c->partial, P.omf, c->lp_out);
    if (pl.xengine)
      hipLaunchKernelGGL(mn_x_verify_records, dim3(grid_for((size_t)c->xw.X.NL, 256)), dim3(256), 0, A.st, P,
                         c->xw.X, c->scalars);
  }
  if (pl.want_cert && !pl.fused_tail && R > 0)      // (either form ends with the records the finisher was given)
    hipLaunchKernelGGL(mn_verify_records, dim3(grid_for(R, 256)), dim3(256), 0, A.st, P, S, A.cur, R,
                       c->scalars, pl.speculate ? (const int*)&c->cnt->n_records : (const int*)nullptr);
  if (!pl.lean) MN_HIP(hipEventRecord(c->ev[4], A.st));
  MN_HIP(hipGetLastError());
  return MN_OK;
}

// Statistics copied out, the fused attempt's clean-up queued, a recording closed; then MN_PENDING or wait and read back.
static int close_attempt(mn_context* c, const ImageCall& call, const Plan& pl, Attempt& A, mn_stats* stats, bool defer) {
  hipStream_t st = A.st;
  const Queued q = {A.mode, A.rounds, pl.finish_limit, call.W * call.H, pl.R0, pl.speculate, pl.want_cert};
  MN_HIP(hipMemcpyAsync(c->h_statblk, c->statblk, c->stat_bytes, hipMemcpyDeviceToHost, st));
  if (pl.fused_tail) {             // (st is the side stream here)
    A.post.launch(st);
    c->cc_clean = 1;
  }
  if (c->replay.capturing) {       // (graph B: on the side stream, where the image forked)
    const int rc = replay_end(c, &c->replay.gB, &c->replay.eB, st);
    if (rc != MN_OK) return rc;
    c->replay.capturing = 0;
    c->replay.state = 2;
    c->replay.queued = q;
  }
  if (defer && pl.speculate) {
    MN_HIP(hipEventRecord(c->ev_done, st));
    c->pend.queued = q;
    return MN_PENDING;
  }
  MN_HIP(hipStreamSynchronize(st));
  return segment_read_back(c, &call.opts, q, stats);
}

// One attempt at an image, as a sequence of stages on one stream.  `speculate`: in components mode the host does
// not wait for the record count and the separability verdict in the middle of the image; finisher and output are
// queued behind the contraction and everything is read at the one synchronisation at the end.  Sign-separable maps
// with few components -- the case the mode exists for -- are done then; otherwise a verdict above is returned and
// mn_segment_finish runs the attempt again on the ordinary path.  `defer` (with a speculative attempt only): return
// MN_PENDING as soon as everything is queued; the caller reads back later with segment_read_back after waiting for ev_done.
static int segment_attempt(mn_context* c, const ImageCall& call, mn_stats* stats, int force_mode, bool speculate, bool defer = false) {
  ImgParams P;
  int rc = begin_call(c, call, call.d_mask && call.d_objcls, stats, &P);
  if (rc != MN_OK) return rc;           // (refused before anything ran: the scores of the image before stay available)
  scores_stale(c);                      // an attempt that fails half-way leaves the context refusing
  // (development aid: MN_DEBUG_FLAGS_OR in the environment is OR-ed into debug_flags, so that a whole
  //  test run can be put through an opt-in code path)
  static const int env_flags = getenv("MN_DEBUG_FLAGS_OR") ? atoi(getenv("MN_DEBUG_FLAGS_OR")) : 0;
  c->debug_flags = call.opts.debug_flags | env_flags;
  c->ext_events = !(call.opts.debug_flags & (MN_DEBUG_NO_EVENTS | MN_DEBUG_SWEEP_EVENT_PACKETS));
  c->core_radius = call.opts.core_radius != 0 ? call.opts.core_radius : MN_DEFAULT_CORE_RADIUS;
  const Plan pl = make_plan(call, force_mode, speculate);
  c->tie_ref = pl.xengine ? call.opts.tie_order : MN_TIES_LOWEST_ID;
  c->tie_used = 0; c->cores_used = 0;
  if (!pl.xengine && (rc = ensure_fast(c)) != MN_OK) return rc;
  // everything but the speculative components attempt and the exact engine works on full-size record lists
  if (!pl.speculate && !pl.xengine && (rc = ensure_general(c)) != MN_OK) return rc;
  Attempt A = {call.stream, pl.mode, pl.mode == MN_MODE_ROUNDS && pl.cores_ok, c->LA, c->LB, 0, 0};
  build_clear_list(c, P, pl, A);
  if ((rc = run_first_phase(c, P, pl, A)) != MN_OK) return rc;
  if ((rc = run_round0(c, P, pl, A)) != MN_OK) return rc;
  if ((rc = run_rounds(c, P, pl, A)) != MN_OK) return rc;
  if ((rc = launch_finisher(c, P, pl, A, call)) != MN_OK) return rc;
  if ((rc = launch_output(c, P, pl, A, call)) != MN_OK) return rc;
  if ((rc = launch_certificate(c, P, pl, A)) != MN_OK) return rc;
  c->last_params = P;
  rc = close_attempt(c, call, pl, A, stats, defer);
  // (MN_PENDING: mn_segment_finish reads the verdict, and clears the flag again if it is not MN_OK)
  if (rc == MN_OK || rc == MN_PENDING) c->last_valid = 1;
  return rc;
}

// The image of last time again, through the same buffers: the sweep between its events, then the two graphs.
static int replay_launch(mn_context* c, const ImageCall& call) {
  ImgParams P;
  const int rc = begin_call(c, call, true, nullptr, &P);
  if (rc != MN_OK) return rc;
  scores_stale(c);
  const hipStream_t st = call.stream;
  c->debug_flags = call.opts.debug_flags;      // (deliberate carry-over: without MN_DEBUG_FLAGS_OR, unlike segment_attempt)
  c->ext_events = !(call.opts.debug_flags & (MN_DEBUG_NO_EVENTS | MN_DEBUG_SWEEP_EVENT_PACKETS));
  c->cores_used = 0;
  const bool timed = !(call.opts.debug_flags & MN_DEBUG_NO_EVENTS) && !c->ext_events;
  if (timed) MN_HIP(hipEventRecord(c->ev[0], st));
  // (the key holds buffers, dtype and options: the recorded form, lean or full as the graphs expect it)
  launch_sweep(c, P, st, c->replay.sweep);
  if (timed) MN_HIP(hipEventRecord(c->ev[10], st));
  MN_HIP(hipGraphLaunch(c->replay.eA, st));
  MN_HIP(hipEventRecord(c->ev_fork, st));
  MN_HIP(hipStreamWaitEvent(c->side, c->ev_fork, 0));
  MN_HIP(hipGraphLaunch(c->replay.eB, c->side));
  MN_HIP(hipEventRecord(c->ev_done, c->side));
  c->last_params = P; c->last_valid = 1;
  c->pend.queued = c->replay.queued;
  memset(&c->pend.stats, 0, sizeof(c->pend.stats));
  c->pend.active = 1;
  return MN_OK;
}

// What two calls must share for the second to replay the first: buffers, stream, shape, element type (with
// MN_MAPS_LOGITS: a logits call never replays a probability call's graphs), options, offsets.  Bytes used of
// key[256]; 0: an offset list too long for it (no replay).
static size_t replay_key(const ImageCall& call, unsigned char* key) {
  memset(key, 0, 256);
  const void* ptrs[6] = {call.d_class, call.d_adj, call.d_mask, call.d_objcls, call.d_part, call.stream};
  const int dims[6] = {call.class_dim, call.offset_dim, call.W, call.H, call.num_classes, call.dtype};
  size_t kb = 0;
  memcpy(key + kb, ptrs, sizeof(ptrs)); kb += sizeof(ptrs);
  memcpy(key + kb, dims, sizeof(dims)); kb += sizeof(dims);
  memcpy(key + kb, &call.opts, sizeof(call.opts)); kb += sizeof(call.opts);
  const size_t ob = sizeof(int) * 2 * (size_t)call.offset_dim;
  if (kb + ob > 256) return 0;
  memcpy(key + kb, call.offs, ob);
  return kb + ob;
}

// First half: queue everything for one image and return.  In components mode (the default for
// large images) nothing has been waited for when this returns; other modes run to completion here.
// The context is busy until mn_segment_finish; inputs and outputs must stay alive until then.
extern "C" int mn_segment_launch_t(mn_context* c, const void* d_class_pred, int class_dim,
                                   const void* d_adj_pred, int offset_dim, int dtype, int W, int H,
                                   int num_classes, const int* offset_list, int* d_mask,
                                   int* d_object_class, int* d_partition, const mn_options* opts,
                                   void* stream) {
  if (!c || c->pend.active || !dtype_ok(dtype, true)) return done(MN_ERR_ARGUMENT);
  HostLaunchTimer host_timer;
  mn_context::Pending& q = c->pend;
  q.call = ImageCall{d_class_pred, d_adj_pred, dtype, class_dim, offset_dim, W, H, num_classes, d_mask, d_object_class, d_partition};
  image_call(&q.call, offset_list, opts, stream);
  const mn_options& o = q.call.opts;
  // ---- replay (MN_DEBUG_REPLAY, with MN_DEBUG_LEAN_EVENTS): see mn_context::Replay ----
  mn_context::Replay& rp = c->replay;
  const bool want_replay = (o.debug_flags & MN_DEBUG_REPLAY) && (o.debug_flags & MN_DEBUG_LEAN_EVENTS) && offset_list &&
                           offset_dim > 0 && offset_dim <= MN_MAX_OFFSETS && W % 4 == 0;
  unsigned char key[256];
  const size_t kb = want_replay ? replay_key(q.call, key) : 0;
  const bool same_key = want_replay && kb && rp.state >= 1 && rp.key_bytes == kb && memcmp(rp.key, key, kb) == 0;
  if (same_key && rp.state == 2 && c->cc_clean) return replay_launch(c, q.call);
  if (want_replay && kb && !same_key) drop_replay_graphs(rp);      // a new key: forget the graphs of the old one
  // second identical call in the steady state (the counters were cleared by the previous image): record
  rp.capturing = (same_key && rp.state == 1 && c->cc_clean) ? 1 : 0;
  const int was_clean = c->cc_clean;
  const int rc = segment_attempt(c, q.call, &q.stats, 0, true, true);
  if (rp.capturing) replay_abandon(rp);      // the attempt did not take the fused path after all, or failed half-way
  if (want_replay && kb && rp.state == 0 && rc == MN_PENDING && was_clean && c->cc_clean &&
      o.variant == MN_VARIANT_CSEGMENT && (W * H) % 4 == 0) {
    memcpy(rp.key, key, kb);       // a fused speculative attempt in the steady state: the next one records
    rp.key_bytes = kb;
    rp.state = 1;
  }
  if (rc == MN_PENDING) { q.active = 1; return MN_OK; }
  if (rc < 0 && rc != MN_ERR_NO_BACKGROUND) return rc;   // rejected or failed: nothing is pending
  q.active = 2;                       // ran to completion on the ordinary path
  q.rc = rc;
  return MN_OK;
}

extern "C" int mn_segment_launch(mn_context* c, const float* d_class_pred, int class_dim,
                                 const float* d_adj_pred, int offset_dim, int W, int H,
                                 int num_classes, const int* offset_list, int* d_mask,
                                 int* d_object_class, int* d_partition, const mn_options* opts,
                                 void* stream) {
  return mn_segment_launch_t(c, d_class_pred, class_dim, d_adj_pred, offset_dim, MN_DTYPE_F32, W, H, num_classes,
                             offset_list, d_mask, d_object_class, d_partition, opts, stream);
}

// Second half: wait for the image queued by mn_segment_launch, read the verdict (a speculative
// attempt that does not hold is redone here on the ordinary path) and fill `stats`.
extern "C" int mn_segment_finish(mn_context* c, mn_stats* stats) {
  if (!c || !c->pend.active) return done(MN_ERR_ARGUMENT);
  const double t_in = host_now_us();
  double t_synced = t_in;
  mn_context::Pending& q = c->pend;
  const mn_options& o = q.call.opts;
  int rc;
  // require_proof: 1 = always, -1 = never, 0 = by mode -- AUTO hands back proven results only, an
  // explicitly requested ROUNDS / COMPONENTS run is taken as a request for that engine's answer
  const bool explicit_mode = o.mode == MN_MODE_EXACT || o.mode == MN_MODE_ROUNDS || o.mode == MN_MODE_COMPONENTS;
  const bool must_prove = o.require_proof > 0 || (o.require_proof == 0 && !explicit_mode);
  if (q.active == 2) {
    rc = q.rc;
  } else {
    MN_HIP(hipSetDevice(c->device));
    MN_HIP(hipEventSynchronize(c->ev_done));
    t_synced = host_now_us();
    memset(&q.stats, 0, sizeof(q.stats));
    rc = segment_read_back(c, &o, q.queued, &q.stats);
    if (rc != MN_OK) scores_stale(c);     // (a verdict: the attempts below set it again; an error: the context refuses)
    // a speculative attempt that does not hold is redone: by the sequential order itself when the
    // caller wants a proven result and the input is not sign-separable (the rounds would only
    // approximate it), else on the ordinary path
    if (rc == MN_RETRY_ROUNDS && must_prove)
      rc = segment_attempt(c, q.call, &q.stats, MN_MODE_EXACT, false);
    else if (rc == MN_RETRY_ROUNDS || rc == MN_RETRY_WAIT)
      rc = segment_attempt(c, q.call, &q.stats, rc == MN_RETRY_ROUNDS ? MN_MODE_ROUNDS : 0, false);
  }
  // A result that is neither certified nor from the sequential order is only an approximation of the
  // reference's result on an order-dependent input: redone by the exact engine (any image size).
  if (rc == MN_OK && must_prove && q.stats.proof == 0) {
    rc = segment_attempt(c, q.call, &q.stats, MN_MODE_EXACT, false);
    if (rc == MN_ERR_CAPACITY) rc = MN_ERR_UNPROVEN;      // (no room for the engine's workspace)
    if (rc == MN_ERR_UNPROVEN) { q.stats.status = rc; g_last_status = rc; }
  }
  // require_proof = 1 does not take "the sequential order, equal priorities in creation order" for proven: the
  // image is redone in the reference's own order among equals (mn_reforder.h: slow, csegment variant only)
  if (rc == MN_OK && o.require_proof > 0 && q.stats.proof == MN_PROOF_SEQUENTIAL_TIES) {
    if (o.variant == MN_VARIANT_CSEGMENT) {
      ImageCall again = q.call;
      again.opts.tie_order = MN_TIES_REFERENCE;
      rc = segment_attempt(c, again, &q.stats, MN_MODE_EXACT, false);
      if (rc == MN_ERR_CAPACITY) rc = MN_ERR_UNPROVEN;
    } else {
      rc = MN_ERR_UNPROVEN;            // (the Python variant's heapq / dict order is not restated)
    }
    if (rc == MN_ERR_UNPROVEN) { q.stats.status = rc; g_last_status = rc; }
  }
  if (stats) *stats = q.stats;
  q.active = 0;
  g_host_us[1] += t_synced - t_in; g_host_us[2] += host_now_us() - t_synced; g_host_n[1]++;
  return rc;
}

extern "C" int mn_segment_device_t(mn_context* c, const void* d_class_pred, int class_dim,
                                   const void* d_adj_pred, int offset_dim, int dtype, int W, int H,
                                   int num_classes, const int* offset_list, int* d_mask,
                                   int* d_object_class, int* d_partition, const mn_options* opts,
                                   void* stream, mn_stats* stats) {
  int rc = MN_ERR_ARGUMENT;
  if (!c || !c->pend.active)          // (a context with an unfinished launch is busy)
    rc = mn_segment_launch_t(c, d_class_pred, class_dim, d_adj_pred, offset_dim, dtype, W, H, num_classes,
                             offset_list, d_mask, d_object_class, d_partition, opts, stream);
  if (rc != MN_OK) {                  // rejected, busy or failed: nothing was left pending
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->status = rc; stats->total_logprob = NAN; }
    return rc;
  }
  return mn_segment_finish(c, stats);
}

extern "C" int mn_segment_device(mn_context* c, const float* d_class_pred, int class_dim,
                                 const float* d_adj_pred, int offset_dim, int W, int H,
                                 int num_classes, const int* offset_list, int* d_mask,
                                 int* d_object_class, int* d_partition, const mn_options* opts,
                                 void* stream, mn_stats* stats) {
  return mn_segment_device_t(c, d_class_pred, class_dim, d_adj_pred, offset_dim, MN_DTYPE_F32, W, H, num_classes,
                             offset_list, d_mask, d_object_class, d_partition, opts, stream, stats);
}

// A batch of images of one shape through the exact engine in ONE launch of its loop (a workgroup per image);
// see include/mergenet_hip.h.
extern "C" int mn_segment_exact_batch_t(mn_context** ctxs, int count, const void* const* d_class_pred, int class_dim,
                                        const void* const* d_adj_pred, int offset_dim, int dtype, int W, int H,
                                        int num_classes, const int* offset_list, int* const* d_mask,
                                        int* const* d_object_class, int* const* d_partition, const mn_options* opts,
                                        void* stream, mn_stats* stats) {
  ImageCall shared = {nullptr, nullptr, dtype, class_dim, offset_dim, W, H, num_classes};   // (maps and outputs: per image, below)
  image_call(&shared, offset_list, opts, stream);
  shared.opts.mode = MN_MODE_EXACT;
  const mn_options& o = shared.opts;
  if (!ctxs || count <= 0 || count > 4096 || !d_class_pred || !d_adj_pred || !d_mask || !d_object_class ||
      !dtype_ok(dtype, true))
    return done(MN_ERR_ARGUMENT);
  for (int i = 0; i < count; i++) {
    if (!ctxs[i] || ctxs[i]->pend.active || ctxs[i]->device != ctxs[0]->device) return done(MN_ERR_ARGUMENT);
    for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) return done(MN_ERR_ARGUMENT);
    const int rc = check_args(ctxs[i], shared);
    if (rc != MN_OK || !d_class_pred[i] || !d_adj_pred[i] || !d_mask[i] || !d_object_class[i]) {
      return done(rc != MN_OK ? rc : MN_ERR_ARGUMENT);
    }
  }
  MN_HIP(hipSetDevice(ctxs[0]->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (the set-up below writes `parent` long before the hand-over sets the flag again: a batch that fails in between
  //  must not leave a context answering for the image it segmented before)
  for (int i = 0; i < count; i++) scores_stale(ctxs[i]);
  // (require_proof reads every image's verdict after the hand-over: statistics are kept also when the caller wants none)
  HostBuf<mn_stats> own_stats((!stats && o.require_proof > 0) ? (size_t)count : 0);
  mn_stats* out = stats ? stats : (o.require_proof > 0 ? (mn_stats*)own_stats : nullptr);
  HostBuf<ImageCall> calls((size_t)count); HostBuf<ImgParams> Ps((size_t)count), rc_P((size_t)count);
  HostBuf<mn_context*> rc_ctx((size_t)count); HostBuf<unsigned char> redo((size_t)count); HostBuf<int> rc_idx((size_t)count);
  if (!calls.ok() || !Ps.ok() || !rc_P.ok() || !rc_ctx.ok() || !redo.ok() || !rc_idx.ok() || !own_stats.ok())
    return done(MN_ERR_INTERNAL);
  int rc = MN_OK;
  for (int i = 0; i < count; i++) {
    calls[i] = shared;
    calls[i].d_class = d_class_pred[i]; calls[i].d_adj = d_adj_pred[i];
    calls[i].d_mask = d_mask[i]; calls[i].d_objcls = d_object_class[i]; calls[i].d_part = d_partition ? d_partition[i] : nullptr;
    fill_params(&Ps[i], calls[i]);
  }
  {
    // more images than compute units: two workgroups per unit if each keeps its LDS under half of it
    int ncu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ctxs[0]->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
    (void)hipGetLastError();
    for (int i = 0; i < count; i++) ctxs[i]->xk.max_blocks = count > ncu ? 6144 : 0;
  }
  const bool ref_possible = o.variant == MN_VARIANT_CSEGMENT;
  // (MN_TIES_REFERENCE: straight to the reference-order loop, as a single call goes)
  const bool ref_only = ref_possible && o.tie_order == MN_TIES_REFERENCE;
  if (!ref_only) rc = exact_run(ctxs, count, Ps, st);
  for (int i = 0; i < count; i++) ctxs[i]->xk.max_blocks = 0;
  if (rc != MN_OK) return done(rc);
  // The tie policy, as a single call applies it: images whose tied choices conflict (or all, with
  // MN_TIES_REFERENCE) are redone in the reference's order among equals -- TOGETHER, one workgroup per image in one
  // launch of that loop.  Inside a batch the loop's cost is shared, so the size limit is higher than for a single
  // call (MN_TIE_LIMIT_BATCH_RECORDS).
  long long tie_limit = MN_TIE_LIMIT_BATCH_RECORDS;
  if (const char* e = getenv("MN_TIE_LIMIT")) tie_limit = atoll(e);
  int n_redo = 0;
  for (int i = 0; i < count; i++) {
    redo[i] = ref_only || (ref_possible && o.tie_order == MN_TIES_DEFAULT && x_ties_unresolved(ctxs[i]->xw.h_ctl) &&
                           (long long)W * H * offset_dim <= tie_limit);
    if (!redo[i]) continue;
    rc_ctx[n_redo] = ctxs[i]; rc_P[n_redo] = Ps[i]; n_redo++;
  }
  if (n_redo > 0) rc = redo_in_reference_order(rc_ctx, n_redo, rc_P, st, !ref_only);
  if (rc != MN_OK) return done(rc);
  // hand-over and output stage of every image (labels, mask, class table, certificate, log-likelihood)
  for (int i = 0; i < count; i++) {
    ctxs[i]->xk.prerun = redo[i] ? 2 : 1;
    const int r = segment_attempt(ctxs[i], calls[i], out ? &out[i] : nullptr, MN_MODE_EXACT, false);
    ctxs[i]->xk.prerun = 0;
    if (r != MN_OK && rc == MN_OK) rc = r;
  }
  // require_proof = 1, as mn_segment_finish applies it to a single call: a result that chose among bit-equal
  // priorities by the engine's own rule (proof 3 -- known only now: a certificate may have proven it after all) is not
  // taken for proven.  Those images are redone TOGETHER in the reference's order among equals, whatever their size
  // (csegment variant), or marked MN_ERR_UNPROVEN (the Python variant, whose heapq / dict order is not restated; or no
  // room for the loop's workspace) -- the exact engine's output then stays in place, and says proof 3.
  if (o.require_proof > 0) {
    int n2 = 0;
    for (int i = 0; i < count; i++) {
      if (out[i].status != MN_OK || out[i].proof != MN_PROOF_SEQUENTIAL_TIES) continue;
      if (!ref_possible) {
        out[i].status = MN_ERR_UNPROVEN;
        if (rc == MN_OK) rc = MN_ERR_UNPROVEN;
        continue;
      }
      rc_ctx[n2] = ctxs[i]; rc_P[n2] = Ps[i]; rc_idx[n2] = i; n2++;
      // (the redo's set-up resets `parent` under the labels of the hand-over above: should it fail, or be given up for
      //  MN_ERR_UNPROVEN, the context refuses; the second hand-over below sets the flag again)
      scores_stale(ctxs[i]);
    }
    const int r2 = n2 > 0 ? redo_in_reference_order(rc_ctx, n2, rc_P, st, true) : MN_OK;
    if (r2 == MN_ERR_CAPACITY) {
      for (int j = 0; j < n2; j++) out[rc_idx[j]].status = MN_ERR_UNPROVEN;
      if (rc == MN_OK) rc = MN_ERR_UNPROVEN;
    } else if (r2 != MN_OK) {
      return done(r2);
    }
    for (int j = 0; j < n2 && r2 == MN_OK; j++) {
      const int i = rc_idx[j];
      ctxs[i]->xk.prerun = 2;
      const int r = segment_attempt(ctxs[i], calls[i], &out[i], MN_MODE_EXACT, false);
      ctxs[i]->xk.prerun = 0;
      if (r != MN_OK && rc == MN_OK) rc = r;
    }
  }
  return done(rc);
}

extern "C" int mn_segment_exact_batch(mn_context** ctxs, int count, const float* const* d_class_pred, int class_dim,
                                      const float* const* d_adj_pred, int offset_dim, int W, int H, int num_classes,
                                      const int* offset_list, int* const* d_mask, int* const* d_object_class,
                                      int* const* d_partition, const mn_options* opts, void* stream,
                                      mn_stats* stats) {
  return mn_segment_exact_batch_t(ctxs, count, reinterpret_cast<const void* const*>(d_class_pred), class_dim,
                                  reinterpret_cast<const void* const*>(d_adj_pred), offset_dim, MN_DTYPE_F32, W, H,
                                  num_classes, offset_list, d_mask, d_object_class, d_partition, opts, stream, stats);
}

extern "C" int mn_score_device_t(mn_context* c, const void* d_class_pred, int class_dim,
                                 const void* d_adj_pred, int offset_dim, int dtype, int W, int H,
                                 int num_classes, const int* offset_list, const mn_options* opts,
                                 void* stream, unsigned char* d_cls_out,
                                 unsigned long long* d_best_out, float* ms_class_pass,
                                 float* ms_edge_pass) {
  ImageCall call = {d_class_pred, d_adj_pred, dtype, class_dim, offset_dim, W, H, num_classes};
  image_call(&call, offset_list, opts, stream);
  ImgParams P;
  int rc = begin_call(c, call, true, nullptr, &P);
  if (rc != MN_OK) return rc;
  scores_stale(c);                 // (run_phase_a: parent, ocls, lpvalid)
  const hipStream_t st = call.stream;
  // (deliberate carry-over: the flags as given, without MN_DEBUG_FLAGS_OR; ext_events and core_radius as the last call left them)
  c->debug_flags = call.opts.debug_flags;
  if ((rc = ensure_fast(c)) != MN_OK || (rc = run_phase_a(c, P, st, true)) != MN_OK) return rc;
  if (d_cls_out) MN_HIP(hipMemcpyAsync(d_cls_out, c->ocls, P.N, hipMemcpyDeviceToDevice, st));
  if (d_best_out)
    MN_HIP(hipMemcpyAsync(d_best_out, c->ball, (size_t)P.N * sizeof(u64), hipMemcpyDeviceToDevice, st));
  MN_HIP(hipStreamSynchronize(st));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
  if (ms_class_pass) *ms_class_pass = ms;
  (void)hipEventElapsedTime(&ms, c->ev[1], c->ev[2]);
  if (ms_edge_pass) *ms_edge_pass = ms;
  return done(MN_OK);
}

extern "C" int mn_score_device(mn_context* c, const float* d_class_pred, int class_dim,
                               const float* d_adj_pred, int offset_dim, int W, int H,
                               int num_classes, const int* offset_list, const mn_options* opts,
                               void* stream, unsigned char* d_cls_out,
                               unsigned long long* d_best_out, float* ms_class_pass,
                               float* ms_edge_pass) {
  return mn_score_device_t(c, d_class_pred, class_dim, d_adj_pred, offset_dim, MN_DTYPE_F32, W, H, num_classes,
                           offset_list, opts, stream, d_cls_out, d_best_out, ms_class_pass, ms_edge_pass);
}

// The affinity-scoring sweep of the default path alone (mn_cc_sign), and what it leaves, for the parity
// test against the oracle's phase A (see include/mergenet_hip.h).
extern "C" int mn_sweep_device_t(mn_context* c, const void* d_class_pred, int class_dim,
                                 const void* d_adj_pred, int offset_dim, int dtype, int W, int H, int num_classes,
                                 const int* offset_list, const mn_options* opts, void* stream,
                                 unsigned* d_bits_out, float* d_neg_out, unsigned char* d_cls_out,
                                 int* d_gsum_out, double* logsum_out, int* info_out) {
  ImageCall call = {d_class_pred, d_adj_pred, dtype, class_dim, offset_dim, W, H, num_classes};
  image_call(&call, offset_list, opts, stream);
  ImgParams P;
  const int rc = begin_call(c, call, d_bits_out && d_neg_out, nullptr, &P);
  if (rc != MN_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = P.N;
  if (ensure_fast(c) != MN_OK) return MN_ERR_NO_DEVICE;      // (deliberate carry-over: any failure reads as "no device" here)
  c->debug_flags = call.opts.debug_flags | MN_DEBUG_NO_EVENTS;
  c->ext_events = 0;
  c->cc_clean = 0;
  scores_stale(c);                 // (the sweep: lpsum as its group sums; ocls and lpvalid in the forms that carry classes)
  const SweepForm F = sweep_form_of(c, P, SWEEP_EXPORT);
  const size_t sign_waves = (size_t)F.waves;
  MN_HIP(hipMemsetAsync(c->scalars, 0, MN_NSCALARS * sizeof(int), st));
  launch_sweep(c, P, st, F);
  MN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_neg_out), 0x7FC00000, (size_t)P.O * N, st));
  hipLaunchKernelGGL(mn_cc_export_neg, dim3((unsigned)grid_for((size_t)N, 256)), dim3(256), 0, st, P,
                     (const unsigned*)c->cc_negbits, d_neg_out);
  MN_HIP(hipMemcpyAsync(d_bits_out, c->cc_bits, (size_t)N * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
  if (d_cls_out && F.cls) MN_HIP(hipMemcpyAsync(d_cls_out, c->cls0, (size_t)N, hipMemcpyDeviceToDevice, st));
  if (d_gsum_out && F.cls)              // (plane c of the sweep's products starts at c * N ints and holds N / 4 of them)
    MN_HIP(hipMemcpy2DAsync(d_gsum_out, (size_t)(N / 4) * sizeof(int), c->lpsum, (size_t)N * sizeof(int),
                            (size_t)(N / 4) * sizeof(int), (size_t)P.C, hipMemcpyDeviceToDevice, st));
  HostBuf<double> hp(sign_waves * 2);
  if (!hp.ok()) return MN_ERR_INTERNAL;
  MN_HIP(hipMemcpyAsync(hp, c->partial, sign_waves * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  MN_HIP(hipMemcpyAsync(c->h_scalars, c->scalars, MN_NSCALARS * sizeof(int), hipMemcpyDeviceToHost, st));
  MN_HIP(hipStreamSynchronize(st));
  double t = 0.0;
  for (size_t b = 0; b < sign_waves; b++) t += hp[2 * b];
  if (logsum_out) *logsum_out = t;
  if (info_out) { info_out[0] = F.px; info_out[1] = F.cls ? 1 : 0; info_out[2] = c->h_scalars[6]; }
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_sweep_device(mn_context* c, const float* d_class_pred, int class_dim,
                               const float* d_adj_pred, int offset_dim, int W, int H, int num_classes,
                               const int* offset_list, const mn_options* opts, void* stream,
                               unsigned* d_bits_out, float* d_neg_out, unsigned char* d_cls_out,
                               int* d_gsum_out, double* logsum_out, int* info_out) {
  return mn_sweep_device_t(c, d_class_pred, class_dim, d_adj_pred, offset_dim, MN_DTYPE_F32, W, H, num_classes,
                           offset_list, opts, stream, d_bits_out, d_neg_out, d_cls_out, d_gsum_out, logsum_out, info_out);
}

// Timing of the sweep alone (tuning; see include/mergenet_hip.h): `reps` launches back to back on `stream`,
// input set i % n_inputs for launch i, in the form the default path launches it.  Returns the average time per
// launch by HIP events around the whole train (launch gaps of consecutive kernels included).
extern "C" int mn_sweep_time_device_t(mn_context* c, const void* const* d_class_pred, const void* const* d_adj_pred,
                                      int dtype, int n_inputs, int class_dim, int offset_dim, int W, int H,
                                      int num_classes, const int* offset_list, const mn_options* opts, void* stream,
                                      int reps, float* us_per_launch) {
  // (the first pair of maps stands for all in the shared checks, which newly reject a null one; each launch fills in its own)
  const bool ok = d_class_pred && d_adj_pred && n_inputs >= 1 && reps >= 1 && us_per_launch;
  ImageCall call = {ok ? d_class_pred[0] : nullptr, ok ? d_adj_pred[0] : nullptr, dtype, class_dim, offset_dim, W, H, num_classes};
  image_call(&call, offset_list, opts, stream);
  ImgParams P;
  const int rc = begin_call(c, call, ok, nullptr, &P);
  if (rc != MN_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ensure_fast(c) != MN_OK) return MN_ERR_NO_DEVICE;      // (deliberate carry-over: any failure reads as "no device" here)
  c->debug_flags = call.opts.debug_flags | MN_DEBUG_NO_EVENTS;
  c->ext_events = 0;
  c->cc_clean = 0;
  scores_stale(c);                 // (the sweep: lpsum as its group sums; ocls and lpvalid in the forms that carry classes)
  MN_HIP(hipMemsetAsync(c->scalars, 0, MN_NSCALARS * sizeof(int), st));
  for (int phase = 0; phase < 2; phase++) {          // a tenth of the launches untimed first
    const int n = phase == 0 ? (reps + 9) / 10 : reps;
    if (phase == 1) MN_HIP(hipEventRecord(c->ev[0], st));
    for (int i = 0; i < n; i++) {
      call.d_class = d_class_pred[i % n_inputs]; call.d_adj = d_adj_pred[i % n_inputs];
      fill_params(&P, call);
      launch_sweep(c, P, st, sweep_form_of(c, P, SWEEP_TIMING));      // (per launch: the alignment of the maps may alternate)
    }
    if (phase == 1) MN_HIP(hipEventRecord(c->ev[1], st));
  }
  MN_HIP(hipStreamSynchronize(st));
  float ms = 0;
  MN_HIP(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
  *us_per_launch = ms * 1e3f / (float)reps;
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_sweep_time_device(mn_context* c, const float* const* d_class_pred, const float* const* d_adj_pred,
                                    int n_inputs, int class_dim, int offset_dim, int W, int H, int num_classes,
                                    const int* offset_list, const mn_options* opts, void* stream, int reps,
                                    float* us_per_launch) {
  return mn_sweep_time_device_t(c, reinterpret_cast<const void* const*>(d_class_pred),
                                reinterpret_cast<const void* const*>(d_adj_pred), MN_DTYPE_F32, n_inputs, class_dim,
                                offset_dim, W, H, num_classes, offset_list, opts, stream, reps, us_per_launch);
}

// Phase A of the exact engine (tests): log-odds and initial priority of every record in the layout
// of the oracle's phase-A export ([offset][source pixel], NaN outside the image), arg-max classes.
extern "C" int mn_exact_phase_a_device_t(mn_context* c, const void* d_class_pred, int class_dim,
                                         const void* d_adj_pred, int offset_dim, int dtype, int W, int H,
                                         int num_classes, const int* offset_list, const mn_options* opts,
                                         void* stream, unsigned char* d_cls_out, float* d_oml_out,
                                         float* d_prio_out) {
  ImageCall call = {d_class_pred, d_adj_pred, dtype, class_dim, offset_dim, W, H, num_classes};
  image_call(&call, offset_list, opts, stream);
  ImgParams P;
  int rc = begin_call(c, call, d_oml_out && d_prio_out, nullptr, &P);
  if (rc != MN_OK) return rc;
  scores_stale(c);                 // (exact_setup: parent)
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (deliberate carry-over: debug_flags is not set here -- nothing below reads it)
  if ((rc = exact_setup(c, P, st)) != MN_OK) return done(rc);
  hipLaunchKernelGGL(mn_x_export_phase_a, dim3(grid_for((size_t)P.N * P.O, 256)), dim3(256), 0, st, P, c->xw.X,
                     d_oml_out, d_prio_out, d_cls_out);
  MN_HIP(hipGetLastError());
  MN_HIP(hipStreamSynchronize(st));
  return done(MN_OK);
}

extern "C" int mn_exact_phase_a_device(mn_context* c, const float* d_class_pred, int class_dim,
                                       const float* d_adj_pred, int offset_dim, int W, int H,
                                       int num_classes, const int* offset_list, const mn_options* opts,
                                       void* stream, unsigned char* d_cls_out, float* d_oml_out,
                                       float* d_prio_out) {
  return mn_exact_phase_a_device_t(c, d_class_pred, class_dim, d_adj_pred, offset_dim, MN_DTYPE_F32, W, H, num_classes,
                                   offset_list, opts, stream, d_cls_out, d_oml_out, d_prio_out);
}

static int ensure_staging(mn_context* c) {
  if (c->d_part) return MN_OK;             // (the last one allocated: the group is whole)
  c->mem.free_group(MN_MEM_STAGING);       // (what an attempt that failed half-way left)
  MN_TRY(dev_alloc(c, MN_MEM_STAGING, &c->d_class, c->N * (size_t)c->maxC));
  MN_TRY(dev_alloc(c, MN_MEM_STAGING, &c->d_same, c->N * (size_t)c->maxO));
  MN_TRY(dev_alloc(c, MN_MEM_STAGING, &c->d_mask, c->N));
  MN_TRY(dev_alloc(c, MN_MEM_STAGING, &c->d_objcls, c->N));
  MN_TRY(dev_alloc(c, MN_MEM_STAGING, &c->d_part, c->N));
  return MN_OK;
}

extern "C" int mn_segment_host(mn_context* c, const float* class_pred, int class_dim,
                               const float* adj_pred, int offset_dim, int W, int H, int num_classes,
                               const int* offset_list, int* mask, int* object_class, int* partition,
                               const mn_options* opts, mn_stats* stats) {
  ImageCall call = {class_pred, adj_pred, MN_DTYPE_F32, class_dim, offset_dim, W, H, num_classes};
  image_call(&call, offset_list, opts, NULL);
  opts = &call.opts;
  int rc = check_args(c, call);
  if (rc == MN_OK && (!class_pred || !adj_pred || !mask || !object_class)) rc = MN_ERR_ARGUMENT;
  if (rc != MN_OK) { if (stats) { memset(stats, 0, sizeof(*stats)); stats->status = rc; } return done(rc); }
  MN_HIP(hipSetDevice(c->device));
  rc = ensure_staging(c);
  if (rc != MN_OK) return rc;
  const size_t N = (size_t)W * H;
  // only the first num_classes planes are used (class_dim == num_classes assumed by the reference)
  MN_HIP(hipMemcpy(c->d_class, class_pred, N * num_classes * sizeof(float), hipMemcpyHostToDevice));
  MN_HIP(hipMemcpy(c->d_same, adj_pred, N * offset_dim * sizeof(float), hipMemcpyHostToDevice));
  rc = mn_segment_device(c, c->d_class, num_classes, c->d_same, offset_dim, W, H, num_classes,
                         offset_list, c->d_mask, c->d_objcls, c->d_part, opts, NULL, stats);
  if (rc != MN_OK && rc != MN_ERR_NO_BACKGROUND && rc != MN_ERR_UNPROVEN) return rc;
  MN_HIP(hipMemcpy(mask, c->d_mask, N * sizeof(int), hipMemcpyDeviceToHost));
  MN_HIP(hipMemcpy(object_class, c->d_objcls, N * sizeof(int), hipMemcpyDeviceToHost));
  if (partition) MN_HIP(hipMemcpy(partition, c->d_part, N * sizeof(int), hipMemcpyDeviceToHost));
  return rc;
}

// ABI-compatible entry (utils/csegment/segment.cc:742-754).  A context is cached per thread and
// grown on demand; failures are reported on stderr and through mn_last_status().
extern "C" void c_run_segmentation(float* class_pred, int class_dim, float* adj_pred, int offset_dim,
                                   int img_width, int img_height, int num_classes, int* offset_list,
                                   int* output, int* object_class, float same_different_bias,
                                   float object_merge_factor, float merge_logprob_bias) {
  // (freed when the thread ends: thread-local objects are destroyed before the HIP runtime's statics)
  struct Cached { mn_context* c = NULL; ~Cached() { if (c) mn_destroy(c); } };
  static thread_local Cached holder;
  mn_context*& cached = holder.c;
  if (img_width <= 0 || img_height <= 0 || num_classes <= 0 || offset_dim <= 0) {
    g_last_status = MN_ERR_ARGUMENT;
    fprintf(stderr, "c_run_segmentation: %s\n", mn_status_string(MN_ERR_ARGUMENT));
    return;
  }
  if (cached && ((size_t)img_width * img_height > cached->N || num_classes > cached->maxC ||
                 offset_dim > cached->maxO)) {
    mn_destroy(cached);
    cached = NULL;
  }
  if (!cached) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    cached = mn_create(dev, img_height, img_width, num_classes, offset_dim);
    if (!cached) {
      fprintf(stderr, "c_run_segmentation: %s\n", mn_status_string(g_last_status));
      return;
    }
  }
  mn_options o;
  mn_default_options(&o);
  o.same_different_bias = same_different_bias;
  o.object_merge_factor = object_merge_factor;
  o.merge_logprob_bias = merge_logprob_bias;
  // (AUTO with the certificate: the reference's own result -- a separable map is proven by the fast
  //  path's certificate, anything else goes through the exact engine)
  const int rc = mn_segment_host(cached, class_pred, class_dim, adj_pred, offset_dim, img_width,
                                 img_height, num_classes, offset_list, output, object_class, NULL,
                                 &o, NULL);
  if (rc != MN_OK) fprintf(stderr, "c_run_segmentation: %s\n", mn_status_string(rc));
}


// ---- producer hand-off / mask post-processing -----------------
extern "C" int mn_prepare_device_t(mn_context* c, const void* d_in, int in_dtype, int channels, int in_height,
                                   int in_width, void* d_out, int out_dtype, int out_height, int out_width,
                                   int apply_sigmoid, int clip, void* stream) {
  if (!c || !d_in || !d_out || channels <= 0 || in_height <= 0 || in_width <= 0 || out_height <= 0 ||
      out_width <= 0 || out_height > 65535 || channels > 65535 || !dtype_ok(in_dtype, false) || !dtype_ok(out_dtype, false))
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mn_prepare_maps, dim3(grid_for(out_width, 256), out_height, channels), dim3(256),
                     0, st, d_in, in_dtype, channels, in_height, in_width, d_out, out_dtype, out_height, out_width,
                     apply_sigmoid, clip);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_prepare_device(mn_context* c, const float* d_in, int channels, int in_height,
                                 int in_width, float* d_out, int out_height, int out_width,
                                 int apply_sigmoid, int clip, void* stream) {
  return mn_prepare_device_t(c, d_in, MN_DTYPE_F32, channels, in_height, in_width, d_out, MN_DTYPE_F32, out_height,
                             out_width, apply_sigmoid, clip, stream);
}

extern "C" int mn_upsample_mask_device(mn_context* c, const int* d_mask, int in_height, int in_width,
                                       int* d_out, int out_height, int out_width, void* stream) {
  if (!c || !d_mask || !d_out || in_height <= 0 || in_width <= 0 || out_height <= 0 ||
      out_width <= 0 || out_height > 65535)
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mn_upsample_mask, dim3(grid_for(out_width, 256), out_height), dim3(256), 0, st,
                     d_mask, in_height, in_width, d_out, out_height, out_width,
                     mn_nearest_scale(in_width, out_width), mn_nearest_scale(in_height, out_height));
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}


// Change points of the column-major label scan (see mn_kernels_prepare.h).  d_points receives
// 3 * count ints laid out as [positions | labels before | labels at] with stride `capacity`;
// returns the count through *count (the call synchronises the stream), MN_ERR_CAPACITY if more
// than `capacity` change points exist.
extern "C" int mn_rle_points_device(mn_context* c, const int* d_mask, int height, int width,
                                    int* d_points, int capacity, int* count, void* stream) {
  if (!c || !d_mask || !d_points || !count || height <= 0 || width <= 0 || capacity <= 0 ||
      (size_t)height * width > c->N)
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = height * width;
  c->cc_clean = 0;                 // (writes the scalar block)
  const int nblk = (int)grid_for(N, MN_RLE_ITEMS);
  hipLaunchKernelGGL(mn_rle_count, dim3(nblk), dim3(256), 0, st, d_mask, height, width, c->block_count);
  hipLaunchKernelGGL(mn_rank_scan, dim3(1), dim3(1024), 0, st, nblk, c->block_count, c->scalars + 5);
  MN_HIP(hipMemcpyAsync(c->h_scalars, c->scalars, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
  MN_HIP(hipStreamSynchronize(st));
  const int total = c->h_scalars[5];
  *count = total;
  if (total > capacity) return done(MN_ERR_CAPACITY);
  hipLaunchKernelGGL(mn_rle_scatter, dim3(nblk), dim3(256), 0, st, d_mask, height, width,
                     (const int*)c->block_count, d_points, d_points + capacity,
                     d_points + 2 * (size_t)capacity);
  MN_HIP(hipGetLastError());
  MN_HIP(hipStreamSynchronize(st));
  return done(MN_OK);
}


extern "C" int mn_sameness_targets_device(mn_context* c, const int* d_mask, int height, int width,
                                          const int* offset_list, int offset_dim, float* d_out,
                                          void* stream) {
  if (!c || !d_mask || !offset_list || !d_out || height <= 0 || width <= 0 || offset_dim <= 0 ||
      offset_dim > MN_MAX_OFFSETS)
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  ImgParams P;
  memset(&P, 0, sizeof(P));
  for (int k = 0; k < offset_dim; k++) { P.di[k] = offset_list[2 * k]; P.dj[k] = offset_list[2 * k + 1]; }
  hipLaunchKernelGGL(mn_sameness_targets, dim3(grid_for((size_t)height * width, 256), offset_dim),
                     dim3(256), 0, static_cast<hipStream_t>(stream), d_mask, height, width, P, d_out);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// Confidence of the instances of the LAST mn_segment_device call on this context:
// d_scores[k-1] = lp[cls] - lp[0] of label k (float32, at least num_instances entries).  The class
// planes passed to that call must still be alive (objects that never merged read them).
extern "C" int mn_instance_scores_device(mn_context* c, float* d_scores, void* stream) {
  // (a context with an unfinished launch is busy: its tail may still be running on the side stream)
  if (!c || !d_scores || !c->last_valid || c->pend.active) return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(mn_instance_scores, dim3(grid_for(c->last_params.N, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), c->last_params, obj_state(c),
                     (const int*)c->label, d_scores);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// ---- instance table, small-instance filter (mn_kernels_instances.h) -------------------------------
// Both entry points only enqueue: no host synchronisation, no copy.  The image is not held to the
// context's capacity (the table is most wanted on the upsampled mask); the context names the device.
extern "C" int mn_instance_table_device(mn_context* c, const int* d_mask, int height, int width,
                                        int num_instances, int* d_table, void* stream) {
  if (!c || !d_mask || height <= 0 || width <= 0 || num_instances < 0 || (num_instances > 0 && !d_table) ||
      (size_t)height * (size_t)width > (size_t)INT_MAX)
    return done(MN_ERR_ARGUMENT);
  if (num_instances == 0) return done(MN_OK);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mn_instance_table_init, dim3(grid_for(num_instances, 256)), dim3(256), 0, st, num_instances,
                     height, width, d_table);
  const int v = row_walk_v(width, sizeof(int), d_mask);
  const RowWalk R = row_walk_aimed(height, width, v, MN_INST_WORKGROUPS, MN_INST_THREADS / 64);
  const dim3 g((unsigned)R.blocks), b(MN_INST_THREADS);
  if (v == 4)
    hipLaunchKernelGGL(mn_instance_table_runs<4>, g, b, 0, st, d_mask, height, width, num_instances, R, d_table);
  else
    hipLaunchKernelGGL(mn_instance_table_runs<1>, g, b, 0, st, d_mask, height, width, num_instances, R, d_table);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_filter_instances_device(mn_context* c, const int* d_mask, int height, int width,
                                          int num_instances, const int* d_table, const int* d_object_class,
                                          const float* d_scores, int min_area, float min_score, int* d_mask_out,
                                          int* d_remap, int* d_table_out, int* d_object_class_out,
                                          float* d_scores_out, int* d_new_count, void* stream) {
  if (!c || !d_mask || !d_mask_out || !d_remap || !d_new_count || height <= 0 || width <= 0 || num_instances < 0 ||
      (size_t)height * (size_t)width > (size_t)INT_MAX ||
      (num_instances > 0 && (!d_table || !d_object_class || !d_table_out || !d_object_class_out ||
                             (d_scores && !d_scores_out))) ||
      // the compaction is out of place (and d_remap is read by the relabel while the mask is written)
      (d_table_out && d_table_out == d_table) || (d_object_class_out && d_object_class_out == d_object_class) ||
      (d_scores_out && d_scores_out == d_scores) || d_remap == d_mask_out || d_remap == d_mask)
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mn_instance_keep, dim3(1), dim3(1024), 0, st, num_instances, d_table, d_object_class, d_scores,
                     min_area, min_score, d_remap, d_table_out, d_object_class_out, d_scores_out, d_new_count);
  const size_t N = (size_t)height * (size_t)width;
  if (N % 4 == 0 && ((reinterpret_cast<uintptr_t>(d_mask) | reinterpret_cast<uintptr_t>(d_mask_out)) & 15) == 0)
    hipLaunchKernelGGL(mn_relabel_mask4, dim3(grid_for(N / 4, 256)), dim3(256), 0, st, d_mask, N / 4, num_instances,
                       (const int*)d_remap, d_mask_out);
  else
    hipLaunchKernelGGL(mn_relabel_mask, dim3(grid_for(N, 256)), dim3(256), 0, st, d_mask, N, num_instances,
                       (const int*)d_remap, d_mask_out);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// ---- overlap table, IoU and matching against the ground truth (mn_kernels_match.h) ------------------
// Both entry points only enqueue: no host synchronisation, no copy.  Nothing of the segmentation path runs here.
extern "C" int mn_overlap_table_device(mn_context* c, const int* d_pred, const int* d_truth, int height, int width,
                                       int num_pred, int num_truth, int* d_table, void* stream) {
  if (!c || !d_pred || !d_truth || !d_table || height <= 0 || width <= 0 || num_pred < 0 || num_truth < 0 ||
      (size_t)height * (size_t)width > (size_t)INT_MAX ||
      ((long long)num_pred + 1) * ((long long)num_truth + 1) > (1LL << 28))
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t entries = (size_t)(num_pred + 1) * (size_t)(num_truth + 1);
  MN_HIP(hipMemsetAsync(d_table, 0, entries * sizeof(int), st));
  const int v = row_walk_v(width, sizeof(int), d_pred, d_truth);
  const RowWalk R = row_walk_aimed(height, width, v, MN_OVL_WORKGROUPS, MN_OVL_THREADS / 64);
  const dim3 g((unsigned)R.blocks), b(MN_OVL_THREADS);
  if (v == 4)
    hipLaunchKernelGGL(mn_overlap_table_runs<4>, g, b, 0, st, d_pred, d_truth, height, width, num_pred, num_truth, R,
                       d_table);
  else
    hipLaunchKernelGGL(mn_overlap_table_runs<1>, g, b, 0, st, d_pred, d_truth, height, width, num_pred, num_truth, R,
                       d_table);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

static MnThresholds match_thresholds(const double* thresholds, int T) {
  MnThresholds th;
  for (int i = 0; i < 16; i++) th.t[i] = thresholds[i < T ? i : T - 1];
  return th;
}

// The launches of one matching, K > 0 and G > 0, on the context's scratch (allocated by the caller).  `ordered`: the
// caller has written the scratch's order_p itself (mn_eval_append_device: its order passes over some detections).
static void match_launch(mn_context* c, hipStream_t st, const int* d_table, int K, int G, const int* d_pred_class,
                         const float* d_pred_score, const int* d_truth_class, const unsigned char* d_truth_crowd,
                         const MnThresholds& th, int T, double area_lo, double area_hi, double* d_iou,
                         int* d_pred_match, int* d_truth_match, unsigned char* d_pred_ignore,
                         unsigned char* d_truth_ignore, bool ordered) {
  hipLaunchKernelGGL(mn_match_areas, dim3((unsigned)((K + 3) / 4 + (G + 63) / 64)), dim3(MN_MATCH_THREADS), 0, st,
                     d_table, K, G, d_truth_crowd, area_lo, area_hi, c->match_work, d_truth_ignore);
  if (!ordered)
    hipLaunchKernelGGL(mn_match_rank, dim3(grid_for(K, MN_MATCH_THREADS)), dim3(MN_MATCH_THREADS), 0, st, K,
                       d_pred_score, c->match_work);
  if (d_iou)
    hipLaunchKernelGGL(mn_match_iou, dim3(grid_for((size_t)K * G, MN_MATCH_THREADS)), dim3(MN_MATCH_THREADS), 0, st,
                       d_table, K, G, d_truth_crowd, (const MnMatchWork*)c->match_work, d_iou);
  hipLaunchKernelGGL(mn_match_greedy, dim3(T), dim3(MN_MATCH_THREADS), 0, st, d_table, K, G,
                     (const MnMatchWork*)c->match_work, d_pred_class, d_truth_class, d_truth_crowd, th, area_lo,
                     area_hi, d_pred_match, d_truth_match, d_pred_ignore);
}

extern "C" int mn_match_overlaps_device(mn_context* c, const int* d_table, int num_pred, int num_truth,
                                         const int* d_pred_class, const float* d_pred_score,
                                         const int* d_truth_class, const unsigned char* d_truth_crowd,
                                         const double* thresholds, int num_thresholds, double area_lo,
                                         double area_hi, double* d_iou, int* d_pred_match, int* d_truth_match,
                                         unsigned char* d_pred_ignore, unsigned char* d_truth_ignore, void* stream) {
  const int K = num_pred, G = num_truth, T = num_thresholds;
  if (!c || !d_table || !thresholds || T < 1 || T > 16 || K < 0 || G < 0 ||
      (K > 0 && (!d_pred_class || !d_pred_match || !d_pred_ignore)) || (G > 0 && (!d_truth_class || !d_truth_match)))
    return done(MN_ERR_ARGUMENT);
  if (K > MN_MATCH_MAX_INSTANCES || G > MN_MATCH_MAX_INSTANCES) return done(MN_ERR_CAPACITY);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (K == 0 || G == 0) {                                        // nothing to match: every output is zero
    if (K > 0) {
      MN_HIP(hipMemsetAsync(d_pred_match, 0, (size_t)T * K * sizeof(int), st));
      MN_HIP(hipMemsetAsync(d_pred_ignore, 0, (size_t)T * K, st));
    }
    if (G > 0) {
      MN_HIP(hipMemsetAsync(d_truth_match, 0, (size_t)T * G * sizeof(int), st));
      if (d_truth_ignore) MN_HIP(hipMemsetAsync(d_truth_ignore, 0, (size_t)G, st));
    }
    return done(MN_OK);
  }
  MN_TRY(ensure_scratch(c, &c->match_work, 1));
  match_launch(c, st, d_table, K, G, d_pred_class, d_pred_score, d_truth_class, d_truth_crowd,
               match_thresholds(thresholds, T), T, area_lo, area_hi, d_iou, d_pred_match, d_truth_match, d_pred_ignore,
               d_truth_ignore, /* ordered */ false);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// ---- the dataset-level evaluation: a log of records, accumulate (mn_kernels_eval.h) ----------------------
// All three only enqueue.  The log and its fill are the caller's; nothing here reads anything back.
extern "C" int mn_eval_append_device(mn_context* c, const int* d_table, int num_pred, int num_truth,
                                      const int* d_pred_class, const float* d_pred_score, const int* d_truth_class,
                                      const unsigned char* d_truth_crowd, const double* thresholds,
                                      int num_thresholds, const double* area_ranges, int num_areas, int max_det,
                                      int num_classes, int image, void* d_records, long long* d_npig, void* stream) {
  const int K = num_pred, G = num_truth, T = num_thresholds, A = num_areas;
  if (!c || !d_table || !thresholds || !area_ranges || !d_npig || T < 1 || T > 16 || A < 1 || A > MN_EVAL_MAX_AREAS ||
      K < 0 || G < 0 || max_det < 1 || num_classes < 1 || image < 0 || (K > 0 && (!d_pred_class || !d_records)) ||
      (G > 0 && !d_truth_class) || (reinterpret_cast<uintptr_t>(d_records) & 15) != 0)
    return done(MN_ERR_ARGUMENT);
  if (K > MN_MATCH_MAX_INSTANCES || G > MN_MATCH_MAX_INSTANCES) return done(MN_ERR_CAPACITY);
  if (K == 0 && G == 0) return done(MN_OK);                      // an image without anything: no record, no count
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  MN_TRY(ensure_scratch(c, &c->match_work, 1));
  MN_TRY(ensure_scratch(c, &c->eval_work, 1));
  MnEvalWork* e = c->eval_work;
  MnAreaRanges ar;
  for (int a = 0; a < MN_EVAL_MAX_AREAS; a++) {
    ar.lo[a] = area_ranges[2 * (a < A ? a : A - 1)];
    ar.hi[a] = area_ranges[2 * (a < A ? a : A - 1) + 1];
  }
  const dim3 b(MN_EVAL_THREADS);
  if (K > 0)
    hipLaunchKernelGGL(mn_eval_rank, dim3(grid_for(K, MN_EVAL_THREADS)), b, 0, st, K, d_pred_class, d_pred_score,
                       max_det, c->match_work, e);
  if (K > 0 && G > 0) {
    const MnThresholds th = match_thresholds(thresholds, T);
    for (int a = 0; a < A; a++)
      match_launch(c, st, d_table, K, G, d_pred_class, d_pred_score, d_truth_class, d_truth_crowd, th, T, ar.lo[a],
                   ar.hi[a], nullptr, e->pred_match + (size_t)a * T * K, e->truth_match,
                   e->pred_ignore + (size_t)a * T * K, nullptr, /* ordered */ true);
  } else {                                                       // nothing to match: the areas alone
    hipLaunchKernelGGL(mn_match_areas, dim3((unsigned)((K + 3) / 4 + (G + 63) / 64)), dim3(MN_MATCH_THREADS), 0, st,
                       d_table, K, G, d_truth_crowd, ar.lo[0], ar.hi[0], c->match_work, (unsigned char*)nullptr);
  }
  if (G > 0)
    hipLaunchKernelGGL(mn_eval_npig, dim3(grid_for(G, MN_EVAL_THREADS)), b, 0, st, G, d_truth_class, d_truth_crowd,
                       (const MnMatchWork*)c->match_work, num_classes, A, ar, reinterpret_cast<u64*>(d_npig));
  if (K > 0)
    hipLaunchKernelGGL(mn_eval_pack, dim3(grid_for(K, MN_EVAL_THREADS)), b, 0, st, K, T, A, ar, max_det,
                       G > 0 ? 1 : 0, d_pred_class, d_pred_score, (const MnMatchWork*)c->match_work,
                       (const MnEvalWork*)e, image, static_cast<uint4*>(d_records));
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_eval_keys_device(mn_context* c, const void* d_records, long long num_records, int num_classes,
                                    long long* d_keys, void* stream) {
  if (!c || num_records < 0 || num_records > (long long)INT_MAX || num_classes < 1 ||
      (num_records > 0 && (!d_records || !d_keys)) || (reinterpret_cast<uintptr_t>(d_records) & 15) != 0)
    return done(MN_ERR_ARGUMENT);
  if (num_records > 0) {
    MN_HIP(hipSetDevice(c->device));
    hipLaunchKernelGGL(mn_eval_keys, dim3(grid_for((size_t)num_records, MN_EVAL_THREADS)), dim3(MN_EVAL_THREADS), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint4*>(d_records), (int)num_records,
                       num_classes, d_keys);
    MN_HIP(hipGetLastError());
  }
  return done(MN_OK);
}

extern "C" int mn_eval_accumulate_device(mn_context* c, const void* d_records, long long num_records,
                                          const long long* d_sorted_keys, const long long* d_sorted_index,
                                          const long long* d_npig, int num_classes, int num_thresholds,
                                          const double* d_rec_thresholds, int num_rec_thresholds, int num_areas,
                                          const int* max_dets, int num_max_dets, double* d_precision,
                                          double* d_recall, double* d_scores, void* stream) {
  const int C = num_classes, T = num_thresholds, R = num_rec_thresholds, A = num_areas, M = num_max_dets;
  bool ok = c && d_npig && max_dets && d_precision && d_recall && d_scores && C >= 1 && T >= 1 && T <= 16 && R >= 0 &&
            (R == 0 || d_rec_thresholds) && A >= 1 && A <= MN_EVAL_MAX_AREAS && M >= 1 && M <= MN_EVAL_MAX_DETS &&
            num_records >= 0 && num_records <= (long long)INT_MAX &&
            (num_records == 0 || (d_records && d_sorted_keys && d_sorted_index)) &&
            (reinterpret_cast<uintptr_t>(d_records) & 15) == 0 && (long long)C * A * M <= (long long)INT_MAX;
  MnMaxDets md;
  for (int m = 0; ok && m < MN_EVAL_MAX_DETS; m++) {
    md.m[m] = max_dets[m < M ? m : M - 1];
    ok = md.m[m] >= 1 && (m == 0 || m >= M || md.m[m] > md.m[m - 1]);
  }
  if (!ok) return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(mn_eval_scan, dim3((unsigned)(C * A * M), (unsigned)T), dim3(MN_EVAL_THREADS), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint4*>(d_records), (int)num_records,
                     d_sorted_keys, d_sorted_index, d_npig, C, T, R, A, M, md, d_rec_thresholds, d_precision, d_recall,
                     d_scores);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// ---- the maps against the ground truth (mn_kernels_mapscore.h) ---------------------------------------
// Enqueues only: no host synchronisation, no copy.  Nothing of the segmentation path runs here.
extern "C" int mn_map_scores_device(mn_context* c, const void* d_class_pred, int class_dim, const void* d_adj_pred,
                                    int offset_dim, int dtype, int img_width, int img_height, int num_classes,
                                    const int* offset_list, const int* d_truth, int num_truth,
                                    const int* d_truth_classes, long long* d_confusion, double* d_sums,
                                    int accumulate, void* stream) {
  const int H = img_height, W = img_width, C = num_classes, O = offset_dim, G = num_truth;
  if (!c || !d_class_pred || !d_adj_pred || !offset_list || !d_truth || !d_confusion || !d_sums || H <= 0 || W <= 0 ||
      C < 1 || C > MN_MAX_CLASSES || class_dim < C || O < 1 || O > MN_MAX_OFFSETS || G < 0 ||
      (G > 0 && !d_truth_classes) || (size_t)H * (size_t)W > (size_t)INT_MAX || W > MN_MS_MAX_WIDTH ||
      !dtype_ok(dtype, true))
    return done(MN_ERR_ARGUMENT);
  const int dt = dtype & 0xFF, logits = (dtype & MN_MAPS_LOGITS) ? 1 : 0;
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  MN_TRY(ensure_scratch(c, &c->ms_partials, (size_t)MN_MS_VALUES * MN_MS_WORKGROUPS));
  if (!accumulate) MN_HIP(hipMemsetAsync(d_confusion, 0, (size_t)C * C * sizeof(long long), st));

  MnMapScoreArgs A;
  memset(&A, 0, sizeof(A));
  A.cls = d_class_pred; A.same = d_adj_pred; A.truth = d_truth; A.truth_classes = d_truth_classes;
  A.H = H; A.W = W; A.C = C; A.O = O; A.G = G;
  A.confusion = reinterpret_cast<unsigned long long*>(d_confusion);
  A.partials = c->ms_partials;
  truth_pass_offsets(offset_list, O, H, W, A.di, A.dj);
  // The grid by (H, W, element type) alone; pixels per lane follow the width and BOTH maps' base addresses.
  const int elem = dt == MN_DTYPE_F32 ? 4 : 2;
  const int slots = truth_pass_slots(H, W, elem, MN_MS_WAVES);
  const int v = row_walk_v(W, elem, d_class_pred, d_adj_pred);
  A.walk = row_walk_fixed(H, W, v, slots, MN_MS_WAVES);
  const dim3 g((unsigned)slots), b(MN_MS_THREADS);
  by_dtype(dt, [&](auto t) {
    by_pixels(t, v, [&](auto px) {
      constexpr int DT = decltype(t)::value, V = decltype(px)::value;
      if (logits) hipLaunchKernelGGL((mn_map_scores_pass<DT, true, V>), g, b, 0, st, A);
      else hipLaunchKernelGGL((mn_map_scores_pass<DT, false, V>), g, b, 0, st, A);
    });
  });
  hipLaunchKernelGGL(mn_map_scores_finish, dim3(3 * O), dim3(64), 0, st, (const double*)c->ms_partials, slots,
                     d_sums, accumulate);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// ---- the training criterion from the label mask (mn_kernels_loss.h) ---------------------------------------
// Enqueues only: no host synchronisation, no copy.  Nothing of the segmentation path runs here.
extern "C" int mn_mask_bce_device(mn_context* c, const void* d_class_logits, const void* d_same_logits, int dtype,
                                  int img_width, int img_height, int num_classes, int offset_dim,
                                  const int* offset_list, const int* d_truth, int num_truth,
                                  const int* d_truth_classes, void* d_grad_class, void* d_grad_same,
                                  float scale_class, float scale_same, double* d_sums, int accumulate, void* stream) {
  const int H = img_height, W = img_width, C = num_classes, O = offset_dim, G = num_truth;
  if (!c || !d_truth || !d_sums || H <= 0 || W <= 0 || C < 0 || C > MN_MAX_CLASSES || O < 0 || O > MN_MAX_OFFSETS ||
      C + O == 0 || (C > 0 && !d_class_logits) || (O > 0 && (!d_same_logits || !offset_list)) || G < 0 ||
      (G > 0 && !d_truth_classes) || (size_t)H * (size_t)W > (size_t)INT_MAX || W > MN_MS_MAX_WIDTH ||
      !dtype_ok(dtype, false) || !std::isfinite(scale_class) || !std::isfinite(scale_same))
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  MN_TRY(ensure_scratch(c, &c->ms_partials, (size_t)MN_MS_VALUES * MN_MS_WORKGROUPS));

  MnMaskBceArgs A;
  memset(&A, 0, sizeof(A));
  A.cls = C ? d_class_logits : nullptr; A.same = O ? d_same_logits : nullptr;
  A.gcls = C ? d_grad_class : nullptr; A.gsame = O ? d_grad_same : nullptr;
  A.truth = d_truth; A.truth_classes = d_truth_classes;
  A.H = H; A.W = W; A.C = C; A.O = O; A.G = G;
  A.scale_cls = scale_class; A.scale_same = scale_same;
  A.partials = c->ms_partials;
  truth_pass_offsets(offset_list, O, H, W, A.di, A.dj);
  // The grid by (H, W, element type) alone.  So are the pixels a lane holds (row_walk_v without bases); the four
  // bases only decide between wide accesses and single elements.
  const int dt = dtype & 0xFF;
  const int elem = dt == MN_DTYPE_F32 ? 4 : 2;
  const int slots = truth_pass_slots(H, W, elem, MN_BCE_WAVES);
  const int p = row_walk_v(W, elem, nullptr);
  A.wide = std::min(row_walk_v(W, elem, A.cls, A.same), row_walk_v(W, elem, A.gcls, A.gsame)) == p ? 1 : 0;
  A.walk = row_walk_fixed(H, W, p, slots, MN_BCE_WAVES);
  const dim3 g((unsigned)slots), b(MN_BCE_THREADS);
  by_dtype(dt, [&](auto t) {
    by_pixels(t, p, [&](auto px) {
      hipLaunchKernelGGL((mn_mask_bce_pass<decltype(t)::value, decltype(px)::value>), g, b, 0, st, A);
    });
  });
  hipLaunchKernelGGL(mn_map_scores_finish, dim3(2 + O), dim3(64), 0, st, (const double*)c->ms_partials, slots,
                     d_sums, accumulate);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// ---- Dice and weighted multi-BCE from the label mask (mn_kernels_planeloss.h) ----------------------------
// Enqueue only: no host synchronisation, no copy.  Nothing of the segmentation path runs here.
// What the sums and the gradient pass check alike, and the kernel argument they share (d_grad: null for the sums).
static bool plane_call(MnPlaneArgs* A, const mn_context* c, const void* d_logits, int dtype, int W, int H, int part,
                       int NP, const int* offset_list, const int* d_truth, int G, const int* d_truth_classes,
                       int flags, void* d_grad) {
  const bool cls = part == MN_PART_CLASS;
  if (!c || !d_logits || !d_truth || H <= 0 || W <= 0 || (!cls && part != MN_PART_OFFSET) || NP < 1 ||
      NP > (cls ? MN_MAX_CLASSES : MN_MAX_OFFSETS) || (!cls && !offset_list) || G < 0 ||
      (cls && G > 0 && !d_truth_classes) || (size_t)H * (size_t)W > (size_t)INT_MAX || W > MN_MS_MAX_WIDTH ||
      !dtype_ok(dtype, false) || (flags & ~(MN_PLANE_COMPLEMENT | MN_PLANE_TERMS)))
    return false;
  memset(A, 0, sizeof(*A));
  A->maps = d_logits; A->grad = d_grad; A->truth = d_truth; A->truth_classes = cls ? d_truth_classes : nullptr;
  A->H = H; A->W = W; A->NP = NP; A->G = cls ? G : 0; A->part = part;
  A->comp = (flags & MN_PLANE_COMPLEMENT) ? 1 : 0;
  if (!cls) truth_pass_offsets(offset_list, NP, H, W, A->di, A->dj);
  // The grid by (H, W, element type) alone.  So are the pixels a lane holds (row_walk_v without bases); the bases
  // only decide between wide accesses and single elements.
  const int elem = (dtype & 0xFF) == MN_DTYPE_F32 ? 4 : 2;
  const int slots = truth_pass_slots(H, W, elem, MN_PL_WAVES);
  const int p = row_walk_v(W, elem, nullptr);
  A->wide = row_walk_v(W, elem, d_logits, d_grad) == p ? 1 : 0;
  A->walk = row_walk_fixed(H, W, p, slots, MN_PL_WAVES);
  return true;
}

extern "C" int mn_plane_sums_device(mn_context* c, const void* d_logits, int dtype, int img_width, int img_height,
                                    int part, int num_planes, const int* offset_list, const int* d_truth,
                                    int num_truth, const int* d_truth_classes, int flags, double* d_sums,
                                    int accumulate, void* stream) {
  MnPlaneArgs A;
  if (!d_sums || !plane_call(&A, c, d_logits, dtype, img_width, img_height, part, num_planes, offset_list, d_truth,
                             num_truth, d_truth_classes, flags, nullptr))
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  MN_TRY(ensure_scratch(c, &c->pl_partials, (size_t)MN_PL_VALUES * MN_MS_WORKGROUPS));
  A.partials = c->pl_partials;
  const int slots = A.walk.blocks;
  const dim3 g((unsigned)slots), b(MN_PL_THREADS);
  by_dtype(dtype & 0xFF, [&](auto t) {
    by_pixels(t, A.walk.v, [&](auto px) {
      constexpr int DT = decltype(t)::value, V = decltype(px)::value;
      if (flags & MN_PLANE_TERMS) hipLaunchKernelGGL((mn_plane_sums_pass<DT, V, true>), g, b, 0, st, A);
      else hipLaunchKernelGGL((mn_plane_sums_pass<DT, V, false>), g, b, 0, st, A);
    });
  });
  hipLaunchKernelGGL(mn_map_scores_finish, dim3(MN_PL_ROWS * num_planes + 1), dim3(64), 0, st,
                     (const double*)c->pl_partials, slots, d_sums, accumulate);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_plane_coeffs_device(mn_context* c, int criterion, int flags, const double* d_sums, int num_planes,
                                      double pixels, double smooth, double scale, float* d_coeffs, double* d_loss,
                                      int accumulate, void* stream) {
  const bool dice = criterion == MN_CRIT_DICE;
  if (!c || !d_sums || !d_coeffs || !d_loss || num_planes < 1 || num_planes > MN_MAX_CLASSES ||
      (!dice && criterion != MN_CRIT_MBCE) || (flags & ~(MN_PLANE_COMPLEMENT | MN_PLANE_TERMS)) ||
      (!dice && (flags & MN_PLANE_COMPLEMENT)) || !std::isfinite(pixels) || !std::isfinite(smooth) ||
      !std::isfinite(scale) || pixels < 0.0 || (dice && !(smooth > 0.0)))
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipLaunchKernelGGL(mn_plane_coeffs, dim3(1), dim3(MN_PL_COEFF_THREADS), 0, static_cast<hipStream_t>(stream),
                     criterion, (flags & MN_PLANE_COMPLEMENT) ? 1 : 0, d_sums, num_planes, pixels, smooth, scale,
                     d_coeffs, d_loss, accumulate);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_plane_grad_device(mn_context* c, const void* d_logits, int dtype, int img_width, int img_height,
                                    int part, int num_planes, const int* offset_list, const int* d_truth,
                                    int num_truth, const int* d_truth_classes, int flags, const float* d_coeffs,
                                    const float* d_factor, void* d_grad, void* stream) {
  MnPlaneArgs A;
  if (!d_coeffs || !d_grad || !plane_call(&A, c, d_logits, dtype, img_width, img_height, part, num_planes,
                                          offset_list, d_truth, num_truth, d_truth_classes, flags, d_grad))
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  A.coeffs = d_coeffs; A.factor = d_factor;
  const dim3 g((unsigned)A.walk.blocks), b(MN_PL_THREADS);
  by_dtype(dtype & 0xFF, [&](auto t) {
    by_pixels(t, A.walk.v, [&](auto px) {
      hipLaunchKernelGGL((mn_plane_grad_pass<decltype(t)::value, decltype(px)::value>), g, b, 0,
                         static_cast<hipStream_t>(stream), A);
    });
  });
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// ---- cross-entropy over the planes of one part, from the label mask (mn_kernels_celoss.h) ---------------
// Enqueues only: no host synchronisation, no copy.  Nothing of the segmentation path runs here.
extern "C" int mn_mask_ce_device(mn_context* c, const void* d_logits, int dtype, int img_width, int img_height,
                                 int part, int num_planes, const int* offset_list, const int* d_truth, int num_truth,
                                 const int* d_truth_classes, void* d_grad, float scale, double* d_sums, int accumulate,
                                 void* stream) {
  MnPlaneArgs Q;                  // what plane_call refuses is refused here; its grid and walk are this pass's too
  static_assert(MN_CE_WAVES == MN_PL_WAVES, "mn_mask_ce_device takes the walk that plane_call lays out");
  if (!d_sums || !std::isfinite(scale) || !plane_call(&Q, c, d_logits, dtype, img_width, img_height, part, num_planes,
                                                      offset_list, d_truth, num_truth, d_truth_classes, 0, d_grad))
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  MN_TRY(ensure_scratch(c, &c->ms_partials, (size_t)MN_MS_VALUES * MN_MS_WORKGROUPS));

  MnMaskCeArgs A;
  memset(&A, 0, sizeof(A));
  A.maps = Q.maps; A.grad = Q.grad; A.truth = Q.truth; A.truth_classes = Q.truth_classes;
  A.H = Q.H; A.W = Q.W; A.NP = Q.NP; A.G = Q.G; A.part = Q.part; A.wide = Q.wide;
  A.scale = scale;
  A.walk = Q.walk;
  A.partials = c->ms_partials;
  memcpy(A.di, Q.di, sizeof(A.di));
  memcpy(A.dj, Q.dj, sizeof(A.dj));
  // The form by the plane count alone: resident up to MN_CE_RESIDENT_MAX planes, in the smallest bucket, else streaming.
  const int bucket = mn_ce_bucket(A.NP);
  const dim3 g((unsigned)A.walk.blocks), b(MN_CE_THREADS);
  by_dtype(dtype & 0xFF, [&](auto t) {
    by_pixels(t, A.walk.v, [&](auto px) {
      constexpr int DT = decltype(t)::value, V = decltype(px)::value;
      if (bucket == 4) hipLaunchKernelGGL((mn_mask_ce_pass<DT, V, 4>), g, b, 0, st, A);
      else if (bucket == 10) hipLaunchKernelGGL((mn_mask_ce_pass<DT, V, 10>), g, b, 0, st, A);
      else if (bucket == MN_CE_RESIDENT_MAX) hipLaunchKernelGGL((mn_mask_ce_pass<DT, V, MN_CE_RESIDENT_MAX>), g, b, 0, st, A);
      else hipLaunchKernelGGL((mn_mask_ce_pass<DT, V, 0>), g, b, 0, st, A);
    });
  });
  hipLaunchKernelGGL(mn_map_scores_finish, dim3(MN_CE_VALUES), dim3(64), 0, st, (const double*)c->ms_partials,
                     A.walk.blocks, d_sums, accumulate);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// ---- class maps from a tiled semantic network (mn_kernels_tiles.h) -------------------------------------
// Enqueues only: no host synchronisation, no copy, no allocation.  The geometry is checked here, on the host arrays,
// so that the kernel never meets a pixel without a covering tile or a tile that leaves the image.
static bool tile_axis_ok(const int* starts, int n, int side, int size) {
  if (!starts || n < 1 || n > MN_TILES_MAX_STARTS || side <= 0 || size <= 0) return false;
  int sorted[MN_TILES_MAX_STARTS];
  for (int i = 0; i < n; i++) {
    if (starts[i] < 0 || starts[i] > size - side) return false;   // the tile leaves the image (side > size: every start)
    int k = i;
    for (; k > 0 && sorted[k - 1] > starts[i]; k--) sorted[k] = sorted[k - 1];
    sorted[k] = starts[i];
  }
  int reach = 0;                                                  // rows (columns) 0 .. reach - 1 are covered
  for (int i = 0; i < n; i++) {
    if (sorted[i] > reach) return false;
    reach = std::max(reach, sorted[i] + side);
  }
  return reach >= size;
}

extern "C" int mn_tile_class_maps_device(mn_context* c, const void* d_tiles, const void* d_flip_tiles, int dtype,
                                         int net_classes, int tile_height, int tile_width,
                                         const int* row_starts, int num_rows, const int* col_starts, int num_cols,
                                         int img_height, int img_width, int num_classes,
                                         void* d_out, int out_dtype, int clip, void* stream) {
  const int H = img_height, W = img_width, Cn = net_classes, C = num_classes;
  bool ok = c && d_tiles && d_out && row_starts && col_starts && H > 0 && W > 0 && tile_height > 0 && tile_width > 0 &&
            Cn >= 1 && Cn <= MN_TILES_MAX_CLASSES && C >= 1 && C <= Cn && dtype_ok(dtype, false) &&
            dtype_ok(out_dtype, false);
  ok = ok && tile_axis_ok(row_starts, num_rows, tile_height, H) && tile_axis_ok(col_starts, num_cols, tile_width, W);
  const long long blocks_per_row = ok ? ((long long)W + MN_TILES_THREADS - 1) / MN_TILES_THREADS : 0;
  if (!ok || blocks_per_row * (long long)H > (long long)INT_MAX)
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  MnTileArgs A;
  memset(&A, 0, sizeof(A));
  A.tiles = d_tiles; A.flip = d_flip_tiles; A.out = d_out;
  A.Cn = Cn; A.C = C; A.th = tile_height; A.tw = tile_width; A.nr = num_rows; A.nc = num_cols; A.H = H; A.W = W;
  A.blocks_per_row = (int)blocks_per_row;
  A.out_dtype = out_dtype; A.clip = clip ? 1 : 0;
  for (int i = 0; i < num_rows; i++) A.rs[i] = row_starts[i];
  for (int j = 0; j < num_cols; j++) A.cs[j] = col_starts[j];
  const dim3 g((unsigned)(blocks_per_row * H)), b(MN_TILES_THREADS);
  by_dtype(dtype, [&](auto t) {
    constexpr int DT = decltype(t)::value;
    if (Cn <= 8) hipLaunchKernelGGL((mn_tile_class_maps<DT, 8>), g, b, 0, st, A);
    else if (Cn <= 20) hipLaunchKernelGGL((mn_tile_class_maps<DT, 20>), g, b, 0, st, A);
    else if (Cn <= 32) hipLaunchKernelGGL((mn_tile_class_maps<DT, 32>), g, b, 0, st, A);
    else hipLaunchKernelGGL((mn_tile_class_maps<DT, MN_TILES_MAX_CLASSES>), g, b, 0, st, A);
  });
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

// Wire format of the mask exchange (mergenet_amd/distributed.py): d_wire is int16
// [n_pixels + 1 + max_instances + 4] = labels, instance count, classes padded with -1, and the
// four 16-bit words (low first) of the float64 total log-likelihood.
extern "C" int mn_pack_wire_device(const int* d_mask, const int* d_object_class, int num_instances,
                                   double total_logprob, int n_pixels, int max_instances,
                                   short* d_wire, void* stream) {
  if (!d_mask || !d_object_class || !d_wire || n_pixels <= 0 || max_instances <= 0 ||
      max_instances > 32767 || num_instances < 0 || num_instances > max_instances)
    return done(MN_ERR_ARGUMENT);
  const size_t threads = (size_t)(n_pixels >> 2) > (size_t)max_instances + 1 ? (size_t)(n_pixels >> 2)
                                                                              : (size_t)max_instances + 1;
  hipLaunchKernelGGL(mn_pack_wire, dim3(grid_for(threads < 4 ? 4 : threads, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), n_pixels, max_instances, num_instances,
                     total_logprob, d_mask, d_object_class, d_wire);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}


extern "C" size_t mn_runs_wire_words(int capacity, int max_instances) {
  if (capacity <= 0 || max_instances <= 0) return 0;
  return 4 + (size_t)capacity + (size_t)(capacity + 1) / 2 + (size_t)(max_instances + 3) / 4;
}

extern "C" int mn_pack_runs_device(mn_context* c, const int* d_mask, const int* d_object_class,
                                   int num_instances, double total_logprob, int n_pixels, int capacity,
                                   int max_instances, int* d_wire, void* stream) {
  if (!c || !d_mask || !d_object_class || !d_wire || n_pixels <= 0 || (size_t)n_pixels > c->N ||
      capacity <= 0 || max_instances <= 0 || num_instances < 0 || num_instances > max_instances ||
      num_instances > 32767)
    return done(MN_ERR_ARGUMENT);
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nblk = (int)grid_for(n_pixels, MN_RLE_ITEMS);
  int* total = c->wire_counts + nblk;
  hipLaunchKernelGGL(mn_runs_count, dim3(nblk), dim3(256), 0, st, d_mask, n_pixels, c->wire_counts);
  hipLaunchKernelGGL(mn_rank_scan, dim3(1), dim3(1024), 0, st, nblk, c->wire_counts, total);
  hipLaunchKernelGGL(mn_runs_scatter, dim3(nblk), dim3(256), 0, st, d_mask, n_pixels,
                     (const int*)c->wire_counts, (const int*)total, capacity, max_instances, num_instances,
                     total_logprob, d_object_class, d_wire);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_unpack_runs_batch_device(const int* d_wires, long long wire_stride_words, int count,
                                           int n_pixels, int capacity, int max_instances, int* d_masks,
                                           int* d_tables, void* stream) {
  if (!d_wires || !d_masks || n_pixels <= 0 || capacity <= 0 || max_instances <= 0 || count <= 0 || count > 65535 ||
      wire_stride_words < (long long)mn_runs_wire_words(capacity, max_instances))
    return done(MN_ERR_ARGUMENT);
  const size_t threads = (size_t)n_pixels > (size_t)max_instances ? (size_t)n_pixels : (size_t)max_instances;
  hipLaunchKernelGGL(mn_runs_unpack, dim3(grid_for(threads, 256), (unsigned)count), dim3(256), 0,
                     static_cast<hipStream_t>(stream), d_wires, n_pixels, capacity, max_instances, d_masks, d_tables,
                     wire_stride_words);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}

extern "C" int mn_unpack_runs_device(const int* d_wire, int n_pixels, int capacity, int max_instances,
                                     int* d_mask, int* d_table, void* stream) {
  return mn_unpack_runs_batch_device(d_wire, (long long)mn_runs_wire_words(capacity, max_instances), 1, n_pixels,
                                     capacity, max_instances, d_mask, d_table, stream);
}

// ---- COCO RLE strings on the host (native twin of mergenet_amd/rle.py::from_change_points) ------
static inline void rle_put(unsigned char* out, long long cap, long long& w, long long x) {
  bool more = true;
  while (more) {
    int ch = (int)(x & 0x1F);
    x >>= 5;                                  // arithmetic shift: keeps the sign
    more = (ch & 0x10) ? (x != -1) : (x != 0);
    if (more) ch |= 0x20;
    if (w < cap) out[w] = (unsigned char)(ch + 48);
    w++;
  }
}

extern "C" long long mn_rle_encode_host(const int* points, int capacity, int n, int height, int width,
                                        int num_instances, unsigned char* out, long long out_capacity,
                                        long long* offsets, int* areas) {
  if (!points || n < 0 || capacity < n || height <= 0 || width <= 0 || num_instances < 0 || !offsets ||
      (!out && out_capacity > 0))
    return MN_ERR_ARGUMENT;
  const int* pos = points;
  const int* prev = points + capacity;
  const int* cur = points + 2 * (size_t)capacity;
  const long long N = (long long)height * width;
  const int K = num_instances;
  // a change point (j, a, b) ends a run of label a and starts a run of label b at j; positions are
  // ascending, so the starts (and ends) of one label are ascending too: two counting passes
  int* first = static_cast<int*>(calloc((size_t)2 * (K + 2), sizeof(int)));
  int* buf = static_cast<int*>(malloc(sizeof(int) * (size_t)(2 * (n > 0 ? n : 1))));
  if (!first || !buf) { free(first); free(buf); return MN_ERR_INTERNAL; }
  int* sfirst = first;
  int* efirst = first + K + 2;
  for (int i = 0; i < n; i++) {
    if (cur[i] >= 1 && cur[i] <= K) sfirst[cur[i] + 1]++;
    if (prev[i] >= 1 && prev[i] <= K) efirst[prev[i] + 1]++;
  }
  for (int k = 1; k <= K + 1; k++) { sfirst[k] += sfirst[k - 1]; efirst[k] += efirst[k - 1]; }
  int* starts = buf;
  int* ends = buf + n;
  {
    int* sw = static_cast<int*>(malloc(sizeof(int) * (size_t)(2 * (K + 2))));
    if (!sw) { free(first); free(buf); return MN_ERR_INTERNAL; }
    int* ew = sw + K + 2;
    memcpy(sw, sfirst, sizeof(int) * (size_t)(K + 2));
    memcpy(ew, efirst, sizeof(int) * (size_t)(K + 2));
    for (int i = 0; i < n; i++) {
      if (cur[i] >= 1 && cur[i] <= K) starts[sw[cur[i]]++] = pos[i];
      if (prev[i] >= 1 && prev[i] <= K) ends[ew[prev[i]]++] = pos[i];
    }
    free(sw);
  }
  long long w = 0;
  for (int k = 1; k <= K; k++) {
    offsets[k - 1] = w;
    const int s0 = sfirst[k], s1 = sfirst[k + 1], e0 = efirst[k], e1 = efirst[k + 1];
    long long last = 0, c2 = 0, c1 = 0;      // the counts one and two places back
    long long area = 0;
    int emitted = 0;
    auto emit = [&](long long c) {
      long long x = c;
      if (emitted > 2) x -= c2;
      rle_put(out, out_capacity, w, x);
      c2 = c1; c1 = c;
      emitted++;
    };
    for (int i = s0; i < s1; i++) {
      const long long a = starts[i];
      const long long b = (e0 + (i - s0) < e1) ? ends[e0 + (i - s0)] : N;   // the last run may reach the end
      emit(a - last);
      emit(b - a);
      area += b - a;
      last = b;
    }
    if (last < N || emitted == 0) emit(N - last);
    if (areas) areas[k - 1] = (int)area;
  }
  offsets[K] = w;
  free(first);
  free(buf);
  return w;
}

// ---- COCO RLE back into a label mask (mn_kernels_rle.h; the decoding half of the RLE path) -----------------
// Host: pycocotools' compressed counts string -> counts (native twin of mergenet_amd/rle.py::string_to_counts).
extern "C" long long mn_rle_counts_host(const unsigned char* s, long long len, unsigned* counts, long long capacity,
                                        long long* total) {
  if ((!s && len > 0) || len < 0 || capacity < 0 || (!counts && capacity > 0)) return MN_ERR_ARGUMENT;
  long long n = 0, sum = 0, p = 0;
  long long back1 = 0, back2 = 0;               // the counts one and two places back
  while (p < len) {
    unsigned long long bits = 0;
    int k = 0;
    bool more = true;
    while (more) {
      if (p >= len) return MN_ERR_ARGUMENT;      // the string ends inside a group
      const int ch = (int)s[p++] - 48;
      if (ch < 0 || ch > 63) return MN_ERR_ARGUMENT;
      if (k >= 12) return MN_ERR_CAPACITY;       // more than 60 bits: no count of 31 bits is written so
      bits |= (unsigned long long)(ch & 0x1F) << (5 * k);
      more = (ch & 0x20) != 0;
      k++;
      if (!more && (ch & 0x10)) bits |= ~0ull << (5 * k);
    }
    long long x = (long long)bits;
    if (n > 2) x += back2;
    if (x < 0) return MN_ERR_ARGUMENT;
    if (x > 0x7fffffffLL) return MN_ERR_CAPACITY;
    if (n < capacity) counts[n] = (unsigned)x;
    n++;
    sum += x;
    back2 = back1;
    back1 = x;
  }
  if (total) *total = sum;
  return n;
}

// Enqueues only: no allocation, no copy, no host synchronisation.  Not held to the context's capacity.
extern "C" int mn_rle_decode_device(mn_context* c, const unsigned* d_counts, const int* d_starts, int num_annotations,
                                    int num_counts, const int* d_values, int height, int width,
                                    unsigned* d_scratch_ends, int* d_scratch_records, int* d_mask, int* d_area,
                                    void* stream) {
  const int A = num_annotations;
  if (!c || !d_mask || height <= 0 || width <= 0 || (size_t)height * (size_t)width > (size_t)INT_MAX ||
      A < 0 || A > MN_RLE_MAX_ANNOTATIONS || num_counts < 0 ||
      (A > 0 && (!d_starts || !d_scratch_records)) || (num_counts > 0 && (!d_counts || !d_scratch_ends)))
    return done(MN_ERR_ARGUMENT);
  static_assert(sizeof(MnRleRecord) == MN_RLE_RECORD_INTS * sizeof(int), "the record size the header states");
  MN_HIP(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  MnRleRecord* rec = reinterpret_cast<MnRleRecord*>(d_scratch_records);
  if (A > 0)
    hipLaunchKernelGGL(mn_rle_scan, dim3(A), dim3(MN_RLE_SCAN_THREADS), 0, st, d_counts, d_starts, num_counts,
                       (unsigned)(height * width), d_scratch_ends, rec, d_area);
  hipLaunchKernelGGL(mn_rle_paint, dim3(grid_for(width, MN_RLE_TILE_COLS), grid_for(height, 64)),
                     dim3(MN_RLE_PAINT_THREADS), 0, st, (const unsigned*)d_scratch_ends, (const MnRleRecord*)rec,
                     d_values, A, height, width, d_mask);
  MN_HIP(hipGetLastError());
  return done(MN_OK);
}
