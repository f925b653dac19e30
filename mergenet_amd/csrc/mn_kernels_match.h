// mn_kernels_match.h -- a label mask against the ground-truth label mask on the device: the overlap table of the
// two masks in one pass, and from it the IoU of every pair and COCO's greedy matching per IoU threshold.
//
// Reference work replaced (the Cityscapes caller's last stage and the ground truth it is held to):
//   COCOeval(...).evaluate()          egs/cityscape/local/evaluate.py:67-73    computeIoU + evaluateImg per image
//   anns_to_mask                      utils/dataset.py:486-506                 the truth label mask compared with
//   (accumulate, the dataset-level part, is mn_kernels_eval.h)
// Definitions, the whole of both computations (mergenet_hip.h gives them in full):
//   table[p][g] = number of pixels with prediction label p and truth label g, p in 0..K, g in 0..G; a label
//                 outside its range counts as 0;
//   area_p[k] = sum of row k, area_g[j] = sum of column j, iou[k][j] = table[k][j] / (area_p + area_g - table[k][j])
//                 (/ area_p for a crowd truth instance; 0 where the denominator is 0), float64, ONE division;
//   matching: per threshold, detections by descending score take the best truth instance still free (or crowd) of
//                 their class with iou >= min(t, 1 - 1e-10): non-ignored before ignored, then the greatest IoU,
//                 then the greatest label.
#pragma once

#include "mn_device.h"
#include "mn_row_walk.h"

// Two constants of the pass; a variant build for tools/time_overlap_table.py may set them (-D...):
#ifndef MN_OVL_LDS_DIM
#define MN_OVL_LDS_DIM 64         /* a workgroup accumulates the pairs with p < 64 and g < 64 in LDS (64 x 64 ints =
                                     16 KB) and adds what it gathered to the global table once, at its end; every
                                     other pair goes straight to the global table.
                                     0 = no LDS table, one global atomicAdd per run (the simpler form).
                                     Measured (profiles/overlap_table_time.log): 16 us with the LDS table against
                                     106 us without on the default path's 1024x2048 mask, where every chunk of
                                     background adds to table[0][0]; 11.9 against 11.4 us on every pixel its own
                                     label, where no pair is held in LDS */
#endif
#ifndef MN_OVL_WORKGROUPS
#define MN_OVL_WORKGROUPS 256     /* workgroups aimed at (one per CU), as MN_INST_WORKGROUPS */
#endif
#define MN_OVL_THREADS 256
#define MN_OVL_LDS (MN_OVL_LDS_DIM > 0)
#define MN_OVL_LDS_COLS (MN_OVL_LDS ? MN_OVL_LDS_DIM : 1)   /* row length of the LDS table */

// One run of `len` pixels of the pair (p, g), both already inside 0..K and 0..G.
__device__ __forceinline__ void mn_ovl_run(int* sh, int lds_p, int lds_g, int* __restrict__ table, int G, int p,
                                           int g, int len) {
  if (MN_OVL_LDS && p < lds_p && g < lds_g)
    atomicAdd(&sh[p * MN_OVL_LDS_COLS + g], len);
  else
    atomicAdd(table + (size_t)p * (size_t)(G + 1) + (size_t)g, len);
}

// The walk of mn_row_walk.h over TWO masks, V = 4 or 1 (BOTH bases decide it), the next chunk's loads in flight
// over this chunk's work.
// A pixel is the head of a run when EITHER mask differs from the pixel before it (the lane before for a lane's
// first pixel; the first pixel of a chunk is always a head); a head reads where its run ends from
// mn_walk_run_end.  Only heads update the table, by the run's length.
// Labels are clamped BEFORE they form an address: a prediction label outside 0..K and a truth label outside 0..G
// -- both masks are the caller's memory -- read as 0.  Pixels of the last chunk of a row past W read as -1 in both
// masks: they end the run before them and are counted nowhere, so the entries sum to H * W.
template <int V>
__global__ __launch_bounds__(MN_OVL_THREADS) void mn_overlap_table_runs(const int* __restrict__ pred,
                                                                        const int* __restrict__ truth, int H, int W,
                                                                        int K, int G, const RowWalk R,
                                                                        int* __restrict__ table) {
  __shared__ int sh[MN_OVL_LDS_COLS * MN_OVL_LDS_COLS];
  const int lds_p = min(K + 1, MN_OVL_LDS_DIM), lds_g = min(G + 1, MN_OVL_LDS_DIM);
  if (MN_OVL_LDS) {
    for (int i = threadIdx.x; i < lds_p * MN_OVL_LDS_COLS; i += MN_OVL_THREADS) sh[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const RowSpan span = row_walk_span(R, (long long)blockIdx.x * (MN_OVL_THREADS / 64) + (threadIdx.x >> 6));

  auto load = [&](long long c, int* a, int* t) {
    int x, y;
    row_walk_pixel(R, V, c, lane, &x, &y);
#pragma unroll
    for (int j = 0; j < V; j++) a[j] = t[j] = -1;
    if (x < W) {
      const size_t at = (size_t)y * W + x;
      mn_walk_labels<V, true>(pred + at, a);
      mn_walk_labels<V, true>(truth + at, t);
#pragma unroll
      for (int j = 0; j < V; j++) {
        a[j] = ((unsigned)a[j] <= (unsigned)K) ? a[j] : 0;
        t[j] = ((unsigned)t[j] <= (unsigned)G) ? t[j] : 0;
      }
    }
  };

  int na[V], nt[V];
  if (span.c0 < span.c1) load(span.c0, na, nt);
  for (long long c = span.c0; c < span.c1; c++) {
    int a[V], t[V];
#pragma unroll
    for (int j = 0; j < V; j++) { a[j] = na[j]; t[j] = nt[j]; }
    if (c + 1 < span.c1) load(c + 1, na, nt);            // the next chunk's loads are in flight over this chunk's work

    int before_a = __shfl_up(a[V - 1], 1), before_t = __shfl_up(t[V - 1], 1);
    if (lane == 0) before_a = -2;                    // (labels are >= -1 here: the chunk's first pixel is a head)
    bool head[V];
#pragma unroll
    for (int j = 0; j < V; j++)
      head[j] = a[j] != (j == 0 ? before_a : a[j > 0 ? j - 1 : 0]) ||
                t[j] != (j == 0 ? before_t : t[j > 0 ? j - 1 : 0]);
    const int next_head = mn_walk_next_head<V>(head, lane);
#pragma unroll
    for (int j = 0; j < V; j++) {
      if (!head[j] || a[j] < 0) continue;            // (a[j] < 0: past W, in both masks)
      mn_ovl_run(sh, lds_p, lds_g, table, G, a[j], t[j], mn_walk_run_end<V>(head, j, next_head) - j);
    }
  }

  if (MN_OVL_LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < lds_p * MN_OVL_LDS_COLS; i += MN_OVL_THREADS) {
      const int n = sh[i];
      if (n == 0) continue;                          // only the pairs this workgroup met (columns >= lds_g stay 0)
      atomicAdd(table + (size_t)(i / MN_OVL_LDS_COLS) * (size_t)(G + 1) + (size_t)(i % MN_OVL_LDS_COLS), n);
    }
  }
}

// ---- IoU and matching from the table --------------------------------------------------------------------------
// Arrays per instance are indexed label - 1 (the library's convention); table rows and columns by the label itself.

#define MN_MATCH_THREADS 256

struct MnThresholds { double t[16]; };

// Scratch of one matching call, in the context (allocated at first use): everything the kernels below hand on.
struct MnMatchWork {
  double area_p[MN_MATCH_MAX_INSTANCES];
  double area_g[MN_MATCH_MAX_INSTANCES];
  int order_p[MN_MATCH_MAX_INSTANCES];            // order_p[r] = label of the detection taken r-th
  unsigned char ign_g[MN_MATCH_MAX_INSTANCES];
};

__device__ __forceinline__ double mn_match_iou_of(int inter, double ap, double ag, bool crowd) {
  const double i = (double)inter;
  const double den = crowd ? ap : ap + ag - i;       // (integers below 2^53: exact)
  return den != 0.0 ? i / den : 0.0;
}

// Blocks 0 .. ceil(K / 4) - 1: one wave per prediction label, the sum of its row (columns 0..G).
// The blocks behind them: 64 truth labels each, the sums of their columns (rows 0..K) in four slices of rows
// joined through LDS, and the ignore flag of each.
__global__ __launch_bounds__(MN_MATCH_THREADS) void mn_match_areas(const int* __restrict__ table, int K, int G,
                                                                   const unsigned char* __restrict__ crowd,
                                                                   double area_lo, double area_hi,
                                                                   MnMatchWork* __restrict__ w,
                                                                   unsigned char* __restrict__ truth_ignore) {
  __shared__ long long part[MN_MATCH_THREADS];
  const int row_blocks = (K + 3) / 4;
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  if ((int)blockIdx.x < row_blocks) {
    const int k = blockIdx.x * 4 + slice + 1;
    if (k > K) return;
    const int* row = table + (size_t)k * (size_t)(G + 1);
    long long s = 0;
    for (int g = lane; g <= G; g += 64) s += row[g];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) w->area_p[k - 1] = (double)s;
    return;
  }
  const int j = ((int)blockIdx.x - row_blocks) * 64 + lane + 1;
  long long s = 0;
  if (j <= G)
    for (int p = slice; p <= K; p += 4) s += table[(size_t)p * (size_t)(G + 1) + (size_t)j];
  part[threadIdx.x] = s;
  __syncthreads();
  if (slice == 0 && j <= G) {
    const double ag = (double)(part[lane] + part[64 + lane] + part[128 + lane] + part[192 + lane]);
    const unsigned char ign = ((crowd && crowd[j - 1]) || ag < area_lo || ag > area_hi) ? 1 : 0;
    w->area_g[j - 1] = ag;
    w->ign_g[j - 1] = ign;
    if (truth_ignore) truth_ignore[j - 1] = ign;
  }
}

// order_p[rank of label k] = k: the rank is the number of detections taken before it -- those of greater score, of
// equal score and smaller label, and, for a NaN score, every score that is none (a NaN sorts last).  O(K^2).
__global__ __launch_bounds__(MN_MATCH_THREADS) void mn_match_rank(int K, const float* __restrict__ score,
                                                                  MnMatchWork* __restrict__ w) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  if (!score) { w->order_p[k] = k + 1; return; }
  const float sk = score[k];
  const bool nk = sk != sk;
  int rank = 0;
  for (int i = 0; i < K; i++) {
    const float si = score[i];
    const bool ni = si != si;
    const bool first = (ni != nk) ? nk : (ni ? i < k : (si > sk || (si == sk && i < k)));
    rank += first ? 1 : 0;
  }
  w->order_p[rank] = k + 1;
}

__global__ __launch_bounds__(MN_MATCH_THREADS) void mn_match_iou(const int* __restrict__ table, int K, int G,
                                                                 const unsigned char* __restrict__ crowd,
                                                                 const MnMatchWork* __restrict__ w,
                                                                 double* __restrict__ iou) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)K * (size_t)G) return;
  const int k = (int)(i / (size_t)G), j = (int)(i % (size_t)G);
  iou[i] = mn_match_iou_of(table[(size_t)(k + 1) * (size_t)(G + 1) + (size_t)(j + 1)], w->area_p[k], w->area_g[j],
                           crowd && crowd[j]);
}

// One workgroup per threshold.  Detections go one after the other in rank order; the lanes stride over the truth
// labels, each keeps its best candidate (group: 2 = not ignored, 1 = ignored; IoU; label) and the workgroup picks
// the winner: the greater group, then the greater IoU, then the greater label -- the last of equals in truth order,
// which lists each group in ascending label.  truth_match of this threshold lives in LDS; entry j is read and
// written by ONE lane, the one that strides over j, so the loop needs a single barrier per detection (the waves'
// candidates alternate between two sets of slots).
__global__ __launch_bounds__(MN_MATCH_THREADS) void mn_match_greedy(const int* __restrict__ table, int K, int G,
                                                                    const MnMatchWork* __restrict__ w,
                                                                    const int* __restrict__ pred_class,
                                                                    const int* __restrict__ truth_class,
                                                                    const unsigned char* __restrict__ crowd,
                                                                    MnThresholds th, double area_lo, double area_hi,
                                                                    int* __restrict__ pred_match,
                                                                    int* __restrict__ truth_match,
                                                                    unsigned char* __restrict__ pred_ignore) {
  __shared__ int tm[MN_MATCH_MAX_INSTANCES];
  __shared__ double s_iou[2][MN_MATCH_THREADS / 64];
  __shared__ int s_key[2][MN_MATCH_THREADS / 64];     // group * 8192 + label, 0 = no candidate
  const int t = blockIdx.x, tid = threadIdx.x;
  const double lo = fmin(th.t[t], 1.0 - 1e-10);
  for (int j = tid; j < G; j += MN_MATCH_THREADS) tm[j] = 0;   // (each lane its own entries: no barrier)
  int taken = 0;                                      // detections that went through the barrier below
  for (int r = 0; r < K; r++) {
    const int d = w->order_p[r];
    // d forms addresses, so it is held to 1..K.  mn_match_rank's ranks are a permutation; mn_eval_rank enters the
    // detections it leaves out of the matching as 0.  An entry passed over runs no barrier, so the slots below
    // alternate on the count of detections taken, not on r: two taken in a row never share a set of slots.
    if ((unsigned)(d - 1) >= (unsigned)K) continue;
    const double ap = w->area_p[d - 1];
    const int cls = pred_class[d - 1];
    const int* row = table + (size_t)d * (size_t)(G + 1);
    int key = 0;
    double best = -1.0;
    for (int j = tid + 1; j <= G; j += MN_MATCH_THREADS) {
      const int inter = row[j];
      if (inter == 0 && lo > 0.0) continue;           // (most pairs: an IoU of 0 passes no positive threshold)
      if (truth_class[j - 1] != cls) continue;
      const bool cr = crowd && crowd[j - 1];
      if (tm[j - 1] != 0 && !cr) continue;
      const double v = mn_match_iou_of(inter, ap, w->area_g[j - 1], cr);
      if (!(v >= lo)) continue;
      const int kj = (w->ign_g[j - 1] ? 8192 : 16384) + j;
      // (j ascends within a lane: among equal groups and IoUs the later one has the greater label)
      if ((kj >> 13) > (key >> 13) || ((kj >> 13) == (key >> 13) && v >= best)) { key = kj; best = v; }
    }
    for (int s = 32; s > 0; s >>= 1) {
      const int okey = __shfl_xor(key, s);
      const double obest = __shfl_xor(best, s);
      const int g0 = key >> 13, g1 = okey >> 13;
      if (g1 > g0 || (g1 == g0 && (obest > best || (obest == best && okey > key)))) { key = okey; best = obest; }
    }
    const int buf = taken++ & 1;
    if ((tid & 63) == 0) { s_key[buf][tid >> 6] = key; s_iou[buf][tid >> 6] = best; }
    __syncthreads();
    key = s_key[buf][0]; best = s_iou[buf][0];
#pragma unroll
    for (int q = 1; q < MN_MATCH_THREADS / 64; q++) {
      const int okey = s_key[buf][q];
      const double obest = s_iou[buf][q];
      const int g0 = key >> 13, g1 = okey >> 13;
      if (g1 > g0 || (g1 == g0 && (obest > best || (obest == best && okey > key)))) { key = okey; best = obest; }
    }
    const int m = key & 8191;                         // the matched truth label, 0 = none (labels <= 4096)
    if (m && ((m - 1) % MN_MATCH_THREADS) == tid) tm[m - 1] = d;     // a crowd instance keeps the last d
    if (tid == 0) {
      pred_match[(size_t)t * K + (d - 1)] = m;
      pred_ignore[(size_t)t * K + (d - 1)] = m ? w->ign_g[m - 1] : ((ap < area_lo || ap > area_hi) ? 1 : 0);
    }
  }
  for (int j = tid; j < G; j += MN_MATCH_THREADS) truth_match[(size_t)t * G + j] = tm[j];
}
