// mn_kernels_instances.h -- the instance table of a label mask on the device: area and bounding box per
// instance, the small-instance filter and the dense renumbering of the survivors.
//
// Reference work replaced (the Cityscapes caller and its evaluator):
//   convert_to_coco_result            egs/cityscape/local/segment.py:165-186   one result per instance
//   the zero-area drop                egs/cityscape/local/evaluate.py:52-54    before COCOeval
//   (COCO.loadRes then derives area and bbox from every RLE on the host)
// Definitions, the whole of both computations:
//   table[k-1] = {number of pixels with label k, least x, least y, greatest x, greatest y of those pixels}, and
//                {0, W, H, -1, -1} -- the identities of sum, min and max over the image -- where there is none;
//   the filter keeps label k iff area[k-1] >= min_area (and score[k-1] >= min_score where scores are given) and
//                gives the kept labels the numbers 1..K' in ascending old label, every other pixel 0.
#pragma once

#include "mn_device.h"
#include "mn_row_walk.h"

// Two constants of the pass; a variant build for tools/time_instance_table.py may set them (-D...):
#ifndef MN_INST_LDS_LABELS
#define MN_INST_LDS_LABELS 1024   /* labels a workgroup accumulates in LDS: 5 x 4 KB = 20 KB, 8 workgroups per CU;
                                     0 = no LDS table, every run updates the global table (the simpler form) */
#endif
#ifndef MN_INST_WORKGROUPS
#define MN_INST_WORKGROUPS 256    /* workgroups aimed at (one per CU): a wave walks total loads / (4 x this) loads in
                                     a row, so that a workgroup's LDS table gathers several rows before it is
                                     flushed; at 1024x2048 that is 8 loads (measured: 1 / 2 / 4 / 8 / 16 loads per
                                     wave take 48 / 29 / 18 / 15 / 18 us, profiles/instance_table_time.log) */
#endif
#define MN_INST_THREADS 256
#define MN_INST_LDS (MN_INST_LDS_LABELS > 0)

__global__ __launch_bounds__(256) void mn_instance_table_init(int K, int H, int W, int* __restrict__ table) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  int* r = table + 5 * (size_t)k;
  r[0] = 0; r[1] = W; r[2] = H; r[3] = -1; r[4] = -1;
}

// One run of `len` pixels of `label` (1..K) on row y, columns xs..xe: into the workgroup's LDS table (fields
// apart, MN_INST_LDS_LABELS ints each) for the labels it holds, else straight into the global table.
__device__ __forceinline__ void mn_inst_run(int* sh, int lds_rows, int* __restrict__ table, int label, int len,
                                            int xs, int xe, int y) {
  const int l = label - 1;
  if (MN_INST_LDS && l < lds_rows) {
    atomicAdd(&sh[l], len);
    atomicMin(&sh[MN_INST_LDS_LABELS + l], xs);
    atomicMin(&sh[2 * MN_INST_LDS_LABELS + l], y);
    atomicMax(&sh[3 * MN_INST_LDS_LABELS + l], xe);
    atomicMax(&sh[4 * MN_INST_LDS_LABELS + l], y);
  } else {
    int* r = table + 5 * (size_t)l;
    atomicAdd(r, len);
    atomicMin(r + 1, xs);
    atomicMin(r + 2, y);
    atomicMax(r + 3, xe);
    atomicMax(r + 4, y);
  }
}

// The walk of mn_row_walk.h over one mask, V = 4 or 1, the next chunk's load in flight over this chunk's work.
// Masks are piecewise constant along a row, so only the first pixel of a run (its head) updates the table: the
// heads are found against the pixel before (the lane before for a lane's first pixel; the first pixel of a chunk
// is always a head), and a head reads where its run ends from mn_walk_run_end.
// Label 0 and every label outside 1..K -- the mask is the caller's memory -- are read as 0 and update nothing;
// so are the pixels of a row's last chunk past W.
template <int V>
__global__ __launch_bounds__(MN_INST_THREADS) void mn_instance_table_runs(const int* __restrict__ mask, int H, int W,
                                                                          int K, const RowWalk R,
                                                                          int* __restrict__ table) {
  __shared__ int sh[MN_INST_LDS ? 5 * MN_INST_LDS_LABELS : 1];
  const int lds_rows = min(K, MN_INST_LDS_LABELS);
  if (MN_INST_LDS) {
    for (int i = threadIdx.x; i < lds_rows; i += MN_INST_THREADS) {
      sh[i] = 0;
      sh[MN_INST_LDS_LABELS + i] = W;
      sh[2 * MN_INST_LDS_LABELS + i] = H;
      sh[3 * MN_INST_LDS_LABELS + i] = -1;
      sh[4 * MN_INST_LDS_LABELS + i] = -1;
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const RowSpan span = row_walk_span(R, (long long)blockIdx.x * (MN_INST_THREADS / 64) + (threadIdx.x >> 6));

  auto load = [&](long long c, int* a, int* xo, int* yo) {
    row_walk_pixel(R, V, c, lane, xo, yo);
    const int x = *xo, y = *yo;
#pragma unroll
    for (int j = 0; j < V; j++) a[j] = 0;
    if (x < W) {
      mn_walk_labels<V, true>(mask + (size_t)y * W + x, a);
#pragma unroll
      for (int j = 0; j < V; j++) a[j] = ((unsigned)(a[j] - 1) < (unsigned)K) ? a[j] : 0;
    }
  };

  int nxt[V], nx = 0, ny = 0;
  if (span.c0 < span.c1) load(span.c0, nxt, &nx, &ny);
  for (long long c = span.c0; c < span.c1; c++) {
    int a[V];
#pragma unroll
    for (int j = 0; j < V; j++) a[j] = nxt[j];
    const int x = nx, y = ny;
    if (c + 1 < span.c1) load(c + 1, nxt, &nx, &ny);     // the next chunk's load is in flight over this chunk's work

    int before = __shfl_up(a[V - 1], 1);
    if (lane == 0) before = -1;                      // (labels are >= 0 here: the chunk's first pixel is a head)
    bool head[V];
#pragma unroll
    for (int j = 0; j < V; j++) head[j] = a[j] != (j == 0 ? before : a[j > 0 ? j - 1 : 0]);
    const int next_head = mn_walk_next_head<V>(head, lane);
#pragma unroll
    for (int j = 0; j < V; j++) {
      if (!head[j] || a[j] == 0) continue;
      const int len = mn_walk_run_end<V>(head, j, next_head) - j;
      // (a run of a label > 0 ends before the pixels past W, which read as 0: xs + len - 1 < W)
      mn_inst_run(sh, lds_rows, table, a[j], len, x + j, x + j + len - 1, y);
    }
  }

  if (MN_INST_LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < lds_rows; i += MN_INST_THREADS) {
      const int n = sh[i];
      if (n == 0) continue;                          // only the rows this workgroup touched
      int* r = table + 5 * (size_t)i;
      atomicAdd(r, n);
      atomicMin(r + 1, sh[MN_INST_LDS_LABELS + i]);
      atomicMin(r + 2, sh[2 * MN_INST_LDS_LABELS + i]);
      atomicMax(r + 3, sh[3 * MN_INST_LDS_LABELS + i]);
      atomicMax(r + 4, sh[4 * MN_INST_LDS_LABELS + i]);
    }
  }
}

// keep[k] = area >= min_area && (no scores || score >= min_score); remap[0] = 0, remap[k] = 1 + kept labels below
// k, or 0; table, class table and scores of the kept labels move to their new places OUT of place; the class
// table is -1 from K' up to K (segment.cc:497-509, the library's convention); *new_count = K'.
// ONE workgroup of 1024 lanes walks the labels 1024 at a time with a running count (the pattern of mn_rank_scan
// and mn_rank_assign: a ballot per wave, the 16 wave counts through LDS), so any K is served in order.
__global__ __launch_bounds__(1024) void mn_instance_keep(int K, const int* __restrict__ table,
                                                         const int* __restrict__ object_class,
                                                         const float* __restrict__ scores, int min_area,
                                                         float min_score, int* __restrict__ remap,
                                                         int* __restrict__ table_out,
                                                         int* __restrict__ object_class_out,
                                                         float* __restrict__ scores_out,
                                                         int* __restrict__ new_count) {
  __shared__ int sh_w[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int running = 0;
  if (threadIdx.x == 0) remap[0] = 0;
  for (int base = 0; base < K; base += 1024) {
    const int k = base + (int)threadIdx.x;           // label k + 1
    bool keep = false;
    if (k < K) keep = table[5 * (size_t)k] >= min_area && (!scores || scores[k] >= min_score);
    const u64 m = __ballot(keep);
    if (lane == 0) sh_w[wave] = __popcll(m);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < 16; w++) { if (w < wave) woff += sh_w[w]; tot += sh_w[w]; }
    if (k < K) {
      if (keep) {
        const int r = running + woff + __popcll(m & ((1ull << lane) - 1ull));
        remap[k + 1] = r + 1;
        for (int f = 0; f < 5; f++) table_out[5 * (size_t)r + f] = table[5 * (size_t)k + f];
        object_class_out[r] = object_class[k];
        if (scores) scores_out[r] = scores[k];
      } else {
        remap[k + 1] = 0;
      }
    }
    running += tot;
    __syncthreads();
  }
  for (int k = running + (int)threadIdx.x; k < K; k += 1024) object_class_out[k] = -1;
  if (threadIdx.x == 0) *new_count = running;
}

// out[p] = remap[mask[p]] for labels 0..K, 0 for anything else.  A lane reads its own pixels before it writes
// them and no other lane's, so out may be the mask itself (neither is __restrict__).
__global__ __launch_bounds__(256) void mn_relabel_mask(const int* mask, size_t N, int K,
                                                       const int* __restrict__ remap, int* out) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int v = mask[p];
  out[p] = ((unsigned)v <= (unsigned)K) ? remap[v] : 0;
}

// The same, four pixels per lane (N % 4 == 0, both buffers 16-byte aligned).
__global__ __launch_bounds__(256) void mn_relabel_mask4(const int* mask, size_t N4, int K,
                                                        const int* __restrict__ remap, int* out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N4) return;
  const int4 v = *reinterpret_cast<const int4*>(mask + 4 * g);
  int4 o;
  o.x = ((unsigned)v.x <= (unsigned)K) ? remap[v.x] : 0;
  o.y = ((unsigned)v.y <= (unsigned)K) ? remap[v.y] : 0;
  o.z = ((unsigned)v.z <= (unsigned)K) ? remap[v.z] : 0;
  o.w = ((unsigned)v.w <= (unsigned)K) ? remap[v.w] : 0;
  *reinterpret_cast<int4*>(out + 4 * g) = o;
}
