// mn_kernels_mapscore.h -- the network's maps themselves against the ground truth, on the device: the confusion
// matrix of the argmax class and, per offset, the soft intersection / union sums of "different instance".
//
// Reference work replaced (every validation pass, on the host, one plane copy per offset):
//   runningScore.update / _fast_hist   utils/score.py:20-32     argmax of the class planes -> confusion matrix
//   offsetIoU.update                   utils/score.py:77-86     sum((1-pred)*(1-gt)), sum(1-pred) + sum(1-gt) - that
//   their callers                      utils/train_utils.py:84-121,183-219, utils/inference_utils.py:46-47,98-99
//   the targets they are fed           utils/dataset.py:259-277 (mn_sameness_targets: never materialised here)
// Definitions (mergenet_hip.h gives them in full; labels.map_scores is the numpy statement):
//   p                = the element widened to float32 (mn_sigmoid of it for logits); no clip, no bias;
//   predicted class  = lowest index among the greatest p over the C class planes;
//                      (a NaN is outside the contract, as in every other pass: it is never greater, numpy takes it)
//   truth class      = 0 for truth label 0 (and any label outside 0..G), truth_classes[g - 1] for label g;
//                      pixels whose truth class is outside 0..C-1 are left out of the confusion matrix;
//   per offset k     = (di, dj): a pixel is DIFFERENT when (r + di, c + dj) is inside the image and carries another
//                      truth label (the raw labels are compared, as mn_sameness_targets does); d = 1.0f - p;
//                      sums[0][k] = sum of d over the different pixels, sums[1][k] = sum of d over all pixels,
//                      sums[2][k] = the number of different pixels; float64 sums.
#pragma once

#include "mn_device.h"
#include "mn_row_walk.h"
#include "mn_truth_pass.h"        // what this pass shares with mn_mask_bce_pass: the grid, the truth reads, the sums

#define MN_MS_THREADS 256
#define MN_MS_WAVES (MN_MS_THREADS / 64)
#define MN_MS_OG 5                /* offsets whose loads are in flight together (and whose sums a lane holds) */
#define MN_MS_CG 4                /* class planes whose loads are in flight together */
#define MN_MS_LDS_CLASSES 32      /* C <= this: the confusion counts of a workgroup gather in LDS (C * C ints, 4 KB
                                     at most -- no occupancy lost); above it every count is a global atomic */
#define MN_MS_MAX_WIDTH (1 << 30) /* widest image taken: a row's chunks are counted in ints, chunk * 64 * V + lane * V
                                     stays below W + 512 (the entry point refuses a wider image) */

struct MnMapScoreArgs {
  const void* cls;                // [C][N]
  const void* same;               // [O][N]
  const int* truth;               // [N] label mask
  const int* truth_classes;       // [G] (may be null when G == 0)
  int H, W, C, O, G;
  RowWalk walk;                   // walk.blocks: the grid, and the slots of the partials buffer
  unsigned long long* confusion;  // [C][C], added to
  double* partials;               // [3 * O][walk.blocks]
  int di[MN_MAX_OFFSETS];
  int dj[MN_MAX_OFFSETS];
};

__device__ __forceinline__ void mn_ms_count(int* sh, bool lds, unsigned long long* confusion, int key, int n) {
  if (lds) atomicAdd(&sh[key], n);
  else atomicAdd(confusion + key, (unsigned long long)n);
}

// The walk of mn_row_walk.h, V = 8, 4 or 1 by the maps' width and bases (the truth mask is read unaligned), in two
// passes over the wave's chunks, so that every map element is loaded once:
//   1. the class planes, MN_MS_CG in flight: the running argmax per pixel (a later plane wins only when greater:
//      the lowest index among equals), then one count per pixel at (truth class, predicted class);
//   2. the sameness planes in groups of MN_MS_OG offsets: per offset of the group a lane keeps its two float64 sums
//      and its count in registers over all its chunks; the wave adds them up with a fixed butterfly of shuffles.
// The truth mask is read through the cache: a pixel's own label once per pass and group, its neighbour once per offset
// (the rule: mn_truth_pass.h).  Every load of a map is the walk's wide one: V follows the bases.  The workgroup's 3 * O sums
// go to its slot of the partials buffer, mn_map_scores_finish adds the slots up.  No floating-point atomic anywhere.
template <int DT, bool LG, int V>
__global__ __launch_bounds__(MN_MS_THREADS) void mn_map_scores_pass(const MnMapScoreArgs A) {
  __shared__ int sh_conf[MN_MS_LDS_CLASSES * MN_MS_LDS_CLASSES];
  __shared__ double sh_part[MN_MS_WAVES][MN_MS_VALUES];
  const int H = A.H, W = A.W, C = A.C, O = A.O, G = A.G;
  const size_t N = (size_t)H * (size_t)W;
  const bool lds = C <= MN_MS_LDS_CLASSES;
  if (lds) {
    for (int i = threadIdx.x; i < C * C; i += MN_MS_THREADS) sh_conf[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const RowSpan span = row_walk_span(A.walk, (long long)blockIdx.x * MN_MS_WAVES + wv);

  // ---- 1. class planes -> confusion counts ----
  for (long long c = span.c0; c < span.c1; c++) {
    int x, y;
    row_walk_pixel(A.walk, V, c, lane, &x, &y);
    const bool in = x < W;
    const size_t at = (size_t)y * W + (size_t)(in ? x : 0);
    float best[V];
    int arg[V], key[V];
#pragma unroll
    for (int j = 0; j < V; j++) { best[j] = 0.0f; arg[j] = 0; key[j] = -1; }
    if (in) {
      for (int q0 = 0; q0 < C; q0 += MN_MS_CG) {
        float v[MN_MS_CG][V];
#pragma unroll
        for (int q = 0; q < MN_MS_CG; q++)
          if (q0 + q < C) mn_plane_load<DT, LG, V>(A.cls, (size_t)(q0 + q) * N + at, true, v[q]);
#pragma unroll
        for (int q = 0; q < MN_MS_CG; q++) {
          if (q0 + q >= C) continue;
#pragma unroll
          for (int j = 0; j < V; j++)
            if (q0 + q == 0 || v[q][j] > best[j]) { best[j] = v[q][j]; arg[j] = q0 + q; }
        }
      }
      int t[V];
      mn_walk_labels<V, false>(A.truth + at, t);
#pragma unroll
      for (int j = 0; j < V; j++) {
        const int tc = mn_truth_class(t[j], A.truth_classes, G);
        key[j] = ((unsigned)tc < (unsigned)C) ? tc * C + arg[j] : -1;        // (the test of mn_kept_class)
      }
    }
    // A chunk that lies in one (truth class, predicted class) cell -- most of an image -- is ONE count; any other
    // chunk counts per lane, equal neighbours within the lane joined.
    const int k0 = __shfl(key[0], 0);
    bool same = true;
#pragma unroll
    for (int j = 0; j < V; j++) same = same && key[j] == k0;
    if (__ballot(same) == ~0ull) {
      if (lane == 0 && k0 >= 0) mn_ms_count(sh_conf, lds, A.confusion, k0, 64 * V);
    } else {
      int run = 0;
#pragma unroll
      for (int j = 0; j < V; j++) {
        run++;
        const int next = j + 1 < V ? key[j + 1 < V ? j + 1 : j] : -2;      // (-2: no key, the lane's last run ends)
        if (next != key[j]) {
          if (key[j] >= 0) mn_ms_count(sh_conf, lds, A.confusion, key[j], run);
          run = 0;
        }
      }
    }
  }

  // ---- 2. sameness planes -> the three sums per offset ----
  for (int g0 = 0; g0 < O; g0 += MN_MS_OG) {
    double s_diff[MN_MS_OG], s_all[MN_MS_OG];
    int n_diff[MN_MS_OG];
#pragma unroll
    for (int g = 0; g < MN_MS_OG; g++) { s_diff[g] = 0.0; s_all[g] = 0.0; n_diff[g] = 0; }
    for (long long c = span.c0; c < span.c1; c++) {
      int x, y;
      row_walk_pixel(A.walk, V, c, lane, &x, &y);
      if (x >= W) continue;                          // (no shuffle or barrier inside this loop)
      const size_t at = (size_t)y * W + (size_t)x;
      float v[MN_MS_OG][V];
#pragma unroll
      for (int g = 0; g < MN_MS_OG; g++)
        if (g0 + g < O) mn_plane_load<DT, LG, V>(A.same, (size_t)(g0 + g) * N + at, true, v[g]);
      int t[V];
      mn_walk_labels<V, false>(A.truth + at, t);
#pragma unroll
      for (int g = 0; g < MN_MS_OG; g++) {
        if (g0 + g >= O) continue;
        const unsigned yy = (unsigned)y + (unsigned)A.di[g0 + g], xx = (unsigned)x + (unsigned)A.dj[g0 + g];
        int nb[V];
#pragma unroll
        for (int j = 0; j < V; j++) nb[j] = t[j];    // (the neighbour rule of mn_truth_pass.h)
        if (yy < (unsigned)H) {
          const int* row = A.truth + (size_t)yy * W;
          if (V >= 4 && xx < (unsigned)W && xx + V <= (unsigned)W) {
            mn_walk_labels<V, false>(row + xx, nb);
          } else {
#pragma unroll
            for (int j = 0; j < V; j++)
              if (xx + j < (unsigned)W) nb[j] = row[xx + j];
          }
        }
#pragma unroll
        for (int j = 0; j < V; j++) {
          const double d = (double)(1.0f - v[g][j]);
          const bool diff = nb[j] != t[j];
          s_all[g] += d;
          s_diff[g] += diff ? d : 0.0;
          n_diff[g] += diff ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < MN_MS_OG; g++) {
      if (g0 + g >= O) continue;
      double a = s_diff[g], b = s_all[g];
      long long n = n_diff[g];
      mn_wave_sums(a, b, n);
      if (lane == 0) {
        sh_part[wv][g0 + g] = a;
        sh_part[wv][O + g0 + g] = b;
        sh_part[wv][2 * O + g0 + g] = (double)n;     // (an integer below 2^53: exact)
      }
    }
  }

  mn_truth_flush<MN_MS_WAVES>(sh_part, 3 * O, A.partials, A.walk.blocks);
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += MN_MS_THREADS) {
      const int n = sh_conf[i];
      if (n) atomicAdd(A.confusion + i, (unsigned long long)n);
    }
}
