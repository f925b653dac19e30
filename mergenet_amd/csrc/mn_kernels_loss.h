// mn_kernels_loss.h -- the training criterion from the label mask: the BCE-with-logits loss of the class planes and
// of the offset planes and, in the same pass, its gradient.  No target plane is written or read.
//
// Reference work replaced (every training and validation step):
//   torch.nn.BCEWithLogitsLoss on both parts   egs/cityscape/local/train.py:183-195, egs/coco/local/train.py:145,156
//   cls_loss + alpha * ofs_loss, backward      utils/train_utils.py:42-79,145-180
//   the targets they are fed                   utils/dataset.py:259-277 (offsets), :419-429 (classes)
// Definitions (mergenet_hip.h gives them in full; labels.mask_bce is the numpy statement):
//   x            = the element widened exactly to float32;
//   truth class  = 0 for truth label 0 (and any label outside 0..G), truth_classes[g - 1] for label g;
//   target y     = class plane q: (truth class == q); offset plane k = (di, dj): 1 unless (r + di, c + dj) is inside
//                  the image and carries another truth label (raw labels, the rule of mn_map_scores_pass);
//   term         = softplus(z), z = y ? -x : x, as fmaxf(z, 0) + log1pf(expf(-fabsf(z))) in float32;
//   gradient     = (mn_sigmoid(x) - y) * scale in float32, rounded to nearest even into the element type;
//   ignore class = a pixel whose truth class is outside 0..C-1: no class term, gradient 0 on every class plane
//                  (the store is made); it takes part in the offset planes like any other pixel;
//   sums         = float64 [2 + O]: [0] class terms of the kept pixels, [1 + k] terms of offset plane k,
//                  [1 + O] the number of kept pixels.
// expf(-|z|) is a normal float32 up to |x| of about 87 and underflows beyond: from there the term of a wrong-side
// logit is still |x| to the last bit, the term of a right-side one falls to 0 through the subnormals -- outside the
// relative bound the tests hold the sums to (2^-21 per term).  NaN in a map is undefined, as in every other pass.
//
// Resource report of the compiler for gfx950 (-Rpass-analysis=kernel-resource-usage): no scratch and no spilled
// VGPR in any of the eight instantiations (float32 has no 8-pixel form: a 16-byte access is four of its elements).
//   pixels per lane        float32     float16     bfloat16        (VGPRs; waves per SIMD: 4 at 8 pixels per lane,
//          8                  --         107         111            6 at 4, 8 at 1)
//          4                  77          76          78
//          1                  58          58          58
#pragma once

#include "mn_device.h"
#include "mn_row_walk.h"
#include "mn_truth_pass.h"        // what this pass shares with mn_map_scores_pass: the grid, the truth reads, the sums

#define MN_BCE_THREADS 256
#define MN_BCE_WAVES (MN_BCE_THREADS / 64)
#define MN_BCE_OG 5               /* offset planes whose loads are in flight together (and whose sums a lane holds) */
#define MN_BCE_CG 4               /* class planes whose loads are in flight together */

struct MnMaskBceArgs {
  const void* cls;                // [C][N] logits (null when C == 0)
  const void* same;               // [O][N] logits (null when O == 0)
  void* gcls;                     // [C][N] gradient, the maps' element type, or null
  void* gsame;                    // [O][N] gradient or null
  const int* truth;               // [N] label mask
  const int* truth_classes;       // [G] (may be null when G == 0)
  int H, W, C, O, G;
  int wide;                       // every map and gradient base admits the wide access of the walk's P pixels
  float scale_cls, scale_same;
  RowWalk walk;                   // walk.blocks: the grid, and the slots of the partials buffer; walk.v: P
  double* partials;               // [2 + O][walk.blocks]
  int di[MN_MAX_OFFSETS];
  int dj[MN_MAX_OFFSETS];
};

__device__ __forceinline__ float mn_bce_term(float x, bool y) {
  const float z = y ? -x : x;     // x - x * y without the product: exact for y in {0, 1}
  return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z)));
}
__device__ __forceinline__ float mn_bce_grad(float x, bool y, float scale) {
  return (mn_sigmoid(x) - (y ? 1.0f : 0.0f)) * scale;
}

// The walk of mn_row_walk.h with P pixels per lane, P = 8, 4 or 1 by the element size and the WIDTH alone
// (row_walk_v without bases), so that which pixels a lane holds, and with that the grouping of every float64 sum,
// does not depend on where the caller's buffers lie: bases that do not admit the wide access (A.wide == 0) change
// the loads and stores to single elements (mn_plane_load / mn_plane_store), not the walk.  The sums of an image are
// therefore the same bits whatever the alignment of the maps and gradients, and whether or not a gradient is written.
//   1. the class planes, MN_BCE_CG in flight: per pixel its truth class once, then per plane the term (added to the
//      lane's float64 sum for a kept pixel) and the gradient, stored as soon as the group's values are in;
//   2. the offset planes in groups of MN_BCE_OG: per offset of the group a lane keeps its float64 sum in registers
//      over all its chunks, as mn_map_scores_pass does; neighbour labels by the same rule (mn_truth_pass.h).
// Every map element is loaded once and every gradient element stored once; a lane past W loads and stores nothing.
// The truth mask is read through the cache.  The wave adds its lanes' sums with the fixed butterfly, the workgroup
// writes all 2 + O values to its slot of the partials buffer (no clearing needed), mn_map_scores_finish adds the
// slots in a fixed order.  No floating-point atomic anywhere.
template <int DT, int P>
__global__ __launch_bounds__(MN_BCE_THREADS) void mn_mask_bce_pass(const MnMaskBceArgs A) {
  __shared__ double sh_part[MN_BCE_WAVES][MN_BCE_VALUES];
  const int H = A.H, W = A.W, C = A.C, O = A.O, G = A.G;
  const size_t N = (size_t)H * (size_t)W;
  const bool wide = A.wide != 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const RowSpan span = row_walk_span(A.walk, (long long)blockIdx.x * MN_BCE_WAVES + wv);

  // ---- 1. class planes ----
  {
    double s_cls = 0.0;
    int kept = 0;
    const bool want = A.gcls != nullptr;
    const float scale = A.scale_cls;
    if (C > 0) {
      for (long long c = span.c0; c < span.c1; c++) {
        int x, y;
        row_walk_pixel(A.walk, P, c, lane, &x, &y);
        if (x >= W) continue;                          // (no shuffle or barrier inside this loop)
        const size_t at = (size_t)y * W + (size_t)x;
        int t[P], tc[P];
        mn_walk_labels<P, false>(A.truth + at, t);
#pragma unroll
        for (int j = 0; j < P; j++) {
          tc[j] = mn_kept_class(t[j], A.truth_classes, G, C);
          kept += tc[j] >= 0 ? 1 : 0;
        }
        for (int q0 = 0; q0 < C; q0 += MN_BCE_CG) {
          float v[MN_BCE_CG][P];
#pragma unroll
          for (int q = 0; q < MN_BCE_CG; q++)
            if (q0 + q < C) mn_plane_load<DT, false, P>(A.cls, (size_t)(q0 + q) * N + at, wide, v[q]);
#pragma unroll
          for (int q = 0; q < MN_BCE_CG; q++) {
            if (q0 + q >= C) continue;
            float g[P];
#pragma unroll
            for (int j = 0; j < P; j++) {
              const bool yes = tc[j] == q0 + q, keep = tc[j] >= 0;
              const double term = (double)mn_bce_term(v[q][j], yes);
              s_cls += keep ? term : 0.0;
              if (want) g[j] = keep ? mn_bce_grad(v[q][j], yes, scale) : 0.0f;
            }
            if (want) mn_plane_store<DT, P>(A.gcls, (size_t)(q0 + q) * N + at, wide, g);
          }
        }
      }
    }
    long long n = kept;
    mn_wave_sums(s_cls, n);
    if (lane == 0) {
      sh_part[wv][0] = s_cls;
      sh_part[wv][1 + O] = (double)n;                  // (an integer below 2^53: exact)
    }
  }

  // ---- 2. offset planes ----
  {
    const bool want = A.gsame != nullptr;
    const float scale = A.scale_same;
    for (int g0 = 0; g0 < O; g0 += MN_BCE_OG) {
      double s_same[MN_BCE_OG];
#pragma unroll
      for (int g = 0; g < MN_BCE_OG; g++) s_same[g] = 0.0;
      for (long long c = span.c0; c < span.c1; c++) {
        int x, y;
        row_walk_pixel(A.walk, P, c, lane, &x, &y);
        if (x >= W) continue;
        const size_t at = (size_t)y * W + (size_t)x;
        float v[MN_BCE_OG][P];
#pragma unroll
        for (int g = 0; g < MN_BCE_OG; g++)
          if (g0 + g < O) mn_plane_load<DT, false, P>(A.same, (size_t)(g0 + g) * N + at, wide, v[g]);
        int t[P];
        mn_walk_labels<P, false>(A.truth + at, t);
#pragma unroll
        for (int g = 0; g < MN_BCE_OG; g++) {
          if (g0 + g >= O) continue;
          const unsigned yy = (unsigned)y + (unsigned)A.di[g0 + g], xx = (unsigned)x + (unsigned)A.dj[g0 + g];
          int nb[P];
#pragma unroll
          for (int j = 0; j < P; j++) nb[j] = t[j];    // (the neighbour rule of mn_truth_pass.h)
          if (yy < (unsigned)H) {
            const int* row = A.truth + (size_t)yy * W;
            if (P >= 4 && xx < (unsigned)W && xx + P <= (unsigned)W) {
              mn_walk_labels<P, false>(row + xx, nb);
            } else {
#pragma unroll
              for (int j = 0; j < P; j++)
                if (xx + j < (unsigned)W) nb[j] = row[xx + j];
            }
          }
          float gr[P];
#pragma unroll
          for (int j = 0; j < P; j++) {
            const bool yes = nb[j] == t[j];
            s_same[g] += (double)mn_bce_term(v[g][j], yes);
            if (want) gr[j] = mn_bce_grad(v[g][j], yes, scale);
          }
          if (want) mn_plane_store<DT, P>(A.gsame, (size_t)(g0 + g) * N + at, wide, gr);
        }
      }
#pragma unroll
      for (int g = 0; g < MN_BCE_OG; g++) {
        if (g0 + g >= O) continue;
        double a = s_same[g];
        mn_wave_sums(a);
        if (lane == 0) sh_part[wv][1 + g0 + g] = a;
      }
    }
  }

  mn_truth_flush<MN_BCE_WAVES>(sh_part, 2 + O, A.partials, A.walk.blocks);
}
