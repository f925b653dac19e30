// mn_kernels_planeloss.h -- the criteria whose gradient needs totals over a whole plane, from the label mask: the
// soft Dice loss and the weighted multi-BCE loss.  No target plane is written or read.
//
// Reference work replaced (training with --loss dice / --loss mbce):
//   SoftDiceLoss, MultiBCEWithLogitsLoss       utils/loss.py:38-76
//   their selection for a part of the output   egs/cityscape/local/train.py:193-204, egs/coco/local/train.py:143-154
//   the targets they are fed                   utils/dataset.py:259-277 (offsets), :419-429 (classes)
// The gradient of an element depends on sums over its plane, so one pass cannot do it.  Three steps, one part of the
// network's output (the class planes or the offset planes) per call:
//   1. mn_plane_sums_pass    per plane the sums below, float64, in the manner of mn_mask_bce_pass;
//   2. mn_plane_coeffs       per plane the value of the criterion and four float32 coefficients, one small launch;
//   3. mn_plane_grad_pass    the gradient from the logits, the label mask and the coefficients.
// Definitions (mergenet_hip.h gives them in full; labels.plane_sums / plane_coeffs / plane_grad are the numpy statement):
//   x, truth class, target y, ignore class: as in mn_kernels_loss.h (MN_PART_CLASS: its class planes, MN_PART_OFFSET:
//   its offset planes; the ignore class exists in the class part only);
//   s = mn_sigmoid(x);  MN_PLANE_COMPLEMENT: q = mn_sigmoid(-x), z = !y -- never 1 - s, which cancels where the z set
//   is sparse (mode '0' on offset planes) -- else q = s, z = y;  term = mn_bce_term(x, y);
//   sums float64 [5 * P + 1], row r of plane p at r * P + p: Q = sum q, I = sum of q where z, Z = number of z,
//   L1 = sum of term where y, L0 = sum of term where !y (both 0 without MN_PLANE_TERMS: no log1pf is spent), then the
//   number of pixels that took part;
//   gradient = f * (q * (1 - q) * (z ? c0 : c1) + (s - y) * (y ? c2 : c3)) in float32, rounded to nearest even into
//   the element type; 0 for an ignored pixel (the store is made).
// expf of the sigmoid is a normal float32 up to |x| of about 87, as in mn_kernels_loss.h.  NaN in a map is undefined.
//
// Resource report of the compiler for gfx950 (-Rpass-analysis=kernel-resource-usage): no scratch and no spilled
// VGPR in any of the 24 instantiations (float32 has no 8-pixel form: a 16-byte access is four of its elements).
//   VGPRs                          float32     float16     bfloat16
//   sums, terms     8 per lane        --         172         172
//                   4                134         133         133
//                   1                103         103         103
//   sums, no terms  8                 --         128         128
//                   4                 96          96          95
//                   1                 74          74          74
//   gradient        8                 --          91         106
//                   4                 65          65          80
//                   1                 37          33          34
// Waves per SIMD: sums with terms 2 / 3 / 4 at 8 / 4 / 1 pixels per lane, without them 4 / 5 / 6; gradient 4-5 / 6-7 / 7.
// mn_plane_coeffs: 42 VGPRs, 1 KiB of LDS.  The sums pass holds 20 KiB of LDS (its 5 * 127 + 1 values per wave).
#pragma once

#include "mn_device.h"
#include "mn_row_walk.h"
#include "mn_truth_pass.h"
#include "mn_kernels_loss.h"      // mn_bce_term

#define MN_PL_THREADS 256
#define MN_PL_WAVES (MN_PL_THREADS / 64)
#define MN_PL_G 4                 /* planes whose loads are in flight together (and whose sums a lane holds) */
#define MN_PL_ROWS 5
#define MN_PL_VALUES (MN_PL_ROWS * MN_MAX_CLASSES + 1)   /* more than MN_MS_VALUES: a partials buffer of its own */
#define MN_PL_COEFF_THREADS 128
static_assert(MN_MAX_OFFSETS <= MN_MAX_CLASSES && MN_MAX_CLASSES <= MN_PL_COEFF_THREADS,
              "the class part has the most planes; mn_plane_coeffs takes one plane per thread");

struct MnPlaneArgs {
  const void* maps;               // [NP][N] logits
  void* grad;                     // [NP][N] gradient, the maps' element type (the gradient pass)
  const int* truth;               // [N] label mask
  const int* truth_classes;       // [G] (may be null when G == 0; the class part only)
  const float* coeffs;            // [4][NP] (the gradient pass)
  const float* factor;            // one float32 or null (the gradient pass)
  int H, W, NP, G;
  int part;                       // MN_PART_CLASS or MN_PART_OFFSET
  int comp;                       // MN_PLANE_COMPLEMENT
  int wide;                       // every map and gradient base admits the wide access of the walk's P pixels
  RowWalk walk;                   // walk.blocks: the grid, and the slots of the partials buffer; walk.v: P
  double* partials;               // [5 * NP + 1][walk.blocks] (the sums pass)
  int di[MN_MAX_OFFSETS];
  int dj[MN_MAX_OFFSETS];
};

// The truth classes of a lane's P pixels (class part; -1: an ignored pixel).
template <int P>
__device__ __forceinline__ void mn_plane_classes(const MnPlaneArgs& A, const int* t, int* tc) {
#pragma unroll
  for (int j = 0; j < P; j++) tc[j] = mn_kept_class(t[j], A.truth_classes, A.G, A.NP);
}
// The targets of plane pl for a lane's P pixels from column x of row y: yes[j] = the target is 1, keep[j] = the pixel
// takes part.  Class part: from the truth classes tc.  Offset part: from the labels t and the neighbours' (the
// neighbour rule of mn_truth_pass.h, the lines of mn_mask_bce_pass).  The part is uniform over the launch.
template <int P>
__device__ __forceinline__ void mn_plane_targets(const MnPlaneArgs& A, int pl, int x, int y, const int* t, const int* tc,
                                                 bool* yes, bool* keep) {
  if (A.part == MN_PART_CLASS) {
#pragma unroll
    for (int j = 0; j < P; j++) { yes[j] = tc[j] == pl; keep[j] = tc[j] >= 0; }
  } else {
    const int H = A.H, W = A.W;
    const unsigned yy = (unsigned)y + (unsigned)A.di[pl], xx = (unsigned)x + (unsigned)A.dj[pl];
    int nb[P];
#pragma unroll
    for (int j = 0; j < P; j++) nb[j] = t[j];
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
#pragma unroll
    for (int j = 0; j < P; j++) { yes[j] = nb[j] == t[j]; keep[j] = true; }
  }
}

// 1. The sums.  The walk of mn_mask_bce_pass: P pixels per lane by the element size and the WIDTH alone, the grid by
// (H, W, element size) alone, so the grouping of every float64 sum does not depend on where the map lies; a base
// that does not admit the wide access (A.wide == 0) changes the loads to single elements, not the walk.  The planes
// are taken in groups of MN_PL_G: a lane keeps the group's sums in registers over all its chunks (Z as an int: a lane
// holds fewer than 2^31 pixels).  Each logit is loaded once; a lane past W loads nothing.  The wave adds its lanes'
// sums with the fixed butterfly, the workgroup writes all 5 * NP + 1 values to its slot of the partials buffer (no
// clearing needed), mn_map_scores_finish adds the slots in a fixed order.  No floating-point atomic anywhere.
template <int DT, int P, bool TERMS>
__global__ __launch_bounds__(MN_PL_THREADS) void mn_plane_sums_pass(const MnPlaneArgs A) {
  __shared__ double sh_part[MN_PL_WAVES][MN_PL_VALUES];
  const int W = A.W, NP = A.NP;
  const size_t N = (size_t)A.H * (size_t)W;
  const bool wide = A.wide != 0, comp = A.comp != 0, cls = A.part == MN_PART_CLASS;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const RowSpan span = row_walk_span(A.walk, (long long)blockIdx.x * MN_PL_WAVES + wv);
  int pixels = 0;

  for (int g0 = 0; g0 < NP; g0 += MN_PL_G) {
    double sq[MN_PL_G], si[MN_PL_G], s1[MN_PL_G], s0[MN_PL_G];
    int nz[MN_PL_G];
#pragma unroll
    for (int g = 0; g < MN_PL_G; g++) { sq[g] = si[g] = s1[g] = s0[g] = 0.0; nz[g] = 0; }
    for (long long c = span.c0; c < span.c1; c++) {
      int x, y;
      row_walk_pixel(A.walk, P, c, lane, &x, &y);
      if (x >= W) continue;                            // (no shuffle or barrier inside this loop)
      const size_t at = (size_t)y * W + (size_t)x;
      float v[MN_PL_G][P];
#pragma unroll
      for (int g = 0; g < MN_PL_G; g++)
        if (g0 + g < NP) mn_plane_load<DT, false, P>(A.maps, (size_t)(g0 + g) * N + at, wide, v[g]);
      int t[P], tc[P];
      mn_walk_labels<P, false>(A.truth + at, t);
      if (cls) mn_plane_classes<P>(A, t, tc);
      if (g0 == 0) {
#pragma unroll
        for (int j = 0; j < P; j++) pixels += (!cls || tc[j] >= 0) ? 1 : 0;
      }
#pragma unroll
      for (int g = 0; g < MN_PL_G; g++) {
        if (g0 + g >= NP) continue;
        bool yes[P], keep[P];
        mn_plane_targets<P>(A, g0 + g, x, y, t, tc, yes, keep);
#pragma unroll
        for (int j = 0; j < P; j++) {
          const float xv = v[g][j];
          const bool z = yes[j] != comp;
          const double q = keep[j] ? (double)mn_sigmoid(comp ? -xv : xv) : 0.0;
          sq[g] += q;
          si[g] += z ? q : 0.0;
          nz[g] += (keep[j] && z) ? 1 : 0;
          if (TERMS) {
            const double term = keep[j] ? (double)mn_bce_term(xv, yes[j]) : 0.0;
            s1[g] += yes[j] ? term : 0.0;
            s0[g] += yes[j] ? 0.0 : term;
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < MN_PL_G; g++) {
      if (g0 + g >= NP) continue;
      double a = sq[g], b = si[g], d = s1[g], e = s0[g];
      long long n = nz[g];
      mn_wave_sums(a, b, n, d, e);
      if (lane == 0) {
        sh_part[wv][0 * NP + g0 + g] = a;
        sh_part[wv][1 * NP + g0 + g] = b;
        sh_part[wv][2 * NP + g0 + g] = (double)n;      // (an integer below 2^53: exact)
        sh_part[wv][3 * NP + g0 + g] = d;
        sh_part[wv][4 * NP + g0 + g] = e;
      }
    }
  }
  long long n = pixels;
  mn_wave_sums(n);
  if (lane == 0) sh_part[wv][MN_PL_ROWS * NP] = (double)n;
  mn_truth_flush<MN_PL_WAVES>(sh_part, MN_PL_ROWS * NP + 1, A.partials, A.walk.blocks);
}

// 2. The coefficients: one workgroup, thread p takes plane p, all in float64; each coefficient is rounded once to
// float32.  Thread 0 adds the planes' values in ascending order; the loss is stored or added to.
//   MN_CRIT_DICE   D = Q + Z + smooth, value = 1 - (2 I + smooth) / D, c1 = sigma scale (2 I + smooth) / D^2,
//                  c0 = c1 - sigma scale 2 / D, c2 = c3 = 0; sigma = -1 with the complement (dq/dx = -q (1 - q)).
//   MN_CRIT_MBCE   w = (pixels - Q + 1) / (Q + 1), value = w L1 + L0, c0 = c1 = scale L1 (-(pixels + 2) / (Q + 1)^2)
//                  (the weight's own derivative), c2 = scale w, c3 = scale.
__global__ __launch_bounds__(MN_PL_COEFF_THREADS) void mn_plane_coeffs(int criterion, int comp,
                                                                        const double* __restrict__ sums, int NP,
                                                                        double pixels, double smooth, double scale,
                                                                        float* __restrict__ coeffs,
                                                                        double* __restrict__ loss, int accumulate) {
  __shared__ double sh_value[MN_PL_COEFF_THREADS];
  const int p = threadIdx.x;
  if (p < NP) {
    const double Q = sums[p], I = sums[NP + p], Z = sums[2 * NP + p], L1 = sums[3 * NP + p], L0 = sums[4 * NP + p];
    double value, c0, c1, c2, c3;
    if (criterion == MN_CRIT_DICE) {
      const double sigma = comp ? -1.0 : 1.0, D = Q + Z + smooth, top = 2.0 * I + smooth;
      value = 1.0 - top / D;
      c1 = sigma * scale * top / (D * D);
      c0 = c1 - sigma * scale * 2.0 / D;
      c2 = c3 = 0.0;
    } else {
      const double S1 = Q + 1.0, w = (pixels - Q + 1.0) / S1;
      value = w * L1 + L0;
      c0 = c1 = scale * L1 * (-(pixels + 2.0) / (S1 * S1));
      c2 = scale * w;
      c3 = scale;
    }
    coeffs[p] = (float)c0;
    coeffs[NP + p] = (float)c1;
    coeffs[2 * NP + p] = (float)c2;
    coeffs[3 * NP + p] = (float)c3;
    sh_value[p] = value;
  }
  __syncthreads();
  if (p == 0) {
    double s = 0.0;
    for (int i = 0; i < NP; i++) s += sh_value[i];
    s *= scale;
    *loss = accumulate ? *loss + s : s;
  }
}

// 3. The gradient: the same walk; per chunk the labels once, then the planes in groups of MN_PL_G, each logit loaded
// once and each gradient element stored once.  BOTH: the (s - y) part is wanted (some c2 or c3 is not zero).
template <int DT, int P, bool BOTH>
__device__ __forceinline__ void mn_plane_grad_walk(const MnPlaneArgs& A, float f, int lane, RowSpan span) {
  const int W = A.W, NP = A.NP;
  const size_t N = (size_t)A.H * (size_t)W;
  const bool wide = A.wide != 0, comp = A.comp != 0, cls = A.part == MN_PART_CLASS;
  for (long long c = span.c0; c < span.c1; c++) {
    int x, y;
    row_walk_pixel(A.walk, P, c, lane, &x, &y);
    if (x >= W) continue;
    const size_t at = (size_t)y * W + (size_t)x;
    int t[P], tc[P];
    mn_walk_labels<P, false>(A.truth + at, t);
    if (cls) mn_plane_classes<P>(A, t, tc);
    for (int g0 = 0; g0 < NP; g0 += MN_PL_G) {
      float v[MN_PL_G][P];
#pragma unroll
      for (int g = 0; g < MN_PL_G; g++)
        if (g0 + g < NP) mn_plane_load<DT, false, P>(A.maps, (size_t)(g0 + g) * N + at, wide, v[g]);
#pragma unroll
      for (int g = 0; g < MN_PL_G; g++) {
        const int pl = g0 + g;
        if (pl >= NP) continue;
        const float c0 = A.coeffs[pl], c1 = A.coeffs[NP + pl];
        const float c2 = BOTH ? A.coeffs[2 * NP + pl] : 0.0f, c3 = BOTH ? A.coeffs[3 * NP + pl] : 0.0f;
        bool yes[P], keep[P];
        mn_plane_targets<P>(A, pl, x, y, t, tc, yes, keep);
        float gr[P];
#pragma unroll
        for (int j = 0; j < P; j++) {
          const float xv = v[g][j];
          const bool z = yes[j] != comp;
          const float q = mn_sigmoid(comp ? -xv : xv);
          float e = q * (1.0f - q) * (z ? c0 : c1);
          if (BOTH) {
            float s = q;
            if (comp) s = mn_sigmoid(xv);
            e += (s - (yes[j] ? 1.0f : 0.0f)) * (yes[j] ? c2 : c3);
          }
          gr[j] = keep[j] ? f * e : 0.0f;
        }
        mn_plane_store<DT, P>(A.grad, (size_t)pl * N + at, wide, gr);
      }
    }
  }
}

template <int DT, int P>
__global__ __launch_bounds__(MN_PL_THREADS) void mn_plane_grad_pass(const MnPlaneArgs A) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const RowSpan span = row_walk_span(A.walk, (long long)blockIdx.x * MN_PL_WAVES + wv);
  // whether any plane has a c2 or c3 that is not zero: lane l looks at planes l and l + 64, the wave votes -- uniform
  bool some = false;
  for (int p = lane; p < A.NP; p += 64) some = some || A.coeffs[2 * A.NP + p] != 0.0f || A.coeffs[3 * A.NP + p] != 0.0f;
  const bool both = __ballot(some) != 0;
  const float f = A.factor ? *A.factor : 1.0f;
  if (both) mn_plane_grad_walk<DT, P, true>(A, f, lane, span);
  else mn_plane_grad_walk<DT, P, false>(A, f, lane, span);
}
