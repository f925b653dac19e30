// mn_kernels_celoss.h -- the cross-entropy criterion from the label mask: the softmax over the planes of ONE part of
// the network's output against the pixel's target plane and, in the same pass, its gradient.  No target plane is
// written or read, no argmax plane either.
//
// Reference work replaced (training with --loss ce):
//   CrossEntropyLossOneHot                     utils/loss.py:24-35: F.cross_entropy(input, target.max(1)[1])
//   its selection for a part of the output     egs/cityscape/local/train.py:193-204 (the 10 offset planes),
//                                              egs/coco/local/train.py:145-154 (the 81 class planes)
//   the targets it is fed                      utils/dataset.py:259-277 (offsets), :419-429 (classes)
// Definitions (mergenet_hip.h gives them in full; labels.mask_ce is the numpy statement):
//   x            = the element widened exactly to float32; truth class and neighbour rule as in mn_kernels_loss.h;
//   target plane = class part: the pixel's truth class; outside 0..P-1 the pixel is an ignore class: term 0,
//                  gradient 0 on every plane (the store is made), not counted among the kept pixels;
//                  offset part: the least k whose offset target is 1 (the neighbour at (di_k, dj_k) is outside the
//                  image or carries the pixel's own label), plane 0 if there is none; every pixel is kept
//                  -- what target.max(1)[1] elects on the reference's one-hot planes, the first maximal plane;
//   the float32 arithmetic of a pixel, P planes x_0 .. x_{P-1}, each operation rounded (no fused multiply-add):
//     m    = max_q x_q                      a = the first q with x_q == m
//     e_q  = expf(x_q - m) for q != a       (e_a is 1: what the lane computed for it is not used)
//     r    = sum of e_q, q != a, ascending q
//     term = log1pf(r) + (m - x_target)     (both summands >= 0; the second is 0 exactly when x_target == m)
//     p_q  = e_q * (1 / (1 + r)), p_a = 1 / (1 + r);   g_q = (p_q - [q == target]) * scale
//   log1pf(r), not logf(1 + r): where the target is the maximum and the other planes lie far below, the term is
//   about r, and 1 + r would lose it.  One reciprocal per pixel and one product per element, not a division per
//   element: within the 2.5 ulp the bounds of tests/test_gpu_mask_ce.py allow for either.
//   gradient     = g_q rounded to nearest even into the element type;
//   sums         = float64 [2]: [0] the terms of the kept pixels, each widened before it is added, [1] their number.
// expf(x_q - m) underflows for x_q more than about 87 below the maximum: that e_q is below 2^-126 and counts as
// 0 or a subnormal, either inside the bounds.  NaN or infinity in a map is undefined, as in every other pass.
//
// Two forms, chosen on the host by the plane count P alone (mn_ce_bucket), so that a result never depends on where
// the buffers lie:
//   resident   P <= MN_CE_RESIDENT_MAX = 20 (the recipes' 9 class and 10 offset planes, the semantic network's
//              19): the lane loads all planes of its pixels at once -- every load of the chunk is in flight together
//              -- and keeps them in registers; max, sum, term and gradient follow with no second read and ONE expf
//              per element.  The plane loops are unrolled to a compile-time bound PB = 4, 10 or 20 (the smallest
//              that holds P; steps of planes beyond P are skipped by a branch that is uniform over the launch).
//              The lane keeps the pixels of the walk -- 8, 4 or 1, what a 16-byte access of a plane gives -- in
//              every bucket, 160 values at PB = 20 with 8 pixels: a quarter of the 512 VGPRs a lane can have, 2
//              waves per SIMD.  Halving the pixels there (two 8-byte accesses per plane) would give 4 waves, but
//              what hides the memory latency is the bytes in flight, and one wave of that form has 20 KiB of loads
//              outstanding; the walk and the grid stay those of every other truth pass.
//   streaming  the rest, up to MN_MAX_CLASSES = 127 planes (COCO's 81): three sweeps over the planes of the chunk,
//              MN_CE_CG planes' loads in flight together -- 1. the maximum, its first plane and x_target, 2. the
//              sum r, 3. (with a gradient only) the gradient, which takes expf a second time.  Sweeps 2 and 3 read
//              again what sweep 1 read a moment ago: 64 * pixels * P elements per wave, 41 KiB at 81 planes of 8
//              bfloat16 pixels, 83 KiB of 4 float32 pixels.
//              Measured at 1024x2048 with 81 planes (profiles/mask_ce_time.log): the second sweep costs about 5 % of
//              the rate the resident form reaches, the third with its expf a third of the float32 call; the repeats
//              are served by the caches (by size mostly the Infinity Cache, not the 4 MiB L2; no counters taken).
// Same arithmetic in both forms, in the same order.
//
// Resource report of the compiler for gfx950 (-Rpass-analysis=kernel-resource-usage): no scratch and no spilled
// VGPR in any of the 32 instantiations (float32 has no 8-pixel form: a 16-byte access is four of its elements).
//   VGPRs (waves per SIMD)         float32      float16      bfloat16
//   resident, PB = 4    8 px          --        135 (3)      138 (3)
//                       4 px        79 (6)       79 (6)       82 (5)
//                       1 px        40 (8)       40 (8)       42 (8)
//   resident, PB = 10   8 px          --        158 (3)      163 (3)
//                       4 px        91 (5)       92 (5)       95 (5)
//                       1 px        47 (7)       47 (7)       49 (7)
//   resident, PB = 20   8 px          --        239 (2)      244 (2)
//                       4 px       132 (3)      133 (3)      136 (3)
//                       1 px        57 (7)       57 (7)       60 (7)
//   streaming           8 px          --        158 (3)      176 (2)
//                       4 px       102 (4)       91 (5)      106 (4)
//                       1 px        46 (8)       46 (8)       46 (8)
// 64 bytes of LDS.  The unrolled forms keep the planes' base addresses in scalar registers: the PB = 10 and PB = 20
// forms move up to 31 and 102 of them into lanes of a vector register and back (SGPR spills; no memory is involved).
#pragma once

#include "mn_device.h"
#include "mn_row_walk.h"
#include "mn_truth_pass.h"        // the grid, the truth reads, the sums: shared with the other passes over a truth mask

#define MN_CE_THREADS 256
#define MN_CE_WAVES (MN_CE_THREADS / 64)
#define MN_CE_VALUES 2            /* the sum of the terms, the kept pixels */
#define MN_CE_CG 4                /* streaming form: planes whose loads are in flight together */
#define MN_CE_RESIDENT_MAX 20     /* the resident form's largest bucket */
static_assert(MN_CE_VALUES <= MN_MS_VALUES, "the pass shares the partials buffer of mn_map_scores_device");

// The bound of the resident form's plane loops for P planes; 0: the streaming form.
static inline int mn_ce_bucket(int P) { return P <= 4 ? 4 : P <= 10 ? 10 : P <= MN_CE_RESIDENT_MAX ? MN_CE_RESIDENT_MAX : 0; }

// The waves per SIMD the register allocator is held to (left alone it takes up to 256 VGPRs in every form with 8
// pixels): 2 where a lane keeps 160 values and in the streaming form with 8 pixels (three unrolled sweeps; at 3 the
// bfloat16 one spills), 3 in the other forms with 8 pixels or 80 values, else 4 -- the most that spills nothing.
constexpr int mn_ce_waves(int P, int PB) {
  return (P * PB >= 160 || (P == 8 && PB == 0)) ? 2 : (P == 8 || P * PB >= 80) ? 3 : 4;
}

struct MnMaskCeArgs {
  const void* maps;               // [NP][N] logits
  void* grad;                     // [NP][N] gradient, the maps' element type, or null
  const int* truth;               // [N] label mask
  const int* truth_classes;       // [G] (may be null when G == 0; the class part only)
  int H, W, NP, G;
  int part;                       // MN_PART_CLASS or MN_PART_OFFSET
  int wide;                       // the map and gradient bases admit the wide access of the walk's P pixels
  float scale;
  RowWalk walk;                   // walk.blocks: the grid, and the slots of the partials buffer; walk.v: P
  double* partials;               // [2][walk.blocks]
  int di[MN_MAX_OFFSETS];
  int dj[MN_MAX_OFFSETS];
};

// One plane's step of the first sweep for a lane's P pixels: the running maximum, its first plane, x_target.
template <int P>
__device__ __forceinline__ void mn_ce_max(int q, const float* v, const int* tgt, float* m, int* a, float* xt) {
#pragma unroll
  for (int j = 0; j < P; j++) {
    if (v[j] > m[j]) { m[j] = v[j]; a[j] = q; }        // (strictly greater: the FIRST maximal plane stays)
    xt[j] = tgt[j] == q ? v[j] : xt[j];
  }
}
// ... of the second: e_q, left in v, and the sum without plane a.
template <int P>
__device__ __forceinline__ void mn_ce_sum(int q, float* v, const float* m, const int* a, float* r) {
#pragma unroll
  for (int j = 0; j < P; j++) {
    v[j] = expf(v[j] - m[j]);
    r[j] += a[j] == q ? 0.0f : v[j];                   // (r + 0 is r: plane a adds nothing)
  }
}
// ... of the third: the gradient from e_q in v and inv = 1 / (1 + r), left in v.
template <int P>
__device__ __forceinline__ void mn_ce_grad(int q, float* v, const int* tgt, const int* a, const float* inv, float scale) {
#pragma unroll
  for (int j = 0; j < P; j++) {
    const float p = (a[j] == q ? 1.0f : v[j]) * inv[j];
    v[j] = tgt[j] >= 0 ? (p - (tgt[j] == q ? 1.0f : 0.0f)) * scale : 0.0f;
  }
}

// The walk of mn_mask_bce_pass: P pixels per lane by the element size and the WIDTH alone, the grid by (H, W, element
// size) alone, and the form by the plane count alone, so which pixels a lane holds, the arithmetic of each and the
// grouping of the float64 sum do not depend on where the caller's buffers lie: bases that do not admit the wide
// access (A.wide == 0) change the loads and stores to single elements, not the walk.  The sums of an image are
// therefore the same bits whatever the alignment of the map and the gradient, and whether or not a gradient is
// written.  Every gradient element is stored once; a lane past W loads and stores nothing.  The truth mask is read
// through the cache.  The wave adds its lanes' sums with the fixed butterfly, the workgroup writes both values to its
// slot of the partials buffer (no clearing needed), mn_map_scores_finish adds the slots in a fixed order.  No
// floating-point atomic anywhere.
template <int DT, int P, int PB>
__global__ __launch_bounds__(MN_CE_THREADS, mn_ce_waves(P, PB)) void mn_mask_ce_pass(const MnMaskCeArgs A) {
  __shared__ double sh_part[MN_CE_WAVES][MN_CE_VALUES];
  const int H = A.H, W = A.W, NP = A.NP;
  const size_t N = (size_t)H * (size_t)W;
  const bool wide = A.wide != 0, want = A.grad != nullptr;
  const float scale = A.scale;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const RowSpan span = row_walk_span(A.walk, (long long)blockIdx.x * MN_CE_WAVES + wv);
  double s = 0.0;
  int kept = 0;

  for (long long c = span.c0; c < span.c1; c++) {
    int x, y;
    row_walk_pixel(A.walk, P, c, lane, &x, &y);
    if (x >= W) continue;                              // (no shuffle or barrier inside this loop)
    const size_t at = (size_t)y * W + (size_t)x;
    [[maybe_unused]] float xs[PB > 0 ? PB : 1][P];     // resident form: every plane of the lane's pixels
    if constexpr (PB > 0) {
#pragma unroll
      for (int q = 0; q < PB; q++)
        if (q < NP) mn_plane_load<DT, false, P>(A.maps, (size_t)q * N + at, wide, xs[q]);
    }

    // ---- the target plane of each pixel; -1: an ignored pixel ----
    int t[P], tgt[P];
    mn_walk_labels<P, false>(A.truth + at, t);
    if (A.part == MN_PART_CLASS) {
#pragma unroll
      for (int j = 0; j < P; j++) tgt[j] = mn_kept_class(t[j], A.truth_classes, A.G, NP);
    } else {
#pragma unroll
      for (int j = 0; j < P; j++) tgt[j] = 0;
      for (int k = NP - 1; k >= 0; k--) {              // descending: the least k with target 1 is written last
        const unsigned yy = (unsigned)y + (unsigned)A.di[k], xx = (unsigned)x + (unsigned)A.dj[k];
        int nb[P];
#pragma unroll
        for (int j = 0; j < P; j++) nb[j] = t[j];      // (the neighbour rule of mn_truth_pass.h)
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
        for (int j = 0; j < P; j++) tgt[j] = nb[j] == t[j] ? k : tgt[j];
      }
    }

    float m[P], xt[P], r[P];
    int a[P];
#pragma unroll
    for (int j = 0; j < P; j++) { m[j] = -INFINITY; a[j] = 0; xt[j] = 0.0f; r[j] = 0.0f; }

    if constexpr (PB > 0) {
      // ---- resident: no second read, one expf per element ----
#pragma unroll
      for (int q = 0; q < PB; q++)
        if (q < NP) mn_ce_max<P>(q, xs[q], tgt, m, a, xt);
#pragma unroll
      for (int q = 0; q < PB; q++)
        if (q < NP) mn_ce_sum<P>(q, xs[q], m, a, r);
      if (want) {
        float inv[P];
#pragma unroll
        for (int j = 0; j < P; j++) inv[j] = 1.0f / (1.0f + r[j]);
#pragma unroll
        for (int q = 0; q < PB; q++) {
          if (q >= NP) continue;
          mn_ce_grad<P>(q, xs[q], tgt, a, inv, scale);
          mn_plane_store<DT, P>(A.grad, (size_t)q * N + at, wide, xs[q]);
        }
      }
    } else {
      // ---- streaming: the planes of the chunk three times, the second and third time through the cache ----
      for (int q0 = 0; q0 < NP; q0 += MN_CE_CG) {
        float v[MN_CE_CG][P];
#pragma unroll
        for (int q = 0; q < MN_CE_CG; q++)
          if (q0 + q < NP) mn_plane_load<DT, false, P>(A.maps, (size_t)(q0 + q) * N + at, wide, v[q]);
#pragma unroll
        for (int q = 0; q < MN_CE_CG; q++)
          if (q0 + q < NP) mn_ce_max<P>(q0 + q, v[q], tgt, m, a, xt);
      }
      for (int q0 = 0; q0 < NP; q0 += MN_CE_CG) {
        float v[MN_CE_CG][P];
#pragma unroll
        for (int q = 0; q < MN_CE_CG; q++)
          if (q0 + q < NP) mn_plane_load<DT, false, P>(A.maps, (size_t)(q0 + q) * N + at, wide, v[q]);
#pragma unroll
        for (int q = 0; q < MN_CE_CG; q++)
          if (q0 + q < NP) mn_ce_sum<P>(q0 + q, v[q], m, a, r);
      }
      if (want) {
        float inv[P];
#pragma unroll
        for (int j = 0; j < P; j++) inv[j] = 1.0f / (1.0f + r[j]);
        for (int q0 = 0; q0 < NP; q0 += MN_CE_CG) {
          float v[MN_CE_CG][P];
#pragma unroll
          for (int q = 0; q < MN_CE_CG; q++)
            if (q0 + q < NP) mn_plane_load<DT, false, P>(A.maps, (size_t)(q0 + q) * N + at, wide, v[q]);
#pragma unroll
          for (int q = 0; q < MN_CE_CG; q++) {
            if (q0 + q >= NP) continue;
            float unused[P];
#pragma unroll
            for (int j = 0; j < P; j++) unused[j] = 0.0f;
            mn_ce_sum<P>(q0 + q, v[q], m, a, unused);  // (e_q once more: the same value as in the second sweep)
            mn_ce_grad<P>(q0 + q, v[q], tgt, a, inv, scale);
            mn_plane_store<DT, P>(A.grad, (size_t)(q0 + q) * N + at, wide, v[q]);
          }
        }
      }
    }

#pragma unroll
    for (int j = 0; j < P; j++) {
      const bool keep = tgt[j] >= 0;
      const double term = (double)(log1pf(r[j]) + (m[j] - xt[j]));
      s += keep ? term : 0.0;
      kept += keep ? 1 : 0;
    }
  }

  long long n = kept;
  mn_wave_sums(s, n);
  if (lane == 0) {
    sh_part[wv][0] = s;
    sh_part[wv][1] = (double)n;                        // (an integer below 2^53: exact)
  }
  mn_truth_flush<MN_CE_WAVES>(sh_part, MN_CE_VALUES, A.partials, A.walk.blocks);
}
