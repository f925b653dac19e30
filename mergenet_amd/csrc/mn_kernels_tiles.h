// mn_kernels_tiles.h -- class maps from a tiled semantic network, assembled on the device.
//
// Reference work replaced: tile_predict (models/pspnet_caffe.py:492-560, switched on in
// egs/cityscape/local/class_infer.py:58-64), the producer of the production recipe's CLASS maps.  It runs a Cn-class
// semantic network on overlapping tiles, each plain and horizontally flipped, and does the rest in numpy on the host,
// with a .cpu() and a .cuda() per tile: softmax over the Cn classes, the two passes averaged, the "stuff" classes
// folded into one background plane by a maximum, the tiles summed into the image, the sum divided by a per-pixel
// cover count and renormalised over the C planes kept.
//
// Here ONE gather kernel does it: a lane owns one image pixel, finds the tiles that cover it, reads their logits once
// and writes the pixel's C values.  Nothing is scattered, so there is no atomic, no count plane and no second launch.
//   per tile pixel   p1 = softmax(logits over Cn) as expf(x - max) / sum, sum in ascending class
//                    with a flip tensor: p2 the same at tile column tw - 1 - x, p = (p1 + p2) * 0.5f; else p = p1
//                    q[0] = max of p over the first Cn - C + 1 classes (AFTER the average), q[k] = p[Cn - C + k]
//   per image pixel  acc[k] = sum of q[k] over the covering tiles in ascending tile index, s[k] = acc[k] / count,
//                    out[k] = s[k] / (s[0] + ... + s[C-1]) summed in ascending k, then the merger's clip if asked
// all in float32.
//
// Registers, not scratch: a private array stays in VGPRs only while every index into it is a compile-time constant, so
// the class loops are unrolled to a compile-time bound CNB >= Cn (8, 20, 32 or 64: the host picks the smallest) and the
// classes beyond Cn are carried along as probabilities of exactly 0.  The accumulators are indexed by NETWORK class
// for the same reason (output plane k = class - (Cn - C) is then only an address).  A tile's logits are loaded once
// into x[CNB] (and once more for the flipped line), turned into exponentials in place, and leave as probabilities: one
// expf per logit.  76 VGPRs at CNB = 20 (6 waves per SIMD), 235 at CNB = 64 (2 waves), no scratch in any form.
//
// Loads: a wave takes 64 consecutive columns of one image row, so for one tile and class it reads one run of
// consecutive elements (the flipped line: the same run reversed).  Tile starts are arbitrary, so the run's alignment
// differs per tile; one element per lane.  Lanes of a wave may lie in different column tiles: the loop over column
// tiles is divergent there and nowhere else (the row is uniform over the workgroup).
#pragma once

#include "mn_device.h"
#include "mn_kernels_prepare.h"

#define MN_TILES_MAX_STARTS 32    /* per axis: the starts travel as kernel arguments */
#define MN_TILES_MAX_CLASSES 64   /* network classes */
#define MN_TILES_THREADS 256

struct MnTileArgs {
  const void* tiles;   // [nr * nc][Cn][th][tw]
  const void* flip;    // the same shape, or NULL
  void* out;           // [C][H][W]
  int Cn, C, th, tw, nr, nc, H, W;
  int blocks_per_row;  // workgroups of MN_TILES_THREADS columns per image row
  int out_dtype, clip;
  int rs[MN_TILES_MAX_STARTS];
  int cs[MN_TILES_MAX_STARTS];
};

template <int DT>
__device__ __forceinline__ float mn_tile_ld(const void* base, size_t i) {
  if constexpr (DT == MN_DTYPE_F32) return static_cast<const float*>(base)[i];
  else return mn_widen<DT>(static_cast<const mn_u16*>(base)[i]);
}

// softmax over the Cn classes of one tile pixel: the elements at + c * plane go in, p[c] comes out.  No branch: a
// test per class, uniform or not, would put every load into a block of its own behind a wait for the one before
// (in the assembly of that form: 40 loads, 40 waits for all loads), so all CNB loads are issued together -- the classes beyond Cn re-read class Cn - 1
// and then count as -inf: they leave the maximum alone, their exponential is exactly 0 and adds nothing to the sum.
template <int DT, int CNB>
__device__ __forceinline__ void mn_tile_softmax(const void* base, size_t at, size_t plane, int Cn, float (&x)[CNB]) {
#pragma unroll
  for (int c = 0; c < CNB; c++) x[c] = mn_tile_ld<DT>(base, at + (size_t)min(c, Cn - 1) * plane);
  float m = x[0];
#pragma unroll
  for (int c = 1; c < CNB; c++) {
    x[c] = c < Cn ? x[c] : -INFINITY;
    m = fmaxf(m, x[c]);
  }
  float sum = 0.0f;
#pragma unroll
  for (int c = 0; c < CNB; c++) { x[c] = expf(x[c] - m); sum += x[c]; }
#pragma unroll
  for (int c = 0; c < CNB; c++) x[c] = x[c] / sum;
}

template <int DT, int CNB>
__global__ __launch_bounds__(MN_TILES_THREADS) void mn_tile_class_maps(MnTileArgs A) {
  const int y = (int)(blockIdx.x / (unsigned)A.blocks_per_row);
  const int x = (int)(blockIdx.x - (unsigned)y * (unsigned)A.blocks_per_row) * MN_TILES_THREADS + (int)threadIdx.x;
  if (x >= A.W) return;
  const int Cn = A.Cn, nstuff = A.Cn - A.C + 1;
  const size_t plane = (size_t)A.th * (size_t)A.tw;
  const bool flipped = A.flip != nullptr;

  unsigned cover = 0;   // bit j: column tile j holds this lane's column
  for (int j = 0; j < A.nc; j++) cover |= (unsigned)(x >= A.cs[j] && x - A.cs[j] < A.tw) << j;

  float acc[CNB];       // by network class; the entries of the stuff classes stay unused
#pragma unroll
  for (int c = 0; c < CNB; c++) acc[c] = 0.0f;
  float acc0 = 0.0f;
  int count = 0;
  for (int i = 0; i < A.nr; i++) {
    const int ty = y - A.rs[i];
    if (ty < 0 || ty >= A.th) continue;                     // uniform over the workgroup
    for (int j = 0; j < A.nc; j++) {
      if (!((cover >> j) & 1u)) continue;
      const int tx = x - A.cs[j];
      const size_t row = (size_t)(i * A.nc + j) * (size_t)Cn * plane + (size_t)ty * (size_t)A.tw;
      float p[CNB];
      mn_tile_softmax<DT, CNB>(A.tiles, row + (size_t)tx, plane, Cn, p);
      if (flipped) {
        float p2[CNB];
        mn_tile_softmax<DT, CNB>(A.flip, row + (size_t)(A.tw - 1 - tx), plane, Cn, p2);
#pragma unroll
        for (int c = 0; c < CNB; c++) p[c] = (p[c] + p2[c]) * 0.5f;
      }
      // selects, not branches: p[c] is 0 from Cn on, and adding 0 leaves a sum of probabilities as it is
      float q0 = p[0];
#pragma unroll
      for (int c = 1; c < CNB; c++) {
        q0 = c < nstuff ? fmaxf(q0, p[c]) : q0;
        acc[c] += c >= nstuff ? p[c] : 0.0f;
      }
      acc0 += q0;
      count++;
    }
  }

  const float n = (float)count;                              // >= 1: the host refuses an uncovered row or column
  acc0 = acc0 / n;
  float total = acc0;
#pragma unroll
  for (int c = 1; c < CNB; c++)
    if (c >= nstuff && c < Cn) { acc[c] = acc[c] / n; total += acc[c]; }

  const size_t N = (size_t)A.H * (size_t)A.W;
  const size_t at = (size_t)y * (size_t)A.W + (size_t)x;
  const int shift = Cn - A.C;                                // output plane of network class c >= nstuff: c - shift
#pragma unroll
  for (int c = 0; c < CNB; c++) {
    if (c != 0 && !(c >= nstuff && c < Cn)) continue;
    float v = (c == 0 ? acc0 : acc[c]) / total;
    if (A.clip) v = mn_clip(v);
    const size_t o = (size_t)(c == 0 ? 0 : c - shift) * N + at;
    if (A.out_dtype == MN_DTYPE_F32) static_cast<float*>(A.out)[o] = v;
    else static_cast<mn_u16*>(A.out)[o] = A.out_dtype == MN_DTYPE_F16 ? mn_narrow_f16(v) : mn_narrow_bf16(v);
  }
}
