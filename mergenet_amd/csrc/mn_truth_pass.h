// mn_truth_pass.h -- what the passes over the network's maps and a truth label mask share: mn_map_scores_pass
// (mn_kernels_mapscore.h), mn_mask_bce_pass (mn_kernels_loss.h) and mn_plane_sums_pass / mn_plane_grad_pass
// (mn_kernels_planeloss.h).  They walk the image by mn_row_walk.h, read a pixel's truth label and its neighbours'
// under ONE rule, keep float64 sums per lane, add them up in a fixed order into the workgroup's slot of a partials
// buffer (one for the first two, one of its own for the plane sums), and leave the slots to mn_map_scores_finish
// (the gradient pass of the plane losses keeps no sums).  The host part -- the
// grid and the clamp of the offsets -- is plain C++ that g++ alone compiles (tests/tools/row_walk_check.cpp,
// tests/test_row_walk.py).
#pragma once
#include "mn_row_walk.h"

#ifndef MN_MS_WORKGROUPS
#define MN_MS_WORKGROUPS 1024     /* most workgroups of a pass = most slots of the partials buffer (4 per CU) */
#endif
#ifndef MN_MS_MIN_CHUNKS
#define MN_MS_MIN_CHUNKS 2        /* a wave takes at least this many chunks before the grid grows */
#endif

// The grid of a pass, and the slots of the partials buffer it fills: a function of (H, W, element size) alone.  It is
// sized for the widest loads of the element type (16 bytes per lane); fewer pixels per lane mean more chunks per wave,
// not another grid, so the partial sums group the same way whatever the bases allow.
static inline int truth_pass_slots(int H, int W, int elem_size, int waves_per_block) {
  const int widest = 16 / elem_size;
  const long long nominal = (long long)H * ((W + 64 * widest - 1) / (64 * widest));
  const long long per_block = (long long)waves_per_block * MN_MS_MIN_CHUNKS;
  const long long want = (nominal + per_block - 1) / per_block;
  return (int)(want < MN_MS_WORKGROUPS ? want : MN_MS_WORKGROUPS);
}
// The O offsets of the caller's list, (di, dj) pairs, as the kernels take them: an offset of H rows or W columns or
// more leaves the image whatever its size, so each is held to -H..H / -W..W -- row + di and column + dj stay ints.
static inline void truth_pass_offsets(const int* offset_list, int O, int H, int W, int* di, int* dj) {
  for (int k = 0; k < O; k++) {
    const int a = offset_list[2 * k], b = offset_list[2 * k + 1];
    di[k] = a < -H ? -H : (a > H ? H : a);
    dj[k] = b < -W ? -W : (b > W ? W : b);
  }
}

#if defined(__HIPCC__) || defined(__HIP__)
#include "mn_kernels_cc.h"        // the streaming typed loaders and stores (mn_ld_stream*_t, mn_st_stream_t)

// The partials buffer, [values][MN_MS_WORKGROUPS] doubles, is the context's and serves both passes.
#define MN_MS_VALUES (3 * MN_MAX_OFFSETS)      /* map scores: three sums per offset */
#define MN_BCE_VALUES (2 + MN_MAX_OFFSETS)     /* BCE: the class sum, one sum per offset, the kept pixels */
static_assert(MN_BCE_VALUES <= MN_MS_VALUES, "the BCE pass shares the partials buffer of mn_map_scores_device");

// The truth class of label t: 0 for label 0 and any label outside 1..G, truth_classes[t - 1] else.
__device__ __forceinline__ int mn_truth_class(int t, const int* truth_classes, int G) {
  // the label is held to 1..G BEFORE it forms an address: the mask is the caller's memory
  return ((unsigned)t - 1u < (unsigned)G) ? truth_classes[(unsigned)t - 1u] : 0;
}
// ... and -1 where that is outside 0..C-1: left out of the confusion matrix, the ignore class of the criterion.
__device__ __forceinline__ int mn_kept_class(int t, const int* truth_classes, int G, int C) {
  const int cl = mn_truth_class(t, truth_classes, G);
  return ((unsigned)cl < (unsigned)C) ? cl : -1;
}

// The neighbour labels of a lane, nb[j] = the truth label at (y + di, x + dj + j) for j < V -- the rule of both passes:
//   * the own label t[j] where the neighbour is outside the image ("same");
//   * reads stay inside the neighbour's ROW of the mask: the 16-byte form only where all V columns are inside 0..W-1,
//     single reads under a column test otherwise; a row outside the image is not read at all;
//   * row + di and column + dj are taken in unsigned arithmetic: |di| <= H and |dj| <= W (truth_pass_offsets holds
//     them to that), so a sum below 0 wraps to 2^31 or more and fails the same test as one past the edge.
// The dozen lines that do this stand in each kernel, not here: as a function the compiler arranges them otherwise
// (the first column's load is shared between the two forms, the rest becomes a 12-byte load), and both passes were
// measurably slower for it at 1024x2048 (profiles/truth_pass_time.log).

// A lane's V consecutive elements of one plane, from element i.  wide: one access -- V = 8 16 bytes of 16-bit values,
// V = 4 16 bytes (float32) or 8 bytes; else -- a base off that boundary, uniform over the launch -- V single
// elements.  V = 1 is the single element either way.
template <int DT, bool LG, int V>
__device__ __forceinline__ void mn_plane_load(const void* base, size_t i, bool wide, float* v) {
  if (V == 1 || wide) {
    if constexpr (V == 8) {
      mn_ld_stream8_t<DT, LG>(base, i, v);
    } else if constexpr (V == 4) {
      const float4 t = mn_ld_stream4_t<DT, LG>(base, i);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      v[0] = mn_ld_stream1_t<DT, LG>(base, i);
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; j++) v[j] = mn_ld_stream1_t<DT, LG>(base, i + j);
  }
}
template <int DT, int V>
__device__ __forceinline__ void mn_plane_store(void* base, size_t i, bool wide, const float* g) {
  if (V == 1 || wide) {
    mn_st_stream_t<DT, V>(base, i, g);
  } else {
#pragma unroll
    for (int j = 0; j < V; j++) mn_st_stream_t<DT, 1>(base, i + j, g + j);
  }
}

// The wave's sums of the lanes' values (double or long long), each left in every lane, by a fixed butterfly of
// shuffles: the same grouping on every run.  Several values go through the one loop step by step together.
template <typename... T>
__device__ __forceinline__ void mn_wave_sums(T&... v) {
  for (int s = 32; s > 0; s >>= 1) ((v += __shfl_xor(v, s)), ...);
}

// The workgroup's flush, called by all its WAVES * 64 threads once lane 0 of every wave has written its wave's n
// values to sh_part[wave]: value i of the workgroup, the waves added in ascending order, goes to its slot of the
// partials buffer.  Every workgroup writes all n values, so the buffer needs no clearing.
template <int WAVES, int VALUES>
__device__ __forceinline__ void mn_truth_flush(const double (*sh_part)[VALUES], int n, double* partials, int blocks) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += WAVES * 64) {
    double s = sh_part[0][i];
#pragma unroll
    for (int q = 1; q < WAVES; q++) s += sh_part[q][i];
    partials[(size_t)i * blocks + blockIdx.x] = s;
  }
}

// One wave per value: lane l adds the slots l*per .. l*per + per-1 in ascending order, the lanes' sums meet in the
// fixed butterfly.  The image's total is then stored, or -- accumulate -- added to what the caller's buffer holds in
// ONE IEEE addition: the running total of a validation or training loop.
__global__ __launch_bounds__(64) void mn_map_scores_finish(const double* __restrict__ partials, int slots,
                                                            double* __restrict__ sums, int accumulate) {
  const int lane = threadIdx.x;
  const int per = (slots + 63) / 64;
  const double* p = partials + (size_t)blockIdx.x * slots;
  double s = 0.0;
  for (int i = lane * per; i < min(slots, (lane + 1) * per); i++) s += p[i];
  mn_wave_sums(s);
  if (lane == 0) sums[blockIdx.x] = accumulate ? sums[blockIdx.x] + s : s;
}
#endif
