// mn_row_walk.h -- the one walk of the passes that stream a label mask (and the maps beside it) row by row:
// mn_instance_table_runs, mn_overlap_table_runs, mn_map_scores_pass, mn_mask_bce_pass, mn_plane_sums_pass and
// mn_plane_grad_pass (what the last four share beyond the walk -- their grid, the truth reads, the sums -- is
// mn_truth_pass.h).  The host part is plain C++ that g++ alone
// compiles (tests/tools/row_walk_check.cpp, tests/test_row_walk.py).
// A chunk is 64 * V consecutive pixels of ONE row; lane l of the wave holds pixels V*l .. V*l + V-1 of it.  The image
// is total_chunks = H * chunks_per_row (<= H * W) chunks, numbered row by row; wave w of the grid takes the
// chunks_per_wave chunks from w * chunks_per_wave, both ends of that span clamped to total_chunks (a wave past the
// image has an empty span).  The last chunk of a row may reach past W.  V > 1 only where W % V == 0 (row_walk_v), and
// a lane's first column x is a multiple of V, so a lane is wholly inside the row (x + V <= W) or wholly past it:
// `x < W` is the whole bound test of a lane's V pixels; what a lane past W holds instead is the pass's own choice.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__HIP__)
#include "mn_device.h"
#define MN_WALK_HD __host__ __device__ __forceinline__
#else
#define MN_WALK_HD static inline
#endif
// (a kernel argument, what the kernels read first.)  blocks: workgroups of waves_per_block waves; v: the kernel's V
struct RowWalk { int chunks_per_row, total_chunks, chunks_per_wave, blocks, v; };
// V: the widest load, 16 bytes per lane (4 labels or float32 values, 8 16-bit values), where the width is a multiple
// of it and every base loaded that way (one or two: a, b) is 16-byte aligned; 16-bit maps else take 4 (8-byte loads)
// where W % 4 == 0 and the bases are 8-byte aligned; else single elements, any W and any base.
static inline int row_walk_v(int W, int elem_size, const void* a, const void* b = nullptr) {
  const uintptr_t bases = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b);
  const int widest = 16 / elem_size;
  if (W % widest == 0 && (bases & 15) == 0) return widest;
  return (elem_size == 2 && W % 4 == 0 && (bases & 7) == 0) ? 4 : 1;
}

// The grid is given (the map scores: their partial sums must group the same way whatever V is).
static inline RowWalk row_walk_fixed(int H, int W, int v, int blocks, int waves_per_block) {
  const int per_row = (W + 64 * v - 1) / (64 * v), total = H * per_row, waves = blocks * waves_per_block;
  return RowWalk{per_row, total, (total + waves - 1) / waves, blocks, v};
}
// The grid is aimed at `aim_blocks` workgroups (the tables): that gives a wave's share; no more blocks than shares.
static inline RowWalk row_walk_aimed(int H, int W, int v, int aim_blocks, int waves_per_block) {
  RowWalk R = row_walk_fixed(H, W, v, aim_blocks, waves_per_block);
  R.blocks = (R.total_chunks + waves_per_block * R.chunks_per_wave - 1) / (waves_per_block * R.chunks_per_wave);
  return R;
}
struct RowSpan { long long c0, c1; };             // the chunks c0 <= c < c1 of one wave
MN_WALK_HD long long row_walk_min(long long a, long long b) { return a < b ? a : b; }
MN_WALK_HD RowSpan row_walk_span(const RowWalk& R, long long wave) {
  const long long c0 = row_walk_min(wave * (long long)R.chunks_per_wave, (long long)R.total_chunks);
  return RowSpan{c0, row_walk_min(c0 + (long long)R.chunks_per_wave, (long long)R.total_chunks)};
}
// Row y and first column x of the v pixels that `lane` holds of chunk c.
MN_WALK_HD void row_walk_pixel(const RowWalk& R, int v, long long c, int lane, int* x, int* y) {
  *y = (int)(c / R.chunks_per_row);
  *x = ((int)(c - (long long)*y * R.chunks_per_row) * 64 + lane) * v;
}
#if defined(__HIPCC__) || defined(__HIP__)
// V labels of one row from p: one int (V = 1), else V / 4 loads of four ints, ALIGNED to 16 bytes (V = 4) or not.
template <int V, bool ALIGNED>
__device__ __forceinline__ void mn_walk_labels(const int* __restrict__ p, int* a) {
  static_assert(V == 1 || V == 4 || (V == 8 && !ALIGNED), "whole loads of four ints, or one int");
  if constexpr (V == 1) a[0] = *p;
#pragma unroll
  for (int h = 0; h < V / 4; h++) {
    const int4 u = ALIGNED ? *reinterpret_cast<const int4*>(p + 4 * h) : mn_ld_int4_unaligned(p + 4 * h);
    a[4 * h] = u.x; a[4 * h + 1] = u.y; a[4 * h + 2] = u.z; a[4 * h + 3] = u.w;
  }
}

// The ends of the runs of one chunk.  head[j]: this lane's pixel j begins a run (the pass says what that means; the
// first pixel of a chunk must be one).  Positions count from this lane's FIRST pixel.  mn_walk_next_head, called by
// the whole wave together (one ballot per pixel slot): the first head of the first later lane that has one, else the
// chunk's end.  mn_walk_run_end, for a head j: one past its run's last pixel -- the next head in its own lane, else
// `next_head` -- so the run is that less j pixels long.
template <int V>
__device__ __forceinline__ int mn_walk_next_head(const bool* head, int lane) {
  u64 b[V], any = 0;
#pragma unroll
  for (int j = 0; j < V; j++) { b[j] = __ballot(head[j]); any |= b[j]; }
  const u64 later = any & ~((2ull << lane) - 1ull);       // (lane 63: 2 << 63 wraps to 0, the mask to all ones)
  int next_in_chunk = 64 * V;
  if (later) {
    const int ln = __ffsll((long long)later) - 1;
    int jn = V - 1;
#pragma unroll
    for (int j = V - 1; j >= 0; j--) if ((b[j] >> ln) & 1ull) jn = j;
    next_in_chunk = ln * V + jn;
  }
  return next_in_chunk - lane * V;
}
template <int V>
__device__ __forceinline__ int mn_walk_run_end(const bool* head, int j, int next_head) {
#pragma unroll
  for (int j2 = V - 1; j2 > j; j2--) if (head[j2]) next_head = j2;
  return next_head;
}
#endif
