// Host shim of mn_row_walk.h for tests/test_row_walk.py: the header the mask passes are launched and walked by,
// compiled by g++ alone.
#include <stddef.h>

#include "../../mergenet_amd/csrc/mn_row_walk.h"

extern "C" int row_walk_v_check(int W, int elem_size, unsigned long long bases) {
  return row_walk_v(W, elem_size, reinterpret_cast<const void*>((uintptr_t)bases));
}

// fixed != 0: `blocks` is the grid; else it is the number of workgroups aimed at.
// out[5]: v, chunks_per_row, total_chunks, chunks_per_wave, blocks.
extern "C" void row_walk_check(int H, int W, int v, int fixed, int blocks, int waves_per_block, int* out) {
  const RowWalk R = fixed ? row_walk_fixed(H, W, v, blocks, waves_per_block)
                          : row_walk_aimed(H, W, v, blocks, waves_per_block);
  out[0] = R.v; out[1] = R.chunks_per_row; out[2] = R.total_chunks; out[3] = R.chunks_per_wave; out[4] = R.blocks;
}

// r[5]: the same five values, as a RowWalk.
static RowWalk walk_of(const int* r) {
  RowWalk R;
  R.v = r[0]; R.chunks_per_row = r[1]; R.total_chunks = r[2]; R.chunks_per_wave = r[3]; R.blocks = r[4];
  return R;
}

extern "C" void row_walk_span_check(const int* r, long long wave, long long* out) {
  const RowWalk R = walk_of(r);
  const RowSpan s = row_walk_span(R, wave);
  out[0] = s.c0; out[1] = s.c1;
}

// Every wave of the grid walks its span as a kernel does: visits[y * W + x] counts the visits of each pixel of the
// H x W image.  Returns the number of lanes that break the walk's promise: x < W yet x + v > W, or a row outside
// the image.
extern "C" long long row_walk_cover(int H, int W, const int* r, int waves_per_block, int* visits) {
  const RowWalk R = walk_of(r);
  long long broken = 0;
  for (long long wave = 0; wave < (long long)R.blocks * waves_per_block; wave++) {
    const RowSpan s = row_walk_span(R, wave);
    for (long long c = s.c0; c < s.c1; c++)
      for (int lane = 0; lane < 64; lane++) {
        int x, y;
        row_walk_pixel(R, R.v, c, lane, &x, &y);
        if (x >= W) continue;
        if (x < 0 || x + R.v > W || y < 0 || y >= H) { broken++; continue; }
        for (int j = 0; j < R.v; j++) visits[(size_t)y * W + x + j]++;
      }
  }
  return broken;
}
