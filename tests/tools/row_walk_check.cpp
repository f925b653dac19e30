// Host shim of mn_row_walk.h and of the host part of mn_truth_pass.h for tests/test_row_walk.py: the headers the mask
// passes are launched and walked by, compiled by g++ alone -- as a shared library, and as a program (main, below) that
// runs under the address and undefined-behaviour sanitizers.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../mergenet_amd/csrc/mn_row_walk.h"
#include "../../mergenet_amd/csrc/mn_truth_pass.h"

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

extern "C" int truth_pass_slots_check(int H, int W, int elem_size, int waves_per_block) {
  return truth_pass_slots(H, W, elem_size, waves_per_block);
}

// offset_list: O (di, dj) pairs; out: the O clamped pairs in the same layout.
extern "C" void truth_pass_offsets_check(const int* offset_list, int O, int H, int W, int* out) {
  int* di = static_cast<int*>(malloc(sizeof(int) * (size_t)(O > 0 ? O : 1)));
  int* dj = static_cast<int*>(malloc(sizeof(int) * (size_t)(O > 0 ? O : 1)));
  truth_pass_offsets(offset_list, O, H, W, di, dj);
  for (int k = 0; k < O; k++) { out[2 * k] = di[k]; out[2 * k + 1] = dj[k]; }
  free(di);
  free(dj);
}

// The program: the arguments are a sequence of requests, each answered by one line of numbers.  The arrays are
// allocated at their exact sizes, so that a read or write past O pairs is an error under the address sanitizer.
//   slots H W elem_size waves_per_block      -> the grid
//   offsets H W O di dj di dj ...            -> the O clamped pairs
int main(int argc, char** argv) {
  int i = 1;
  while (i < argc) {
    const char kind = argv[i][0];
    if (kind == 's' && i + 4 < argc) {
      printf("%d\n", truth_pass_slots_check(atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4])));
      i += 5;
    } else if (kind == 'o' && i + 3 < argc && atoi(argv[i + 3]) >= 0 && i + 3 + 2 * atoi(argv[i + 3]) < argc) {
      const int H = atoi(argv[i + 1]), W = atoi(argv[i + 2]), O = atoi(argv[i + 3]);
      int* in = static_cast<int*>(malloc(sizeof(int) * 2 * (size_t)(O > 0 ? O : 1)));
      int* out = static_cast<int*>(malloc(sizeof(int) * 2 * (size_t)(O > 0 ? O : 1)));
      for (int k = 0; k < 2 * O; k++) in[k] = (int)atoll(argv[i + 4 + k]);
      truth_pass_offsets_check(in, O, H, W, out);
      for (int k = 0; k < 2 * O; k++) printf(k + 1 < 2 * O ? "%d " : "%d", out[k]);
      printf("\n");
      free(in);
      free(out);
      i += 4 + 2 * O;
    } else {
      fprintf(stderr, "row_walk_check: bad request at argument %d\n", i);
      return 2;
    }
  }
  return 0;
}
