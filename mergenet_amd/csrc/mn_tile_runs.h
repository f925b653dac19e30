// mn_tile_runs.h -- the mask arithmetic of the tile stage's rows (mn_cc_tiles, mn_cc_tiles4): where the run of a
// pixel starts, from the link mask of its 64-pixel tile row.  Bit c of the mask says that pixel c is joined to pixel
// c + 1 of the same tile row (bit 63 is never set: the link across the tile's right border is the border stage's).
// Plain integer arithmetic that g++ alone compiles (tests/tools/tile_runs_check.cpp, tests/test_tiles4_runs.py).
#pragma once
#if defined(__HIPCC__) || defined(__HIP__)
#define MN_RUNS_HD __host__ __device__ __forceinline__
#else
#define MN_RUNS_HD static inline
#endif

// Run start of column `col` (0..63): one past the highest column below `col` that has NO link to its successor.
MN_RUNS_HD int mn_run_start(unsigned long long links, int col) {
  const unsigned long long below = col ? (~links & ((1ull << col) - 1ull)) : 0ull;
  return below ? (64 - __builtin_clzll(below)) : 0;
}

// A lane of mn_cc_tiles4 holds the four columns 4 * l16 + j, j = 0..3, and their link bits as the nibble L (bit j:
// column 4 * l16 + j is joined to its successor; L is the lane's nibble of `links`).  The first column's start comes
// from the mask, each further one is its predecessor's where the two are joined and itself where they are not.
MN_RUNS_HD void mn_run_starts4(unsigned long long links, int l16, unsigned L, int start[4]) {
  const int col = 4 * l16;
  start[0] = mn_run_start(links, col);
  start[1] = (L & 1u) ? start[0] : col + 1;
  start[2] = (L & 2u) ? start[1] : col + 2;
  start[3] = (L & 4u) ? start[2] : col + 3;
}
