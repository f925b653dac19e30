// Stand-alone check of mn_tile_runs.h for tests/test_tiles4_runs.py: the run starts the tile stage of the labelling
// takes from a tile row's link mask, against a loop that walks left pixel by pixel.  Compiled by g++ alone, with the
// address and undefined-behaviour sanitizers; prints one line and exits 0 when every mask agrees.
#include <stdint.h>
#include <stdio.h>

#include "../../mergenet_amd/csrc/mn_tile_runs.h"

// column `col` belongs to the run of col - 1 iff bit col - 1 (col - 1 is joined to its successor) is set
static int naive_start(unsigned long long links, int col) {
  int s = col;
  while (s > 0 && ((links >> (s - 1)) & 1ull)) s--;
  return s;
}

static long long checked = 0;

static int check_mask(unsigned long long links) {
  for (int col = 0; col < 64; col++) {
    const int got = mn_run_start(links, col), want = naive_start(links, col);
    if (got != want) {
      printf("mn_run_start(%#llx, %d) = %d, the loop says %d\n", links, col, got, want);
      return 1;
    }
  }
  for (int l16 = 0; l16 < 16; l16++) {
    const unsigned L = (unsigned)(links >> (4 * l16)) & 15u;
    int s[4] = {-1, -1, -1, -1};
    mn_run_starts4(links, l16, L, s);
    for (int j = 0; j < 4; j++) {
      const int want = naive_start(links, 4 * l16 + j);
      if (s[j] != want) {
        printf("mn_run_starts4(%#llx, %d, %#x)[%d] = %d, the loop says %d\n", links, l16, L, j, s[j], want);
        return 1;
      }
    }
    // the kernel clears the lane's fourth bit in the row's last lane (the link across the tile's right border):
    // the lane's own starts must not depend on it
    int s3[4];
    mn_run_starts4(links, l16, L & 7u, s3);
    for (int j = 0; j < 4; j++)
      if (s3[j] != s[j]) {
        printf("mn_run_starts4(%#llx, %d): start %d depends on the lane's fourth link bit\n", links, l16, j);
        return 1;
      }
  }
  checked++;
  return 0;
}

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next_random() {                 // xorshift64*
  state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
  return state * 0x2545F4914F6CDD1Dull;
}

int main() {
  if (check_mask(0ull) || check_mask(~0ull) || check_mask(~0ull >> 1)) return 1;
  for (int b = 0; b < 64; b++)
    if (check_mask(1ull << b) || check_mask(~(1ull << b))) return 1;
  for (int n = 0; n < 4096; n++) {
    const uint64_t a = next_random(), b = next_random(), c = next_random();
    // every density of links: half, a quarter (short runs), three quarters and seven eighths (long runs)
    if (check_mask(a) || check_mask(a & b) || check_mask(a | b) || check_mask(a | b | c)) return 1;
  }
  printf("tile runs ok: %lld masks\n", checked);
  return 0;
}
