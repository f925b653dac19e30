// mn_kernels_rle.h -- the ground-truth label mask from COCO run-length encodings on the device: the decoding half
// of the RLE path (mn_rle_points_device + mn_rle_encode_host are the encoding half).
//
// Reference work replaced:
//   anns_to_mask / anns_to_mask_class   utils/dataset.py:486-522   one maskUtils.decode per annotation, painted in
//                                                                  list order with mask = m * (mask == 0) + mask
//   maskUtils.area                      egs/cityscape/local/evaluate.py:48-54
// Definitions (mergenet_amd/rle.py::label_mask is the numpy statement):
//   the counts of one annotation are the lengths of alternating 0/1 runs of its binary mask in COLUMN-major order,
//   the first run zeros; run i (0-based) covers the scan positions [end[i-1], end[i]) with end[i] the inclusive
//   prefix sum of the counts, and is set when i is odd.  A position p is inside the annotation iff the number of
//   ends <= p is odd; a zero-length run gives two equal ends, which cancel.
//   mask[p] = the value of the FIRST annotation in list order with a nonzero value that p is inside, else 0.
//   area[a] = the sum of a's odd-indexed counts.
// Two kernels:
//   mn_rle_scan    one workgroup per annotation: prefix sum of its counts -> the run ends, clamped to H * W, and a
//                  record {first set position, one past the last set position, where its ends start, how many};
//   mn_rle_paint   a GATHER: a wave owns 64 rows of MN_RLE_WAVE_COLS columns, looks up for the annotations in list
//                  order which ends fall into the 64 positions of each column, and takes the first annotation
//                  that covers a row; the labels wait in an LDS tile and leave row by row.
// No scan position ever forms an address: ends are compared with positions and subtracted from them (a shift count
// below 64); the addresses are indices into the counts (bounded by num_counts), the annotations, and row / column
// coordinates tested against H and W.
#pragma once

#include "mn_device.h"

#define MN_RLE_SCAN_THREADS 256
#define MN_RLE_SCAN_ITEMS 4          /* consecutive counts per thread: a chunk of the scan is 1024 counts */
// Forms of the paint pass; a variant build for tools/time_rle_decode.py sets another (-DMN_RLE_PAINT_FORM=n),
// profiles/rle_decode_time.log has all three:
//   0  a LANE per (annotation, column): 8 annotations x 8 columns are looked up side by side, each lane bisecting
//      the annotation's ends for its own column (what ships);
//   1  a WAVE per (annotation, column), one after the other, the index of the first end behind the segment's start
//      carried from column to column and looked for among the 64 ends from there;
//   2  as 1, with a fresh bisection of all ends in every column.
#ifndef MN_RLE_PAINT_FORM
#define MN_RLE_PAINT_FORM 0
#endif
#if MN_RLE_PAINT_FORM == 0
#define MN_RLE_PAINT_THREADS 512
#define MN_RLE_WAVE_COLS 8           /* columns a wave paints; the workgroup's tile is 64 rows x 64 columns */
#else
#define MN_RLE_PAINT_THREADS 256
#define MN_RLE_WAVE_COLS 16
#define MN_RLE_CARRY (MN_RLE_PAINT_FORM == 1)
#endif
#define MN_RLE_SLOTS (64 / MN_RLE_WAVE_COLS)      /* form 0: annotations a wave looks up side by side */
#define MN_RLE_TILE_COLS (MN_RLE_WAVE_COLS * (MN_RLE_PAINT_THREADS / 64))
#define MN_RLE_TILE_PITCH 65         /* ints per tile column in LDS: 64 rows + 1, so that both the column-wise
                                        writes and the row-wise reads touch 64 different banks */

// Record of one annotation, written by mn_rle_scan and read by mn_rle_paint (4 ints, 16 bytes).
struct MnRleRecord {
  int first;   // first set scan position; H * W when nothing is set
  int last;    // one past the last set scan position; 0 when nothing is set
  int begin;   // index of its first end in the ends array (its starts[] entry held to 0..num_counts)
  int count;   // number of its ends (begin + count <= num_counts)
};

// One workgroup per annotation.  A chunk is 256 threads x 4 consecutive counts; the inclusive prefix sum of a chunk
// is taken per thread, then across the lanes of a wave by shuffles, then across the four waves through LDS, and a
// carry joins the chunks.  Sums are 64-bit and every end is clamped to N = H * W before it is stored, so whatever
// the counts hold the ends are ascending values in 0..N.  The next chunk's counts are loaded before this chunk's
// barriers.  area = sum over the odd runs of (end - end before), which is the sum of the odd counts whenever the
// counts sum to no more than N.
__global__ __launch_bounds__(MN_RLE_SCAN_THREADS) void mn_rle_scan(const unsigned* __restrict__ counts,
                                                                   const int* __restrict__ starts, int num_counts,
                                                                   unsigned N, unsigned* __restrict__ ends,
                                                                   MnRleRecord* __restrict__ rec,
                                                                   int* __restrict__ area) {
  __shared__ u64 wave_sum[MN_RLE_SCAN_THREADS / 64];
  __shared__ int red[3][MN_RLE_SCAN_THREADS / 64];
  const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned T = (unsigned)num_counts;
  const unsigned s0 = min((unsigned)starts[a], T);                   // (a negative start reads as "at the end")
  const unsigned s1 = min(max((unsigned)starts[a + 1], s0), T);
  const int n = (int)(s1 - s0);
  const int chunk = MN_RLE_SCAN_THREADS * MN_RLE_SCAN_ITEMS;

  auto load = [&](int base, unsigned* c) {
#pragma unroll
    for (int k = 0; k < MN_RLE_SCAN_ITEMS; k++) {
      const int i = base + tid * MN_RLE_SCAN_ITEMS + k;
      c[k] = i < n ? counts[s0 + (unsigned)i] : 0u;
    }
  };

  u64 carry = 0;                        // the end before this chunk, <= N
  int my_area = 0, my_first = (int)N, my_last = 0;
  unsigned next[MN_RLE_SCAN_ITEMS];
  if (n > 0) load(0, next);
  for (int base = 0; base < n; base += chunk) {
    unsigned c[MN_RLE_SCAN_ITEMS];
#pragma unroll
    for (int k = 0; k < MN_RLE_SCAN_ITEMS; k++) c[k] = next[k];
    if (base + chunk < n) load(base + chunk, next);
    u64 mine = 0;
#pragma unroll
    for (int k = 0; k < MN_RLE_SCAN_ITEMS; k++) mine += c[k];
    u64 incl = mine;                    // inclusive over the lanes of this wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    u64 before = carry, total = 0;
#pragma unroll
    for (int q = 0; q < MN_RLE_SCAN_THREADS / 64; q++) {
      const u64 s = wave_sum[q];
      if (q < wave) before += s;
      total += s;
    }
    __syncthreads();                    // (wave_sum is written again in the next chunk)
    u64 run = before + incl - mine;     // the end before this thread's first count (unclamped)
#pragma unroll
    for (int k = 0; k < MN_RLE_SCAN_ITEMS; k++) {
      const int i = base + tid * MN_RLE_SCAN_ITEMS + k;
      const unsigned lo = (unsigned)min(run, (u64)N);
      run += c[k];
      const unsigned hi = (unsigned)min(run, (u64)N);
      if (i < n) {
        ends[s0 + (unsigned)i] = hi;
        if ((i & 1) && hi > lo) {
          my_area += (int)(hi - lo);
          my_first = min(my_first, (int)lo);
          my_last = max(my_last, (int)hi);
        }
      }
    }
    carry = min(carry + total, (u64)N);
  }

#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    my_area += __shfl_xor(my_area, d);
    my_first = min(my_first, __shfl_xor(my_first, d));
    my_last = max(my_last, __shfl_xor(my_last, d));
  }
  if (lane == 0) { red[0][wave] = my_area; red[1][wave] = my_first; red[2][wave] = my_last; }
  __syncthreads();
  if (tid == 0) {
    int ar = 0, fi = (int)N, la = 0;
#pragma unroll
    for (int q = 0; q < MN_RLE_SCAN_THREADS / 64; q++) {
      ar += red[0][q];
      fi = min(fi, red[1][q]);
      la = max(la, red[2][q]);
    }
    MnRleRecord r;
    r.first = fi; r.last = la; r.begin = (int)s0; r.count = n;
    rec[a] = r;
    if (area) area[a] = ar;
  }
}

// First index j in 0..n with e[j] > p (n when there is none), by a four-way search: three probes per step, which
// are independent loads, so a step costs one memory latency and there are half as many steps as in a bisection.
__device__ __forceinline__ int mn_rle_upper4(const unsigned* __restrict__ e, int n, unsigned p) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int len = hi - lo;
    const int m1 = lo + (len >> 2), m2 = lo + (len >> 1), m3 = lo + (len >> 1) + (len >> 2);   // lo <= m1 <= m2 <= m3 < hi
    const unsigned v1 = e[m1], v2 = e[m2], v3 = e[m3];
    if (v1 > p) hi = m1;
    else if (v2 > p) { lo = m1 + 1; hi = m2; }
    else if (v3 > p) { lo = m2 + 1; hi = m3; }
    else lo = m3 + 1;
  }
  return lo;
}

#if MN_RLE_PAINT_FORM == 0
// A workgroup paints a tile of 64 rows x 64 columns, a wave 64 rows x 8 columns of it.  The pass is bound by the
// latency of dependent loads (the search for the ends of one column), so the lanes of a wave search side by side:
// in the LOOK-UP a lane stands for one (annotation, column) pair, in the PAINT for one row.
//   Candidates: the annotations in list order, 64 at a time, each lane testing one record against the wave's range
//   of positions (the value 0 paints nothing and is dropped); a ballot lists the candidates in order.
//   Look-up, 8 candidates x 8 columns at a time: lane (slot, c) takes the slot-th candidate and column c, whose
//   segment is the positions p0 .. p0 + rows - 1, p0 = column * H + first row.  j = number of the annotation's ends
//   <= p0 (four-way search); from there it reads ends, four per step, while they lie inside the segment and XORs the
//   bit (end - p0) into a word -- two equal ends, a zero-length run, cancel.  A prefix XOR over the word turns the
//   toggles into the inside bits of the 64 rows, inverted when j is odd (the segment starts inside a set run).
//   Paint: the words that are not zero, in lane order -- slot by slot, so per column in list order -- are read by
//   every lane; row `lane` takes the value where its bit is set and its label is still 0.
// Every loop over ends advances, so it is bounded by the number of counts.
__global__ __launch_bounds__(MN_RLE_PAINT_THREADS) void mn_rle_paint(const unsigned* __restrict__ ends,
                                                                     const MnRleRecord* __restrict__ rec,
                                                                     const int* __restrict__ values, int A, int H,
                                                                     int W, int* __restrict__ mask) {
  __shared__ int tile[MN_RLE_TILE_COLS * MN_RLE_TILE_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * 64;                                    // first row of the tile (< H)
  const int x0 = blockIdx.x * MN_RLE_TILE_COLS + wave * MN_RLE_WAVE_COLS;      // first column of this wave
  const int rows = min(64, H - r0);                                  // >= 1
  const int cols = min(MN_RLE_WAVE_COLS, W - x0);                    // may be <= 0: nothing to paint
  int* mine = tile + wave * MN_RLE_WAVE_COLS * MN_RLE_TILE_PITCH;
#pragma unroll
  for (int c = 0; c < MN_RLE_WAVE_COLS; c++) mine[c * MN_RLE_TILE_PITCH + lane] = 0;

  if (cols > 0) {
    // positions this wave covers: [wave_lo, wave_hi), both <= H * W < 2^31
    const int wave_lo = x0 * H + r0, wave_hi = (x0 + cols - 1) * H + r0 + rows;
    const int c = lane % MN_RLE_WAVE_COLS, slot = lane / MN_RLE_WAVE_COLS;      // the look-up's pair of this lane
    const bool my_col = c < cols;
    const int p0 = my_col ? (x0 + c) * H + r0 : 0, p1 = p0 + rows;   // its segment [p0, p1), p1 <= H * W
    for (int a0 = 0; a0 < A; a0 += 64) {
      const int a = a0 + lane;
      MnRleRecord r;
      r.first = 0x7fffffff; r.last = 0; r.begin = 0; r.count = 0;
      int value = 0;
      if (a < A) {
        r = rec[a];
        value = values ? values[a] : a + 1;
      }
      u64 todo = __ballot(value != 0 && r.first < wave_hi && r.last > wave_lo);
      while (todo) {
        int from = -1;                                               // the lane that holds my candidate's record
#pragma unroll
        for (int s = 0; s < MN_RLE_SLOTS; s++) {
          if (todo) {
            if (slot == s) from = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
          }
        }
        const int src = max(from, 0);
        const int first = __shfl(r.first, src), last = __shfl(r.last, src), begin = __shfl(r.begin, src);
        const int n = __shfl(r.count, src), v = __shfl(value, src);
        u64 word = 0;
        if (from >= 0 && my_col && first < p1 && last > p0) {
          const unsigned* __restrict__ e = ends + begin;
          const int j = mn_rle_upper4(e, n, (unsigned)p0);
          u64 x = 0;
          bool more = true;
          for (int k = j; more && k < n; k += 4) {
            unsigned ev[4];
#pragma unroll
            for (int i = 0; i < 4; i++) ev[i] = (k + i < n) ? e[k + i] : 0xffffffffu;
#pragma unroll
            for (int i = 0; i < 4; i++) {
              more = more && ev[i] < (unsigned)p1;                   // (ascending: behind the first end past the
              if (more) x ^= 1ull << ((ev[i] - (unsigned)p0) & 63);  //  segment nothing is inside it; p0 < end < p1)
            }
          }
          x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
          if (j & 1) x = ~x;
          const int live = min(rows, last - p0);                     // >= 1: rows of the image before `last`
          if (live < 64) x &= (1ull << live) - 1ull;
          word = x;
        }
        u64 filled = __ballot(word != 0);
        const unsigned word_lo = (unsigned)word, word_hi = (unsigned)(word >> 32);
        while (filled) {
          const int l = __ffsll((long long)filled) - 1;
          filled &= filled - 1;
          const u64 w = (u64)(unsigned)__builtin_amdgcn_readlane((int)word_lo, l) |
                        ((u64)(unsigned)__builtin_amdgcn_readlane((int)word_hi, l) << 32);
          const int vv = __builtin_amdgcn_readlane(v, l);
          int* cell = mine + (l % MN_RLE_WAVE_COLS) * MN_RLE_TILE_PITCH + lane;
          if (((w >> lane) & 1ull) && *cell == 0) *cell = vv;
        }
      }
    }
  }
  __syncthreads();
  // row by row: lane = column of the tile, 256 contiguous bytes per store
  const int tx = blockIdx.x * MN_RLE_TILE_COLS + lane;
  if (tx < W)
    for (int r = wave; r < rows; r += MN_RLE_PAINT_THREADS / 64)
      mask[(size_t)(r0 + r) * (size_t)W + (size_t)tx] = tile[lane * MN_RLE_TILE_PITCH + r];
}

#else   // ---- forms 1 and 2: kept for the timing tool ------------------------------------------------------------
// First index j in lo..hi with e[j] > p (hi when there is none); the same for every lane of the wave.
__device__ __forceinline__ int mn_rle_upper(const unsigned* __restrict__ e, int lo, int hi, unsigned p) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (e[mid] > p) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// A workgroup paints a tile of 64 rows x 64 columns, a wave 64 rows x 16 columns of it; lane = row.  For the
// annotations in list order, 64 at a time: each lane tests one record against the wave's range of positions (and
// drops the value 0, which paints nothing), a ballot lists the candidates in order.  For a candidate the wave
// goes through its columns; the segment of a column is the positions p0 .. p0 + 63, p0 = column * H + first row:
//   j     = number of the annotation's ends <= p0 (MN_RLE_CARRY: looked for among the 64 ends behind the j of
//           the column before, by bisection of the rest when it is not there; else by bisection of all of them);
//   T     = XOR over the ends e inside the segment behind p0 of the bit e - p0, read 64 ends at a time until one lies
//           behind the segment (two equal ends cancel: a zero-length run toggles nothing);
//   lane l is inside iff j + popcount(T & bits 0..l) is odd, and takes the value if its label is still 0.
// Every loop over ends advances by at least one end, so it is bounded by the number of counts.
__global__ __launch_bounds__(MN_RLE_PAINT_THREADS) void mn_rle_paint(const unsigned* __restrict__ ends,
                                                                     const MnRleRecord* __restrict__ rec,
                                                                     const int* __restrict__ values, int A, int H,
                                                                     int W, int* __restrict__ mask) {
  __shared__ int tile[MN_RLE_TILE_COLS * MN_RLE_TILE_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * 64;                                    // first row of the tile (< H)
  const int x0 = blockIdx.x * MN_RLE_TILE_COLS + wave * MN_RLE_WAVE_COLS;      // first column of this wave
  const int rows = min(64, H - r0);                                  // >= 1
  const int cols = min(MN_RLE_WAVE_COLS, W - x0);                    // may be <= 0: nothing to paint
  int* mine = tile + wave * MN_RLE_WAVE_COLS * MN_RLE_TILE_PITCH;
#pragma unroll
  for (int c = 0; c < MN_RLE_WAVE_COLS; c++) mine[c * MN_RLE_TILE_PITCH + lane] = 0;

  if (cols > 0) {
    // positions this wave covers: [wave_lo, wave_hi), both <= H * W < 2^31
    const int wave_lo = x0 * H + r0, wave_hi = (x0 + cols - 1) * H + r0 + rows;
    for (int a0 = 0; a0 < A; a0 += 64) {
      const int a = a0 + lane;
      MnRleRecord r;
      r.first = 0x7fffffff; r.last = 0; r.begin = 0; r.count = 0;
      int value = 0;
      if (a < A) {
        r = rec[a];
        value = values ? values[a] : a + 1;
      }
      u64 todo = __ballot(value != 0 && r.first < wave_hi && r.last > wave_lo);
      while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int first = __builtin_amdgcn_readlane(r.first, b), last = __builtin_amdgcn_readlane(r.last, b);
        const int n = __builtin_amdgcn_readlane(r.count, b);
        const int v = __builtin_amdgcn_readlane(value, b);
        const unsigned* __restrict__ e = ends + __builtin_amdgcn_readlane(r.begin, b);
        int j = 0;                                                   // ends before it are <= p0 (carried on)
        for (int c = 0; c < cols; c++) {
          const int p0 = (x0 + c) * H + r0, p1 = p0 + rows;
          if (first >= p1 || last <= p0) continue;
          // j = number of ends <= p0; the window of 64 ends from k on is in ek, past the list a value no position
          // reaches; `valid` = its lanes that hold an end > p0 (ascending: the lanes from some lane on)
          int k = j;
          u64 valid = ~0ull;
          unsigned ek = 0;
          if (MN_RLE_CARRY) {
            ek = (k + lane < n) ? e[k + lane] : 0xffffffffu;
            valid = __ballot(ek > (unsigned)p0);
            if (valid) j += __ffsll((long long)valid) - 1;
            else j = mn_rle_upper(e, j + 64, n, (unsigned)p0);       // all 64 are real ends <= p0
          } else {
            j = mn_rle_upper(e, 0, n, (unsigned)p0);
          }
          if (!valid || !MN_RLE_CARRY) {
            k = j;
            valid = ~0ull;
            ek = (k + lane < n) ? e[k + lane] : 0xffffffffu;
          }
          u64 toggles = 0;
          for (;;) {
            const u64 below = __ballot(ek < (unsigned)p1);           // ends inside the segment or before it
            u64 in = below & valid;                                  // p0 < end < p1
            const int d = (int)(ek - (unsigned)p0);                  // 1..63 for the lanes of `in`
            while (in) {
              const int l = __ffsll((long long)in) - 1;
              in &= in - 1;
              toggles ^= 1ull << (__builtin_amdgcn_readlane(d, l) & 63);
            }
            if (!(below >> 63)) break;                               // lane 63: past the list or behind the segment
            k += 64;                                                 // (lane 63 held a real end: k + 63 < n)
            valid = ~0ull;
            ek = (k + lane < n) ? e[k + lane] : 0xffffffffu;
          }
          const u64 upto = (2ull << lane) - 1ull;                    // bits 0..lane (lane 63: all ones)
          const int parity = (j + __popcll(toggles & upto)) & 1;
          if (parity && lane < rows && p0 + lane < last && mine[c * MN_RLE_TILE_PITCH + lane] == 0)
            mine[c * MN_RLE_TILE_PITCH + lane] = v;
        }
      }
    }
  }
  __syncthreads();
  // row by row: lane = column of the tile, 256 contiguous bytes per store
  const int tx = blockIdx.x * MN_RLE_TILE_COLS + lane;
  if (tx < W)
    for (int r = wave; r < rows; r += MN_RLE_PAINT_THREADS / 64)
      mask[(size_t)(r0 + r) * (size_t)W + (size_t)tx] = tile[lane * MN_RLE_TILE_PITCH + r];
}
#endif
