// mn_kernels_eval.h -- the dataset-level half of the evaluation on the device: a log of one record per detection,
// appended per image, and from it COCOeval's precision[T,R,K,A,M], recall[T,K,A,M] and scores[T,R,K,A,M].
//
// Reference work replaced (the end of the Cityscapes and COCO callers):
//   COCOeval(...).accumulate()        egs/cityscape/local/evaluate.py:67-73    per class, area range and maxDets:
//                                                                              concatenate, mergesort, cumsum, envelope,
//                                                                              searchsorted
//   (evaluate() per image is mn_kernels_match.h; summarize() is a few means of these arrays, taken on the host)
// Definitions (mergenet_hip.h gives them in full; labels.eval_records / labels.coco_accumulate are the statements):
//   per image: rank[d] = detections of d's class before d in detection order; a detection with rank >= the largest
//     maxDets is left out of the matching; one matching per area range; a record per detection, in detection order;
//     npig[c][a] += truth instances of class c that range a does not ignore;
//   per (class k, range a, maxDets m, threshold t): the records of class k with rank < m, by descending score
//     (stable, NaN last): tp / fp = running counts of the matched / unmatched among the non-ignored,
//     rc = tp / npig, pr = tp / (fp + tp + eps), pr made non-increasing from the right, and per recall threshold the
//     pr and score at the first position with rc >= the threshold.  float64, every division ONE IEEE division of
//     exact integers: the arrays equal the numpy statement bit for bit.
#pragma once

#include <float.h>

#include "mn_device.h"
#include "mn_kernels_match.h"

#define MN_EVAL_THREADS 256       /* == MN_EVAL_CHUNK: a lane per record of the chunk */
static_assert(MN_EVAL_THREADS == MN_EVAL_CHUNK, "the scan takes one record per lane");

// A record: 32 bytes, two 16-byte stores.  Bit a * T + t of `matched` / `ignored` belongs to area range a and
// threshold t (A * T <= 64).
//   word 0: class   1: score (float32 bits)   2: rank   3: image ordinal
//   words 4-5: matched (low word first)   6-7: ignored
struct MnAreaRanges { double lo[MN_EVAL_MAX_AREAS], hi[MN_EVAL_MAX_AREAS]; };
struct MnMaxDets { int m[MN_EVAL_MAX_DETS]; };

// Scratch of one append, in the context (allocated at first use).
struct MnEvalWork {
  int order[MN_MATCH_MAX_INSTANCES];              // order[p] = label - 1 of the detection taken p-th (ALL detections)
  int rank[MN_MATCH_MAX_INSTANCES];               // by label - 1
  int pred_match[MN_EVAL_MAX_AREAS * 16 * MN_MATCH_MAX_INSTANCES];             // [A][T][K]
  unsigned char pred_ignore[MN_EVAL_MAX_AREAS * 16 * MN_MATCH_MAX_INSTANCES];   // [A][T][K]
  int truth_match[16 * MN_MATCH_MAX_INSTANCES];   // [T][G]: of the range matched last; nothing reads it
};

__device__ __forceinline__ bool mn_eval_before(float si, int i, float sk, int k) {
  // detection i is taken before detection k (the order of mn_match_rank: descending score, equal scores by label,
  // NaN last)
  const bool ni = si != si, nk = sk != sk;
  return (ni != nk) ? nk : (ni ? i < k : (si > sk || (si == sk && i < k)));
}

// Every workgroup keeps all K classes and scores in LDS (32 KB at K = 4096); a lane per detection counts the
// detections before it, K comparisons, and among them those of its class.  Writes the order of ALL detections for
// the pack kernel, and the order the matching walks: there a detection beyond the cut is entered as label 0, which
// mn_match_greedy passes over -- it neither matches nor holds a truth instance.  (An entry passed over runs no
// barrier there; the loop's LDS slots alternate on the detections it takes, so passing over is ordered.)  Without scores every score is 1
// (egs/cityscape/local/segment.py:181) and the order is the labels'.
__global__ __launch_bounds__(MN_EVAL_THREADS) void mn_eval_rank(int K, const int* __restrict__ pred_class,
                                                                const float* __restrict__ score, int max_det,
                                                                MnMatchWork* __restrict__ w,
                                                                MnEvalWork* __restrict__ e) {
  __shared__ int s_cls[MN_MATCH_MAX_INSTANCES];
  __shared__ float s_sc[MN_MATCH_MAX_INSTANCES];
  for (int i = threadIdx.x; i < K; i += MN_EVAL_THREADS) {
    s_cls[i] = pred_class[i];
    s_sc[i] = score ? score[i] : 1.0f;
  }
  __syncthreads();
  const int k = blockIdx.x * MN_EVAL_THREADS + threadIdx.x;
  if (k >= K) return;
  const int ck = s_cls[k];
  const float sk = s_sc[k];
  int pos = 0, rank = 0;
  for (int i = 0; i < K; i++) {                     // (every lane reads the same entry: an LDS broadcast)
    const bool first = mn_eval_before(s_sc[i], i, sk, k);
    pos += first ? 1 : 0;
    rank += (first && s_cls[i] == ck) ? 1 : 0;
  }
  // pos counts detections other than k: 0 <= pos <= K - 1, and the order is total, so the positions are a permutation
  e->order[pos] = k;
  e->rank[k] = rank;
  w->order_p[pos] = rank < max_det ? k + 1 : 0;
}

// npig[c][a] += 1 for every truth instance j of class c in 0..C-1 that range a does not ignore.  area_g is what
// mn_match_areas left (it does not depend on the range).  Integer atomics: the sum has no order.
__global__ __launch_bounds__(MN_EVAL_THREADS) void mn_eval_npig(int G, const int* __restrict__ truth_class,
                                                                const unsigned char* __restrict__ crowd,
                                                                const MnMatchWork* __restrict__ w, int C, int A,
                                                                MnAreaRanges ar, u64* __restrict__ npig) {
  const int j = blockIdx.x * MN_EVAL_THREADS + threadIdx.x;
  if (j >= G) return;
  const int c = truth_class[j];
  if ((unsigned)c >= (unsigned)C || (crowd && crowd[j])) return;
  const double ag = w->area_g[j];
  for (int a = 0; a < A; a++)
    if (!(ag < ar.lo[a] || ag > ar.hi[a])) atomicAdd(npig + (size_t)c * A + a, 1ull);
}

// A lane per detection, in detection order: lane p writes the record of the detection taken p-th.  A detection
// beyond the cut, and every detection of an image without truth instances (matched == 0: no matching ran), is
// unmatched: ignored iff its own area lies outside the range.
__global__ __launch_bounds__(MN_EVAL_THREADS) void mn_eval_pack(int K, int T, int A, MnAreaRanges ar, int max_det,
                                                                int matched, const int* __restrict__ pred_class,
                                                                const float* __restrict__ score,
                                                                const MnMatchWork* __restrict__ w,
                                                                const MnEvalWork* __restrict__ e, int image,
                                                                uint4* __restrict__ rec) {
  const int p = blockIdx.x * MN_EVAL_THREADS + threadIdx.x;
  if (p >= K) return;
  const int d = e->order[p];
  if ((unsigned)d >= (unsigned)K) return;           // (a permutation of 0..K-1; d forms addresses, so it is held to them)
  const int rank = e->rank[d];
  const bool in_matching = matched && rank < max_det;
  const double ap = w->area_p[d];
  u64 mt = 0, ig = 0;
  for (int a = 0; a < A; a++) {
    const bool outside = ap < ar.lo[a] || ap > ar.hi[a];
    for (int t = 0; t < T; t++) {
      const size_t at = ((size_t)a * T + t) * (size_t)K + (size_t)d;
      const bool m = in_matching && e->pred_match[at] != 0;
      const bool i = in_matching ? e->pred_ignore[at] != 0 : outside;
      mt |= (u64)(m ? 1 : 0) << (a * T + t);
      ig |= (u64)(i ? 1 : 0) << (a * T + t);
    }
  }
  const float s = score ? score[d] : 1.0f;
  rec[2 * (size_t)p] = make_uint4((unsigned)pred_class[d], __float_as_uint(s), (unsigned)rank, (unsigned)image);
  rec[2 * (size_t)p + 1] = make_uint4((unsigned)mt, (unsigned)(mt >> 32), (unsigned)ig, (unsigned)(ig >> 32));
}

// ---- accumulate -----------------------------------------------------------------------------------------------

// key = class << 32 | score key: ascending keys are ascending class, then DESCENDING score with NaN last; equal
// scores (-0 and +0 are equal) give equal keys, so a stable sort keeps their order in the log.  A class outside
// 0..C-1 becomes C: behind every class that is selected.
__global__ __launch_bounds__(MN_EVAL_THREADS) void mn_eval_keys(const uint4* __restrict__ rec, int N, int C,
                                                                i64* __restrict__ keys) {
  const int i = blockIdx.x * MN_EVAL_THREADS + threadIdx.x;
  if (i >= N) return;
  const uint4 h = rec[2 * (size_t)i];
  const unsigned c = h.x < (unsigned)C ? h.x : (unsigned)C;
  float s = __uint_as_float(h.y);
  unsigned u = 0xFFFFFFFFu;                          // NaN: behind every score (no other score maps here)
  if (s == s) {
    if (s == 0.0f) s = 0.0f;
    const unsigned b = __float_as_uint(s);
    u = ~((b & 0x80000000u) ? ~b : (b | 0x80000000u));
  }
  keys[i] = (i64)(((u64)c << 32) | (u64)u);
}

__device__ __forceinline__ int mn_eval_lower_bound(const i64* __restrict__ keys, int N, i64 v) {
  int lo = 0, hi = N;                                // first position with keys[p] >= v; lo <= mid < hi <= N throughout
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One workgroup per (class k, area range a, maxDets m, threshold t): blockIdx.x = (k * A + a) * M + m, blockIdx.y = t.
// The class's records are the positions [s0, s1) of the sorted log.  Pass 1 counts the selected records (rank < m),
// their true and false positives and finds the first of them.  Pass 2 walks the segment BACKWARDS in chunks of
// MN_EVAL_CHUNK, a lane per record: a wave64 + LDS inclusive prefix sum of the two counts packed in one 64-bit word,
// made global by what the chunks before hold (the totals less the chunks already walked); pr at every selected
// position; an inclusive suffix maximum of pr over the chunk joined with the maximum of the chunks behind (the
// carry): the envelope.  The first position with rc >= a threshold is the first selected record (rc of "before" is
// below everything) or a position where tp rises, so those lanes alone look for the thresholds they answer, and
// write them.  What no position answers -- thresholds above the last rc, NaN ones, all of them when nothing is
// selected -- is written 0 at the end; with npig == 0 everything is -1.  Every entry is written exactly once.
__global__ __launch_bounds__(MN_EVAL_THREADS) void mn_eval_scan(const uint4* __restrict__ rec, int N,
                                                                const i64* __restrict__ keys,
                                                                const i64* __restrict__ index,
                                                                const i64* __restrict__ npig, int C, int T, int R,
                                                                int A, int M, MnMaxDets md,
                                                                const double* __restrict__ rec_thr,
                                                                double* __restrict__ precision,
                                                                double* __restrict__ recall,
                                                                double* __restrict__ scores) {
  __shared__ i64 s_sum[MN_EVAL_THREADS / 64];
  __shared__ double s_max[MN_EVAL_THREADS / 64];
  __shared__ int s_red[MN_EVAL_THREADS / 64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.x % M, a = (blockIdx.x / M) % A, k = blockIdx.x / (M * A), t = blockIdx.y;
  const int max_det = md.m[m], bit = a * T + t;
  auto out_at = [&](int r) { return ((((size_t)t * R + r) * C + k) * A + a) * M + m; };
  const size_t recall_at = (((size_t)t * C + k) * A + a) * M + m;

  const i64 np = npig[(size_t)k * A + a];
  if (np <= 0) {
    for (int r = tid; r < R; r += MN_EVAL_THREADS) { precision[out_at(r)] = -1.0; scores[out_at(r)] = -1.0; }
    if (tid == 0) recall[recall_at] = -1.0;
    return;
  }
  const double dn = (double)np;
  const int s0 = mn_eval_lower_bound(keys, N, (i64)k << 32);
  const int s1 = mn_eval_lower_bound(keys, N, (i64)(k + 1) << 32);

  // the record at sorted position i: selected?  its flags and score
  auto load = [&](int i, int& tpf, int& fpf, float& score) {
    tpf = fpf = 0;
    const i64 src = index[i];
    if ((u64)src >= (u64)N) return false;            // (a permutation of 0..N-1; it forms an address)
    const uint4 h = rec[2 * (size_t)src];
    if ((int)h.x != k || (int)h.z >= max_det) return false;
    const uint4 b = rec[2 * (size_t)src + 1];
    const bool mt = (((u64)b.x | ((u64)b.y << 32)) >> bit) & 1ull;
    const bool ig = (((u64)b.z | ((u64)b.w << 32)) >> bit) & 1ull;
    tpf = (mt && !ig) ? 1 : 0;
    fpf = (!mt && !ig) ? 1 : 0;
    score = __uint_as_float(h.y);
    return true;
  };

  int tp = 0, fp = 0, nd = 0, first = N;
  for (int i = s0 + tid; i < s1; i += MN_EVAL_THREADS) {
    int tpf, fpf;
    float sc;
    if (load(i, tpf, fpf, sc)) { nd++; tp += tpf; fp += fpf; first = min(first, i); }
  }
  for (int d = 32; d > 0; d >>= 1) {
    tp += __shfl_xor(tp, d); fp += __shfl_xor(fp, d); nd += __shfl_xor(nd, d); first = min(first, __shfl_xor(first, d));
  }
  if (lane == 0) { s_red[wave][0] = tp; s_red[wave][1] = fp; s_red[wave][2] = nd; s_red[wave][3] = first; }
  __syncthreads();
  tp = fp = nd = 0; first = N;
  for (int q = 0; q < MN_EVAL_THREADS / 64; q++) {
    tp += s_red[q][0]; fp += s_red[q][1]; nd += s_red[q][2]; first = min(first, s_red[q][3]);
  }
  const double rc_last = (double)tp / dn;
  if (tid == 0) recall[recall_at] = nd > 0 ? rc_last : 0.0;

  int tp_end = tp, fp_end = fp;                      // the counts up to the end of the chunk at hand
  double carry = -1.0;                               // maximum of pr behind the chunk at hand (pr >= 0 where selected)
  for (int c = (s1 - s0 + MN_EVAL_CHUNK - 1) / MN_EVAL_CHUNK - 1; c >= 0 && nd > 0; c--) {
    const int i = s0 + c * MN_EVAL_CHUNK + tid;
    int tpf = 0, fpf = 0;
    float sc = 0.0f;
    const bool sel = i < s1 && load(i, tpf, fpf, sc);
    i64 incl = ((i64)tpf << 32) | (i64)fpf;
    for (int d = 1; d < 64; d <<= 1) {
      const i64 o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == 63) s_sum[wave] = incl;
    __syncthreads();
    i64 total = 0;
    for (int q = 0; q < MN_EVAL_THREADS / 64; q++) {
      const i64 v = s_sum[q];
      if (q < wave) incl += v;
      total += v;
    }
    const int tpi = tp_end - (int)(total >> 32) + (int)(incl >> 32);
    const int fpi = fp_end - (int)(total & 0xFFFFFFFFll) + (int)(incl & 0xFFFFFFFFll);
    const double pr = sel ? (double)tpi / ((double)fpi + (double)tpi + DBL_EPSILON) : -1.0;
    double suf = pr;
    for (int d = 1; d < 64; d <<= 1) {
      const double o = __shfl_down(suf, d);
      if (lane + d < 64) suf = fmax(suf, o);
    }
    if (lane == 0) s_max[wave] = suf;
    __syncthreads();
    double behind = carry, all = carry;
    for (int q = 0; q < MN_EVAL_THREADS / 64; q++) {
      const double v = s_max[q];
      if (q > wave) behind = fmax(behind, v);
      all = fmax(all, v);
    }
    if (sel && (tpf || i == first)) {
      const double env = fmax(suf, behind);
      const double rc = (double)tpi / dn, rc_before = (double)(tpi - tpf) / dn;
      for (int r = 0; r < R; r++) {
        const double thr = rec_thr[r];
        if (thr <= rc && (i == first || !(thr <= rc_before))) {
          precision[out_at(r)] = env;
          scores[out_at(r)] = (double)sc;
        }
      }
    }
    carry = all;
    tp_end -= (int)(total >> 32);
    fp_end -= (int)(total & 0xFFFFFFFFll);
  }
  for (int r = tid; r < R; r += MN_EVAL_THREADS)
    if (!(nd > 0 && rec_thr[r] <= rc_last)) { precision[out_at(r)] = 0.0; scores[out_at(r)] = 0.0; }
}
