// mn_kernels_score.h -- phase A, the affinity-scoring pass (HBM-bound; roofline-judged).
//
// Reference work replaced: ObjectSegmenter::ObjectSegmenter (utils/csegment/segment.cc:153-232):
//   HOT LOOP 1 (:198-207)  per pixel C x logf + first-max argmax      -> mn_class_pass
//   HOT LOOP 2 (:209-231)  per in-bounds (pixel, offset): logf(p), log(1-p), log-odds,
//                          class delta, initial priority, heap push if >= 0 -> mn_edge_pass
// Instead of materialising 20.7 M records and a heap, the edge pass consumes every score on
// the fly and keeps, per pixel, only the best incident record (priority, partner): that is the
// first selection step of the merge phase.  Algorithmic HBM reads: 4*(C+O) bytes per pixel.
#pragma once

#include "mn_device.h"

// ---- class pass: cls[p] = first-max argmax_c logf(class[c][p]) -------------------------------
// 4 consecutive pixels per lane (16-byte loads, 1 KiB per wave-instruction); planes are
// [C][N] so consecutive lanes read consecutive addresses of one plane.
__global__ __launch_bounds__(256) void mn_class_pass(ImgParams P, unsigned char* __restrict__ cls_out) {
  const int n4 = P.N >> 2;
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 best;
    int b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    for (int c = 0; c < P.C; c++) {
      float4 v = mn_ld_class4(P, c, 4 * i);
      if (P.clip) { v.x = mn_clip(v.x); v.y = mn_clip(v.y); v.z = mn_clip(v.z); v.w = mn_clip(v.w); }
      float4 l;
      l.x = logf(v.x); l.y = logf(v.y); l.z = logf(v.z); l.w = logf(v.w);
      if (c == 0) {
        best = l;
      } else {
        if (l.x > best.x) { best.x = l.x; b0 = c; }
        if (l.y > best.y) { best.y = l.y; b1 = c; }
        if (l.z > best.z) { best.z = l.z; b2 = c; }
        if (l.w > best.w) { best.w = l.w; b3 = c; }
      }
    }
    uchar4 o;
    o.x = (unsigned char)b0; o.y = (unsigned char)b1; o.z = (unsigned char)b2; o.w = (unsigned char)b3;
    *reinterpret_cast<uchar4*>(cls_out + 4 * (size_t)i) = o;
  }
  // tail pixels when N is not a multiple of 4
  const int tail0 = n4 << 2;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < P.N - tail0) {
    const int p = tail0 + t;
    float best = 0.0f;
    int b = 0;
    for (int c = 0; c < P.C; c++) {
      const float l = logf(mn_ld_class(P, c, p));
      if (c == 0 || l > best) { best = l; b = c; }
    }
    cls_out[p] = (unsigned char)b;
  }
}

// ---- edge pass: best incident record per pixel ------------------------------------------------
// One lane per pixel; a wave covers 64 consecutive columns of one row, so each of the 2*O
// sameness loads (own value for the outgoing edge, the neighbour's value for the incoming one)
// is a coalesced row segment shifted by a constant.  FIRST = true scores every edge (round 0,
// sub-round 0).  FIRST = false is a later matching sub-round: only edges between two still
// unmatched pixels with positive likelihood gain compete.
template <bool FIRST>
__global__ __launch_bounds__(256) void mn_edge_pass_generic(ImgParams P, ObjState S,
                                                    const unsigned char* __restrict__ matched,
                                                    u64* __restrict__ best_out,
                                                    const int* __restrict__ progress, int s) {
  if (!FIRST && !progress[s - 1]) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.N) return;
  if (!FIRST && matched[p]) { best_out[p] = 0; return; }
  const int r = p / P.W, c = p - r * P.W;
  u64 best = 0;
  for (int k = 0; k < P.O; k++) {
    const int di = P.di[k], dj = P.dj[k];
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {
      // dir 0: outgoing edge p -> q = p + o_k, value stored at p
      // dir 1: incoming edge q = p - o_k -> p, value stored at q
      const int rr = dir ? r - di : r + di;
      const int cc = dir ? c - dj : c + dj;
      if (rr < 0 || rr >= P.H || cc < 0 || cc >= P.W) continue;
      const int q = rr * P.W + cc;
      if (!FIRST && matched[q]) continue;
      const int src = dir ? q : p;
      const float v = mn_same_value(P, mn_ld_same(P, k, src));
      const float oml = mn_fixed_to_float(mn_edge_fixed(v));
      int mc;
      bool pos;
      const float prio = mn_score(P, S, min(p, q), max(p, q), oml, &mc, &pos);
      if (!(prio >= 0.0f)) continue;
      if (!FIRST && !pos) continue;
      const u64 key = mn_pack(prio, q);
      best = key > best ? key : best;
    }
  }
  best_out[p] = best;
}


// ---- edge pass, fast form -----------------------------------------------------------------------
// Same result as the generic form under object_merge_factor > 0, with far less arithmetic: for
// two pixels of the SAME arg-max class the class delta is 0 and the priority is a monotone
// function of the sameness value, so those edges are ranked by the raw value (ties: lower
// partner id) and only the winner's log-odds are evaluated.  Edges between pixels of different
// classes (object boundaries; rare) take the full scoring path.  All 2*O sameness loads and
// 2*O class loads of a pixel are issued before any of them is used (OT is a compile-time offset
// count so the staging arrays live in registers).
__device__ __forceinline__ float mn_pixel_pair_prio(const ImgParams& P, int lo, int hi, int clo,
                                                    int chi, float v, bool* gain_pos) {
  // both objects are single pixels: lp = logf(class plane), n1 = n2 = 1
  const float x = mn_same_value(P, v);
  const float oml = mn_fixed_to_float(mn_edge_fixed(x));
  float cdl = 0.0f;
  if (clo != chi) {
    float best = 0.0f, a0 = 0.0f, b0 = 0.0f;
    for (int c = 0; c < P.C; c++) {
      const float a = logf(mn_ld_class(P, c, lo));
      const float b = logf(mn_ld_class(P, c, hi));
      const float j = a + b;
      if (c == 0 || j > best) best = j;
      if (c == clo) a0 = a;
      if (c == chi) b0 = b;
    }
    cdl = (best - a0) - b0;
  }
  const float num = oml * P.omf + cdl;
  *gain_pos = num > 0.0f;
  if (P.variant == MN_VARIANT_CSEGMENT) return num / 2.0f + P.bias;
  return (num + P.bias) / 1.0f;
}

template <int OT, bool FIRST, bool CLIP>
__global__ __launch_bounds__(256) void mn_edge_pass_fast(ImgParams P,
                                                         const unsigned char* __restrict__ cls0,
                                                         const unsigned char* __restrict__ matched,
                                                         u64* __restrict__ best_out,
                                                         const int* __restrict__ progress, int s) {
  if (!FIRST && !progress[s - 1]) return;   // previous sub-round paired nothing (see mn_pix_match)
  const int tile = mn_xcd_tile((P.N + 255) >> 8, P.banded);
  if (tile < 0) return;
  const int p = tile * 256 + threadIdx.x;
  if (p >= P.N) return;
  if (!FIRST && matched[p]) { best_out[p] = 0; return; }
  const int r = p / P.W, c = p - r * P.W;
  // stage 0: issue every load of the pixel (2*OT sameness values, 2*OT class bytes) before any of
  // them is used -- the staging arrays are registers (compile-time OT, full unroll)
  float val[2 * OT];
  int nb[2 * OT];
  unsigned char nbc[2 * OT];
  const int cp = cls0[p];
#pragma unroll
  for (int k = 0; k < OT; k++) {
    const int di = P.di[k], dj = P.dj[k];
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {
      const int rr = dir ? r - di : r + di;
      const int cc = dir ? c - dj : c + dj;
      const bool ok = (unsigned)rr < (unsigned)P.H && (unsigned)cc < (unsigned)P.W;
      const unsigned q = ok ? (unsigned)(rr * P.W + cc) : (unsigned)p;
      val[2 * k + dir] = mn_ld_same(P, k, (int)(dir ? q : (unsigned)p));
      nbc[2 * k + dir] = cls0[q];
      bool live = ok;
      if (!FIRST) live = live && !matched[q];
      nb[2 * k + dir] = live ? (int)q : -1;
    }
  }
  // pass 1 (branch-free): edges to pixels of the same class, ranked by (raw value, lower id)
  // through one 64-bit max of (value bits << 32 | ~partner); values are in (0, 1], so their
  // bit patterns order like the floats.
  u64 bestkey = 0;
  float diffmax = -1.0f;      // largest raw value on an edge across a class boundary
#pragma unroll
  for (int e = 0; e < 2 * OT; e++) {
    float v = val[e];
    if (CLIP) v = mn_clip(v);
    const bool live = nb[e] >= 0;
    const bool samec = live && nbc[e] == cp;
    diffmax = (live && nbc[e] != cp) ? fmaxf(diffmax, v) : diffmax;
    const u64 key = ((u64)__float_as_uint(v) << 32) | (u64)(0x7FFFFFFFu - (unsigned)nb[e]);
    const u64 cand = samec ? key : 0ull;
    bestkey = cand > bestkey ? cand : bestkey;
  }
  const float bestv = bestkey ? __uint_as_float((unsigned)(bestkey >> 32)) : -1.0f;
  const int bestq = mn_pack_partner(bestkey);
  // pass 2: edges across a class boundary (rare).  Their class delta is <= 0, so such an edge can
  // only win if its raw value is at least the best same-class value, and can only reach priority
  // >= 0 (or positive gain in later sub-rounds) above a value threshold: nearly all are skipped.
  u64 best = 0;
  const float vmin = fmaxf(bestv, FIRST ? P.vmin_first : fmaxf(P.vmin_first, 0.499f));
  if (diffmax >= vmin) {
#pragma unroll 1
    for (int e = 0; e < 2 * OT; e++) {
      const int k = e >> 1, dir = e & 1;
      const int rr = dir ? r - P.di[k] : r + P.di[k];
      const int cc = dir ? c - P.dj[k] : c + P.dj[k];
      if (!((unsigned)rr < (unsigned)P.H && (unsigned)cc < (unsigned)P.W)) continue;
      const int q = rr * P.W + cc;
      if (!FIRST && matched[q]) continue;
      const int cq = cls0[q];
      if (cq == cp) continue;
      float v = mn_ld_same(P, k, (dir ? q : p));
      if (CLIP) v = mn_clip(v);
      if (!(v >= vmin)) continue;
      bool pos;
      const int lo = min(p, q), hi = max(p, q);
      const float prio = mn_pixel_pair_prio(P, lo, hi, lo == p ? cp : cq, lo == p ? cq : cp, v, &pos);
      if (prio >= 0.0f && (FIRST || pos)) {
        const u64 key = mn_pack(prio, q);
        best = key > best ? key : best;
      }
    }
  }
  if (bestkey) {
    bool pos;
    const float prio = mn_pixel_pair_prio(P, min(p, bestq), max(p, bestq), cp, cp, bestv, &pos);
    if (prio >= 0.0f && (FIRST || pos)) {
      const u64 key = mn_pack(prio, bestq);
      best = key > best ? key : best;
    }
  }
  best_out[p] = best;
}
