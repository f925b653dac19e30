// mn_sweep_form.h -- the form of one launch of the sweep (mn_cc_sign), decided once, on the host, from plain values.
//
// Host only, no HIP: mn_kernels_cc.h includes it for LeanOut and the block size, the host launches what
// sweep_form returns, and tests/tools/sweep_form_check.cpp compiles it with g++ alone (tests/test_sweep_form.py).
#pragma once
#include <stddef.h>

#include "../../include/mergenet_hip.h"

#define MN_CC_SIGN_THREADS 256

// Where the lean form's outputs lie (what they are: "LEAN" in mn_kernels_cc.h).  {-1, 0, 0, 0}: not the lean form.
struct LeanOut { int kh; int packed; int rec0; int flag0; };

// The unit offsets (0, +1) and (+-1, 0), first of each in the list, if it has them (generate_offsets always does):
// the tile and border stages of the labelling take them, and `kh` marks the lean form's uniform groups.
struct UnitOffsets { int kh, kv, dv; };
static inline UnitOffsets unit_offsets(const int* di, const int* dj, int O) {
  UnitOffsets u = {-1, -1, 0};
  for (int k = 0; k < O; k++) {
    if (u.kh < 0 && di[k] == 0 && dj[k] == 1) u.kh = k;
    if (u.kv < 0 && dj[k] == 0 && (di[k] == 1 || di[k] == -1)) { u.kv = k; u.dv = di[k]; }
  }
  return u;
}

enum SweepAsker {
  SWEEP_COMPONENTS,   // the pure components path: mn_cc_sums(_lean) and mn_cc_cross are the only readers
  SWEEP_CORES,        // first step of the general rounds: the rounds read the full form
  SWEEP_EXPORT,       // mn_sweep_device: the full form is what it hands out
  SWEEP_TIMING        // mn_sweep_time_device: as the pure components path launches it
};

struct SweepForm {
  int px;             // pixels per lane: 1, 4 or 8
  bool cls;           // the lane takes the class planes too
  bool lean_cls;      // ... and leaves the roots' class and validity flag to mn_cc_finish
  bool lean_form;     // packed masks where O <= 16, one record per uniform group of 64 pixels (LO)
  bool plain;         // no clip beyond the loader's own and no same_different_bias: mn_cc_value
  LeanOut LO;
  unsigned blocks;    // of MN_CC_SIGN_THREADS lanes
  int waves;          // one partial sum each (the tail and the certificate add them up)
};

// px.  4 whenever the planes stay aligned for a lane's one load per plane (N % 4 == 0): with W % 4 != 0 one lane per
// row runs over the row's end (mn_cc_sign: `straddle`; W >= 4: its four pixels then span at most two rows, which is
// what mn_cc_sign assumes), else 1.  A 16-bit map takes 8 -- one 16-byte load per plane, as the float32 map's 4 --
// where N % 8 == 0, W % 8 == 0 (no lane runs over a row's end) and the planes are 16-byte aligned (`aligned16`: both
// maps); MN_DEBUG_SWEEP16_4PX keeps it at 4 (8-byte loads).  What the sweep leaves is laid out per 4 pixels either way.
// cls: only where a lane's pixels are whole pixels of the image, px >= 4.
// lean_form: the product path; MN_DEBUG_SWEEP_FULL_FORM keeps the full form there (the yardstick inside one build);
// so does an image too small for the records to fit into the free part of the `lpsum` planes.
// plain: a 16-bit map is always clipped on load, its plain form is the clip alone; logits likewise (sigmoid + clip).
static inline SweepForm sweep_form(int N, int W, int O, const int* di, const int* dj, int dtype, bool logits, bool clip,
                                   float sdb, bool aligned16, int debug_flags, SweepAsker who) {
  SweepForm F;
  if (!((N & 3) == 0 && W >= 4)) F.px = 1;
  else if (dtype != MN_DTYPE_F32 && !(debug_flags & MN_DEBUG_SWEEP16_4PX) && (N & 7) == 0 && (W & 7) == 0 && aligned16) F.px = 8;
  else F.px = 4;
  F.cls = F.px >= 4;
  F.lean_cls = F.cls && (who == SWEEP_COMPONENTS || who == SWEEP_TIMING);
  F.lean_form = F.lean_cls && !(debug_flags & MN_DEBUG_SWEEP_FULL_FORM) && N >= 64;
  F.LO = LeanOut{-1, 0, 0, 0};
  if (F.lean_form) {
    F.LO.kh = unit_offsets(di, dj, O).kh;
    F.LO.packed = O <= 16 ? 1 : 0;
    F.LO.rec0 = (N / 4 + 1) & ~1;                     // (i64 records: an even int index behind the per-lane values)
    F.LO.flag0 = F.LO.rec0 + 2 * ((N + 63) / 64);     // (the groups' words of plane 0 behind its records)
  }
  F.plain = (dtype != MN_DTYPE_F32 || logits || !clip) && sdb == 0.0f;
  F.blocks = (unsigned)(((size_t)(N / F.px) + MN_CC_SIGN_THREADS - 1) / MN_CC_SIGN_THREADS);
  F.waves = (int)(F.blocks * (MN_CC_SIGN_THREADS / 64));
  return F;
}
