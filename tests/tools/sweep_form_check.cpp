// Host shim of mn_sweep_form.h for tests/test_sweep_form.py: the header the library decides the sweep's form with,
// compiled by g++ alone.
#include "../../mergenet_amd/csrc/mn_sweep_form.h"

// offs: [O][2] as (di, dj).  out[14]: px, cls, lean_cls, lean_form, plain, LO.kh, LO.packed, LO.rec0, LO.flag0,
// blocks, waves, then unit_offsets' kh, kv, dv.
extern "C" void sweep_form_check(int N, int W, int O, const int* offs, int dtype, int logits, int clip, float sdb,
                                 int aligned16, int debug_flags, int who, int* out) {
  int di[MN_MAX_OFFSETS], dj[MN_MAX_OFFSETS];
  for (int k = 0; k < O; k++) { di[k] = offs[2 * k]; dj[k] = offs[2 * k + 1]; }
  const SweepForm F = sweep_form(N, W, O, di, dj, dtype, logits != 0, clip != 0, sdb, aligned16 != 0, debug_flags,
                                 static_cast<SweepAsker>(who));
  const UnitOffsets u = unit_offsets(di, dj, O);
  const int v[14] = {F.px, F.cls, F.lean_cls, F.lean_form, F.plain, F.LO.kh, F.LO.packed, F.LO.rec0, F.LO.flag0,
                     (int)F.blocks, F.waves, u.kh, u.kv, u.dv};
  for (int i = 0; i < 14; i++) out[i] = v[i];
}
