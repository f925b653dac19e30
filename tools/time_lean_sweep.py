"""The sweep alone in its lean and its full form, alternating in one process (mn_sweep_time_device; debug_flags bit 9
keeps the full form):   python tools/time_lean_sweep.py [rounds]
4 input sets of 1024x2048 (C = 9, O = 10) in rotation: 638 MB, beyond the 256 MB Infinity Cache.  MN_DTYPE=bfloat16 |
float16: the 16-bit sweep (8 pixels per lane)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mergenet_amd import synth, segmenter as seg

H, W, C = 1024, 2048, 9
offs = synth.generate_offsets(40, 10)
dtype = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[os.environ.get("MN_DTYPE", "float32")]
ins = []
for i in range(4):
    im = synth.synth_v1(H, W, C, offs, 1000 + i)
    ins.append((torch.from_numpy(im.class_probs).cuda().to(dtype), torch.from_numpy(im.sameness_probs).cuda().to(dtype)))
m = seg.Merger(H, W, C, len(offs))
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
res = {"lean": [], "full": []}
for r in range(rounds):
    for name, flags in (("lean", 0), ("full", seg.MN_DEBUG_SWEEP_FULL_FORM)):
        o = seg.default_options(merge_logprob_bias=0.03, debug_flags=flags)
        res[name].append(m.sweep_time(ins, offs, o, reps=400))
nbytes = (4.0 if dtype == torch.float32 else 2.0) * (C + len(offs)) * H * W
for name in ("lean", "full"):
    print("%s %s sweep alone, back to back, alternating: %s us per launch (4 input sets in rotation) -> %.3f of 8 TB/s" % (
        os.environ.get("MN_DTYPE", "float32"), name, " ".join("%.2f" % x for x in res[name]),
        nbytes / (min(res[name]) * 1e-6) / 8e12), flush=True)
m.close()
