#!/usr/bin/env python
"""The sweep alone (mn_sweep_time_device_t) by element type of the maps and by form of the 16-bit sweep.

    python tools/sweep_dtype.py [--parent-lib PATH] [--reps 400] [--repeats 5]

1024x2048, C = 9, O = 10 (MN_H, MN_W: another shape), synth-v1 seeds 1000-1003 quantised, the four input sets
in rotation (319 MB in 16 bits, 638 MB in float32: beyond the 256 MB Infinity Cache), one warm-up round, then
`repeats` rounds that alternate: float32 sweep, and for float16 and bfloat16 each form of the sweep -- 8 pixels
per lane with one 16-byte load per plane, 4 pixels per lane with 8-byte loads (debug_flags bit 8).  The float32
maps are the widened float16 ones; they are timed as production runs them (no clip) and clipped on load as the
16-bit maps always are, the form that sees the same values through the same arithmetic.  Prints microseconds
per launch (median, min-max over the repeats), the algorithmic bytes read and the fraction of 8 TB/s.

--parent-lib: a build of the parent commit's library (it has no typed entry points); its float32 sweep is timed
on the same inputs in a fresh child process (a process binds one library) before and after this build's.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inputs(H, W, C, offs):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lowp_util
    from mergenet_amd import synth
    sets = {"float32": [], "float16": [], "bfloat16": []}
    for seed in range(1000, 1004):
        im = synth.synth_v1(H, W, C, offs, seed)
        for dtype in ("float16", "bfloat16"):
            cb, _ = lowp_util.quantize(im.class_probs, dtype)
            sb, _ = lowp_util.quantize(im.sameness_probs, dtype)
            pair = (lowp_util.to_torch(cb, dtype, "cuda"), lowp_util.to_torch(sb, dtype, "cuda"))
            sets[dtype].append(pair)
            if dtype == "float16":
                sets["float32"].append((pair[0].float().contiguous(), pair[1].float().contiguous()))
    return sets


def child(args):
    sys.path.insert(0, ROOT)
    from mergenet_amd import segmenter as seg, synth
    H, W, C = int(os.environ.get("MN_H", 1024)), int(os.environ.get("MN_W", 2048)), 9
    offs = synth.generate_offsets(40, 10)
    sets = inputs(H, W, C, offs)
    m = seg.Merger(H, W, C, len(offs))
    tag = os.environ.get("MN_TAG", "this build")
    typed = hasattr(m.lib, "mn_sweep_time_device_t")
    # (float32 twice: as production runs it, without the clip, and clipped on load as a 16-bit map always is)
    forms = [("float32", "4 px / 16-byte loads         ", 0, 0), ("float32", "4 px / 16-byte loads, clipped", 0, 1)]
    if typed:
        for dtype in ("float16", "bfloat16"):
            forms.append((dtype, "8 px / 16-byte loads, clipped", 0, 0))
            forms.append((dtype, "4 px /  8-byte loads, clipped", seg.MN_DEBUG_SWEEP16_4PX, 0))
    times = {f: [] for f in forms}
    for rep in range(args.repeats + 1):                      # round 0 warms up
        for f in forms:
            dtype, _, flags, clip = f
            o = seg.default_options(merge_logprob_bias=0.03, clip_inputs=clip, debug_flags=flags)
            us = m.sweep_time(sets[dtype], offs, o, reps=args.reps)
            if rep:
                times[f].append(us)
    for f in forms:
        dtype, form, _, _ = f
        t = times[f]
        nbytes = (4.0 if dtype == "float32" else 2.0) * (C + len(offs)) * H * W
        med = statistics.median(t)
        print("%-12s %-9s %s: %7.2f us per launch (min %.2f max %.2f over %d repeats of %d launches)  "
              "%.1f MB read -> %.3f of 8 TB/s" % (tag, dtype, form, med, min(t), max(t), len(t), args.reps,
                                                  nbytes / 1e6, nbytes / (med * 1e-6) / 8e12), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if os.environ.get("MN_CHILD"):
        child(args)
        return 0
    runs = [("this build", "")]
    if args.parent_lib:
        runs = [("parent", args.parent_lib), ("this build", ""), ("parent", args.parent_lib)]
    for tag, lib in runs:
        env = dict(os.environ, MN_CHILD="1", MN_TAG=tag)
        env.pop("MN_LIB", None)
        if lib:
            env["MN_LIB"] = os.path.abspath(lib)
        res = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, timeout=420)
        if res.returncode != 0:                              # nothing more on the GPU after a failure
            print("%s: exit status %d" % (tag, res.returncode), flush=True)
            return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
