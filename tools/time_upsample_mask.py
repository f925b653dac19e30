#!/usr/bin/env python
"""mn_upsample_mask at 512x1024 -> 1024x2048 (2 MiB read, 8 MiB written), this build against a build of another commit.

    python tools/time_upsample_mask.py [--parent-lib PATH] [--runs 3] [--reps 200] [--repeats 5]

The kernel takes cv2's INTER_NEAREST index in double (one product and one floor per axis and lane; the two scale
factors come from the host).  --parent-lib: a build of the commit before, which took the index in float32, e.g.
    git archive HEAD~1 mergenet_amd/csrc include | tar -x -C build_diag/parent
    make -C build_diag/parent/mergenet_amd/csrc ../libmergenet_hip.so
The two builds are timed alternately, `runs` times each, every run in a child process of its own (a process binds one
library): parent, this build, parent, this build, ...  The run stops after the first child that fails.

A run: GPU TIME per call -- the stream is first kept busy by large matmuls, then `reps` calls are queued between two
HIP events, so the GPU runs them back to back; the result goes to 40 output buffers in rotation (320 MB: beyond the
Infinity Cache), the 2 MiB source stays the same.  One warm-up round, then `repeats` rounds; median (min max).  Before
anything is timed the result is compared with resize.upsample_mask (this build) or only reported (the other build:
at this size pair the float32 and the double index agree everywhere, so both are expected to be equal to it).
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (512, 1024, 1024, 2048)


def child(args):
    tag = os.environ.get("MN_TAG", "this build")

    import numpy as np
    import torch
    from mergenet_amd import resize, segmenter as seg

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    Hin, Win, Ho, Wo = SHAPE
    merger = seg.Merger(Hin, Win, 2, 2)
    lib = merger.lib
    src = np.arange(Hin * Win, dtype=np.int32).reshape(Hin, Win)
    d_src = torch.from_numpy(src).to(dev)
    copies = 40
    outs = [torch.empty((Ho, Wo), dtype=torch.int32, device=dev) for _ in range(copies)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    spin_a = torch.randn((8192, 8192), device=dev)

    def call(i):
        rc = lib.mn_upsample_mask_device(merger.handle, d_src.data_ptr(), Hin, Win, outs[i % copies].data_ptr(), Ho, Wo,
                                         stream)
        assert rc == 0

    def gpu_time(reps):
        for _ in range(4):
            torch.mm(spin_a, spin_a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps                # microseconds per call, GPU time

    call(0)
    equal = bool(np.array_equal(outs[0].cpu().numpy(), resize.upsample_mask(src, Ho, Wo)))
    assert equal or os.environ.get("MN_LIB"), "this build differs from resize.upsample_mask"
    times = [gpu_time(args.reps) for _ in range(args.repeats + 1)][1:]      # round 0 warms up
    t = statistics.median(times)
    print("[%-10s] mn_upsample_mask %dx%d -> %dx%d %8.2f us per call (min %.2f max %.2f over %d rounds of %d calls), "
          "%.0f GB/s of source + result; equal to the cv2 statement: %s" %
          (tag, Hin, Win, Ho, Wo, t, min(times), max(times), len(times), args.reps,
           (Hin * Win + Ho * Wo) * 4 / t / 1e3, "yes" if equal else "NO"), flush=True)
    merger.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if os.environ.get("MN_CHILD"):
        return child(args)
    order = ([("parent", args.parent_lib)] if args.parent_lib else []) + [("this build", "")]
    for _ in range(args.runs):
        for tag, lib in order:
            env = dict(os.environ, MN_CHILD="1", MN_TAG=tag)
            env.pop("MN_LIB", None)
            if lib:
                env["MN_LIB"] = os.path.abspath(lib)
            res = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, timeout=120)
            if res.returncode != 0:                          # nothing more on the GPU after a failure
                print("%s: exit status %d" % (tag, res.returncode), flush=True)
                return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
