#!/usr/bin/env python
"""mn_instance_table / filter_instances against what a user composes from stock PyTorch ops on the same masks.

    python tools/time_instance_table.py [--reps 100] [--repeats 5] [--variant-lib LABEL=PATH ...] [--quick]

Masks: (a) the 1024x2048 mask the default path gives for the benchmark's generator (synth-v1, seed 1000, C = 9,
O = 10, opts 0/1/0.03); (b) the worst case for any per-run scheme, every pixel its own label (a random
permutation), at 256x512: K = 131072, runs of length 1, nearly every label beyond the LDS table.  Each mask is
held in `copies` buffers used in rotation (more than 256 MB in all for (a): beyond the Infinity Cache).

Yardstick (the table): torch.bincount for the areas, four scatter_reduce (amin / amax) for the boxes, on an
int64 copy of the labels (both ops want one); the x / y coordinate tensors are made once, outside the clock.
Yardstick (the filter): a cumsum over the kept labels, remap[mask] and boolean compaction of table and classes,
K' read on the host -- one synchronisation, as in Merger.filter_instances.

TWO KINDS OF FIGURE, not to be compared with each other.  "table" rows: the stream is first kept busy by large
matmuls, then `reps` calls are queued between two HIP events, so the GPU runs them back to back and the figure is
GPU time per call.  "filter" rows: every call ends in a host synchronisation (K'), so nothing can be queued and
the figure is the time of a call as the host sees it, launch and read-back latency included.  One warm-up
round, then `repeats` rounds of `reps` calls (5 for the torch table) that alternate the rows; median (min - max) over the rounds.  Results are compared
before anything is timed.

--variant-lib: builds of the library with other constants of the pass (mn_kernels_instances.h), each timed in a
child process of its own on the same masks (a process binds one library), e.g.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DMN_INST_LDS_LABELS=0 -shared \
          mergenet_amd/csrc/mergenet_hip.hip -o build_diag/lib_inst_no_lds.so
for the simpler form (every run straight to the global table), or -DMN_INST_WORKGROUPS=n for the launch shape.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    tag = os.environ.get("MN_TAG", "this build")

    import numpy as np
    import torch
    from mergenet_amd import segmenter as seg, synth

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    H, W, C = (256, 512, 9) if args.quick else (1024, 2048, 9)
    offs = synth.generate_offsets(40, 10)
    img = synth.synth_v1(H, W, C, offs, 1000)
    merger = seg.Merger(H, W, C, len(offs))
    opts = seg.default_options(same_different_bias=0.0, object_merge_factor=1.0, merge_logprob_bias=0.03,
                               require_proof=seg.MN_PROVE_NEVER)
    mask, classes, _, st = merger.segment(torch.from_numpy(img.class_probs).to(dev),
                                          torch.from_numpy(img.sameness_probs).to(dev), offs, opts)
    K = st["num_instances"]
    hw, ww = 256, 512
    worst = torch.from_numpy((np.random.default_rng(8).permutation(hw * ww) + 1).astype(np.int32).reshape(hw, ww)).to(dev)
    cases = [("default path, seed 1000, %dx%d, K = %d" % (H, W, K), mask, classes[:K].contiguous(), K),
             ("every pixel its own label, %dx%d, K = %d" % (hw, ww, hw * ww), worst,
              (torch.arange(hw * ww, device=dev, dtype=torch.int32) % 8 + 1), hw * ww)]

    spin_a = torch.randn((8192, 8192), device=dev)

    def spin():
        for _ in range(4):
            torch.mm(spin_a, spin_a)

    def timed(fn, n_inputs, reps, queued=True):
        if queued:
            spin()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i % n_inputs)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps                 # microseconds per call

    for title, m0, cls, k in cases:
        h, w = m0.shape
        copies = max(2, min(64, -(-320 * 2 ** 20 // (m0.numel() * 4))))
        masks = [m0.clone() for _ in range(copies)]
        xs = torch.arange(w, device=dev, dtype=torch.int32).repeat(h)
        ys = torch.arange(h, device=dev, dtype=torch.int32).repeat_interleave(w)

        def torch_table(i):
            idx = masks[i].reshape(-1).to(torch.int64)
            area = torch.bincount(idx, minlength=k + 1)
            x0 = torch.full((k + 1,), w, dtype=torch.int32, device=dev).scatter_reduce(0, idx, xs, "amin")
            y0 = torch.full((k + 1,), h, dtype=torch.int32, device=dev).scatter_reduce(0, idx, ys, "amin")
            x1 = torch.full((k + 1,), -1, dtype=torch.int32, device=dev).scatter_reduce(0, idx, xs, "amax")
            y1 = torch.full((k + 1,), -1, dtype=torch.int32, device=dev).scatter_reduce(0, idx, ys, "amax")
            return area, x0, y0, x1, y1

        def our_table(i):
            return merger.instance_table(masks[i], k)

        table = our_table(0)
        area, x0, y0, x1, y1 = torch_table(0)
        want = torch.stack([area[1:k + 1].to(torch.int32), x0[1:], y0[1:], x1[1:], y1[1:]], 1)
        assert torch.equal(table, want), "the two routes disagree"
        areas = table[:, 0]
        min_area = max(2, int(areas.float().median().item()))

        def torch_filter(i):
            keep = table[:, 0] >= min_area
            remap = torch.zeros((k + 1,), dtype=torch.int32, device=dev)
            remap[1:] = torch.where(keep, torch.cumsum(keep, 0).to(torch.int32), 0)
            new_mask = remap[masks[i].to(torch.int64)]
            new_table, new_cls = table[keep], cls[keep]                  # boolean compaction: synchronises
            return new_mask, new_table, new_cls, int(new_table.shape[0])

        def our_filter(i):
            return merger.filter_instances(masks[i], cls, k, min_area=min_area, table=table)

        a, b = torch_filter(0), our_filter(0)
        assert b[4] == a[3] and torch.equal(b[0], a[0]) and torch.equal(b[3], a[1]) and torch.equal(b[1][:b[4]], a[2])

        forms = [("table  torch: bincount + 4 scatter_reduce     (GPU time)  ", torch_table, True),
                 ("table  mn_instance_table                      (GPU time)  ", our_table, True),
                 ("filter torch: cumsum, remap[mask], table[keep] (host time)", torch_filter, False),
                 ("filter Merger.filter_instances, table given    (host time)", our_filter, False)]
        times = {name: [] for name, _, _ in forms}
        for rnd in range(args.repeats + 1):                              # round 0 warms up
            for name, fn, queued in forms:
                # (the torch table takes a third of a second per call on mask (a): a few calls are a long window)
                us = timed(fn, copies, min(args.reps, 5) if fn is torch_table else args.reps, queued)
                if rnd:
                    times[name].append(us)
        print("[%s] %s; %d copies of the mask in rotation (%.0f MB); min_area = %d" %
              (tag, title, copies, copies * m0.numel() * 4 / 2 ** 20, min_area), flush=True)
        for name, _, _ in forms:
            t = times[name]
            print("  %s %9.2f us per call (min %.2f max %.2f over %d rounds)" %
                  (name, statistics.median(t), min(t), max(t), len(t)), flush=True)
    merger.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="256x512 instead of 1024x2048 for mask (a)")
    ap.add_argument("--variant-lib", action="append", default=[], metavar="LABEL=PATH")
    args = ap.parse_args()
    if os.environ.get("MN_CHILD"):
        return child(args)
    runs = [("this build", "")] + [tuple(v.split("=", 1)) for v in args.variant_lib]
    for tag, lib in runs:
        env = dict(os.environ, MN_CHILD="1", MN_TAG=tag)
        env.pop("MN_LIB", None)
        if lib:
            env["MN_LIB"] = os.path.abspath(lib)
        res = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, timeout=280)
        if res.returncode != 0:                              # nothing more on the GPU after a failure
            print("%s: exit status %d" % (tag, res.returncode), flush=True)
            return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
