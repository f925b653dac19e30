#!/usr/bin/env python
"""mn_map_scores against the nearest yardsticks on the same maps.

    python tools/time_map_scores.py [--reps 50] [--repeats 5] [--variant-lib LABEL=PATH ...] [--quick]

Maps: the benchmark's generator (synth-v1, seed 1000, 1024x2048, C = 9, O = 10) in float32 and in bfloat16; the truth
is the generator's own instance mask and class list.  Each dtype is held in enough copies, used in rotation, to pass
the 256 MB Infinity Cache (4 sets of 152 MiB in float32, 6 of 76 MiB in bfloat16), each with a mask of its own.

Rows, all GPU TIME per call: the stream is first kept busy by large matmuls, then `reps` calls are queued between two
HIP events, so the GPU runs them back to back (the sweep is timed by the library the same way: mn_sweep_time_device).
    mn_map_scores        the pass of this build: every map element once, the mask through the cache
    sweep                Merger.sweep_time on the same maps: it reads the same planes and writes more -- the nearest
                         existing pass
    torch composition    what a user writes today: argmax + bincount for the confusion matrix, then
                         Merger.sameness_targets (ten float32 target planes) and products with sum(dtype=float64)
GB/s are against the byte count from the shapes, (C + O) * H * W * element size + 4 * H * W.
One warm-up round, then `repeats` rounds that alternate the rows; median (min - max) over the rounds.  Before anything
is timed the results are compared: with labels.map_scores (exact counts, sums within n_pixels * 2^-53 relative), with
the torch composition, and two calls with each other byte for byte.

--variant-lib: builds of the library with other constants of the pass (mn_kernels_mapscore.h), each timed in a child
process of its own on the same maps (a process binds one library), e.g.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DMN_MS_WORKGROUPS=512 -shared \
          mergenet_amd/csrc/mergenet_hip.hip -o build_diag/lib_ms_wg512.so
The run stops after the first child that fails.
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
    from mergenet_amd import labels, segmenter as seg, synth

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    H, W, C = (256, 512, 9) if args.quick else (1024, 2048, 9)
    offs = synth.generate_offsets(40, 10)
    O = len(offs)
    img = synth.synth_v1(H, W, C, offs, 1000)
    merger = seg.Merger(H, W, C, O)
    opts = seg.default_options(merge_logprob_bias=0.03)
    truth_np = np.ascontiguousarray(img.instances, np.int32)
    classes_np = np.asarray(img.instance_class[1:], np.int32)
    G = int(classes_np.size)
    truth_classes = torch.from_numpy(classes_np).to(dev)
    by_label = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), truth_classes.long()])
    n = H * W

    spin_a = torch.randn((8192, 8192), device=dev)

    def spin():
        for _ in range(4):
            torch.mm(spin_a, spin_a)

    def timed(fn, n_inputs, reps):
        spin()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i % n_inputs)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps                  # microseconds per call, GPU time

    for dtype in (torch.float32, torch.bfloat16):
        elem = 4 if dtype == torch.float32 else 2
        floor = (C + O) * n * elem + 4 * n
        copies = -(-320 * 2 ** 20 // ((C + O) * n * elem)) + 1
        cp0 = torch.from_numpy(img.class_probs).to(dev).to(dtype)
        sp0 = torch.from_numpy(img.sameness_probs).to(dev).to(dtype)
        sets = [(cp0.clone(), sp0.clone()) for _ in range(copies)]
        truths = [torch.from_numpy(truth_np).to(dev) for _ in range(copies)]

        def ours(i):
            return merger.map_scores(sets[i][0], sets[i][1], offs, truths[i], truth_classes)

        def composed(i):
            cp, sp = sets[i]
            pred = cp.argmax(0).reshape(-1)
            tcls = by_label[truths[i].reshape(-1).long()]
            conf = torch.bincount(tcls * C + pred, minlength=C * C).reshape(C, C)
            gd = 1 - merger.sameness_targets(truths[i], offs)
            pd = 1 - sp.float()
            return conf, torch.stack([(pd * gd).sum((1, 2), dtype=torch.float64), pd.sum((1, 2), dtype=torch.float64),
                                      gd.sum((1, 2), dtype=torch.float64)])

        got = ours(0)
        again = ours(0)
        assert got["sums"].cpu().numpy().tobytes() == again["sums"].cpu().numpy().tobytes(), "two calls differ"
        assert torch.equal(got["confusion"], again["confusion"])
        want_conf, want_sums = labels.map_scores(cp0.float().cpu().numpy(), sp0.float().cpu().numpy(), offs, truth_np,
                                                 classes_np, G)
        sums = got["sums"].cpu().numpy()
        assert np.array_equal(got["confusion"].cpu().numpy(), want_conf), "confusion matrix differs from the statement"
        assert np.array_equal(sums[2], want_sums[2])
        rel = np.abs(sums[:2] - want_sums[:2]) / np.where(want_sums[:2] > 0, want_sums[:2], 1.0)
        assert (rel <= n * 2.0 ** -53).all(), "sums differ from the statement by %g relative" % rel.max()
        t_conf, t_sums = composed(0)
        assert torch.equal(t_conf, got["confusion"]), "confusion matrix differs from the torch composition"
        t_rel = (np.abs(t_sums.cpu().numpy() - want_sums) / np.where(want_sums > 0, want_sums, 1.0)).max()
        assert t_rel <= n * 2.0 ** -53, "the torch composition differs from the statement by %g relative" % t_rel
        _, iou = labels.class_scores(want_conf)
        print("[%s] %s %dx%d, C = %d, O = %d, G = %d; %d sets in rotation (%.0f MB); equal to the statement (sums "
              "within %.2g relative, bound %.2g; torch composition within %.2g); mean IoU of the classes %.4f, of the "
              "offsets %.4f" % (tag, str(dtype).replace("torch.", ""), H, W, C, O, G, copies,
                               copies * (C + O) * n * elem / 2 ** 20, rel.max(), n * 2.0 ** -53, t_rel,
                               float(np.nanmean(iou)), labels.offset_iou(want_sums)[1]), flush=True)

        rows = ["mn_map_scores                          ", "sweep (Merger.sweep_time) on these maps",
                "torch: argmax+bincount, targets, sums  "]
        times = {r: [] for r in rows}
        for rnd in range(args.repeats + 1):                      # round 0 warms up
            us = [timed(ours, copies, args.reps), merger.sweep_time(sets, offs, opts, reps=args.reps),
                  timed(composed, copies, max(2, args.reps // 5))]
            if rnd:
                for r, u in zip(rows, us):
                    times[r].append(u)
        for r in rows:
            t = times[r]
            med = statistics.median(t)
            print("  %s %9.2f us per call (min %.2f max %.2f over %d rounds)  %7.0f GB/s of the %.0f MB floor" %
                  (r, med, min(t), max(t), len(t), floor / med * 1e-3, floor / 1e6), flush=True)
        del sets, truths
        torch.cuda.empty_cache()
    merger.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="256x512 instead of 1024x2048")
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
        res = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, timeout=500)
        if res.returncode != 0:                              # nothing more on the GPU after a failure
            print("%s: exit status %d" % (tag, res.returncode), flush=True)
            return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
