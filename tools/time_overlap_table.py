#!/usr/bin/env python
"""mn_overlap_table / match_instances against the nearest yardsticks on the same masks.

    python tools/time_overlap_table.py [--reps 100] [--repeats 5] [--variant-lib LABEL=PATH ...] [--quick]

Masks: (a) the 1024x2048 mask the default path gives for the benchmark's generator (synth-v1, seed 1000, C = 9,
O = 10, opts 0/1/0.03) against the generator's own ground-truth instance mask; (b) the worst case for any per-run
scheme, every pixel its own prediction label (a random permutation) against nine blobs in the truth, at 256x512:
K = 131072, runs of length 1, nearly every pair beyond any LDS table; (c), for the matching alone, 4096 instances
on either side (the capacity) at 256x512.  Each mask is held in `copies` buffers used in rotation (more than 256 MB
per side for (a): beyond the Infinity Cache).

Rows.  "table" rows are GPU TIME per call: the stream is first kept busy by large matmuls, then `reps` calls are
queued between two HIP events, so the GPU runs them back to back.
    mn_overlap_table                  the pass over both masks, in the form this build holds (MN_OVL_LDS_DIM)
    mn_instance_table                 on the prediction mask alone: half the bytes, the nearest existing pass
    torch.bincount                    what a user composes today:
                                      torch.bincount(pred.long() * (G + 1) + truth.long(), minlength=(K + 1) * (G + 1))
The "match" row is HOST-VISIBLE TIME per call, not to be compared with the rows above: Merger.match_instances at
the ten COCO thresholds with IoUs, the enqueue plus ONE synchronisation, so launch latency is in it.
One warm-up round, then `repeats` rounds of `reps` calls (10 for torch.bincount) that alternate the rows; median (min - max) over the
rounds.  Results are compared (with torch.bincount and with labels.match_instances) before anything is timed.

--variant-lib: builds of the library with another form of the pass (mn_kernels_match.h), each timed in a child
process of its own on the same masks (a process binds one library), e.g.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DMN_OVL_LDS_DIM=0 -shared \
          mergenet_amd/csrc/mergenet_hip.hip -o build_diag/lib_ovl_no_lds.so
for the simpler form (one global atomicAdd per run).  The run stops after the first child that fails.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

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
    img = synth.synth_v1(H, W, C, offs, 1000)
    merger = seg.Merger(H, W, C, len(offs))
    opts = seg.default_options(same_different_bias=0.0, object_merge_factor=1.0, merge_logprob_bias=0.03,
                               require_proof=seg.MN_PROVE_NEVER)
    mask, classes, _, st = merger.segment(torch.from_numpy(img.class_probs).to(dev),
                                          torch.from_numpy(img.sameness_probs).to(dev), offs, opts)
    K = st["num_instances"]
    truth = torch.from_numpy(np.ascontiguousarray(img.instances, np.int32)).to(dev)
    truth_classes = torch.tensor(img.instance_class[1:], dtype=torch.int32, device=dev)
    G = int(truth_classes.numel())

    hw, ww = 256, 512
    rng = np.random.default_rng(8)
    worst = torch.from_numpy((rng.permutation(hw * ww) + 1).astype(np.int32).reshape(hw, ww)).to(dev)
    blobs = np.zeros((hw, ww), np.int32)
    for k in range(1, 10):
        y, x = rng.integers(0, hw), rng.integers(0, ww)
        blobs[max(0, y - hw // 6):y + hw // 6 + 1, max(0, x - ww // 6):x + ww // 6 + 1] = k
    blobs = torch.from_numpy(blobs).to(dev)

    cells = (np.arange(hw)[:, None] // 4) * (ww // 8) + np.arange(ww)[None, :] // 8 + 1      # 64 x 64 cells of 4 x 8
    full_t = torch.from_numpy(cells.astype(np.int32)).to(dev)
    full_p = torch.from_numpy(np.roll(cells, 1, 1).astype(np.int32)).to(dev)
    cap = seg.MN_MATCH_MAX_INSTANCES
    assert int(cells.max()) == cap

    # title, prediction, truth, K, G, prediction classes, truth classes, table timed, matching timed
    cases = [("default path against the generator's truth, seed 1000, %dx%d, K = %d, G = %d" % (H, W, K, G),
              mask, truth, K, G, classes[:K].contiguous(), truth_classes, True, True),
             ("every pixel its own prediction label against nine blobs, %dx%d, K = %d, G = 9" % (hw, ww, hw * ww),
              worst, blobs, hw * ww, 9, None, None, True, False),
             ("%d instances on either side (the matching's capacity), %dx%d" % (cap, hw, ww), full_p, full_t, cap, cap,
              (torch.arange(cap, device=dev, dtype=torch.int32) % 3 + 1),
              (torch.arange(cap, device=dev, dtype=torch.int32) % 3 + 1), False, True)]

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
            return e0.elapsed_time(e1) * 1e3 / reps             # microseconds per call, GPU time
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(reps):
            fn(i % n_inputs)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / reps          # microseconds per call as the host sees it

    for title, p0, t0_, k, g, pcls, tcls, time_table, time_match in cases:
        copies = max(2, min(64, -(-320 * 2 ** 20 // (p0.numel() * 4))))
        preds = [p0.clone() for _ in range(copies)]
        truths = [t0_.clone() for _ in range(copies)]

        def our_overlap(i):
            return merger.overlap_table(preds[i], truths[i], k, g)

        def our_instance(i):
            return merger.instance_table(preds[i], k)

        def torch_overlap(i):
            return torch.bincount(preds[i].reshape(-1).long() * (g + 1) + truths[i].reshape(-1).long(),
                                  minlength=(k + 1) * (g + 1))

        table = our_overlap(0)
        assert torch.equal(table.reshape(-1), torch_overlap(0).to(torch.int32)), "the two routes disagree"
        assert int(table.sum().item()) == p0.numel()
        forms = []
        if time_table:
            forms += [("table  mn_overlap_table, both masks             (GPU time) ", our_overlap, True),
                      ("table  mn_instance_table, the prediction alone  (GPU time) ", our_instance, True),
                      ("table  torch.bincount of pred * (G + 1) + truth (GPU time) ", torch_overlap, True)]
        if time_match:
            def our_match(i):
                return merger.match_instances(table, pcls, tcls, return_iou=True)

            got = our_match(0)
            want = labels.match_instances(table.cpu().numpy(), pcls.cpu().numpy(), tcls.cpu().numpy())
            assert got["iou"].cpu().numpy().tobytes() == want["iou"].tobytes(), "IoU differs from the numpy statement"
            for key in ("pred_match", "truth_match", "pred_ignore", "truth_ignore"):
                assert np.array_equal(got[key].cpu().numpy(), want[key]), key
            matched = int((want["pred_match"][0] > 0).sum())
            forms += [("match  Merger.match_instances, 10 thresholds, IoU (host time)", our_match, False)]
        times = {name: [] for name, _, _ in forms}
        for rnd in range(args.repeats + 1):                              # round 0 warms up
            for name, fn, queued in forms:
                # (torch.bincount serialises on a few addresses: a few calls are a long window already)
                us = timed(fn, copies, min(args.reps, 10) if fn is torch_overlap else args.reps, queued)
                if rnd:
                    times[name].append(us)
        print("[%s] %s; %d copies of each mask in rotation (%.0f MB per side)%s" %
              (tag, title, copies, copies * p0.numel() * 4 / 2 ** 20,
               "; %d detections matched at 0.5" % matched if time_match else ""), flush=True)
        for name, _, _ in forms:
            t = times[name]
            print("  %s %9.2f us per call (min %.2f max %.2f over %d rounds)" %
                  (name, statistics.median(t), min(t), max(t), len(t)), flush=True)
        if not time_match:
            print("  match  not timed: K is above the matching's capacity of %d" % cap, flush=True)
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
        res = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, timeout=500)
        if res.returncode != 0:                              # nothing more on the GPU after a failure
            print("%s: exit status %d" % (tag, res.returncode), flush=True)
            return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
