#!/usr/bin/env python
"""Merger.dataset_eval -- add per image, accumulate at the end -- against the same evaluation done on the host.

    python tools/time_dataset_eval.py [--load cityscapes|coco|both] [--repeats 3] [--quick]

Loads (overlap tables drawn directly: most detections share 5-39 pixels with one truth instance; scores are
distinct float32 values, so no order depends on ties):
    cityscapes   500 images x 60 detections, 30 truth instances, C = 9    (a Cityscapes-val-like pass)
    coco         5000 images x 100 detections, 20 truth instances, C = 81 (a COCO-val-like pass)
COCO's ten thresholds, four area ranges (scaled to the tables' areas), maxDets (1, 10, 100), 101 recall thresholds.

Rows, per load:
    add, GPU time          N adds queued behind a busy stream between two events: what the device spends per image
    add, one area range    the same with a single area range: the difference is three more matchings
    add, host time         host clock around the N calls without a synchronisation: what the loop pays per image
    accumulate             events around keys / sort / scan, and the host clock around accumulate() + synchronise
    host route             per image: Merger.match_instances once per area range, its arrays copied to the host
                           (one synchronisation per image); at the end labels.coco_accumulate(form="closed") on those
The host route's arrays are compared with the device's (np.array_equal) before its times are printed.  Median
(min - max) over `repeats` rounds after one warm-up round; the host route runs once.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AREA_RANGES = [(0.0, 1e10), (0.0, 20.0), (20.0, 40.0), (40.0, 1e10)]
LOADS = {"cityscapes": (500, 60, 30, 9), "coco": (5000, 100, 20, 81)}


def tables(np, rng, count, K, G):
    t = np.zeros((count, K + 1, G + 1), np.int32)
    t[:, 0, 0] = 50
    t[:, 1:, 0] = rng.integers(1, 10, (count, K))
    t[:, 0, 1:] = rng.integers(0, 10, (count, G))
    paired = rng.random((count, K)) < 0.7
    j = rng.integers(1, G + 1, (count, K))
    n = rng.integers(5, 40, (count, K))
    i, k = np.nonzero(paired)
    t[i, k + 1, j[i, k]] += n[i, k]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--load", default="both", choices=["cityscapes", "coco", "both"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a tenth of the images")
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from mergenet_amd import labels, segmenter as seg

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    merger = seg.Merger(64, 128, 9, 10)
    spin_a = torch.randn((8192, 8192), device=dev)

    def med(v):
        return "%10.1f us (min %.1f max %.1f)" % (statistics.median(v), min(v), max(v))

    for name in (["cityscapes", "coco"] if args.load == "both" else [args.load]):
        N, K, G, C = LOADS[name]
        if args.quick:
            N //= 10
        rng = np.random.default_rng(31)
        pool = 64
        tab = tables(np, rng, pool, K, G)
        pcls = rng.integers(1, C, (pool, K)).astype(np.int32)
        # a truth instance has the class of the detection that covers it best
        tcls = np.stack([pcls[p][np.argmax(tab[p, 1:, 1:], axis=0)] for p in range(pool)]).astype(np.int32)
        crowd = (rng.random((pool, G)) < 0.05).astype(np.uint8)
        scores = (rng.permutation(N * K).astype(np.float32) / np.float32(N * K)).reshape(N, K)
        d_tab = [torch.from_numpy(tab[p]).to(dev) for p in range(pool)]
        d_pcls, d_tcls, d_crowd = (torch.from_numpy(a).to(dev) for a in (pcls, tcls, crowd))
        d_scores = torch.from_numpy(scores).to(dev)

        def run_adds(ev):
            for i in range(N):
                p = i % pool
                ev.add(d_tab[p], d_pcls[p], d_tcls[p], d_scores[i], d_crowd[p])

        ev = merger.dataset_eval(C, area_ranges=AREA_RANGES, capacity=N * K)
        ev1 = merger.dataset_eval(C, area_ranges=AREA_RANGES[:1], capacity=N * K)
        gpu, gpu1, host = [], [], []
        for rnd in range(args.repeats + 1):
            for e, out in ((ev, gpu), (ev1, gpu1)):
                e.reset()
                for _ in range(4):
                    torch.mm(spin_a, spin_a)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run_adds(e)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    out.append(e0.elapsed_time(e1) * 1e3 / N)
            ev.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_adds(ev)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if rnd:
                host.append((t1 - t0) * 1e6 / N)
        # accumulate: the three steps between events, and the call as a user makes it
        T, R, A, M = len(ev.thresholds), len(ev.rec_thresholds), len(ev.area_ranges), len(ev.max_dets)
        steps = {"keys": [], "sort": [], "scan": [], "call": []}
        for rnd in range(args.repeats + 1):
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            raw = torch.empty((ev.num_records,), dtype=torch.int64, device=dev)
            out = [torch.empty(s, dtype=torch.float64, device=dev) for s in ((T, R, C, A, M), (T, C, A, M), (T, R, C, A, M))]
            torch.cuda.synchronize()
            marks[0].record()
            assert ev._keys(merger.handle, ev._log.data_ptr(), ev.num_records, C, raw.data_ptr(), None) == 0
            marks[1].record()
            keys, index = torch.sort(raw, stable=True)
            marks[2].record()
            assert ev._accumulate(merger.handle, ev._log.data_ptr(), ev.num_records, keys.data_ptr(), index.data_ptr(),
                                  ev._npig.data_ptr(), C, T, ev._rec_dev.data_ptr(), R, A, ev._max_dets_c, M,
                                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None) == 0
            marks[3].record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = ev.accumulate()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert torch.equal(result["recall"], out[1])
            if rnd:
                for key, a, b in (("keys", 0, 1), ("sort", 1, 2), ("scan", 2, 3)):
                    steps[key].append(marks[a].elapsed_time(marks[b]) * 1e3)
                steps["call"].append((t1 - t0) * 1e6)
        summary = ev.summarize(result)
        print("[%s] %d images x %d detections, %d truth instances, C = %d: %d records; AP %.4f AP50 %.4f AR@100 %.4f"
              % (name, N, K, G, C, ev.num_records, summary["AP"], summary["AP50"], summary["AR@100"]), flush=True)
        print("  add, GPU time per image (4 area ranges)        %s" % med(gpu))
        print("  add, GPU time per image (1 area range)         %s" % med(gpu1))
        print("  add, host time per image (enqueue, no sync)    %s" % med(host))
        print("  accumulate: keys kernel (GPU time)             %s" % med(steps["keys"]))
        print("  accumulate: torch stable sort (GPU time)       %s" % med(steps["sort"]))
        print("  accumulate: scan kernel (GPU time)             %s" % med(steps["scan"]))
        print("  accumulate() + synchronise (host time)         %s" % med(steps["call"]), flush=True)
        if args.no_host_route:
            continue
        # the host route: match per image and area range, copy, synchronise; accumulate in numpy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = []
        for i in range(N):
            p = i % pool
            per_range = [merger.match_instances(d_tab[p], d_pcls[p], d_tcls[p], scores=d_scores[i], crowd=d_crowd[p],
                                                area_range=r) for r in AREA_RANGES]
            host_arrays = [{k: m[k].cpu().numpy() for k in ("pred_match", "pred_ignore", "truth_ignore")}
                           for m in per_range]
            order = labels.detection_order(scores[i], K)
            rank = np.zeros(K, np.int32)
            seen = {}
            for d in order:
                rank[d] = seen.get(int(pcls[p][d]), 0)
                seen[int(pcls[p][d])] = int(rank[d]) + 1
            npig = np.zeros((C, A), np.int64)
            for a, h in enumerate(host_arrays):
                np.add.at(npig[:, a], tcls[p][~h["truth_ignore"]], 1)
            recs.append({"classes": pcls[p][order], "scores": scores[i][order], "rank": rank[order],
                         "image": np.full(K, i, np.int32),
                         "matched": np.stack([h["pred_match"][:, order] > 0 for h in host_arrays]),
                         "ignored": np.stack([h["pred_ignore"][:, order] for h in host_arrays]), "npig": npig})
        t1 = time.perf_counter()
        want = labels.coco_accumulate(recs, C, form="closed")
        t2 = time.perf_counter()
        for key in ("precision", "recall", "scores", "npig"):
            assert np.array_equal(result[key].cpu().numpy(), want[key]), "%s differs from the host route" % key
        print("  host route: match, copy, synchronise per image %10.1f us per image (%.2f s in all)"
              % ((t1 - t0) * 1e6 / N, t1 - t0))
        print("  host route: labels.coco_accumulate on the host %10.2f s; the arrays equal the device's bit for bit"
              % (t2 - t1), flush=True)
    merger.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
