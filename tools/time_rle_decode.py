#!/usr/bin/env python
"""mn_rle_decode_device / Merger.decode_rle against the nearest yardsticks on the same annotations.

    python tools/time_rle_decode.py [--reps 100] [--repeats 5] [--variant-lib LABEL=PATH ...] [--quick]

Workloads, both at 1024x2048 (--quick: 256x512):
  (a) the ground-truth instance mask of the benchmark's generator (synth-v1, seed 1000, C = 9, O = 10), encoded per
      label by Merger.encode_rle: what a validation loop reads from an annotation file;
  (b) a stress set: 200 overlapping rectangles of a sixteenth of the image each, every one cut into stripes three
      rows high, so runs of 3 pixels: several million counts, about twenty ends in a 64-row segment per annotation
      and a dozen annotations over the average pixel; handed over as count lists.

Rows.  GPU TIME per call: the stream is first kept busy by large matmuls, then `reps` calls are queued between two
HIP events, so the GPU runs them back to back; the mask goes to `copies` output buffers in rotation (more than
256 MB: beyond the Infinity Cache), and so do the counts.
    mn_rle_decode_device              the two kernels, counts and starts already on the device
    torch composition                 per annotation torch.repeat_interleave of the run parities (output_size given,
                                      so nothing synchronises), a transposed view, torch.where(mask == 0, ...)
HOST-VISIBLE TIME per call (a host clock around the call and ONE synchronisation; not to be compared with the rows
above):
    Merger.decode_rle                 from the items (strings in (a): native parse; count lists in (b): numpy
                                      conversion), three small copies, the kernels
    numpy label_mask + copy           today's path: rle.label_mask on the host and the 4 * H * W byte copy of the mask
The floor is the mask itself: 4 * H * W bytes stored once.
One warm-up round, then `repeats` rounds that alternate the rows; median (min - max) over the rounds.  The numpy
path runs once per workload (it takes seconds) and its result is what every other row is compared with before
anything is timed.

--variant-lib: builds of the library with the other form of the paint pass (mn_kernels_rle.h), each timed in a child
process of its own on the same annotations (a process binds one library), e.g.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DMN_RLE_CARRY=0 -shared \
          mergenet_amd/csrc/mergenet_hip.hip -o build_diag/lib_rle_fresh_search.so
for a fresh bisection of the ends in every column.  The run stops after the first child that fails.
"""
import argparse
import ctypes
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
    from mergenet_amd import rle, segmenter as seg, synth

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    H, W, C = (256, 512, 9) if args.quick else (1024, 2048, 9)
    N = H * W
    offs = synth.generate_offsets(40, 10)
    img = synth.synth_v1(H, W, C, offs, 1000)
    merger = seg.Merger(H, W, C, len(offs))
    lib = merger.lib

    truth = np.ascontiguousarray(img.instances, np.int32)
    G = int(truth.max())
    gt = [r["counts"] for r in merger.encode_rle(torch.from_numpy(truth).to(dev), G)]

    rng = np.random.default_rng(5)
    stripes = ((np.arange(H)[:, None] // 3) % 2).astype(np.uint8)
    stress = []
    for _ in range(200 if not args.quick else 40):
        y, x = int(rng.integers(0, H - H // 4)), int(rng.integers(0, W - W // 4))
        b = np.zeros((H, W), np.uint8)
        b[y:y + H // 4, x:x + W // 4] = stripes[y:y + H // 4]
        stress.append(rle.binary_mask_counts(b))

    spin_a = torch.randn((8192, 8192), device=dev)

    def spin():
        for _ in range(4):
            torch.mm(spin_a, spin_a)

    def gpu_time(fn, reps):
        spin()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps                # microseconds per call, GPU time

    def host_time(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(reps):
            fn(i)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / reps          # microseconds per call as the host sees it

    for title, items in (("(a) the generator's ground truth, seed 1000, encoded per label", gt),
                         ("(b) stress: overlapping striped rectangles, runs of 3", stress)):
        A = len(items)
        lists = [np.asarray(rle.string_to_counts(it) if isinstance(it, bytes) else it, np.int64) for it in items]
        flat = np.concatenate(lists).astype(np.uint32).view(np.int32)
        starts = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int32)
        T = int(flat.size)

        t0 = time.perf_counter()
        want = rle.label_mask([c.tolist() for c in lists], H, W)
        d_want = torch.from_numpy(want).to(dev)
        torch.cuda.synchronize()
        numpy_us = (time.perf_counter() - t0) * 1e6

        copies = max(2, min(64, -(-320 * 2 ** 20 // (N * 4))))
        outs = [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(copies)]
        in_copies = max(2, min(copies, -(-320 * 2 ** 20 // max(1, T * 4))))
        d_counts = [torch.from_numpy(flat).to(dev) for _ in range(in_copies)]
        d_starts = torch.from_numpy(starts).to(dev)
        ends = torch.empty((max(1, T),), dtype=torch.int32, device=dev)
        records = torch.empty((max(1, A), 4), dtype=torch.int32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def kernels(i):
            rc = lib.mn_rle_decode_device(merger.handle, d_counts[i % in_copies].data_ptr(), d_starts.data_ptr(), A, T,
                                          None, H, W, ends.data_ptr(), records.data_ptr(),
                                          outs[i % copies].data_ptr(), None, stream)
            assert rc == 0

        d_lists = [torch.from_numpy(c).to(dev) for c in lists]
        d_parity = [(torch.arange(len(c), device=dev) & 1).to(torch.int32) for c in lists]

        d_value = [torch.tensor(a + 1, dtype=torch.int32, device=dev) for a in range(A)]

        def composition(i):
            mask = torch.zeros((H, W), dtype=torch.int32, device=dev)
            for a in range(A):
                m = torch.repeat_interleave(d_parity[a], d_lists[a], output_size=N).view(W, H).t()
                mask = torch.where((mask == 0) & (m != 0), d_value[a], mask)
            return mask

        def whole_call(i):
            return merger.decode_rle(items, H, W)

        kernels(0)
        assert torch.equal(outs[0], d_want), "the kernels differ from rle.label_mask"
        assert torch.equal(composition(1), d_want), "the torch composition differs from rle.label_mask"
        assert torch.equal(whole_call(0), d_want), "Merger.decode_rle differs from rle.label_mask"

        forms = [("kernels   mn_rle_decode_device                     (GPU time) ", kernels, gpu_time, args.reps),
                 ("compose   torch repeat_interleave + where per annot. (GPU time) ", composition, gpu_time, 2),
                 ("call      Merger.decode_rle from the items          (host time)", whole_call, host_time,
                  max(2, args.reps // 10))]
        times = {name: [] for name, _, _, _ in forms}
        for rnd in range(args.repeats + 1):                              # round 0 warms up
            for name, fn, clock, reps in forms:
                us = clock(fn, reps)
                if rnd:
                    times[name].append(us)
        print("[%s] %s; %dx%d, A = %d, %d counts (%.2f MB); %d output masks in rotation (%.0f MB)" %
              (tag, title, H, W, A, T, T * 4 / 2 ** 20, copies, copies * N * 4 / 2 ** 20), flush=True)
        for name, _, _, _ in forms:
            t = times[name]
            print("  %s %11.2f us per call (min %.2f max %.2f over %d rounds)" %
                  (name, statistics.median(t), min(t), max(t), len(t)), flush=True)
        print("  today     numpy rle.label_mask + the copy of the mask  (host time) %11.2f us, one run" % numpy_us,
              flush=True)
        k = statistics.median(times[forms[0][0]])
        print("  floor     the mask is %.2f MB, stored once; the kernels' %.2f us are %.1f GB/s of mask" %
              (N * 4 / 2 ** 20, k, N * 4 / k / 1e3), flush=True)
    merger.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="256x512 and 40 stress annotations")
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
