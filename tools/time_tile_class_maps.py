#!/usr/bin/env python
"""mn_tile_class_maps against the composition a user writes in torch today, at the production shape.

    python tools/time_tile_class_maps.py [--reps 20] [--repeats 5] [--quick]

Shape: the production recipe's: image 1024x2048, tiles 713x713 at the reference's starts (3 x 4 =
12 tiles), Cn = 19 network classes folded to C = 9 planes, with the flipped pass.  Logits: seeded normal values times 4,
in float32 and in bfloat16.  The tiles of one call are 927 MB in float32 (463 MB in bfloat16), beyond the 256 MB
Infinity Cache on their own, so no rotation of inputs is needed.

Rows, all GPU TIME per call: the stream is first kept busy by large matmuls, then `reps` calls are queued between two
HIP events, so the GPU runs them back to back.
    mn_tile_class_maps   the kernel of this build: every tile logit once, the C planes written once
    torch composition    per tile softmax of both passes, flip, average, maximum over the stuff classes, slice-add into
                         the image and into a count plane; then the two divisions (about ten launches per tile)
TB/s are against the byte floor from the shapes, T*th*tw*Cn*esize*2 + C*H*W*out_size.
One warm-up round, then `repeats` rounds that alternate the rows; median (min - max) over the rounds.  Before anything
is timed the kernel's output is compared with the torch composition (float32 arithmetic on both sides: twice the bound
of the tests, (Cn + cover_max + C + 8) * 2^-24 each) and two calls with each other bit for bit.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="image 256x512, tiles 177x177")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from mergenet_amd import segmenter as seg, tiles as mt

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    H, W, side = (256, 512, 177) if args.quick else (1024, 2048, 713)
    Cn, C = 19, 9
    rows, cols = mt.tile_starts(H, side), mt.tile_starts(W, side)
    T = len(rows) * len(cols)
    cover_max = int(mt.tile_cover_count(rows, cols, side, side, H, W).max())
    merger = seg.Merger(64, 64, C, 1)                       # the call is not held to the context's capacity
    spin_a = torch.randn((8192, 8192), device=dev)

    def spin():
        for _ in range(4):
            torch.mm(spin_a, spin_a)

    def timed(fn, reps):
        spin()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps                  # microseconds per call, GPU time

    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    for dtype in (torch.float32, torch.bfloat16):
        esize = 4 if dtype == torch.float32 else 2
        floor = T * side * side * Cn * esize * 2 + C * H * W * esize
        tiles = (torch.randn((T, Cn, side, side), device=dev, generator=gen) * 4.0).to(dtype)
        flips = (torch.randn((T, Cn, side, side), device=dev, generator=gen) * 4.0).to(dtype)

        def ours():
            return merger.tile_class_maps(tiles, flips, rows, cols, H, W, C)

        def composed():
            pred = torch.zeros((C, H, W), dtype=torch.float32, device=dev)
            count = torch.zeros((H, W), dtype=torch.float32, device=dev)
            t = 0
            for r in rows:
                for c in cols:
                    p = (F.softmax(tiles[t].float(), dim=0) + F.softmax(flips[t].float(), dim=0).flip(-1)) / 2.0
                    pred[0, r:r + side, c:c + side] += p[:Cn - C + 1].max(dim=0)[0]
                    pred[1:, r:r + side, c:c + side] += p[Cn - C + 1:]
                    count[r:r + side, c:c + side] += 1.0
                    t += 1
            score = pred / count[None]
            return (score / score.sum(0, keepdim=True)).to(dtype)

        got, again, want = ours(), ours(), composed()
        assert torch.equal(got.view(torch.int32 if esize == 4 else torch.int16),
                           again.view(torch.int32 if esize == 4 else torch.int16)), "two calls differ"
        err = float((got.float() - want.float()).abs().max())
        bound = 2 * (Cn + cover_max + C + 8) * 2.0 ** -24 + (2.0 ** -8 if esize == 2 else 0.0)   # + two bfloat16 roundings
        assert err <= bound, "differs from the torch composition by %g (bound %g)" % (err, bound)
        print("%s: image %dx%d, %d tiles %dx%d (cover up to %d), Cn = %d -> C = %d, with flip; tiles %.0f MB + planes "
              "%.0f MB; within %.2g of the torch composition (bound %.2g)"
              % (str(dtype).replace("torch.", ""), H, W, T, side, side, cover_max, Cn, C,
                 T * side * side * Cn * esize * 2 / 1e6, C * H * W * esize / 1e6, err, bound), flush=True)
        del got, again, want

        names = ["mn_tile_class_maps                     ", "torch: softmax, flip, max, slice-add, /"]
        times = {r: [] for r in names}
        for rnd in range(args.repeats + 1):                      # round 0 warms up
            us = [timed(ours, args.reps), timed(composed, max(2, args.reps // 5))]
            if rnd:
                for r, u in zip(names, us):
                    times[r].append(u)
        for r in names:
            t = times[r]
            med = statistics.median(t)
            print("  %s %10.1f us per call (min %.1f max %.1f over %d rounds)  %6.2f TB/s of the %.0f MB floor" %
                  (r, med, min(t), max(t), len(t), floor / med * 1e-6, floor / 1e6), flush=True)
        del tiles, flips
        torch.cuda.empty_cache()
    merger.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
