#!/usr/bin/env python
"""mn_mask_ce against what it replaces and against the nearest existing pass, on the same tensors.

    python tools/time_mask_ce.py [--reps 30] [--repeats 5] [--quick] > profiles/mask_ce_time.log

1024x2048, float32 and bfloat16.  Three rows of planes:
    offset part, 10 planes      the Cityscapes recipe's --loss ce (resident form, bucket 10)
    class part, 9 planes        (resident form, bucket 10)
    class part, 81 planes       the COCO recipe's (streaming form: the planes are read three times, twice without a
                                gradient)
Logits: uniform in -8..8 from a seeded generator; the truth is the benchmark generator's instance mask (synth-v1, seed
1000) with its class list -- for 81 planes the classes are spread over 0..80.  Each row's logits are held in enough
copies, used in rotation, to pass the 256 MB Infinity Cache, each with a mask and a gradient buffer of its own.

Per row, all GPU TIME per call: the stream is first kept busy by large matmuls, then `reps` calls are queued between two
HIP events, so the GPU runs them back to back.
    mask_ce, loss + gradient    Merger.mask_ce with the gradient
    mask_ce, loss only          grad=False: the validation loss
    torch, loss + gradient      what a user writes today: the target planes on the device (Merger.sameness_targets, or
                                the one-hot class planes from the label mask), target.max(0)[1], F.cross_entropy,
                                backward into the logits' .grad
    torch, loss only            the same under torch.no_grad(), without backward
    mask_bce, loss + gradient   Merger.mask_bce on the same planes (as class planes / as offset planes): the nearest
    mask_bce, loss only         existing pass -- another criterion, the same reads and writes
GB/s are against the byte count from the shapes: P * H * W * element size for the logits read ONCE, as much again for
the gradient where one is written, + 4 * H * W for the mask.  The streaming form reads the planes three (two) times, the
repeats through the cache: its share of that floor says what the re-reads cost.
One warm-up round, then `repeats` rounds that alternate the rows; median (min - max) over the rounds.  Before anything
is timed the results are compared: the sums and the gradient with labels.mask_ce within the bounds of
tests/test_gpu_mask_ce.py, the loss with the torch composition, and two calls with each other byte for byte.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="256x512 instead of 1024x2048")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    from mergenet_amd import labels, segmenter as seg, synth

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    H, W = (256, 512) if args.quick else (1024, 2048)
    n = H * W
    offs = synth.generate_offsets(40, 10)
    img = synth.synth_v1(H, W, 9, offs, 1000)
    merger = seg.Merger(H, W, 9, 10)
    truth_np = np.ascontiguousarray(img.instances, np.int32)
    classes9 = np.asarray(img.instance_class[1:], np.int32)
    G = int(classes9.size)
    U = 2.0 ** -24

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
        name = str(dtype).replace("torch.", "")
        for part, P in (("offset", 10), ("class", 9), ("class", 81)):
            classes_np = classes9 if P == 9 else (classes9.astype(np.int64) * 9 + np.arange(G) % 9).astype(np.int32) % P
            truth_classes = torch.from_numpy(classes_np).to(dev)
            by_label = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), truth_classes.long()])
            part_offs = offs if part == "offset" else None
            scale = 1.0 / n
            plane_bytes = P * n * elem
            copies = -(-320 * 2 ** 20 // plane_bytes) + 1
            rng = np.random.default_rng(1000 + P)
            pred0 = torch.from_numpy((rng.random((P, H, W), dtype=np.float32) * 16 - 8)).to(dev).to(dtype)
            preds = [pred0.clone() for _ in range(copies)]
            grads = [torch.empty_like(pred0) for _ in range(copies)]
            leaves = [p.clone().requires_grad_() for p in preds]
            truths = [torch.from_numpy(truth_np).to(dev) for _ in range(copies)]

            def ours(i):
                return merger.mask_ce(preds[i], part, part_offs, truths[i], truth_classes, scale, out=grads[i])

            def ours_loss(i):
                return merger.mask_ce(preds[i], part, part_offs, truths[i], truth_classes, grad=False)

            def target(i):
                if part == "offset":
                    planes = merger.sameness_targets(truths[i], offs)
                else:
                    planes = (by_label[truths[i].long()][None] == torch.arange(P, device=dev)[:, None, None]).to(dtype)
                return planes.max(0)[1]

            def composed(i):
                x = leaves[i]
                x.grad = None
                loss = F.cross_entropy(x[None], target(i)[None])
                loss.backward()
                return loss

            def composed_loss(i):
                with torch.no_grad():
                    return F.cross_entropy(preds[i][None], target(i)[None])

            def bce(i):
                if part == "offset":
                    return merger.mask_bce(None, preds[i], offs, truths[i], truth_classes, 1.0, scale, out=(None, grads[i]))
                return merger.mask_bce(preds[i], None, [], truths[i], truth_classes, scale, 1.0, out=(grads[i], None))

            def bce_loss(i):
                if part == "offset":
                    return merger.mask_bce(None, preds[i], offs, truths[i], truth_classes, grad=False)
                return merger.mask_bce(preds[i], None, [], truths[i], truth_classes, grad=False)

            got, again = ours(0), ours(0)
            kept_grad = grads[0].float().cpu().numpy().astype(np.float64)
            assert got["sums"].cpu().numpy().tobytes() == again["sums"].cpu().numpy().tobytes(), "two calls differ"
            assert ours_loss(0)["sums"].cpu().numpy().tobytes() == got["sums"].cpu().numpy().tobytes(), "grad=False differs"
            wide = pred0.float().cpu().numpy()
            want_sums, want_grad = labels.mask_ce(wide, part, part_offs, truth_np, classes_np, G, scale)
            sums = got["sums"].cpu().numpy()
            assert sums[1] == want_sums[1] == n, "the generator has no ignore class"
            D = min(88.0, float((wide.max(axis=0) - wide.min(axis=0)).max()))
            rel = abs(sums[0] - want_sums[0]) / want_sums[0]
            assert rel <= (D + P + 5) * U + n * 2.0 ** -53, "sum differs from the statement by %g relative" % rel
            half = 0.0 if elem == 4 else 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want_grad), 2.0 ** -126))) - 8)
            worst = (np.abs(kept_grad - want_grad) / ((2 * D + P + 12) * U * scale + half)).max()
            assert worst <= 1.0, "gradient differs from the statement: %g of the bound" % worst
            ours_value, want_value = float(sums[0] * scale), float(want_sums[0] * scale)
            torch_value = float(composed(0).item())
            print("[%s, %s part, %d planes] %dx%d, G = %d; %d sets in rotation (%.0f MB of logits); loss %.9g, statement "
                  "%.9g, torch composition %.9g; sum within %.2g relative of the statement, gradient within %.3g of its "
                  "bound" % (name, part, P, H, W, G, copies, copies * plane_bytes / 2 ** 20, ours_value, want_value,
                             torch_value, rel, worst), flush=True)
            # (a check that the composition computes the same function, not of its precision: in bfloat16 torch
            # rounds the log-softmax planes and the loss to 8 bits)
            assert abs(torch_value - want_value) <= (2.0 ** -5 if elem == 2 else 2.0 ** -18) * want_value, \
                "the torch composition computes another loss"

            rows = [("mask_ce, loss + gradient               ", 2 * plane_bytes + 4 * n, ours, args.reps),
                    ("mask_ce, loss only (grad=False)        ", plane_bytes + 4 * n, ours_loss, args.reps),
                    ("torch: targets + cross_entropy + backward", 2 * plane_bytes + 4 * n, composed, max(2, args.reps // 5)),
                    ("torch: targets + cross_entropy, no_grad", plane_bytes + 4 * n, composed_loss, max(2, args.reps // 5)),
                    ("mask_bce on these planes, loss + gradient", 2 * plane_bytes + 4 * n, bce, args.reps),
                    ("mask_bce on these planes, loss only    ", plane_bytes + 4 * n, bce_loss, args.reps)]
            times = {r[0]: [] for r in rows}
            for rnd in range(args.repeats + 1):                  # round 0 warms up
                for r, _, fn, reps in rows:
                    us = timed(fn, copies, reps)
                    if rnd:
                        times[r].append(us)
            med = {}
            for r, floor, _, _ in rows:
                t = times[r]
                med[r] = statistics.median(t)
                print("  %s %9.2f us per call (min %.2f max %.2f over %d rounds)  %7.0f GB/s of the %.0f MB floor" %
                      (r, med[r], min(t), max(t), len(t), floor / med[r] * 1e-3, floor / 1e6), flush=True)
            k = [r[0] for r in rows]
            print("  ratios: torch composition / mask_ce with gradient %.2f, without %.2f; mask_ce / mask_bce with "
                  "gradient %.2f, without %.2f" % (med[k[2]] / med[k[0]], med[k[3]] / med[k[1]], med[k[0]] / med[k[4]],
                                                   med[k[1]] / med[k[5]]), flush=True)
            del preds, grads, leaves, truths
            torch.cuda.empty_cache()
    merger.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
