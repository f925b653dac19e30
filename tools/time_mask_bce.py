#!/usr/bin/env python
"""mn_mask_bce against what it replaces and against the nearest existing pass, on the same tensors.

    python tools/time_mask_bce.py [--reps 50] [--repeats 5] [--quick]

Logits: the benchmark's generator (synth-v1, seed 1000, 1024x2048, C = 9, O = 10) turned into logits
(log p - log(1 - p) of the clipped probabilities) in float32 and in bfloat16; the truth is the generator's own instance
mask and class list.  Each dtype is held in enough copies, used in rotation, to pass the 256 MB Infinity Cache, each
with a mask and -- for the rows that write one -- a gradient buffer of its own.

Rows, all GPU TIME per call: the stream is first kept busy by large matmuls, then `reps` calls are queued between two
HIP events, so the GPU runs them back to back (the sweep is timed by the library the same way: mn_sweep_time_device).
    mask_bce, loss + gradient   Merger.mask_bce with both gradients: every logit read once, every gradient written once
    mask_bce, loss only         grad=False: the validation loss
    torch, loss + gradient      what a user writes today: Merger.sameness_targets (ten float32 target planes), the
                                one-hot class planes from the label mask, torch.nn.BCEWithLogitsLoss on both parts,
                                cls_loss + alpha * ofs_loss, backward into the logits' .grad
    torch, loss only            the same under torch.no_grad(), without backward
    sweep                       Merger.sweep_time on the probabilities of the same maps: it reads the same planes
GB/s are against the byte count from the shapes: (C + O) * H * W * element size for the logits, as much again for the
gradient where one is written, + 4 * H * W for the mask.
One warm-up round, then `repeats` rounds that alternate the rows; median (min - max) over the rounds.  Before anything
is timed the results are compared: the sums and the gradient with labels.mask_bce within the bounds of
tests/test_gpu_mask_bce.py, the loss with the torch composition, and two calls with each other byte for byte.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="256x512 instead of 1024x2048")
    args = ap.parse_args()

    import numpy as np
    import torch
    from mergenet_amd import labels, segmenter as seg, synth

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    H, W, C = (256, 512, 9) if args.quick else (1024, 2048, 9)
    offs = synth.generate_offsets(40, 10)
    O = len(offs)
    alpha = 1.0
    img = synth.synth_v1(H, W, C, offs, 1000)
    merger = seg.Merger(H, W, C, O)
    opts = seg.default_options(merge_logprob_bias=0.03)
    truth_np = np.ascontiguousarray(img.instances, np.int32)
    classes_np = np.asarray(img.instance_class[1:], np.int32)
    G = int(classes_np.size)
    truth_classes = torch.from_numpy(classes_np).to(dev)
    by_label = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), truth_classes.long()])
    n = H * W
    scale_c, scale_s = 1.0 / (C * n), alpha / (O * n)

    def logit(p):
        p = np.clip(p.astype(np.float64), 2.0 ** -23, 1 - 2.0 ** -23)
        return (np.log(p) - np.log1p(-p)).astype(np.float32)

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

    bce = torch.nn.BCEWithLogitsLoss()
    for dtype in (torch.float32, torch.bfloat16):
        elem = 4 if dtype == torch.float32 else 2
        name = str(dtype).replace("torch.", "")
        plane_bytes = (C + O) * n * elem
        copies = -(-320 * 2 ** 20 // plane_bytes) + 1
        pred0 = torch.cat([torch.from_numpy(logit(img.class_probs)), torch.from_numpy(logit(img.sameness_probs))])
        pred0 = pred0.to(dev).to(dtype)
        preds = [pred0.clone() for _ in range(copies)]
        grads = [torch.empty_like(pred0) for _ in range(copies)]
        leaves = [p.clone().requires_grad_() for p in preds]
        probs = [(torch.sigmoid(p[:C].float()).to(dtype).contiguous(), torch.sigmoid(p[C:].float()).to(dtype).contiguous())
                 for p in preds]
        truths = [torch.from_numpy(truth_np).to(dev) for _ in range(copies)]

        def ours(i):
            return merger.mask_bce(preds[i][:C], preds[i][C:], offs, truths[i], truth_classes, scale_c, scale_s,
                                   out=(grads[i][:C], grads[i][C:]))

        def ours_loss(i):
            return merger.mask_bce(preds[i][:C], preds[i][C:], offs, truths[i], truth_classes, grad=False)

        def targets(i):
            tcls = by_label[truths[i].long()]
            cls_t = (tcls[None] == torch.arange(C, device=dev)[:, None, None]).to(dtype)
            return cls_t, merger.sameness_targets(truths[i], offs).to(dtype)

        def composed(i):
            x = leaves[i]
            x.grad = None
            cls_t, ofs_t = targets(i)
            loss = bce(x[:C], cls_t) + alpha * bce(x[C:], ofs_t)
            loss.backward()
            return loss

        def composed_loss(i):
            with torch.no_grad():
                cls_t, ofs_t = targets(i)
                return bce(preds[i][:C], cls_t) + alpha * bce(preds[i][C:], ofs_t)

        got, again = ours(0), ours(0)
        assert got["sums"].cpu().numpy().tobytes() == again["sums"].cpu().numpy().tobytes(), "two calls differ"
        assert ours_loss(0)["sums"].cpu().numpy().tobytes() == got["sums"].cpu().numpy().tobytes(), "grad=False differs"
        wide = pred0.float().cpu().numpy()
        want_sums, want_gc, want_gs = labels.mask_bce(wide[:C], wide[C:], offs, truth_np, classes_np, G, scale_c, scale_s)
        sums = got["sums"].cpu().numpy()
        assert sums[-1] == want_sums[-1] == n, "the generator has no ignore class"
        rel = np.abs(sums[:-1] - want_sums[:-1]) / want_sums[:-1]
        assert (rel <= 2.0 ** -21 + C * n * 2.0 ** -53).all(), "sums differ from the statement by %g relative" % rel.max()
        g = grads[0].float().cpu().numpy().astype(np.float64)
        ref = np.concatenate([want_gc, want_gs])
        scale = np.concatenate([np.full(C, scale_c), np.full(O, scale_s)])[:, None, None]
        half = 0.0 if elem == 4 else 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 8)
        worst = (np.abs(g - ref) / (2.0 ** -21 * scale + half)).max()
        assert worst <= 1.0, "gradient differs from the statement: %g of the bound" % worst
        ours_value = float(sums[0] * scale_c + sums[1:1 + O].sum() * scale_s)
        want_value = float(want_sums[0] * scale_c + want_sums[1:1 + O].sum() * scale_s)
        torch_value = float(composed(0).item())
        print("[%s] %dx%d, C = %d, O = %d, G = %d; %d sets in rotation (%.0f MB of logits); loss %.9g, statement "
              "%.9g, torch composition %.9g; sums within %.2g relative of the statement (bound %.2g), gradient within "
              "%.2g of its bound" % (name, H, W, C, O, G, copies, copies * plane_bytes / 2 ** 20, ours_value,
                                     want_value, torch_value, rel.max(), 2.0 ** -21, worst), flush=True)
        assert abs(torch_value - want_value) <= (2.0 ** -7 if elem == 2 else 2.0 ** -18) * want_value, \
            "the torch composition computes another loss"

        rows = [("mask_bce, loss + gradient              ", 2 * plane_bytes + 4 * n),
                ("mask_bce, loss only (grad=False)       ", plane_bytes + 4 * n),
                ("torch: targets + BCEWithLogits + backward", 2 * plane_bytes + 4 * n),
                ("torch: targets + BCEWithLogits, no_grad", plane_bytes + 4 * n),
                ("sweep (Merger.sweep_time), these maps  ", plane_bytes)]
        times = {r[0]: [] for r in rows}
        for rnd in range(args.repeats + 1):                      # round 0 warms up
            us = [timed(ours, copies, args.reps), timed(ours_loss, copies, args.reps),
                  timed(composed, copies, max(2, args.reps // 5)), timed(composed_loss, copies, max(2, args.reps // 5)),
                  merger.sweep_time(probs, offs, opts, reps=args.reps)]
            if rnd:
                for r, u in zip(rows, us):
                    times[r[0]].append(u)
        med = {}
        for r, floor in rows:
            t = times[r]
            med[r] = statistics.median(t)
            print("  %s %9.2f us per call (min %.2f max %.2f over %d rounds)  %7.0f GB/s of the %.0f MB floor" %
                  (r, med[r], min(t), max(t), len(t), floor / med[r] * 1e-3, floor / 1e6), flush=True)
        print("  ratios: torch composition / mask_bce with gradient %.2f, without %.2f; mask_bce with gradient / "
              "sweep %.2f, without / sweep %.2f" % (med[rows[2][0]] / med[rows[0][0]], med[rows[3][0]] / med[rows[1][0]],
                                                   med[rows[0][0]] / med[rows[4][0]], med[rows[1][0]] / med[rows[4][0]]),
              flush=True)
        del preds, grads, leaves, probs, truths
        torch.cuda.empty_cache()
    merger.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
