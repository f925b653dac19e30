#!/usr/bin/env python
"""The Dice and weighted multi-BCE criteria from the label mask against the torch composition they replace.

    python tools/time_plane_losses.py [--reps 30] [--repeats 5] [--quick] [--out profiles/plane_losses_time.log]

Logits: the benchmark's generator (synth-v1, seed 1000, 1024x2048, C = 9, O = 10) turned into logits, in float32 and
in bfloat16; the truth is the generator's own instance mask and class list.  One image per call (B = 1).  Variants:
the 10 offset planes under Dice mode '0' (the Cityscapes recipe's --loss dice) and under MBCE, the 9 class planes under
Dice mode '1' and under MBCE.  Each dtype is held in enough copies, used in rotation, to pass the 256 MB Infinity
Cache, each with a mask, a target tensor and a gradient buffer of its own.

Rows, all GPU TIME per image: the stream is first kept busy by large matmuls, then `reps` calls are queued between
two HIP events, so the GPU runs them back to back.
    three steps          Merger.plane_sums + plane_coeffs + plane_grad (the incoming gradient read from the device)
    sums + coefficients  the forward alone (what runs under torch.no_grad())
    gradient pass        plane_grad alone
    torch composition    the same criterion on target planes that are ALREADY BUILT (float tensors of the logits'
                         dtype): forward + backward into the logits' .grad.  Written vectorised over the planes, which
                         is faster than the reference's loop over them (utils/loss.py:49-57): the comparison errs in
                         torch's favour.
One warm-up round, then `repeats` rounds that alternate the rows; median (min - max) over the rounds.  Before anything
is timed the loss is compared with the composition's and two runs with each other byte for byte.  A variant that does
not beat the composition is reported as such: nothing here is a threshold.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_losses_time.log"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from mergenet_amd import segmenter as seg, synth

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda", 0)
    H, W, C = (256, 512, 9) if args.quick else (1024, 2048, 9)
    offs = synth.generate_offsets(40, 10)
    O = len(offs)
    img = synth.synth_v1(H, W, C, offs, 1000)
    merger = seg.Merger(64, 128, C, O)                          # (the passes take any image size)
    truth_np = np.ascontiguousarray(img.instances, np.int32)
    truth_classes = torch.from_numpy(np.asarray(img.instance_class[1:], np.int32)).to(dev)
    by_label = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), truth_classes.long()])
    n = H * W
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

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

    def dice_composition(x, t, mode):
        p = torch.sigmoid(x)
        if mode == "0":
            p, t = 1 - p, 1 - t
        return (1 - (2.0 * (p * t).sum((1, 2)) + 1.0) / (p.sum((1, 2)) + t.sum((1, 2)) + 1.0)).sum()

    def mbce_composition(x, t):
        s = torch.sigmoid(x).sum((1, 2))
        weight = ((n - s + 1) / (s + 1))[:, None, None] * t + (1 - t)
        return (weight * torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")).mean()

    say("# Dice and weighted multi-BCE from the label mask (Merger.plane_sums + plane_coeffs + plane_grad) against the torch")
    say("# composition of the same criterion with its target planes already built, forward + backward; %dx%d, one image per" % (H, W))
    say("# call, GPU time between HIP events behind a busy stream, %d calls per round, median (min - max) over %d rounds;" % (args.reps, args.repeats))
    say("# tensors in rotation beyond the Infinity Cache.  %s" % torch.cuda.get_device_name(0))
    variants = [("offset", O, "dice", "0"), ("offset", O, "mbce", None), ("class", C, "dice", "1"), ("class", C, "mbce", None)]
    for dtype in (torch.float32, torch.bfloat16):
        elem = 4 if dtype == torch.float32 else 2
        name = str(dtype).replace("torch.", "")
        for part, P, crit, mode in variants:
            planes = img.sameness_probs if part == "offset" else img.class_probs
            plane_bytes = P * n * elem
            copies = -(-320 * 2 ** 20 // plane_bytes) + 1
            pred0 = torch.from_numpy(logit(planes)).to(dev).to(dtype)
            preds = [pred0.clone() for _ in range(copies)]
            grads = [torch.empty_like(pred0) for _ in range(copies)]
            leaves = [p.clone().requires_grad_() for p in preds]
            truths = [torch.from_numpy(truth_np).to(dev) for _ in range(copies)]
            if part == "offset":
                target0 = merger.sameness_targets(truths[0], offs).to(dtype)
            else:
                target0 = (by_label[truths[0].long()][None] == torch.arange(C, device=dev)[:, None, None]).to(dtype)
            targets = [target0.clone() for _ in range(copies)]
            tc = truth_classes if part == "class" else None
            comp = mode == "0"
            factor = torch.ones((), dtype=torch.float32, device=dev)
            scale = 1.0 if crit == "dice" else 1.0 / (P * n)
            sums_buf = torch.empty((5 * P + 1,), dtype=torch.float64, device=dev)
            coeff_buf = torch.empty((4, P), dtype=torch.float32, device=dev)

            def forward(i):
                s = merger.plane_sums(preds[i], part, offs, truths[i], tc, complement=comp, terms=crit == "mbce", out=sums_buf)
                return merger.plane_coeffs(crit, s, pixels=n, smooth=1.0, scale=scale, complement=comp, out=coeff_buf)

            def backward(i):
                return merger.plane_grad(preds[i], part, offs, truths[i], tc, coeff_buf, factor=factor, complement=comp,
                                         out=grads[i])

            def ours(i):
                res = forward(i)
                backward(i)
                return res

            def composed(i):
                x = leaves[i]
                x.grad = None
                loss = dice_composition(x, targets[i], mode) if crit == "dice" else mbce_composition(x, targets[i])
                loss.backward()
                return loss

            a = ours(0)["loss"].item()
            g0 = grads[0].clone()
            b = ours(0)["loss"].item()
            assert a == b and torch.equal(g0.view(torch.int16), grads[0].view(torch.int16)), "two runs differ"
            want = float(composed(0).item())
            tol = 2.0 ** -4 if elem == 2 else 2.0 ** -16
            assert abs(a - want) <= tol * abs(want), "the torch composition computes another loss: %g against %g" % (want, a)
            gdiff = (grads[0].float() - leaves[0].grad.float()).abs().max().item() / leaves[0].grad.float().abs().max().item()
            say("[%s, %s planes, %s%s] P = %d, %d sets in rotation (%.0f MB of logits); loss %.9g, torch composition %.9g; "
                "greatest gradient difference %.2g of the greatest element" %
                (name, part, crit, "" if mode is None else " mode '%s'" % mode, P, copies, copies * plane_bytes / 2 ** 20,
                 a, want, gdiff))
            rows = ["three steps: sums + coefficients + gradient", "  sums + coefficients (forward)            ",
                    "  gradient pass (backward)                 ", "torch composition, forward + backward      "]
            times = {r: [] for r in rows}
            for rnd in range(args.repeats + 1):                  # round 0 warms up
                us = [timed(ours, copies, args.reps), timed(forward, copies, args.reps), timed(backward, copies, args.reps),
                      timed(composed, copies, max(2, args.reps // 5))]
                if rnd:
                    for r, u in zip(rows, us):
                        times[r].append(u)
            med = {r: statistics.median(times[r]) for r in rows}
            for r in rows:
                t = times[r]
                say("  %s %9.2f us per image (min %.2f max %.2f over %d rounds)" % (r, med[r], min(t), max(t), len(t)))
            ratio = med[rows[3]] / med[rows[0]]
            say("  torch composition / three steps: %.2f%s" % (ratio, "" if ratio > 1 else "  -- THE COMPOSITION IS FASTER HERE"))
            del preds, grads, leaves, truths, targets
            torch.cuda.empty_cache()
    merger.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
