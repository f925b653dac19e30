"""What the sigmoid on load costs the sweep, and what it saves (one process, one context):
    python tests/tools/gpu_logits_sweep_time.py [repetitions, default 3]
Everything at 1024x2048, C=9, O=10, 4 input sets in rotation (beyond the 256 MB Infinity Cache), float32 and bfloat16:
  (a) the sweep on probabilities                       Merger.sweep_time, back-to-back launches
  (b) the sweep on logits (MN_MAPS_LOGITS)             the same, logits=True
  (c) Merger.prepare(x, apply_sigmoid=True) at unchanged size over the [C+O] planes: the pass (b) makes
      unnecessary, HIP events around back-to-back calls (the output tensor comes from the caching allocator)
  (d) torch.sigmoid over the same planes, the pass examples/pspnet_pipeline.py runs without --logits (informational)
(a) .. (d) alternate inside every repetition, so that a drift of the clocks shows in all of them.  A library or binding
without the flag (the commit before it, also as MN_LIB=<its build>) runs (a), (c), (d) and the probability half of the
record below.
Then, informational: tied_steps / tied_conflicts / proof of MN_MODE_EXACT on the bfloat16 blurred (radius 2) 256x512
map, as logits and as the bfloat16 probabilities rounded from the same logits (what a caller had to pass before)."""
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def logit(p):
    """log(p) - log1p(-p) in float64 on the device (+inf where synth writes 1.0)."""
    import torch
    p = p.double()
    return torch.log(p) - torch.log1p(-p)


def main():
    import torch
    from mergenet_amd import synth, segmenter as seg
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    H, W, C = 1024, 2048, 9
    offs = synth.generate_offsets(40, 10)
    O = len(offs)
    have_logits = "logits" in inspect.signature(seg.Merger.sweep_time).parameters
    if have_logits:                      # (MN_LIB may name a build from before the flag: it refuses the dtype)
        probe = seg.Merger(8, 8, C, O)
        z = torch.zeros((C + O, 8, 8), device="cuda")
        try:
            probe.sweep(z[:C], z[C:], offs, logits=True)
        except seg.MergeNetError:
            have_logits = False
        probe.close()
    print("%s: logits %s" % (seg.LIB_PATH, "available" if have_logits else "NOT available: (b) not measured"), flush=True)
    sets = {"float32": [], "bfloat16": []}          # per dtype: (probabilities [C+O,H,W], logits [C+O,H,W])
    for i in range(4):
        im = synth.synth_v1(H, W, C, offs, 1000 + i)
        p = torch.cat([torch.from_numpy(im.class_probs), torch.from_numpy(im.sameness_probs)]).cuda()
        x = logit(p)
        sets["float32"].append((p.contiguous(), x.float().contiguous()))
        sets["bfloat16"].append((p.to(torch.bfloat16).contiguous(), x.float().to(torch.bfloat16).contiguous()))
        del im
    m = seg.Merger(H, W, C, O)
    o = seg.default_options(merge_logprob_bias=0.03)

    def events(fn, n=100):
        for i in range(10):
            fn(i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    rows = {}
    for rep in range(reps):
        for dt in ("float32", "bfloat16"):
            ps = [(p[:C], p[C:]) for p, _ in sets[dt]]
            xs = [(x[:C], x[C:]) for _, x in sets[dt]]
            rows.setdefault(("a sweep, probabilities", dt), []).append(m.sweep_time(ps, offs, o, reps=400))
            if have_logits:
                rows.setdefault(("b sweep, logits", dt), []).append(m.sweep_time(xs, offs, o, reps=400, logits=True))
            full = [x for _, x in sets[dt]]
            rows.setdefault(("c prepare(apply_sigmoid), same dtype out", dt), []).append(
                events(lambda i: m.prepare(full[i % 4], H, W, apply_sigmoid=True, clip=True, out_dtype=full[0].dtype)))
            rows.setdefault(("d torch.sigmoid", dt), []).append(events(lambda i: torch.sigmoid(full[i % 4])))
    print("us per launch at %dx%d, C=%d, O=%d, 4 input sets in rotation; one column per repetition" % (H, W, C, O))
    for (what, dt), r in sorted(rows.items()):
        print("  (%s) %-9s %s   min %.2f max %.2f" % (what, dt, " ".join("%8.2f" % v for v in r), min(r), max(r)))
    for dt in ("float32", "bfloat16"):
        a, c = rows[("a sweep, probabilities", dt)], rows[("c prepare(apply_sigmoid), same dtype out", dt)]
        line = "  %-9s (a) + (c) = %.2f us (minima)" % (dt, min(a) + min(c))
        if have_logits:
            b = rows[("b sweep, logits", dt)]
            line += "; (b) = %.2f us: %s" % (min(b), "below" if max(b) < min(a) + min(c) else "NOT below")
        print(line)
    m.close()
    del sets

    # ---- ties: 16-bit logits against 16-bit probabilities of the same network output ----
    H, W = 256, 512
    im = synth.blurred_v1(H, W, C, offs, 8001, radius=2)
    x = logit(torch.cat([torch.from_numpy(im.class_probs), torch.from_numpy(im.sameness_probs)]).cuda())
    x = x.float().to(torch.bfloat16).contiguous()
    p = torch.sigmoid(x.float()).to(torch.bfloat16).contiguous()        # what autocast leaves behind the sigmoid
    m = seg.Merger(H, W, C, O)
    o = seg.default_options(mode=seg.MN_MODE_EXACT)
    forms = [("bfloat16 probabilities", p, {})] + ([("bfloat16 logits", x, dict(logits=True))] if have_logits else [])
    for what, t, kw in forms:
        _, _, _, st = m.segment(t[:C], t[C:], offs, o, **kw)
        print("blurred (radius 2) %dx%d seed 8001, MN_MODE_EXACT, %-22s: tied_steps %d tied_conflicts %d proof %d "
              "(instances %d, distinct sameness values %d)" %
              (H, W, what, st["tied_steps"], st["tied_conflicts"], st["proof"], st["num_instances"],
               int(torch.unique((torch.sigmoid(t[C:].float()) if kw else t[C:].float())).numel())))
    m.close()


if __name__ == "__main__":
    main()
