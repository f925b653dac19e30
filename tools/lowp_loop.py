#!/usr/bin/env python
"""A loop of fast-path calls on bfloat16 (or float16 / float32) maps, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/lowp_loop.py [N] [--dtype bfloat16]

1024x2048, C = 9, O = 10, synth-v1 seeds 1000-1003 quantised, N images (default 24) through two contexts in
turn on one stream (the launch of image i+1 precedes the read-back of image i), speculative fast path
(require_proof = -1).  The trace lists the kernels of the float32 loop, the sweep in its 16-bit form, and no
conversion kernel: the maps are read in the width they have."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("images", nargs="?", type=int, default=24)
    ap.add_argument("--dtype", choices=["bfloat16", "float16", "float32"], default="bfloat16")
    args = ap.parse_args()
    import torch
    import lowp_util
    from mergenet_amd import segmenter as seg, synth
    H, W, C = 1024, 2048, 9
    offs = synth.generate_offsets(40, 10)
    ins = []
    for seed in range(1000, 1004):
        im = synth.synth_v1(H, W, C, offs, seed)
        if args.dtype == "float32":
            ins.append((torch.from_numpy(im.class_probs).cuda(), torch.from_numpy(im.sameness_probs).cuda()))
        else:
            ins.append((lowp_util.to_torch(lowp_util.quantize(im.class_probs, args.dtype)[0], args.dtype, "cuda"),
                        lowp_util.to_torch(lowp_util.quantize(im.sameness_probs, args.dtype)[0], args.dtype, "cuda")))
    mergers = [seg.Merger(H, W, C, len(offs)) for _ in range(2)]
    o = seg.default_options(require_proof=-1, debug_flags=seg.MN_DEBUG_LEAN_EVENTS)
    pending = None
    proofs = {}
    for i in range(args.images):
        nxt = mergers[i % 2].segment_async(ins[i % 4][0], ins[i % 4][1], offs, o)
        if pending is not None:
            st = pending.result()[3]
            proofs[st["proof"]] = proofs.get(st["proof"], 0) + 1
        pending = nxt
    st = pending.result()[3]
    proofs[st["proof"]] = proofs.get(st["proof"], 0) + 1
    torch.cuda.synchronize()
    print("%d images in %s: mode_used %d, %d instances, proof counts %s" %
          (args.images, args.dtype, st["mode_used"], st["num_instances"], proofs))
    for m in mergers:
        m.close()


if __name__ == "__main__":
    main()
