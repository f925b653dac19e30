"""16-bit probability maps for the tests: quantisation in numpy, the twelve tests/golden/lowp_*.npz vectors.

numpy has no bfloat16, so both formats travel as their uint16 bit patterns plus the float32 values those
patterns widen to (widening is exact).  The stored expected results come from the reference's own merger run
on the WIDENED values: quantising makes a different input, whose result is not that of the float32 maps.
"""
import hashlib
import json
import os

import numpy as np

from mergenet_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = ("float16", "bfloat16")
OPTS = (0.0, 1.0, 0.03)          # same_different_bias, object_merge_factor, merge_logprob_bias
SHAPE = dict(H=64, W=128, C=9, offsets=[40, 10])


def quantize(a, dtype):
    """float array -> (uint16 bit patterns, float32 widening) of its round-to-nearest-even 16-bit values."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "float16":
        h = a.astype(np.float16)
        return h.view(np.uint16).copy(), h.astype(np.float32)
    if dtype != "bfloat16":
        raise ValueError(dtype)
    u = a.view(np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = np.where(nan, (u >> np.uint64(16)) | np.uint64(0x0040), r)
    bits = r.astype(np.uint16)
    return bits, widen(bits, dtype)


def widen(bits, dtype):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "float16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def unit_interval_patterns(dtype):
    """Every bit pattern whose value lies in [0, 1]: +0 .. 1.0 (subnormals included)."""
    one = 0x3C00 if dtype == "float16" else 0x3F80
    return np.arange(0, one + 1, dtype=np.uint16)


def to_torch(bits, dtype, device=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16))
    t = t.view(torch.float16 if dtype == "float16" else torch.bfloat16)
    return t.to(device).contiguous() if device is not None else t


def torch_dtype(dtype):
    import torch
    return torch.float16 if dtype == "float16" else torch.bfloat16


def confident(H, W, C, offs, seed):
    """Saturated maps: logits +18 / -18 by the side of 0.5 the synth-v1 value lies on, plus a uniform
    (-1, 1) term; sigmoid in float64, then float32.  In 16 bits most of them are exactly 1.0 (and, in
    float16, exactly 0.0 or subnormal): the always-on clip, exact widening and massive ties."""
    s = synth.synth_v1(H, W, C, offs, seed, num_instances=4)

    def planes(p, stream):
        u = synth.uniform01(seed, stream, p.size).astype(np.float64).reshape(p.shape)
        logit = np.where(p > 0.5, 18.0, -18.0) + (2.0 * u - 1.0)
        return (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)

    return planes(s.class_probs, 101), planes(s.sameness_probs, 102)


def specs():
    out = []
    for kind, seeds in (("synth", (1001, 1003)), ("blur", (8001, 8002)), ("confident", (1001, 1003))):
        for seed in seeds:
            for dtype in DTYPES:
                sp = dict(SHAPE, name="lowp_%s_s%d_%s" % (kind, seed, "f16" if dtype == "float16" else "bf16"),
                          kind=kind, seed=seed, dtype=dtype, num_instances=4, opts=list(OPTS))
                if kind == "blur":
                    sp.update(radius=2, noise=0.05)
                out.append(sp)
    return out


def names():
    return [s["name"] for s in specs()]


def float_inputs(spec):
    offs = synth.generate_offsets(*spec["offsets"])
    H, W, C = spec["H"], spec["W"], spec["C"]
    if spec["kind"] == "synth":
        s = synth.synth_v1(H, W, C, offs, spec["seed"], num_instances=spec["num_instances"])
        return s.class_probs, s.sameness_probs, offs
    if spec["kind"] == "blur":
        s = synth.blurred_v1(H, W, C, offs, spec["seed"], radius=spec["radius"], noise=spec["noise"],
                             num_instances=spec["num_instances"])
        return s.class_probs, s.sameness_probs, offs
    cp, sp = confident(H, W, C, offs, spec["seed"])
    return cp, sp, offs


def quantized_inputs(spec):
    """dict: class_bits / same_bits (uint16), class_probs / sameness_probs (their float32 widening), offsets."""
    cp, sp, offs = float_inputs(spec)
    cb, cw = quantize(cp, spec["dtype"])
    sb, sw = quantize(sp, spec["dtype"])
    return dict(class_bits=cb, same_bits=sb, class_probs=cw, sameness_probs=sw, offsets=offs)


def digest(class_bits, same_bits):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(class_bits).tobytes())
    h.update(np.ascontiguousarray(same_bits).tobytes())
    return h.hexdigest()


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    spec = json.loads(str(z["spec"]))
    q = quantized_inputs(spec)
    assert digest(q["class_bits"], q["same_bits"]) == str(z["sha256"]), \
        "a 16-bit rounding of the generator moved: regenerate with tests/golden/make_golden_lowp.py"
    q.update(spec=spec, dtype=spec["dtype"], opts=tuple(spec["opts"]), mask=z["mask"],
             object_class=[int(c) for c in z["object_class"]])
    return q
