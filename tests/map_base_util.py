"""The case table of test_map_base.py and test_gpu_map_base.py: where the class and sameness maps of a call start.

Every entry point that takes an image accepts its maps at any element-aligned address, and the kernels behind them
read through 8- and 16-byte loads.  The table is the smallest shapes at which each form of the sweep (mn_sweep_form.h)
exists, the three element types, and -- per element type -- the bases a caller can hand in, counted in bytes behind a
16-byte boundary, for the class maps, for the sameness maps and for both.

Inputs are label maps of topology_util turned into maps by lean_util.maps_from_labels; with the options (0, 1, 0)
nothing merges after the first phase and the expected partition is exactly topology_util.components.  The 16-bit maps
are lowp_util.quantize of the float32 ones, and every reference runs on their exact widening.

The expected pixels per lane (PX_*) are written out by hand from the rule in mn_sweep_form.h, one literal per row; the
function under test computes none of them.

CPU only; torch is imported where a function needs it.
"""
import functools

import numpy as np

import lean_util
import lowp_util
import topology_util as tu

OPTS = (0.0, 1.0, 0.0)
DTYPES = ("float32", "float16", "bfloat16")

# Bytes behind a 16-byte boundary.
OFFSETS = {"float32": (4, 8, 12), "float16": (2, 4, 8, 14), "bfloat16": (2, 4, 8, 14)}


def pairs(dtype):
    """(class base, sameness base) of every call: the aligned pair, then per offset b the pairs (b, 0), (0, b) and
    (b, b') with b' the next offset of the list (b' != b)."""
    offs = OFFSETS[dtype]
    out = [(0, 0)]
    for i, b in enumerate(offs):
        out += [(b, 0), (0, b), (b, offs[(i + 1) % len(offs)])]
    return out


def edge_pairs(dtype):
    """(b, 0) and (0, b) for the smallest and the largest b."""
    lo, hi = OFFSETS[dtype][0], OFFSETS[dtype][-1]
    return [(lo, 0), (0, lo), (hi, 0), (0, hi)]


# ---- shapes ----------------------------------------------------------------------------------------------------------
#
# SHAPES[name] makes the label map; the comment says what N and W are modulo the load widths.  Expected pixels per lane,
# by hand from mn_sweep_form.h:
#   N % 4 != 0 or W < 4                                   -> 1
#   float32 otherwise                                     -> 4, whatever the bases
#   16 bits, N % 8 == 0 and W % 8 == 0, BOTH bases % 16 == 0 (and not MN_DEBUG_SWEEP16_4PX)  -> 8
#   16 bits otherwise                                     -> 4
# PX[name] = (float32, 16 bits with both bases aligned, 16 bits with a base off a 16-byte boundary)
#
# The two last shapes are the control, one pixel per lane and scalar loads.  Random labels leave 4046 records between
# their components, more than the 1024 the speculative tail takes, so the library redoes their `tail` attempt on the
# waited one; the serpentine of the same size has few records and reaches mn_cc_tail from scalar loads too.
SHAPES = {
    "comb3-32x136":         lambda: tu.comb(32, 136, False, teeth=3),     # N = 4352: N % 8 == 0, W % 8 == 0
    "serpentine-1-1-17x68": lambda: tu.serpentine(17, 68, 1, 1),          # N = 1156: N % 8 == 4, W % 4 == 0
    "serpentine-2-2-34x66": lambda: tu.serpentine(34, 66, 2, 2),          # N = 2244: N % 4 == 0, W % 4 == 2
    "serpentine-1-1-18x4":  lambda: tu.serpentine(18, 4, 1, 1),           # N = 72: one lane per row
    "serpentine-1-1-18x8":  lambda: tu.serpentine(18, 8, 1, 1),           # N = 144: the smallest 8 pixels per lane
    "percolation-35x68":    lambda: tu.percolation(35, 68, 0.6, 7),       # N = 2380: N % 8 == 4; many negative edges
    "random3-35x131":       lambda: tu.random_labels(35, 131, 3, 11),     # N = 4585: N % 4 != 0, scalar loads
    "serpentine-1-1-35x131": lambda: tu.serpentine(35, 131, 1, 1),        # N = 4585 again, few records
}
PX = {
    "comb3-32x136":         (4, 8, 4),
    "serpentine-1-1-17x68": (4, 4, 4),
    "serpentine-2-2-34x66": (4, 4, 4),
    "serpentine-1-1-18x4":  (4, 4, 4),
    "serpentine-1-1-18x8":  (4, 8, 4),
    "percolation-35x68":    (4, 4, 4),
    "random3-35x131":       (1, 1, 1),
    "serpentine-1-1-35x131": (1, 1, 1),
}
PX_16_4PX = {"comb3-32x136": 4}          # under MN_DEBUG_SWEEP16_4PX, 16 bits, every pair of bases
HW = {"comb3-32x136": (32, 136), "serpentine-1-1-17x68": (17, 68), "serpentine-2-2-34x66": (34, 66),
      "serpentine-1-1-18x4": (18, 4), "serpentine-1-1-18x8": (18, 8), "percolation-35x68": (35, 68),
      "random3-35x131": (35, 131), "serpentine-1-1-35x131": (35, 131)}


def expected_px(shape, dtype, pair, sweep16_4px=False):
    """The table's pixels per lane of one row (a look-up, no rule)."""
    f32, lowp_aligned, lowp_off = PX[shape]
    if dtype == "float32":
        return f32
    if sweep16_4px:
        return PX_16_4PX[shape]
    return lowp_aligned if pair == (0, 0) else lowp_off


CASE_SHAPE = {}          # case name -> name of its shape in SHAPES


def _cases():
    out = []
    for shape, make in SHAPES.items():
        lists = [("unit", tu.UNIT), ("up", tu.UNIT_UP)]
        if shape == "percolation-35x68":
            lists.append(("real", tu.REAL))
        for tag, offs in lists:
            c = tu.Case("%s-%s" % (shape, tag), make, offs)
            CASE_SHAPE[c.name] = shape
            out.append(c)
    return out


def shape_of(case):
    return CASE_SHAPE[case.name]


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FIRST_OF_SHAPE = {shape: next(c for c in CASES if shape_of(c) == shape) for shape in SHAPES}


# ---- inputs and references ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def host_maps(name, dtype):
    """(class values, sameness values, class bits | None, sameness bits | None): the float32 values the kernels see
    (for a 16-bit dtype the exact widening of the quantised maps) and the uint16 patterns that travel."""
    case = BY_NAME[name]
    cp, sp = lean_util.maps_from_labels(case.lab, tu.CLASS_OF_LABEL, tu.C, case.offs)
    if dtype == "float32":
        out = (cp, sp, None, None)
    else:
        cb, cw = lowp_util.quantize(cp, dtype)
        sb, sw = lowp_util.quantize(sp, dtype)
        out = (cw, sw, cb, sb)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_logits(name, dtype):
    """The same maps as logits: log(p / (1 - p)) in float64 of the float32 maps, rounded to the dtype (+inf where an
    edge leaves the image).  (logit values float32 -- widened for 16 bits --, uint16 patterns | None) per map."""
    case = BY_NAME[name]
    out = []
    for p in lean_util.maps_from_labels(case.lab, tu.CLASS_OF_LABEL, tu.C, case.offs):
        p = p.astype(np.float64)
        with np.errstate(divide="ignore"):
            x = (np.log(p) - np.log1p(-p)).astype(np.float32)
        if dtype == "float32":
            out.append((x, None))
        else:
            bits, wide = lowp_util.quantize(x, dtype)
            out.append((wide, bits))
    (cx, cb), (sx, sb) = out
    for a in (cx, sx, cb, sb):
        if a is not None:
            a.setflags(write=False)
    return cx, sx, cb, sb


def probabilities_of_logits(x):
    """float32 1 / (1 + exp(-x)), each operation in float64 and one rounding at the end (the kernels take it in
    float32: a few ulp of a term apart, far inside the 1e-5 of total_logprob)."""
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(mask, classes, number of components) of the union-find labelling."""
    case = BY_NAME[name]
    mask, classes = tu.reference_mask(case.comp, case.lab, tu.CLASS_OF_LABEL)
    mask.setflags(write=False)
    return mask, classes, tu.count(case.comp)


# ---- tensors at a given base -----------------------------------------------------------------------------------------------

GUARD = 16          # elements on either side of a view (a multiple of 16 bytes for every element size used here)


def at_base_guarded(t, nbytes, fill=0):
    """(view, buffer, first element of the view in the buffer): a contiguous copy of the device tensor `t` that starts
    `nbytes` behind a 16-byte boundary, inside a buffer filled with `fill` that reaches GUARD elements and more past
    either end of it."""
    import torch
    assert 0 <= nbytes < 16 and nbytes % t.element_size() == 0
    start = GUARD + nbytes // t.element_size()
    buf = torch.full((t.numel() + 3 * GUARD,), fill, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf, start


def at_base(t, nbytes):
    """test_gpu_map_scores.off_base for any element-multiple byte count: `t` on the device, contiguous, `nbytes`
    behind a 16-byte boundary."""
    view = at_base_guarded(t, nbytes)[0]
    assert view.data_ptr() % 16 == nbytes and view.is_contiguous()
    return view


def guards_hold(buf, start, numel, fill):
    """Both GUARD-element stretches around elements start .. start + numel - 1 of `buf` still hold `fill`."""
    before, after = buf[start - GUARD:start], buf[start + numel:start + numel + GUARD]
    return bool((before == fill).all().item()) and bool((after == fill).all().item())


def to_device(values, bits, dtype):
    """The map on the device in its element type: the float32 values, or the 16-bit patterns."""
    import torch
    if dtype == "float32":
        return torch.from_numpy(np.array(values, order="C")).cuda()
    return lowp_util.to_torch(np.array(bits, order="C"), dtype, "cuda")
