"""The lean form of what the sweep leaves (packed edge masks, one record per uniform 64-pixel group) against the full
form inside one build: ``debug_flags |= MN_DEBUG_SWEEP_FULL_FORM`` keeps the full form on the components path, and everything a call
returns -- mask, class table with its -1 padding, partition, every counter of the stats, ``total_logprob`` -- must be
equal, bit for bit.  The class sums are integer sums, so there is no tolerance anywhere in this file.

Every case asserts ``mode_used == 3`` (the comparison proves nothing on a call that left the components path), and --
with labels.uniform_groups on the positive masks the full-form sweep exports -- that a case meant to have uniform
groups has some and a case meant to have none has none.

Inputs are built from a label map (lean_util.maps_from_labels: sameness 0.95 inside a label, 0.05 across, class maps
peaked on the label's class) or, where stated, by synth_v1.
"""
import numpy as np
import pytest
import torch

import lean_util
import lowp_util
from mergenet_amd import labels, segmenter as seg, synth
from test_gpu_lowp import STATS

pytestmark = pytest.mark.gpu

FULL = seg.MN_DEBUG_SWEEP_FULL_FORM            # the full form on the product path
OFFS10 = [tuple(int(x) for x in o) for o in synth.generate_offsets(40, 10)]


def _result(out):
    mask, table, part, st = out
    torch.cuda.synchronize()
    return dict(mask=mask.cpu().numpy(), table=table.cpu().numpy(),
                part=part.cpu().numpy() if part is not None else None, stats=st)


def _assert_equal(got, want, what):
    assert got["stats"]["status"] == want["stats"]["status"] == 0, what
    assert got["stats"]["mode_used"] == want["stats"]["mode_used"] == seg.MN_MODE_COMPONENTS, (what, got["stats"])
    assert np.array_equal(got["mask"], want["mask"]), what
    assert np.array_equal(got["table"], want["table"]), what           # (the -1 padding included)
    if got["part"] is not None and want["part"] is not None:
        assert np.array_equal(got["part"], want["part"]), what
    for k in STATS + ["rounds", "initial_records"]:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])
    a, b = got["stats"]["total_logprob"], want["stats"]["total_logprob"]
    assert a == b or (np.isnan(a) and np.isnan(b)), (what, a, b)


def _device(a, dtype="float32"):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "float32":
        return torch.from_numpy(a).cuda()
    bits, _ = lowp_util.quantize(a, dtype)
    return lowp_util.to_torch(bits, dtype, "cuda")


def _both(cp, sp, offs, dtype="float32", logits=False, flags=0, sweep_flags=0, **opts):
    """(lean result, full result, sweep export of the full form) of one call, in a fresh context each."""
    C, H, W = cp.shape
    d = (_device(cp, dtype), _device(sp, dtype))
    out = []
    for extra in (0, FULL):
        m = seg.Merger(H, W, C, len(offs))
        try:
            o = seg.default_options(mode=seg.MN_MODE_COMPONENTS, require_proof=-1, debug_flags=flags | extra, **opts)
            out.append(_result(m.segment(d[0], d[1], offs, o, want_partition=True, logits=logits)))
        finally:
            m.close()
    m = seg.Merger(H, W, C, len(offs))
    try:
        so = seg.default_options(debug_flags=sweep_flags, **{k: v for k, v in opts.items()
                                                           if k in ("same_different_bias", "clip_inputs")})
        sw = m.sweep(d[0], d[1], offs, so, logits=logits)
        sw = dict(sw, bits=sw["bits"].cpu().numpy().view(np.uint32))
    finally:
        m.close()
    return out[0], out[1], sw


def _flags(sw, offs):
    return labels.uniform_groups(sw["bits"], offs)


def _synth(H, W, C, offs, seed, k):
    s = synth.synth_v1(H, W, C, offs, seed, num_instances=k)
    return s.class_probs, s.sameness_probs


def _two_instances(H, W):
    """Background, one instance in the left half, one in the right: runs of links longer than 64 pixels."""
    lab = np.zeros((H, W), np.int32)
    lab[2:H - 2, 3:W // 2 - 2] = 1
    lab[3:H - 1, W // 2 + 1:W - 1] = 2
    return lab


# ---- uniform groups exist ---------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,C,k", [(32, 256, 9, 4), (24, 192, 1, 3), (32, 256, 17, 4)])
def test_uniform_groups_synth(H, W, C, k):
    """synth_v1.  C = 1: one class plane.  C = 17: the class loop of the sums kernel takes a second round of 9."""
    cp, sp = _synth(H, W, C, OFFS10, 1000 + C, k)
    lean, full, sw = _both(cp, sp, OFFS10)
    f = _flags(sw, OFFS10)
    print("%dx%d C=%d: %d of %d groups uniform" % (H, W, C, f.sum(), f.size))
    assert sw["pixels_per_lane"] == 4
    assert f.any() and not f.all()
    _assert_equal(lean, full, (H, W, C))


def test_last_partial_group():
    """17 x 68: N % 64 == 4 -- a last group of one lane, which is never uniform -- beside groups that are."""
    H, W = 17, 68
    lab = np.zeros((H, W), np.int32)
    lab[4:12, 1:W - 1] = 1
    cp, sp = lean_util.maps_from_labels(lab, {0: 0, 1: 3}, 9, OFFS10)
    lean, full, sw = _both(cp, sp, OFFS10)
    f = _flags(sw, OFFS10)
    assert np.array_equal(sw["bits"], lean_util.pos_bits_of(lab, OFFS10))
    assert f.any() and not f[-1] and (H * W) % 64 == 4
    _assert_equal(lean, full, "17x68")


# ---- no group may be uniform --------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,px", [(24, 100, 4),      # W % 4 == 0, groups cross the rows' ends
                                    (30, 66, 4),       # N % 4 == 0, W % 4 != 0: straddling lanes
                                    (17, 64, 4),       # a group is a row
                                    (9, 13, 1)])       # N % 4 != 0: one pixel per lane, the full form throughout
def test_no_uniform_group(H, W, px):
    lab = lean_util.stripes(H, W, 20)
    cp, sp = lean_util.maps_from_labels(lab, {0: 0, 1: 2, 2: 5, 3: 1}, 9, OFFS10)
    lean, full, sw = _both(cp, sp, OFFS10)
    assert sw["pixels_per_lane"] == px
    assert not _flags(sw, OFFS10).any()
    _assert_equal(lean, full, (H, W))


def test_rows_end_inside_whole_labels():
    """24 x 100 with wide labels: the groups inside a row are uniform, those across a row's end are not."""
    lab = np.zeros((24, 100), np.int32)
    lab[2:22, 3:97] = 1
    cp, sp = lean_util.maps_from_labels(lab, {0: 0, 1: 4}, 9, OFFS10)
    lean, full, sw = _both(cp, sp, OFFS10)
    f = _flags(sw, OFFS10)
    for g in np.nonzero(f)[0]:
        assert (64 * g) // 100 == (64 * g + 63) // 100
    assert f.any() and not f.all()
    _assert_equal(lean, full, "24x100 wide")


def test_offsets_without_the_unit_step():
    """No (0, +1) in the list: no group is uniform, whatever the maps (the labelling has only its vertical unit)."""
    offs = [(1, 0), (0, 2), (2, 1), (0, 3)]
    lab = _two_instances(32, 256)
    cp, sp = lean_util.maps_from_labels(lab, {0: 0, 1: 2, 2: 6}, 9, offs)
    lean, full, sw = _both(cp, sp, offs)
    assert not _flags(sw, offs).any()
    _assert_equal(lean, full, "no (0,1)")


# ---- packing limit --------------------------------------------------------------------------------------------

def _half_plane(n):
    """n offsets of the upper half plane, (0, 1) and (1, 0) first: no offset together with its negation."""
    rest = [(i, j) for i in range(0, 5) for j in range(-4, 5) if (i > 0 or j > 1) and (i, j) != (1, 0)]
    return ([(0, 1), (1, 0)] + rest)[:n]


@pytest.mark.parametrize("O", [16, 17, 32])
def test_packing_limit(O):
    """O = 16: both masks share a word and bit 15 -- next to the negative half -- is in use.  O = 17, 32: two arrays."""
    offs = _half_plane(O)
    assert len(offs) == O
    synth.validate_offsets(offs)
    lab = _two_instances(32, 256)
    cp, sp = lean_util.maps_from_labels(lab, {0: 0, 1: 2, 2: 6}, 9, offs)
    lean, full, sw = _both(cp, sp, offs)
    top = (sw["bits"] >> np.uint32(O - 1)) & 1
    assert top.any() and not top.all()                     # the highest offset has positive edges
    assert np.isfinite(sw["neg"][O - 1].cpu().numpy()).any()   # ... and negative ones
    assert _flags(sw, offs).any()
    _assert_equal(lean, full, O)


# ---- non-flat parents -------------------------------------------------------------------------------------------

def test_non_flat_parents(oracle):
    """One instance of two blobs five background columns apart, joined only by offset (0, 9): the hook hangs the
    second blob's root -- 192 columns wide from column 64 on, so it holds whole uniform groups, and with the larger
    pixel ids -- under the first one's, and its pixels stay two steps from their root.  A second instance beside it
    gives mn_cc_cross records with such an end."""
    offs = [(1, 0), (0, 1), (0, 9)]
    H, W = 8, 320
    lab = np.zeros((H, W), np.int32)
    lab[2:6, 4:59] = 1
    lab[2:6, 64:256] = 1
    lab[2:6, 256:300] = 2
    cp, sp = lean_util.maps_from_labels(lab, {0: 0, 1: 3, 2: 5}, 9, offs)
    lean, full, sw = _both(cp, sp, offs, clip_inputs=1)
    f = _flags(sw, offs).reshape(H, W // 64)
    assert f[2:6, 1:4].all()                               # the second blob's groups are uniform
    _assert_equal(lean, full, "two blobs")
    assert lean["stats"]["num_instances"] == 2
    m = lean["mask"]
    assert m[3, 10] == m[3, 100] != 0 and m[3, 270] not in (0, m[3, 10]) and m[3, 61] == 0
    o = seg.default_options()
    ref = oracle.run_csegment(cp, sp, 9, offs, o.same_different_bias, o.object_merge_factor, o.merge_logprob_bias)
    got_cls = [int(c) for c in lean["table"][: lean["stats"]["num_instances"]]]
    assert oracle.masks_equivalent(lean["mask"], got_cls, ref.mask, ref.object_class)


# ---- forms of the sweep ---------------------------------------------------------------------------------------------

def _logit32(p):
    p = p.astype(np.float64)
    with np.errstate(divide="ignore"):
        return (np.log(p) - np.log1p(-p)).astype(np.float32)          # (+inf where an edge leaves the image)


@pytest.mark.parametrize("form", ["bfloat16_px8", "float16_px4", "logits", "bias", "clip"])
def test_forms_of_the_sweep(form):
    H, W, C = 32, 256, 9
    cp, sp = _synth(H, W, C, OFFS10, 1009, 4)
    kw = dict(bfloat16_px8=dict(dtype="bfloat16"),
              float16_px4=dict(dtype="float16", flags=seg.MN_DEBUG_SWEEP16_4PX, sweep_flags=seg.MN_DEBUG_SWEEP16_4PX),
              logits=dict(logits=True), bias=dict(same_different_bias=0.1), clip=dict(clip_inputs=1))[form]
    if form == "logits":
        cp, sp = _logit32(cp), _logit32(sp)
    lean, full, sw = _both(cp, sp, OFFS10, **kw)
    assert sw["pixels_per_lane"] == (8 if form == "bfloat16_px8" else 4)
    f = _flags(sw, OFFS10)
    assert f.any() and not f.all()
    _assert_equal(lean, full, form)


# ---- replay -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [0, FULL])
def test_replay_through_fixed_buffers(extra):
    """debug_flags 16 | 32: four calls through the same buffers (recorded at the second, replayed from the third) give
    what the plain call gives -- in the lean form, and in the full form under bit 9 (its own replay key)."""
    H, W, C = 32, 256, 9
    cp, sp = _synth(H, W, C, OFFS10, 1011, 4)
    d = (_device(cp), _device(sp))
    m = seg.Merger(H, W, C, len(OFFS10))
    try:
        plain = seg.default_options(mode=seg.MN_MODE_COMPONENTS, require_proof=-1, debug_flags=FULL)
        want = _result(m.segment(d[0], d[1], OFFS10, plain))
        out = (torch.empty((H, W), dtype=torch.int32, device="cuda"), torch.empty((H * W,), dtype=torch.int32, device="cuda"))
        o = seg.default_options(mode=seg.MN_MODE_COMPONENTS, require_proof=-1,
                                debug_flags=seg.MN_DEBUG_LEAN_EVENTS | seg.MN_DEBUG_REPLAY | extra)
        for i in range(4):
            out[0].fill_(-7)
            got = _result(m.segment_async(d[0], d[1], OFFS10, o, out=out).result())
            _assert_equal(got, want, ("replay", extra, i))
    finally:
        m.close()
