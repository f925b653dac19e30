"""Merger.tile_class_maps / mn_tile_class_maps_device on the GPU: the class planes of an image from the logits of a
tiled semantic network, against tiles.tile_class_maps_reference (float64), bit-exact where the contract says so, and end
to end into the merger."""
import ctypes
import functools

import numpy as np
import pytest

from mergenet_amd import tiles as mt
from tiles_util import CASES, make_case, tolerance

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def merger():
    from mergenet_amd import segmenter as seg
    m = seg.Merger(48, 64, 4, 6)            # the capacity says nothing here: the call works at any image size
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs on the host, float64 reference): computed once, shared, never written to."""
    inputs = make_case(name)
    ref = mt.tile_class_maps_reference(*inputs)
    ref.setflags(write=False)
    return inputs, ref


def on_gpu(name, dtype=None):
    import torch
    (tiles, flips, rows, cols, H, W, C), _ = case(name)
    t = torch.from_numpy(tiles).cuda()
    f = None if flips is None else torch.from_numpy(flips).cuda()
    if dtype is not None:
        t = t.to(dtype)
        f = None if f is None else f.to(dtype)
    return t, f, rows, cols, H, W, C


def bits(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_float64_reference(merger, name):
    import torch
    t, f, rows, cols, H, W, C = on_gpu(name)
    _, ref = case(name)
    out = merger.tile_class_maps(t, f, rows, cols, H, W, C)
    assert out.shape == (C, H, W) and out.dtype == torch.float32 and out.device == t.device
    got = out.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    tol = tolerance(name)
    off_one = float(np.abs(got.sum(axis=0) - 1.0).max())
    print("case %s: max abs error %.3g (bound %.3g); planes sum to 1 within %.3g (bound %.3g)"
          % (name, err, tol, off_one, C * 2.0 ** -23))
    assert np.isfinite(got).all()
    assert err <= tol
    assert off_one <= C * 2.0 ** -23
    # two calls give identical bits
    again = merger.tile_class_maps(t, f, rows, cols, H, W, C)
    assert np.array_equal(bits(out), bits(again))


@pytest.mark.parametrize("name", ["a", "d", "f"])
def test_clip_is_the_clamp_of_the_unclipped_output(merger, name):
    t, f, rows, cols, H, W, C = on_gpu(name)
    plain = merger.tile_class_maps(t, f, rows, cols, H, W, C)
    clipped = merger.tile_class_maps(t, f, rows, cols, H, W, C, clip=True)
    want = plain.clamp(EPS, 1.0 - EPS)
    assert np.array_equal(bits(clipped), bits(want))
    if name == "d":      # saturated: the clamp changes something
        assert not np.array_equal(bits(clipped), bits(plain))


@pytest.mark.parametrize("name", ["a", "c", "f"])
@pytest.mark.parametrize("half", ["float16", "bfloat16"])
def test_sixteen_bit_output_is_the_rounded_float32_output(merger, name, half):
    import torch
    dt = getattr(torch, half)
    t, f, rows, cols, H, W, C = on_gpu(name)
    for clip in (False, True):
        full = merger.tile_class_maps(t, f, rows, cols, H, W, C, clip=clip)
        narrow = merger.tile_class_maps(t, f, rows, cols, H, W, C, out_dtype=dt, clip=clip)
        assert narrow.dtype == dt
        assert np.array_equal(bits(narrow), bits(full.to(dt)))


@pytest.mark.parametrize("name", ["a", "e", "f", "g", "h"])
@pytest.mark.parametrize("half", ["float16", "bfloat16"])
def test_sixteen_bit_tiles_are_widened_exactly(merger, name, half):
    import torch
    dt = getattr(torch, half)
    t, f, rows, cols, H, W, C = on_gpu(name, dt)
    got = merger.tile_class_maps(t, f, rows, cols, H, W, C, out_dtype=torch.float32)
    want = merger.tile_class_maps(t.float(), None if f is None else f.float(), rows, cols, H, W, C)
    assert np.array_equal(bits(got), bits(want))
    default = merger.tile_class_maps(t, f, rows, cols, H, W, C)          # out_dtype=None: the tiles' dtype
    assert default.dtype == dt and np.array_equal(bits(default), bits(want.to(dt)))


def test_the_maximum_follows_the_average(merger):
    """Stuff classes (0.8, 0.1) plain and (0.1, 0.8) flipped average to 0.45 each: plane 0 is 0.45 / 0.55, not what the
    greatest logit alone would give."""
    import torch
    a = torch.log(torch.tensor([0.8, 0.1, 0.1])).reshape(1, 3, 1, 1).contiguous().cuda()
    b = torch.log(torch.tensor([0.1, 0.8, 0.1])).reshape(1, 3, 1, 1).contiguous().cuda()
    out = merger.tile_class_maps(a, b, [0], [0], 1, 1, 2).cpu().numpy().reshape(2)
    assert np.abs(out - np.array([0.45, 0.1]) / 0.55).max() <= (3 + 1 + 2 + 8) * 2.0 ** -24


def test_the_flipped_pass_is_read_reversed(merger):
    """A flip tensor that is the plain one with its columns reversed changes nothing: (p + p) * 0.5 == p exactly."""
    t, _, rows, cols, H, W, C = on_gpu("e")
    plain = merger.tile_class_maps(t, None, rows, cols, H, W, C)
    both = merger.tile_class_maps(t, t.flip(-1).contiguous(), rows, cols, H, W, C)
    assert np.array_equal(bits(plain), bits(both))


def test_argument_errors_launch_nothing(merger):
    import torch
    from mergenet_amd import segmenter as seg
    t, f, rows, cols, H, W, C = on_gpu("a")
    T, Cn, th, tw = t.shape
    call = functools.partial(merger.tile_class_maps, t, f)
    bad = [
        dict(rows=rows, cols=cols, H=H, W=W - 1, C=C),                        # the last column tile leaves the image
        dict(rows=rows, cols=cols, H=H - 1, W=W, C=C),                        # the last row tile leaves the image
        dict(rows=[-1] + rows[1:], cols=cols, H=H, W=W, C=C),                 # a negative start
        dict(rows=rows, cols=cols, H=H, W=W + 1, C=C),                        # the last column uncovered
        dict(rows=rows, cols=[0, 0, 0, cols[-1]], H=H, W=W, C=C),             # columns 24..28 uncovered
        dict(rows=[1] + rows[1:], cols=cols, H=H, W=W, C=C),                  # row 0 uncovered
        dict(rows=rows, cols=cols, H=H, W=W, C=0),
        dict(rows=rows, cols=cols, H=H, W=W, C=Cn + 1),
        dict(rows=rows, cols=cols, H=0, W=W, C=C),
        dict(rows=rows, cols=cols, H=H, W=-3, C=C),
    ]
    for kw in bad:
        with pytest.raises(seg.MergeNetError) as e:
            call(kw["rows"], kw["cols"], kw["H"], kw["W"], kw["C"])
        assert e.value.status == -1, kw
    # more than 32 starts on an axis; more than 64 network classes
    many = torch.zeros((33, 2, 1, 4), device="cuda")
    with pytest.raises(seg.MergeNetError):
        merger.tile_class_maps(many, None, [0] * 33, [0], 1, 4, 2)
    with pytest.raises(seg.MergeNetError):
        merger.tile_class_maps(many, None, [0], [0] * 33, 1, 4, 2)
    wide = torch.zeros((1, 65, 2, 2), device="cuda")
    with pytest.raises(seg.MergeNetError):
        merger.tile_class_maps(wide, None, [0], [0], 2, 2, 3)

    # what the method cannot express: null pointers, unknown dtypes, the logits flag, non-positive tile sizes
    fn = merger.lib.mn_tile_class_maps_device
    out = torch.empty((C, H, W), device="cuda")
    r = (ctypes.c_int * len(rows))(*rows)
    c = (ctypes.c_int * len(cols))(*cols)
    good = dict(ctx=merger.handle, tiles=t.data_ptr(), flip=f.data_ptr(), dtype=0, Cn=Cn, th=th, tw=tw, rows=r,
                nr=len(rows), cols=c, nc=len(cols), H=H, W=W, C=C, out=out.data_ptr(), out_dtype=0, clip=0, stream=None)

    def raw(**change):
        a = dict(good, **change)
        return fn(a["ctx"], a["tiles"], a["flip"], a["dtype"], a["Cn"], a["th"], a["tw"], a["rows"], a["nr"], a["cols"],
                  a["nc"], a["H"], a["W"], a["C"], a["out"], a["out_dtype"], a["clip"], a["stream"])

    for change in (dict(ctx=None), dict(tiles=None), dict(out=None), dict(rows=None), dict(cols=None),
                   dict(dtype=3), dict(out_dtype=7), dict(dtype=-1),
                   dict(dtype=seg.MN_MAPS_LOGITS), dict(out_dtype=seg.MN_MAPS_LOGITS | 2),
                   dict(th=0), dict(tw=-1), dict(Cn=0), dict(nr=0), dict(nc=-2), dict(nr=33), dict(Cn=65),
                   dict(H=0), dict(W=-3), dict(C=0), dict(C=Cn + 1), dict(H=H - 1), dict(W=W + 1)):
        assert raw(**change) == -1, change
    torch.cuda.synchronize()
    # the good call goes through, by the raw entry point (flip NULL is legal) and by the method
    assert raw(flip=None) == 0
    (tiles, _, _, _, _, _, _), _ = case("a")
    want = mt.tile_class_maps_reference(tiles, None, rows, cols, H, W, C)
    assert np.abs(out.cpu().numpy() - want).max() <= tolerance("a")
    assert raw() == 0
    assert np.abs(out.cpu().numpy() - case("a")[1]).max() <= tolerance("a")


def test_runs_on_the_current_stream(merger):
    import torch
    t, f, rows, cols, H, W, C = on_gpu("b")
    want = merger.tile_class_maps(t, f, rows, cols, H, W, C)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = merger.tile_class_maps(t, f, rows, cols, H, W, C)
    side.synchronize()
    assert np.array_equal(bits(got), bits(want))


def test_tile_class_maps_then_segment_equals_host_pipeline(oracle):
    """Tile logits -> (device) class planes, clipped -> merger, against the CPU oracle on the assembled planes copied
    to the host (the pattern of test_prepare_then_segment_equals_host_pipeline)."""
    import torch
    from mergenet_amd import segmenter as seg, synth
    offs = synth.generate_offsets(8, 6)
    C, Cn, H, W, th, tw = 4, 7, 48, 64, 32, 40
    s = synth.synth_v1(H, W, C, offs, 77, num_instances=3)
    rng = np.random.RandomState(7)
    logp = np.log(s.class_probs.astype(np.float64).clip(1e-6, 1.0))

    def net_logits(jitter_seed):
        """[Cn,H,W]: the instance classes keep log p; the background's log p goes to the four stuff classes, each
        with its own jitter below it."""
        r = np.random.RandomState(jitter_seed)
        stuff = logp[0][None] - np.abs(r.standard_normal((Cn - C + 1, H, W))) * 0.5
        return np.concatenate([stuff, logp[1:]]).astype(np.float32)

    rows, cols = mt.tile_starts(H, th), mt.tile_starts(W, tw)
    plain, flipped = net_logits(int(rng.randint(1 << 30))), net_logits(int(rng.randint(1 << 30)))
    tiles = np.stack([plain[:, r:r + th, c:c + tw] for r in rows for c in cols])
    flips = np.stack([flipped[:, r:r + th, c:c + tw][:, :, ::-1] for r in rows for c in cols])
    m = seg.Merger(H, W, C, len(offs))
    maps = m.tile_class_maps(torch.from_numpy(np.ascontiguousarray(tiles)).cuda(),
                             torch.from_numpy(np.ascontiguousarray(flips)).cuda(), rows, cols, H, W, C, clip=True)
    host = maps.cpu().numpy()
    assert host.shape == (C, H, W) and host.min() >= EPS and host.max() <= 1.0 - EPS
    want = mt.tile_class_maps_reference(tiles, flips, rows, cols, H, W, C)
    assert np.abs(host - want.clip(EPS, 1.0 - EPS)).max() <= (Cn + 9 + C + 8) * 2.0 ** -24
    assert (host.argmax(axis=0) == s.class_probs.argmax(axis=0)).mean() > 0.9      # the planes still say what synth said
    same = torch.from_numpy(s.sameness_probs).cuda()
    o = seg.default_options(mode=seg.MN_MODE_EXACT)
    mask, table, _, st = m.segment(maps, same, offs, o)
    ref = oracle.run_csegment(host, s.sameness_probs, C, offs, 0.0, 1.0, 0.03)
    got = [int(c) for c in table.cpu().numpy()[: st["num_instances"]]]
    assert oracle.masks_equivalent(mask.cpu().numpy(), got, ref.mask, ref.object_class), st
    assert st["num_instances"] >= 1
    m.close()
