"""Merger.map_scores on the device against the numpy statement labels.map_scores on the same arrays.

The confusion matrix and sums[2] (a count) are compared exactly.  sums[0] and sums[1] are float64 sums of n_pixels
non-negative terms: the statement returns the correctly rounded sum, any order of float64 additions stays within
n_pixels * 2^-53 of it, relative -- that is the bound; a sum that is 0 must be exactly 0."""
import functools

import numpy as np
import pytest

from mergenet_amd import labels, synth

pytestmark = pytest.mark.gpu

C, G_TRUTH = 9, 7
TRUTH_CLASSES = (3, 1, 8, 255, 2, 1, 5)          # label 4 has class 255: outside 0..C-1, an ignore class
SHAPES = [(1, 1),
          (3, 5),
          (7, 64),       # one chunk of single-element loads per row when unaligned, a quarter chunk of 16-byte loads
          (33, 257),     # single elements, the last chunk of a row reaches past W
          (48, 256),     # 16-byte loads, one chunk per row
          (32, 1028),    # 16-byte loads, the last chunk of a row partly past W
          (64, 1030),    # single elements, several chunks per row
          (256, 1040)]   # 1280 chunks of 16-byte loads: 160 workgroups = 160 slots of the partials buffer, two chunks
                         # per wave, eight per workgroup; unaligned: 4352 chunks, seven per wave (the grid is the same)


def offsets_for(shape):
    H, W = shape
    return synth.generate_offsets(40, 10) + [(-3, 2), (0, -1), (H, 0), (0, W)]


@functools.lru_cache(maxsize=None)
def image(shape, seed=5, span=24):
    """(class maps [C,H,W], sameness maps [O,H,W], truth mask): random float32 maps, the class maps rounded to
    eighths in the left half so that the argmax meets ties; blobs of 7 truth labels, a label out of range and a
    negative one; the sameness maps leave 0..1 in the right quarter."""
    H, W = shape
    rng = np.random.default_rng(seed + 1000 * H + W)
    cp = rng.random((C, H, W), dtype=np.float32)
    cp[:, :, : (W + 1) // 2] = np.round(cp[:, :, : (W + 1) // 2] * 8) / 8
    sp = rng.random((len(offsets_for(shape)), H, W), dtype=np.float32)
    # (1 - p of a probability is a multiple of 2^-24 and at most 1: float64 adds such terms without any rounding, in
    # every order.  The right quarter holds values of -1 down to -2^span instead -- 1 - p stays positive -- so that the
    # additions do round and the bound is put to work.)
    wide = sp[:, :, W - W // 4:]
    wide[...] = -(1.0 + wide) * 2.0 ** rng.integers(0, span, wide.shape)
    truth = np.zeros((H, W), np.int32)
    for k in range(1, G_TRUTH + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        truth[max(0, y - H // 6):y + H // 6 + 1, max(0, x - W // 6):x + W // 6 + 1] = k
    if W > 70:
        truth[H // 2, 60:70] = 5                     # across lanes and across the 64-pixel mark
        truth[H - 1, W - 3:] = G_TRUTH + 4           # out of range: class 0, a label of its own for the sums
        truth[0, 2] = -7
    truth[H - 1, W - 1] = 1
    for a in (cp, sp, truth):
        a.setflags(write=False)
    return cp, sp, truth


@functools.lru_cache(maxsize=None)
def statement(shape):
    cp, sp, truth = image(shape)
    conf, sums = labels.map_scores(cp, sp, offsets_for(shape), truth, TRUTH_CLASSES, G_TRUTH)
    conf.setflags(write=False)
    sums.setflags(write=False)
    return conf, sums


@pytest.fixture(scope="module")
def merger():
    from mergenet_amd import segmenter as seg
    m = seg.Merger(64, 128, 9, 10)
    yield m
    m.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the shared arrays are read-only)


def off_base(t, nbytes=4):
    """The tensor on the device `nbytes` behind a 16-byte boundary (the trick of test_gpu_match.unaligned)."""
    import torch
    step = nbytes // t.element_size()
    buf = torch.zeros((t.numel() + 16,), dtype=t.dtype, device="cuda")
    view = buf[step:step + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == nbytes and view.is_contiguous()
    return view


def classes(values=TRUTH_CLASSES):
    import torch
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def check(got, want, n_pixels, what=""):
    conf, sums = got["confusion"].cpu().numpy(), got["sums"].cpu().numpy()
    want_conf, want_sums = want
    assert conf.dtype == np.int64 and sums.dtype == np.float64
    assert conf.shape == want_conf.shape and sums.shape == want_sums.shape
    assert np.array_equal(conf, want_conf), what
    assert np.array_equal(sums[2], want_sums[2]), what
    bound = n_pixels * 2.0 ** -53
    err = np.abs(sums[:2] - want_sums[:2])
    rel = err[want_sums[:2] > 0] / want_sums[:2][want_sums[:2] > 0]
    print("%s: greatest relative error of a sum %.3g (bound %.3g)" % (what, rel.max() if rel.size else 0.0, bound))
    assert (err <= bound * want_sums[:2]).all(), what          # (a sum that is 0 must be exactly 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_scores_equal_the_statement(merger, shape):
    cp, sp, truth = image(shape)
    offs = offsets_for(shape)
    n = truth.size
    want = statement(shape)
    if shape[0] <= 33:                                           # several offsets leave the image entirely
        assert (want[1][2] == 0).sum() >= 3
    d_cp, d_sp, d_truth = dev(cp), dev(sp), dev(truth)
    got = merger.map_scores(d_cp, d_sp, offs, d_truth, classes())
    check(got, want, n, "aligned")
    assert got["confusion"].sum().item() == n - int(np.isin(truth, [4]).sum())
    # maps and mask 4 bytes off a 16-byte boundary: single-element loads, the same grid
    got = merger.map_scores(off_base(d_cp), off_base(d_sp), offs, off_base(d_truth), classes())
    check(got, want, n, "4 bytes off")


@pytest.mark.parametrize("num_classes,num_offsets", [(1, 3), (127, 3), (9, 32)])
def test_limits_of_classes_and_offsets(merger, num_classes, num_offsets):
    shape = (33, 257)
    H, W = shape
    rng = np.random.default_rng(num_classes + num_offsets)
    cp = rng.random((num_classes, H, W), dtype=np.float32)
    offs = [(k // 6 - 2, k % 6 - 2) for k in range(36) if (k // 6 - 2, k % 6 - 2) != (0, 0)][:num_offsets]
    sp = rng.random((num_offsets, H, W), dtype=np.float32)
    truth = image(shape)[2]
    tc = [int(v) for v in rng.integers(0, num_classes, G_TRUTH)]
    want = labels.map_scores(cp, sp, offs, truth, tc, G_TRUTH)
    got = merger.map_scores(dev(cp), dev(sp), offs, dev(truth), classes(tc))
    check(got, want, truth.size, "C = %d, O = %d" % (num_classes, num_offsets))
    assert got["confusion"].sum().item() == truth.size


def test_no_truth_instances(merger):
    shape = (33, 257)
    cp, sp, truth = image(shape)
    offs = offsets_for(shape)
    want = labels.map_scores(cp, sp, offs, truth, None, 0)
    got = merger.map_scores(dev(cp), dev(sp), offs, dev(truth), None)
    check(got, want, truth.size, "no truth classes")
    assert got["confusion"][1:].sum().item() == 0 and got["confusion"].sum().item() == truth.size
    assert np.array_equal(want[1], statement(shape)[1])          # the sums look at the labels as they stand


def test_ignore_class_is_left_out_of_the_confusion_matrix_only(merger):
    shape = (48, 256)
    cp, sp, truth = image(shape)
    offs = offsets_for(shape)
    tc = [255] * G_TRUTH
    want = labels.map_scores(cp, sp, offs, truth, tc, G_TRUTH)
    got = merger.map_scores(dev(cp), dev(sp), offs, dev(truth), classes(tc))
    check(got, want, truth.size, "every instance ignored")
    inside = ((truth >= 1) & (truth <= G_TRUTH)).sum()
    assert inside > 0 and got["confusion"].sum().item() == truth.size - inside
    assert np.array_equal(want[1], statement(shape)[1])


def block_image(num_classes):
    """40 x 2048 with the predicted class and the truth class constant over wide blocks, as on a real image: most
    chunks of 64 lanes x 4 (256 pixels) or x 8 (512 pixels) lie in ONE (truth class, predicted class) cell and are
    counted once, by 64 * V.  Some rows change class inside a chunk, and one truth label is an ignore class."""
    H, W = 40, 2048
    rng = np.random.default_rng(77 + num_classes)
    dom = np.zeros((H, W), np.int64)
    for r0 in range(0, H, 8):                        # bands of 8 rows, blocks of 512 columns
        dom[r0:r0 + 8] = np.repeat(rng.integers(0, num_classes, W // 512), 512)[None]
    dom[5, 300:1500] = num_classes - 1               # boundaries inside chunks
    dom[17, 1:] = 1 % num_classes
    cp = rng.random((num_classes, H, W), dtype=np.float32) * 0.5
    np.put_along_axis(cp, dom[None], 0.75, axis=0)   # (0.75 is a bfloat16 value; the rest stays below 0.5)
    truth = np.zeros((H, W), np.int32)
    truth[16:, :1024] = 1
    truth[16:, 1024:] = 2
    truth[30:36, 512:1536] = 3                       # ignored
    truth[2, 100:700] = 2
    tc = [num_classes - 1, 1 % num_classes, 255]
    offs = [(0, 1), (3, -2), (-1, 40)]
    sp = rng.random((len(offs), H, W), dtype=np.float32)
    return cp, sp, truth, tc, offs


def uniform_chunks(cp, truth, tc, pixels):
    """Chunks of `pixels` consecutive pixels of a row whose pixels all fall in one cell of the confusion matrix."""
    num_classes = cp.shape[0]
    tcls = np.concatenate([[0], tc])[truth]
    key = np.where(tcls < num_classes, tcls * num_classes + cp.argmax(axis=0), -1).reshape(truth.shape[0], -1, pixels)
    return int(((key == key[:, :, :1]).all(axis=2) & (key[:, :, 0] >= 0)).sum()), key.shape[0] * key.shape[1]


@pytest.mark.parametrize("num_classes", [9, 40])     # 40: above the LDS table, every count a global atomic
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_chunks_inside_one_cell_of_the_confusion_matrix(merger, dtype, num_classes):
    import torch
    cp, sp, truth, tc, offs = block_image(num_classes)
    t_cp, t_sp = dev(cp).to(getattr(torch, dtype)), dev(sp).to(getattr(torch, dtype))
    assert t_cp.data_ptr() % 16 == 0 and t_sp.data_ptr() % 16 == 0       # 4 pixels per lane in float32, 8 in 16 bits
    w_cp, w_sp = t_cp.float().cpu().numpy(), t_sp.float().cpu().numpy()
    uniform, chunks = uniform_chunks(w_cp, truth, tc, 256 if dtype == "float32" else 512)
    assert uniform > chunks // 2 and uniform < chunks                    # both ways of counting are taken
    want = labels.map_scores(w_cp, w_sp, offs, truth, tc, len(tc))
    assert (want[0] >= 256).sum() >= 4
    got = merger.map_scores(t_cp, t_sp, offs, dev(truth), classes(tc))
    check(got, want, truth.size, "%s, C = %d" % (dtype, num_classes))
    assert got["confusion"].sum().item() == truth.size - int((truth == 3).sum())


@pytest.mark.parametrize("shape", [(16, 520), (33, 257), (9, 260)])      # 8 per lane; single elements; W % 8 == 4: 4 per lane
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_16_bit_maps_score_as_their_widened_values(merger, dtype, shape):
    import torch
    cp, sp, truth = image(shape, span=15)                        # (binary16 ends at 65504)
    offs = offsets_for(shape)
    t_cp, t_sp = dev(cp).to(getattr(torch, dtype)), dev(sp).to(getattr(torch, dtype))
    want = labels.map_scores(t_cp.float().cpu().numpy(), t_sp.float().cpu().numpy(), offs, truth, TRUTH_CLASSES, G_TRUTH)
    d_truth = dev(truth)
    check(merger.map_scores(t_cp, t_sp, offs, d_truth, classes()), want, truth.size, "%s aligned" % dtype)
    # 8 bytes behind a 16-byte boundary: 4 per lane where W % 4 == 0; 4 bytes behind: single elements
    check(merger.map_scores(off_base(t_cp, 8), off_base(t_sp, 8), offs, d_truth, classes()), want, truth.size, "8 bytes off")
    check(merger.map_scores(off_base(t_cp, 4), off_base(t_sp, 4), offs, off_base(d_truth), classes()), want, truth.size,
          "4 bytes off")


def far_offsets(shape):
    """(0, 1), then five offsets that leave the image whatever the pixel: by exactly H rows or W columns, by one more,
    and by the ends of the int32 range (the entry point holds each to -H..H / -W..W)."""
    H, W = shape
    return [(0, 1), (H, 0), (0, -W), (H + 1, 0), (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)]


@pytest.mark.parametrize("shape,dtype", [((3, 5), "float32"),          # single elements
                                         ((9, 260), "bfloat16")])       # W % 8 == 4: four pixels per lane
def test_offsets_beyond_the_image_find_no_different_pixel(merger, shape, dtype):
    import torch
    cp, sp, truth = image(shape, span=15)
    offs = far_offsets(shape)
    t_cp, t_sp = dev(cp).to(getattr(torch, dtype)), dev(sp[:len(offs)]).to(getattr(torch, dtype))
    assert t_cp.data_ptr() % 16 == 0 and t_sp.data_ptr() % 16 == 0
    want = labels.map_scores(t_cp.float().cpu().numpy(), t_sp.float().cpu().numpy(), offs, truth, TRUTH_CLASSES, G_TRUTH)
    assert want[1][2, 0] > 0 and (want[1][[0, 2], 1:] == 0).all() and (want[1][1] > 0).all()
    got = merger.map_scores(t_cp, t_sp, offs, dev(truth), classes())
    check(got, want, truth.size, "%s %s" % (shape, dtype))
    sums = got["sums"].cpu().numpy()
    assert (sums[[0, 2], 1:] == 0).all()                         # exactly 0: no neighbour was found, none was read


@pytest.mark.parametrize("shape", [(33, 257), (48, 256)])
def test_float32_logits_equal_the_call_on_their_probabilities_bit_for_bit(merger, shape):
    import torch
    cp, sp, truth = image(shape)
    offs = offsets_for(shape)
    H, W = shape
    l_cp = (dev(cp) - 0.5) * 40.0                                 # logits in -20..20: many saturate to exactly 1.0
    l_sp = (dev(sp) - 0.5) * 40.0
    d_truth = dev(truth)
    got = merger.map_scores(l_cp, l_sp, offs, d_truth, classes(), logits=True)
    p_cp = merger.prepare(l_cp, H, W, apply_sigmoid=True, clip=False)
    p_sp = merger.prepare(l_sp, H, W, apply_sigmoid=True, clip=False)
    assert (p_cp == 1.0).sum().item() > 0
    want = merger.map_scores(p_cp, p_sp, offs, d_truth, classes())
    assert torch.equal(got["confusion"], want["confusion"])
    assert got["sums"].cpu().numpy().tobytes() == want["sums"].cpu().numpy().tobytes()
    check(want, labels.map_scores(p_cp.cpu().numpy(), p_sp.cpu().numpy(), offs, truth, TRUTH_CLASSES, G_TRUTH),
          truth.size, "probabilities of the logits")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_saturated_logits_tie_and_the_lowest_class_wins(merger, dtype):
    import torch
    H, W = 4, 8
    l_cp = torch.full((5, H, W), -3.0, device="cuda")
    l_cp[0] = 1.0
    l_cp[3, 2, 5], l_cp[1, 2, 5], l_cp[4, 2, 5] = 18.0, 20.0, 25.0       # all exactly 1.0 as float32 probabilities
    l_cp = l_cp.to(getattr(torch, dtype))
    l_sp = torch.zeros((1, H, W), device="cuda").to(getattr(torch, dtype))
    truth = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    truth[2, 5] = 1
    got = merger.map_scores(l_cp, l_sp, [(0, 1)], truth, classes([2]), logits=True)
    conf = got["confusion"].cpu().numpy()
    assert conf[2].tolist() == [0, 1, 0, 0, 0]                   # class 1 is the lowest of 1, 3, 4
    assert conf[0].tolist() == [H * W - 1, 0, 0, 0, 0] and conf.sum() == H * W
    assert got["sums"].cpu().numpy().tolist() == [[1.0], [0.5 * H * W], [2.0]]


def test_two_calls_give_byte_identical_results(merger):
    shape = (256, 1040)
    cp, sp, truth = image(shape)
    offs = offsets_for(shape)
    args = (dev(cp), dev(sp), offs, dev(truth), classes())
    a = merger.map_scores(*args)
    b = merger.map_scores(*args)
    assert a["sums"].cpu().numpy().tobytes() == b["sums"].cpu().numpy().tobytes()
    assert a["confusion"].cpu().numpy().tobytes() == b["confusion"].cpu().numpy().tobytes()


def test_into_accumulates_the_running_totals(merger):
    import torch
    shape = (32, 1028)
    cp, sp, truth = image(shape)
    cp2, sp2, truth2 = image(shape, seed=6)
    offs = offsets_for(shape)
    a = merger.map_scores(dev(cp), dev(sp), offs, dev(truth), classes())
    b = merger.map_scores(dev(cp2), dev(sp2), offs, dev(truth2), classes())
    total = {k: v.clone() for k, v in a.items()}
    back = merger.map_scores(dev(cp2), dev(sp2), offs, dev(truth2), classes(), into=total)
    assert back["sums"] is total["sums"] and back["confusion"] is total["confusion"]
    assert not torch.equal(a["sums"], b["sums"])
    assert torch.equal(total["sums"], a["sums"] + b["sums"])     # one IEEE addition per total
    assert torch.equal(total["confusion"], a["confusion"] + b["confusion"])


def test_bad_arguments_raise_and_launch_nothing(merger):
    import torch
    from mergenet_amd import segmenter as seg
    shape = (7, 64)
    cp, sp, truth = image(shape)
    offs = offsets_for(shape)
    d_cp, d_sp, d_truth = dev(cp), dev(sp), dev(truth)
    with pytest.raises(ValueError):
        merger.map_scores(d_cp.cpu(), d_sp, offs, d_truth, classes())              # a tensor on the host
    with pytest.raises(ValueError):
        merger.map_scores(d_cp, d_sp, offs, d_truth.cpu(), classes())
    with pytest.raises(ValueError):
        merger.map_scores(d_cp.transpose(1, 2), d_sp.transpose(1, 2), offs, d_truth, classes())      # not contiguous
    with pytest.raises(ValueError):
        merger.map_scores(d_cp, d_sp, offs, d_truth.long(), classes())             # the mask's dtype
    with pytest.raises(ValueError):
        merger.map_scores(d_cp, d_sp, offs, d_truth, classes().long())
    with pytest.raises(ValueError):
        merger.map_scores(d_cp, d_sp.half(), offs, d_truth, classes())             # two dtypes
    with pytest.raises(ValueError):
        merger.map_scores(d_cp, d_sp, offs, d_truth[:, :32].contiguous(), classes())     # another size
    good = merger.map_scores(d_cp, d_sp, offs, d_truth, classes())
    with pytest.raises(ValueError):
        merger.map_scores(d_cp, d_sp[:3].contiguous(), offs[:3], d_truth, classes(), into=good)   # another O
    wide = torch.zeros((128, 7, 64), device="cuda")
    with pytest.raises(seg.MergeNetError):
        merger.map_scores(wide, d_sp, offs, d_truth, classes())                    # C = 128 > MN_MAX_CLASSES
    check(merger.map_scores(d_cp, d_sp, offs, d_truth, classes()), statement(shape), truth.size, "after the refusals")
