"""What the binding's host-side checks reject, and with which exception type: one wrong-dtype, one non-contiguous and
one wrong-shape argument (and one tensor on the host) for every Merger method that takes tensors, one wrong buffer for
every ``into=`` / ``out=`` / ``coeffs=`` / ``factor=``, the same for ``DatasetEval.add`` and the wire functions.

Every rejection happens before anything is launched.  The types are those the binding raises, pinned so that a change
of the checks' wording or structure cannot change them: ValueError for a tensor that does not fit, AssertionError
where the reference's binding asserts (map shapes against each other and the offsets, the wire functions),
MergeNetError(MN_ERR_ARGUMENT) where the entry point itself would answer that.
"""
import pytest

from mergenet_amd import segmenter as seg

pytestmark = pytest.mark.gpu

H = W = 8
C = O = 2
OFFS = [(0, 1), (1, 0)]


class _Good:
    """One Merger and one well-formed argument of each kind; the cases replace one of them."""

    def __init__(self):
        import torch
        self.torch = torch
        self.m = seg.Merger(H, W, C, O)
        dev = torch.device("cuda", self.m.device)
        self.cp = torch.full((C, H, W), 0.5, dtype=torch.float32, device=dev)
        self.sp = torch.full((O, H, W), 0.5, dtype=torch.float32, device=dev)
        self.mask = torch.zeros((H, W), dtype=torch.int32, device=dev)
        self.i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        self.f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        self.f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        self.i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
        self.u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
        self.tiles = self.f32(1, 3, 4, 4)
        self.ev = self.m.dataset_eval(num_classes=C)

    @staticmethod
    def strided(t):
        """The shape and dtype of `t`, every second element of a buffer twice as wide."""
        wide = t.new_zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],))
        v = wide[..., ::2]
        assert v.shape == t.shape and not v.is_contiguous()
        return v

    def bad(self, t, kind):
        if kind == "dtype":
            return t.to(self.torch.float64 if t.dtype.is_floating_point else self.torch.int64)
        if kind == "strided":
            return self.strided(t)
        if kind == "host":
            return t.cpu()
        assert kind == "rank"
        return t[0]


@pytest.fixture(scope="module")
def g():
    good = _Good()
    yield good
    good.m.close()


KINDS = ("dtype", "strided", "host", "rank")

# ---- methods that take the two maps (Merger._check) -----------------------------------------------------------------

MAP_METHODS = {
    "segment": lambda g, cp, sp, offs: g.m.segment(cp, sp, offs),
    "segment_async": lambda g, cp, sp, offs: g.m.segment_async(cp, sp, offs),
    "score": lambda g, cp, sp, offs: g.m.score(cp, sp, offs),
    "sweep": lambda g, cp, sp, offs: g.m.sweep(cp, sp, offs),
    "sweep_time": lambda g, cp, sp, offs: g.m.sweep_time([(cp, sp)], offs, reps=1),
    "exact_phase_a": lambda g, cp, sp, offs: g.m.exact_phase_a(cp, sp, offs),
    "map_scores": lambda g, cp, sp, offs: g.m.map_scores(cp, sp, offs, g.mask, None),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ("class", "same"))
@pytest.mark.parametrize("method", list(MAP_METHODS))
def test_map_methods_reject_a_bad_map(g, method, which, kind):
    cp = g.bad(g.cp, kind) if which == "class" else g.cp
    sp = g.bad(g.sp, kind) if which == "same" else g.sp
    with pytest.raises(ValueError):
        MAP_METHODS[method](g, cp, sp, OFFS)


@pytest.mark.parametrize("method", list(MAP_METHODS))
def test_map_methods_assert_on_maps_that_do_not_fit_each_other(g, method):
    with pytest.raises(AssertionError):
        MAP_METHODS[method](g, g.cp, g.f32(O, H, W // 2), OFFS)
    with pytest.raises(AssertionError):
        MAP_METHODS[method](g, g.cp, g.sp, OFFS[:1])
    with pytest.raises(ValueError):                          # the two maps share one dtype
        MAP_METHODS[method](g, g.cp, g.sp.half(), OFFS)


# ---- methods that take an int32 [H,W] mask ---------------------------------------------------------------------------

MASK_METHODS = {
    "upsample_mask": lambda g, mask: g.m.upsample_mask(mask, 2 * H, 2 * W),
    "encode_rle": lambda g, mask: g.m.encode_rle(mask, 1),
    "sameness_targets": lambda g, mask: g.m.sameness_targets(mask, OFFS),
    "instance_table": lambda g, mask: g.m.instance_table(mask, 1),
    "filter_instances": lambda g, mask: g.m.filter_instances(mask, g.i32(4), 1),
    "overlap_table.pred": lambda g, mask: g.m.overlap_table(mask, g.mask, 1, 1),
    "overlap_table.truth": lambda g, mask: g.m.overlap_table(g.mask, mask, 1, 1),
    "map_scores.truth": lambda g, mask: g.m.map_scores(g.cp, g.sp, OFFS, mask, None),
    "mask_bce.truth": lambda g, mask: g.m.mask_bce(g.cp, g.sp, OFFS, mask, None),
    "plane_sums.truth": lambda g, mask: g.m.plane_sums(g.cp, "class", None, mask, None),
    "plane_grad.truth": lambda g, mask: g.m.plane_grad(g.cp, "class", None, mask, None, g.f32(4, C)),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method", list(MASK_METHODS))
def test_mask_methods_reject_a_bad_mask(g, method, kind):
    with pytest.raises(ValueError):
        MASK_METHODS[method](g, g.bad(g.mask, kind))


@pytest.mark.parametrize("method", [m for m in MASK_METHODS if "." in m and m != "overlap_table.pred"])
def test_a_truth_mask_has_the_shape_of_what_it_is_held_against(g, method):
    with pytest.raises(ValueError):
        MASK_METHODS[method](g, g.i32(H, W // 2))


# ---- the other tensor arguments, one bad value each ------------------------------------------------------------------

def _cases():
    V, A, E = ValueError, AssertionError, seg.MergeNetError
    return [
        # segment_async: out=(mask, table)
        ("segment_async.out.dtype", V, lambda g: g.m.segment_async(g.cp, g.sp, OFFS, out=(g.f32(H, W), g.i32(H * W)))),
        ("segment_async.out.strided", V, lambda g: g.m.segment_async(g.cp, g.sp, OFFS,
                                                                      out=(g.strided(g.mask), g.i32(H * W)))),
        ("segment_async.out.size", V, lambda g: g.m.segment_async(g.cp, g.sp, OFFS, out=(g.i32(H, W // 2), g.i32(H * W)))),
        ("segment_async.out.table", V, lambda g: g.m.segment_async(g.cp, g.sp, OFFS, out=(g.mask, g.i32(H * W - 1)))),
        ("segment_async.out.host", V, lambda g: g.m.segment_async(g.cp, g.sp, OFFS, out=(g.mask.cpu(), g.i32(H * W)))),
        # prepare
        ("prepare.dtype", V, lambda g: g.m.prepare(g.cp.double(), H, W)),
        ("prepare.strided", V, lambda g: g.m.prepare(g.strided(g.cp), H, W)),
        ("prepare.rank", V, lambda g: g.m.prepare(g.cp[0], H, W)),
        ("prepare.host", V, lambda g: g.m.prepare(g.cp.cpu(), H, W)),
        ("prepare.out_dtype", V, lambda g: g.m.prepare(g.cp, H, W, out_dtype=g.torch.int32)),
        # filter_instances
        ("filter.class_table.dtype", V, lambda g: g.m.filter_instances(g.mask, g.i64(4), 2)),
        ("filter.class_table.strided", V, lambda g: g.m.filter_instances(g.mask, g.strided(g.i32(4)), 2)),
        ("filter.class_table.short", V, lambda g: g.m.filter_instances(g.mask, g.i32(1), 2)),
        ("filter.class_table.host", V, lambda g: g.m.filter_instances(g.mask, g.i32(4).cpu(), 2)),
        ("filter.scores.dtype", V, lambda g: g.m.filter_instances(g.mask, g.i32(4), 2, scores=g.f64(2))),
        ("filter.scores.strided", V, lambda g: g.m.filter_instances(g.mask, g.i32(4), 2, scores=g.strided(g.f32(2)))),
        ("filter.scores.short", V, lambda g: g.m.filter_instances(g.mask, g.i32(4), 2, scores=g.f32(1))),
        ("filter.table.dtype", V, lambda g: g.m.filter_instances(g.mask, g.i32(4), 2, table=g.i64(2, 5))),
        ("filter.table.strided", V, lambda g: g.m.filter_instances(g.mask, g.i32(4), 2, table=g.strided(g.i32(2, 5)))),
        ("filter.table.shape", V, lambda g: g.m.filter_instances(g.mask, g.i32(4), 2, table=g.i32(3, 5))),
        ("filter.negative", V, lambda g: g.m.filter_instances(g.mask, g.i32(4), -1)),
        ("instance_table.negative", V, lambda g: g.m.instance_table(g.mask, -1)),
        ("overlap_table.negative", V, lambda g: g.m.overlap_table(g.mask, g.mask, -1, 1)),
        # match_instances
        ("match.table.dtype", V, lambda g: g.m.match_instances(g.i64(3, 3), g.i32(2), g.i32(2))),
        ("match.table.strided", V, lambda g: g.m.match_instances(g.strided(g.i32(3, 3)), g.i32(2), g.i32(2))),
        ("match.table.rank", V, lambda g: g.m.match_instances(g.i32(9), g.i32(2), g.i32(2))),
        ("match.table.host", V, lambda g: g.m.match_instances(g.i32(3, 3).cpu(), g.i32(2), g.i32(2))),
        ("match.pred_classes.dtype", V, lambda g: g.m.match_instances(g.i32(3, 3), g.i64(2), g.i32(2))),
        ("match.pred_classes.none", V, lambda g: g.m.match_instances(g.i32(3, 3), None, g.i32(2))),
        ("match.truth_classes.strided", V, lambda g: g.m.match_instances(g.i32(3, 3), g.i32(2), g.strided(g.i32(2)))),
        ("match.truth_classes.short", V, lambda g: g.m.match_instances(g.i32(3, 3), g.i32(2), g.i32(1))),
        ("match.scores.dtype", V, lambda g: g.m.match_instances(g.i32(3, 3), g.i32(2), g.i32(2), scores=g.f64(2))),
        ("match.scores.host", V, lambda g: g.m.match_instances(g.i32(3, 3), g.i32(2), g.i32(2), scores=g.f32(2).cpu())),
        ("match.crowd.dtype", V, lambda g: g.m.match_instances(g.i32(3, 3), g.i32(2), g.i32(2), crowd=g.i32(2))),
        ("match.thresholds", V, lambda g: g.m.match_instances(g.i32(3, 3), g.i32(2), g.i32(2), thresholds=[])),
        # DatasetEval.add
        ("eval.table.dtype", V, lambda g: g.ev.add(g.i64(3, 3), g.i32(2), g.i32(2))),
        ("eval.table.strided", V, lambda g: g.ev.add(g.strided(g.i32(3, 3)), g.i32(2), g.i32(2))),
        ("eval.table.rank", V, lambda g: g.ev.add(g.i32(9), g.i32(2), g.i32(2))),
        ("eval.pred_classes.dtype", V, lambda g: g.ev.add(g.i32(3, 3), g.i64(2), g.i32(2))),
        ("eval.pred_classes.none", V, lambda g: g.ev.add(g.i32(3, 3), None, g.i32(2))),
        ("eval.truth_classes.short", V, lambda g: g.ev.add(g.i32(3, 3), g.i32(2), g.i32(1))),
        ("eval.scores.strided", V, lambda g: g.ev.add(g.i32(3, 3), g.i32(2), g.i32(2), scores=g.strided(g.f32(2)))),
        ("eval.crowd.dtype", V, lambda g: g.ev.add(g.i32(3, 3), g.i32(2), g.i32(2), crowd=g.f32(2))),
        # the truth's classes (map_scores, mask_bce, plane_sums)
        ("map_scores.truth_classes.dtype", V, lambda g: g.m.map_scores(g.cp, g.sp, OFFS, g.mask, g.i64(2))),
        ("map_scores.truth_classes.strided", V, lambda g: g.m.map_scores(g.cp, g.sp, OFFS, g.mask, g.strided(g.i32(2)))),
        ("map_scores.truth_classes.rank", V, lambda g: g.m.map_scores(g.cp, g.sp, OFFS, g.mask, g.i32(2, 1))),
        ("map_scores.truth_classes.host", V, lambda g: g.m.map_scores(g.cp, g.sp, OFFS, g.mask, g.i32(2).cpu())),
        ("mask_bce.truth_classes.dtype", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, g.i64(2))),
        ("plane_sums.truth_classes.dtype", V, lambda g: g.m.plane_sums(g.cp, "class", None, g.mask, g.i64(2))),
        # map_scores: into=
        ("map_scores.into.confusion.dtype", V, lambda g: g.m.map_scores(
            g.cp, g.sp, OFFS, g.mask, None, into={"confusion": g.i32(C, C), "sums": g.f64(3, O)})),
        ("map_scores.into.confusion.strided", V, lambda g: g.m.map_scores(
            g.cp, g.sp, OFFS, g.mask, None, into={"confusion": g.strided(g.i64(C, C)), "sums": g.f64(3, O)})),
        ("map_scores.into.sums.shape", V, lambda g: g.m.map_scores(
            g.cp, g.sp, OFFS, g.mask, None, into={"confusion": g.i64(C, C), "sums": g.f64(3, O + 1)})),
        ("map_scores.into.sums.dtype", V, lambda g: g.m.map_scores(
            g.cp, g.sp, OFFS, g.mask, None, into={"confusion": g.i64(C, C), "sums": g.f32(3, O)})),
        # mask_bce
        ("mask_bce.class.dtype", V, lambda g: g.m.mask_bce(g.cp.double(), g.sp.double(), OFFS, g.mask, None)),
        ("mask_bce.class.strided", V, lambda g: g.m.mask_bce(g.strided(g.cp), g.sp, OFFS, g.mask, None)),
        ("mask_bce.same.strided", V, lambda g: g.m.mask_bce(g.cp, g.strided(g.sp), OFFS, g.mask, None)),
        ("mask_bce.class.rank", V, lambda g: g.m.mask_bce(g.f32(C, H, W, 1), g.sp, OFFS, g.mask, None)),
        ("mask_bce.class.host", V, lambda g: g.m.mask_bce(g.cp.cpu(), g.sp, OFFS, g.mask, None)),
        ("mask_bce.dtypes_differ", V, lambda g: g.m.mask_bce(g.cp, g.sp.half(), OFFS, g.mask, None)),
        ("mask_bce.sizes_differ", V, lambda g: g.m.mask_bce(g.cp, g.f32(O, H, W // 2), OFFS, g.mask, None)),
        ("mask_bce.offsets", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS[:1], g.mask, None)),
        ("mask_bce.no_planes", E, lambda g: g.m.mask_bce(None, g.f32(0, H, W), OFFS, g.mask, None)),
        ("mask_bce.into.dtype", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, into=g.f32(2 + O))),
        ("mask_bce.into.shape", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, into={"sums": g.f64(3 + O)})),
        ("mask_bce.into.strided", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, into=g.strided(g.f64(2 + O)))),
        ("mask_bce.out.dtype", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, out=(g.cp.half(), g.sp.clone()))),
        ("mask_bce.out.shape", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, out=(g.cp.clone(), g.f32(O + 1, H, W)))),
        ("mask_bce.out.strided", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, out=(g.strided(g.cp), g.sp.clone()))),
        ("mask_bce.out.none", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, out=(None, g.sp.clone()))),
        ("mask_bce.out.one", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, out=(g.cp.clone(),))),
        ("mask_bce.out.without_grad", V, lambda g: g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, None, grad=False,
                                                                 out=(g.cp.clone(), g.sp.clone()))),
        # plane_sums
        ("plane_sums.part", V, lambda g: g.m.plane_sums(g.cp, "planes", None, g.mask, None)),
        ("plane_sums.logits.dtype", V, lambda g: g.m.plane_sums(g.cp.double(), "class", None, g.mask, None)),
        ("plane_sums.logits.strided", V, lambda g: g.m.plane_sums(g.strided(g.cp), "class", None, g.mask, None)),
        ("plane_sums.logits.rank", V, lambda g: g.m.plane_sums(g.cp[0], "class", None, g.mask, None)),
        ("plane_sums.logits.host", V, lambda g: g.m.plane_sums(g.cp.cpu(), "class", None, g.mask, None)),
        ("plane_sums.offsets", V, lambda g: g.m.plane_sums(g.sp, "offset", OFFS[:1], g.mask, None)),
        ("plane_sums.into.dtype", V, lambda g: g.m.plane_sums(g.cp, "class", None, g.mask, None, into=g.f32(5 * C + 1))),
        ("plane_sums.into.shape", V, lambda g: g.m.plane_sums(g.cp, "class", None, g.mask, None, into=g.f64(5 * C))),
        ("plane_sums.out.strided", V, lambda g: g.m.plane_sums(g.cp, "class", None, g.mask, None,
                                                                out=g.strided(g.f64(5 * C + 1)))),
        ("plane_sums.into_and_out", V, lambda g: g.m.plane_sums(g.cp, "class", None, g.mask, None, into=g.f64(5 * C + 1),
                                                                 out=g.f64(5 * C + 1))),
        # plane_coeffs
        ("plane_coeffs.criterion", V, lambda g: g.m.plane_coeffs("bce", g.f64(5 * C + 1))),
        ("plane_coeffs.sums.dtype", V, lambda g: g.m.plane_coeffs("dice", g.f32(5 * C + 1))),
        ("plane_coeffs.sums.strided", V, lambda g: g.m.plane_coeffs("dice", g.strided(g.f64(5 * C + 1)))),
        ("plane_coeffs.sums.length", V, lambda g: g.m.plane_coeffs("dice", g.f64(5 * C))),
        ("plane_coeffs.sums.rank", V, lambda g: g.m.plane_coeffs("dice", g.f64(1, 5 * C + 1))),
        ("plane_coeffs.sums.host", V, lambda g: g.m.plane_coeffs("dice", g.f64(5 * C + 1).cpu())),
        ("plane_coeffs.out.dtype", V, lambda g: g.m.plane_coeffs("dice", g.f64(5 * C + 1), out=g.f64(4, C))),
        ("plane_coeffs.out.shape", V, lambda g: g.m.plane_coeffs("dice", g.f64(5 * C + 1), out=g.f32(4, C + 1))),
        ("plane_coeffs.out.strided", V, lambda g: g.m.plane_coeffs("dice", g.f64(5 * C + 1), out=g.strided(g.f32(4, C)))),
        ("plane_coeffs.into.dtype", V, lambda g: g.m.plane_coeffs("dice", g.f64(5 * C + 1), into=g.f32())),
        ("plane_coeffs.into.size", V, lambda g: g.m.plane_coeffs("dice", g.f64(5 * C + 1), into={"loss": g.f64(2)})),
        # plane_grad
        ("plane_grad.logits.dtype", V, lambda g: g.m.plane_grad(g.cp.double(), "class", None, g.mask, None, g.f32(4, C))),
        ("plane_grad.logits.strided", V, lambda g: g.m.plane_grad(g.strided(g.cp), "class", None, g.mask, None, g.f32(4, C))),
        ("plane_grad.coeffs.dtype", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.f64(4, C))),
        ("plane_grad.coeffs.shape", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.f32(C, 4, C))),
        ("plane_grad.coeffs.strided", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.strided(g.f32(4, C)))),
        ("plane_grad.factor.dtype", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.f32(4, C), factor=g.f64())),
        ("plane_grad.factor.size", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.f32(4, C), factor=g.f32(2))),
        ("plane_grad.factor.host", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.f32(4, C),
                                                                factor=g.f32().cpu())),
        ("plane_grad.out.dtype", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.f32(4, C), out=g.cp.half())),
        ("plane_grad.out.shape", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.f32(4, C),
                                                              out=g.f32(C + 1, H, W))),
        ("plane_grad.out.strided", V, lambda g: g.m.plane_grad(g.cp, "class", None, g.mask, None, g.f32(4, C),
                                                                out=g.strided(g.cp))),
        # tile_class_maps
        ("tiles.dtype", V, lambda g: g.m.tile_class_maps(g.tiles.double(), None, [0], [0], 4, 4, C)),
        ("tiles.strided", V, lambda g: g.m.tile_class_maps(g.strided(g.tiles), None, [0], [0], 4, 4, C)),
        ("tiles.rank", V, lambda g: g.m.tile_class_maps(g.tiles[0], None, [0], [0], 4, 4, C)),
        ("tiles.host", V, lambda g: g.m.tile_class_maps(g.tiles.cpu(), None, [0], [0], 4, 4, C)),
        ("tiles.flip.dtype", V, lambda g: g.m.tile_class_maps(g.tiles, g.tiles.half(), [0], [0], 4, 4, C)),
        ("tiles.flip.shape", V, lambda g: g.m.tile_class_maps(g.tiles, g.f32(1, 3, 4, 2), [0], [0], 4, 4, C)),
        ("tiles.flip.strided", V, lambda g: g.m.tile_class_maps(g.tiles, g.strided(g.tiles), [0], [0], 4, 4, C)),
        ("tiles.out_dtype", V, lambda g: g.m.tile_class_maps(g.tiles, None, [0], [0], 4, 4, C, out_dtype=g.torch.int32)),
        ("tiles.starts", V, lambda g: g.m.tile_class_maps(g.tiles, None, [0, 0], [0], 4, 4, C)),
        ("tiles.no_image", E, lambda g: g.m.tile_class_maps(g.tiles, None, [0], [0], 0, 4, C)),
        # the wire functions
        ("pack_wire.mask.dtype", A, lambda g: seg.pack_wire(g.i64(H, W), g.i32(4), 1, g.torch.zeros(
            H * W + 16, dtype=g.torch.int16, device=g.mask.device), 4)),
        ("pack_wire.mask.strided", A, lambda g: seg.pack_wire(g.strided(g.mask), g.i32(4), 1, g.torch.zeros(
            H * W + 16, dtype=g.torch.int16, device=g.mask.device), 4)),
        ("pack_wire.wire.dtype", A, lambda g: seg.pack_wire(g.mask, g.i32(4), 1, g.i32(H * W + 16), 4)),
        ("pack_wire.wire.short", A, lambda g: seg.pack_wire(g.mask, g.i32(4), 1, g.torch.zeros(
            H * W, dtype=g.torch.int16, device=g.mask.device), 4)),
        ("pack_runs.mask.dtype", A, lambda g: seg.pack_runs(g.m, g.i64(H, W), g.i32(4), 1,
                                                             g.i32(seg.runs_wire_words(16, 4)), 16, 4)),
        ("pack_runs.mask.strided", A, lambda g: seg.pack_runs(g.m, g.strided(g.mask), g.i32(4), 1,
                                                               g.i32(seg.runs_wire_words(16, 4)), 16, 4)),
        ("pack_runs.table.short", A, lambda g: seg.pack_runs(g.m, g.mask, g.i32(1), 2,
                                                              g.i32(seg.runs_wire_words(16, 4)), 16, 4)),
        ("pack_runs.wire.short", A, lambda g: seg.pack_runs(g.m, g.mask, g.i32(4), 1,
                                                             g.i32(seg.runs_wire_words(16, 4) - 1), 16, 4)),
    ]


CASES = _cases()


@pytest.mark.parametrize("name,exc,call", CASES, ids=[c[0] for c in CASES])
def test_one_bad_argument(g, name, exc, call):
    with pytest.raises(exc) as info:
        call(g)
    assert type(info.value) is exc, (name, type(info.value))
    if exc is seg.MergeNetError:
        assert info.value.status == seg.MN_ERR_ARGUMENT


def test_the_lowp_tests_substring_stays_in_the_dtype_messages(g):
    for call in (lambda: g.m.segment(g.cp.double(), g.sp.double(), OFFS), lambda: g.m.prepare(g.cp.double(), H, W),
                 lambda: g.m.segment(g.strided(g.cp), g.sp, OFFS)):
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            call()


def test_the_good_arguments_are_accepted(g):
    """The fixture's arguments themselves pass every check: a case above fails for the one thing it changes."""
    K = 2
    g.m.filter_instances(g.mask, g.i32(4), K, scores=g.f32(K), table=g.i32(K, 5))
    g.m.match_instances(g.i32(3, 3), g.i32(2), g.i32(2), scores=g.f32(2), crowd=g.u8(2))
    g.m.map_scores(g.cp, g.sp, OFFS, g.mask, g.i32(2), into={"confusion": g.i64(C, C), "sums": g.f64(3, O)})
    g.m.mask_bce(g.cp, g.sp, OFFS, g.mask, g.i32(2), into=g.f64(2 + O), out=(g.cp.clone(), g.sp.clone()))
    g.m.plane_sums(g.cp, "class", None, g.mask, g.i32(2), into=g.f64(5 * C + 1))
    g.m.plane_coeffs("dice", g.f64(5 * C + 1), out=g.f32(4, C), into=g.f64())
    g.m.plane_grad(g.cp, "class", None, g.mask, g.i32(2), g.f32(4, C), factor=g.f32() + 1, out=g.cp.clone())
    g.m.tile_class_maps(g.tiles, g.tiles.clone(), [0], [0], 4, 4, C)
    g.torch.cuda.synchronize()
