"""oracle/certificate.py -- the float64 statement of the certificate's counters -- anchored on the CPU:
on the reference program's own log-likelihood (through the oracle's restatement of
ComputeTotalLogprobFromScratch) and on small cases whose counts are worked out by hand."""
import math

import numpy as np
import pytest

from mergenet_amd import synth
from oracle import certificate as cert

F = np.float32


def _logit(v):
    v = float(F(v))
    return math.log(v) - math.log1p(-v)


def _naive(cp, sp, offsets, part, ocls, sdb, omf, bias):
    """The same definitions as a loop over pixels and offsets, with dictionaries: a second, slow statement that
    shares no array code with oracle/certificate.py (values already inside the clip range)."""
    C, H, W = cp.shape
    sdb, omf, bias = float(F(sdb)), float(F(omf)), float(F(bias))
    bad_e = bad_c = 0
    t_cls = t_same = t_diff = 0.0
    rec, size, lps = {}, {}, {}
    for r in range(H):
        for c in range(W):
            o = int(part[r, c])
            size[o] = size.get(o, 0) + 1
            logs = [math.log(float(cp[k, r, c])) for k in range(C)]
            lps[o] = [a + b for a, b in zip(lps.get(o, [0.0] * C), logs)]
            if logs.index(max(logs)) != ocls[o]:
                bad_c += 1
            t_cls += logs[ocls[o]]
            for k, (di, dj) in enumerate(offsets):
                rr, cc = r + di, c + dj
                if rr < 0 or rr >= H or cc < 0 or cc >= W:
                    continue
                v = float(sp[k, r, c])
                if sdb != 0.0:
                    v = 1.0 / (1.0 + math.exp(-(math.log(v) - math.log1p(-v) + sdb)))
                q = int(part[rr, cc])
                if q == o:
                    t_same += math.log(v)
                    bad_e += 0 if v > 0.5 else 1
                else:
                    t_diff += math.log1p(-v)
                    bad_e += 0 if v < 0.5 else 1
                    key = (min(o, q), max(o, q))
                    e, s = rec.get(key, (0, 0.0))
                    rec[key] = (e + 1, s + math.log(v) - math.log1p(-v))
    prio = {}
    for (a, b), (e, s) in rec.items():
        delta = 0.0
        if ocls[a] != ocls[b]:
            delta = max(x + y for x, y in zip(lps[a], lps[b])) - lps[a][ocls[a]] - lps[b][ocls[b]]
        prio[(a, b)] = (s * omf + delta) / (size[a] + size[b]) + bias
    margin = 1e-6 + 1e-5 * abs(bias)
    bad_r = sum(0 if p < -margin else 1 for p in prio.values())
    return bad_e, bad_c, bad_r, t_cls + omf * (t_same + t_diff), prio, {k: v[0] for k, v in rec.items()}


def _roots_class(N, table):
    out = np.full(N, -1, np.int64)
    for r, c in table.items():
        out[r] = c
    return out


# ---- 3 x 4: two objects, four offsets that leave the image on every side -----------------------------------
#   pixel ids     partition (root)      objects: A = columns 0-1 (root 0, class 0), B = columns 2-3 (root 2, class 1)
#   0 1  2  3     0 0 2 2
#   4 5  6  7     0 0 2 2
#   8 9 10 11     0 0 2 2
# in-bounds edges: (0,1): 9 = 3 in A, 3 across, 3 in B (leaves on the right)
#                  (1,0): 8 = 4 in A, 4 in B           (leaves at the bottom)
#                  (-1,2): 4, all across               (leaves at the top and on the right; NEGATIVE row offset)
#                  (1,-1): 6 = 2 in A, 2 across, 2 in B (leaves on the left and at the bottom)
# one record A-B of 3 + 4 + 2 = 9 edges.
OFFS_3X4 = [(0, 1), (1, 0), (-1, 2), (1, -1)]


def _case_3x4():
    H, W = 3, 4
    part = np.array([[0, 0, 2, 2]] * 3)
    target = np.array([[0, 0, 1, 1]] * 3)
    sp = np.full((4, H, W), 0.5, F)            # 0.5 wherever the edge leaves the image: must never be counted
    for k, (di, dj) in enumerate(OFFS_3X4):
        for r in range(H):
            for c in range(W):
                if 0 <= r + di < H and 0 <= c + dj < W:
                    sp[k, r, c] = 0.8 if target[r, c] == target[r + di, c + dj] else 0.2
    cp = np.empty((2, H, W), F)
    cp[0] = np.where(target == 0, 0.9, 0.2)
    cp[1] = np.where(target == 0, 0.1, 0.8)
    return cp, sp, part, _roots_class(H * W, {0: 0, 2: 1})


def test_hand_3x4_clean():
    cp, sp, part, ocls = _case_3x4()
    assert synth.count_edges(3, 4, OFFS_3X4) == 27
    res = cert.certificate(cp, sp, OFFS_3X4, part, ocls, merge_logprob_bias=0.0)
    assert (res.edge_violations, res.class_violations, res.record_violations) == (0, 0, 0)
    assert int(np.isfinite(res.values).sum()) == 27
    assert list(res.records["u"]) == [0] and list(res.records["v"]) == [2] and list(res.records["edges"]) == [9]
    # nine edges of 0.2 between six pixels of (0.9, 0.1) and six of (0.2, 0.8)
    joint = max(6 * math.log(float(F(0.9))) + 6 * math.log(float(F(0.2))),
                6 * math.log(float(F(0.1))) + 6 * math.log(float(F(0.8))))
    delta = joint - 6 * math.log(float(F(0.9))) - 6 * math.log(float(F(0.8)))
    assert res.priorities[0] == pytest.approx((9 * _logit(0.2) + delta) / 12, rel=1e-12)
    total = 6 * math.log(float(F(0.9))) + 6 * math.log(float(F(0.8))) + \
        (27 - 9) * math.log(float(F(0.8))) + 9 * math.log1p(-float(F(0.2)))
    assert res.total_logprob == pytest.approx(total, rel=1e-12)


def test_hand_3x4_planted_edges_classes_and_the_record():
    cp, sp, part, ocls = _case_3x4()
    sp[0, 0, 0] = 0.5            # inside A, exactly 0.5                       -> violation
    sp[0, 1, 1] = 0.5            # across,   exactly 0.5                       -> violation
    sp[1, 1, 3] = 0.3            # inside B, (1,3) -> (2,3), last column       -> violation
    sp[2, 2, 1] = 0.7            # across by the negative-row offset, last row -> violation
    sp[1, 0, 0] = 0.51           # inside A, just right: no violation
    sp[3, 0, 2] = 0.49           # across (0,2) -> (1,1), just right: no violation
    cp[:, 2, 0] = (0.4, 0.6)     # a pixel of A whose own class is 1           -> class violation
    cp[:, 0, 3] = (0.5, 0.5)     # a pixel of B with a tie: first maximum = 0  -> class violation
    res = cert.certificate(cp, sp, OFFS_3X4, part, ocls, merge_logprob_bias=0.0)
    assert res.edge_violations == 4
    assert res.class_violations == 2
    assert res.record_violations == 0
    # the record: (0,1) 0.2, 0.5, 0.2; (-1,2) 0.2 x 3, 0.7; (1,-1) 0.49, 0.2
    s = 6 * _logit(0.2) + _logit(0.5) + _logit(0.7) + _logit(0.49)
    assert _logit(0.5) == 0.0
    assert res.records["logodds"][0] == pytest.approx(s, rel=1e-12)
    lp_a = [5 * math.log(float(F(0.9))) + math.log(float(F(0.4))), 5 * math.log(float(F(0.1))) + math.log(float(F(0.6)))]
    lp_b = [5 * math.log(float(F(0.2))) + math.log(0.5), 5 * math.log(float(F(0.8))) + math.log(0.5)]
    delta = max(lp_a[0] + lp_b[0], lp_a[1] + lp_b[1]) - lp_a[0] - lp_b[1]
    assert res.priorities[0] == pytest.approx((s + delta) / 12, rel=1e-12)
    # a bias that lifts the record over the margin makes it the one record violation; the other counts stay
    up = cert.certificate(cp, sp, OFFS_3X4, part, ocls, merge_logprob_bias=5.0)
    assert (up.edge_violations, up.class_violations, up.record_violations) == (4, 2, 1)
    assert up.priorities[0] == pytest.approx((s + delta) / 12 + 5.0, rel=1e-12)
    naive = _naive(cp, sp, OFFS_3X4, part, ocls, 0.0, 1.0, 5.0)
    assert naive[:3] == (4, 2, 1)
    assert up.total_logprob == pytest.approx(naive[3], rel=1e-12)


# ---- 2 x 5: three objects, a record of exactly two edges -----------------------------------------------------------
#   pixel ids      partition       X = columns 0-1 (root 0, class 1), Y = columns 2-3 (root 2, class 0),
#   0 1 2 3 4      0 0 2 2 4       Z = column 4 (root 4, class 1)
#   5 6 7 8 9      0 0 2 2 4
# (0,3): 4 edges: column 0 -> 3 is X-Y (2), column 1 -> 4 is X-Z (2)            (leaves on the right)
# (-1,-1): 4 edges from row 1: (1,1)->(0,0) in X, (1,2)->(0,1) Y-X, (1,3)->(0,2) in Y, (1,4)->(0,3) Z-Y
#                                                                                (leaves at the top and on the left)
# records: X-Y 3 edges, X-Z 2 edges, Y-Z 1 edge.
OFFS_2X5 = [(0, 3), (-1, -1)]


def _case_2x5():
    part = np.array([[0, 0, 2, 2, 4]] * 2)
    sp = np.full((2, 2, 5), 0.5, F)
    sp[0, :, 0] = 0.2
    sp[0, 0, 1], sp[0, 1, 1] = 0.4, 0.45          # the two edges of X-Z
    sp[1, 1, 1:] = (0.8, 0.2, 0.8, 0.2)
    cls = np.array([[1, 1, 0, 0, 1]] * 2)
    cp = np.empty((2, 2, 5), F)
    cp[0] = np.where(cls == 0, 0.9, 0.1)
    cp[1] = np.where(cls == 0, 0.1, 0.9)
    return cp, sp, part, _roots_class(10, {0: 1, 2: 0, 4: 1})


def test_hand_2x5_a_record_of_two_edges_on_both_sides_of_the_margin():
    cp, sp, part, ocls = _case_2x5()
    assert synth.count_edges(2, 5, OFFS_2X5) == 8
    res = cert.certificate(cp, sp, OFFS_2X5, part, ocls, object_merge_factor=2.0, merge_logprob_bias=0.2)
    assert (res.edge_violations, res.class_violations) == (0, 0)
    assert [tuple(x) for x in zip(res.records["u"], res.records["v"], res.records["edges"])] == \
        [(0, 2, 3), (0, 4, 2), (2, 4, 1)]
    xz = (_logit(0.4) + _logit(0.45)) * 2.0 / 6 + float(F(0.2))          # same class: no class delta
    assert res.records["class_delta"][1] == 0.0
    assert res.priorities[1] == pytest.approx(xz, rel=1e-12)
    assert xz < -res.margin and res.record_violations == 0
    assert res.margin == pytest.approx(1e-6 + 1e-5 * float(F(0.2)), rel=1e-12)
    # 0.21 lifts X-Z (and only X-Z) over the margin
    up = cert.certificate(cp, sp, OFFS_2X5, part, ocls, object_merge_factor=2.0, merge_logprob_bias=0.21)
    assert up.priorities[1] > 0 and up.record_violations == 1
    assert (up.priorities[[0, 2]] < -0.1).all()
    # between -margin and 0 is a violation too: negative is not enough
    b = float(F(-(xz - float(F(0.2))) - 1e-6))
    near = cert.certificate(cp, sp, OFFS_2X5, part, ocls, object_merge_factor=2.0, merge_logprob_bias=b)
    assert -near.margin < near.priorities[1] < 0 and near.record_violations == 1


def test_hand_2x5_same_different_bias_moves_two_edges_over_the_half():
    """logit(0.4) + 0.5 and logit(0.45) + 0.5 are positive, logit(0.2) + 0.5 is not: the two X-Z edges become
    violations, nothing else changes sides."""
    cp, sp, part, ocls = _case_2x5()
    res = cert.certificate(cp, sp, OFFS_2X5, part, ocls, same_different_bias=0.5)
    assert res.edge_violations == 2
    assert res.values[0, 0, 1] == pytest.approx(1 / (1 + math.exp(-(_logit(0.4) + 0.5))), rel=1e-12)
    naive = _naive(cp, sp, OFFS_2X5, part, ocls, 0.5, 1.0, 0.0)
    assert naive[0] == 2 and res.total_logprob == pytest.approx(naive[3], rel=1e-12)


def test_clip_makes_exact_zero_and_one_finite():
    cp, sp, part, ocls = _case_2x5()
    sp[0, 0, 0] = 0.0           # across
    sp[1, 1, 1] = 1.0           # inside
    res = cert.certificate(cp, sp, OFFS_2X5, part, ocls, clip=True)
    assert res.edge_violations == 0 and math.isfinite(res.total_logprob)
    assert res.values[0, 0, 0] == cert.EPS32 and res.values[1, 1, 1] == 1.0 - cert.EPS32
    assert res.records["logodds"][0] == pytest.approx(_logit(0.2) + _logit(0.2) + math.log(cert.EPS32) -
                                                      math.log1p(-cert.EPS32), rel=1e-12)


def test_object_class_of_root_maps_labels_to_classes():
    mask = np.array([[1, 1, 0, 0, 2]] * 2)
    part = np.array([[0, 0, 2, 2, 4]] * 2)
    got = cert.object_class_of_root(mask, [7, 3], part)
    assert got[0] == 7 and got[2] == 0 and got[4] == 3 and (np.delete(got, [0, 2, 4]) == -1).all()
    with pytest.raises(ValueError):
        cert.object_class_of_root(np.array([[1, 0, 0, 0, 2]] * 2), [7, 3], part)


def test_random_partitions_equal_the_naive_statement():
    """Arbitrary partitions (unions of random pixels, nothing to do with the maps): many violations of every kind."""
    rng = np.random.default_rng(7)
    for trial in range(6):
        H, W, C = int(rng.integers(2, 7)), int(rng.integers(2, 9)), int(rng.integers(2, 5))
        offs = [(0, 1), (1, 0), (-1, 2), (2, -1)][: int(rng.integers(2, 5))]
        cp = rng.uniform(0.05, 0.95, (C, H, W)).astype(F)
        sp = rng.uniform(0.05, 0.95, (len(offs), H, W)).astype(F)
        blocks = rng.integers(0, 4, (H, W))
        part = np.zeros((H, W), np.int64)
        ids = np.arange(H * W).reshape(H, W)
        for b in range(4):
            if (blocks == b).any():
                part[blocks == b] = ids[blocks == b].min()
        ocls = np.full(H * W, -1, np.int64)
        roots = np.unique(part)
        ocls[roots] = rng.integers(0, C, roots.shape[0])
        opts = dict(same_different_bias=[0.0, 0.3][trial % 2], object_merge_factor=[1.0, 0.5, 2.0][trial % 3],
                    merge_logprob_bias=[0.0, 0.03, 3.0][trial % 3])
        res = cert.certificate(cp, sp, offs, part, ocls, **opts)
        e, c, r, total, prio, edges = _naive(cp, sp, offs, part, ocls, opts["same_different_bias"],
                                             opts["object_merge_factor"], opts["merge_logprob_bias"])
        assert (res.edge_violations, res.class_violations, res.record_violations) == (e, c, r), trial
        assert res.total_logprob == pytest.approx(total, rel=1e-12)
        keys = list(zip(res.records["u"].tolist(), res.records["v"].tolist()))
        assert sorted(keys) == sorted(prio)
        for i, k in enumerate(keys):
            assert res.priorities[i] == pytest.approx(prio[k], rel=1e-9, abs=1e-12)
            assert res.records["edges"][i] == edges[k]


# ---- the reference program's own sum ----------------------------------------------------------------------------
# (H, W, offsets, seed): W % 4 in {0, 1, 2, 3}, one row, one column
ANCHORS = [(12, 16, (6, 4), 41), (11, 17, (6, 4), 42), (10, 18, (6, 4), 43), (9, 19, (6, 4), 44),
           (1, 24, (3, 3), 45), (24, 1, (3, 3), 46), (16, 20, (5, 5), 47)]


@pytest.mark.parametrize("H,W,offspec,seed", ANCHORS)
@pytest.mark.parametrize("opts", [(0.0, 1.0, 0.0), (0.2, 0.7, 0.0)])
def test_separable_maps_have_no_violations_and_the_oracles_log_likelihood(oracle, H, W, offspec, seed, opts):
    """On the oracle's own partition of a separable map nothing contradicts the partition, and the float64 sum is
    what the oracle's restatement of ComputeTotalLogprobFromScratch gives, to the 1e-5 the project compares the
    device with.  bias = 0: no record between components can be merged, so the partition is the components."""
    offs = synth.generate_offsets(*offspec)
    s = synth.synth_v1(H, W, 3, offs, seed, noise=0.1, num_instances=2)
    ref = oracle.run_csegment(s.class_probs, s.sameness_probs, 3, offs, *opts)
    ocls = cert.object_class_of_root(ref.mask, ref.object_class, ref.partition)
    res = cert.certificate(s.class_probs, s.sameness_probs, offs, ref.partition, ocls, same_different_bias=opts[0],
                           object_merge_factor=opts[1], merge_logprob_bias=opts[2], clip=True)
    assert int(np.isfinite(res.values).sum()) == synth.count_edges(H, W, offs)
    assert (res.edge_violations, res.class_violations, res.record_violations) == (0, 0, 0)
    assert abs(res.total_logprob - ref.total_logprob) <= 1e-5 * abs(ref.total_logprob)
    assert res.total_logprob == pytest.approx(res.class_term + float(F(opts[1])) * (res.same_term + res.different_term))
    assert cert.options_allow_certificate(opts[1], opts[2])


def test_a_swallowed_instance_shows_in_every_count(oracle):
    """With a large bias the background swallows everything: the oracle's partition is one object, every edge that
    was between instances is now inside it with v < 0.5, and the log-likelihood still equals the oracle's."""
    offs = synth.generate_offsets(6, 4)
    s = synth.synth_v1(12, 16, 3, offs, 41, noise=0.1, num_instances=2)
    ref = oracle.run_csegment(s.class_probs, s.sameness_probs, 3, offs, 0.0, 1.0, 50.0)
    assert np.unique(ref.partition).shape[0] == 1
    ocls = cert.object_class_of_root(ref.mask, ref.object_class, ref.partition)
    res = cert.certificate(s.class_probs, s.sameness_probs, offs, ref.partition, ocls, merge_logprob_bias=50.0)
    inb = np.isfinite(res.values)
    assert res.edge_violations == int((res.values[inb] < 0.5).sum()) > 0
    assert res.record_violations == 0 and res.priorities.shape == (0,)
    assert abs(res.total_logprob - ref.total_logprob) <= 1e-5 * abs(ref.total_logprob)
    assert not cert.options_allow_certificate(1.0, -0.01) and not cert.options_allow_certificate(0.0, 0.0)
