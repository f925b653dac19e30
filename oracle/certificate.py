"""The certificate's counters and the log-likelihood of a GIVEN partition, in plain numpy float64.
TEST INFRASTRUCTURE ONLY.

What ``stats.certified`` / ``stats.proof == 1`` rests on, stated once, away from the
five device forms that compute it (``mn_verify_edges``, ``mn_verify_edges4``, ``mn_cc_certificate``,
``mn_cc_tail``, ``mn_verify_records`` / ``mn_x_verify_records``):

* an edge is an in-bounds (pixel p, offset k) pair; its value ``v`` is the sameness value ``same[k, p]``
  after the clip to ``[eps32, 1 - eps32]`` and ``same_different_bias`` (logit, add, sigmoid);
  inside one object ``v > 0.5`` is required, between two objects ``v < 0.5``; ``v == 0.5`` violates either;
* a pixel's own arg-max class (first maximum) must be its object's class;
* a record is a pair of distinct final objects joined by at least one edge; its fresh csegment priority
  ``(sum of log-odds * omf + class delta) / (n1 + n2) + bias`` must be ``< -(1e-6 + 1e-5 * |bias|)``;
* ``total_logprob = sum_p log class[cls(obj(p)), p] + omf * (sum log v inside + sum log(1 - v) between)``
  (the reference's ``ComputeTotalLogprobFromScratch``, ``utils/csegment/segment.cc:314-350``).

Only the csegment variant is stated here (the Python variant's prune moves objects to label 0 with a
non-zero class).  Everything is a pure function of the maps, the options and the partition handed in: the
partition is NOT recomputed, so the function says what the certificate of THAT partition is.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def record_margin(merge_logprob_bias: float) -> float:
    """How far below zero a record between final objects must score (float32 accumulation margin)."""
    return 1e-6 + 1e-5 * abs(float(np.float32(merge_logprob_bias)))


@dataclass
class Certificate:
    edge_violations: int
    class_violations: int
    record_violations: int
    total_logprob: float
    class_term: float
    same_term: float             # sum of log v over the edges inside one object (not yet times omf)
    different_term: float        # sum of log(1 - v) over the edges between objects
    priorities: np.ndarray       # float64 [R]: fresh priority of every record between final objects
    records: dict                # per record, arrays of length R: u, v (root ids, u < v), edges, logodds (float64
                                 # sum), n_u, n_v, cls_u, cls_v, lp_u, lp_v (float64 [R, C] class log-prob sums),
                                 # class_delta
    margin: float
    values: np.ndarray           # float64 [O, H, W]: v of every edge, NaN where the edge leaves the image
    class_gap: float             # smallest relative distance between a pixel's two largest class values

    @property
    def all_zero(self) -> bool:
        return self.edge_violations == 0 and self.class_violations == 0 and self.record_violations == 0


def options_allow_certificate(object_merge_factor: float, merge_logprob_bias: float) -> bool:
    """The csegment variant's side condition of the claim: ``omf > 0`` and ``bias >= 0``."""
    return float(np.float32(object_merge_factor)) > 0.0 and float(np.float32(merge_logprob_bias)) >= 0.0


def edge_values(same_probs, offsets, *, same_different_bias: float = 0.0, clip: bool = True) -> np.ndarray:
    """``v`` of every (offset, pixel) pair in float64; NaN where the edge leaves the image."""
    sp = np.asarray(same_probs, dtype=np.float32).astype(np.float64)
    O, H, W = sp.shape
    if clip:
        sp = np.clip(sp, EPS32, float(np.float32(1.0) - np.float32(EPS32)))
    sdb = float(np.float32(same_different_bias))
    if sdb != 0.0:
        with np.errstate(divide="ignore", over="ignore"):
            logit = np.log(sp) - np.log1p(-sp) + sdb
            sp = 1.0 / (1.0 + np.exp(-logit))
    out = np.full((O, H, W), np.nan)
    for k, (di, dj) in enumerate(offsets):
        r0, r1 = max(0, -di), min(H, H - di)
        c0, c1 = max(0, -dj), min(W, W - dj)
        if r0 < r1 and c0 < c1:
            out[k, r0:r1, c0:c1] = sp[k, r0:r1, c0:c1]
    return out


def object_class_of_root(mask, classes: Sequence[int], partition) -> np.ndarray:
    """What ``HostContext.segment`` returns -> int [N] array, entry r = class of the object whose surviving pixel
    is r (-1 at pixels that are no root).  Label k of the mask is ``classes[k - 1]``; label 0 is class 0."""
    mask = np.asarray(mask).reshape(-1)
    part = np.asarray(partition).reshape(-1).astype(np.int64)
    table = np.concatenate([[0], np.asarray(list(classes), dtype=np.int64)])
    out = np.full(mask.shape[0], -1, np.int64)
    roots = np.unique(part)
    out[roots] = table[mask[roots]]
    # (a label is a property of the object: every pixel of it carries its root's)
    if not np.array_equal(mask, mask[part]):
        raise ValueError("mask and partition disagree: a pixel's label differs from its root's")
    return out


def certificate(class_probs, same_probs, offsets: Sequence[Tuple[int, int]], partition, object_class_of_root, *,
                same_different_bias: float = 0.0, object_merge_factor: float = 1.0,
                merge_logprob_bias: float = 0.0, clip: bool = True) -> Certificate:
    cp = np.asarray(class_probs, dtype=np.float32).astype(np.float64)
    C, H, W = cp.shape
    N = H * W
    offsets = [(int(i), int(j)) for (i, j) in np.asarray(offsets).reshape(-1, 2)]
    if clip:
        cp = np.clip(cp, EPS32, float(np.float32(1.0) - np.float32(EPS32)))
    omf = float(np.float32(object_merge_factor))
    bias = float(np.float32(merge_logprob_bias))
    part = np.asarray(partition).reshape(H, W).astype(np.int64)
    ocls_root = np.asarray(object_class_of_root).reshape(-1).astype(np.int64)
    if ocls_root.shape[0] != N:
        raise ValueError("object_class_of_root: one entry per pixel id")
    flat = part.reshape(-1)
    if not np.array_equal(flat[flat], flat):
        raise ValueError("partition: every pixel must carry the id of its object's surviving pixel")
    obj_cls = ocls_root[part]                                    # [H, W] class of the pixel's object
    if (obj_cls < 0).any() or (obj_cls >= C).any():
        raise ValueError("object_class_of_root has no class for some object")

    # ---- classes ------------------------------------------------------------------------------------------
    with np.errstate(divide="ignore"):
        lp = np.log(cp)                                            # [C, H, W]
    own = np.argmax(lp, axis=0)                                  # first maximum
    class_violations = int((own != obj_cls).sum())
    class_term = float(np.take_along_axis(lp, obj_cls[None], axis=0).sum())
    top2 = np.sort(cp, axis=0)[-2:] if C > 1 else np.stack([np.zeros((H, W)), cp[0]])
    class_gap = float(((top2[1] - top2[0]) / top2[1]).min())

    # ---- edges ------------------------------------------------------------------------------------------------
    vals = edge_values(same_probs, offsets, same_different_bias=same_different_bias, clip=clip)
    edge_violations = 0
    same_term = 0.0
    diff_term = 0.0
    rec_u, rec_v, rec_s = [], [], []
    for k, (di, dj) in enumerate(offsets):
        r0, r1 = max(0, -di), min(H, H - di)
        c0, c1 = max(0, -dj), min(W, W - dj)
        if r0 >= r1 or c0 >= c1:
            continue
        v = vals[k, r0:r1, c0:c1]
        a = part[r0:r1, c0:c1]
        b = part[r0 + di:r1 + di, c0 + dj:c1 + dj]
        inside = a == b
        edge_violations += int((inside & ~(v > 0.5)).sum()) + int((~inside & ~(v < 0.5)).sum())
        with np.errstate(divide="ignore"):
            lv, l1v = np.log(v), np.log1p(-v)
        same_term += float(lv[inside].sum())
        diff_term += float(l1v[~inside].sum())
        rec_u.append(np.minimum(a, b)[~inside])
        rec_v.append(np.maximum(a, b)[~inside])
        rec_s.append((lv - l1v)[~inside])
    total = class_term + omf * (same_term + diff_term)

    # ---- records between final objects -----------------------------------------------------------------------
    margin = record_margin(bias)
    u = np.concatenate(rec_u) if rec_u else np.zeros(0, np.int64)
    v_ = np.concatenate(rec_v) if rec_v else np.zeros(0, np.int64)
    s = np.concatenate(rec_s) if rec_s else np.zeros(0)
    keys, inv, counts = np.unique(u * N + v_, return_inverse=True, return_counts=True)
    R = keys.shape[0]
    ru, rv = keys // N, keys % N
    logodds = np.bincount(inv.reshape(-1), weights=s, minlength=R) if R else np.zeros(0)
    size = np.bincount(flat, minlength=N)
    roots = np.unique(np.concatenate([ru, rv])) if R else np.zeros(0, np.int64)
    slot = np.full(N, -1, np.int64)
    slot[roots] = np.arange(roots.shape[0])
    member = slot[flat]
    sel = member >= 0
    lpsum = np.zeros((roots.shape[0], C))
    for c in range(C):
        lpsum[:, c] = np.bincount(member[sel], weights=lp[c].reshape(-1)[sel], minlength=roots.shape[0])
    lp_u, lp_v = lpsum[slot[ru]], lpsum[slot[rv]]
    cu, cv = ocls_root[ru], ocls_root[rv]
    if R:
        joint = lp_u + lp_v
        best = joint.max(axis=1)
        own_u = np.take_along_axis(lp_u, cu[:, None], axis=1)[:, 0]
        own_v = np.take_along_axis(lp_v, cv[:, None], axis=1)[:, 0]
        delta = np.where(cu != cv, best - own_u - own_v, 0.0)
    else:
        delta = np.zeros(0)
    n_u, n_v = size[ru], size[rv]
    prio = (logodds * omf + delta) / (n_u + n_v) + bias
    record_violations = int((~(prio < -margin)).sum())
    records = dict(u=ru, v=rv, edges=counts, logodds=logodds, n_u=n_u, n_v=n_v, cls_u=cu, cls_v=cv,
                   lp_u=lp_u, lp_v=lp_v, class_delta=delta)
    return Certificate(edge_violations, class_violations, record_violations, total, class_term, same_term,
                       diff_term, prio, records, margin, vals, class_gap)
