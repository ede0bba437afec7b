"""Reference triangle-overlap queries in numpy: what rt_tri_overlaps_count / rt_tri_overlaps_collect must return on an exact
tree, restated from include/rt_abi.h with no code shared with the kernel.

cuts(P, Q): the float32 predicate, operation for operation (cross, dot and subtraction as the header writes them, every
  operation rounded on its own; np.fmin / np.fmax drop a NaN as fminf / fmaxf do; strict comparisons), vectorised over pairs:
  P, Q broadcastable [..., 3, 3].  boxes(P, Q) is its condition 1, no_separating_axis(P, Q) its condition 2.
brute_force(queries, tris, self_pairs): (lists, counts) -- the sorted id array of every query and their lengths (int64).  Not
  traced, an empty row: a non-finite query component.  self_pairs: query i is triangle i; j is kept iff j > i and none of the
  nine corner pairs is equal (all three components ==).
cuts64(P, Q): a float64 separating-axis test on unit-normalised axes, for judging the float32 predicate: -> (sep, extent), sep
  = the largest gap over the axes (sep <= 0: intersecting, sep > 0: separated), axes shorter than 1e-12 * extent^2 skipped,
  extent = the largest coordinate range of the pair's six corners."""
import numpy as np

import range_ref as rr

F = np.float32


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _fold(f, a, b, c):
    return f(f(a, b), c)


def boxes(P, Q):
    """condition 1: the closed overlap of the two vertex boxes (RT_RANGE_BOX's triangle test against the query's box)"""
    P, Q = np.asarray(P, F), np.asarray(Q, F)
    plo, phi = _fold(np.fmin, P[..., 0, :], P[..., 1, :], P[..., 2, :]), _fold(np.fmax, P[..., 0, :], P[..., 1, :], P[..., 2, :])
    qlo, qhi = _fold(np.fmin, Q[..., 0, :], Q[..., 1, :], Q[..., 2, :]), _fold(np.fmax, Q[..., 0, :], Q[..., 1, :], Q[..., 2, :])
    with np.errstate(invalid="ignore"):
        return ((qlo <= phi) & (qhi >= plo)).all(axis=-1)


def axes(P, Q):
    """the seventeen axes in the header's order, float32: [..., 17, 3]"""
    p0, p1, p2 = P[..., 0, :], P[..., 1, :], P[..., 2, :]
    q0, q1, q2 = Q[..., 0, :], Q[..., 1, :], Q[..., 2, :]
    e = (p1 - p0, p2 - p1, p0 - p2)
    f = (q1 - q0, q2 - q1, q0 - q2)
    nP, nQ = _cross(e[0], e[1]), _cross(f[0], f[1])
    out = [nP, nQ]
    out += [_cross(e[i], f[j]) for i in range(3) for j in range(3)]
    out += [_cross(nP, e[i]) for i in range(3)]
    out += [_cross(nQ, f[j]) for j in range(3)]
    shape = np.broadcast_shapes(*[a.shape for a in out])
    return np.stack([np.broadcast_to(a, shape) for a in out], axis=-2)


def no_separating_axis(P, Q):
    """condition 2, float32: no axis among the seventeen with minP > maxQ or minQ > maxP"""
    P, Q = np.asarray(P, F), np.asarray(Q, F)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p0 = P[..., 0, :]
        Pr = (np.zeros_like(p0), P[..., 1, :] - p0, P[..., 2, :] - p0)
        Qr = (Q[..., 0, :] - p0, Q[..., 1, :] - p0, Q[..., 2, :] - p0)
        A = axes(P, Q)
        ok = np.ones(A.shape[:-2], bool)
        for k in range(17):
            a = A[..., k, :]
            sP = [_dot(a, x) for x in Pr]
            sQ = [_dot(a, x) for x in Qr]
            minP, maxP = _fold(np.fmin, *sP), _fold(np.fmax, *sP)
            minQ, maxQ = _fold(np.fmin, *sQ), _fold(np.fmax, *sQ)
            ok &= ~((minP > maxQ) | (minQ > maxP))
    return ok


def cuts(P, Q):
    return boxes(P, Q) & no_separating_axis(P, Q)


def traced(queries):
    return np.isfinite(np.asarray(queries, F).reshape(-1, 9)).all(axis=1)


def shares_corner(P, Q):
    """any of the nine corner pairs equal: all three components float == (-0 == +0, a NaN equals nothing)"""
    P, Q = np.asarray(P, F), np.asarray(Q, F)
    with np.errstate(invalid="ignore"):
        return (P[..., :, None, :] == Q[..., None, :, :]).all(axis=-1).any(axis=(-1, -2))


def match_matrix(queries, tris, self_pairs=False, chunk=1 << 18):
    """bool [m, n]: cuts(query i, triangle k), with the not-traced rule and (self_pairs) the SELF exclusions.  Condition 2 is
    evaluated on the pairs that pass condition 1 only -- the conjunction is the same."""
    Pq = np.asarray(queries, F).reshape(-1, 3, 3)
    T = np.asarray(tris, F).reshape(-1, 3, 3)
    m, n = Pq.shape[0], T.shape[0]
    out = np.zeros((m, n), bool)
    if m == 0 or n == 0:
        return out
    lo, hi = _fold(np.fmin, Pq[:, 0], Pq[:, 1], Pq[:, 2]), _fold(np.fmax, Pq[:, 0], Pq[:, 1], Pq[:, 2])
    cand = rr.box_matrix(lo, hi, T.reshape(-1, 9)) & traced(Pq)[:, None]
    if self_pairs:
        assert m == n, "SELF: the queries are the scene's triangles"
        cand &= np.arange(n)[None, :] > np.arange(m)[:, None]
    qi, ti = np.nonzero(cand)
    for s in range(0, len(qi), chunk):
        a, b = qi[s:s + chunk], ti[s:s + chunk]
        keep = no_separating_axis(Pq[a], T[b])
        if self_pairs:
            keep &= ~shares_corner(Pq[a], T[b])
        out[a[keep], b[keep]] = True
    return out


def _lists(match):
    lists = [np.nonzero(row)[0].astype(np.uint32) for row in match]
    return lists, np.array([len(x) for x in lists], np.int64)


def brute_force(queries, tris, self_pairs=False):
    return _lists(match_matrix(queries, tris, self_pairs))


def offsets(counts):
    return rr.offsets(counts)


def vertex_boxes(queries):
    """the queries' vertex boxes as (lo, hi): the RT_RANGE_BOX query every row must be a subset of"""
    Pq = np.asarray(queries, F).reshape(-1, 3, 3)
    return _fold(np.fmin, Pq[:, 0], Pq[:, 1], Pq[:, 2]), _fold(np.fmax, Pq[:, 0], Pq[:, 1], Pq[:, 2])


def cuts64(P, Q):
    """float64 separating-axis test on unit axes -> (sep, extent)"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    P, Q = np.broadcast_arrays(P, Q)
    allc = np.concatenate([P, Q], axis=-2)
    extent = (allc.max(axis=-2) - allc.min(axis=-2)).max(axis=-1)
    A = axes(P, Q)                                            # (float64 in, float64 out)
    length = np.linalg.norm(A, axis=-1)
    usable = length >= 1e-12 * extent[..., None] ** 2
    unit = A / np.where(usable, length, 1.0)[..., None]
    sP = np.einsum("...kc,...vc->...kv", unit, P)
    sQ = np.einsum("...kc,...vc->...kv", unit, Q)
    gap = np.maximum(sP.min(-1) - sQ.max(-1), sQ.min(-1) - sP.max(-1))
    gap = np.where(usable, gap, -np.inf)
    return gap.max(axis=-1), extent
