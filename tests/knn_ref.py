"""Reference k-nearest queries in numpy: what rt_k_nearest must return, restated from include/rt_abi.h (k-nearest block) with no
code shared with the kernel.

brute_force_knn(points, dist2_max, tris, k): for each query the candidate set S = { (d2(p, tri[t]), t) : d2 <= dist2_max } with
point_ref.d2 (a NaN d2 is not a candidate: `d <= r` is false for it), sorted by a STABLE sort on dist2 -- the candidates are
laid out in id order, so ties on dist2 keep the lower id first -- and cut to the first k; rows are padded with (+inf, MISS).
An untraced query (non-finite p, NaN or negative dist2_max) is a row of misses."""
import numpy as np

import point_ref as pr

F = np.float32
MISS = pr.MISS
KNN_HIT = np.dtype([("dist2", "<f4"), ("primitive_id", "<u4")])


def brute_force_knn(points, dist2_max, tris, k, chunk=1 << 22):
    """-> KNN_HIT array [len(points), k].  tris: float32 [n, 9]."""
    P = np.asarray(points, F).reshape(-1, 3)
    R = np.broadcast_to(np.asarray(dist2_max, F), (P.shape[0],))
    T = np.asarray(tris, F).reshape(-1, 3, 3)
    n, m = T.shape[0], P.shape[0]
    out = np.zeros((m, k), KNN_HIT)
    out["dist2"], out["primitive_id"] = np.inf, MISS
    ok = pr.traced(P, R)
    step = max(1, chunk // max(n, 1))
    for s in range(0, m, step):
        idx = np.nonzero(ok[s:s + step])[0] + s
        if idx.size == 0 or n == 0:
            continue
        d, _, _ = pr.d2(P[idx, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])
        with np.errstate(invalid="ignore"):
            member = d <= R[idx, None]                        # closed radius; false for NaN
        for row, q in enumerate(idx):
            ids = np.nonzero(member[row])[0]                  # ascending ids
            order = np.argsort(d[row, ids], kind="stable")[:k]
            out["dist2"][q, :order.size] = d[row, ids[order]]
            out["primitive_id"][q, :order.size] = ids[order]
    return out


def ascending(rows):
    """every row is ascending in (dist2, primitive_id), strictly (no pair twice) among its real records"""
    d, i = rows["dist2"], rows["primitive_id"].astype(np.int64)
    real = i[:, 1:] != MISS
    up = (d[:, :-1] < d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & (i[:, :-1] < i[:, 1:]))
    after_miss = (i[:, :-1] == MISS) & real                  # a real record behind a padding entry
    return bool((up | ~real).all()) and not bool(after_miss.any())
