"""Reference range queries in numpy: what rt_range_count / rt_range_collect must return on an exact tree, restated from
include/rt_abi.h with no code shared with the kernel.

sphere(points, dist2_max, tris): triangle k matches query i iff point_ref.d2(p_i, tri_k) <= dist2_max_i (float32, the
closest-point block's routine; a NaN d2 does not match).  Not traced, an empty set: a non-finite p, a NaN or negative dist2_max.
box(lo, hi, tris): triangle k matches iff np.fmin / np.fmax of its corners overlap [lo, hi] on every axis with closed compares
(tlo <= hi and thi >= lo).  Not traced: a NaN component, or lo > hi on an axis.
Both return (lists, counts): the sorted id array of every query and their lengths (int64).  offsets(counts) is the CSR row
array the count call must produce."""
import numpy as np

import point_ref as pr

F = np.float32


def traced_sphere(points, dist2_max):
    return pr.traced(points, dist2_max)


def traced_box(lo, hi):
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(invalid="ignore"):
        return (lo <= hi).all(axis=-1)          # false for a NaN on either side


def _lists(match):
    """match: bool [m, n] -> (list of sorted id arrays, counts)"""
    lists = [np.nonzero(row)[0].astype(np.uint32) for row in match]
    return lists, np.array([len(x) for x in lists], np.int64)


def sphere_matrix(points, dist2_max, tris, chunk=1 << 22):
    P = np.asarray(points, F).reshape(-1, 3)
    R = np.broadcast_to(np.asarray(dist2_max, F), (P.shape[0],))
    T = np.asarray(tris, F).reshape(-1, 3, 3)
    m, n = P.shape[0], T.shape[0]
    out = np.zeros((m, n), bool)
    ok = traced_sphere(P, R)
    step = max(1, chunk // max(n, 1))
    for s in range(0, m, step):
        idx = np.nonzero(ok[s:s + step])[0] + s
        if idx.size == 0 or n == 0:
            continue
        d, _, _ = pr.d2(P[idx, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])
        with np.errstate(invalid="ignore"):
            out[idx] = d <= R[idx, None]
    return out


def box_matrix(lo, hi, tris):
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    T = np.asarray(tris, F).reshape(-1, 3, 3)
    tlo = np.fmin(np.fmin(T[:, 0], T[:, 1]), T[:, 2])
    thi = np.fmax(np.fmax(T[:, 0], T[:, 1]), T[:, 2])
    with np.errstate(invalid="ignore"):
        over = ((tlo[None] <= hi[:, None]) & (thi[None] >= lo[:, None])).all(axis=2)
    return over & traced_box(lo, hi)[:, None]


def sphere(points, dist2_max, tris):
    return _lists(sphere_matrix(points, dist2_max, tris))


def box(lo, hi, tris):
    return _lists(box_matrix(lo, hi, tris))


def offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


# ------------------------------------------------------------------ inputs of the CSR scan tests (range and all-hit ray queries)
SCAN_CHUNK_N = (256 * 1024, 256 * 1024 + 1, 256 * 1025 + 37)   # 1024, 1025 and 1026 workgroups of 256 queries


def scan_tiny_tris():
    """four triangles in the planes z = 1, 2, 3, 4; (0.2, 0.2, z) is well inside each"""
    return np.array([[[-1, -1, z], [3, -1, z], [-1, 3, z]] for z in (1, 2, 3, 4)], F)


def scan_reach_pattern(n):
    """a fixed pattern of reaches 0.5, 1.5 .. 4.5 from (0.2, 0.2, 0): 0 .. 4 of scan_tiny_tris() lie within; no period divides 256"""
    i = np.arange(n, dtype=np.int64)
    return ((i * 7 + i // 256) % 5).astype(F) + F(0.5)
