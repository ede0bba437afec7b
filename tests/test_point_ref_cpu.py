"""CPU tests of the closest-point restatement (tests/point_ref.py) that the GPU tests hold the kernel to: it is accurate
against float64 on ordinary triangles, gives finite, correct distances on the three degenerate kinds of
edge_scenes.signed_zero_mesh, breaks ties on dist2 toward the lower id, and keeps dist2 >= boxdist2 in float32 for points
on and just outside box faces (the inequality the exact pruning rests on)."""
import numpy as np

import edge_scenes
import point_ref as pr

F = np.float32
ULP = 2.0 ** -23


def _rel_err(d32, d64, scale):
    return np.abs(np.sqrt(d32.astype(np.float64)) - d64) / (scale * ULP)


def test_restatement_matches_float64_on_random_triangles():
    rng = np.random.default_rng(11)
    for scale in (1e-3, 1.0, 1e3):
        T = (rng.uniform(-1, 1, (4000, 3, 3)) * scale).astype(F)
        P = (rng.uniform(-2, 2, (4000, 3)) * scale).astype(F)
        d, u, v = pr.d2(P, T[:, 0], T[:, 1], T[:, 2])
        d64 = pr.closest_f64(P, T[:, 0], T[:, 1], T[:, 2])
        M = np.maximum(np.abs(T).reshape(len(T), -1).max(1), np.abs(P).max(1)).astype(np.float64)
        err = _rel_err(d, d64, M)
        assert err.max() <= 8, f"scale {scale}: {err.max():.2f} ulps of the largest coordinate"
        # (u, v) is the closest point: (1-u-v) a + u b + v c, within the same tolerance (before the box clamp)
        assert ((u >= 0) & (v >= 0) & (u + v <= 1 + 1e-6)).all()
        q = (1 - u - v)[:, None].astype(np.float64) * T[:, 0] + u[:, None] * T[:, 1] + v[:, None] * T[:, 2].astype(np.float64)
        dq = np.sqrt(((q - P) ** 2).sum(1))
        assert (np.abs(dq - d64) / (M * ULP)).max() <= 64


def test_points_on_the_triangle_are_at_distance_zero():
    rng = np.random.default_rng(12)
    T = rng.uniform(-1, 1, (500, 3, 3)).astype(F)
    for k in range(3):
        d, u, v = pr.d2(T[:, k], T[:, 0], T[:, 1], T[:, 2])
        assert (d == 0).all()
        assert (u == (k == 1)).all() and (v == (k == 2)).all()


def test_degenerate_triangles(scenes):
    t = edge_scenes.signed_zero_mesh(scenes).reshape(-1, 3, 3)
    point = (t[:, 0] == t[:, 1]).all(1) & (t[:, 1] == t[:, 2]).all(1)
    repeated = ~point & ((t[:, 1] == t[:, 2]).all(1) | (t[:, 0] == t[:, 1]).all(1))
    cr = np.cross((t[:, 1] - t[:, 0]).astype(np.float64), (t[:, 2] - t[:, 0]).astype(np.float64))
    collinear = ~point & ~repeated & (np.abs(cr).max(1) <= 1e-5)
    assert point.sum() >= 4 and repeated.sum() >= 4 and collinear.sum() >= 4
    rng = np.random.default_rng(13)
    P = rng.uniform(-14, 14, (3000, 3)).astype(F)
    P[:50] = t[point][0][0]                                      # some points exactly on a degenerate corner
    for sel in (point, repeated, collinear):
        for tri in t[sel]:
            d, u, v = pr.d2(P, tri[0], tri[1], tri[2])
            assert np.isfinite(d).all() and np.isfinite(u).all() and np.isfinite(v).all()
            d64 = pr.closest_f64(P, tri[0], tri[1], tri[2])
            M = max(float(np.abs(tri).max()), 14.0)
            assert _rel_err(d, d64, M).max() <= 8
    # the point-triangle is its vertex
    tri = t[point][0]
    d, _, _ = pr.d2(P, tri[0], tri[1], tri[2])
    exp = ((P - tri[0]) ** 2).astype(F)
    assert (d == (exp[:, 0] + exp[:, 1]) + exp[:, 2]).all()


def test_ties_go_to_the_lower_id(scenes):
    tris = scenes.grid_mesh(8, 2).reshape(-1, 3, 3)
    # every vertex of the mesh is shared by several triangles: the query on it reports dist2 0 and the lowest id touching it
    verts = tris.reshape(-1, 3)
    pts = np.unique(verts, axis=0)[:40]
    d, i, u, v = pr.brute_force(pts, np.full(len(pts), np.inf, F), tris.reshape(-1, 9))
    assert (d == 0).all()
    for k, p in enumerate(pts):
        owners = np.nonzero((tris == p).all(2).any(1))[0]
        assert i[k] == owners.min(), (p, owners, i[k])
    # the radius: exactly at the minimum is a hit, one float below is a miss
    P = np.array([[0.3, 5.0, 0.7], [2.2, -3.0, 4.1]], F)
    d, i, _, _ = pr.brute_force(P, np.full(2, np.inf, F), tris.reshape(-1, 9))
    d2, i2, _, _ = pr.brute_force(P, d, tris.reshape(-1, 9))
    assert (d2 == d).all() and (i2 == i).all()
    d3, i3, _, _ = pr.brute_force(P, np.nextafter(d, F(0)), tris.reshape(-1, 9))
    assert (i3 == pr.MISS).all() and np.isinf(d3).all()


def test_untraced_queries_miss():
    tris = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], F)
    P = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, 0, -np.inf], [0, 0, 1], [0, 0, 1], [0, 0, 1]], F)
    R = np.array([np.inf, np.inf, np.inf, np.nan, -1.0, -0.0], F)
    d, i, u, v = pr.brute_force(P, R, tris)
    assert (i[:5] == pr.MISS).all() and np.isinf(d[:5]).all() and (u[:5] == 0).all() and (v[:5] == 0).all()
    assert i[5] == pr.MISS                 # -0 is a radius of 0: a traced query, but the triangle is at distance 1
    d, i, _, _ = pr.brute_force(P[5:], np.array([1.0], F), tris)
    assert i[0] == 0 and d[0] == 1


def test_monotone_on_adversarial_points():
    """dist2 >= boxdist2 for every box that contains the vertex box -- points on box faces, one ulp either side, -0 / +0"""
    rng = np.random.default_rng(14)
    T = rng.uniform(-3, 3, (3000, 3, 3)).astype(F)
    T[:300] = np.where(rng.random((300, 3, 3)) < 0.5, F(0), T[:300]) * np.where(rng.random((300, 3, 3)) < 0.5, F(-1), F(1))
    lo, hi = T.min(1), T.max(1)
    grow = rng.uniform(0, 0.5, (len(T), 2, 3)).astype(F) * (rng.random((len(T), 2, 3)) < 0.5)
    blo, bhi = (lo - grow[:, 0]).astype(F), (hi + grow[:, 1]).astype(F)
    for k in range(12):
        axis = k % 3
        P = rng.uniform(-4, 4, (len(T), 3)).astype(F)
        face = blo[:, axis] if k < 6 else bhi[:, axis]
        if k % 6 < 2:
            P[:, axis] = face
        elif k % 6 < 4:
            P[:, axis] = np.nextafter(face, F(-np.inf) if k < 6 else F(np.inf))
        else:
            P[:, axis] = np.where(face == 0, F(-0.0), np.nextafter(face, F(0)))
        P = np.where(rng.random(P.shape) < 0.1, F(-0.0), P)
        for box in ((lo, hi), (blo, bhi)):
            d, _, _ = pr.d2(P, T[:, 0], T[:, 1], T[:, 2])
            assert (d >= pr.box_d2(P, *box)).all()
