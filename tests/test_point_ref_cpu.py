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


def test_collinear_triangles_with_rounding_residues():
    """c = a + w (b - a) rounded to float32: Ericson's va, vb, vc are then rounding residues of any sign, and a face point
    formed from them alone lies anywhere along the triangle, or off it.  (The collinear triangles of signed_zero_mesh have
    exact midpoints: their residues are zero.)  Found by the `points` scene of tests/small_scenes.py."""
    for seed, scale, off in ((15, 1, 0), (16, 1e-3, 0), (17, 1, 50), (18, 100, 0), (19, 0.01, 3)):
        rng = np.random.default_rng(seed)
        n = 4000
        a, b = ((rng.uniform(-1, 1, (n, 3)) * scale + off).astype(F) for _ in range(2))
        c = (a + (b - a) * rng.uniform(-0.5, 1.5, (n, 1)).astype(F)).astype(F)
        P = (rng.uniform(-1.5, 1.5, (n, 3)) * scale + off).astype(F)
        M = np.abs(np.concatenate([a, b, c, P], 1)).max(1).astype(np.float64)
        for corners in ((a, b, c), (c, a, b), (b, c, a)):
            d, u, v = pr.d2(P, *corners)
            assert np.isfinite(d).all() and ((u >= 0) & (v >= 0) & (u + v <= 1 + 1e-6)).all()
            err = _rel_err(d, pr.closest_f64(P, *corners), M)
            assert err.max() <= 8, f"scale {scale} at {off}: {err.max():.1f} ulps of the largest coordinate on {(err > 8).sum()} of {n}"


def test_a_repeated_corner_in_any_position():
    """Ericson's region of an edge of two equal corners would answer by that corner whatever the other edge offers
    (signed_zero_mesh repeats the LAST corner only, which never reaches that region)"""
    rng = np.random.default_rng(20)
    n = 3000
    a, b = rng.uniform(-1, 1, (n, 3)).astype(F), rng.uniform(-1, 1, (n, 3)).astype(F)
    P = rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    for corners in ((a, a, b), (a, b, a), (b, a, a), (a, b, b)):
        d, _, _ = pr.d2(P, *corners)
        assert _rel_err(d, pr.closest_f64(P, *corners), 1.5).max() <= 8


def _collinear_errors(n):
    """ulps of the largest coordinate between d2 and float64 on 15 n collinear triangles: five scales and offsets, the three
    rotations of the corners"""
    out = []
    for seed, scale, off in ((1, 1, 0), (2, 1e-3, 0), (3, 1, 50), (4, 100, 0), (5, 0.01, 3)):
        rng = np.random.default_rng(seed)
        a, b = ((rng.uniform(-1, 1, (n, 3)) * scale + off).astype(F) for _ in range(2))
        c = (a + (b - a) * rng.uniform(-0.5, 1.5, (n, 1)).astype(F)).astype(F)
        P = (rng.uniform(-1.5, 1.5, (n, 3)) * scale + off).astype(F)
        M = np.abs(np.concatenate([a, b, c, P], 1)).max(1).astype(np.float64)
        for corners in ((a, b, c), (c, a, b), (b, c, a)):
            out.append(_rel_err(pr.d2(P, *corners)[0], pr.closest_f64(P, *corners), M))
    return np.concatenate(out)


def test_the_noise_factor_is_where_the_sweep_puts_it(monkeypatch):
    """FACE_NOISE = 2^-20: on 150,000 collinear triangles the factors 2^-17 .. 2^-21 leave none more than 8 ulps from float64,
    2^-22 and below let noise through as a face; a negative factor is Ericson's rule itself (s > 0 alone)"""
    assert pr.FACE_NOISE == F(2.0 ** -20)
    bad = {}
    for e in (-17, -20, -21, -23, None):
        monkeypatch.setattr(pr, "FACE_NOISE", F(-1) if e is None else F(2.0 ** e))
        err = _collinear_errors(10000)
        bad[e] = int((err > 8).sum())
        print(f"FACE_NOISE {'none (Ericson)' if e is None else f'2^{e}'}: {bad[e]} of {err.size} beyond 8 ulps, worst {err.max():.1f}")
    assert bad[-17] == 0 and bad[-20] == 0 and bad[-21] == 0, bad
    assert bad[-23] > 0 and bad[None] > 100, f"the sample does not need the gate: {bad}"


def _pairs_that_differ(tris, points, monkeypatch):
    """(d2 under the rule, d2 under Ericson's face rule, float64 distance) of the (point, triangle) pairs whose d2 differs"""
    T = tris.reshape(-1, 3, 3)
    new, old, ref = [], [], []
    for s0 in range(0, len(points), 64):
        q = points[s0:s0 + 64]
        monkeypatch.setattr(pr, "FACE_NOISE", F(2.0 ** -20))
        dn = pr.d2(q[:, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])[0]
        monkeypatch.setattr(pr, "FACE_NOISE", F(-1))             # s > -noise: Ericson's s > 0 alone, overflowed products too
        do = pr.d2(q[:, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])[0]
        i, j = np.nonzero(dn.view(np.uint32) != do.view(np.uint32))
        new.append(dn[i, j]); old.append(do[i, j]); ref.append(pr.closest_f64(q[i], T[j, 0], T[j, 1], T[j, 2]))
    return np.concatenate(new), np.concatenate(old), np.concatenate(ref)


def test_the_gate_changes_ordinary_scenes_nowhere_and_the_fractal_toward_float64(scenes, monkeypatch):
    """With a negative FACE_NOISE the face rule is Ericson's.  On the grid and soup scenes with the GPU tests' point sets no
    (point, triangle) pair has another d2 under the gate.  On the fractal scene some do: its coordinates reach 2^45, the
    products overflow, s and the noise are both infinite and the face weights NaN -- an infinite noise is never cleared, so
    the edges answer, and the gated value is the one closer to float64"""
    from test_gpu_point_queries import _point_sets
    from test_gpu_ray_queries import _scene
    for name in ("grid", "soup"):
        tris = np.ascontiguousarray(_scene(name, scenes)[0], F).reshape(-1, 9)
        for kind, p in _point_sets(tris, sum(name.encode())).items():
            new, _, _ = _pairs_that_differ(tris, p[:256], monkeypatch)
            assert new.size == 0, f"{name}/{kind}: {new.size} pairs change"
    tris = np.ascontiguousarray(_scene("fractal", scenes)[0], F).reshape(-1, 9)
    sets = _point_sets(tris, sum(b"fractal"))
    new, old, ref = (np.concatenate(x) for x in zip(*(_pairs_that_differ(tris, sets[k][:256], monkeypatch)
                                                      for k in ("near", "on_vertex_edge"))))
    with np.errstate(all="ignore"):
        en, eo = (np.abs(np.sqrt(d.astype(np.float64)) - ref) / np.maximum(ref, 1e-300) for d in (new, old))
    closer = int((en < eo).sum())
    print(f"fractal: {new.size} pairs differ, the gated d2 is closer to float64 in {closer}; median relative error "
          f"{np.median(en):.2e} against {np.median(eo):.2e}")
    assert new.size >= 100 and closer >= 0.99 * new.size and np.median(en) < 1e-3 * np.median(eo)
