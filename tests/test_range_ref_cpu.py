"""CPU tests of the range-query restatement (tests/range_ref.py) that the GPU tests hold the kernels to:
1. against float64: a triangle whose float64 distance is clearly inside or clearly outside the radius is classified the same
   way (those within a few ulps of the radius are excluded); the box predicate equals a float64 interval test exactly (it only
   compares);
2. against the closest-point restatement: a sphere set is non-empty iff point_ref.brute_force hits within the same dist2_max,
   and the closest triangle is a member;
3. the not-traced rules, the closed edges (radius exactly at d2, a box face exactly on a vertex, -0 against +0);
4. every (scene, query set) the GPU test runs returns something for at least a quarter of its queries and at least NQ ids in
   total, by the reference alone -- a GPU test over empty sets cannot pass."""
import numpy as np
import pytest

import point_ref as pr
import range_ref as rr
import range_sets as rs

F = np.float32


def test_sphere_classification_matches_float64():
    rng = np.random.default_rng(31)
    for scale in (1e-3, 1.0, 1e3):
        T = (rng.uniform(-1, 1, (300, 3, 3)) * scale).astype(F)
        P = (rng.uniform(-1.5, 1.5, (200, 3)) * scale).astype(F)
        R = ((rng.uniform(0.05, 1.5, 200) * scale) ** 2).astype(F)
        got = rr.sphere_matrix(P, R, T.reshape(-1, 9))
        d64 = pr.closest_f64(P[:, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])
        r64 = np.sqrt(R.astype(np.float64))[:, None]
        M = max(float(np.abs(T).max()), float(np.abs(P).max()))
        tol = 16 * M * 2.0 ** -23             # a few ulps of the largest coordinate (the d2 accuracy test allows 8)
        inside, outside = d64 < r64 - tol, d64 > r64 + tol
        assert inside.sum() > 1000 and outside.sum() > 1000
        assert got[inside].all() and not got[outside].any()


def test_box_predicate_is_an_interval_test():
    rng = np.random.default_rng(32)
    T = rng.uniform(-1, 1, (500, 3, 3)).astype(F)
    c = rng.uniform(-1, 1, (300, 3)).astype(F)
    h = rng.uniform(0, 0.4, (300, 3)).astype(F)
    lo, hi = (c - h).astype(F), (c + h).astype(F)
    got = rr.box_matrix(lo, hi, T.reshape(-1, 9))
    T64 = T.astype(np.float64)
    tlo, thi = T64.min(1), T64.max(1)
    exp = ((tlo[None] <= hi[:, None].astype(np.float64)) & (thi[None] >= lo[:, None].astype(np.float64))).all(2)
    assert (got == exp).all() and got.any() and not got.all()
    lists, counts = rr.box(lo, hi, T.reshape(-1, 9))
    assert (counts == exp.sum(1)).all() and all((np.diff(x.astype(np.int64)) > 0).all() for x in lists)
    assert (rr.offsets(counts) == np.concatenate([[0], np.cumsum(exp.sum(1))])).all()


def test_sphere_sets_agree_with_the_closest_point(scenes):
    tris = rs.scene_tris("soup", scenes)
    sets = rs.query_sets(tris, 5)
    for kind in ("near", "uniform", "on_vertex_edge"):
        q = sets["sphere", kind]
        lists, counts = rr.sphere(q["p"], q["dist2_max"], tris)
        d, i, _, _ = pr.brute_force(q["p"], q["dist2_max"], tris)
        assert ((counts > 0) == (i != pr.MISS)).all()
        assert all(i[k] in lists[k] for k in np.nonzero(counts)[0])


def test_not_traced_and_closed_edges():
    tris = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 2, 1, 0, 2, 0, 1, 2]], F)
    P = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, 0, -np.inf], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]], F)
    R = np.array([np.inf, np.inf, np.inf, np.nan, -1.0, -np.inf, np.inf, 1.0], F)
    lists, counts = rr.sphere(P, R, tris)
    assert (counts == [0, 0, 0, 0, 0, 0, 2, 2]).all()                       # +inf: everything; exactly at the radius: both
    _, counts = rr.sphere(P[7:], np.nextafter(F(1), F(0)), tris)
    assert counts[0] == 0                                                   # the next float below rejects
    _, counts = rr.sphere(P[7:], F(-0.0), tris)
    assert counts[0] == 0                                                   # -0 is a radius of 0: traced, nothing that near
    _, counts = rr.sphere(np.zeros((1, 3), F), F(-0.0), tris)
    assert counts[0] == 1                                                   # ... but a point on the triangle is
    # boxes: NaN or lo > hi is not traced; a face exactly on a vertex coordinate accepts; -0 against +0 accepts
    lo = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0.5, 0, 0], [-1, -1, -0.0], [-1, -1, -1], [1, 1, 0]], F)
    hi = np.array([[1, 1, 2], [1, 1, 0], [1, 1, 1], [0.25, 1, 1], [-0.0, -0.0, 0.0], [np.nextafter(F(0), F(-1)), 1, 1], [2, 2, 0]], F)
    _, counts = rr.box(lo, hi, tris)
    assert (counts == [2, 1, 0, 0, 1, 0, 1]).all()
    assert not rr.traced_box(lo, hi)[2] and not rr.traced_box(lo, hi)[3] and rr.traced_box(lo, hi)[4]


@pytest.mark.parametrize("name", rs.SCENES)
def test_the_gpu_query_sets_are_not_empty(scenes, name):
    tris = rs.scene_tris(name, scenes)
    sets = rs.query_sets(tris, rs.seed_of(name))
    assert len(sets) == 6
    for (shape, kind), q in sets.items():
        if shape == "sphere":
            _, counts = rr.sphere(q["p"], q["dist2_max"], tris)
        else:
            _, counts = rr.box(q["lo"], q["hi"], tris)
        assert len(counts) == rs.NQ
        print(f"{name}/{shape}/{kind}: non-empty {int((counts > 0).sum())}/{rs.NQ}, ids {int(counts.sum())}, "
              f"largest {int(counts.max())}")
        assert (counts > 0).sum() * 4 >= rs.NQ, f"{name}/{shape}/{kind}: only {(counts > 0).sum()} non-empty sets"
        assert counts.sum() >= rs.NQ, f"{name}/{shape}/{kind}: only {counts.sum()} ids"
