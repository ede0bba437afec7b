"""CPU tests of the numpy k-nearest reference (tests/knn_ref.py), the yardstick of tests/test_gpu_knn.py: k = 1 is the
closest-point brute force, rows ascend in (dist2, id), ties on dist2 go to the lower id, the radius is closed, short rows are
padded with (+inf, MISS), untraced queries and NaN distances are left out."""
import numpy as np

import knn_ref as kr
import point_ref as pr

F = np.float32


def _points(tris, n, seed):
    rng = np.random.default_rng(seed)
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return (lo + rng.random((n, 3)) * (hi - lo) * 1.2 - 0.1 * (hi - lo)).astype(F)


def test_k1_is_the_closest_point_brute_force(scenes):
    tris = scenes.soup(300, 5, size=0.1)
    p = _points(tris, 200, 1)
    for r in (np.inf, F(0.01)):
        d, i, _, _ = pr.brute_force(p, r, tris)
        rows = kr.brute_force_knn(p, r, tris, 1)
        assert rows.shape == (200, 1)
        assert (rows["dist2"][:, 0].view(np.uint32) == d.view(np.uint32)).all() and (rows["primitive_id"][:, 0] == i).all()
    assert (kr.brute_force_knn(p, F(0.01), tris, 1)["primitive_id"] == pr.MISS).any()    # the radius bites


def test_rows_ascend_and_smaller_k_is_a_prefix(scenes):
    tris = scenes.soup(300, 5, size=0.1)          # a quarter of the soup are exact copies: ties on dist2
    p = _points(tris, 100, 2)
    r32 = kr.brute_force_knn(p, np.inf, tris, 32)
    assert kr.ascending(r32) and (r32["primitive_id"] < 300).all()
    d = r32["dist2"]
    assert (d[:, 1:] == d[:, :-1]).any(), "the duplicated triangles must show as ties"
    for k in (1, 2, 7):
        assert (kr.brute_force_knn(p, np.inf, tris, k).view(np.uint32) == r32[:, :k].view(np.uint32)).all()
    # every row is the k smallest of the whole candidate set: nothing left out is below the last entry
    T = tris.reshape(-1, 3, 3)
    dall, _, _ = pr.d2(p[:, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])
    for q in range(len(p)):
        rest = np.setdiff1d(np.arange(300), r32["primitive_id"][q])
        assert (dall[q, rest] >= d[q, -1]).all()
        assert (dall[q, r32["primitive_id"][q]].view(np.uint32) == d[q].view(np.uint32)).all()
    assert not kr.ascending(r32[:, ::-1])


def test_points_on_grid_vertices_list_the_lowest_ids_first(scenes):
    G = 6
    tris = scenes.grid_mesh(G, 3)
    T = tris.reshape(-1, 3, 3)
    # interior vertex (i, j) is a corner of six triangles: cells (i-1, j-1) B, (i, j-1) A and B, (i-1, j) A and B, (i, j) A
    pts, want = [], []
    for i, j in ((1, 1), (3, 2), (5, 4)):
        cell = lambda ci, cj: 2 * (cj * G + ci)
        pts.append(T[cell(i, j), 0])
        want.append(sorted([cell(i - 1, j - 1) + 1, cell(i, j - 1), cell(i, j - 1) + 1, cell(i - 1, j), cell(i - 1, j) + 1,
                            cell(i, j)]))
    pts = np.array(pts, F)
    rows = kr.brute_force_knn(pts, np.inf, tris, 8)
    for q in range(3):
        assert (rows["dist2"][q, :6] == 0).all() and rows["dist2"][q, 6] > 0
        assert rows["primitive_id"][q, :6].tolist() == want[q]
    # k below the number of ties: the lowest ids
    rows = kr.brute_force_knn(pts, np.inf, tris, 4)
    for q in range(3):
        assert rows["primitive_id"][q].tolist() == want[q][:4]
    # radius 0 is closed: exactly the six
    rows = kr.brute_force_knn(pts, F(0), tris, 8)
    for q in range(3):
        assert rows["primitive_id"][q, :6].tolist() == want[q] and (rows["primitive_id"][q, 6:] == kr.MISS).all()


def test_radius_is_closed_and_rows_are_padded(scenes):
    tris = scenes.soup(200, 9, dup_fraction=0.0, size=0.1)
    p = _points(tris, 50, 3)
    full = kr.brute_force_knn(p, np.inf, tris, 8)
    for j in (0, 3, 7):
        r = full["dist2"][:, j]
        at = kr.brute_force_knn(p, r, tris, 8)
        assert (at[:, :j + 1].view(np.uint32) == full[:, :j + 1].view(np.uint32)).all()
        pos = r > 0
        below = kr.brute_force_knn(p, np.where(pos, np.nextafter(r, F(0)), r), tris, 8)
        assert (below["primitive_id"][pos, j] != full["primitive_id"][pos, j]).all()
        strict = full["dist2"][:, j - 1] < r if j else np.ones(len(p), bool)
        sel = pos & strict
        assert sel.any() and (below["primitive_id"][sel, j] == kr.MISS).all() and np.isinf(below["dist2"][sel, j]).all()
    # fewer triangles than k: padded
    rows = kr.brute_force_knn(p, np.inf, tris[:5], 8)
    assert (rows["primitive_id"][:, :5] < 5).all() and (rows["primitive_id"][:, 5:] == kr.MISS).all()
    assert np.isinf(rows["dist2"][:, 5:]).all() and kr.ascending(rows)
    assert np.sort(rows["primitive_id"][:, :5], axis=1).tolist() == [[0, 1, 2, 3, 4]] * len(p)
    # no triangles at all
    rows = kr.brute_force_knn(p, np.inf, tris[:0], 3)
    assert (rows["primitive_id"] == kr.MISS).all() and np.isinf(rows["dist2"]).all()


def test_untraced_queries_and_nan_distances_are_left_out(scenes):
    tris = scenes.soup(50, 4, dup_fraction=0.0, size=0.1)
    p = _points(tris, 8, 4)
    r = np.full(8, np.inf, F)
    p[0, 0], p[1, 1], p[2, 2] = np.nan, np.inf, -np.inf
    r[3], r[4], r[5] = np.nan, -1.0, -np.inf
    rows = kr.brute_force_knn(p, r, tris, 4)
    assert (rows["primitive_id"][:6] == kr.MISS).all() and np.isinf(rows["dist2"][:6]).all()
    assert (rows["primitive_id"][6:] < 50).all()
    # a triangle whose d2 is NaN (every corner NaN: nothing for fminf / fmaxf to keep) is not a candidate, even with an
    # infinite radius
    bad = tris.copy()
    bad[7] = np.nan
    d, _, _ = pr.d2(p[6], bad[7, 0:3], bad[7, 3:6], bad[7, 6:9])
    assert np.isnan(d)
    rows = kr.brute_force_knn(p[6:], np.inf, bad, 50)
    assert (rows["primitive_id"] != 7).all() and (rows["primitive_id"][:, 49] == kr.MISS).all()
    assert (rows["primitive_id"][:, :49] < 50).all() and kr.ascending(rows)
