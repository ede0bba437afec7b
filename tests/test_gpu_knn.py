"""GPU tests of the k-nearest queries (rt_k_nearest) on every tree the builders make.

1. rows bit-equal to the numpy brute force (tests/knn_ref.py) on the six non-split tree kinds of five scenes, for k in
   {1, 2, 7, 32} and near-surface, uniform, on-vertex / on-edge (ties on dist2) and far points -- and so identical across trees;
2. k = 1 against rt_closest_points on the same queries: (dist2, id) bit-equal;
3. batch sizes 1, 63, 257, 1000: rows past num_queries keep their fill, a row does not depend on its neighbours;
4. the radius: exactly at rank j's dist2 keeps it, one float below drops it; padded rows; untraced queries; an empty tree;
5. the ids of a row as a set equal the sphere range query's set when fewer than k triangles lie within the radius;
6. split trees: records real bit for bit, ids distinct, rows ascending, each rank within the documented bound; exact after a refit;
7. refit of non-split trees: rows equal the brute force over the moved triangles;
8. the deep fractal trees and wide collapsed trees: exact with status 0;
9. hand-built trees with more than 64 pending entries: RT_KNN_STACK_OVERFLOW with real, distinct, sorted records when the
   restarts cannot avoid the overflow; the exact row with status 0 when a restart drops nothing;
10. build + query + counters captured in one HIP graph replay the eager rows and counters;
11. counters are deterministic."""
import numpy as np
import pytest

import edge_scenes
import knn_ref as kr
import point_ref as pr
import range_ref as rr
from test_gpu_point_queries import (EXACT_TREES, SPLIT_TREES, SCENES, Trees, _closest, _comb, _comb_triangles, _download, _move,
                                    _point_sets, _queries)
from test_gpu_ray_queries import _gpu_tree, _scene

pytestmark = pytest.mark.gpu

F = np.float32
NP = 256                  # points per query set
KS = (1, 2, 7, 32)


# ------------------------------------------------------------------ helpers
@pytest.fixture(scope="module")
def trees(rt, scenes):
    return Trees(rt, scenes)


_SETS, _EXP32 = {}, {}


def _sets(tris, key, seed):
    """the four point sets of test_gpu_point_queries, NP points each (computed once per key)"""
    if key not in _SETS:
        _SETS[key] = {k: np.ascontiguousarray(p[:NP]) for k, p in _point_sets(tris, seed).items()}
    return _SETS[key]


def _exp32(tris, key, seed):
    """the brute-force rows for k = 32 and an infinite radius (computed once per key); the rows for a smaller k are their prefix"""
    if key not in _EXP32:
        _EXP32[key] = {k: kr.brute_force_knn(p, np.inf, tris, 32) for k, p in _sets(tris, key, seed).items()}
        for e in _EXP32[key].values():
            e.setflags(write=False)
    return _EXP32[key]


def _knn(rt, triangles, nodes, root, count, queries, k, counters=False, status=False, n_alloc=None):
    """queries: POINT_QUERY numpy array -> (KNN_HIT array [n_alloc or n, k], counters uint64[4] or None, status or None)"""
    import torch
    q = rt.to_device(np.ascontiguousarray(queries, rt.POINT_QUERY)).view(torch.float32).view(-1, 4)
    n = q.shape[0]
    out = torch.full((n_alloc or n, k, 2), 7.0, dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda") if counters else None
    st = torch.zeros(1, dtype=torch.int32, device="cuda") if status else None
    assert rt.KNearest(triangles, nodes, root, count, q, k, out[:n], counters=ctr, status=st) == n
    torch.cuda.synchronize()
    rows = out.cpu().numpy().view(rt.KNN_HIT).reshape(-1, k)
    return (rows, ctr.cpu().numpy().astype(np.uint64) if counters else None, rt.knn_status(st) if status else None)


def _knn_tree(rt, g, queries, k, **kw):
    inp, root, count = g
    return _knn(rt, inp.triangles_out, inp.nodes_out, root, count, queries, k, **kw)


def _assert_rows_equal(got, exp, what):
    g, e = got.view(np.uint32).reshape(len(got), -1), exp.view(np.uint32).reshape(len(exp), -1)
    assert g.shape == e.shape, f"{what}: shapes {g.shape} and {e.shape}"
    bad = np.nonzero((g != e).any(1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rows differ, first at {bad[:5]}: got {got[bad[0]]} expected {exp[bad[0]]}")


def _assert_real_distinct_sorted(rows, p, tris, what):
    """every non-miss record is d2(p, tri[id]) bit for bit, a row holds no id twice, rows ascend, misses come last"""
    T = tris.reshape(-1, 3, 3)
    ids = rows["primitive_id"]
    real = ids != kr.MISS
    assert (ids[real] < T.shape[0]).all(), f"{what}: an id beyond the scene"
    assert np.isinf(rows["dist2"][~real]).all()
    safe = np.where(real, ids, 0)
    d, _, _ = pr.d2(p[:, None, :], T[safe, 0], T[safe, 1], T[safe, 2])
    assert (rows["dist2"].view(np.uint32)[real] == d.view(np.uint32)[real]).all(), f"{what}: a dist2 that is not d2(p, tri[id])"
    for r in range(len(rows)):
        assert len(set(ids[r][real[r]].tolist())) == int(real[r].sum()), f"{what}: row {r} holds an id twice: {ids[r]}"
    assert kr.ascending(rows), f"{what}: a row is not ascending in (dist2, id)"


# ------------------------------------------------------------------ 1: exact on every non-split tree
@pytest.mark.parametrize("name", SCENES)
def test_rows_equal_the_brute_force_on_every_tree(rt, trees, name):
    tris = trees.tris(name)
    seed = sum(name.encode())
    sets, exp = _sets(tris, name, seed), _exp32(tris, name, seed)
    e = exp["on_vertex_edge"]
    ties = (e["dist2"][:, 1:] == e["dist2"][:, :-1]) & (e["primitive_id"][:, 1:] != kr.MISS)
    # (the fractal's triangles share no corner: a point on one of them is at distance 0 from that one alone)
    assert ties.any() or name == "fractal", f"{name}: the on-vertex / on-edge points must give ties on dist2"
    for tree in EXACT_TREES:
        g = trees.gpu(name, tree)
        for k in KS:
            for key, p in sets.items():
                got, ctr, st = _knn_tree(rt, g, _queries(p), k, counters=True, status=True)
                _assert_rows_equal(got, exp[key][:, :k], f"{name}/{tree}/k={k}/{key}")
                assert st == 0 and ctr[0] > 0 and ctr[1] >= len(p) and ctr[2] == 0 and ctr[3] == 0


# ------------------------------------------------------------------ 2: k = 1 is the closest-point query
@pytest.mark.parametrize("name", SCENES)
def test_k1_equals_closest_points(rt, trees, name):
    tris = trees.tris(name)
    sets = _sets(tris, name, sum(name.encode()))
    kinds = ("bottom_up", "sah_pairs") + (() if name == "fractal" else SPLIT_TREES)
    for tree in kinds:
        inp, root, count = trees.gpu(name, tree)
        for key in ("near", "on_vertex_edge", "uniform"):
            q = _queries(sets[key])
            got, _, _ = _knn_tree(rt, (inp, root, count), q, 1)
            hits, _, _ = _closest(rt, inp.triangles_out, inp.nodes_out, root, count, q)
            assert (got["dist2"][:, 0].view(np.uint32) == hits["dist2"].view(np.uint32)).all(), f"{name}/{tree}/{key}"
            assert (got["primitive_id"][:, 0] == hits["primitive_id"]).all(), f"{name}/{tree}/{key}"


# ------------------------------------------------------------------ 3: batch sizes
@pytest.mark.parametrize("n", (1, 63, 257, 1000))
def test_batch_sizes_fill_and_shuffle(rt, trees, n):
    tris = trees.tris("grid")
    g = trees.gpu("grid", "hybrid_pairs")
    full = _point_sets(tris, seed=31)
    p = np.concatenate([full["near"][:(n + 1) // 2], full["uniform"]])[:n]
    k = 7
    got, _, st = _knn_tree(rt, g, _queries(p), k, status=True, n_alloc=n + 50)
    assert st == 0
    assert (got[n:].view(np.float32) == 7.0).all(), "rows past num_queries were written"
    _assert_rows_equal(got[:n], kr.brute_force_knn(p, np.inf, tris, k), f"batch of {n}")
    perm = np.random.default_rng(n).permutation(n)
    shuffled, _, _ = _knn_tree(rt, g, _queries(p[perm]), k)
    _assert_rows_equal(shuffled, got[:n][perm], f"batch of {n}, shuffled")


# ------------------------------------------------------------------ 4: radius, padding, untraced queries, an empty tree
def test_radius_padding_untraced_and_empty_tree(rt, trees):
    tris = trees.tris("soup")
    g = trees.gpu("soup", "sah_pairs")
    p = _sets(tris, "soup", sum(b"soup"))["uniform"][:200]
    k = 8
    full = kr.brute_force_knn(p, np.inf, tris, k)
    for j in (0, 3, 7):
        r = full["dist2"][:, j].copy()
        # exactly at rank j's dist2: ranks 0 .. j are there
        got, _, _ = _knn_tree(rt, g, _queries(p, r), k)
        _assert_rows_equal(got, kr.brute_force_knn(p, r, tris, k), f"radius = rank {j}")
        _assert_rows_equal(got[:, :j + 1], full[:, :j + 1], f"radius = rank {j}: the ranks up to it")
        # one float below: rank j is gone
        pos = r > 0
        below = np.where(pos, np.nextafter(r, F(0)), r)
        got, _, _ = _knn_tree(rt, g, _queries(p, below), k)
        exp = kr.brute_force_knn(p, below, tris, k)
        _assert_rows_equal(got, exp, f"radius below rank {j}")
        strict = pos & ((full["dist2"][:, j - 1] < r) if j else True)
        assert strict.sum() > 100 and (got["primitive_id"][strict, j] == kr.MISS).all()
    # a 5-triangle scene with k = 8: three misses behind five records
    five = np.ascontiguousarray(tris[:5])
    got, _, st = _knn_tree(rt, _gpu_tree(rt, five, "bottom_up"), _queries(p), k, status=True)
    assert st == 0
    _assert_rows_equal(got, kr.brute_force_knn(p, np.inf, five, k), "five triangles")
    assert (got["primitive_id"][:, :5] < 5).all() and (got["primitive_id"][:, 5:] == kr.MISS).all()
    assert np.isinf(got["dist2"][:, 5:]).all()
    # untraced: non-finite p, NaN or negative radius -> rows of {+inf, MISS} and no tests counted
    bad = _queries(p[:6])
    bad["p"][0, 0], bad["p"][1, 1], bad["p"][2, 2] = np.nan, np.inf, -np.inf
    bad["dist2_max"][3], bad["dist2_max"][4], bad["dist2_max"][5] = np.nan, -1.0, -np.inf
    got, ctr, _ = _knn_tree(rt, g, bad, k, counters=True)
    assert (got["primitive_id"] == kr.MISS).all() and np.isinf(got["dist2"]).all() and (got["dist2"] > 0).all()
    assert (ctr == 0).all()
    # an empty tree: every row is misses, nothing counted
    inp = g[0]
    got, ctr, _ = _knn(rt, inp.triangles_out, inp.nodes_out, 0, 0, _queries(p[:10]), k, counters=True)
    assert (got["primitive_id"] == kr.MISS).all() and np.isinf(got["dist2"]).all() and (ctr == 0).all()


# ------------------------------------------------------------------ 5: consistency with the sphere range query
def test_row_ids_equal_the_range_query_set(rt, trees):
    import torch
    tris = trees.tris("grid")
    p = _sets(tris, "grid", sum(b"grid"))["near"]
    r2 = F(1.0)
    lists, counts = rr.sphere(p, np.full(len(p), r2, F), tris)
    assert 0 < counts.max() < 32 and counts.min() >= 1, "the radius must leave every row short of k = 32"
    q = _queries(p, r2)
    for tree in ("pairs", "sah"):
        inp, root, count = trees.gpu("grid", tree)
        got, _, st = _knn_tree(rt, (inp, root, count), q, 32, status=True)
        assert st == 0
        off, ids = rt.RangeQuery(inp.triangles_out, inp.nodes_out, root, count, rt.to_device(q).view(torch.float32))
        off, ids = off.cpu().numpy(), ids.cpu().numpy().view(np.uint32)
        for i in range(len(p)):
            row = got["primitive_id"][i]
            mine = row[row != kr.MISS]
            theirs = ids[off[i]:off[i + 1]]
            assert len(mine) == len(theirs) == counts[i] and set(mine.tolist()) == set(theirs.tolist()), f"{tree}: query {i}"


# ------------------------------------------------------------------ 6: split trees
@pytest.mark.parametrize("name", ("grid", "soup", "cornell", "signed_zero"))
def test_split_trees_are_real_distinct_sorted_and_within_the_bound(rt, trees, name):
    tris = trees.tris(name)
    T = tris.reshape(-1, 3, 3)
    seed = sum(name.encode())
    sets, exp = _sets(tris, name, seed), _exp32(tris, name, seed)
    for tree in SPLIT_TREES:
        g = trees.gpu(name, tree)
        for k in (7, 32):
            for key, p in sets.items():
                got, _, st = _knn_tree(rt, g, _queries(p), k, status=True)
                assert st == 0
                what = f"{name}/{tree}/k={k}/{key}"
                assert (got["primitive_id"] < T.shape[0]).all(), f"{what}: a miss with an infinite radius"
                _assert_real_distinct_sorted(got, p, tris, what)
                bf = exp[key][:, :k]
                assert (got["dist2"] >= bf["dist2"]).all(), what
                M = max(float(np.abs(T).max()), float(np.abs(p).max()))
                excess = np.sqrt(got["dist2"].astype(np.float64)) - np.sqrt(bf["dist2"].astype(np.float64))
                assert excess.max() <= 2.0 ** -20 * M, f"{what}: {excess.max()} beyond 2^-20 * {M}"


# ------------------------------------------------------------------ 6 (refit of a split tree) + 7: refit
@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs", "sah_splits", "sah_pairs_splits"))
def test_refit_then_query_is_exact(rt, scenes, tree):
    import torch
    tris = _scene("grid", scenes)[0]
    inp, root, count = _gpu_tree(rt, np.ascontiguousarray(tris, F), tree)
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    moved = _move(tris, 1.5)
    inp.triangles_in.copy_(rt.to_device(moved))
    rt.Refit(inp, root, count, plan)
    torch.cuda.synchronize()
    assert rt.refit_status(plan, inp.num_triangles) == 0
    sets = _point_sets(moved, seed=15)
    for key in ("near", "on_vertex_edge"):
        p = sets[key][:NP]
        got, _, st = _knn_tree(rt, (inp, root, count), _queries(p), 7, status=True)
        assert st == 0
        _assert_rows_equal(got, kr.brute_force_knn(p, np.inf, moved, 7), f"refit {tree}/{key}")


# ------------------------------------------------------------------ 8: deep and wide trees
def test_deep_and_wide_trees_are_exact(rt, trees):
    tris = trees.tris("fractal")
    seed = sum(b"fractal")
    p, exp = _sets(tris, "fractal", seed)["near"], _exp32(tris, "fractal", seed)["near"]
    for tree in ("bottom_up", "sah", "hybrid"):
        for k in (1, 7):
            got, _, st = _knn_tree(rt, trees.gpu("fractal", tree), _queries(p), k, status=True)
            assert st == 0
            _assert_rows_equal(got, exp[:, :k], f"fractal/{tree}/k={k}")
    tris = trees.tris("grid")
    seed = sum(b"grid")
    sets, exp = _sets(tris, "grid", seed), _exp32(tris, "grid", seed)
    inp, root, count = trees.gpu("grid", "bottom_up")
    nodes, leaves = _download(rt, inp, tris.shape[0])
    for width in (3, 4, 7):
        wn, wr, wc = edge_scenes.collapse_wide(nodes, root, count, width, rt.NODE)
        wd = rt.to_device(wn)
        for k in (1, 7):
            for key in ("near", "uniform"):
                got, _, st = _knn(rt, inp.triangles_out, wd, wr, wc, _queries(sets[key]), k, status=True)
                assert st == 0
                _assert_rows_equal(got, exp[key][:, :k], f"width {width}/k={k}/{key}")


# ------------------------------------------------------------------ 9: stack overflow
def test_stack_overflow_is_flagged_and_the_rows_are_real_distinct_and_sorted(rt):
    """80 pending leaves on every pass (every box around the query point); the nearest triangle is among the dropped pushes,
    so the first pass and both restarts miss it: the flag is set, and the rows -- whose triangles every restart met again --
    hold real records, each id once, in order"""
    L = 80
    rng = np.random.default_rng(5)
    tris = _comb_triangles(rng, L, lambda k: 2.0 + k % 7 if k != 70 else 1.0)   # triangle 70 (pushed at depth 71): nearest
    leaves, nodes = _comb(rt, tris, tight_leaf_boxes=False)
    flat = tris.reshape(-1, 9)
    p = np.zeros((4, 3), F)
    p[1:] = rng.uniform(-0.05, 0.05, (3, 3))
    visited = np.array(list(range(64)) + [L])         # per pass: the bottom leaf and the 64 kept pushes
    got, ctr, st = _knn(rt, leaves, nodes, 0, 2, _queries(p), 4, counters=True, status=True)
    assert st & rt.RT_KNN_STACK_OVERFLOW
    _assert_real_distinct_sorted(got, p, flat, "loose comb, k = 4")
    assert (got["primitive_id"] != kr.MISS).all()
    bf = kr.brute_force_knn(p, np.inf, flat, 4)
    assert (bf["primitive_id"][:, 0] == 70).all() and (got["primitive_id"] != 70).all()   # the nearest was dropped: flagged
    sub = kr.brute_force_knn(p, np.inf, flat[visited], 4)                                   # the 4 nearest of what was visited
    assert (got["dist2"].view(np.uint32) == sub["dist2"].view(np.uint32)).all()
    assert (got["primitive_id"] == visited[sub["primitive_id"]]).all()
    assert ctr[1] == 4 * 3 * (64 + 1)
    # a list that never fills (k = 32, ten visited triangles within the radius): the restarts meet every record again with
    # room left in the list, and still no id appears twice
    r2 = F(2.5 * 2.5)
    got, _, st = _knn(rt, leaves, nodes, 0, 2, _queries(p, r2), 32, status=True)
    assert st & rt.RT_KNN_STACK_OVERFLOW
    _assert_real_distinct_sorted(got, p, flat, "loose comb, k = 32")
    sub = kr.brute_force_knn(p, r2, flat[visited], 32)
    m = (sub["primitive_id"] != kr.MISS).sum(1)
    assert (m >= 5).all() and (m < 32).all()
    assert (got["dist2"].view(np.uint32) == sub["dist2"].view(np.uint32)).all()
    assert (np.where(sub["primitive_id"] != kr.MISS, visited[np.minimum(sub["primitive_id"], len(visited) - 1)], kr.MISS)
            == got["primitive_id"]).all()


def test_a_restart_after_an_overflow_gives_the_exact_row(rt):
    """the first pass overflows (the list fills only at the bottom of the comb, so all 80 leaves are pushed and 16 dropped) and
    misses triangle 70, the nearest; the restart starts from the first pass's list, prunes most leaves by their tight boxes,
    drops nothing, meets the listed triangles again and finds triangle 70: the exact row, each id once, status 0, one restart"""
    L = 80
    rng = np.random.default_rng(6)
    radius = {70: 1.0, L: 5.0}
    tris = _comb_triangles(rng, L, lambda k: radius.get(k, 12.0 + k % 7))
    leaves, nodes = _comb(rt, tris, tight_leaf_boxes=True)
    flat = tris.reshape(-1, 9)
    p = np.zeros((4, 3), F)
    p[1:] = rng.uniform(-0.05, 0.05, (3, 3))
    # the construction: after the first pass the bound is at most the 4th smallest d2 of the leaves it visited (the bottom leaf
    # and the 64 kept pushes); fewer than 64 tight leaf boxes lie within that bound, so the restart drops nothing
    visited = np.array(list(range(64)) + [L])
    bound = kr.brute_force_knn(p, np.inf, flat[visited], 4)["dist2"][:, 3]
    T = tris.reshape(-1, 3, 3)
    boxd = np.stack([pr.box_d2(p, T[k].min(0), T[k].max(0)) for k in range(L)], axis=1)
    assert ((boxd <= bound[:, None]).sum(1) < 60).all()
    got, ctr, st = _knn(rt, leaves, nodes, 0, 2, _queries(p), 4, counters=True, status=True)
    assert st == 0
    _assert_rows_equal(got, kr.brute_force_knn(p, np.inf, flat, 4), "comb with a restart")
    assert (got["primitive_id"][:, 0] == 70).all()
    _assert_real_distinct_sorted(got, p, flat, "comb with a restart")
    assert ctr[0] == 4 * 2 * (2 * L)      # two passes over the 80 two-slot nodes: one restart


# ------------------------------------------------------------------ 10: hipGraph
def test_build_and_queries_in_a_hip_graph(rt, scenes):
    import torch
    G, k = 40, 7
    tris = scenes.grid_mesh(G, 3)
    flat = np.ascontiguousarray(tris, F).reshape(-1, 9)
    inp = rt.BuildInput.allocate(tris)
    sets = _point_sets(flat, seed=9)
    pts = np.concatenate([sets["near"][:NP], sets["on_vertex_edge"][:NP]])
    q = rt.to_device(_queries(pts)).view(torch.float32).view(-1, 4)
    n = q.shape[0]
    out = torch.empty((n, k, 2), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        rt.RunBottomUpBuild(inp)
        rt.KNearest(inp.triangles_out, inp.nodes_out, 0, 2, q, k, out, counters=ctr, status=st)

    one_frame()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (out, ctr, st)]
    _assert_rows_equal(out.cpu().numpy().view(rt.KNN_HIT).reshape(-1, k), kr.brute_force_knn(pts, np.inf, flat, k), "eager")
    assert int(st[0]) == 0 and int(ctr[1]) >= n

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()                       # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(0)
        ctr.fill_(-1)
        st.fill_(-1)
        inp.nodes_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip((out, ctr, st), eager):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                               exp.view(torch.int32) if exp.dtype == torch.float32 else exp)


# ------------------------------------------------------------------ 11: counters
def test_counters_are_deterministic(rt, trees):
    tris = trees.tris("soup")
    sets = _sets(tris, "soup", sum(b"soup"))
    q = _queries(np.concatenate([sets["near"], sets["uniform"]]))
    q["dist2_max"][::5] = F(0.01)
    q["dist2_max"][3::50] = -1.0          # untraced
    traced = int(pr.traced(q["p"], q["dist2_max"]).sum())
    assert 0 < traced < len(q)
    for tree in ("pairs", "sah_pairs_splits"):
        g = trees.gpu("soup", tree)
        for k in (1, 8, 32):
            r1, c1, _ = _knn_tree(rt, g, q, k, counters=True)
            r2, c2, _ = _knn_tree(rt, g, q, k, counters=True)
            assert (c1 == c2).all() and (r1.view(np.uint32) == r2.view(np.uint32)).all()
            assert c1[0] > 0 and c1[1] >= traced and c1[2] == 0 and c1[3] == 0
