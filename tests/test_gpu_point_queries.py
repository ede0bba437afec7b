"""GPU tests of the closest-point queries (rt_closest_points) on every tree the builders make.

1. bit-exact against the numpy brute force over the caller's triangles (tests/point_ref.py) on the six non-split tree kinds
   of five scenes, for near-surface, uniform, on-vertex / on-edge and far points -- and so identical across tree kinds;
   accuracy against float64 on every scene but the fractal (whose 2^43 coordinates overflow Ericson's products);
2. the precondition of exactness, checked on the downloaded Node[]: every reachable slot box contains the vertex boxes of the
   triangles below it;
3. split trees: dist2 is d2(p, tri[id]) bit for bit and within the documented bound of the brute-force minimum;
4. refit (also of a split tree): queries on the refitted tree equal the brute force over the moved triangles bit for bit;
5. the radius: just below the minimum misses, exactly at it hits; untraced queries miss and count nothing; records past
   num_queries are not written;
6. the deep fractal trees and wide collapsed trees: exact with status 0;
7. hand-built trees with more than 64 pending entries: when the restarts from the best so far cannot avoid the overflow,
   RT_POINT_STACK_OVERFLOW is set and the record is still a real (d2, id); when a restart drops nothing, the record is exact
   and the status 0;
8. build + queries + counters captured in one HIP graph replay the eager records and counters."""
import numpy as np
import pytest

import edge_scenes
import point_ref as pr
from test_gpu_ray_queries import _gpu_tree, _scene

pytestmark = pytest.mark.gpu

EXACT_TREES = ("bottom_up", "pairs", "hybrid", "hybrid_pairs", "sah", "sah_pairs")
SPLIT_TREES = ("sah_splits", "sah_pairs_splits")
SCENES = ("grid", "soup", "cornell", "signed_zero", "fractal")
F = np.float32
MASK = 0x1FFFFFFF
NQ = 1024                 # points per query set


# ------------------------------------------------------------------ helpers
class Trees:
    def __init__(self, rt, scenes):
        self.rt, self.scenes = rt, scenes
        self._sc, self._g = {}, {}

    def tris(self, name):
        if name not in self._sc:
            self._sc[name] = np.ascontiguousarray(_scene(name, self.scenes)[0], F).reshape(-1, 9)
        return self._sc[name]

    def gpu(self, name, tree):
        if (name, tree) not in self._g:
            self._g[name, tree] = _gpu_tree(self.rt, self.tris(name), tree)
        return self._g[name, tree]


@pytest.fixture(scope="module")
def trees(rt, scenes):
    return Trees(rt, scenes)


def _closest(rt, triangles, nodes, root, count, queries, counters=False, status=False, n_alloc=None):
    """queries: POINT_QUERY numpy array -> (POINT_HIT array, counters uint64[4] or None, status or None)"""
    import torch
    q = rt.to_device(np.ascontiguousarray(queries, rt.POINT_QUERY)).view(torch.float32).view(-1, 4)
    n = q.shape[0]
    hits = torch.full((n_alloc or n, 4), 7.0, dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda") if counters else None
    st = torch.zeros(1, dtype=torch.int32, device="cuda") if status else None
    rt.ClosestPoints(triangles, nodes, root, count, q, hits[:n], counters=ctr, status=st)
    torch.cuda.synchronize()
    out = hits.cpu().numpy().view(rt.POINT_HIT).reshape(-1)
    return (out, ctr.cpu().numpy().astype(np.uint64) if counters else None,
            rt.point_status(st) if status else None)


def _query_tree(rt, g, queries, **kw):
    inp, root, count = g
    return _closest(rt, inp.triangles_out, inp.nodes_out, root, count, queries, **kw)


def _queries(points, dist2_max=np.inf):
    q = np.zeros(len(points), dtype=[("p", "<f4", 3), ("dist2_max", "<f4")])
    q["p"] = points
    q["dist2_max"] = dist2_max
    return q


def _point_sets(tris, seed):
    """near-surface, uniform in the 1.5x box, exactly on vertices and edge midpoints, far away"""
    rng = np.random.default_rng(seed)
    T = tris.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
    ext = float((hi - lo).max())
    k = rng.integers(0, len(T), NQ)
    b = rng.dirichlet((1, 1, 1), NQ)
    on = (b[:, :, None] * T[k]).sum(1)
    nrm = np.cross(T[k, 1] - T[k, 0], T[k, 2] - T[k, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    near = on + nrm * rng.uniform(-0.01, 0.01, (NQ, 1)) * ext
    c, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    uniform = c + rng.uniform(-1, 1, (NQ, 3)) * half
    verts = T[k, rng.integers(0, 3, NQ)]
    j = rng.integers(0, 3, NQ)
    mids = (T[k, j] + T[k, (j + 1) % 3]) * 0.5
    exact = np.where(rng.random((NQ, 1)) < 0.5, verts, mids)
    d = rng.normal(size=(NQ, 3))
    far = c + d / np.linalg.norm(d, axis=1, keepdims=True) * ext * rng.uniform(3, 30, (NQ, 1))
    return {name: np.ascontiguousarray(p, F) for name, p in
            (("near", near), ("uniform", uniform), ("on_vertex_edge", exact), ("far", far))}


def _expected(points, dist2_max, tris):
    d, i, u, v = pr.brute_force(points, dist2_max, tris)
    e = np.zeros(len(d), dtype=[("dist2", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])
    e["dist2"], e["primitive_id"], e["u"], e["v"] = d, i, u, v
    return e


def _assert_records_equal(got, exp, what):
    g, e = got.view(np.uint32).reshape(-1, 4), exp.view(np.uint32).reshape(-1, 4)
    bad = np.nonzero((g != e).any(1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} records differ, first at {bad[:5]}: got {got[bad[:3]]} "
                           f"expected {exp[bad[:3]]}")


def _reachable_boxes_contain(rt, nodes, leaves, root, count, tris):
    """every reachable slot box contains the vertex boxes of the caller's triangles below it (iterative post-order)"""
    T = tris.reshape(-1, 3, 3)
    tlo, thi = T.min(1), T.max(1)
    bad = []

    def leaf_box(li):
        rec = leaves[li]
        ids = [int(rec["primitive_id_0"])]
        if int(rec["primitive_id_1"]) == ids[0] + 1:
            ids.append(ids[0] + 1)
        return tlo[ids].min(0), thi[ids].max(0)

    def run_box(first, cnt, memo):
        lo, hi = np.full(3, np.inf, F), np.full(3, -np.inf, F)
        for s in range(first, first + cnt):
            if s in memo:
                slo, shi = memo[s]
                lo, hi = np.minimum(lo, slo), np.maximum(hi, shi)
        return lo, hi

    memo = {}
    stack = [(root, count, False)]
    while stack:
        first, cnt, done = stack.pop()
        if not done:
            stack.append((first, cnt, True))
            for s in range(first, first + cnt):
                typ = int(nodes["w28"][s]) >> 29
                if typ == 1:
                    stack.append((int(nodes["w28"][s]) & MASK, int(nodes["w12"][s]) >> 29, False))
            continue
        for s in range(first, first + cnt):
            typ = int(nodes["w28"][s]) >> 29
            if typ == 0:
                continue
            if typ == 2:
                lo, hi = leaf_box(int(nodes["w28"][s]) & MASK)
            else:
                lo, hi = run_box(int(nodes["w28"][s]) & MASK, int(nodes["w12"][s]) >> 29, memo)
            memo[s] = (lo, hi)
            if not ((nodes["min"][s] <= lo).all() and (nodes["max"][s] >= hi).all()):
                bad.append(s)
    return bad


def _download(rt, inp, n):
    nodes = rt.to_host(inp.nodes_out, rt.NODE, rt.NodesBytes(n) // 32)
    leaves = rt.to_host(inp.triangles_out, rt.TRIANGLE_PAIR, n)
    return nodes, leaves


# ------------------------------------------------------------------ 1 + 2: exact on every non-split tree
@pytest.mark.parametrize("name", SCENES)
def test_exact_against_brute_force_on_every_tree(rt, trees, name):
    tris = trees.tris(name)
    sets = _point_sets(tris, seed=sum(name.encode()))
    exp = {k: _expected(p, np.inf, tris) for k, p in sets.items()}
    for tree in EXACT_TREES:
        g = trees.gpu(name, tree)
        nodes, leaves = _download(rt, g[0], tris.shape[0])
        bad = _reachable_boxes_contain(rt, nodes, leaves, g[1], g[2], tris)
        assert not bad, f"{name}/{tree}: slot boxes {bad[:5]} do not contain the vertex boxes below them"
        for k, p in sets.items():
            got, ctr, st = _query_tree(rt, g, _queries(p), counters=True, status=True)
            _assert_records_equal(got, exp[k], f"{name}/{tree}/{k}")
            assert st == 0 and ctr[0] > 0 and ctr[1] >= len(p) and ctr[2] == 0 and ctr[3] == 0
    if name != "fractal":
        T = tris.reshape(-1, 3, 3)
        M = float(np.abs(T).max())
        for k, p in sets.items():
            d64 = pr.brute_force_f64(p, tris)
            Mk = max(M, float(np.abs(p).max()))
            err = np.abs(np.sqrt(exp[k]["dist2"].astype(np.float64)) - d64) / (Mk * 2.0 ** -23)
            assert err.max() <= 16, f"{name}/{k}: {err.max():.1f} ulps of the largest coordinate against float64"


# ------------------------------------------------------------------ 3: split trees
@pytest.mark.parametrize("name", ("grid", "soup", "cornell", "signed_zero"))
def test_split_trees_are_real_and_within_the_bound(rt, trees, name):
    tris = trees.tris(name)
    T = tris.reshape(-1, 3, 3)
    sets = _point_sets(tris, seed=7 + len(name))
    for tree in SPLIT_TREES:
        g = trees.gpu(name, tree)
        for k, p in sets.items():
            got, _, st = _query_tree(rt, g, _queries(p), status=True)
            assert st == 0
            ids = got["primitive_id"]
            assert (ids < T.shape[0]).all(), f"{name}/{tree}/{k}: a miss with an infinite radius"
            d, u, v = pr.d2(p, T[ids, 0], T[ids, 1], T[ids, 2])
            assert (got["dist2"].view(np.uint32) == d.view(np.uint32)).all()
            assert (got["u"].view(np.uint32) == u.view(np.uint32)).all() and (got["v"].view(np.uint32) == v.view(np.uint32)).all()
            bf = _expected(p, np.inf, tris)
            assert (got["dist2"] >= bf["dist2"]).all()
            M = max(float(np.abs(T).max()), float(np.abs(p).max()))
            excess = np.sqrt(got["dist2"].astype(np.float64)) - np.sqrt(bf["dist2"].astype(np.float64))
            assert excess.max() <= 2.0 ** -20 * M, f"{name}/{tree}/{k}: {excess.max()} beyond 2^-20 * {M}"


# ------------------------------------------------------------------ 4: refit
def _move(tris, t):
    """a smooth deformation applied per vertex: shared vertices stay shared (pairs stay pairs)"""
    v = tris.reshape(-1, 3).astype(np.float64)
    out = v.copy()
    out[:, 1] += 0.3 * np.sin(0.7 * v[:, 0] + t) * np.cos(0.5 * v[:, 2])
    out[:, 0] += 0.1 * np.cos(0.3 * v[:, 2] + t)
    return np.ascontiguousarray(out.astype(F).reshape(-1, 9))


@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs", "sah_splits"))
def test_refit_then_query_is_exact(rt, scenes, tree):
    import torch
    tris = _scene("grid", scenes)[0]
    inp, root, count = _gpu_tree(rt, np.ascontiguousarray(tris, F), tree)
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    for step in (1.0, 2.5):
        moved = _move(tris, step)
        inp.triangles_in.copy_(rt.to_device(moved))
        rt.Refit(inp, root, count, plan)
        torch.cuda.synchronize()
        assert rt.refit_status(plan, inp.num_triangles) == 0
        nodes, leaves = _download(rt, inp, moved.shape[0])
        assert not _reachable_boxes_contain(rt, nodes, leaves, root, count, moved)
        for k, p in _point_sets(moved, seed=int(step * 10)).items():
            got, _, st = _query_tree(rt, (inp, root, count), _queries(p), status=True)
            assert st == 0
            _assert_records_equal(got, _expected(p, np.inf, moved), f"refit {tree}/{k}")


# ------------------------------------------------------------------ 5: radius, untraced queries, bounds of the batch
def test_radius_untraced_and_batch_end(rt, trees):
    tris = trees.tris("soup")
    g = trees.gpu("soup", "sah_pairs")
    p = _point_sets(tris, seed=3)["uniform"][:500]
    exact = _expected(p, np.inf, tris)
    assert (exact["dist2"] > 0).sum() > 400
    pos = exact["dist2"] > 0
    # exactly at the minimum: a hit with the same record; one float below: a miss
    got, _, _ = _query_tree(rt, g, _queries(p, exact["dist2"]))
    _assert_records_equal(got, exact, "radius = minimum")
    below = np.where(pos, np.nextafter(exact["dist2"], F(0)), exact["dist2"])
    got, _, _ = _query_tree(rt, g, _queries(p, below))
    assert (got["primitive_id"][pos] == pr.MISS).all() and np.isinf(got["dist2"][pos]).all()
    assert (got["u"][pos] == 0).all() and (got["v"][pos] == 0).all()
    _assert_records_equal(got, _expected(p, below, tris), "radius below the minimum")
    # untraced: non-finite p, NaN or negative radius -> {+inf, MISS, 0, 0} and no tests counted
    bad = _queries(p[:8])
    bad["p"][0, 0], bad["p"][1, 1], bad["p"][2, 2] = np.nan, np.inf, -np.inf
    bad["dist2_max"][3], bad["dist2_max"][4], bad["dist2_max"][5] = np.nan, -1.0, -np.inf
    bad = bad[:6]
    got, ctr, _ = _query_tree(rt, g, bad, counters=True)
    assert (got["primitive_id"] == pr.MISS).all() and np.isinf(got["dist2"]).all()
    assert (got["u"] == 0).all() and (got["v"] == 0).all() and (ctr == 0).all()
    # records past num_queries are not written
    got, _, _ = _query_tree(rt, g, _queries(p[:70]), n_alloc=200)
    assert (got[70:].view(np.float32).reshape(-1, 4) == 7.0).all()
    _assert_records_equal(got[:70], exact[:70], "batch of 70")
    # an empty tree: every query misses, nothing counted
    inp = g[0]
    got, ctr, _ = _closest(rt, inp.triangles_out, inp.nodes_out, 0, 0, _queries(p[:10]), counters=True)
    assert (got["primitive_id"] == pr.MISS).all() and (ctr == 0).all()


# ------------------------------------------------------------------ 6: deep and wide trees
def test_deep_and_wide_trees_are_exact(rt, trees):
    tris = trees.tris("fractal")
    p = _point_sets(tris, seed=21)["near"]
    exp = _expected(p, np.inf, tris)
    for tree in ("bottom_up", "sah", "hybrid"):
        got, _, st = _query_tree(rt, trees.gpu("fractal", tree), _queries(p), status=True)
        assert st == 0
        _assert_records_equal(got, exp, f"fractal/{tree}")
    tris = trees.tris("grid")
    inp, root, count = trees.gpu("grid", "bottom_up")
    nodes, leaves = _download(rt, inp, tris.shape[0])
    sets = _point_sets(tris, seed=22)
    for width in (3, 4, 7):
        wn, wr, wc = edge_scenes.collapse_wide(nodes, root, count, width, rt.NODE)
        wd = rt.to_device(wn)
        for k in ("near", "uniform"):
            got, _, st = _closest(rt, inp.triangles_out, wd, wr, wc, _queries(sets[k]), status=True)
            assert st == 0
            _assert_records_equal(got, _expected(sets[k], np.inf, tris), f"width {width}/{k}")


# ------------------------------------------------------------------ 7: stack overflow
def _comb(rt, tris, tight_leaf_boxes):
    """a comb over len(tris) - 1 levels: node k = (box child k+1, leaf k) in slots (2k, 2k+1), the last node = (leaf L, leaf
    L-1).  Box slots span [-50, 50]^3 (around every query point: boxdist2 0, so the box child is always the nearest and the
    leaf is pushed).  Leaf slots span the same box, or with tight_leaf_boxes their triangle's vertex box."""
    L = len(tris) - 1
    nodes = np.zeros(2 * L, rt.NODE)
    for k in range(L):
        last = k == L - 1
        for s in (2 * k, 2 * k + 1):
            nodes["min"][s], nodes["max"][s] = (-50, -50, -50), (50, 50, 50)
        if tight_leaf_boxes:
            nodes["min"][2 * k + 1], nodes["max"][2 * k + 1] = tris[k].min(0), tris[k].max(0)
        # w12 = parent : 29 | count : 3 -- the count is the child run's length (read for box slots); parents are not read
        nodes["w12"][2 * k] = 1 << 29 if last else 2 << 29
        nodes["w28"][2 * k] = (2 << 29) | L if last else (1 << 29) | (2 * (k + 1))
        nodes["w12"][2 * k + 1] = 1 << 29
        nodes["w28"][2 * k + 1] = (2 << 29) | k
    leaves = np.zeros(L + 1, rt.TRIANGLE_PAIR)
    for k in range(L + 1):
        leaves["v0"][k], leaves["v1"][k], leaves["v2"][k], leaves["v3"][k] = tris[k, 0], tris[k, 1], tris[k, 2], tris[k, 2]
        leaves["primitive_id_0"][k] = k
    return rt.to_device(leaves), rt.to_device(nodes)


def _comb_triangles(rng, L, radius):
    tris = np.zeros((L + 1, 3, 3), F)
    for k in range(L + 1):
        c = rng.normal(size=3)
        tris[k] = c / np.linalg.norm(c) * radius(k) + rng.uniform(-0.1, 0.1, (3, 3))
    return tris


def test_stack_overflow_is_flagged_and_the_record_is_real(rt):
    """80 pending leaves on every pass (every box around the query point); the nearest triangle is among the dropped pushes,
    so the first pass and both restarts miss it: the flag is set and the record is still a real (d2, id)"""
    L = 80
    rng = np.random.default_rng(5)
    tris = _comb_triangles(rng, L, lambda k: 2.0 + k % 7 if k != 70 else 1.0)   # triangle 70 (pushed at depth 71): nearest
    leaves, nodes = _comb(rt, tris, tight_leaf_boxes=False)
    p = np.zeros((4, 3), F)
    p[1:] = rng.uniform(-0.05, 0.05, (3, 3))
    got, ctr, st = _closest(rt, leaves, nodes, 0, 2, _queries(p), counters=True, status=True)
    assert st & rt.RT_POINT_STACK_OVERFLOW
    ids = got["primitive_id"]
    assert (ids <= L).all()
    T = tris.reshape(-1, 3, 3)
    d, u, v = pr.d2(p, T[ids, 0], T[ids, 1], T[ids, 2])
    assert (got["dist2"].view(np.uint32) == d.view(np.uint32)).all()
    bf = _expected(p, np.inf, tris.reshape(-1, 9))
    assert (bf["primitive_id"] == 70).all() and (ids != 70).all()    # the nearest was dropped, and that is flagged
    assert ctr[1] == 4 * 3 * (64 + 1)     # per query and pass (the first and two restarts): the bottom leaf and 64 kept pushes


def test_a_restart_after_an_overflow_gives_the_exact_record(rt):
    """the first pass overflows (before the first leaf the best is +inf, so all 80 leaves are pushed) and misses the nearest
    triangle 70; the restart starts from the best of the first pass, prunes every other leaf by its tight box, drops nothing
    and finds triangle 70: exact record, status 0, exactly one restart"""
    L = 80
    rng = np.random.default_rng(6)
    radius = {70: 1.0, L: 5.0}
    tris = _comb_triangles(rng, L, lambda k: radius.get(k, 12.0 + k % 7))
    leaves, nodes = _comb(rt, tris, tight_leaf_boxes=True)
    p = np.zeros((4, 3), F)
    p[1:] = rng.uniform(-0.05, 0.05, (3, 3))
    # the construction: every far leaf's box is farther than the bottom leaf L, which the first pass finds
    T = tris.reshape(-1, 3, 3)
    far = [k for k in range(L) if k != 70]
    dL, _, _ = pr.d2(p, T[L, 0], T[L, 1], T[L, 2])
    bmin = np.min([pr.box_d2(p, T[k].min(0), T[k].max(0)) for k in far], axis=0)
    assert (bmin > dL).all()
    got, ctr, st = _closest(rt, leaves, nodes, 0, 2, _queries(p), counters=True, status=True)
    assert st == 0
    _assert_records_equal(got, _expected(p, np.inf, tris.reshape(-1, 9)), "comb with a restart")
    assert (got["primitive_id"] == 70).all()
    assert ctr[0] == 4 * 2 * (2 * L)      # two passes over the 80 two-slot nodes: one restart
    assert ctr[1] == 4 * (1 + 2)          # first pass: leaf L; restart: leaf L, then leaf 70


# ------------------------------------------------------------------ 8: hipGraph
def test_build_and_queries_in_a_hip_graph(rt, scenes):
    import torch
    G = 40
    tris = scenes.grid_mesh(G, 3)
    inp = rt.BuildInput.allocate(tris)
    p = _point_sets(np.ascontiguousarray(tris, F).reshape(-1, 9), seed=9)
    q = rt.to_device(_queries(np.concatenate([p["near"], p["uniform"]]))).view(torch.float32).view(-1, 4)
    n = q.shape[0]
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        rt.RunBottomUpBuild(inp)
        rt.ClosestPoints(inp.triangles_out, inp.nodes_out, 0, 2, q, hits, counters=ctr, status=st)

    one_frame()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (hits, ctr, st)]
    assert int((hits.view(torch.int32)[:, 1] != -1).sum()) == n
    _assert_records_equal(hits.cpu().numpy().view(rt.POINT_HIT).reshape(-1),
                          _expected(q.cpu().numpy().view(rt.POINT_QUERY).reshape(-1)["p"], np.inf,
                                    np.ascontiguousarray(tris, F).reshape(-1, 9)), "eager")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()                       # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        hits.fill_(0)
        ctr.fill_(-1)
        st.fill_(-1)
        inp.nodes_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip((hits, ctr, st), eager):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                               exp.view(torch.int32) if exp.dtype == torch.float32 else exp)
