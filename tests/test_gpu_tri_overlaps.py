"""GPU tests of the triangle-overlap queries (rt_tri_overlaps_count / rt_tri_overlaps_collect) on every tree the builders make.

1. exactness: per query the sorted ids equal the numpy float32 brute force (tests/tri_overlap_ref.py), offsets equal the
   cumulative sum of its counts, no id appears twice -- six non-split tree kinds x five scenes x four query sets (proved
   non-empty on the CPU, tests/test_tri_overlap_ref_cpu.py) and SELF on every scene x six trees -- and so identical across tree
   kinds;
2. count / collect consistency: collect's counts equal the differences of offsets, both calls count the same tests, [2] = [3] =
   0, the sentinels behind offsets, ids and counts are intact;
3. edges: a query with a NaN or inf corner gives 0 and counts nothing; an empty tree; an empty batch still writes offsets[0]; a
   batch of 257 queries; a query that only touches a triangle in one vertex matches; a -0 / +0 shared corner is excluded in SELF
   mode;
4. truncation with fixed-K offsets: the flag, K distinct true matches per full segment, exact counts, neighbours intact;
5. refit (also of a split tree), then SELF: the result equals the brute force over the moved triangles;
6. split trees before refit: every id is a true match, count and collect agree;
7. a hand-built comb with 80 pending entries sets RT_TRI_STACK_OVERFLOW and returns a subset; deep fractal trees and wide
   collapsed trees are exact with status 0;
8. cross-check: on every non-split tree each row is a subset of the RT_RANGE_BOX row of the query's vertex box;
9. build + count + collect captured in one HIP graph replay the eager results."""
import numpy as np
import pytest

import edge_scenes
import range_sets as rs
import tri_overlap_ref as tr
import tri_overlap_sets as ts
from test_gpu_point_queries import _comb, _comb_triangles, _download, _move
from test_gpu_range_queries import EXACT_TREES, PAD, SENT, SPLIT_TREES, Result, Trees
from test_gpu_range_queries import _range as _box_range
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def trees(rt, scenes):
    return Trees(rt, scenes)


class Expected:
    """the brute force of every (scene, set) and of SELF, computed once per module"""
    def __init__(self, trees):
        self.trees, self._memo = trees, {}

    def sets(self, name):
        key = ("sets", name)
        if key not in self._memo:
            self._memo[key] = ts.query_sets(self.trees.tris(name), ts.seed_of(name))
        return self._memo[key]

    def of(self, name, kind):
        key = (name, kind)
        if key not in self._memo:
            tris = self.trees.tris(name)
            self._memo[key] = tr.brute_force(tris, tris, self_pairs=True) if kind == "self" else \
                tr.brute_force(self.sets(name)[kind], tris)
        return self._memo[key]


@pytest.fixture(scope="module")
def expected(trees):
    return Expected(trees)


# ------------------------------------------------------------------ helpers
def _count(rt, triangles, nodes, root, count, q, self_pairs):
    import torch
    n = len(q)
    qd = rt.to_device(np.ascontiguousarray(q, F)).view(torch.float32)
    off = torch.full((n + 1 + PAD,), SENT, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert rt.TriOverlapsCount(triangles, nodes, root, count, qd, off[:n + 1], self_pairs=self_pairs, counters=ctr,
                               status=st) == n
    torch.cuda.synchronize()
    o = off.cpu().numpy()
    assert (o[n + 1:] == SENT).all(), "TriOverlapsCount wrote past offsets[n]"
    return o[:n + 1], ctr.cpu().numpy().astype(np.uint64), rt.tri_overlap_status(st), (qd, off)


def _collect(rt, triangles, nodes, root, count, n, qd, off_dev, capacity, self_pairs):
    import torch
    ids = torch.full((capacity + PAD,), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    rt.TriOverlapsCollect(triangles, nodes, root, count, qd, off_dev[:n + 1], ids, self_pairs=self_pairs, counts=cnt[:n],
                          counters=ctr, status=st)
    torch.cuda.synchronize()
    i, c = ids.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert (i[capacity:] == SENT).all(), "TriOverlapsCollect wrote past the last segment"
    assert (c[n:] == SENT).all(), "TriOverlapsCollect wrote counts past num_queries"
    return i[:capacity], c[:n], ctr.cpu().numpy().astype(np.uint64), rt.tri_overlap_status(st)


def _overlaps_raw(rt, tri, nod, root, count, q, self_pairs=False):
    """count, then collect into exactly offsets[n] ids.  Asserts what must hold on ANY tree: count and collect agree (2)."""
    r = Result()
    r.offsets, r.ctr_count, r.st_count, (qd, off) = _count(rt, tri, nod, root, count, q, self_pairs)
    n = len(q)
    assert r.offsets[0] == 0 and (np.diff(r.offsets) >= 0).all()
    total = int(r.offsets[n])
    ids, r.counts, r.ctr_collect, r.st_collect = _collect(rt, tri, nod, root, count, n, qd, off, total, self_pairs)
    assert (r.counts.astype(np.int64) == np.diff(r.offsets)).all(), "collect's counts differ from the differences of offsets"
    assert (ids != SENT).all(), "a segment was not filled"
    assert (r.ctr_count == r.ctr_collect).all(), f"counters differ: count {r.ctr_count}, collect {r.ctr_collect}"
    assert r.ctr_count[2] == 0 and r.ctr_count[3] == 0
    assert r.st_count == r.st_collect and not (r.st_collect & rt.RT_TRI_TRUNCATED)
    r.lists = [ids[r.offsets[k]:r.offsets[k + 1]] for k in range(n)]
    return r


def _overlaps(rt, g, q, self_pairs=False):
    inp, root, count = g
    return _overlaps_raw(rt, inp.triangles_out, inp.nodes_out, root, count, q, self_pairs)


def _assert_exact(r, exp, what):
    lists, counts = exp
    assert (r.offsets == tr.offsets(counts)).all(), \
        f"{what}: offsets differ, first at query {np.nonzero(np.diff(r.offsets) != counts)[0][:5]}"
    for k, (got, e) in enumerate(zip(r.lists, lists)):
        s = np.sort(got)
        assert (s == e).all(), f"{what}: query {k}: got {s[:8]}... expected {e[:8]}..."     # (sorted and equal: no duplicates)


# ------------------------------------------------------------------ 1 + 2 + 8: exact on every non-split tree
@pytest.mark.parametrize("name", ts.SCENES)
def test_exact_against_brute_force_on_every_tree(rt, trees, expected, name):
    tris = trees.tris(name)
    for kind in ts.KINDS + ("self",):
        q = tris if kind == "self" else expected.sets(name)[kind]
        exp = expected.of(name, kind)
        if kind != "self":
            assert (exp[1] > 0).sum() * 4 >= ts.NQ and exp[1].sum() >= ts.NQ       # (the CPU test's guarantee, restated)
        lo, hi = tr.vertex_boxes(q)
        boxq = rs.box_queries(lo, hi)
        first = None
        for tree in EXACT_TREES:
            g = trees.gpu(name, tree)
            r = _overlaps(rt, g, q, self_pairs=kind == "self")
            print(f"{name}/{tree}/{kind}: ids {int(r.offsets[-1])}, box tests {int(r.ctr_count[0])}, "
                  f"leaf records {int(r.ctr_count[1])}")
            _assert_exact(r, exp, f"{name}/{tree}/{kind}")
            assert r.st_count == 0 and r.ctr_count[0] > 0 and r.ctr_count[1] > 0
            sorted_lists = [np.sort(x) for x in r.lists]
            if first is None:
                first = sorted_lists
                # 8: each row is a subset of the box query's row, and the two traversals examine the same slots and leaves
                b = _box_range(rt, g, boxq)
                assert all(np.isin(x, y).all() for x, y in zip(r.lists, b.lists)), f"{name}/{tree}/{kind}: not a subset"
                assert (b.ctr_count[:2] == r.ctr_count[:2]).all()
            assert all((a == b).all() for a, b in zip(first, sorted_lists))


@pytest.mark.parametrize("tree", EXACT_TREES)
def test_rows_are_subsets_of_the_box_query(rt, trees, expected, tree):
    """8 on every non-split tree (the test above checks it on the first tree of each scene)"""
    tris = trees.tris("soup")
    g = trees.gpu("soup", tree)
    for kind in ("moved", "degenerate"):
        q = expected.sets("soup")[kind]
        lo, hi = tr.vertex_boxes(q)
        r, b = _overlaps(rt, g, q), _box_range(rt, g, rs.box_queries(lo, hi))
        assert all(np.isin(x, y).all() for x, y in zip(r.lists, b.lists))
        assert (np.diff(b.offsets) >= np.diff(r.offsets)).all() and b.offsets[-1] > r.offsets[-1] > 0
        assert (b.ctr_count[:2] == r.ctr_count[:2]).all()


# ------------------------------------------------------------------ 3: edges
def test_untraced_empty_tree_and_batch_ends(rt, trees, expected):
    import torch
    tris = trees.tris("soup")
    g = trees.gpu("soup", "sah_pairs")
    inp, root, count = g
    q = expected.sets("soup")["moved"]
    # untraced: a NaN or an infinity in any of the nine components gives 0 and counts nothing
    bad = np.repeat(tris[:1], 9, axis=0).copy()
    for k in range(9):
        bad[k, k] = (np.nan, np.inf, -np.inf)[k % 3]
    assert tr.brute_force(tris[:1], tris)[1][0] >= 1
    for self_pairs in (False, True):
        r = _overlaps(rt, g, bad, self_pairs)
        assert (r.offsets == 0).all() and (r.ctr_count == 0).all() and (r.ctr_collect == 0).all()
    # ... and does not disturb its traced neighbours
    mixed = q[:70].copy()
    mixed[3, 4], mixed[64, 0] = np.nan, np.inf
    _assert_exact(_overlaps(rt, g, mixed), tr.brute_force(mixed, tris), "mixed")
    # a batch that ends inside a wave and inside a workgroup
    exp = expected.of("soup", "moved")
    for n in (1, 70, 257):
        _assert_exact(_overlaps(rt, g, q[:n]), ([x for x in exp[0][:n]], exp[1][:n]), f"batch of {n}")
    # an empty tree: every set is empty, nothing counted
    r = _overlaps_raw(rt, inp.triangles_out, inp.nodes_out, 0, 0, q[:300])
    assert (r.offsets == 0).all() and (r.ctr_count == 0).all()
    # an empty batch still writes offsets[0] = 0
    off = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    empty = torch.empty((0, 9), dtype=torch.float32, device="cuda")
    for self_pairs in (False, True):
        off.fill_(SENT)
        assert rt.TriOverlapsCount(inp.triangles_out, inp.nodes_out, root, count, empty, off[:1], self_pairs=self_pairs) == 0
        torch.cuda.synchronize()
        assert off.cpu().numpy().tolist() == [0, SENT, SENT, SENT]


def test_touching_in_one_vertex_and_signed_zero_corners(rt):
    """a query that only touches a triangle in one vertex matches (the comparisons are strict); in SELF mode a corner shared as
    -0 against +0 excludes the pair, and a pair that crosses without a shared corner is reported once, in the lower row"""
    A = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    B = [(0.2, 0.2, -1), (0.2, 0.2, 1), (0.9, 0.9, 1)]                 # pierces A, no shared corner
    C = [(-0.0, 0.0, -0.0), (0.5, 0.5, 1), (0.5, 0.5, -1)]             # pierces A, shares A's corner 0 up to the zero's sign
    far = [[(10 + k, 10, 10), (11 + k, 10, 10), (10 + k, 11, 10)] for k in range(5)]
    tris = np.array([A, B, C] + far, F).reshape(-1, 9)
    exp_self = tr.brute_force(tris, tris, self_pairs=True)
    assert [x.tolist() for x in exp_self[0][:3]] == [[1], [2], []]
    touch = np.array([[(1, 0, 0), (2, 0, 1), (2, 1, -1)],              # meets A in A's corner 1 only
                      [(0.25, 0.25, 0), (0.25, 0.25, 1), (1, 1, 1)],   # a corner in A's interior
                      [(1, 0, 0)] * 3,                                 # a point on A's corner
                      [(1, 0, np.nextafter(F(0), F(1)))] * 3], F).reshape(-1, 9)     # ... and one denormal above it
    exp_touch = tr.brute_force(touch, tris)
    assert [0 in x for x in exp_touch[0]] == [True, True, True, False]
    for tree in ("bottom_up", "pairs", "sah", "sah_pairs"):
        g = _gpu_tree(rt, tris, tree)
        _assert_exact(_overlaps(rt, g, tris, self_pairs=True), exp_self, f"self/{tree}")
        _assert_exact(_overlaps(rt, g, touch), exp_touch, f"touch/{tree}")
        _assert_exact(_overlaps(rt, g, tris), tr.brute_force(tris, tris), f"plain/{tree}")


def test_signed_zero_scene_self_pairs_on_pair_trees(rt, trees, expected):
    """the signed-zero mesh stores the same corner as -0 in one triangle and +0 in its neighbour: SELF must treat them as shared"""
    tris = trees.tris("signed_zero")
    T = tris.reshape(-1, 3, 3)
    lists, counts = expected.of("signed_zero", "self")
    plain = tr.brute_force(tris[:200], tris)
    # the exclusion matters here: without it the neighbours (shared corners, some through -0 == +0) are reported
    assert plain[1].sum() > counts[:200].sum() + 200
    zeros = (T == 0) & np.signbit(T)
    assert zeros.any()
    for tree in ("pairs", "hybrid_pairs", "sah_pairs"):
        _assert_exact(_overlaps(rt, trees.gpu("signed_zero", tree), tris, self_pairs=True), (lists, counts), f"signed zero/{tree}")


# ------------------------------------------------------------------ 4: truncation with fixed-K offsets
@pytest.mark.parametrize("self_pairs", (False, True))
def test_fixed_k_truncation(rt, trees, expected, self_pairs):
    import torch
    name, K = ("fractal", 1) if self_pairs else ("grid", 2)
    tris = trees.tris(name)
    g = trees.gpu(name, "pairs")
    inp, root, count = g
    q = tris if self_pairs else expected.sets(name)["moved"]
    lists, counts = expected.of(name, "self" if self_pairs else "moved")
    n = len(q)
    assert (counts > K).sum() > 20 and (counts <= K).sum() > 20                      # both sides of K occur
    qd = rt.to_device(np.ascontiguousarray(q, F)).view(torch.float32)
    off = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
    ids, cnt, _, st = _collect(rt, inp.triangles_out, inp.nodes_out, root, count, n, qd, off, n * K, self_pairs)
    assert st == rt.RT_TRI_TRUNCATED
    assert (cnt.astype(np.int64) == counts).all(), "counts must be exact beyond the room"
    seg = ids.reshape(n, K)
    for k in range(n):
        m = min(int(counts[k]), K)
        assert np.isin(seg[k, :m], lists[k]).all() and len(set(seg[k, :m].tolist())) == m, f"query {k}"
        assert (seg[k, m:] == SENT).all(), f"query {k} wrote past its matches"
    # the truncated segments are the head of the untruncated traversal order
    full = _overlaps(rt, g, q, self_pairs)
    assert all((seg[k, :min(int(counts[k]), K)] == full.lists[k][:K]).all() for k in range(n))
    # room everywhere: no flag
    off = (torch.arange(n + 1, dtype=torch.int64) * int(counts.max())).cuda()
    _, _, _, st = _collect(rt, inp.triangles_out, inp.nodes_out, root, count, n, qd, off, n * int(counts.max()), self_pairs)
    assert st == 0


# ------------------------------------------------------------------ 5: refit, then SELF
def _crumple(tris, t):
    """_move's smooth deformation, then the sheet folded over itself along a line near its middle (x -> |x - c|): the two halves
    lie on top of each other, 0.6 apart in x, and their random heights make them cut each other all over.  Applied per vertex, so
    shared vertices stay shared (pairs stay pairs)."""
    v = _move(tris, t).reshape(-1, 3).astype(np.float64)
    c = 0.5 * (v[:, 0].min() + v[:, 0].max()) + 0.3
    v[:, 0] = np.abs(v[:, 0] - c)
    return np.ascontiguousarray(v.astype(F).reshape(-1, 9))


@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs", "sah_splits"))
def test_refit_then_self(rt, scenes, tree):
    import torch
    tris = rs.scene_tris("grid", scenes)
    inp, root, count = _gpu_tree(rt, tris, tree)
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    for step in (1.0, 2.5):
        moved = _crumple(tris, step)
        inp.triangles_in.copy_(rt.to_device(moved))
        rt.Refit(inp, root, count, plan)
        torch.cuda.synchronize()
        assert rt.refit_status(plan, inp.num_triangles) == 0
        exp = tr.brute_force(moved, moved, self_pairs=True)
        assert exp[1].sum() >= 64, "the deformation must make the sheet cut itself"
        r = _overlaps(rt, (inp, root, count), moved, self_pairs=True)
        assert r.st_count == 0
        if "splits" in tree:
            # refit writes unclipped boxes, so every match is reached -- through each of its references: as sets
            assert all(np.array_equal(np.unique(got), e) for got, e in zip(r.lists, exp[0])), f"refit {tree}"
        else:
            _assert_exact(r, exp, f"refit {tree}")


# ------------------------------------------------------------------ 6: split trees before refit
@pytest.mark.parametrize("name", ("grid", "soup", "cornell", "signed_zero"))
def test_split_trees_report_true_matches(rt, trees, expected, name):
    tris = trees.tris(name)
    for kind in ts.KINDS + ("self",):
        q = tris if kind == "self" else expected.sets(name)[kind]
        lists, counts = expected.of(name, kind)
        for tree in SPLIT_TREES:
            r = _overlaps(rt, trees.gpu(name, tree), q, self_pairs=kind == "self")     # (count and collect agree: asserted inside)
            assert r.st_count == 0
            assert all(np.isin(got, e).all() for got, e in zip(r.lists, lists)), f"{name}/{tree}/{kind}: a false match"
            assert r.offsets[-1] > 0 or counts.sum() == 0


# ------------------------------------------------------------------ 7: deep and wide trees, stack overflow
def test_deep_and_wide_trees_are_exact(rt, trees, expected):
    for kind in ("small", "self"):
        q = trees.tris("fractal") if kind == "self" else expected.sets("fractal")[kind]
        for tree in ("bottom_up", "sah", "hybrid"):
            r = _overlaps(rt, trees.gpu("fractal", tree), q, self_pairs=kind == "self")
            assert r.st_count == 0
            _assert_exact(r, expected.of("fractal", kind), f"fractal/{tree}/{kind}")
    tris = trees.tris("grid")
    inp, root, count = trees.gpu("grid", "bottom_up")
    nodes, _ = _download(rt, inp, tris.shape[0])
    for width in (3, 4, 7):
        wn, wr, wc = edge_scenes.collapse_wide(nodes, root, count, width, rt.NODE)
        wd = rt.to_device(wn)
        for kind in ("moved", "coincident"):
            r = _overlaps_raw(rt, inp.triangles_out, wd, wr, wc, expected.sets("grid")[kind])
            assert r.st_count == 0
            _assert_exact(r, expected.of("grid", kind), f"width {width}/{kind}")


def test_stack_overflow_is_flagged_and_the_result_is_a_subset(rt):
    """a comb of 80 two-slot nodes whose boxes all contain the query's box: every node pushes its leaf and descends, so 80
    entries are pending before the first pop; the 16 pushes beyond 64 are dropped, flagged, and missing from the result.  Every
    comb triangle is made to cross the query triangle (a long sliver through the origin's neighbourhood)."""
    L = 80
    rng = np.random.default_rng(5)
    tris = _comb_triangles(rng, L, lambda k: 2.0 + k % 7)
    # stretch every comb triangle through the plane z = 0 inside the query: corners (x, y, +-5) around a point near the origin
    for k in range(L + 1):
        c = rng.uniform(-0.2, 0.2, 2)
        tris[k] = [(c[0], c[1], -5.0 - k % 3), (c[0] + 0.05, c[1], 5.0 + k % 5), (c[0], c[1] + 0.05, 5.0)]
    leaves, nodes = _comb(rt, tris, tight_leaf_boxes=False)
    q = np.array([[(-1, -1, 0.01 * j), (2, -1, 0.01 * j), (-1, 2, 0.01 * j)] for j in range(4)], F).reshape(-1, 9)
    lists, counts = tr.brute_force(q, tris.reshape(-1, 9))
    assert (counts == L + 1).all()                      # the truth: every triangle
    r = _overlaps_raw(rt, leaves, nodes, 0, 2, q)
    assert r.st_count & rt.RT_TRI_STACK_OVERFLOW and r.st_collect & rt.RT_TRI_STACK_OVERFLOW
    for k in range(4):
        got = np.sort(r.lists[k])
        assert np.isin(got, lists[k]).all() and len(np.unique(got)) == len(got)
        assert (got == np.concatenate([np.arange(64), [L]])).all()     # the 64 kept pushes and the bottom leaf
    assert r.ctr_count[1] == 4 * 65 and r.ctr_count[0] == 4 * 2 * L


# ------------------------------------------------------------------ 9: hipGraph
def test_build_count_and_collect_in_a_hip_graph(rt, scenes):
    import torch
    tris = _crumple(np.ascontiguousarray(scenes.grid_mesh(40, 3), F).reshape(-1, 9), 1.0)
    inp = rt.BuildInput.allocate(tris)
    n = tris.shape[0]
    moved = ts.query_sets(tris, 9)["moved"]
    K = 64
    work = []
    for q, self_pairs in ((moved, False), (tris, True)):
        m = len(q)
        work.append(dict(q=q, self_pairs=self_pairs, qd=rt.to_device(q).view(torch.float32),
                         off=torch.empty(m + 1, dtype=torch.int64, device="cuda"),
                         fixed=(torch.arange(m + 1, dtype=torch.int64) * K).cuda(),
                         ids=torch.empty(m * K, dtype=torch.int32, device="cuda"),
                         cnt=torch.empty(m, dtype=torch.int32, device="cuda"),
                         scratch=rt.device_bytes(rt.TriOverlapsScratchBytes(m))))
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        rt.RunBottomUpBuild(inp)
        for w in work:
            w["ids"].fill_(-1)
            rt.TriOverlapsCount(inp.triangles_out, inp.nodes_out, 0, 2, w["qd"], w["off"], self_pairs=w["self_pairs"],
                                scratch=w["scratch"], counters=ctr, status=st)
            rt.TriOverlapsCollect(inp.triangles_out, inp.nodes_out, 0, 2, w["qd"], w["fixed"], w["ids"],
                                  self_pairs=w["self_pairs"], counts=w["cnt"], counters=ctr, status=st)

    def outputs():
        return [t for w in work for t in (w["off"], w["ids"], w["cnt"])] + [ctr, st]

    one_frame()
    torch.cuda.synchronize()
    eager = [t.clone() for t in outputs()]
    for w in work:                       # the eager frame is right: offsets and the per-query sets (K holds every set here)
        lists, counts = tr.brute_force(w["q"], tris, self_pairs=w["self_pairs"])
        assert counts.max() <= K and counts.sum() >= 64
        assert (w["off"].cpu().numpy() == tr.offsets(counts)).all() and (w["cnt"].cpu().numpy() == counts).all()
        seg = w["ids"].cpu().numpy().view(np.uint32).reshape(-1, K)
        assert all((np.sort(seg[k, :counts[k]]) == lists[k]).all() for k in range(len(lists)))
    assert int(st.item()) == 0

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
        for t in outputs():
            t.fill_(-7)
        inp.nodes_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip(outputs(), eager):
            assert torch.equal(got, exp)


def test_tri_overlaps_convenience(rt, trees, expected):
    import torch
    tris = trees.tris("cornell")
    inp, root, count = trees.gpu("cornell", "sah")
    for kind in ("moved", "self"):
        q = tris if kind == "self" else expected.sets("cornell")[kind]
        lists, counts = expected.of("cornell", kind)
        off, ids = rt.TriOverlaps(inp.triangles_out, inp.nodes_out, root, count, rt.to_device(q).view(torch.float32),
                                  self_pairs=kind == "self")
        assert off.dtype == torch.int64 and ids.dtype == torch.int32 and ids.numel() == counts.sum()
        o, i = off.cpu().numpy(), ids.cpu().numpy().view(np.uint32)
        assert (o == tr.offsets(counts)).all()
        assert all((np.sort(i[o[k]:o[k + 1]]) == lists[k]).all() for k in range(len(lists)))
