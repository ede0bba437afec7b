"""GPU tests of the range queries (rt_range_count / rt_range_collect) on every tree the builders make.

1. exactness: per query the sorted ids equal the numpy brute force (tests/range_ref.py), offsets equal the cumulative sum of
   its counts, no id appears twice -- six non-split tree kinds x five scenes x both shapes x three query sets (proved
   non-empty on the CPU, tests/test_range_ref_cpu.py) -- and so identical across tree kinds;
2. count / collect consistency: collect's counts equal the differences of offsets, both calls count the same tests, ids past
   each segment and records past num_queries are not written (sentinels);
3. edges: a radius exactly at a triangle's d2 accepts it and the next float below rejects it; a box face exactly on a vertex
   coordinate accepts, -0 against +0 included; untraced queries give 0 and count nothing; a +inf radius returns every triangle;
   an empty tree; an empty batch still writes offsets[0];
4. truncation with fixed-K offsets: the flag, K distinct true matches per full segment, exact counts, neighbours intact;
5. refit (also of a split tree): the sets equal the brute force over the moved triangles;
6. split trees before refit: every id is a true match, count and collect agree;
7. deep fractal trees and wide collapsed trees: exact with status 0; a hand-built comb with 80 pending entries sets
   RT_RANGE_STACK_OVERFLOW and returns a subset;
8. cross-check: ClosestPoints hits iff the sphere count is > 0 and its id is a member;
9. build + count + collect captured in one HIP graph replay the eager results;
10. the shared 64-bit scan (csr_scan.hip) past one chunk of 1024 workgroups and past its lowest 21-bit limb."""
import numpy as np
import pytest

import edge_scenes
import point_ref as pr
import range_ref as rr
import range_sets as rs
from test_gpu_point_queries import _closest, _comb, _comb_triangles, _download, _move, _queries
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

EXACT_TREES = ("bottom_up", "pairs", "hybrid", "hybrid_pairs", "sah", "sah_pairs")
SPLIT_TREES = ("sah_splits", "sah_pairs_splits")
F = np.float32
SENT = 0x5EA7BEEF        # sentinel word of every output buffer
PAD = 64                 # sentinel words behind every output buffer


# ------------------------------------------------------------------ helpers
class Trees:
    def __init__(self, rt, scenes):
        self.rt, self.scenes = rt, scenes
        self._sc, self._g = {}, {}

    def tris(self, name):
        if name not in self._sc:
            self._sc[name] = rs.scene_tris(name, self.scenes)
        return self._sc[name]

    def gpu(self, name, tree):
        if (name, tree) not in self._g:
            self._g[name, tree] = _gpu_tree(self.rt, self.tris(name), tree)
        return self._g[name, tree]


@pytest.fixture(scope="module")
def trees(rt, scenes):
    return Trees(rt, scenes)


class Result:
    pass


def _shape(rt, q):
    return rt.kRangeBox if "lo" in q.dtype.names else rt.kRangeSphere


def _count(rt, triangles, nodes, root, count, q):
    """-> (offsets int64[n+1] numpy, counters uint64[4], status, device tensors for a following collect)"""
    import torch
    n = len(q)
    qd = rt.to_device(q).view(torch.float32)
    off = torch.full((n + 1 + PAD,), SENT, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert rt.RangeCount(triangles, nodes, root, count, qd, off[:n + 1], shape=_shape(rt, q), counters=ctr, status=st) == n
    torch.cuda.synchronize()
    o = off.cpu().numpy()
    assert (o[n + 1:] == SENT).all(), "RangeCount wrote past offsets[n]"
    return o[:n + 1], ctr.cpu().numpy().astype(np.uint64), rt.range_status(st), (qd, off)


def _collect(rt, triangles, nodes, root, count, q, qd, off_dev, capacity):
    """-> (ids uint32[capacity] numpy, counts uint32[n], counters, status); sentinels behind ids and counts are checked"""
    import torch
    n = len(q)
    ids = torch.full((capacity + PAD,), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    rt.RangeCollect(triangles, nodes, root, count, qd, off_dev[:n + 1], ids, shape=_shape(rt, q), counts=cnt[:n], counters=ctr,
                    status=st)
    torch.cuda.synchronize()
    i, c = ids.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert (i[capacity:] == SENT).all(), "RangeCollect wrote past the last segment"
    assert (c[n:] == SENT).all(), "RangeCollect wrote counts past num_queries"
    return i[:capacity], c[:n], ctr.cpu().numpy().astype(np.uint64), rt.range_status(st)


def _range(rt, g, q):
    """count, then collect into exactly offsets[n] ids: a Result with offsets, lists (per query, traversal order), counts,
    both calls' counters and statuses.  Asserts what must hold on ANY tree: count and collect agree."""
    inp, root, count = g
    return _range_raw(rt, inp.triangles_out, inp.nodes_out, root, count, q)


def _range_raw(rt, tri, nod, root, count, q):
    r = Result()
    r.offsets, r.ctr_count, r.st_count, (qd, off) = _count(rt, tri, nod, root, count, q)
    n = len(q)
    assert r.offsets[0] == 0 and (np.diff(r.offsets) >= 0).all()
    total = int(r.offsets[n])
    ids, r.counts, r.ctr_collect, r.st_collect = _collect(rt, tri, nod, root, count, q, qd, off, total)
    assert (r.counts.astype(np.int64) == np.diff(r.offsets)).all(), "collect's counts differ from the differences of offsets"
    assert (ids != SENT).all(), "a segment was not filled"
    assert (r.ctr_count == r.ctr_collect).all(), f"counters differ: count {r.ctr_count}, collect {r.ctr_collect}"
    assert r.ctr_count[2] == 0 and r.ctr_count[3] == 0
    assert r.st_count == r.st_collect and not (r.st_collect & rt.RT_RANGE_TRUNCATED)
    r.lists = [ids[r.offsets[k]:r.offsets[k + 1]] for k in range(n)]
    return r


def _expected(q, tris):
    if "lo" in q.dtype.names:
        return rr.box(q["lo"], q["hi"], tris)
    return rr.sphere(q["p"], q["dist2_max"], tris)


def _assert_exact(r, exp, what):
    lists, counts = exp
    assert (r.offsets == rr.offsets(counts)).all(), \
        f"{what}: offsets differ, first at query {np.nonzero(np.diff(r.offsets) != counts)[0][:5]}"
    for k, (got, e) in enumerate(zip(r.lists, lists)):
        s = np.sort(got)
        assert (s == e).all(), f"{what}: query {k}: got {s[:8]}... expected {e[:8]}..."     # (sorted and equal: no duplicates)


# ------------------------------------------------------------------ 1 + 2: exact on every non-split tree
@pytest.mark.parametrize("name", rs.SCENES)
def test_exact_against_brute_force_on_every_tree(rt, trees, name):
    tris = trees.tris(name)
    sets = rs.query_sets(tris, rs.seed_of(name))
    for key, q in sets.items():
        exp = _expected(q, tris)
        assert (exp[1] > 0).sum() * 4 >= rs.NQ and exp[1].sum() >= rs.NQ       # (the CPU test's guarantee, restated)
        first = None
        for tree in EXACT_TREES:
            r = _range(rt, trees.gpu(name, tree), q)
            print(f"{name}/{tree}/{key}: ids {int(r.offsets[-1])}, box tests {int(r.ctr_count[0])}, "
                  f"triangle tests {int(r.ctr_count[1])}")
            _assert_exact(r, exp, f"{name}/{tree}/{key}")
            assert r.st_count == 0 and r.ctr_count[0] > 0 and r.ctr_count[1] > 0
            sorted_lists = [np.sort(x) for x in r.lists]
            if first is None:
                first = sorted_lists
            assert all((a == b).all() for a, b in zip(first, sorted_lists))


# ------------------------------------------------------------------ 3: edges
def test_radius_edges_untraced_and_batch_ends(rt, trees):
    import torch
    tris = trees.tris("soup")
    T = tris.reshape(-1, 3, 3)
    g = trees.gpu("soup", "sah_pairs")
    sets = rs.query_sets(tris, 3)
    p = sets["sphere", "uniform"]["p"][:200]
    # a radius exactly at the d2 of the 5th nearest triangle accepts it; the next float below rejects it
    d, _, _ = pr.d2(p[:, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])
    kth = np.argsort(d, axis=1, kind="stable")[:, 4]
    at = d[np.arange(len(p)), kth]
    assert (at > 0).all()
    q = rs.sphere_queries(p, 0)
    q["dist2_max"] = at
    r = _range(rt, g, q)
    _assert_exact(r, _expected(q, tris), "radius at d2")
    assert all(kth[k] in r.lists[k] for k in range(len(p))) and (r.counts >= 5).all()
    q["dist2_max"] = np.nextafter(at, F(0))
    r = _range(rt, g, q)
    _assert_exact(r, _expected(q, tris), "radius below d2")
    assert all(kth[k] not in r.lists[k] for k in range(len(p)))
    # a box face exactly on a vertex coordinate accepts; one float further rejects that triangle
    k = np.arange(200)
    tlo, thi = T[k].min(1), T[k].max(1)
    big = F(10.0)
    lo, hi = np.full((200, 3), -big, F), np.full((200, 3), big, F)
    hi[:, 0] = tlo[:, 0]                                           # the query's +x face on the triangle's lowest x
    qb = rs.box_queries(lo, hi)
    r = _range(rt, g, qb)
    _assert_exact(r, _expected(qb, tris), "box face on a vertex")
    assert all(k[j] in r.lists[j] for j in range(200))
    qb["hi"][:, 0] = np.nextafter(tlo[:, 0], F(-np.inf))
    r = _range(rt, g, qb)
    _assert_exact(r, _expected(qb, tris), "box face below a vertex")
    assert all(k[j] not in r.lists[j] for j in range(200))
    # untraced: 0 matches and no tests counted
    bad = rs.sphere_queries(p[:6], 1.0)
    bad["p"][0, 0], bad["p"][1, 1], bad["p"][2, 2] = np.nan, np.inf, -np.inf
    bad["dist2_max"][3], bad["dist2_max"][4], bad["dist2_max"][5] = np.nan, -1.0, -np.inf
    r = _range(rt, g, bad)
    assert (r.offsets == 0).all() and (r.ctr_count == 0).all() and (r.ctr_collect == 0).all()
    badb = rs.box_queries(np.zeros((4, 3), F), np.ones((4, 3), F))
    badb["lo"][0, 1], badb["hi"][1, 2], badb["lo"][2, 0] = np.nan, np.nan, 2.0
    badb["lo"][3], badb["hi"][3] = (0.5, 0.5, 0.5), (0.5, 0.5, np.nextafter(F(0.5), F(0)))
    r = _range(rt, g, badb)
    assert (r.offsets == 0).all() and (r.ctr_count == 0).all() and (r.ctr_collect == 0).all()
    # a +inf radius returns every triangle
    q = rs.sphere_queries(p[:3], 0)
    q["dist2_max"] = np.inf
    r = _range(rt, g, q)
    assert all((np.sort(x) == np.arange(T.shape[0])).all() for x in r.lists)
    # a batch that ends inside a wave and inside a workgroup
    for n in (1, 70, 257):
        qq = sets["sphere", "near"][:n]
        _assert_exact(_range(rt, g, qq), _expected(qq, tris), f"batch of {n}")
    # an empty tree: every set is empty, nothing counted
    inp = g[0]
    r = _range_raw(rt, inp.triangles_out, inp.nodes_out, 0, 0, sets["box", "near"][:300])
    assert (r.offsets == 0).all() and (r.ctr_count == 0).all()
    # an empty batch still writes offsets[0] = 0
    off = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    empty = torch.empty((0, 4), dtype=torch.float32, device="cuda")
    assert rt.RangeCount(inp.triangles_out, inp.nodes_out, g[1], g[2], empty, off[:1]) == 0
    torch.cuda.synchronize()
    assert off.cpu().numpy().tolist() == [0, SENT, SENT, SENT]


def test_signed_zero_box_faces(rt, trees):
    """a query face at -0.0 against vertex coordinates of +0.0 (and the reverse) overlaps: the compare is closed and -0 == +0"""
    tris = trees.tris("signed_zero")
    T = tris.reshape(-1, 3, 3)
    tlo, thi = T.min(1), T.max(1)
    big = F(100.0)
    q = rs.box_queries(np.full((4, 3), -big, F), np.full((4, 3), big, F))
    q["hi"][0, 1] = F(-0.0)           # everything at or below y = 0
    q["hi"][1, 1] = F(0.0)
    q["lo"][2, 0], q["hi"][2, 0] = F(0.0), F(-0.0)       # the plane x = 0: lo = +0 > hi = -0 is NOT lo > hi (they are equal)
    q["lo"][3, 2], q["hi"][3, 2] = F(-0.0), F(0.0)
    exp = _expected(q, tris)
    zero_y = np.nonzero((tlo[:, 1] == 0) & ~np.signbit(tlo[:, 1]))[0]
    assert zero_y.size and np.isin(zero_y, exp[0][0]).all() and (exp[1] > 0).all()
    for tree in ("bottom_up", "hybrid_pairs", "sah"):
        _assert_exact(_range(rt, trees.gpu("signed_zero", tree), q), exp, f"signed zero/{tree}")


# ------------------------------------------------------------------ 4: truncation with fixed-K offsets
@pytest.mark.parametrize("shape", ("sphere", "box"))
def test_fixed_k_truncation(rt, trees, shape):
    import torch
    tris = trees.tris("grid")
    g = trees.gpu("grid", "pairs")
    inp, root, count = g
    q = rs.query_sets(tris, 17)[shape, "uniform"]
    n, K = len(q), 6
    lists, counts = _expected(q, tris)
    assert (counts > K).sum() > 20 and ((counts > 0) & (counts < K)).sum() > 20       # both sides of K occur
    qd = rt.to_device(q).view(torch.float32)
    off = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
    ids, cnt, _, st = _collect(rt, inp.triangles_out, inp.nodes_out, root, count, q, qd, off, n * K)
    assert st == rt.RT_RANGE_TRUNCATED
    assert (cnt.astype(np.int64) == counts).all(), "counts must be exact beyond the room"
    seg = ids.reshape(n, K)
    for k in range(n):
        m = min(int(counts[k]), K)
        assert np.isin(seg[k, :m], lists[k]).all() and len(set(seg[k, :m].tolist())) == m, f"query {k}"
        assert (seg[k, m:] == SENT).all(), f"query {k} wrote past its matches"
    # the truncated segments are the head of the untruncated traversal order
    full = _range(rt, g, q)
    assert all((seg[k, :min(int(counts[k]), K)] == full.lists[k][:K]).all() for k in range(n))
    # room everywhere: no flag
    off = (torch.arange(n + 1, dtype=torch.int64) * int(counts.max())).cuda()
    _, _, _, st = _collect(rt, inp.triangles_out, inp.nodes_out, root, count, q, qd, off, n * int(counts.max()))
    assert st == 0


# ------------------------------------------------------------------ 5: refit
@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs", "sah_splits"))
def test_refit_then_query(rt, scenes, tree):
    import torch
    tris = rs.scene_tris("grid", scenes)
    inp, root, count = _gpu_tree(rt, tris, tree)
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    for step in (1.0, 2.5):
        moved = _move(tris, step)
        inp.triangles_in.copy_(rt.to_device(moved))
        rt.Refit(inp, root, count, plan)
        torch.cuda.synchronize()
        assert rt.refit_status(plan, inp.num_triangles) == 0
        for key, q in rs.query_sets(moved, int(step * 10)).items():
            r = _range(rt, (inp, root, count), q)
            exp = _expected(q, moved)
            assert r.st_count == 0
            if "splits" in tree:
                # refit writes unclipped boxes, so every match is reached -- through each of its references: as sets
                assert all(np.array_equal(np.unique(got), e) for got, e in zip(r.lists, exp[0])), f"refit {tree}/{key}"
            else:
                _assert_exact(r, exp, f"refit {tree}/{key}")


# ------------------------------------------------------------------ 6: split trees before refit
@pytest.mark.parametrize("name", ("grid", "soup", "cornell", "signed_zero"))
def test_split_trees_report_true_matches(rt, trees, name):
    tris = trees.tris(name)
    for key, q in rs.query_sets(tris, 7 + len(name)).items():
        lists, counts = _expected(q, tris)
        for tree in SPLIT_TREES:
            r = _range(rt, trees.gpu(name, tree), q)          # (count and collect agree: asserted inside)
            assert r.st_count == 0
            assert all(np.isin(got, e).all() for got, e in zip(r.lists, lists)), f"{name}/{tree}/{key}: a false match"
            assert r.offsets[-1] > 0


# ------------------------------------------------------------------ 7: deep and wide trees, stack overflow
def test_deep_and_wide_trees_are_exact(rt, trees):
    tris = trees.tris("fractal")
    sets = rs.query_sets(tris, 21)
    for key in (("sphere", "near"), ("box", "near")):
        exp = _expected(sets[key], tris)
        for tree in ("bottom_up", "sah", "hybrid"):
            r = _range(rt, trees.gpu("fractal", tree), sets[key])
            assert r.st_count == 0
            _assert_exact(r, exp, f"fractal/{tree}/{key}")
    tris = trees.tris("grid")
    inp, root, count = trees.gpu("grid", "bottom_up")
    nodes, _ = _download(rt, inp, tris.shape[0])
    sets = rs.query_sets(tris, 22)
    for width in (3, 4, 7):
        wn, wr, wc = edge_scenes.collapse_wide(nodes, root, count, width, rt.NODE)
        wd = rt.to_device(wn)
        for key in (("sphere", "uniform"), ("box", "uniform")):
            r = _range_raw(rt, inp.triangles_out, wd, wr, wc, sets[key])
            assert r.st_count == 0
            _assert_exact(r, _expected(sets[key], tris), f"width {width}/{key}")


@pytest.mark.parametrize("shape", ("sphere", "box"))
def test_stack_overflow_is_flagged_and_the_result_is_a_subset(rt, shape):
    """a comb of 80 two-slot nodes whose boxes all contain the region: every node pushes its leaf and descends, so 80 entries
    are pending before the first pop; the 16 pushes beyond 64 are dropped, flagged, and missing from the result"""
    L = 80
    rng = np.random.default_rng(5)
    tris = _comb_triangles(rng, L, lambda k: 2.0 + k % 7)
    leaves, nodes = _comb(rt, tris, tight_leaf_boxes=False)
    if shape == "sphere":
        q = rs.sphere_queries(rng.uniform(-0.05, 0.05, (4, 3)).astype(F), 20.0)
    else:
        q = rs.box_queries(np.full((4, 3), -20, F), np.full((4, 3), 20, F))
    lists, counts = _expected(q, tris.reshape(-1, 9))
    assert (counts == L + 1).all()                      # the truth: every triangle
    r = _range_raw(rt, leaves, nodes, 0, 2, q)
    assert r.st_count & rt.RT_RANGE_STACK_OVERFLOW and r.st_collect & rt.RT_RANGE_STACK_OVERFLOW
    for k in range(4):
        got = np.sort(r.lists[k])
        assert np.isin(got, lists[k]).all() and len(np.unique(got)) == len(got)
        assert (got == np.concatenate([np.arange(64), [L]])).all()     # the 64 kept pushes and the bottom leaf
    assert r.ctr_count[1] == 4 * 65 and r.ctr_count[0] == 4 * 2 * L


# ------------------------------------------------------------------ 8: cross-check against the closest-point query
@pytest.mark.parametrize("name", ("grid", "soup"))
def test_closest_point_is_a_member(rt, trees, name):
    tris = trees.tris(name)
    g = trees.gpu(name, "hybrid_pairs")
    inp, root, count = g
    for kind in ("near", "uniform", "on_vertex_edge"):
        q = rs.query_sets(tris, 40)["sphere", kind]
        r = _range(rt, g, q)
        hits, _, _ = _closest(rt, inp.triangles_out, inp.nodes_out, root, count, _queries(q["p"], q["dist2_max"]))
        hit = hits["primitive_id"] != pr.MISS
        assert (hit == (r.counts > 0)).all() and hit.sum() * 4 >= len(q)
        assert all(hits["primitive_id"][k] in r.lists[k] for k in np.nonzero(hit)[0])


# ------------------------------------------------------------------ 9: hipGraph
def test_build_count_and_collect_in_a_hip_graph(rt, scenes):
    import torch
    tris = np.ascontiguousarray(scenes.grid_mesh(40, 3), F).reshape(-1, 9)
    inp = rt.BuildInput.allocate(tris)
    sets = rs.query_sets(tris, 9)
    K = 256
    work = []
    for key in (("sphere", "near"), ("box", "uniform")):
        q = sets[key]
        n = len(q)
        work.append(dict(q=q, qd=rt.to_device(q).view(torch.float32), shape=_shape(rt, q),
                         off=torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                         fixed=(torch.arange(n + 1, dtype=torch.int64) * K).cuda(),
                         ids=torch.empty(n * K, dtype=torch.int32, device="cuda"),
                         cnt=torch.empty(n, dtype=torch.int32, device="cuda"),
                         scratch=rt.device_bytes(rt.RangeScratchBytes(n))))
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        rt.RunBottomUpBuild(inp)
        for w in work:
            w["ids"].fill_(-1)
            rt.RangeCount(inp.triangles_out, inp.nodes_out, 0, 2, w["qd"], w["off"], shape=w["shape"], scratch=w["scratch"],
                          counters=ctr, status=st)
            rt.RangeCollect(inp.triangles_out, inp.nodes_out, 0, 2, w["qd"], w["fixed"], w["ids"], shape=w["shape"],
                            counts=w["cnt"], counters=ctr, status=st)

    def outputs():
        return [t for w in work for t in (w["off"], w["ids"], w["cnt"])] + [ctr, st]

    one_frame()
    torch.cuda.synchronize()
    eager = [t.clone() for t in outputs()]
    for w in work:                       # the eager frame is right: offsets and the per-query sets (K holds every set here)
        lists, counts = _expected(w["q"], tris)
        assert counts.max() <= K and counts.sum() >= len(w["q"])
        assert (w["off"].cpu().numpy() == rr.offsets(counts)).all() and (w["cnt"].cpu().numpy() == counts).all()
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


def test_range_query_convenience(rt, trees):
    import torch
    tris = trees.tris("cornell")
    inp, root, count = trees.gpu("cornell", "sah")
    for key in (("sphere", "uniform"), ("box", "near")):
        q = rs.query_sets(tris, 2)[key]
        lists, counts = _expected(q, tris)
        off, ids = rt.RangeQuery(inp.triangles_out, inp.nodes_out, root, count, rt.to_device(q).view(torch.float32),
                                 shape=_shape(rt, q))
        assert off.dtype == torch.int64 and ids.dtype == torch.int32 and ids.numel() == counts.sum()
        o, i = off.cpu().numpy(), ids.cpu().numpy().view(np.uint32)
        assert (o == rr.offsets(counts)).all()
        assert all((np.sort(i[o[k]:o[k + 1]]) == lists[k]).all() for k in range(len(lists)))


# ------------------------------------------------------------------ 10. the scan past one chunk and past one limb
@pytest.fixture(scope="module")
def tiny(rt):
    return _gpu_tree(rt, rr.scan_tiny_tris(), "bottom_up")


@pytest.fixture(scope="module")
def chunk_counts():
    """brute-force counts of the largest chunk-loop batch, computed once; a smaller batch is its prefix"""
    reach = rr.scan_reach_pattern(max(rr.SCAN_CHUNK_N))
    counts = rr.sphere_matrix(np.tile(F([0.2, 0.2, 0.0]), (len(reach), 1)), reach * reach, rr.scan_tiny_tris()).sum(axis=1)
    assert set(np.unique(counts)) == {0, 1, 2, 3, 4}
    return counts


@pytest.mark.parametrize("n", rr.SCAN_CHUNK_N)
def test_count_scan_chunk_loop(rt, tiny, chunk_counts, n):
    """more than 1024 workgroups: the one-workgroup scan over the block sums runs its chunk loop (RangeCount only)"""
    inp, root, count = tiny
    reach = rr.scan_reach_pattern(n)
    q = _queries(np.tile(F([0.2, 0.2, 0.0]), (n, 1)), reach * reach)
    offsets, _, status, _ = _count(rt, inp.triangles_out, inp.nodes_out, root, count, q)
    exp = np.concatenate([[0], np.cumsum(chunk_counts[:n], dtype=np.int64)])
    assert status == 0
    assert offsets[n] == chunk_counts[:n].sum()
    assert (offsets == exp).all(), f"first wrong offset at query {int(np.argmax(offsets != exp))}"


def test_count_scan_limb_carry(rt, scenes):
    """every query matches all 16400 triangles: the prefix passes 2^21 inside a workgroup (at lane 128) and in the block
    totals, so both scans carry out of their lowest 21-bit limb (RangeCount only)"""
    ntri, n = 16400, 512
    inp, root, count = _gpu_tree(rt, scenes.soup(ntri, 11), "bottom_up")
    pts = np.random.default_rng(5).uniform(-1.0, 2.0, (n, 3)).astype(F)
    offsets, _, status, _ = _count(rt, inp.triangles_out, inp.nodes_out, root, count, _queries(pts, F(1e30)))
    assert status == 0
    assert 128 * ntri >= 1 << 21 > 127 * ntri
    assert (offsets == ntri * np.arange(n + 1, dtype=np.int64)).all()
