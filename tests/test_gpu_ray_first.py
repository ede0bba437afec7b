"""GPU tests of the first-K ray query (rt_ray_first_hits) on every tree the builders make, against tests/ray_first_ref.py: the
all-hit tree walk over the tree's own bytes with the gate of every record, from which E (the row of a decided ray), the decided
flag and the envelope (claims 1 and 3 of include/rt_abi.h, which hold on every ray) follow with no kernel involved.

1. k in {1, 2, 3, 8, 32} on the eight trees of the four scenes of test_gpu_ray_hits.py: the undecided share of the reference
   alone is under the cap (asserted before the kernel's rows are looked at); the row of every decided ray is E, bit for bit;
   claims 1 and 3 on every ray; the counters are at most the all-hit walk's;
2. k = 32 where the longest row is below 32: the row is the sorted W and the counters equal rt_ray_hits_count's;
3. the bound shrinks: counters at most rt_ray_hits_count's, strictly fewer box tests on the rays from inside with tmax = +inf;
4. order and ties on a stack of 40 parallel quads, plain and with every triangle duplicated under a second id;
5. dead rays, sentinels, the empty tree, batch ends, a window that excludes the first layers;
6. refit; 7. build + query in one hipGraph; 8. stack overflow: the flag, and rows that are sorted subsets of W."""
import numpy as np
import pytest

import range_sets as rs
import ray_first_ref as rf
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

TREES = ("bottom_up", "pairs", "hybrid", "hybrid_pairs", "sah", "sah_pairs", "sah_splits", "sah_pairs_splits")
SCENES = ("grid", "soup", "cornell", "fractal")
KS = (1, 2, 3, 8, 32)
F = np.float32
SENT = 0x5EA7BEEF        # sentinel word of every output buffer
PAD = 64                 # sentinel records behind every output buffer


# ------------------------------------------------------------------ helpers
def _dev_rays(rt, rays):
    import torch
    return rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)


def _first(rt, tri, nod, root, count, rays, k):
    """-> (rows: HIT [n, k], counters uint64[4], status).  64 sentinel records lie behind the rows and must survive; every
    record of every row must have been written."""
    import torch
    rd = _dev_rays(rt, rays)
    n = rd.shape[0]
    buf = torch.full(((n * k + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    out = buf[:n * k * 4].view(torch.float32).view(n, k, 4)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert rt.RayFirstHits(tri, nod, root, count, rd, k, out, counters=ctr, status=st) == n
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[n * k * 4:] == SENT).all(), "RayFirstHits wrote past the last row"
    assert (h[:n * k * 4].reshape(-1, 4) != SENT).any(1).all(), "a record of a row was not written"
    c = ctr.cpu().numpy().astype(np.uint64)
    assert c[2] == 0 and c[3] == 0
    return h[:n * k * 4].view(rf.HIT).reshape(n, k), c, rt.ray_first_status(st)


def _all_hit_counters(rt, tri, nod, root, count, rays):
    import torch
    rd = _dev_rays(rt, rays)
    off = torch.empty(rd.shape[0] + 1, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    rt.RayHitsCount(tri, nod, root, count, rd, off, counters=ctr)
    torch.cuda.synchronize()
    return ctr.cpu().numpy().astype(np.uint64), np.diff(off.cpu().numpy())


def _download(rt, inp):
    n = inp.num_triangles
    return rt.to_host(inp.nodes_out, rt.NODE, rt.NodesBytes(n) // 32), rt.to_host(inp.triangles_out, rt.TRIANGLE_PAIR, n)


class Walk:
    """the reference of one (tree, ray set): W with gates, its counters, and Ws -- computed once, never changed"""
    def __init__(self, nodes, leaves, root, count, rays):
        self.rays = rays
        self.rows, self.gates, self.box_tests, self.leaf_visits = rf.walk_gated(nodes, leaves, root, count, rays)
        self.dedup = rf.dedup_all(self.rows, self.gates)
        self.nonempty = int(sum(len(r) > 0 for r in self.rows))

    def expected(self, k):
        return rf.expected(self.rows, self.gates, k, self.rays["tmax"], dedup=self.dedup)


def _check_rows(rows, walk, k, what, exp=None):
    """the row of every decided ray is E bit for bit; claims 1 and 3 on every ray, decided or not.  -> number of rows that
    differ from E"""
    exp = walk.expected(k) if exp is None else exp
    n = len(walk.rays)
    want = rf.padded(exp, k)
    equal = (rows.view(np.uint32).reshape(n, -1) == want.view(np.uint32).reshape(n, -1)).all(1)
    decided = np.array([e[1] for e in exp], bool)
    wrong = np.nonzero(decided & ~equal)[0]
    assert len(wrong) == 0, f"{what}: k {k}: {len(wrong)} decided rays differ from E; ray {wrong[0]}: {rows[wrong[0]]} != {want[wrong[0]]}"
    for i in range(n):
        why = rf.envelope_violation(rows[i], walk.rows[i], walk.gates[i], k, walk.rays["tmax"][i])
        assert why is None, f"{what}: k {k}: ray {i}: {why}"
    return int((~equal).sum())


class World:
    """scenes, their ray sets, built trees and, per (scene, tree), the reference over the downloaded bytes -- computed once"""
    def __init__(self, rt, scenes):
        self.rt, self.scenes = rt, scenes
        self._sc, self._g, self._w = {}, {}, {}

    def scene(self, name):
        if name not in self._sc:
            tris = rs.scene_tris(name, self.scenes)
            self._sc[name] = tris, rf.ray_sets(tris, rf.SEEDS[name]).astype(self.rt.RAY)
        return self._sc[name]

    def gpu(self, name, tree):
        if (name, tree) not in self._g:
            self._g[name, tree] = _gpu_tree(self.rt, self.scene(name)[0], tree)
        return self._g[name, tree]

    def walk(self, name, tree):
        if (name, tree) not in self._w:
            inp, root, count = self.gpu(name, tree)
            nodes, leaves = _download(self.rt, inp)
            self._w[name, tree] = Walk(nodes, leaves, root, count, self.scene(name)[1])
        return self._w[name, tree]


@pytest.fixture(scope="module")
def world(rt, scenes):
    return World(rt, scenes)


# ------------------------------------------------------------------ 1: decided rays are E, every ray is inside the envelope
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_rows_against_the_gated_walk(world, name, tree):
    rt = world.rt
    inp, root, count = world.gpu(name, tree)
    rays = world.scene(name)[1]
    walk = world.walk(name, tree)
    what = f"{name}/{tree}"
    assert len(rays) == 2048 and walk.nonempty >= len(rays) // 8 and max(len(r) for r in walk.rows) >= 2, "the ray set is not trivial"
    for k in KS:
        exp = walk.expected(k)
        share = rf.undecided_share(exp, walk.rows)            # the reference alone: a condition on the inputs
        print(f"{what}: k {k}: {100 * share:.3f} % of {walk.nonempty} rays undecided")
        assert share <= rf.CAP, f"{what}: k {k}: {100 * share:.2f} % of the rays are undecided"
        rows, ctr, status = _first(rt, inp.triangles_out, inp.nodes_out, root, count, rays, k)
        assert status == 0, f"{what}: k {k}: status {status}"
        differ = _check_rows(rows, walk, k, what, exp)
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits, \
            f"{what}: k {k}: counters {ctr[:2]} exceed the all-hit walk's {walk.box_tests}, {walk.leaf_visits}"
        print(f"{what}: k {k}: {differ} rows differ from E; box tests {int(ctr[0])} of {walk.box_tests}, "
              f"leaf visits {int(ctr[1])} of {walk.leaf_visits}")


# ------------------------------------------------------------------ 2: rows shorter than k
@pytest.mark.parametrize("tree", TREES)
def test_k_above_the_longest_row_is_the_sorted_all_hit_row(world, tree):
    rt = world.rt
    inp, root, count = world.gpu("grid", tree)
    rays = world.scene("grid")[1]
    walk = world.walk("grid", tree)
    longest = max(len(r) for r in walk.rows)                  # (duplicates of a split tree included: |Ws| <= |W| < k)
    assert 2 <= longest < 32, f"grid/{tree}: the longest all-hit row has {longest} records"
    rows, ctr, status = _first(rt, inp.triangles_out, inp.nodes_out, root, count, rays, 32)
    assert status == 0
    exp = walk.expected(32)
    assert all(e[1] for e in exp), "a ray with |W| <= k is always decided"
    want = rf.padded(exp, 32)
    assert rows.tobytes() == want.tobytes(), "the row is not the sorted all-hit row"
    for i, (ws, _) in enumerate(walk.dedup):
        assert (rows["primitive_id"][i] != rf.MISS).sum() == len(ws)
    hits_ctr, lengths = _all_hit_counters(rt, inp.triangles_out, inp.nodes_out, root, count, rays)
    assert (lengths == [len(r) for r in walk.rows]).all()
    assert (ctr == hits_ctr).all(), f"grid/{tree}: counters {ctr[:2]}, rt_ray_hits_count's {hits_ctr[:2]}"
    assert ctr[0] == walk.box_tests and ctr[1] == walk.leaf_visits


# ------------------------------------------------------------------ 3: the bound shrinks
@pytest.mark.parametrize("tree", ("bottom_up", "hybrid_pairs", "sah_pairs"))
def test_counters_fall_below_the_all_hit_query(world, tree):
    rt = world.rt
    inp, root, count = world.gpu("grid", tree)
    rays = world.scene("grid")[1]
    inside_inf = rays[3 * 512:]                               # ray_sets' fourth kind: from inside, tmax = +inf
    assert len(inside_inf) == 512 and np.isinf(inside_inf["tmax"]).all()
    for batch, strictly in ((rays, False), (inside_inf, True)):
        hits_ctr, lengths = _all_hit_counters(rt, inp.triangles_out, inp.nodes_out, root, count, batch)
        assert lengths.max() > 8 or not strictly, "some ray must cross more than k triangles"
        for k in (1, 8):
            _, ctr, status = _first(rt, inp.triangles_out, inp.nodes_out, root, count, batch, k)
            assert status == 0 and ctr[0] <= hits_ctr[0] and ctr[1] <= hits_ctr[1], f"k {k}: {ctr[:2]} against {hits_ctr[:2]}"
            print(f"grid/{tree}: {len(batch)} rays, k {k}: box tests {int(ctr[0])} / {int(hits_ctr[0])}, "
                  f"leaf visits {int(ctr[1])} / {int(hits_ctr[1])}")
            if strictly:
                assert ctr[0] < hits_ctr[0], f"k {k}: {ctr[0]} box tests, the all-hit query {hits_ctr[0]}: the bound never shrank"


# ------------------------------------------------------------------ 4: order and ties
LAYERS = 40


def _quad_stack(layers=LAYERS):
    """parallel unit quads at z = 0 .. layers-1, two triangles each that share the diagonal (pairs merge them).  With
    origin.z = -1 and dir.z = 1 every edge component is 0 or +-1, so Moller-Trumbore's t of layer j is exactly j + 1, and so is
    the slab front of a flat box at z = j: the ties below are exact and every ray is decided"""
    tris = np.zeros((2 * layers, 3, 3), F)
    for k in range(layers):
        a, b, c, d = (0, 0, k), (1, 0, k), (1, 1, k), (0, 1, k)
        tris[2 * k], tris[2 * k + 1] = (a, b, c), (a, c, d)
    return np.ascontiguousarray(tris.reshape(-1, 9))


def _stack_rays(rt, n, seed):
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, rt.RAY)
    rays["origin"][:, :2] = rng.uniform(0.2, 0.8, (n, 2))
    rays["origin"][:, 2] = -1.0
    rays["dir"] = (0.003, -0.002, 1.0)
    rays["tmin"], rays["tmax"] = 0.0, np.inf
    return rays


@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs"))
def test_layers_come_in_order(rt, tree):
    assert LAYERS > rt.RT_RAY_FIRST_MAX_K
    inp, root, count = _gpu_tree(rt, _quad_stack(), tree)
    rays = _stack_rays(rt, 200, 4)
    walk = Walk(*_download(rt, inp)[:2], root, count, rays)
    assert all(len(r) == LAYERS for r in walk.rows), "every ray crosses every layer once"
    for k in (1, 5, 32):
        rows, ctr, status = _first(rt, inp.triangles_out, inp.nodes_out, root, count, rays, k)
        assert status == 0
        assert all(e[1] for e in walk.expected(k)), "exact coordinates: every ray is decided"
        assert _check_rows(rows, walk, k, f"stack/{tree}") == 0
        assert (rows["primitive_id"] // 2 == np.arange(k)[None, :]).all(), f"k {k}: not the first {k} layers in order"
        assert (rows["t"] == np.arange(1, k + 1, dtype=F)[None, :]).all()
        assert ctr[0] < walk.box_tests or k == 32


@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs"))
def test_ties_go_to_the_lower_id(rt, tree):
    tris = _quad_stack()
    nt = tris.shape[0]
    inp, root, count = _gpu_tree(rt, np.ascontiguousarray(np.concatenate([tris, tris])), tree)     # triangle j again as j + nt
    rays = _stack_rays(rt, 200, 5)
    walk = Walk(*_download(rt, inp)[:2], root, count, rays)
    assert all(len(r) == 2 * LAYERS for r in walk.rows)
    for k in (1, 2, 5, 32):
        rows, _, status = _first(rt, inp.triangles_out, inp.nodes_out, root, count, rays, k)
        assert status == 0
        assert all(e[1] for e in walk.expected(k)), "exact coordinates: every ray is decided"
        assert _check_rows(rows, walk, k, f"doubled stack/{tree}") == 0
        j = np.arange(k)
        assert (rows["t"] == (j // 2 + 1).astype(F)[None, :]).all(), f"k {k}: layer j twice, then layer j + 1"
        ids = rows["primitive_id"].astype(np.int64)
        assert (ids[:, 0::2] < nt).all() and (ids[:, 1::2] == ids[:, 0:2 * (k // 2):2] + nt).all(), \
            f"k {k}: a tie on t does not list the lower id first (an odd k ends on the lower id of its pair)"
        assert (ids[:, 0::2] // 2 == (j[0::2] // 2)[None, :]).all()


# ------------------------------------------------------------------ 5: dead rays, the empty tree, batch ends, windows
def test_dead_rays_the_empty_tree_and_batch_ends(world):
    rt = world.rt
    rays = world.scene("soup")[1]
    inp, root, count = world.gpu("soup", "hybrid_pairs")
    tri, nod = inp.triangles_out, inp.nodes_out
    k = 3
    full, _, _ = _first(rt, tri, nod, root, count, rays, k)
    nan = F(np.nan)
    deg = rays[:9].copy()
    deg["tmin"][0], deg["tmax"][0] = 5.0, 1.0                 # tmin > tmax
    deg["origin"][1, 0] = nan
    deg["dir"][2, 1] = nan
    deg["tmin"][3] = nan
    deg["tmax"][4] = nan
    deg["dir"][5] = nan
    deg["origin"][6] = nan
    deg["tmin"][7], deg["tmax"][7] = 1e-5, 0.0
    deg["tmin"][8], deg["tmax"][8] = 0.0, -1.0                # an off-frame lane of GenerateCameraRays
    assert not rf.live(deg).any()
    rows, ctr, status = _first(rt, tri, nod, root, count, deg, k)
    assert rows.tobytes() == rf.miss_records(9 * k).tobytes() and (ctr == 0).all() and status == 0
    # dead rays among live ones: rows of misses, the others' rows are the batch's own
    mixed = rays[:300].copy()
    mixed[10:300:29] = deg[np.arange(len(mixed[10:300:29])) % 9]
    dead = ~rf.live(mixed)
    assert dead.sum() == 10
    rows, _, _ = _first(rt, tri, nod, root, count, mixed, k)
    assert rows[dead].tobytes() == rf.miss_records(10 * k).tobytes()
    assert rows[~dead].tobytes() == full[:300][~dead].tobytes()
    # an empty tree (count = 0): every row misses, nothing counted
    rows, ctr, status = _first(rt, tri, nod, 0, 0, rays[:300], k)
    assert rows.tobytes() == rf.miss_records(300 * k).tobytes() and (ctr == 0).all() and status == 0
    # batch ends (sentinels behind every buffer: checked inside)
    for n in (1, 63, 64, 65, 255, 257):
        for kk in (1, k):
            rows, _, _ = _first(rt, tri, nod, root, count, rays[:n], kk)
            assert rows.tobytes() == np.ascontiguousarray(full[:n, :kk]).tobytes(), f"batch of {n}, k {kk}"


def test_a_window_that_excludes_the_first_layers(rt):
    inp, root, count = _gpu_tree(rt, _quad_stack(), "pairs")
    rays = _stack_rays(rt, 130, 6)
    rays["tmin"], rays["tmax"] = 3.0, 9.5                     # layers at t = 3 (closed at tmin) .. 9
    walk = Walk(*_download(rt, inp)[:2], root, count, rays)
    assert all(len(r) == 7 for r in walk.rows)
    for k, live_records in ((1, 1), (4, 4), (7, 7), (8, 7), (32, 7)):
        rows, _, status = _first(rt, inp.triangles_out, inp.nodes_out, root, count, rays, k)
        assert status == 0 and _check_rows(rows, walk, k, "window") == 0
        assert (rows["t"][:, :live_records] == np.arange(3, 3 + live_records, dtype=F)[None, :]).all()
        assert (rows["primitive_id"][:, live_records:] == rf.MISS).all()


# ------------------------------------------------------------------ 6: refit
def _move(tris, t):
    """a smooth deformation applied per vertex: shared vertices stay shared (pairs stay pairs)"""
    v = tris.reshape(-1, 3).astype(np.float64)
    out = v.copy()
    out[:, 1] += 0.3 * np.sin(0.7 * v[:, 0] + t) * np.cos(0.5 * v[:, 2])
    out[:, 0] += 0.1 * np.cos(0.3 * v[:, 2] + t)
    return np.ascontiguousarray(out.astype(F).reshape(-1, 9))


@pytest.mark.parametrize("tree", ("bottom_up", "sah_pairs"))
def test_refit_then_rows_follow_the_refitted_bytes(rt, scenes, tree):
    import torch
    tris = rs.scene_tris("grid", scenes)
    inp, root, count = _gpu_tree(rt, tris, tree)
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    moved = _move(tris, 1.0)
    inp.triangles_in.copy_(rt.to_device(moved))
    rt.Refit(inp, root, count, plan)
    torch.cuda.synchronize()
    assert rt.refit_status(plan, inp.num_triangles) == 0
    rays = rf.ray_sets(moved, 91, per_kind=256).astype(rt.RAY)
    walk = Walk(*_download(rt, inp)[:2], root, count, rays)
    assert walk.nonempty > len(rays) // 4
    for k in (1, 4):
        exp = walk.expected(k)
        assert rf.undecided_share(exp, walk.rows) <= rf.CAP
        rows, ctr, status = _first(rt, inp.triangles_out, inp.nodes_out, root, count, rays, k)
        assert status == 0
        _check_rows(rows, walk, k, f"refit {tree}", exp)
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits


# ------------------------------------------------------------------ 7: hipGraph
def test_build_and_query_in_a_hip_graph(rt, scenes):
    import torch
    G = 40
    tris = scenes.grid_mesh(G, 3)
    inp = rt.BuildInput.allocate(tris)
    n, k = 700, 4
    all_rays = rf.ray_sets(tris, 17, per_kind=256).astype(rt.RAY)
    rd = _dev_rays(rt, all_rays[:n]).clone()
    out = torch.empty((n, k, 4), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        rt.RunBottomUpBuild(inp)
        rt.RayFirstHits(inp.triangles_out, inp.nodes_out, 0, 2, rd, k, out, counters=ctr, status=st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()                       # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for batch in (all_rays[300:300 + n], all_rays[200:200 + n]):
        rd.copy_(_dev_rays(rt, batch))
        out.fill_(0)
        ctr.fill_(-1)
        inp.nodes_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(rf.HIT).reshape(n, k)
        got_ctr, got_st = ctr.cpu().numpy().astype(np.uint64), int(st.item())
        eager, eager_ctr, eager_st = _first(rt, inp.triangles_out, inp.nodes_out, 0, 2, batch, k)
        assert got.tobytes() == eager.tobytes() and (got_ctr == eager_ctr).all() and got_st == eager_st == 0
        assert (eager["primitive_id"][:, 0] != rf.MISS).sum() > n // 4 and (eager["primitive_id"][:, 1] != rf.MISS).any()


# ------------------------------------------------------------------ 8: stack overflow
def _comb(rt, L, rng):
    """a comb of L two-slot nodes: node k = (box child k+1, leaf k) in slots (2k, 2k+1), the last node = (leaf L, leaf L-1).
    Every box spans [-50, 50]^3, so a ray that starts inside enters every slot with one front: every node pushes its leaf and
    descends (ties go to the lower slot), and L entries are pending before the first pop.  Triangles: L + 1 large ones around
    the origin at radius 2 .. 8."""
    tris = np.zeros((L + 1, 3, 3), F)
    for k in range(L + 1):
        c = rng.normal(size=3)
        c /= np.linalg.norm(c)
        e1 = np.cross(c, (0.3, 0.5, 0.8))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(c, e1)
        r = 2.0 + k % 7
        tris[k] = (c * r - 2 * e1 - 2 * e2, c * r + 3 * e1 - 2 * e2, c * r - 2 * e1 + 3 * e2)
    nodes = np.zeros(2 * L, rt.NODE)
    for k in range(L):
        last = k == L - 1
        for s in (2 * k, 2 * k + 1):
            nodes["min"][s], nodes["max"][s] = (-50, -50, -50), (50, 50, 50)
        nodes["w12"][2 * k] = 1 << 29 if last else 2 << 29
        nodes["w28"][2 * k] = (2 << 29) | L if last else (1 << 29) | (2 * (k + 1))
        nodes["w12"][2 * k + 1] = 1 << 29
        nodes["w28"][2 * k + 1] = (2 << 29) | k
    leaves = np.zeros(L + 1, rt.TRIANGLE_PAIR)
    leaves["v0"], leaves["v1"], leaves["v2"], leaves["v3"] = tris[:, 0], tris[:, 1], tris[:, 2], tris[:, 2]
    leaves["primitive_id_0"] = np.arange(L + 1)
    return nodes, leaves


def test_stack_overflow_is_flagged_and_rows_are_sorted_subsets(rt):
    L = 80
    rng = np.random.default_rng(5)
    nodes, leaves = _comb(rt, L, rng)
    n = 70                                        # ends inside the second wave
    rays = np.zeros(n, rt.RAY)
    rays["origin"] = rng.uniform(-0.05, 0.05, (n, 3))
    rays["dir"] = rng.normal(size=(n, 3))
    rays["tmin"], rays["tmax"] = 0.0, np.inf
    walk = Walk(nodes, leaves, 0, 2, rays)
    assert sum(len(r) for r in walk.rows) > n
    tri, nod = rt.to_device(leaves), rt.to_device(nodes)
    for k in (1, 8, 32):
        rows, ctr, status = _first(rt, tri, nod, 0, 2, rays, k)
        assert status & rt.RT_RAY_FIRST_STACK_OVERFLOW, f"k {k}: 80 pending entries and no flag"
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits
        found = 0
        for i in range(n):
            is_live = rows["primitive_id"][i] != rf.MISS
            m = int(is_live.sum())
            found += m
            assert not is_live[m:].any() and rows[i, m:].tobytes() == rf.miss_records(k - m).tobytes()
            wbytes = {w.tobytes() for w in walk.rows[i]}
            for j in range(m):
                assert rows[i, j].tobytes() in wbytes, f"k {k}: ray {i}: record {j} is not in the all-hit row"
                assert j == 0 or rf.below(rows[i, j - 1], rows[i, j]), f"k {k}: ray {i}: not strictly ascending"
        assert found > 0
