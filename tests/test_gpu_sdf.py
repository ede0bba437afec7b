"""GPU tests of the signed-distance and occupancy queries (rt_signed_distance / rt_occupancy / rt_generate_grid_points).

1. equals the composition: on every tree kind and closed mesh, sdist bits, primitive_id and the occupancy byte are what
   rt_closest_points + rt_ray_hits_count per direction + the vote give (tests/sdf_ref.py::compose), bit for bit, for votes 1 and
   3, default and caller directions (one axis-aligned) -- on split trees the distance half only;
2. equals the truth: on the stable points of the CPU test, inside is the analytic inside and |sdist| the float64 distance;
3. radius; 4. liveness, batch ends, the empty tree; 5. counters; 6. stack overflow; 7. refit; 8. hipGraph; 9. the lattice."""
import numpy as np
import pytest

import sdf_ref as sr
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

TREES = ("bottom_up", "pairs", "hybrid", "hybrid_pairs", "sah", "sah_pairs", "sah_splits", "sah_pairs_splits")
EXACT_TREES = TREES[:6]
F = np.float32
SENT = 0x5EA7BEEF        # sentinel word of every output buffer
PAD = 64                 # sentinel records behind every output buffer
COMBOS = ((1, None), (3, None), (1, sr.CALLER_DIRS), (3, sr.CALLER_DIRS))


class Result:
    pass


def _dev_queries(rt, q):
    import torch
    return rt.to_device(np.ascontiguousarray(q, rt.POINT_QUERY)).view(torch.float32).view(-1, 4)


def _run(rt, tree, q, votes=3, dirs=None):
    """SignedDistance and Occupancy on the same queries, sentinels behind both outputs -> Result"""
    import torch
    tri, nod, root, count = tree
    n = len(q)
    qd = _dev_queries(rt, q)
    r = Result()
    out = torch.full(((n + PAD) * 2,), SENT, dtype=torch.int32, device="cuda")
    ins = torch.full((n + PAD,), 0x5E, dtype=torch.uint8, device="cuda")
    ctr_s, ctr_o = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2))
    st_s, st_o = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    assert rt.SignedDistance(tri, nod, root, count, qd, out[:2 * n], votes=votes, dirs=dirs, counters=ctr_s, status=st_s) == n
    assert rt.Occupancy(tri, nod, root, count, qd, ins[:n], votes=votes, dirs=dirs, counters=ctr_o, status=st_o) == n
    torch.cuda.synchronize()
    o, b = out.cpu().numpy().view(np.uint32), ins.cpu().numpy()
    assert (o[2 * n:] == SENT).all(), "SignedDistance wrote past out[n]"
    assert (b[n:] == 0x5E).all(), "Occupancy wrote past inside[n]"
    rec = o[:2 * n].view(sr.SDF_HIT)
    r.sdist, r.prim, r.inside = rec["sdist"].copy(), rec["primitive_id"].copy(), b[:n].copy()
    r.ctr_sdf, r.ctr_occ = (c.cpu().numpy().astype(np.uint64) for c in (ctr_s, ctr_o))
    r.st_sdf, r.st_occ = rt.sdf_status(st_s), rt.sdf_status(st_o)
    assert set(np.unique(r.inside).tolist()) <= {0, 1}
    assert r.ctr_sdf[2] == 0 and r.ctr_sdf[3] == 0 and r.ctr_occ[2] == 0 and r.ctr_occ[3] == 0
    return r


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


class World:
    """built trees per (mesh, tree kind), computed once"""
    def __init__(self, rt):
        self.rt, self._g = rt, {}

    def tree(self, name, kind):
        if (name, kind) not in self._g:
            inp, root, count = _gpu_tree(self.rt, np.array(sr.mesh(name)), kind)
            self._g[name, kind] = (inp, (inp.triangles_out, inp.nodes_out, root, count))
        return self._g[name, kind][1]


@pytest.fixture(scope="module")
def world(rt):
    return World(rt)


# ------------------------------------------------------------------ 1: equals the composition
@pytest.mark.parametrize("name", sr.MESHES)
@pytest.mark.parametrize("kind", TREES)
def test_equals_the_composition(world, name, kind):
    rt = world.rt
    tree = world.tree(name, kind)
    q = sr.queries(sr.mixed_points(name, 2048))
    assert len(q) == 2048
    split = "splits" in kind
    for votes, dirs in COMBOS:
        what = f"{name}/{kind}/votes {votes}/{'default' if dirs is None else 'caller'} dirs"
        c = sr.compose(rt, tree, q, votes, dirs)
        r = _run(rt, tree, q, votes, dirs)
        assert c["status"] == 0 and r.st_sdf == 0 and r.st_occ == 0, f"{what}: status {c['status']}, {r.st_sdf}, {r.st_occ}"
        assert (r.prim == c["primitive_id"]).all(), f"{what}: {(r.prim != c['primitive_id']).sum()} primitive ids differ"
        if split:          # the distance half only: the parity of a split tree means nothing
            assert (_bits(np.abs(r.sdist)) == _bits(np.abs(c["sdist"]))).all(), f"{what}: |sdist| differs"
            continue
        bad = _bits(r.sdist) != _bits(c["sdist"])
        assert not bad.any(), f"{what}: {bad.sum()} sdist differ, first at {np.argmax(bad)}: {r.sdist[bad][:3]} vs {c['sdist'][bad][:3]}"
        assert (r.inside == c["inside"]).all(), f"{what}: {(r.inside != c['inside']).sum()} occupancy bytes differ"
        if votes == 3:
            assert c["cast"][2].any(), f"{what}: no query cast its third vote: that path is not tested"
        assert (np.signbit(r.sdist) == ((r.inside == 1) & (r.sdist != 0))).all(), f"{what}: sign and occupancy disagree"
        assert not np.signbit(r.sdist[r.sdist == 0]).any(), f"{what}: a point on the surface must give +0"
        assert (r.ctr_sdf[:2] == c["counters"]).all() and (r.ctr_occ[:2] == c["vote_counters"].sum(0)).all(), \
            f"{what}: counters {r.ctr_sdf[:2]} / {r.ctr_occ[:2]}, the composition {c['counters']} / {c['vote_counters'].sum(0)}"
    assert (r.sdist == 0).sum() >= 16 and 0 < r.inside.sum() < len(q), "the point set is not trivial"


# ------------------------------------------------------------------ 2: equals the truth
@pytest.mark.parametrize("name", sr.MESHES)
def test_equals_the_truth(world, name):
    rt = world.rt
    s = sr.truth_set(name)
    pts, inside, dist = s["points"], s["inside"], s["dist"]
    assert len(pts) >= sr.STABLE_SHARE * s["candidates"]
    assert inside.sum() >= 50 and (~inside).sum() >= 50
    if name == "shell":
        assert sr.in_cavity(pts).sum() >= 50
    M = max(float(np.abs(pts).max()), float(np.abs(sr.mesh(name)).max()))
    tol = 4 * 2.0 ** -23 * M
    q = sr.queries(pts)
    for kind in EXACT_TREES:
        tree = world.tree(name, kind)
        for votes in (1, 3):
            r = _run(rt, tree, q, votes)
            what = f"{name}/{kind}/votes {votes}"
            assert r.st_sdf == 0 and r.st_occ == 0
            err = np.abs(np.abs(r.sdist).astype(np.float64) - dist)
            print(f"{what}: max |sdist| error {err.max():.3e} (bound {tol:.3e}), wrong inside {(r.inside.astype(bool) != inside).sum()}")
            assert (r.inside.astype(bool) == inside).all(), f"{what}: inside wrong on {(r.inside.astype(bool) != inside).sum()} points"
            assert (err <= tol).all(), f"{what}: |sdist| off by {err.max():.3e} > {tol:.3e}"
            assert ((r.sdist < 0) == inside).all(), f"{what}: the sign of sdist does not match inside"
            assert (r.prim < sr.mesh(name).shape[0]).all()


# ------------------------------------------------------------------ 3: radius
@pytest.mark.parametrize("kind", ("bottom_up", "sah_pairs"))
def test_radius(world, kind):
    rt = world.rt
    name = "icosphere"
    s = sr.truth_set(name)
    pts, inside, dist = s["points"][:2048], s["inside"][:2048], s["dist"][:2048]
    tree = world.tree(name, kind)
    radius = 0.1
    q = sr.queries(pts, F(radius * radius))
    r = _run(rt, tree, q)
    full = _run(rt, tree, sr.queries(pts))
    far, near = dist > radius * 1.001, dist < radius * 0.999
    assert far.sum() > 200 and near.sum() > 100 and (far & inside).sum() > 20 and (far & ~inside).sum() > 20
    assert (r.prim[far] == rt.MISS).all()
    assert (r.sdist[far & ~inside] == np.inf).all() and (r.sdist[far & inside] == -np.inf).all()
    assert (r.prim[near] == full.prim[near]).all() and (_bits(r.sdist[near]) == _bits(full.sdist[near])).all()
    assert (r.inside == full.inside).all(), "occupancy ignores dist2_max"
    c = sr.compose(rt, tree, q)
    assert (_bits(r.sdist) == _bits(c["sdist"])).all() and (r.prim == c["primitive_id"]).all()
    assert (r.ctr_sdf[0] < full.ctr_sdf[0]), "a small radius prunes the distance phase"


# ------------------------------------------------------------------ 4: liveness and edges
def test_dead_queries_batch_ends_and_the_empty_tree(world):
    rt = world.rt
    name = "torus"
    tree = world.tree(name, "hybrid_pairs")
    pts = sr.mixed_points(name, 600)
    q = sr.queries(pts)
    assert len(q) == 600
    nan, inf = F(np.nan), F(np.inf)
    dead = q[:8].copy()
    dead["p"][0, 0] = nan
    dead["p"][1, 1] = inf
    dead["p"][2, 2] = -inf
    dead["p"][3] = nan
    dead["dist2_max"][4] = nan
    dead["dist2_max"][5] = -1.0
    dead["dist2_max"][6] = -inf
    dead["p"][7], dead["dist2_max"][7] = 0, -1                 # an off-lattice lane of GenerateGridPoints
    r = _run(rt, tree, dead)
    assert (r.prim == rt.MISS).all() and (_bits(r.sdist) == _bits(F(np.inf))).all() and (r.inside == 0).all()
    assert (r.ctr_sdf == 0).all() and (r.ctr_occ == 0).all() and r.st_sdf == 0
    # dead queries among live ones: the others' records are the batch's own
    full = _run(rt, tree, q)
    mixed = q.copy()
    mixed[5:600:41] = dead[np.arange(len(mixed[5:600:41])) % 8]
    r = _run(rt, tree, mixed)
    d = np.zeros(len(q), bool)
    d[5:600:41] = True
    assert (r.prim[d] == rt.MISS).all() and (r.inside[d] == 0).all() and (r.sdist[d] == np.inf).all()
    assert (_bits(r.sdist[~d]) == _bits(full.sdist[~d])).all() and (r.prim[~d] == full.prim[~d]).all()
    assert (r.inside[~d] == full.inside[~d]).all()
    # a point exactly on a vertex: +0, whatever the votes say
    verts = np.array(sr.mesh(name)).reshape(-1, 3)[:100]
    r = _run(rt, tree, sr.queries(verts))
    assert (_bits(r.sdist) == 0).all(), "a vertex of the mesh must give sdist = +0"
    # batch ends (sentinels: checked inside _run)
    for n in (1, 63, 64, 65, 257):
        r = _run(rt, tree, q[:n])
        assert (_bits(r.sdist) == _bits(full.sdist[:n])).all() and (r.prim == full.prim[:n]).all(), f"batch of {n}"
        assert (r.inside == full.inside[:n]).all(), f"batch of {n}"
    # a NaN caller direction: that vote is dead (count 0, even)
    dirs = sr.CALLER_DIRS.copy()
    dirs[1, 2] = nan
    r = _run(rt, tree, q, 3, dirs)
    c = sr.compose(rt, tree, q, 3, dirs)
    assert (r.inside == c["inside"]).all() and (_bits(r.sdist) == _bits(c["sdist"])).all() and (c["counts"][1] == 0).all()
    # an empty tree (count = 0): every query a miss and outside, nothing counted
    tri, nod, _, _ = tree
    r = _run(rt, (tri, nod, 0, 0), q)
    assert (r.prim == rt.MISS).all() and (_bits(r.sdist) == _bits(F(np.inf))).all() and (r.inside == 0).all()
    assert (r.ctr_sdf == 0).all() and (r.ctr_occ == 0).all() and r.st_sdf == 0 and r.st_occ == 0


# ------------------------------------------------------------------ 5: counters
@pytest.mark.parametrize("kind", ("pairs", "sah"))
def test_counters(world, kind):
    import torch
    rt = world.rt
    name = "torus"
    tree = world.tree(name, kind)
    # points near the surface, where single rays graze edges: some first votes disagree
    q = sr.queries(sr.mixed_points(name, 4096, seed=11))
    assert len(q) == 4096
    for dirs in (None, sr.CALLER_DIRS):
        # votes = 1: exactly rt_ray_hits_count's counters for the same rays (entered slots and visited leaves do not depend on
        # the visiting order)
        c1 = sr.compose(rt, tree, q, 1, dirs)
        r1 = _run(rt, tree, q, 1, dirs)
        assert (r1.ctr_occ[:2] == c1["vote_counters"][0]).all(), f"{r1.ctr_occ[:2]} vs {c1['vote_counters'][0]}"
        # votes = 3: the sum over the traversals the early-out rule says were run
        c3 = sr.compose(rt, tree, q, 3, dirs)
        r3 = _run(rt, tree, q, 3, dirs)
        third = c3["cast"][2]
        assert (third == ((c3["counts"][0] % 2) != (c3["counts"][1] % 2))).all()
        assert third.sum() > 0, "no query cast its third vote: the early-out path is not tested"
        assert (r3.ctr_occ[:2] == c3["vote_counters"].sum(0)).all(), f"{r3.ctr_occ[:2]} vs {c3['vote_counters'].sum(0)}"
        assert (r3.ctr_sdf[:2] == c3["counters"]).all()
        assert (r3.ctr_sdf[:2] - r3.ctr_occ[:2] == r1.ctr_sdf[:2] - r1.ctr_occ[:2]).all(), "the distance phase counts the same"
        assert (c3["vote_counters"][0] == c1["vote_counters"][0]).all()
        print(f"{name}/{kind}: third vote cast for {int(third.sum())} of {len(q)} points; counters {r3.ctr_sdf[:2]}")
        # two runs agree
        again = _run(rt, tree, q, 3, dirs)
        assert (again.ctr_sdf == r3.ctr_sdf).all() and (again.ctr_occ == r3.ctr_occ).all()
        assert (_bits(again.sdist) == _bits(r3.sdist)).all() and (again.inside == r3.inside).all()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6: stack overflow
def _comb(rt, L, rng):
    """a comb of L two-slot nodes: node k = (box child k+1, leaf k) in slots (2k, 2k+1), the last node = (leaf L, leaf L-1).
    Every box spans [-50, 50]^3, so a ray that starts inside enters every slot: every node pushes its leaf and descends, and
    L entries are pending before the first pop.  Triangles: L + 1 large ones around the origin at radius 2 .. 8.
    (tests/test_gpu_ray_hits.py's comb, restated.)"""
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


def test_stack_overflow_is_flagged(rt):
    rng = np.random.default_rng(5)
    n = 70                                        # ends inside the second wave
    pts = rng.uniform(-0.05, 0.05, (n, 3)).astype(F)
    q = sr.queries(pts)
    # deep: 80 pending entries > 64 in every traversal
    L = 80
    nodes, leaves = _comb(rt, L, rng)
    tree = (rt.to_device(leaves), rt.to_device(nodes), 0, 2)
    for votes in (1, 3):
        r = _run(rt, tree, q, votes)              # (the call returns)
        assert r.st_sdf & rt.RT_SDF_STACK_OVERFLOW and r.st_occ & rt.RT_SDF_STACK_OVERFLOW
        assert ((r.prim <= L) | (r.prim == rt.MISS)).all(), "every primitive_id is a real triangle or RT_MISS"
        assert np.isfinite(r.sdist[r.prim != rt.MISS]).all()
    # shallow: nothing is dropped, flag 0, the composition's result
    L = 40
    nodes, leaves = _comb(rt, L, rng)
    tree = (rt.to_device(leaves), rt.to_device(nodes), 0, 2)
    for votes in (1, 3):
        r = _run(rt, tree, q, votes)
        c = sr.compose(rt, tree, q, votes)
        assert r.st_sdf == 0 and r.st_occ == 0 and c["status"] == 0
        assert (_bits(r.sdist) == _bits(c["sdist"])).all() and (r.prim == c["primitive_id"]).all()
        assert (r.inside == c["inside"]).all() and (r.prim <= L).all()
        assert (r.ctr_sdf[:2] == c["counters"]).all()


def test_overflowed_distance_equals_closest_points(rt):
    """(|sdist|, primitive_id) is rt_closest_points's record also where pushes were dropped: the deep comb (80 pending entries
    against 64 slots), where every pass of both calls drops pushes and the record depends on which ones.  The sign and the
    occupancy byte are not compared: the parity rays overflow too, and their counts are lower bounds."""
    import torch
    rng = np.random.default_rng(5)
    n = 70                                        # ends inside the second wave
    q = sr.queries(rng.uniform(-0.05, 0.05, (n, 3)).astype(F))
    L = 80
    nodes, leaves = _comb(rt, L, rng)
    tree = (rt.to_device(leaves), rt.to_device(nodes), 0, 2)
    hits = torch.full((n, 4), np.nan, dtype=torch.float32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    rt.ClosestPoints(*tree, _dev_queries(rt, q), hits, status=st)
    h = hits.cpu().numpy().view(rt.POINT_HIT).reshape(-1)
    cp_over = bool(rt.point_status(st) & rt.RT_POINT_STACK_OVERFLOW)
    cp_miss = h["primitive_id"] == rt.MISS
    assert cp_over, "the comb is meant to overflow the distance traversal"
    assert (~cp_miss).any() and (h["primitive_id"][~cp_miss] <= L).all()
    with np.errstate(invalid="ignore"):
        cp_dist = np.where(cp_miss, F(np.inf), np.sqrt(h["dist2"], dtype=F)).astype(F)
    for votes in (1, 3):
        r = _run(rt, tree, q, votes)
        assert (r.prim == h["primitive_id"]).all()
        assert ((r.prim == rt.MISS) == cp_miss).all()
        assert (_bits(np.abs(r.sdist)) == _bits(cp_dist)).all()
        assert bool(r.st_sdf & rt.RT_SDF_STACK_OVERFLOW) == cp_over


# ------------------------------------------------------------------ 7: refit
def _scale_shear(tris):
    """per vertex, from its float32 bits alone: shared vertices stay shared, the mesh stays closed"""
    v = np.asarray(tris, F).reshape(-1, 3).astype(np.float64)
    A = np.array([[1.3, 0.25, 0.0], [0.0, 0.8, -0.15], [0.1, 0.0, 1.1]])
    return np.ascontiguousarray((v @ A.T + np.array((0.05, 0.0, -0.1))).astype(F).reshape(-1, 9))


@pytest.mark.parametrize("kind", ("bottom_up", "sah"))
def test_refit_then_signed_distance(rt, kind):
    import torch
    tris = np.array(sr.mesh("icosphere"))
    inp, root, count = _gpu_tree(rt, tris, kind)
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    moved = _scale_shear(tris)
    inp.triangles_in.copy_(rt.to_device(moved))
    rt.Refit(inp, root, count, plan)
    torch.cuda.synchronize()
    assert rt.refit_status(plan, inp.num_triangles) == 0
    tree = (inp.triangles_out, inp.nodes_out, root, count)
    # the truth on the moved mesh, chosen by the reference alone
    rng = np.random.default_rng(77)
    V = moved.reshape(-1, 3).astype(np.float64)
    c, half = (V.min(0) + V.max(0)) / 2, (V.max(0) - V.min(0)) / 2
    cand = rng.uniform(c - 1.5 * half, c + 1.5 * half, (1500, 3)).astype(F)
    b = sr.brute_f64(moved, cand, sr.DEFAULT_DIRS)
    keep = (b["dist"] >= sr.NEAR) & b["stable"]
    assert keep.sum() >= sr.STABLE_SHARE * len(cand)
    pts, dist = cand[keep], b["dist"][keep]
    inside = np.abs(sr.winding_f64(moved, pts)) > 0.5
    assert inside.sum() >= 50 and (~inside).sum() >= 50
    q = sr.queries(pts)
    r = _run(rt, tree, q)
    cmp = sr.compose(rt, tree, q)
    assert r.st_sdf == 0 and cmp["status"] == 0
    assert (_bits(r.sdist) == _bits(cmp["sdist"])).all() and (r.prim == cmp["primitive_id"]).all()
    assert (r.inside == cmp["inside"]).all()
    tol = 4 * 2.0 ** -23 * max(float(np.abs(pts).max()), float(np.abs(moved).max()))
    err = np.abs(np.abs(r.sdist).astype(np.float64) - dist)
    print(f"refit {kind}: max |sdist| error {err.max():.3e} (bound {tol:.3e})")
    assert (r.inside.astype(bool) == inside).all() and ((r.sdist < 0) == inside).all()
    assert (err <= tol).all(), f"refit {kind}: |sdist| off by {err.max():.3e} > {tol:.3e}"


# ------------------------------------------------------------------ 8: hipGraph
def test_grid_sdf_and_occupancy_in_a_hip_graph(world):
    import torch
    rt = world.rt
    tree = world.tree("torus", "sah_pairs")
    tri, nod, root, count = tree
    dims, origin, spacing = (13, 9, 6), (-1.6, -1.5, -0.9), (0.27, 0.33, 0.35)
    n = rt.GridPointCount(dims, bricks=True)
    qd = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    ins = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        rt.GenerateGridPoints(origin, spacing, dims, qd, bricks=True)
        rt.SignedDistance(tri, nod, root, count, qd, out, counters=ctr, status=st)
        rt.Occupancy(tri, nod, root, count, qd, ins, counters=ctr, status=st)

    # the eager result
    one_frame()
    torch.cuda.synchronize()
    eager = (qd.cpu().numpy().tobytes(), out.cpu().numpy().tobytes(), ins.cpu().numpy().tobytes(), ctr.cpu().numpy().tolist())
    assert eager[0] == sr.lattice(origin, spacing, dims, bricks=True).tobytes()
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
        # (origin, spacing, dims and the directions are host arguments baked in at capture: both replays give the eager result)
        qd.fill_(7.0)
        out.fill_(7.0)
        ins.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        got = (qd.cpu().numpy().tobytes(), out.cpu().numpy().tobytes(), ins.cpu().numpy().tobytes(), ctr.cpu().numpy().tolist())
        assert got == eager and int(st.item()) == 0
    assert 0 < int(ins.sum().item()) < n


# ------------------------------------------------------------------ 9: the lattice
def test_grid_points_equal_the_lattice(rt):
    import torch
    origin, spacing = (-1.0, 0.5, 0.25), (0.1, 0.3, 0.7)
    for dims in ((1, 1, 1), (4, 4, 4), (5, 3, 9), (17, 1, 2)):
        for bricks in (False, True):
            n = rt.GridPointCount(dims, bricks)
            buf = torch.full(((n + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
            assert rt.GenerateGridPoints(origin, spacing, dims, buf[:4 * n], dist2_max=2.5, bricks=bricks) == n
            torch.cuda.synchronize()
            b = buf.cpu().numpy().view(np.uint32)
            assert (b[4 * n:] == SENT).all(), "GenerateGridPoints wrote past its records"
            ref = sr.lattice(origin, spacing, dims, bricks, dist2_max=2.5)
            assert len(ref) == n and b[:4 * n].tobytes() == ref.tobytes(), f"dims {dims}, bricks {bricks}"
            if bricks:
                off = ref["dist2_max"] == -1
                assert off.sum() == n - dims[0] * dims[1] * dims[2]
    # a lattice with a zero dimension runs nothing
    buf = torch.full((64,), SENT, dtype=torch.int32, device="cuda")
    assert rt.GenerateGridPoints(origin, spacing, (3, 0, 2), buf, bricks=True) == 0
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


def test_brick_lattice_occupancy_equals_row_major(world):
    import torch
    rt = world.rt
    tri, nod, root, count = world.tree("torus", "bottom_up")
    dims = (20, 20, 20)
    V = np.array(sr.mesh("torus")).reshape(-1, 3)
    lo, hi = V.min(0) - 0.1, V.max(0) + 0.1
    origin, spacing = lo, (hi - lo) / 19
    res = {}
    for bricks in (False, True):
        n = rt.GridPointCount(dims, bricks)
        qd = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        ins = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        rt.GenerateGridPoints(origin, spacing, dims, qd, bricks=bricks)
        rt.Occupancy(tri, nod, root, count, qd, ins, status=st)
        torch.cuda.synchronize()
        assert rt.sdf_status(st) == 0
        res[bricks] = ins.cpu().numpy()
    idx = sr.brick_index(dims)
    assert (res[True][idx] == res[False]).all(), "the brick lattice gives other bits than the row-major one"
    dead = np.ones(len(res[True]), bool)
    dead[idx] = False
    assert (res[True][dead] == 0).all() and 100 < res[False].sum() < 8000 - 100
    # against the winding number, on the stable lattice points away from the surface
    q = sr.lattice(origin, spacing, dims)
    b = sr.brute_f64(sr.mesh("torus"), q["p"], sr.DEFAULT_DIRS)
    ok = (b["dist"] >= sr.NEAR) & b["stable"]
    assert ok.sum() >= sr.STABLE_SHARE * len(q)
    assert (res[False][ok].astype(bool) == sr.analytic_inside("torus", q["p"][ok])).all()
