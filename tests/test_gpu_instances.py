"""GPU tests of instancing (rt_prepare_instances + a TLAS built over the proxies + rt_intersect_rays_instanced).

1. prepare: proxies bit-exact against tests/instance_ref.py's float32 restatement, world_to_object within a few ulp of the
   float64 inverse, bad-BLAS / singular / NaN-matrix instances flagged and never hit;
2. the TLAS over the proxies equals the oracle's tree over the same proxies (bottom-up, hybrid, sah);
3. one identity instance of each of the 8 BLAS kinds on the five scenes of test_gpu_ray_queries: hit records bit-identical to
   rt_intersect_rays on the BLAS, instance 0 on every hit, the same triangle tests;
4. exact composition: 7 instances (rotation, non-uniform scale, mirror, shear, translation, two overlapping copies, a second
   BLAS of another kind): where float64 shows the answer is unique, every record equals the minimum-t rt_intersect_rays result
   over the instances on the float32-transformed rays, bit for bit;
5. float64 brute force over the flattened world triangles (shade_ref.cast): hit / miss, instance, primitive, t, (u, v);
   any-hit hits where closest-hit hits with a genuine hit in [tmin, tmax]; tmax = nextafter(t, 0) misses;
6. dynamic scene: moved instances (prepare + TLAS rebuild) and a refitted, deformed BLAS (rt_refit + prepare) against float64;
7. edges: 1, 2, 3 instances; degenerate and NaN rays; records past num_rays; the pair-prefetch instantiation;
8. prepare + TLAS build + query captured in one HIP graph, replayed after the instance buffer is rewritten in place."""
import collections

import numpy as np
import pytest

import instance_ref as ir
import shade_ref
import test_gpu_ray_queries as rq

pytestmark = pytest.mark.gpu

TLAS_KINDS = ("bottom_up", "hybrid", "sah")
BIG = rq.BIG
RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
Tree = collections.namedtuple("Tree", "triangles_out nodes_out")   # what rq._query reads of a BuildInput


# ------------------------------------------------------------------ scene plumbing
def _blas(world, name, tree):
    """(triangles, table entry (tris, nodes, root, count), root box) of a BLAS from the ray-query tests' world"""
    rt = world.rt
    tris = world.scene(name)[0]
    inp, root, count = world.gpu(name, tree)
    nodes = rt.to_host(inp.nodes_out, rt.NODE)
    return tris, (inp.triangles_out, inp.nodes_out, root, count), ir.root_box(nodes, root, count)


class Instanced:
    """device buffers of one instanced scene: BLAS table, instances, proxies, records, status, TLAS"""

    def __init__(self, rt, blas_entries, instances, tlas="bottom_up"):
        import torch
        self.rt, self.kind = rt, tlas
        self.n = instances.size
        self.entries = list(blas_entries)
        self.table = rt.accel_table(self.entries)
        self.instances = rt.to_device(np.ascontiguousarray(instances))
        self.tlas = rt.BuildInput.allocate(np.zeros((max(self.n, 1), 9), np.float32), sah=tlas == "sah")
        self.tlas.num_triangles = self.n
        self.records = torch.zeros(max(self.n, 1) * 64, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(4, dtype=torch.uint8, device="cuda")

    def prepare(self, stream=None):
        self.rt.PrepareInstances(self.instances, self.n, self.table, len(self.entries), self.tlas.triangles_in, self.records,
                                 self.status, stream=stream)

    def build(self, stream=None):
        rt = self.rt
        if self.kind == "sah":
            rt.RunSahBuild(self.tlas, rt.Arguments(build_type=rt.kSAH), stream=stream)
        else:
            hyb = self.kind == "hybrid"
            rt.RunBottomUpBuild(self.tlas, rt.Arguments(build_type=rt.kHybrid if hyb else rt.kBottomUp), hybrid=hyb,
                                stream=stream)

    @property
    def root(self):
        if self.kind == "sah":
            return 0, 1
        return (2 * max(self.n, 1) + 1 if self.kind == "hybrid" else 0), 2

    def frame(self, stream=None):
        self.prepare(stream)
        self.build(stream)

    def query(self, rays, hits, ids, any_hit=False, num_primitives=0, counters=None, stream=None):
        root, count = self.root
        self.rt.IntersectRaysInstanced(self.tlas.triangles_out, self.tlas.nodes_out, root, count, self.records, self.n,
                                       self.table, len(self.entries), rays, hits, ids, any_hit=any_hit,
                                       num_primitives=num_primitives, counters=counters, stream=stream)

    def run(self, rays, any_hit=False, num_primitives=0, counters=False):
        """numpy RAY array -> (HIT array, instance ids, counters)"""
        import torch
        rt = self.rt
        d = rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)
        n = d.shape[0]
        hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        ids = torch.empty(n, dtype=torch.int32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda") if counters else None
        self.query(d, hits, ids, any_hit=any_hit, num_primitives=num_primitives, counters=ctr)
        torch.cuda.synchronize()
        return (hits.cpu().numpy().view(rt.HIT).reshape(-1), ids.cpu().numpy().view(np.uint32),
                ctr.cpu().numpy().astype(np.uint64) if counters else None)

    def host_records(self):
        return self.rt.to_host(self.records, self.rt.INSTANCE_RECORD, self.n)

    def host_proxies(self):
        return self.rt.to_host(self.tlas.triangles_in, np.float32, 9 * self.n).reshape(-1, 9)


def _affine(R, t=(0, 0, 0)):
    return np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)])


def _world_rays(world_tris, n, seed):
    """rays from outside the scene box at interior points (as rq._ray_sets 'outside'), plus random [tmin, tmax] windows"""
    rng = np.random.default_rng(seed)
    P = world_tris.reshape(-1, 3)
    lo, hi = P.min(axis=0), P.max(axis=0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = c + u * ext * 1.2
    d = (lo + rng.random((n, 3)) * (hi - lo) - o) * rng.uniform(0.3, 2.0, size=(n, 1))
    r = np.zeros(n, RAY)
    r["origin"], r["dir"], r["tmin"], r["tmax"] = o, d, 0.0, np.inf
    w = r.copy()
    a, b = rng.random(n) * 1.2, rng.random(n) * 1.2
    w["tmin"], w["tmax"] = np.minimum(a, b), np.maximum(a, b)
    return np.concatenate([r, w])


def _f64_world(world_tris, rays):
    return shade_ref.cast(rays["origin"].astype(np.float64), rays["dir"].astype(np.float64), world_tris,
                          rays["tmin"].astype(np.float64), rays["tmax"].astype(np.float64))


def _window_ok(world_tris, rays, ref):
    """the hit / miss decision does not move when [tmin, tmax] is loosened or tightened by 1e-4 (relative)"""
    lo, hi = rays["tmin"].astype(np.float64), rays["tmax"].astype(np.float64)
    o, d = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    loose = shade_ref.cast(o, d, world_tris, lo * (1 - 1e-4) - 1e-9, hi * (1 + 1e-4))
    tight = shade_ref.cast(o, d, world_tris, lo * (1 + 1e-4) + 1e-9, hi * (1 - 1e-4))
    return (loose["hit"] == tight["hit"]) & (loose["tri"] == tight["tri"]) & (loose["tri"] == ref["tri"])


def _check_world(sc, world_tris, inst_of, prim_of, rays, what, bound=0.02):
    """closest hit against float64 brute force over the flattened world triangles; any-hit; tmax honoured"""
    hits, ids, _ = sc.run(rays)
    ref = _f64_world(world_tris, rays)
    stable = ref["stable"] & _window_ok(world_tris, rays, ref)
    assert 1 - stable.mean() <= bound, f"{what}: unstable fraction {1 - stable.mean():.4f}"
    got = hits["primitive_id"] != 0xFFFFFFFF
    assert ((ids != 0xFFFFFFFF) == got).all(), f"{what}: instance id and primitive id disagree on hit / miss"
    bad = stable & (got != ref["hit"])
    assert not bad.any(), f"{what}: hit / miss differs on {bad.sum()} stable rays (first {np.nonzero(bad)[0][:5]})"
    m = stable & ref["hit"]
    k = ref["tri"][m]
    assert (ids[m] == inst_of[k]).all(), f"{what}: instance"
    assert (hits["primitive_id"][m] == prim_of[k]).all(), f"{what}: primitive"
    t_ref = ref["t"][m]
    assert (np.abs(hits["t"][m] - t_ref) <= 1e-5 * np.maximum(1, t_ref)).all(), f"{what}: t"
    assert (np.abs(hits["u"][m] - ref["u"][m]) <= 2e-4).all() and (np.abs(hits["v"][m] - ref["v"][m]) <= 2e-4).all(), \
        f"{what}: (u, v)"
    assert (hits["t"][~got] == np.inf).all()
    assert got.sum() > 50, f"{what}: too few hits to mean anything"
    # any-hit: hits exactly where closest-hit hits, a genuine hit inside [tmin, tmax], never closer than the closest
    a, aid, _ = sc.run(rays, any_hit=True)
    ah = a["primitive_id"] != 0xFFFFFFFF
    assert (ah == got).all(), f"{what}: any-hit hits on {ah.sum()} rays, closest-hit on {got.sum()}"
    assert ((a["t"][ah] >= rays["tmin"][ah]) & (a["t"][ah] <= rays["tmax"][ah]) & (a["t"][ah] >= hits["t"][ah])).all()
    flat = {(int(i), int(p)): j for j, (i, p) in enumerate(zip(inst_of, prim_of))}
    idx = np.array([flat[(int(i), int(p))] for i, p in zip(aid[ah], a["primitive_id"][ah])], np.int64)
    V = world_tris.reshape(-1, 3, 3)[idx]
    o, d = rays["origin"][ah].astype(np.float64), rays["dir"][ah].astype(np.float64)
    e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    hv = np.cross(d, e2)
    f = 1.0 / (e1 * hv).sum(axis=1)
    s = o - V[:, 0]
    u, q = f * (s * hv).sum(axis=1), np.cross(s, e1)
    v, t = f * (d * q).sum(axis=1), f * (e2 * q).sum(axis=1)
    tol = 1e-3
    assert ((u >= -tol) & (v >= -tol) & (u + v <= 1 + tol)).all(), f"{what}: any-hit record off its triangle"
    assert (np.abs(t - a["t"][ah]) <= 1e-4 * np.maximum(1, np.abs(t))).all(), f"{what}: any-hit t"
    # tmax honoured
    sel = got & (hits["t"] > rays["tmin"])
    r2 = rays[sel].copy()
    r2["tmax"] = np.nextafter(hits["t"][sel], np.float32(0))
    again, aids, _ = sc.run(r2)
    assert (again["primitive_id"] == 0xFFFFFFFF).all() and (aids == 0xFFFFFFFF).all(), f"{what}: hits beyond tmax"
    print(f"{what}: {rays.size} rays, unstable {100 * (1 - stable.mean()):.2f} %, hits {got.mean():.2f}")
    return hits, ids


@pytest.fixture(scope="module")
def world(rt, scenes, ora):
    return rq.World(rt, scenes, ora)


_SECOND = {}


def _second_blas(world):
    """another height field, built as an SAH tree with pairs (its triangles pair up): cached per module"""
    if "b" not in _SECOND:
        tris = world.scenes.grid_mesh(16, 9)
        inp, root, count = rq._gpu_tree(world.rt, tris, "sah_pairs")
        nodes = world.rt.to_host(inp.nodes_out, world.rt.NODE)
        _SECOND["b"] = tris, (inp.triangles_out, inp.nodes_out, root, count), ir.root_box(nodes, root, count), inp
    return _SECOND["b"][:3]


def _composition(world):
    """7 instances of two BLASes: grid_mesh(24) (LBVH) and grid_mesh(16) (SAH with pairs)"""
    ga, ea, ba = _blas(world, "grid", "bottom_up")
    gb, eb, bb = _second_blas(world)
    ext = float(np.ptp(ga.reshape(-1, 3), axis=0).max())
    R = ir.rotation(0.3, -0.5, 0.9)
    mats = [
        _affine(R, (0, 0, 0)),                                          # rotation
        _affine(np.diag([1.5, 0.6, 2.0]), (1.3 * ext, 0, 0)),           # non-uniform scale
        _affine(np.diag([-1.0, 1.0, 1.0]), (0, 1.3 * ext, 0)),          # mirror (negative determinant)
        _affine([[1, 0.4, 0], [0, 1, 0.3], [0.2, 0, 1]], (0, 0, 1.3 * ext)),   # shear
        _affine(np.eye(3), (-1.2 * ext, 0.5 * ext, 0.2 * ext)),         # translation
        _affine(R, (0.07 * ext, 0.05 * ext, -0.03 * ext)),              # overlaps instance 0
        _affine(ir.rotation(0.1, 0.2, 0.3) * 1.2, (-0.3 * ext, -1.2 * ext, 0)),   # the second BLAS
    ]
    inst = ir.instance_array(mats, [0, 0, 0, 0, 0, 0, 1])
    return [ga, gb], [ea, eb], [ba, bb], inst


# ------------------------------------------------------------------ 1: prepare
def test_prepare_bit_exact_and_flags(world):
    rt = world.rt
    blas_tris, entries, boxes, inst = _composition(world)
    bad = ir.instance_array([np.eye(3, 4), np.zeros((3, 4)), np.full((3, 4), np.nan), np.eye(3, 4)], [5, 0, 0, 2])
    allinst = np.concatenate([inst, bad])
    # table entry 2: an empty tree (count 0) -- a bad BLAS
    entries = entries + [(entries[0][0], entries[0][1], 0, 0)]
    boxes = boxes + [None]
    for kind in TLAS_KINDS:
        sc = Instanced(rt, entries, allinst, kind)
        sc.frame()
        assert rt.instance_status(sc.status) == rt.RT_INSTANCE_BAD_BLAS | rt.RT_INSTANCE_SINGULAR
        prox, inv, flags = ir.prepare(allinst, boxes)
        got = sc.host_proxies()
        assert got.tobytes() == prox.tobytes(), f"{kind}: proxies differ from the float32 restatement"
        rec = sc.host_records()
        assert (rec["flags"] == flags).all() and (rec["blas"] == allinst["blas"]).all() and (rec["spare"] == 0).all()
        assert flags.tolist()[-4:] == [1, 2, 2, 1]
        ok = flags == 0
        W = rec["world_to_object"][ok].astype(np.float64)
        # ulp of each entry, floored at 1e-8 of its row's largest entry (a zero of the exact inverse comes out as ~1e-17)
        scale = np.maximum(np.abs(inv[ok]), 1e-8 * np.abs(inv[ok]).max(axis=2, keepdims=True)).astype(np.float32)
        err = np.abs(W - inv[ok]) / np.spacing(scale).astype(np.float64)
        assert err.max() <= 4, f"{kind}: world_to_object {err.max():.1f} ulp from the float64 inverse"
        # flagged instances are never hit, even by rays aimed straight at the geometry they would place
        wt, inst_of, prim_of = ir.world_triangles(blas_tris, inst)
        rays = _world_rays(wt, 600, seed=7)
        hits, ids, _ = sc.run(rays)
        assert (ids[ids != 0xFFFFFFFF] < inst.size).all(), f"{kind}: a flagged instance was hit"
        assert (ids != 0xFFFFFFFF).sum() > 50


# ------------------------------------------------------------------ 2: the TLAS over the proxies
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_tlas_over_proxies_matches_oracle(world, ora, kind):
    rt = world.rt
    _, entries, _, inst = _composition(world)
    rng = np.random.default_rng(3)
    mats = [_affine(ir.rotation(*rng.uniform(-1, 1, 3)), rng.uniform(-200, 200, 3)) for _ in range(65)]
    many = ir.instance_array(mats, rng.integers(0, 2, 65))
    for instances in (inst, many):
        sc = Instanced(rt, entries, instances, kind)
        sc.tlas.nodes_out.fill_(0)
        sc.frame()
        prox = sc.host_proxies()
        o = {"bottom_up": ora.build_bvh, "hybrid": ora.build_hybrid, "sah": ora.build_sah}[kind](prox)
        got = rt.to_host(sc.tlas.nodes_out, rt.NODE, o["nodes"].shape[0])
        assert got.tobytes() == o["nodes"].tobytes(), f"{kind}: TLAS nodes differ from the oracle's over the same proxies"
        leaves = rt.to_host(sc.tlas.triangles_out, rt.TRIANGLE_PAIR, o["leaves"].shape[0])
        for f in ("v0", "v1", "v2", "v3", "primitive_id_0"):
            assert (leaves[f] == o["leaves"][f]).all(), f"{kind}: TLAS leaf records ({f})"
        assert sorted(leaves["primitive_id_0"].tolist()) == list(range(instances.size))


# ------------------------------------------------------------------ 3: identity instance == rt_intersect_rays
def _positive_zeros(rays):
    r = rays.copy()
    for f in ("origin", "dir"):
        r[f] = r[f] + np.float32(0)      # -0 + +0 = +0: the identity transform then reproduces every component
    return r


@pytest.mark.parametrize("name", rq.SCENES)
@pytest.mark.parametrize("tree", rq.TREES)
def test_identity_instance_equals_intersect_rays(world, name, tree):
    rt = world.rt
    tris, cam = world.scene(name)
    _, entry, _ = _blas(world, name, tree)
    sets = rq._ray_sets(tris, seed=31)
    cam_rays = rq._camera_rays(rt, cam, rq.W, rq.H, 1, True).cpu().numpy().view(rt.RAY).reshape(-1)
    rays = _positive_zeros(np.concatenate([sets["outside"].astype(rt.RAY), sets["window"].astype(rt.RAY), cam_rays]))
    exp, ec = rq._query(rt, world.gpu(name, tree), rays, counters=True)
    for kind in TLAS_KINDS:
        sc = Instanced(rt, [entry], ir.instance_array([np.eye(3, 4)], [0]), kind)
        sc.frame()
        assert rt.instance_status(sc.status) == 0
        assert (sc.host_records()["world_to_object"] == np.eye(3, 4, dtype=np.float32)).all()
        hits, ids, c = sc.run(rays, counters=True)
        assert hits.tobytes() == exp.tobytes(), f"{name}/{tree} TLAS {kind}: records differ from rt_intersect_rays"
        assert ((ids == 0) == (exp["primitive_id"] != 0xFFFFFFFF)).all() and ((ids == 0) | (ids == 0xFFFFFFFF)).all()
        assert c[1] == ec[1], f"{name}/{tree} TLAS {kind}: triangle tests {c[1]} vs {ec[1]}"
        # (box tests: the TLAS's are added, but a ray that misses the single proxy box costs one test where the BLAS's own
        # root pair costs two -- the totals are not ordered)
        assert c[0] > 0
        a, aid, _ = sc.run(rays, any_hit=True)
        ea, _ = rq._query(rt, world.gpu(name, tree), rays, any_hit=True)
        assert a.tobytes() == ea.tobytes(), f"{name}/{tree} TLAS {kind}: any-hit records differ"


# ------------------------------------------------------------------ 4: exact composition
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_exact_composition(world, kind):
    rt = world.rt
    blas_tris, entries, _, inst = _composition(world)
    sc = Instanced(rt, entries, inst, kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    wt, inst_of, prim_of = ir.world_triangles(blas_tris, inst)
    rays = _world_rays(wt, 1500, seed=11)
    hits, ids, _ = sc.run(rays)
    rec = sc.host_records()
    # the minimum-t result of rt_intersect_rays over every instance, on the float32 object rays of the records
    best = np.zeros(rays.size, rt.HIT)
    best["t"], best["primitive_id"] = np.inf, 0xFFFFFFFF
    best_id = np.full(rays.size, 0xFFFFFFFF, np.uint32)
    for k in range(inst.size):
        e = entries[int(inst["blas"][k])]
        h, _ = rq._query(rt, (Tree(e[0], e[1]), e[2], e[3]), ir.object_rays(rays.astype(rt.RAY), rec["world_to_object"][k]))
        take = (h["primitive_id"] != 0xFFFFFFFF) & (h["t"] < best["t"])
        best[take], best_id[take] = h[take], k
    ref = _f64_world(wt, rays)
    unique = ref["stable"] & _window_ok(wt, rays, ref) & np.where(ref["hit"], best_id == inst_of[np.maximum(ref["tri"], 0)], True)
    assert unique.mean() > 0.97, f"unique fraction {unique.mean():.3f}"
    assert hits[unique].tobytes() == best[unique].tobytes(), \
        f"{kind}: {np.sum(hits[unique] != best[unique])} records differ from the per-instance minimum"
    assert (ids[unique] == best_id[unique]).all()
    assert (best_id[unique] != 0xFFFFFFFF).sum() > 200 and len(set(best_id[unique].tolist()) - {0xFFFFFFFF}) >= 5


# ------------------------------------------------------------------ 5: float64 brute force
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_against_float64(world, kind):
    rt = world.rt
    blas_tris, entries, _, inst = _composition(world)
    sc = Instanced(rt, entries, inst, kind)
    sc.frame()
    wt, inst_of, prim_of = ir.world_triangles(blas_tris, inst)
    _check_world(sc, wt, inst_of, prim_of, _world_rays(wt, 1500, seed=13), f"composition TLAS {kind}")


# ------------------------------------------------------------------ 6: dynamic scene
def test_dynamic_scene(world):
    import torch
    rt = world.rt
    blas_tris, entries, _, inst = _composition(world)
    sc = Instanced(rt, entries, inst, "bottom_up")
    sc.frame()
    # rigid motion: every instance moves; prepare + TLAS rebuild
    rng = np.random.default_rng(5)
    moved = inst.copy()
    ext = float(np.ptp(blas_tris[0].reshape(-1, 3), axis=0).max())
    for k in range(inst.size):
        M = moved["object_to_world"][k].astype(np.float64)
        R = ir.rotation(*rng.uniform(-0.4, 0.4, 3))
        moved["object_to_world"][k] = np.hstack([R @ M[:, :3], (R @ M[:, 3] + rng.uniform(-0.3, 0.3, 3) * ext)[:, None]])
    sc.instances.copy_(rt.to_device(moved))
    sc.frame()
    wt, inst_of, prim_of = ir.world_triangles(blas_tris, moved)
    _check_world(sc, wt, inst_of, prim_of, _world_rays(wt, 1200, seed=17), "moved instances")
    # deformation: a private copy of the grid BLAS refitted to deformed vertices, then prepare again (its box changed)
    g = rq._gpu_tree(rt, blas_tris[0], "bottom_up")
    inp, root, count = g
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    P = blas_tris[0].reshape(-1, 3).astype(np.float64)
    lo = P.min(axis=0)
    q = (P - lo) / ext
    deformed = (P + 0.1 * ext * np.sin(3.0 * q[:, [1, 2, 0]])).astype(np.float32).reshape(-1, 9)
    inp.triangles_in.copy_(rt.to_device(deformed))
    rt.Refit(inp, root, count, plan)
    torch.cuda.synchronize()
    assert rt.refit_status(plan, inp.num_triangles) == 0
    sc2 = Instanced(rt, [(inp.triangles_out, inp.nodes_out, root, count), entries[1]], moved, "sah")
    sc2.frame()
    assert rt.instance_status(sc2.status) == 0
    wt2, inst_of2, prim_of2 = ir.world_triangles([deformed, blas_tris[1]], moved)
    _check_world(sc2, wt2, inst_of2, prim_of2, _world_rays(wt2, 1200, seed=19), "refitted BLAS")


# ------------------------------------------------------------------ 7: edges
@pytest.mark.parametrize("count", (1, 2, 3))
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_few_instances(world, count, kind):
    rt = world.rt
    blas_tris, entries, _, inst = _composition(world)
    sub = inst[[0, 6, 2][:count]]
    sc = Instanced(rt, entries, sub, kind)
    sc.frame()
    wt, inst_of, prim_of = ir.world_triangles(blas_tris, sub)
    _check_world(sc, wt, inst_of, prim_of, _world_rays(wt, 800, seed=23 + count), f"{count} instances TLAS {kind}")


def test_degenerate_rays_batch_edges_and_prefetch(world):
    import ctypes
    import torch
    rt = world.rt
    blas_tris, entries, _, inst = _composition(world)
    sc = Instanced(rt, entries, inst, "bottom_up")
    sc.frame()
    wt, _, _ = ir.world_triangles(blas_tris, inst)
    good = _world_rays(wt, 500, seed=29).astype(rt.RAY)
    nan = np.float32(np.nan)
    deg = good[:8].copy()
    deg["dir"][0] = 0.0
    deg["origin"][1, 0] = nan
    deg["dir"][2, 1] = nan
    deg["tmin"][3], deg["tmax"][3] = 5.0, 1.0
    deg["tmin"][4], deg["tmax"][4] = 1e-5, 0.0
    deg["tmin"][5] = nan
    deg["tmax"][6] = nan
    deg["dir"][7] = nan
    hits, ids, ctr = sc.run(deg, counters=True)
    assert (hits["primitive_id"] == rt.MISS).all() and (hits["t"] == np.inf).all() and (ids == rt.MISS).all()
    assert ctr[1] == 0
    ok, oid, _ = sc.run(good)
    assert (oid != rt.MISS).sum() > 100
    # the pair-prefetch instantiation gives the same records
    pf, pid, _ = sc.run(good, num_primitives=BIG)
    assert pf.tobytes() == ok.tobytes() and (pid == oid).all()
    pa, _, _ = sc.run(good, any_hit=True, num_primitives=BIG)
    na, _, _ = sc.run(good, any_hit=True)
    assert pa.tobytes() == na.tobytes()
    # records past num_rays keep their poison
    root, count = sc.root
    a = rt._Accel(rt._ptr(sc.tlas.triangles_out), rt._ptr(sc.tlas.nodes_out), root, count)
    for n in (1, 63, 65, 1001):
        rays = np.tile(good, (n + good.size - 1) // good.size)[:n]
        rd = rt.to_device(rays)
        hits = torch.full(((n + 64) * 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        idb = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = rt.lib().rt_intersect_rays_instanced(ctypes.byref(a), rt._ptr(sc.records), sc.n, rt._ptr(sc.table), 2,
                                                  rt._ptr(rd), rt._ptr(hits), rt._ptr(idb), n, 0, 0, None,
                                                  rt._stream_ptr(None))
        assert rc == 0
        torch.cuda.synchronize()
        hv, iv = hits.cpu().numpy(), idb.cpu().numpy()
        assert (hv[4 * n:] == 0x5A5A5A5A).all() and (iv[n:] == 0x5A5A5A5A).all(), f"num_rays {n}: records past the batch"
        exp = np.tile(ok, (n + good.size - 1) // good.size)[:n]
        assert hv[:4 * n].view(np.float32).view(rt.HIT).tobytes() == exp.tobytes()
        assert (iv[:n].view(np.uint32) == np.tile(oid, (n + good.size - 1) // good.size)[:n]).all()


# ------------------------------------------------------------------ 8: hipGraph
def test_prepare_build_and_query_in_a_hip_graph(world):
    import torch
    rt = world.rt
    blas_tris, entries, _, inst = _composition(world)
    sc = Instanced(rt, entries, inst, "bottom_up")
    wt, _, _ = ir.world_triangles(blas_tris, inst)
    rays = rt.to_device(_world_rays(wt, 2000, seed=37).astype(rt.RAY)).view(torch.float32).view(-1, 8)
    n = rays.shape[0]
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    anyh = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")

    ids_any = torch.empty_like(ids)

    def one_frame():
        ctr.zero_()
        sc.frame()
        sc.query(rays, hits, ids, counters=ctr)
        sc.query(rays, anyh, ids_any, any_hit=True)

    moved = inst.copy()
    moved["object_to_world"][:, :, 3] += np.float32(0.05) * np.arange(inst.size, dtype=np.float32)[:, None]
    eager = {}
    for key, instances in (("a", inst), ("b", moved)):
        sc.instances.copy_(rt.to_device(instances))
        one_frame()
        torch.cuda.synchronize()
        eager[key] = [t.clone() for t in (hits, anyh, ids, ids_any, ctr)]
    assert int((eager["a"][2] != -1).sum()) > 100
    assert not torch.equal(eager["a"][0], eager["b"][0]), "the moved scene must give other records"

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for key in ("a", "b", "a"):
        sc.instances.copy_(rt.to_device(inst if key == "a" else moved))   # rewritten in place: same buffer
        for t in (hits, anyh, ids, ids_any):
            t.fill_(0)
        sc.tlas.nodes_out.zero_()
        sc.records.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip((hits, anyh, ids, ids_any, ctr), eager[key]):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                               exp.view(torch.int32) if exp.dtype == torch.float32 else exp), key
