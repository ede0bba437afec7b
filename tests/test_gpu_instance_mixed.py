"""GPU tests of mixed instancing (rt_intersect_rays_instanced_mixed: triangle and sphere BLASes under one TLAS) against
tests/instance_mixed_ref.py, the numpy restatement of the header (tests/test_instance_mixed_ref_cpu.py checks that reference on
its own), and against the two sibling queries.

1. a table of RT_GEOM_TRIANGLES only: hits, instance ids, box and triangle tests byte-equal to rt_intersect_rays_instanced;
2. one identity instance over a sphere tree: hits and sphere tests byte-equal to rt_intersect_rays_spheres;
3. exact composition of the mixed world: where float64 shows the answer is unique, every record equals the minimum-t result of
   rt_intersect_rays / rt_intersect_rays_spheres over the instances on the float32 object rays, bit for bit;
4. float64 brute force over the mixed world: hit / miss, instance, primitive, t, the far-root flag, the miss record; any hit;
   tmax = nextafter(t, 0) misses;
5. what is never entered or hit: an unknown kind, a sphere BLAS without a sphere array, a count below some leaf ids, the
   invalid spheres, a flagged instance;
6. small and edge shapes, batch sizes, degenerate rays, counters;
7. prepare_spheres + sphere BLAS build + prepare_instances + TLAS build + both query modes in one HIP graph, replayed after the
   sphere buffer and the instance matrices are rewritten in place."""
import numpy as np
import pytest

import instance_mixed_ref as mr
import instance_ref as ir
import sphere_ref as sr
import test_gpu_instances as gi
import test_gpu_ray_queries as rq
import test_gpu_spheres as gs

pytestmark = pytest.mark.gpu

TLAS_KINDS = ("bottom_up", "hybrid", "sah")
F = np.float32
MISS = mr.MISS


# ------------------------------------------------------------------ plumbing
class Blases:
    """the built BLASes of a world: table entries (tris, nodes, root, count) and geometry entries (None | (spheres, count))"""

    def __init__(self, rt, data, kinds, trees):
        import torch
        self.entries, self.geoms, self.keep = [], [], []
        for d, k, tree in zip(data, kinds, trees):
            if k == mr.TRIANGLES:
                inp, root, count = rq._gpu_tree(rt, d, tree)
                self.entries.append((inp.triangles_out, inp.nodes_out, root, count))
                self.geoms.append(None)
                self.keep.append(inp)
            else:
                s = gs.Spheres(rt, d, tree).frame()
                torch.cuda.synchronize()
                assert rt.sphere_status(s.status) == (0 if sr.valid(d).all() else rt.RT_SPHERE_BAD)
                self.entries.append((s.tree.triangles_out, s.tree.nodes_out) + s.root)
                self.geoms.append((s.spheres, s.n))
                self.keep.append(s)


class Mixed(gi.Instanced):
    """test_gpu_instances.Instanced with a geometry table: query() is the mixed call, sibling() the all-triangle one"""

    def __init__(self, rt, entries, geoms, instances, tlas="bottom_up"):
        super().__init__(rt, entries, instances, tlas)
        self.geoms = geoms                          # kept alive; a device tensor is taken as the table itself
        self.geom_table = geoms if hasattr(geoms, "data_ptr") else rt.geometry_table(list(geoms))

    def query(self, rays, hits, ids, any_hit=False, num_primitives=0, counters=None, stream=None):
        root, count = self.root
        self.rt.IntersectRaysInstancedMixed(self.tlas.triangles_out, self.tlas.nodes_out, root, count, self.records, self.n,
                                            self.table, self.geom_table, len(self.entries), rays, hits, ids, any_hit=any_hit,
                                            counters=counters, stream=stream)

    def sibling(self, rays, any_hit=False):
        """rt_intersect_rays_instanced(num_primitives = 0) on the same buffers -> (HIT array, ids, counters)"""
        import torch
        d = gs._dev_rays(self.rt, rays)
        hits = torch.empty((d.shape[0], 4), dtype=torch.float32, device="cuda")
        ids = torch.empty(d.shape[0], dtype=torch.int32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        gi.Instanced.query(self, d, hits, ids, any_hit=any_hit, counters=ctr)
        torch.cuda.synchronize()
        return (hits.cpu().numpy().view(self.rt.HIT).reshape(-1), ids.cpu().numpy().view(np.uint32),
                ctr.cpu().numpy().astype(np.uint64))


def _raw_geometry(rt, rows):
    """a geometry table from (data pointer, count, kind) rows: entries geometry_table() would not write"""
    tab = np.zeros(len(rows), rt.GEOMETRY)
    for k, row in enumerate(rows):
        tab[k] = row
    return rt.to_device(tab)


@pytest.fixture(scope="module")
def world(rt, scenes, ora):
    return rq.World(rt, scenes, ora)


@pytest.fixture(scope="module")
def mixed(rt):
    """the mixed world's BLASes, built once"""
    w = mr.world()
    return w, Blases(rt, w.data, w.kinds, mr.BLAS_TREES)


@pytest.fixture(scope="module")
def scene(rt, mixed):
    """the mixed world under each TLAS kind, prepared and built once"""
    import torch
    cache = {}

    def get(kind):
        if kind not in cache:
            w, b = mixed
            sc = Mixed(rt, b.entries, b.geoms, w.instances, kind)
            sc.frame()
            torch.cuda.synchronize()
            assert rt.instance_status(sc.status) == 0
            cache[kind] = sc
        return cache[kind]
    return get


def _composition(world):
    """test_gpu_instances._composition, rebuilt: 7 instances of grid_mesh(24) (LBVH) and grid_mesh(16, 9) (SAH with pairs)"""
    rt = world.rt
    ga = world.scene("grid")[0]
    ia, ra, ca = world.gpu("grid", "bottom_up")
    gb = world.scenes.grid_mesh(16, 9)
    ib, rb, cb = rq._gpu_tree(rt, gb, "sah_pairs")
    ext = float(np.ptp(ga.reshape(-1, 3), axis=0).max())
    R = ir.rotation(0.3, -0.5, 0.9)
    A = gi._affine
    mats = [A(R, (0, 0, 0)), A(np.diag([1.5, 0.6, 2.0]), (1.3 * ext, 0, 0)), A(np.diag([-1.0, 1.0, 1.0]), (0, 1.3 * ext, 0)),
            A([[1, 0.4, 0], [0, 1, 0.3], [0.2, 0, 1]], (0, 0, 1.3 * ext)), A(np.eye(3), (-1.2 * ext, 0.5 * ext, 0.2 * ext)),
            A(R, (0.07 * ext, 0.05 * ext, -0.03 * ext)), A(ir.rotation(0.1, 0.2, 0.3) * 1.2, (-0.3 * ext, -1.2 * ext, 0))]
    inst = ir.instance_array(mats, [0, 0, 0, 0, 0, 0, 1])
    entries = [(ia.triangles_out, ia.nodes_out, ra, ca), (ib.triangles_out, ib.nodes_out, rb, cb)]
    return [ga, gb], entries, inst, (ia, ib)


def _canon_prims(w, ids, prims):
    """reported primitive ids with sphere indices mapped to the first exact copy (the reference's canonical index)"""
    out = prims.astype(np.int64).copy()
    for i in w.sphere_inst:
        m = ids == i
        out[m] = w.canon[w.blas[i]][out[m]]
    return out


def _check_miss_records(hits, ids, what):
    miss = hits["primitive_id"] == MISS
    assert ((ids == MISS) == miss).all(), f"{what}: instance id and primitive id disagree on hit / miss"
    rec = hits[miss]
    assert (rec["t"] == np.inf).all() and (rec["u"].view(np.uint32) == 0).all() and (rec["v"].view(np.uint32) == 0).all(), what
    return ~miss


def _check_f64(sc, ref, what, min_hits=50):
    """closest hit against the float64 brute force on stable rays; any hit; tmax honoured"""
    w, f, st, rays = ref.world, ref.f64, ref.stable, ref.rays
    hits, ids, _ = sc.run(rays)
    got = _check_miss_records(hits, ids, what)
    print(f"{what}: {rays.size} rays, unstable {100 * ref.unstable_share:.2f} %, hits {int(got.sum())}")
    assert ref.unstable_share <= mr.CAP, what
    bad = st & (got != f["hit"])
    assert not bad.any(), f"{what}: hit / miss differs on {bad.sum()} stable rays (first {np.flatnonzero(bad)[:5]})"
    m = st & f["hit"]
    assert (ids[m] == f["inst"][m]).all(), f"{what}: instance"
    assert (_canon_prims(w, ids, hits["primitive_id"])[m] == f["prim"][m]).all(), f"{what}: primitive"
    t_ref = f["t"][m]
    assert (np.abs(hits["t"][m] - t_ref) <= 1e-5 * np.maximum(1, t_ref)).all(), f"{what}: t"
    sph = m & (f["kind"] == mr.SPHERES)
    assert (hits["u"][sph] == f["far"][sph].astype(F)).all() and (hits["v"][sph].view(np.uint32) == 0).all(), f"{what}: far root"
    on_sphere = got & np.isin(ids, w.sphere_inst)
    assert np.isin(hits["u"][on_sphere], (0.0, 1.0)).all() and (hits["v"][on_sphere].view(np.uint32) == 0).all(), what
    assert got.sum() >= min_hits, f"{what}: too few hits to mean anything"
    # any hit: exactly where closest hit hits, inside the window, never closer than the closest, on the reported primitive
    a, aid, _ = sc.run(rays, any_hit=True)
    ah = _check_miss_records(a, aid, f"{what} any-hit")
    assert (ah == got).all(), f"{what}: any-hit hits on {ah.sum()} rays, closest-hit on {got.sum()}"
    at = a["t"][ah]
    assert ((at >= rays["tmin"][ah]) & (at <= rays["tmax"][ah]) & (at >= hits["t"][ah])).all(), f"{what}: any-hit t"
    assert (aid[ah] < w.n).all()
    ta, tb = mr.crossing64(w, rays[ah], aid[ah].astype(np.int64), a["primitive_id"][ah].astype(np.int64))
    err = np.fmin(np.abs(at - ta), np.abs(at - tb))
    assert (err <= 1e-4 * np.maximum(1, np.abs(at))).all(), f"{what}: an any-hit record is not a crossing of its primitive"
    # tmax honoured: a window that ends one ulp before the closest hit holds nothing
    sel = got & (hits["t"] > 0)
    cut = rays[sel].copy()
    cut["tmax"] = np.nextafter(hits["t"][sel], F(0))
    for any_hit in (False, True):
        again, aids, _ = sc.run(cut, any_hit=any_hit)
        assert (again["primitive_id"] == MISS).all() and (aids == MISS).all(), f"{what}: hits beyond tmax"
    return hits, ids


# ------------------------------------------------------------------ 1: all-triangle table == rt_intersect_rays_instanced
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_all_triangle_table_equals_the_instanced_query(world, kind):
    rt = world.rt
    blas_tris, entries, inst, _keep = _composition(world)
    sc = Mixed(rt, entries, [None, None], inst, kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    wt, _, _ = ir.world_triangles(blas_tris, inst)
    rays = gi._world_rays(wt, 1500, seed=11)
    for any_hit in (False, True):
        hits, ids, c = sc.run(rays, any_hit=any_hit, counters=True)
        exp, eid, ec = sc.sibling(rays, any_hit=any_hit)
        assert hits.tobytes() == exp.tobytes(), f"TLAS {kind} any_hit {any_hit}: records differ from rt_intersect_rays_instanced"
        assert (ids == eid).all()
        assert c[0] == ec[0] and c[1] == ec[1], f"TLAS {kind} any_hit {any_hit}: tests {c[:2]} vs {ec[:2]}"
        assert (ids != MISS).sum() > 200 and c[1] > 0


# ------------------------------------------------------------------ 2: identity sphere instance == rt_intersect_rays_spheres
@pytest.mark.parametrize("kind", gs.KINDS)
@pytest.mark.parametrize("name", sr.SCENES)
def test_identity_sphere_instance_equals_the_sphere_query(rt, name, kind):
    s = sr.gpu_scene(name)
    sp = gs.Spheres(rt, s, kind).frame()
    rays = gi._positive_zeros(sr.make_rays(s, 61, n=3000))
    sc = Mixed(rt, [(sp.tree.triangles_out, sp.tree.nodes_out) + sp.root], [(sp.spheres, sp.n)],
               ir.instance_array([np.eye(3, 4)], [0]), kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    assert (sc.host_records()["world_to_object"] == np.eye(3, 4, dtype=F)).all()
    for any_hit in (False, True):
        exp, ec = sp.run(rays, counters=True, any_hit=any_hit)
        hits, ids, c = sc.run(rays, any_hit=any_hit, counters=True)
        assert hits.tobytes() == exp.tobytes(), f"{name} {kind} any_hit {any_hit}: records differ from rt_intersect_rays_spheres"
        assert c[1] == ec[1], f"{name} {kind} any_hit {any_hit}: sphere tests {c[1]} vs {ec[1]}"
        hit = exp["primitive_id"] != MISS
        assert (ids[hit] == 0).all() and (ids[~hit] == MISS).all()
        assert hit.sum() > 300 and c[0] > 0


# ------------------------------------------------------------------ 3: exact composition
def _per_instance_minimum(rt, w, b, rays, rec, counts=None):
    """the minimum-t result over the instances of rt_intersect_rays / rt_intersect_rays_spheres on the float32 object rays"""
    import torch
    best = np.zeros(rays.size, rt.HIT)
    best["t"], best["primitive_id"] = np.inf, MISS
    best_id = np.full(rays.size, MISS, np.uint32)
    for k in range(w.n):
        blas = int(w.blas[k])
        e = b.entries[blas]
        obj = ir.object_rays(rays.astype(rt.RAY), rec["world_to_object"][k])
        if w.kinds[blas] == mr.TRIANGLES:
            h, _ = rq._query(rt, (gi.Tree(e[0], e[1]), e[2], e[3]), obj)
        else:
            spheres, ns = b.geoms[blas]
            d = gs._dev_rays(rt, obj)
            out = torch.empty((d.shape[0], 4), dtype=torch.float32, device="cuda")
            rt.IntersectRaysSpheres(e[0], e[1], e[2], e[3], spheres, ns if counts is None else counts.get(blas, ns), d, out)
            torch.cuda.synchronize()
            h = out.cpu().numpy().view(rt.HIT).reshape(-1)
        take = (h["primitive_id"] != MISS) & (h["t"] < best["t"])
        best[take], best_id[take] = h[take], k
    return best, best_id


@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_exact_composition(rt, mixed, scene, kind):
    w, b = mixed
    sc = scene(kind)
    ref = mr.reference(mr.SEEDS[0])
    rays, f = ref.rays, ref.f64
    hits, ids, _ = sc.run(rays)
    best, best_id = _per_instance_minimum(rt, w, b, rays, sc.host_records())
    judged = ref.stable & np.where(f["hit"], best_id.astype(np.int64) == f["inst"], True)
    print(f"TLAS {kind}: judged share {judged.mean():.4f}")
    assert judged.mean() > 0.95, f"judged share {judged.mean():.3f}"
    assert hits[judged].tobytes() == best[judged].tobytes(), \
        f"{kind}: {np.sum(hits[judged] != best[judged])} records differ from the per-instance minimum"
    assert (ids[judged] == best_id[judged]).all()
    on = best_id[judged]
    assert np.isin(on, w.sphere_inst).sum() > 200 and (np.isin(on, np.flatnonzero(w.inst_kind == mr.TRIANGLES))).sum() > 200
    assert len(set(on.tolist()) - {MISS}) >= 6


# ------------------------------------------------------------------ 4: float64 brute force
@pytest.mark.parametrize("seed", mr.SEEDS)
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_against_float64(scene, kind, seed):
    ref = mr.reference(seed)
    hits, ids = _check_f64(scene(kind), ref, f"mixed world TLAS {kind} seed {seed}", min_hits=400)
    w, f = ref.world, ref.f64
    far = ref.stable & f["hit"] & f["far"]
    assert far.sum() > 0 and (hits["u"][far] == 1).all()
    # the four invalid spheres of both sets, placed where every ray into their instance would hit them, are never hit
    for i in w.sphere_inst:
        m = ids == i
        assert sr.valid(w.data[w.blas[i]])[hits["primitive_id"][m]].all(), f"instance {i}: an invalid sphere was hit"


# ------------------------------------------------------------------ 5: never entered, never hit
def test_never_entered_or_hit(rt, mixed, scene):
    w, b = mixed
    ref = mr.reference(mr.SEEDS[0])
    rays, st = ref.rays, ref.stable
    base, base_ids, _ = scene("bottom_up").run(rays)
    base_any, base_any_ids, _ = scene("bottom_up").run(rays, any_hit=True)
    # three instances of the lattice, scaled to cover the whole scene (a wall of tangent spheres: every ray is aimed at them):
    # 8 through a table entry of kind 7, 9 through a sphere entry without a sphere array, 10 with a singular matrix (flagged)
    boxes = w.boxes()
    lo, hi = np.min([x[0] for x in boxes], axis=0), np.max([x[1] for x in boxes], axis=0)
    big = gi._affine(np.eye(3) * float((hi - lo).max()) * 0.6, (lo + hi) / 2)
    extra = ir.instance_array([big, big, np.zeros((3, 4))], [4, 5, 3])
    inst = np.concatenate([w.instances, extra])
    entries = b.entries + [b.entries[3], b.entries[3]]
    lat, nlat = b.geoms[3]
    cloud, ncloud = b.geoms[2]
    rows = [(0, 0, 0), (0, 0, 0), (cloud.data_ptr(), ncloud, 1), (lat.data_ptr(), nlat, 1)]
    # the wall is a wall: with valid entries nearly every ray hits instance 8 or 9
    sc = Mixed(rt, entries, _raw_geometry(rt, rows + [(lat.data_ptr(), nlat, 1)] * 2), inst)
    sc.frame()
    assert rt.instance_status(sc.status) == rt.RT_INSTANCE_SINGULAR
    _, ids, _ = sc.run(rays[:ref.rays.size // 2])
    assert np.isin(ids, (8, 9)).mean() > 0.8, "the extra instances do not cover the scene"
    # ... and with the entries under test none does, and the rest of the scene answers as the scene without them
    sc.geom_table = _raw_geometry(rt, rows + [(lat.data_ptr(), nlat, 7), (0, nlat, 1)])
    hits, ids, c = sc.run(rays, counters=True)
    assert (ids[ids != MISS] < 8).all(), "an instance that must not be entered was hit"
    assert hits[st].tobytes() == base[st].tobytes() and (ids[st] == base_ids[st]).all()
    a, aid, _ = sc.run(rays, any_hit=True)
    assert ((aid != MISS) == (base_any_ids != MISS)).all() and (aid[aid != MISS] < 8).all()
    # (the sibling reads no table: it walks the three lattices' leaves as triangles -- only the hit / miss of the mixed call is held)

    # a count below some leaf ids: those spheres are never hit, the others still are
    keep = 700
    sc = Mixed(rt, b.entries, _raw_geometry(rt, [(0, 0, 0), (0, 0, 0), (cloud.data_ptr(), keep, 1), (lat.data_ptr(), nlat, 1)]),
               w.instances)
    sc.frame()
    hits, ids, _ = sc.run(rays)
    in_cloud = np.isin(base_ids, np.flatnonzero(w.blas == 2))
    removed = in_cloud & (base["primitive_id"] >= keep)
    assert removed.sum() > 50 and (in_cloud & ~removed).sum() > 50
    now_cloud = np.isin(ids, np.flatnonzero(w.blas == 2))
    assert (hits["primitive_id"][now_cloud] < keep).all(), "a sphere at or above count was hit"
    same = st & ~removed
    assert hits[same].tobytes() == base[same].tobytes() and (ids[same] == base_ids[same]).all()
    assert (hits["t"][removed] >= base["t"][removed]).all()
    best, best_id = _per_instance_minimum(rt, w, b, rays[removed], sc.host_records(), counts={2: keep})
    agree = (best_id == ids[removed]) & (best["primitive_id"] == hits["primitive_id"][removed])
    assert agree.mean() > 0.95 and hits[removed][agree].tobytes() == best[agree].tobytes()


# ------------------------------------------------------------------ 6: small and edge shapes
def _small(rt, data, kinds, trees, mats, blas, n_rays, seed, kind="bottom_up"):
    w = mr.World([np.ascontiguousarray(d, F) for d in data], kinds, ir.instance_array(mats, blas))
    b = Blases(rt, w.data, w.kinds, trees)
    sc = Mixed(rt, b.entries, b.geoms, w.instances, kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    return w, b, sc, mr.Reference(w, mr.world_rays(w, n_rays, seed))


@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_small_scenes(rt, scenes, kind):
    one = np.array([[0.25, -0.5, 0.75, 1.5]], F)
    M = gi._affine(ir.rotation(0.4, 0.1, -0.7) @ np.diag([2.0, 1.0, 0.5]), (3, -2, 1))
    w, b, sc, ref = _small(rt, [one], (mr.SPHERES,), ("bottom_up",), [M], [0], 384, 71, kind)
    _check_f64(sc, ref, f"one instance of one sphere TLAS {kind}")
    # one triangle instance plus one sphere instance side by side (a coincident distance would be an unstable ray)
    few = np.array([[0.1, -0.2, 0.3, 0.5], [1.2, 0.1, -0.1, 0.4], [-0.9, 0.8, 0.2, 0.7]], F)
    w, b, sc, ref = _small(rt, [scenes.grid_mesh(4, 3), few], (mr.TRIANGLES, mr.SPHERES), ("bottom_up", "sah"),
                           [gi._affine(ir.rotation(0.2, 0.3, 0.1), (0, 0, 0)), gi._affine(np.eye(3) * 1.5, (2, 2.5, 2))], [0, 1],
                           384, 72, kind)
    hits, ids = _check_f64(sc, ref, f"a mesh and a sphere set TLAS {kind}")
    assert (ids == 0).sum() > 30 and (ids == 1).sum() > 30


def test_edge_shapes(rt, scenes):
    import torch
    # r = 0 under a scale by 2 (exact in float32): hit only by a line through the centre; o' = (-1, 1, -1), d' = (.5, .25, 1), t = 4
    s = np.array([[1, 2, 3, 0], [4, 0, 0, 0.5], [0, 5, 0, 0.25]], F)
    w, b, sc, _ = _small(rt, [s], (mr.SPHERES,), ("bottom_up",), [gi._affine(np.eye(3) * 2.0)], [0], 8, 73)
    assert (sc.host_records()["world_to_object"][0] == np.eye(3, 4, dtype=F) * F(0.5)).all()
    rays = np.zeros(2, mr.RAY)
    rays["origin"] = [(-2, 2, -2), (-2 + 2e-3, 2, -2)]
    rays["dir"] = [(1, 0.5, 2), (1, 0.5, 2)]
    rays["tmax"] = np.inf
    hits, ids, _ = sc.run(rays)
    assert hits["primitive_id"].tolist() == [0, MISS] and ids.tolist() == [0, MISS] and hits["t"][0] == 4.0
    assert hits["u"][0] == 0 and hits["v"][0] == 0

    # a sphere BLAS with count = 0 is entered and tests nothing; the mesh beside it answers as before
    few =np.array([[0.1, -0.2, 0.3, 0.5], [1.2, 0.1, -0.1, 0.4], [-0.9, 0.8, 0.2, 0.7]], F)
    w, b, sc, ref = _small(rt, [scenes.grid_mesh(4, 3), few], (mr.TRIANGLES, mr.SPHERES), ("bottom_up", "bottom_up"),
                           [gi._affine(np.eye(3)), gi._affine(np.eye(3) * 1.5, (2, 2.5, 2))], [0, 1], 256, 74)
    full, full_ids, cf = sc.run(ref.rays, counters=True)
    assert (full_ids == 1).sum() > 30
    spheres, ns = b.geoms[1]
    sc.geom_table = _raw_geometry(rt, [(0, 0, 0), (spheres.data_ptr(), 0, 1)])
    hits, ids, c = sc.run(ref.rays, counters=True)
    assert (ids != 1).all() and c[1] < cf[1] and c[0] > 0
    on_mesh = full_ids == 0
    assert hits[on_mesh].tobytes() == full[on_mesh].tobytes()
    sphere_only = Mixed(rt, [b.entries[1]], _raw_geometry(rt, [(spheres.data_ptr(), 0, 1)]),
                        ir.instance_array([np.eye(3, 4)], [0]))
    sphere_only.frame()
    hits, ids, c = sphere_only.run(ref.rays, counters=True)
    assert (ids == MISS).all() and (hits["primitive_id"] == MISS).all() and c[1] == 0 and c[0] > 0

    # num_instances = 0: an empty TLAS, every ray misses
    d = gs._dev_rays(rt, ref.rays[:100])
    out = torch.full((100, 4), -7.0, dtype=torch.float32, device="cuda")
    oid = torch.full((100,), 5, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    rt.IntersectRaysInstancedMixed(None, None, 0, 0, None, 0, None, sc.geom_table, 0, d, out, oid, counters=ctr)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(rt.HIT).reshape(-1)
    assert (got["primitive_id"] == MISS).all() and (got["t"] == np.inf).all() and (oid.cpu().numpy().view(np.uint32) == MISS).all()
    assert (ctr.cpu().numpy()[:2] == 0).all()


def test_batch_sizes_degenerate_rays_and_counters(rt, scene):
    import torch
    sc = scene("bottom_up")
    ref = mr.reference(mr.SEEDS[1])
    good = ref.rays[:1024]
    full, full_ids, _ = sc.run(good)
    assert (full_ids != MISS).sum() > 200
    d = gs._dev_rays(rt, good)
    for any_hit in (False, True):
        exp, exp_ids, _ = sc.run(good, any_hit=any_hit)
        for n in (1, 63, 64, 65, 256, 257):
            hits = torch.full((n + 64, 4), -7.0, dtype=torch.float32, device="cuda")
            ids = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            sc.query(d[:n], hits, ids, any_hit=any_hit)
            torch.cuda.synchronize()
            hv, iv = hits.cpu().numpy(), ids.cpu().numpy()
            assert hv[:n].view(rt.HIT).reshape(-1).tobytes() == exp[:n].tobytes(), n
            assert (iv[:n].view(np.uint32) == exp_ids[:n]).all(), n
            assert (hv[n:] == F(-7.0)).all() and (iv[n:] == 0x5A5A5A5A).all(), f"num_rays {n}: records past the batch"
    # degenerate rays: a miss each.  A NaN component or an empty window is not traced (no test at all); a ray without a
    # direction is traced as in rt_intersect_rays_instanced and reaches no leaf
    nan = F(np.nan)
    deg = good[:7].copy()
    deg["origin"][0, 0] = nan
    deg["dir"][1, 1] = nan
    deg["tmin"][2], deg["tmax"][2] = 5.0, 1.0
    deg["tmin"][3], deg["tmax"][3] = 1e-5, 0.0
    deg["tmin"][4] = nan
    deg["tmax"][5] = nan
    deg["dir"][6] = nan
    still = good[:1].copy()
    still["dir"] = 0
    for any_hit in (False, True):
        hits, ids, ctr = sc.run(deg, any_hit=any_hit, counters=True)
        assert (hits["primitive_id"] == MISS).all() and (hits["t"] == np.inf).all() and (ids == MISS).all()
        assert (hits["u"] == 0).all() and (hits["v"] == 0).all()
        assert ctr[0] == 0 and ctr[1] == 0, "a ray that is not traced counts no test"
        hits, ids, ctr = sc.run(still, any_hit=any_hit, counters=True)
        assert (hits["primitive_id"] == MISS).all() and (hits["t"] == np.inf).all() and (ids == MISS).all() and ctr[1] == 0
    # counters add across launches; a permutation of the rays leaves the test counts unchanged
    n = good.size
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    for any_hit in (False, True):
        _, _, c1 = sc.run(good, any_hit=any_hit, counters=True)
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        sc.query(d, hits, ids, any_hit=any_hit, counters=ctr)
        sc.query(d, hits, ids, any_hit=any_hit, counters=ctr)
        torch.cuda.synchronize()
        assert (ctr.cpu().numpy().astype(np.uint64) == 2 * c1).all() and c1[0] > 0 and c1[1] > 0
        perm = np.random.default_rng(5).permutation(n)
        ph, pid, c2 = sc.run(good[perm], any_hit=any_hit, counters=True)
        assert (c2[:2] == c1[:2]).all(), f"any_hit {any_hit}: test counts {c2[:2]} after a permutation, {c1[:2]} before"
        e, eid, _ = sc.run(good, any_hit=any_hit)
        assert ph.tobytes() == e[perm].tobytes() and (pid == eid[perm]).all()


# ------------------------------------------------------------------ 7: hipGraph
def test_everything_in_one_hip_graph(rt, scenes):
    import torch
    mesh = scenes.grid_mesh(16, 9)
    cloud = {"a": sr.gpu_scene("cloud"), "b": sr.moved(sr.gpu_scene("cloud"), 1)}
    ext = 16.0
    mats = {"a": [gi._affine(ir.rotation(0.3, -0.5, 0.9)), gi._affine(np.diag([1.5, 0.6, 2.0]) * 6.0, (1.4 * ext, 0, 0)),
                  gi._affine(np.eye(3) * 5.0, (0.5 * ext, 0.2 * ext, 0.5 * ext))]}
    mats["b"] = [m + np.array([[0, 0, 0, 0.3 * (k + 1)], [0, 0, 0, -0.2], [0, 0, 0, 0.1 * k]]) for k, m in enumerate(mats["a"])]
    worlds = {key: mr.World([mesh, cloud[key]], (mr.TRIANGLES, mr.SPHERES), ir.instance_array(mats[key], [0, 1, 1]))
              for key in ("a", "b")}
    refs = {key: mr.Reference(worlds[key], mr.world_rays(worlds["a"], 600, 81)) for key in ("a", "b")}

    inp, root, count = rq._gpu_tree(rt, mesh, "sah_pairs")
    sp = gs.Spheres(rt, cloud["a"], "bottom_up")
    sc = Mixed(rt, [(inp.triangles_out, inp.nodes_out, root, count), (sp.tree.triangles_out, sp.tree.nodes_out) + sp.root],
               [None, (sp.spheres, sp.n)], worlds["a"].instances, "bottom_up")
    rays = gs._dev_rays(rt, refs["a"].rays)
    n = rays.shape[0]
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    anyh = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ids_any = torch.empty_like(ids)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")

    def one_frame():
        ctr.zero_()
        sp.frame()          # rt_prepare_spheres + the sphere BLAS build
        sc.frame()          # rt_prepare_instances + the TLAS build
        sc.query(rays, hits, ids, counters=ctr)
        sc.query(rays, anyh, ids_any, any_hit=True)

    def load(key):
        sp.upload(cloud[key])                                          # rewritten in place: the same buffers
        sc.instances.copy_(rt.to_device(worlds[key].instances))

    eager = {}
    for key in ("a", "b"):
        load(key)
        one_frame()
        torch.cuda.synchronize()
        eager[key] = [t.clone() for t in (hits, anyh, ids, ids_any, ctr)]
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

    class Replayed:
        """_check_f64's view of the graph's output buffers: run() hands back what the replay wrote for the graph's own rays, and
        runs any other batch (the tmax cut) eagerly on the same buffers"""

        def run(self, r, any_hit=False, counters=False):
            if r.size == n and r.tobytes() == refs["a"].rays.tobytes():
                h, i = (anyh, ids_any) if any_hit else (hits, ids)
                return h.cpu().numpy().view(rt.HIT).reshape(-1), i.cpu().numpy().view(np.uint32), None
            return sc.run(r, any_hit=any_hit)

    for key in ("a", "b", "a"):
        load(key)
        for t in (hits, anyh, ids, ids_any):
            t.fill_(0)
        sp.tree.nodes_out.zero_()
        sc.tlas.nodes_out.zero_()
        sc.records.fill_(0xFF)
        sp.status.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert rt.sphere_status(sp.status) == rt.RT_SPHERE_BAD and rt.instance_status(sc.status) == 0
        for g, e in zip((hits, anyh, ids, ids_any, ctr), eager[key]):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                               e.view(torch.int32) if e.dtype == torch.float32 else e), key
        _check_f64(Replayed(), refs[key], f"graph replay {key}")
