"""GPU tests of mixed instancing with capsules (rt_intersect_rays_instanced_mixed_capsules: triangle, sphere and capsule BLASes
under one TLAS) against tests/instance_capsule_ref.py, the numpy restatement of the header (tests/test_instance_capsule_ref_cpu.py
checks that reference on its own), and against the sibling queries.

1. no capsules in the table: hits, instance ids, box and primitive tests byte-equal to rt_intersect_rays_instanced_mixed, with
   an index list to rt_intersect_rays_instanced_mixed_indexed;
2. one identity instance over a capsule tree: records and capsule tests byte-equal to rt_intersect_rays_capsules;
3. degenerate capsules (p0 == p1) against the sphere BLAS of the same spheres under the same instances: byte-equal;
4. exact composition: where float64 shows the answer is unique, every record equals the minimum-t result of rt_intersect_rays /
   rt_intersect_rays_spheres / rt_intersect_rays_capsules over the instances on the float32 object rays, bit for bit;
5. float64 brute force over the three-kind world: hit / miss, instance, primitive, t, the far-root flag, the miss record; any
   hit; tmax = nextafter(t, 0) misses; the far-root problem gives u == 1;
6. what is never entered or hit: an unknown kind, a capsule BLAS without a capsule array, a flagged instance, a count below
   some leaf ids, the invalid capsules;
7. small shapes, batch sizes, degenerate rays, an empty TLAS, count == 0;
8. the index list: rt_sort_rays's order over the TLAS, out-of-range entries, unlisted records untouched;
9. 2 and 5 on trees re-packed into runs of 1..7 slots with NONE slots (tests/wide_trees.py);
10. prepare_capsules + capsule BLAS build + prepare_instances + TLAS build + both query modes in one HIP graph, replayed after
    the capsule buffer and the instance matrices are rewritten in place."""
import numpy as np
import pytest

import capsule_ref as cr
import instance_capsule_ref as icr
import instance_mixed_ref as mr
import instance_ref as ir
import sphere_ref as sr
import test_gpu_capsules as gc
import test_gpu_instance_mixed as gm
import test_gpu_instances as gi
import test_gpu_ray_queries as rq
import test_gpu_spheres as gs
import wide_trees as wt

pytestmark = pytest.mark.gpu

TLAS_KINDS = gm.TLAS_KINDS
F = np.float32
MISS = icr.MISS
PATTERN = 0x5A5A5A5A


# ------------------------------------------------------------------ plumbing
class Blases:
    """test_gpu_instance_mixed.Blases with a third kind: a capsule BLAS's geometry entry is (capsules, count, RT_GEOM_CAPSULES)"""

    def __init__(self, rt, data, kinds, trees):
        import torch
        self.entries, self.geoms, self.keep = [], [], []
        for d, k, tree in zip(data, kinds, trees):
            if k == icr.CAPSULES:
                c = gc.Capsules(rt, d, tree).frame()
                torch.cuda.synchronize()
                assert rt.capsule_status(c.status) == (0 if cr.valid(d).all() else rt.RT_CAPSULE_BAD)
                self.entries.append((c.tree.triangles_out, c.tree.nodes_out) + c.root)
                self.geoms.append((c.capsules, c.n, rt.RT_GEOM_CAPSULES))
                self.keep.append(c)
            else:
                b = gm.Blases(rt, [d], [k], [tree])
                self.entries += b.entries
                self.geoms += b.geoms
                self.keep += b.keep


class Caps(gm.Mixed):
    """test_gpu_instance_mixed.Mixed whose query() is the new call (order: through an index list); old() is the mixed call
    without the capsule arm on the same buffers"""
    order = None
    use_old = False

    def query(self, rays, hits, ids, any_hit=False, num_primitives=0, counters=None, stream=None):
        if self.use_old:
            return gm.Mixed.query(self, rays, hits, ids, any_hit=any_hit, counters=counters, stream=stream)
        root, count = self.root
        self.rt.IntersectRaysInstancedMixedCapsules(self.tlas.triangles_out, self.tlas.nodes_out, root, count, self.records,
                                                    self.n, self.table, self.geom_table, len(self.entries), rays, hits, ids,
                                                    self.order, any_hit=any_hit, counters=counters, stream=stream)

    def old(self, rays, any_hit=False):
        """rt_intersect_rays_instanced_mixed on the same buffers -> (HIT array, ids, counters)"""
        self.use_old = True
        try:
            return self.run(rays, any_hit=any_hit, counters=True)
        finally:
            self.use_old = False

    def run_prefilled(self, rays, order=None, any_hit=False, old=False):
        """the call on buffers pre-filled with a pattern -> (hits as uint32 [n, 4], ids as uint32 [n], counters)"""
        import torch
        rt = self.rt
        d = gs._dev_rays(rt, rays)
        n = d.shape[0]
        hits = torch.full((n, 4), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
        ids = torch.full((n,), PATTERN, dtype=torch.int32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        root, count = self.root
        args = (self.tlas.triangles_out, self.tlas.nodes_out, root, count, self.records, self.n, self.table, self.geom_table,
                len(self.entries), d)
        if old:
            rt.IntersectRaysInstancedMixedIndexed(*args, order, hits, ids, any_hit=any_hit, counters=ctr)
        else:
            rt.IntersectRaysInstancedMixedCapsules(*args, hits, ids, order, any_hit=any_hit, counters=ctr)
        torch.cuda.synchronize()
        return (hits.view(torch.int32).cpu().numpy().view(np.uint32), ids.cpu().numpy().view(np.uint32),
                ctr.cpu().numpy().astype(np.uint64))


def _dev_order(rt, order):
    return rt.to_device(np.ascontiguousarray(order, np.uint32))


@pytest.fixture(scope="module")
def mixed(rt):
    """the three-kind world's BLASes, built once"""
    w = icr.world()
    return w, Blases(rt, w.data, w.kinds, icr.BLAS_TREES)


@pytest.fixture(scope="module")
def scene(rt, mixed):
    """the three-kind world under each TLAS kind, prepared and built once"""
    import torch
    cache = {}

    def get(kind):
        if kind not in cache:
            w, b = mixed
            sc = Caps(rt, b.entries, b.geoms, w.instances, kind)
            sc.frame()
            torch.cuda.synchronize()
            assert rt.instance_status(sc.status) == 0
            cache[kind] = sc
        return cache[kind]
    return get


def _canon_prims(w, ids, prims):
    """reported primitive ids with sphere and capsule indices mapped to the first exact copy (the reference's canonical index)"""
    out = prims.astype(np.int64).copy()
    for insts, canon in ((w.sphere_inst, w.canon), (w.capsule_inst, w.ccanon)):
        for i in insts:
            m = ids == i
            out[m] = canon[w.blas[i]][out[m]]
    return out


def _check_capsule_records(sc, w, rays, hits, ids, what):
    """every record of a capsule instance is the float32 formula's for the reported capsule on the object-space ray under the
    device's own world_to_object, in the ray's original window: t, u and v bit for bit; no invalid capsule is reported"""
    rec = sc.host_records()
    n = 0
    for i in w.capsule_inst:
        m = np.flatnonzero(ids == i)
        prim = hits["primitive_id"][m].astype(np.int64)
        data = w.data[w.blas[i]]
        assert (prim < data.shape[0]).all() and cr.valid(data)[prim].all(), f"{what}: instance {i}: an invalid capsule was hit"
        t, far, v = icr.capsule_f32(w, rays[m], i, prim, rec["world_to_object"][i])
        assert not np.isnan(t).any(), f"{what}: instance {i}: a reported capsule is not hit by its ray in float32"
        for got, exp, name in ((hits["t"][m], t, "t"), (hits["u"][m], far.astype(F), "u"), (hits["v"][m], v, "v")):
            assert (gc._bits(got) == gc._bits(exp)).all(), f"{what}: instance {i}: {name} is not the float32 formula's"
        n += m.size
    return n


def _check_f64(sc, ref, what, min_hits=50, t_tol=icr.T_TOL):
    """closest hit against the float64 brute force on stable rays; any hit; tmax honoured (test_gpu_instance_mixed._check_f64
    for three kinds).  A capsule t may be GPU_TOL_FACTOR * t_tol from float64's"""
    w, f, st, rays = ref.world, ref.f64, ref.stable, ref.rays
    hits, ids, _ = sc.run(rays)
    got = gm._check_miss_records(hits, ids, what)
    assert ref.unstable_share <= icr.CAP, what
    bad = st & (got != f["hit"])
    assert not bad.any(), f"{what}: hit / miss differs on {bad.sum()} stable rays (first {np.flatnonzero(bad)[:5]})"
    m = st & f["hit"]
    assert (ids[m] == f["inst"][m]).all(), f"{what}: instance"
    assert (_canon_prims(w, ids, hits["primitive_id"])[m] == f["prim"][m]).all(), f"{what}: primitive"
    caps = m & (f["kind"] == icr.CAPSULES)
    err = cr.t_error(hits["t"][caps], f["t"][caps]).max(initial=0.0)
    print(f"{what}: {rays.size} rays, unstable {100 * ref.unstable_share:.2f} %, hits {int(got.sum())}, on capsules "
          f"{int(caps.sum())}, far roots {int((caps & f['far']).sum())}, max capsule t error {err:.3g} "
          f"(allowed {cr.GPU_TOL_FACTOR * t_tol:.3g})")
    assert err <= cr.GPU_TOL_FACTOR * t_tol, f"{what}: a capsule t is {err:.3g} from float64's"
    rest = m & ~caps
    assert (np.abs(hits["t"][rest] - f["t"][rest]) <= 1e-5 * np.maximum(1, f["t"][rest])).all(), f"{what}: t"
    round_ = m & (f["kind"] != icr.TRIANGLES)
    assert (hits["u"][round_] == f["far"][round_].astype(F)).all(), f"{what}: far root"
    sph = got & np.isin(ids, w.sphere_inst)
    assert np.isin(hits["u"][sph], (0.0, 1.0)).all() and (hits["v"][sph].view(np.uint32) == 0).all(), what
    on_caps = got & np.isin(ids, w.capsule_inst)
    assert np.isin(hits["u"][on_caps], (0.0, 1.0)).all() and ((hits["v"][on_caps] >= 0) & (hits["v"][on_caps] <= 1)).all(), what
    _check_capsule_records(sc, w, rays, hits, ids, what)
    assert got.sum() >= min_hits, f"{what}: too few hits to mean anything"
    # any hit: exactly where closest hit hits, inside the window, never closer than the closest, a genuine record
    a, aid, _ = sc.run(rays, any_hit=True)
    ah = gm._check_miss_records(a, aid, f"{what} any-hit")
    assert (ah == got).all(), f"{what}: any-hit hits on {ah.sum()} rays, closest-hit on {got.sum()}"
    at = a["t"][ah]
    assert ((at >= rays["tmin"][ah]) & (at <= rays["tmax"][ah]) & (at >= hits["t"][ah])).all(), f"{what}: any-hit t"
    assert (aid[ah] < w.n).all()
    _check_capsule_records(sc, w, rays, a, aid, f"{what} any-hit")
    other = ah & ~np.isin(aid, w.capsule_inst)
    ta, tb = mr.crossing64(w, rays[other], aid[other].astype(np.int64), a["primitive_id"][other].astype(np.int64))
    e2 = np.fmin(np.abs(a["t"][other] - ta), np.abs(a["t"][other] - tb))
    assert (e2 <= 1e-4 * np.maximum(1, np.abs(a["t"][other]))).all(), f"{what}: an any-hit record is not a crossing of its primitive"
    # tmax honoured: a window that ends one ulp before the closest hit holds nothing (a far-root hit has its near root behind tmin)
    sel = got & (hits["t"] > 0)
    cut = rays[sel].copy()
    cut["tmax"] = np.nextafter(hits["t"][sel], F(0))
    for any_hit in (False, True):
        again, aids, _ = sc.run(cut, any_hit=any_hit)
        assert (again["primitive_id"] == MISS).all() and (aids == MISS).all(), f"{what}: hits beyond tmax"
    return hits, ids


# ------------------------------------------------------------------ 1: no capsules in the table == the mixed call
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_table_without_capsules_equals_the_mixed_query(rt, kind):
    import torch
    w = mr.world()
    b = gm.Blases(rt, w.data, w.kinds, mr.BLAS_TREES)
    sc = Caps(rt, b.entries, b.geoms, w.instances, kind)
    sc.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(sc.status) == 0
    rays = mr.reference(mr.SEEDS[0]).rays
    rng = np.random.default_rng(3)
    order = rng.permutation(rays.size)[:2500].astype(np.uint32)
    order[::97] = rays.size + 5                                  # out of range: skipped by both calls
    dorder = _dev_order(rt, order)
    for any_hit in (False, True):
        hits, ids, c = sc.run(rays, any_hit=any_hit, counters=True)
        exp, eid, ec = sc.old(rays, any_hit=any_hit)
        assert hits.tobytes() == exp.tobytes(), f"TLAS {kind} any_hit {any_hit}: records differ from rt_intersect_rays_instanced_mixed"
        assert (ids == eid).all()
        assert c[0] == ec[0] and c[1] == ec[1], f"TLAS {kind} any_hit {any_hit}: tests {c[:2]} vs {ec[:2]}"
        assert (ids != MISS).sum() > 400 and c[1] > 0
        h, i, c = sc.run_prefilled(rays, dorder, any_hit=any_hit)
        eh, ei, ec = sc.run_prefilled(rays, dorder, any_hit=any_hit, old=True)
        assert h.tobytes() == eh.tobytes() and i.tobytes() == ei.tobytes(), f"TLAS {kind} any_hit {any_hit}: indexed records differ"
        assert c[0] == ec[0] and c[1] == ec[1]
        assert (i == PATTERN).sum() >= rays.size - 2500


# ------------------------------------------------------------------ 2: identity capsule instance == rt_intersect_rays_capsules
def _identity_case(rt, c, tree_entry, kind):
    sc = Caps(rt, [tree_entry], [(c.capsules, c.n, rt.RT_GEOM_CAPSULES)], ir.instance_array([np.eye(3, 4)], [0]), kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    assert (sc.host_records()["world_to_object"] == np.eye(3, 4, dtype=F)).all()
    return sc


@pytest.mark.parametrize("kind", gc.KINDS)
def test_identity_capsule_instance_equals_the_capsule_query(rt, kind):
    caps = cr.gpu_scene("fibres")
    c = gc.Capsules(rt, caps, kind).frame()
    rays = gi._positive_zeros(cr.make_rays(caps, 61, n=3000))
    sc = _identity_case(rt, c, (c.tree.triangles_out, c.tree.nodes_out) + c.root, kind)
    for any_hit in (False, True):
        exp, ec = c.run(rays, counters=True, any_hit=any_hit)
        hits, ids, cc = sc.run(rays, any_hit=any_hit, counters=True)
        assert hits.tobytes() == exp.tobytes(), f"fibres {kind} any_hit {any_hit}: records differ from rt_intersect_rays_capsules"
        assert cc[1] == ec[1], f"fibres {kind} any_hit {any_hit}: capsule tests {cc[1]} vs {ec[1]}"
        hit = exp["primitive_id"] != MISS
        assert (ids[hit] == 0).all() and (ids[~hit] == MISS).all()
        assert hit.sum() > 300 and cc[0] > 0
    assert ((exp["v"] > 0) & (exp["v"] < 1)).sum() > 100 and (exp["u"] == 1).sum() > 0


# ------------------------------------------------------------------ 3: degenerate capsules == spheres
def test_degenerate_capsules_equal_the_sphere_arm(rt):
    import torch
    s = sr.gpu_scene("cloud")
    caps = np.zeros((s.shape[0], 8), F)
    caps[:, 0:4], caps[:, 4:7] = s, s[:, 0:3]
    sp = gs.Spheres(rt, s, "sah").frame()
    cp = gc.Capsules(rt, caps, "sah").frame()
    torch.cuda.synchronize()
    assert rt.to_host(sp.tree.triangles_in, F, 9 * sp.n).tobytes() == rt.to_host(cp.tree.triangles_in, F, 9 * cp.n).tobytes(), \
        "the proxies of a p0 == p1 capsule and of its sphere differ"
    mats = [mr._affine(ir.rotation(0.3, -0.5, 0.9) * 6.0, (0, 0, 0)), mr._affine(np.diag([1.5, 0.6, 2.0]) * 6.0, (30, 0, 0)),
            mr._affine(np.array([[1, 0.4, 0], [0, 1, 0.3], [0.2, 0, 1]]) * 7.0, (0, 28, 5)),
            mr._affine(np.diag([-1.0, 1.0, 1.0]) * 5.0, (3, 2, 1))]                      # overlaps instance 0
    inst = ir.instance_array(mats, [0, 0, 0, 0])
    w = mr.World([s], (mr.SPHERES,), inst)
    rays = mr.world_rays(w, 1500, 31)
    a = Caps(rt, [(sp.tree.triangles_out, sp.tree.nodes_out) + sp.root], [(sp.spheres, sp.n)], inst)
    b = Caps(rt, [(cp.tree.triangles_out, cp.tree.nodes_out) + cp.root], [(cp.capsules, cp.n, rt.RT_GEOM_CAPSULES)], inst)
    a.frame()
    b.frame()
    torch.cuda.synchronize()
    assert a.host_proxies().tobytes() == b.host_proxies().tobytes(), "the root boxes of the two trees differ"
    for any_hit in (False, True):
        ha, ia, ca = a.run(rays, any_hit=any_hit, counters=True)
        hb, ib, cb = b.run(rays, any_hit=any_hit, counters=True)
        ho, io, co = a.old(rays, any_hit=any_hit)
        assert ha.tobytes() == hb.tobytes() and (ia == ib).all(), f"any_hit {any_hit}: a p0 == p1 capsule is not its sphere"
        assert (ca[:2] == cb[:2]).all(), f"any_hit {any_hit}: tests {ca[:2]} vs {cb[:2]}"
        assert ha.tobytes() == ho.tobytes() and (ia == io).all() and (ca[:2] == co[:2]).all()
        assert (ia != MISS).sum() > 400 and (ha["u"] == 1).sum() > 0 and len(set(ia.tolist()) - {MISS}) == 4


# ------------------------------------------------------------------ 4: exact composition
def _per_instance_minimum(rt, w, b, rays, rec):
    """the minimum-t result over the instances of rt_intersect_rays / rt_intersect_rays_spheres / rt_intersect_rays_capsules on
    the float32 object rays"""
    import torch
    best = np.zeros(rays.size, rt.HIT)
    best["t"], best["primitive_id"] = np.inf, MISS
    best_id = np.full(rays.size, MISS, np.uint32)
    for k in range(w.n):
        blas = int(w.blas[k])
        e = b.entries[blas]
        obj = ir.object_rays(rays.astype(rt.RAY), rec["world_to_object"][k])
        if w.kinds[blas] == icr.TRIANGLES:
            h, _ = rq._query(rt, (gi.Tree(e[0], e[1]), e[2], e[3]), obj)
        else:
            d = gs._dev_rays(rt, obj)
            out = torch.empty((d.shape[0], 4), dtype=torch.float32, device="cuda")
            call = rt.IntersectRaysSpheres if w.kinds[blas] == icr.SPHERES else rt.IntersectRaysCapsules
            call(e[0], e[1], e[2], e[3], b.geoms[blas][0], b.geoms[blas][1], d, out)
            torch.cuda.synchronize()
            h = out.cpu().numpy().view(rt.HIT).reshape(-1)
        take = (h["primitive_id"] != MISS) & (h["t"] < best["t"])
        best[take], best_id[take] = h[take], k
    return best, best_id


@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_exact_composition(rt, mixed, scene, kind):
    w, b = mixed
    sc = scene(kind)
    ref = icr.reference(icr.SEEDS[0])
    f = ref.f64
    hits, ids, _ = sc.run(ref.rays)
    best, best_id = _per_instance_minimum(rt, w, b, ref.rays, sc.host_records())
    judged = ref.stable & np.where(f["hit"], best_id.astype(np.int64) == f["inst"], True)
    print(f"TLAS {kind}: judged share {judged.mean():.4f}")
    assert judged.mean() > 0.95, f"judged share {judged.mean():.3f}"
    assert hits[judged].tobytes() == best[judged].tobytes(), \
        f"{kind}: {np.sum(hits[judged] != best[judged])} records differ from the per-instance minimum"
    assert (ids[judged] == best_id[judged]).all()
    on = best_id[judged]
    for insts in (w.capsule_inst, w.sphere_inst, np.flatnonzero(w.inst_kind == icr.TRIANGLES)):
        assert np.isin(on, insts).sum() > 200
    body = judged & np.isin(ids, w.capsule_inst) & (hits["v"] > 0) & (hits["v"] < 1)
    assert body.sum() > 100, "too few body hits to pin v"


# ------------------------------------------------------------------ 5: float64 brute force
@pytest.mark.parametrize("seed", icr.SEEDS)
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_against_float64(scene, kind, seed):
    ref = icr.reference(seed)
    hits, ids = _check_f64(scene(kind), ref, f"three-kind world TLAS {kind} seed {seed}", min_hits=600)
    w = ref.world
    for i in w.capsule_inst:
        assert (ids == i).sum() > 50, f"capsule instance {i} is hardly hit"
    for i in w.sphere_inst:
        assert sr.valid(w.data[w.blas[i]])[hits["primitive_id"][ids == i]].all(), f"instance {i}: an invalid sphere was hit"


@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_far_roots_under_a_non_uniform_placement(rt, kind):
    ref = icr.far_reference()
    w = ref.world
    b = Blases(rt, w.data, w.kinds, ("bottom_up",))
    sc = Caps(rt, b.entries, b.geoms, w.instances, kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    hits, ids = _check_f64(sc, ref, f"far-root problem TLAS {kind}", t_tol=icr.T_TOL_FAR)
    far = ref.stable & ref.f64["hit"] & ref.f64["far"]
    assert far.sum() >= 50 and (hits["u"][far] == 1).all() and (ids[far] == 0).all()
    assert np.isin(hits["v"][far], (0.0, 1.0)).sum() > 0 and ((hits["v"][far] > 0) & (hits["v"][far] < 1)).sum() > 0


# ------------------------------------------------------------------ 6: never entered, never hit
def test_never_entered_or_hit(rt, mixed, scene):
    import torch
    w, b = mixed
    ref = icr.reference(icr.SEEDS[0])
    rays, st = ref.rays, ref.stable
    base, base_ids, _ = scene("bottom_up").run(rays)
    base_any, base_any_ids, _ = scene("bottom_up").run(rays, any_hit=True)
    # a wall: sphere_ref's lattice as p0 == p1 capsules, scaled to cover the whole scene (tangent spheres: every ray is aimed
    # at them).  Instance 10 enters it through a table entry of kind 7, 11 through a capsule entry without a capsule array, 12
    # has a singular matrix (flagged)
    lat = sr.gpu_scene("lattice")
    wall = np.zeros((lat.shape[0], 8), F)
    wall[:, 0:4], wall[:, 4:7] = lat, lat[:, 0:3]
    wc = gc.Capsules(rt, wall, "sah").frame()
    torch.cuda.synchronize()
    boxes = w.boxes()
    lo, hi = np.min([x[0] for x in boxes], axis=0), np.max([x[1] for x in boxes], axis=0)
    big = gi._affine(np.eye(3) * float((hi - lo).max()) * 0.6, (lo + hi) / 2)
    extra = ir.instance_array([big, big, np.zeros((3, 4))], [4, 5, 3])
    inst = np.concatenate([w.instances, extra])
    wall_entry = (wc.tree.triangles_out, wc.tree.nodes_out) + wc.root
    entries = b.entries + [wall_entry, wall_entry]
    cloud, ncloud = b.geoms[2]
    fib, nfib, _ = b.geoms[3]
    rows = [(0, 0, 0), (0, 0, 0), (cloud.data_ptr(), ncloud, 1), (fib.data_ptr(), nfib, 2)]
    # the wall is a wall: with valid entries nearly every ray hits instance 10 or 11
    sc = Caps(rt, entries, gm._raw_geometry(rt, rows + [(wc.capsules.data_ptr(), wc.n, 2)] * 2), inst)
    sc.frame()
    assert rt.instance_status(sc.status) == rt.RT_INSTANCE_SINGULAR
    _, ids, _ = sc.run(rays[:rays.size // 2])
    assert np.isin(ids, (10, 11)).mean() > 0.8, "the extra instances do not cover the scene"
    # ... and with the entries under test none does, and the rest of the scene answers as the scene without them
    sc.geom_table = gm._raw_geometry(rt, rows + [(wc.capsules.data_ptr(), wc.n, 7), (0, wc.n, 2)])
    hits, ids, c = sc.run(rays, counters=True)
    assert (ids[ids != MISS] < 10).all(), "an instance that must not be entered was hit"
    assert hits[st].tobytes() == base[st].tobytes() and (ids[st] == base_ids[st]).all()
    a, aid, _ = sc.run(rays, any_hit=True)
    assert ((aid != MISS) == (base_any_ids != MISS)).all() and (aid[aid != MISS] < 10).all()
    # the two older calls still do not enter a capsule entry: every hit of theirs lies in a mesh or a sphere instance
    ho, io, _ = scene("bottom_up").old(rays)
    assert not np.isin(io, w.capsule_inst).any() and (io != MISS).sum() > 400

    # a count below some leaf ids: those capsules are never hit, the others still are
    keep = 700
    sc = Caps(rt, b.entries, gm._raw_geometry(rt, rows[:3] + [(fib.data_ptr(), keep, 2)]), w.instances)
    sc.frame()
    hits, ids, _ = sc.run(rays)
    in_caps = np.isin(base_ids, w.capsule_inst)
    removed = in_caps & (base["primitive_id"] >= keep)
    assert removed.sum() > 50 and (in_caps & ~removed).sum() > 50
    now_caps = np.isin(ids, w.capsule_inst)
    assert (hits["primitive_id"][now_caps] < keep).all(), "a capsule at or above count was hit"
    same = st & ~removed
    assert hits[same].tobytes() == base[same].tobytes() and (ids[same] == base_ids[same]).all()
    assert (hits["t"][removed] >= base["t"][removed]).all()
    # the four invalid capsules, placed where every ray into their instance would hit them, are never hit
    assert cr.valid(w.data[3])[base["primitive_id"][in_caps]].all() and (~cr.valid(w.data[3])).sum() == 4


# ------------------------------------------------------------------ 7: small and edge shapes
def _built(rt, w, trees, kind="bottom_up"):
    b = Blases(rt, w.data, w.kinds, trees)
    sc = Caps(rt, b.entries, b.geoms, w.instances, kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    return b, sc


def _small(rt, data, kinds, trees, mats, blas, n_rays, seed, kind="bottom_up"):
    w = icr.World([np.ascontiguousarray(d, F) for d in data], kinds, ir.instance_array(mats, blas))
    b, sc = _built(rt, w, trees, kind)
    return w, b, sc, icr.Reference(w, mr.world_rays(w, n_rays, seed))


@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_small_scenes(rt, scenes, kind):
    one = cr.pack([[0.25, -0.5, 0.75]], [0.6], [[1.0, 0.5, -0.25]])
    M = gi._affine(ir.rotation(0.4, 0.1, -0.7) @ np.diag([2.0, 1.0, 0.5]), (3, -2, 1))
    w, b, sc, ref = _small(rt, [one], (icr.CAPSULES,), ("bottom_up",), [M], [0], 384, 71, kind)
    _check_f64(sc, ref, f"one instance of one capsule TLAS {kind}")
    # one triangle instance plus one two-capsule instance side by side (a coincident distance would be an unstable ray); its
    # fat capsules have a t tolerance of their own, measured on the CPU like the others
    ref = icr.pair_reference()
    b, sc = _built(rt, ref.world, ("bottom_up", "sah"), kind)
    hits, ids = _check_f64(sc, ref, f"a mesh and a two-capsule set TLAS {kind}", t_tol=icr.T_TOL_PAIR)
    assert (ids == 0).sum() > 30 and (ids == 1).sum() > 30
    assert set(hits["primitive_id"][ids == 1].tolist()) == {0, 1}


def test_count_zero_and_empty_tlas(rt, scenes):
    import torch
    two = cr.pack([[0.1, -0.2, 0.3], [1.2, 0.1, -0.1]], [0.5, 0.4], [[-0.9, 0.8, 0.2], [1.2, 0.6, -0.1]])
    w, b, sc, ref = _small(rt, [scenes.grid_mesh(4, 3), two], (icr.TRIANGLES, icr.CAPSULES), ("bottom_up", "bottom_up"),
                           [gi._affine(np.eye(3)), gi._affine(np.eye(3) * 1.5, (2, 2.5, 2))], [0, 1], 256, 74)
    full, full_ids, cf = sc.run(ref.rays, counters=True)
    assert (full_ids == 1).sum() > 30
    # a capsule BLAS with count = 0 is entered and tests nothing; the mesh beside it answers as before
    caps, nc, _ = b.geoms[1]
    sc.geom_table = gm._raw_geometry(rt, [(0, 0, 0), (caps.data_ptr(), 0, 2)])
    hits, ids, c = sc.run(ref.rays, counters=True)
    assert (ids != 1).all() and c[1] < cf[1] and c[0] > 0
    on_mesh = full_ids == 0
    assert hits[on_mesh].tobytes() == full[on_mesh].tobytes()
    only = Caps(rt, [b.entries[1]], gm._raw_geometry(rt, [(caps.data_ptr(), 0, 2)]), ir.instance_array([np.eye(3, 4)], [0]))
    only.frame()
    hits, ids, c = only.run(ref.rays, counters=True)
    assert (ids == MISS).all() and (hits["primitive_id"] == MISS).all() and c[1] == 0 and c[0] > 0
    # num_instances = 0: an empty TLAS, every ray misses, directly and through an index list
    d = gs._dev_rays(rt, ref.rays[:100])
    order = _dev_order(rt, np.arange(100))
    for o in (None, order):
        out = torch.full((100, 4), -7.0, dtype=torch.float32, device="cuda")
        oid = torch.full((100,), 5, dtype=torch.int32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        rt.IntersectRaysInstancedMixedCapsules(None, None, 0, 0, None, 0, None, sc.geom_table, 0, d, out, oid, o, counters=ctr)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(rt.HIT).reshape(-1)
        assert (got["primitive_id"] == MISS).all() and (got["t"] == np.inf).all() and (got["u"] == 0).all()
        assert (oid.cpu().numpy().view(np.uint32) == MISS).all() and (ctr.cpu().numpy()[:2] == 0).all()


def test_batch_sizes_and_degenerate_rays(rt, scene):
    import torch
    sc = scene("bottom_up")
    good = icr.reference(icr.SEEDS[1]).rays[:1024]
    d = gs._dev_rays(rt, good)
    for any_hit in (False, True):
        exp, exp_ids, _ = sc.run(good, any_hit=any_hit)
        assert (exp_ids != MISS).sum() > 200
        for n in (1, 63, 64, 65, 257):
            hits = torch.full((n + 64, 4), -7.0, dtype=torch.float32, device="cuda")
            ids = torch.full((n + 64,), PATTERN, dtype=torch.int32, device="cuda")
            sc.query(d[:n], hits, ids, any_hit=any_hit)
            torch.cuda.synchronize()
            hv, iv = hits.cpu().numpy(), ids.cpu().numpy()
            assert hv[:n].view(rt.HIT).reshape(-1).tobytes() == exp[:n].tobytes(), n
            assert (iv[:n].view(np.uint32) == exp_ids[:n]).all(), n
            assert (hv[n:] == F(-7.0)).all() and (iv[n:] == PATTERN).all(), f"num_rays {n}: records past the batch"
    # degenerate rays: a miss each.  A NaN component or an empty window is not traced (no test at all); a ray without a
    # direction is traced as in rt_intersect_rays_instanced_mixed and reaches no leaf
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
        assert (hits["u"].view(np.uint32) == 0).all() and (hits["v"].view(np.uint32) == 0).all()
        assert ctr[0] == 0 and ctr[1] == 0, "a ray that is not traced counts no test"
        hits, ids, ctr = sc.run(still, any_hit=any_hit, counters=True)
        assert (hits["primitive_id"] == MISS).all() and (hits["t"] == np.inf).all() and (ids == MISS).all() and ctr[1] == 0


# ------------------------------------------------------------------ 8: the index list
def test_index_list(rt, scene):
    import torch
    sc = scene("hybrid")
    rays = icr.reference(icr.SEEDS[0]).rays
    n = rays.size
    d = gs._dev_rays(rt, rays)
    root, count = sc.root
    sorted_order = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    scratch = rt.device_bytes(rt.RaySortScratchBytes(n))
    assert rt.SortRays(sc.tlas.nodes_out, root, count, d, sorted_order, scratch) == n
    torch.cuda.synchronize()
    assert sorted(sorted_order.cpu().numpy().view(np.uint32).tolist()) == list(range(n))
    rng = np.random.default_rng(9)
    part = rng.permutation(n)[:n // 2].astype(np.uint32)
    listed = np.zeros(n, bool)
    listed[part] = True
    part = np.concatenate([part, [n, n + 1, 0xFFFFFFFF]]).astype(np.uint32)[rng.permutation(n // 2 + 3)]
    for any_hit in (False, True):
        direct, direct_ids, dc = sc.run(rays, any_hit=any_hit, counters=True)
        h, i, c = sc.run_prefilled(rays, sorted_order, any_hit=any_hit)
        assert h.tobytes() == direct.tobytes() and (i == direct_ids).all(), f"any_hit {any_hit}: rt_sort_rays's order"
        assert (c[:2] == dc[:2]).all()
        h, i, c = sc.run_prefilled(rays, _dev_order(rt, part), any_hit=any_hit)
        assert h[listed].tobytes() == direct[listed].tobytes() and (i[listed] == direct_ids[listed]).all()
        assert (h[~listed] == PATTERN).all() and (i[~listed] == PATTERN).all(), "an unlisted record was written"
        assert 0 < c[1] < dc[1]
    assert np.isin(direct_ids[listed], icr.world().capsule_inst).sum() > 100


# ------------------------------------------------------------------ 9: wide trees
class _WideCaps(Caps):
    """Caps whose TLAS is swapped for its re-packed copy after the build"""
    wide_root = None

    @property
    def root(self):
        return self.wide_root or gi.Instanced.root.fget(self)


def _host_tree(rt, built):
    return rt.to_host(built.triangles_out, rt.TRIANGLE_PAIR), rt.to_host(built.nodes_out, rt.NODE)


def _widen_tlas(rt, sc, n):
    tl, tn = _host_tree(rt, sc.tlas)
    tlas = wt.Tree(tl[:n].copy(), *wt.repack(tn, *sc.root, none_every=2), rt)
    assert ((tlas.nodes["w28"] >> 29) == wt.NONE).any()
    sc.tlas, sc.wide_root = tlas.pose, (tlas.root, tlas.count)
    return tlas


def test_wide_trees(rt, mixed):
    import torch
    w, b = mixed
    # the fibres' BLAS re-packed into runs of 1..7 slots with NONE slots: test 2 on the wide bytes
    fib = b.keep[3]
    leaves, nodes = _host_tree(rt, fib.tree)
    t = wt.Tree(leaves, *wt.repack(nodes, *fib.root), rt)
    assert set(wt.hist(t.nodes, t.root, t.count)) == set(range(1, 8))
    wide_entry = (t.pose.triangles_out, t.pose.nodes_out, t.root, t.count)
    rays = gi._positive_zeros(cr.make_rays(w.data[3], 61, n=3000))
    d = gs._dev_rays(rt, rays)
    sc = _WideCaps(rt, [wide_entry], [b.geoms[3]], ir.instance_array([np.eye(3, 4)], [0]))
    sc.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(sc.status) == 0 and (sc.host_records()["world_to_object"] == np.eye(3, 4, dtype=F)).all()
    for any_hit in (False, True):
        exp = torch.empty((rays.size, 4), dtype=torch.float32, device="cuda")
        ec = torch.zeros(4, dtype=torch.int64, device="cuda")
        rt.IntersectRaysCapsules(*wide_entry, fib.capsules, fib.n, d, exp, any_hit=any_hit, counters=ec)
        hits, ids, c = sc.run(rays, any_hit=any_hit, counters=True)
        assert hits.tobytes() == exp.cpu().numpy().tobytes(), f"wide fibres any_hit {any_hit}: records differ from rt_intersect_rays_capsules"
        assert c[1] == int(ec.cpu().numpy()[1]) and (ids != MISS).sum() > 300
    # the world with the fibres' BLAS and the TLAS re-packed: test 5 on the wide bytes
    s = _WideCaps(rt, b.entries[:3] + [wide_entry], b.geoms, w.instances)
    s.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(s.status) == 0
    tlas = _widen_tlas(rt, s, w.n)
    assert tlas.count >= 3
    _check_f64(s, icr.reference(icr.SEEDS[0]), "wide three-kind world", min_hits=600)


# ------------------------------------------------------------------ 10: hipGraph
def test_everything_in_one_hip_graph(rt):
    import torch
    refs = icr.graph_references()                                 # a mesh and 376 capsules (the last one invalid), two poses
    worlds = {key: refs[key].world for key in ("a", "b")}
    mesh = worlds["a"].data[0]
    caps = {key: worlds[key].data[1] for key in ("a", "b")}

    inp, root, count = rq._gpu_tree(rt, mesh, "sah_pairs")
    cp = gc.Capsules(rt, caps["a"], "bottom_up")
    sc = Caps(rt, [(inp.triangles_out, inp.nodes_out, root, count), (cp.tree.triangles_out, cp.tree.nodes_out) + cp.root],
              [None, (cp.capsules, cp.n, rt.RT_GEOM_CAPSULES)], worlds["a"].instances, "bottom_up")
    rays = gs._dev_rays(rt, refs["a"].rays)
    n = rays.shape[0]
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    anyh = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ids_any = torch.empty_like(ids)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")

    def one_frame():
        ctr.zero_()
        cp.frame()          # rt_prepare_capsules + the capsule BLAS build
        sc.frame()          # rt_prepare_instances + the TLAS build
        sc.query(rays, hits, ids, counters=ctr)
        sc.query(rays, anyh, ids_any, any_hit=True)

    def load(key):
        cp.upload(caps[key])                                           # rewritten in place: the same buffers
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
        host_records = sc.host_records

        def run(self, r, any_hit=False, counters=False):
            if r.size == n and r.tobytes() == refs["a"].rays.tobytes():
                h, i = (anyh, ids_any) if any_hit else (hits, ids)
                return h.cpu().numpy().view(rt.HIT).reshape(-1), i.cpu().numpy().view(np.uint32), None
            return sc.run(r, any_hit=any_hit)

    for key in ("a", "b", "a"):
        load(key)
        for t in (hits, anyh, ids, ids_any):
            t.fill_(0)
        cp.tree.nodes_out.zero_()
        sc.tlas.nodes_out.zero_()
        sc.records.fill_(0xFF)
        cp.status.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert rt.capsule_status(cp.status) == rt.RT_CAPSULE_BAD and rt.instance_status(sc.status) == 0
        for g, e in zip((hits, anyh, ids, ids_any, ctr), eager[key]):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                               e.view(torch.int32) if e.dtype == torch.float32 else e), key
        _check_f64(Replayed(), refs[key], f"graph replay {key}", min_hits=100, t_tol=icr.T_TOL_GRAPH)
