"""GPU tests of the filtered instanced ray query (rt_intersect_rays_instanced_filtered: an instance visibility mask asked at the
TLAS leaf, world-space face culling, a per-ray (instance, primitive) skip) against tests/instance_filter_ref.py, on the scenes
of test_gpu_instances (grid_mesh(24) / grid_mesh(16), at most 7 instances, at most 3,000 rays per batch).

1. keep-all: over the three TLAS builders and both spellings (nulls; all-ones masks, zero flags, skip_instance = RT_MISS) the
   call is byte-equal to rt_intersect_rays_instanced in hits, instance_ids and all four counters; a NULL filter is equal too;
2. identity instance: one identity instance of each of the 8 tree kinds on two scenes, cull_back / cull_front / skip-nearest:
   hits byte-equal to rt_intersect_rays_filtered on the BLAS, closest and any-hit;
3. exact composition: on unique rays the record and the instance id equal the minimum-t result of rt_intersect_rays_filtered
   over the entered instances, each queried on its float32 object rays with its effective filter, bit for bit -- cull back,
   cull front, CULL_DISABLE on two instances, FLIP_FACING on the mirror, skip of the primary (instance, primitive) on a bounce
   batch (with rays whose skipped primitive id is hit in the OTHER copy of the same BLAS and reported there), three-group
   instance masks against random per-ray masks;
4. float64: hit / miss, instance, primitive and t against the filtered float64 brute force over the kept world triangles on
   unique rays, test_gpu_instances._check_world's tolerances on every arm (on the bounce batch t is checked where the float32
   start point resolves that bound: instance_filter_ref.t_resolved); any-hit hits iff closest-hit hits;
5. masks save work: a ray mask matching no instance gives all misses, zero triangle tests and exactly the box tests of the
   TLAS alone; excluding instance k gives the bytes of the unfiltered query over the scene rebuilt without k;
6. edges: 1, 2, 3 instances; batch ends with records past num_rays untouched; NaN and empty-window rays; a per_instance array
   shorter than the scene; mask 0 everywhere; the pair-prefetch instantiation; a singular instance; prepare + TLAS build +
   filtered query in one HIP graph replayed after per_instance is rewritten in place."""
import ctypes

import numpy as np
import pytest

import instance_filter_ref as fr
import instance_ref as ir
import ray_filter_ref as rx
import test_gpu_instances as ti
import test_gpu_ray_queries as rq
from test_gpu_ray_filter import _closest

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
BIG = rq.BIG              # >= 8 << 20: the scene-size hint that selects the pair-prefetch instantiation
UNFILTERED = "unfiltered"


# ------------------------------------------------------------------ plumbing
def _dev_ifilter(rt, flt):
    """fr.InstanceFilter (host arrays) -> rt.InstanceHitFilter (device arrays); None stays None (filter = NULL)"""
    import torch
    if flt is None:
        return None
    pi = None if flt.per_instance is None else rt.to_device(flt.per_instance).view(torch.int32).view(-1, 2)
    pr = None if flt.per_ray is None else rt.to_device(flt.per_ray).view(torch.int32).view(-1, 4)
    return rt.InstanceHitFilter(flt.flags, flt.ray_mask, pi, pr)


def _run(sc, rays, flt, any_hit=False, num_primitives=0, dev_filter=None):
    """numpy RAY array through the filtered call (UNFILTERED: rt_intersect_rays_instanced) -> (HIT array, ids, counters)"""
    import torch
    rt = sc.rt
    d = rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)
    n = d.shape[0]
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    if flt is UNFILTERED:
        sc.query(d, hits, ids, any_hit=any_hit, num_primitives=num_primitives, counters=ctr)
    else:
        root, count = sc.root
        hf = dev_filter if dev_filter is not None else _dev_ifilter(rt, flt)
        rt.IntersectRaysInstancedFiltered(sc.tlas.triangles_out, sc.tlas.nodes_out, root, count, sc.records, sc.n, sc.table,
                                          len(sc.entries), d, hits, ids, hf, any_hit=any_hit, num_primitives=num_primitives,
                                          counters=ctr)
    torch.cuda.synchronize()
    return (hits.cpu().numpy().view(rt.HIT).reshape(-1), ids.cpu().numpy().view(np.uint32),
            ctr.cpu().numpy().astype(np.uint64))


class Comp:
    """the 7-instance composition: its scenes per TLAS kind, the shared ray batch and the float64 candidates -- computed once,
    never changed"""

    def __init__(self, world):
        self.rt = world.rt
        self.blas_tris, self.entries, self.boxes, self.inst = ti._composition(world)
        assert self.inst.tobytes() == fr.composition_instances(self.blas_tris[0]).tobytes(), \
            "instance_filter_ref.composition_instances is no longer test_gpu_instances._composition"
        self.wt, self.inst_of, self.prim_of = ir.world_triangles(self.blas_tris, self.inst)
        self.rays = fr.world_rays(self.wt, fr.RAYS, fr.SEED).astype(self.rt.RAY)
        assert len(self.rays) <= 3000
        self.cand = fr.candidates(self.rays, self.wt)
        self._sc, self._ref, self._bounce = {}, {}, None

    def scene(self, kind):
        if kind not in self._sc:
            sc = ti.Instanced(self.rt, self.entries, self.inst, kind)
            sc.frame()
            assert self.rt.instance_status(sc.status) == 0
            self._sc[kind] = sc
        return self._sc[kind]

    def arm(self, name):
        """-> (rays, filter, float64 reference, unique) of arm `name` (fr.ARMS, or "skip" on its bounce batch)"""
        if name not in self._ref:
            if name == "skip":
                rays, per_ray, cand = self.bounce()
                flt = fr.InstanceFilter(0, 0, None, per_ray)
            else:
                rays, cand = self.rays, self.cand
                flt = fr.make_arm(name, self.inst.size, len(rays))
            ref, unique = fr.brute_force(cand, self.inst_of, self.prim_of, rays, flt)
            assert unique.mean() >= 0.95, f"{name}: unique share {unique.mean():.4f}"
            self._ref[name] = rays, flt, ref, unique
        return self._ref[name]

    def bounce(self):
        """the bounce batch off the unfiltered primary hits of the shared rays"""
        if self._bounce is None:
            first, first_inst, _ = _run(self.scene("bottom_up"), self.rays, UNFILTERED)
            rays, per_ray = fr.bounce_batch(self.rays, first, first_inst, self.wt, self.inst_of, self.prim_of, fr.BOUNCE_SEED)
            rays = rays.astype(self.rt.RAY)
            assert 300 < len(rays) <= 3000
            self._bounce = rays, per_ray, fr.candidates(rays, self.wt)
        return self._bounce


@pytest.fixture(scope="module")
def world(rt, scenes, ora):
    return rq.World(rt, scenes, ora)


@pytest.fixture(scope="module")
def comp(world):
    return Comp(world)


def _keep_all_arrays(num_instances, n):
    """the second spelling of keep-all: arrays of all-ones masks, zero flags, skip_instance = RT_MISS (ray_mask 0 and a
    skip_id that exists: neither may act)"""
    per_ray = np.zeros(n, fr.INSTANCE_RAY_FILTER)
    per_ray["mask"], per_ray["skip_instance"], per_ray["skip_id"], per_ray["pad"] = fr.ALL, MISS, 5, 0x5A5A5A5A
    return fr.InstanceFilter(0, 0, fr.instance_filters(num_instances), per_ray)


# ------------------------------------------------------------------ 1: keep-all
@pytest.mark.parametrize("kind", ti.TLAS_KINDS)
def test_keep_all_equals_the_unfiltered_call(comp, kind):
    sc = comp.scene(kind)
    rays = comp.rays
    for any_hit in (False, True):
        exp, eid, ec = _run(sc, rays, UNFILTERED, any_hit=any_hit)
        assert (eid != MISS).sum() > 200 and ec[0] > 0 and ec[1] > 0
        for what, flt in (("NULL", None), ("nulls", fr.InstanceFilter()), ("arrays", _keep_all_arrays(sc.n, len(rays)))):
            hits, ids, c = _run(sc, rays, flt, any_hit=any_hit)
            assert hits.tobytes() == exp.tobytes(), f"{kind} {what} any_hit={any_hit}: hits differ from the unfiltered call"
            assert ids.tobytes() == eid.tobytes(), f"{kind} {what} any_hit={any_hit}: instance ids differ"
            assert (c == ec).all(), f"{kind} {what} any_hit={any_hit}: counters {c} vs {ec}"


# ------------------------------------------------------------------ 2: identity instance == rt_intersect_rays_filtered
@pytest.mark.parametrize("name", ("grid", "soup"))
@pytest.mark.parametrize("tree", rq.TREES)
def test_identity_instance_equals_filtered_ray_query(world, name, tree):
    rt = world.rt
    tris, _ = world.scene(name)
    g = world.gpu(name, tree)
    _, entry, _ = ti._blas(world, name, tree)
    sets = rq._ray_sets(tris, seed=31)
    rays = ti._positive_zeros(np.concatenate([sets["outside"].astype(rt.RAY), sets["window"].astype(rt.RAY)]))
    n = len(rays)
    sc = ti.Instanced(rt, [entry], ir.instance_array([np.eye(3, 4)], [0]), "bottom_up")
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    nearest = rq._query(rt, g, rays)[0]["primitive_id"]
    assert (nearest != MISS).sum() > 100
    flat = np.zeros(n, rx.RAY_FILTER)
    flat["mask"], flat["skip_id"] = rx.ALL, nearest
    inst = np.zeros(n, fr.INSTANCE_RAY_FILTER)
    inst["mask"], inst["skip_instance"], inst["skip_id"] = fr.ALL, 0, nearest
    for what, bf, jf in (("cull_back", rx.Filter(rx.CULL_BACK), fr.InstanceFilter(fr.CULL_BACK)),
                         ("cull_front", rx.Filter(rx.CULL_FRONT), fr.InstanceFilter(fr.CULL_FRONT)),
                         ("skip_nearest", rx.Filter(0, 0, None, flat), fr.InstanceFilter(0, 0, None, inst))):
        for any_hit in (False, True):
            exp, ec = _closest(rt, g, rays, bf, any_hit=any_hit)
            hits, ids, c = _run(sc, rays, jf, any_hit=any_hit)
            assert hits.tobytes() == exp.tobytes(), f"{name}/{tree} {what} any_hit={any_hit}: records differ from the BLAS's"
            assert ((ids == 0) == (exp["primitive_id"] != MISS)).all() and ((ids == 0) | (ids == MISS)).all()
            assert c[1] == ec[1], f"{name}/{tree} {what}: triangle tests {c[1]} vs {ec[1]}"
        if what == "skip_nearest":
            assert (hits["primitive_id"] != nearest)[nearest != MISS].all()


# ------------------------------------------------------------------ 3: exact composition
def _per_instance_minimum(comp, sc, rays, flt, any_hit=False):
    """the minimum-t result of rt_intersect_rays_filtered over the entered instances: each instance on its float32 object rays
    (the records' own world_to_object) with its effective filter"""
    rt = comp.rt
    n = len(rays)
    rec = sc.host_records()
    best = np.zeros(n, rt.HIT)
    best["t"], best["primitive_id"] = np.inf, MISS
    best_id = np.full(n, MISS, np.uint32)
    for k in range(comp.inst.size):
        e = comp.entries[int(comp.inst["blas"][k])]
        eff, entered = fr.effective(flt, k, rec["world_to_object"][k], n)
        h, _ = _closest(rt, (ti.Tree(e[0], e[1]), e[2], e[3]), ir.object_rays(rays, rec["world_to_object"][k]), eff)
        take = entered & (h["primitive_id"] != MISS) & (h["t"] < best["t"])
        best[take], best_id[take] = h[take], k
    return best, best_id


@pytest.mark.parametrize("arm,kind", [(a, ti.TLAS_KINDS[i % 3]) for i, a in enumerate(fr.ARMS + ("skip",))])
def test_exact_composition(comp, arm, kind):
    sc = comp.scene(kind)
    rays, flt, ref, unique = comp.arm(arm)
    hits, ids, _ = _run(sc, rays, flt)
    best, best_id = _per_instance_minimum(comp, sc, rays, flt)
    assert hits[unique].tobytes() == best[unique].tobytes(), \
        f"{arm}/{kind}: {np.sum(hits[unique] != best[unique])} records differ from the per-instance minimum"
    assert (ids[unique] == best_id[unique]).all(), f"{arm}/{kind}: instance ids"
    assert (best_id[unique] != MISS).sum() > 100
    base, base_id, _ = _run(sc, rays, UNFILTERED)
    assert ((ids != base_id) | (hits["primitive_id"] != base["primitive_id"])).sum() > 20, f"{arm}: the filter changes too little"
    if arm == "flip_facing":          # FLIP_FACING on the mirror: equal to no mirror flip -- CULL_BACK on the object-space side
        k = fr.MIRROR
        e = comp.entries[0]
        W = sc.host_records()["world_to_object"][k]
        plain, _ = _closest(comp.rt, (ti.Tree(e[0], e[1]), e[2], e[3]), ir.object_rays(rays, W), rx.Filter(rx.CULL_BACK))
        sel = unique & (ids == k)
        assert sel.sum() > 10 and hits[sel].tobytes() == plain[sel].tobytes()
    if arm == "cull_disable":
        cb, cb_id, _ = _run(sc, rays, fr.make_arm("cull_back", comp.inst.size, len(rays)))
        assert (np.isin(ids, fr.DISABLED) & (cb_id != ids)).sum() > 5, "CULL_DISABLE brings back hits cull_back loses"
    if arm == "skip":
        pr = flt.per_ray
        assert not ((ids == pr["skip_instance"]) & (hits["primitive_id"] == pr["skip_id"])).any(), "a ray hit what it skips"
        own = (base_id == pr["skip_instance"]) & (base["primitive_id"] == pr["skip_id"])
        other = unique & (hits["primitive_id"] == pr["skip_id"]) & (ids != pr["skip_instance"]) & (ids != MISS)
        print(f"skip: {own.sum()} of {len(rays)} bounce rays hit their own triangle unfiltered; {other.sum()} unique rays report "
              f"the skipped primitive id in the other copy")
        assert own.sum() > 50 and other.sum() >= 10 and set(ids[other].tolist()) <= set(fr.OVERLAP)
    if arm == "masks":
        got = ids != MISS
        assert (((np.uint32(1) << (ids[got] % fr.GROUPS)) & flt.per_ray["mask"][got]) != 0).all(), "a masked instance was hit"


# ------------------------------------------------------------------ 4: float64 brute force over the kept world triangles
def _check_f64(comp, sc, rays, flt, ref, unique, what, t_ok=None):
    """hit / miss, instance and primitive on the unique rays; t within test_gpu_instances._check_world's bound,
    1e-5 * max(1, t), on the unique rays of `t_ok` (all of them when None); any-hit iff closest-hit"""
    hits, ids, _ = _run(sc, rays, flt)
    got = hits["primitive_id"] != MISS
    assert ((ids != MISS) == got).all(), f"{what}: instance id and primitive id disagree on hit / miss"
    bad = unique & (got != ref["hit"])
    assert not bad.any(), f"{what}: hit / miss differs on {bad.sum()} unique rays (first {np.nonzero(bad)[0][:5]})"
    m = unique & ref["hit"]
    k = ref["tri"][m]
    assert (ids[m] == comp.inst_of[k]).all(), f"{what}: instance"
    assert (hits["primitive_id"][m] == comp.prim_of[k]).all(), f"{what}: primitive"
    ratio = np.zeros(len(rays))
    ratio[m] = np.abs(hits["t"][m] - ref["t"][m]) / (1e-5 * np.maximum(1, ref["t"][m]))
    mt = m if t_ok is None else m & t_ok
    print(f"{what}: {len(rays)} rays, unique {unique.mean():.4f}, hits {got.mean():.2f}; t error / bound: worst {ratio[mt].max():.3f} "
          f"on the {mt.sum()} hits t is checked on; on all {m.sum()} unique hits worst {ratio[m].max():.3f}, {(ratio[m] > 1).sum()} above 1")
    assert (ratio[mt] <= 1).all(), f"{what}: t"
    assert (hits["t"][~got] == np.inf).all()
    assert mt.sum() > 100, f"{what}: too few hits to mean anything"
    a, aid, _ = _run(sc, rays, flt, any_hit=True)
    ah = a["primitive_id"] != MISS
    assert (ah == got).all(), f"{what}: any-hit hits on {ah.sum()} rays, closest-hit on {got.sum()}"
    assert ((a["t"][ah] >= rays["tmin"][ah]) & (a["t"][ah] <= rays["tmax"][ah]) & (a["t"][ah] >= hits["t"][ah])).all()
    return hits, ids


@pytest.mark.parametrize("arm,kind", [(a, ti.TLAS_KINDS[(i + 1) % 3]) for i, a in enumerate(fr.ARMS + ("skip",))])
def test_against_filtered_float64(comp, arm, kind):
    """The bound on t is _check_world's on every arm.  The skip arm's rays start ON a surface, at coordinates of magnitude ~50
    with distances travelled of ~1: there t is checked on the hits whose float32 start point resolves the bound
    (instance_filter_ref.t_resolved, a condition on the inputs; hit / miss, instance and primitive are checked on every
    unique ray).  Measured on the skip arm (714 rays, 308 unique hits): t is checked on 176 hits, worst error 0.28 of the
    bound; over all 308 the worst is 1.77 of the bound, 2 hits above it, both met at |cos| about 0.1.  On the five other arms
    (rays from outside the scene) t is checked on every unique hit: worst 0.04 of the bound."""
    rays, flt, ref, unique = comp.arm(arm)
    t_ok = None
    if arm == "skip":
        t_ok = fr.t_resolved(comp.bounce()[2], ref, rays, 1e-5 * np.maximum(1, ref["t"]))
    _check_f64(comp, comp.scene(kind), rays, flt, ref, unique, f"{arm} TLAS {kind}", t_ok=t_ok)


# ------------------------------------------------------------------ 5: masks save work
def test_a_mask_matching_no_instance_costs_the_tlas_alone(comp):
    import torch
    rt = comp.rt
    rays = comp.rays
    groups = (np.uint32(1) << (np.arange(comp.inst.size, dtype=np.uint32) % fr.GROUPS)).astype(np.uint32)
    for kind in ti.TLAS_KINDS:
        sc = ti.Instanced(rt, comp.entries, comp.inst, kind)      # a private copy: its records are rewritten below
        sc.frame()
        _, _, full = _run(sc, rays, UNFILTERED)
        masked = {}
        for what, flt in (("ray_mask", fr.InstanceFilter(0, 1 << fr.GROUPS, fr.instance_filters(sc.n, masks=groups))),
                          ("instance masks 0", fr.InstanceFilter(0, fr.ALL, fr.instance_filters(sc.n, masks=0)))):
            hits, ids, c = _run(sc, rays, flt)
            assert (hits["primitive_id"] == MISS).all() and (hits["t"] == np.inf).all() and (ids == MISS).all(), f"{kind} {what}"
            assert c[1] == 0, f"{kind} {what}: {c[1]} triangle tests"
            a, aid, ca = _run(sc, rays, flt, any_hit=True)
            assert (aid == MISS).all() and (ca == c).all()
            masked[what] = c
        # the same scene with every instance flagged unusable: the unfiltered call then walks the TLAS alone
        sc.records.view(torch.int32).view(-1, 16)[:, 13] = rt.RT_INSTANCE_SINGULAR
        torch.cuda.synchronize()
        eh, eid, tlas_only = _run(sc, rays, UNFILTERED)
        assert (eid == MISS).all() and tlas_only[1] == 0
        assert set(masked) == {"ray_mask", "instance masks 0"}
        for what, c in masked.items():
            assert c[0] == tlas_only[0], f"{kind} {what}: box tests {c[0]} with every instance masked, {tlas_only[0]} for the TLAS alone"
            assert 0 < c[0] < full[0], f"{kind} {what}: the masked run must cost less than the full one ({c[0]} vs {full[0]})"


@pytest.mark.parametrize("k,kind", ((0, "bottom_up"), (fr.MIRROR, "hybrid"), (fr.SECOND, "sah")))
def test_excluding_an_instance_equals_the_scene_without_it(comp, k, kind):
    rt = comp.rt
    rays = comp.rays
    masks = np.full(comp.inst.size, fr.ALL, np.uint32)
    masks[k] = 0
    flt = fr.InstanceFilter(0, fr.ALL, fr.instance_filters(comp.inst.size, masks=masks))
    ref, unique = fr.brute_force(comp.cand, comp.inst_of, comp.prim_of, rays, flt)
    assert unique.mean() >= 0.95
    hits, ids, c = _run(comp.scene(kind), rays, flt)
    without = ti.Instanced(rt, comp.entries, np.delete(comp.inst, k), kind)
    without.frame()
    exp, eid, ec = _run(without, rays, UNFILTERED)
    eid = np.where((eid != MISS) & (eid >= k), eid + 1, eid).astype(np.uint32)          # the instance indices of the full scene
    assert hits[unique].tobytes() == exp[unique].tobytes(), f"excluding {k}: records differ from the scene without it"
    assert (ids[unique] == eid[unique]).all() and not (ids == k).any()
    _, _, full = _run(comp.scene(kind), rays, UNFILTERED)
    assert c[1] < full[1] and c[0] < full[0], "a masked instance is never entered: fewer tests than the full scene"
    assert (ids[unique] != MISS).sum() > 100


# ------------------------------------------------------------------ 6: edges
@pytest.mark.parametrize("count", (1, 2, 3))
def test_few_instances(comp, count):
    rt = comp.rt
    sub = comp.inst[[0, 6, 2][:count]]
    kind = ti.TLAS_KINDS[count % 3]
    sc = ti.Instanced(rt, comp.entries, sub, kind)
    sc.frame()
    wt, inst_of, prim_of = ir.world_triangles(comp.blas_tris, sub)
    rays = fr.world_rays(wt, 400, 23 + count).astype(rt.RAY)
    cand = fr.candidates(rays, wt)
    n = len(rays)
    per_ray = np.zeros(n, fr.INSTANCE_RAY_FILTER)
    per_ray["mask"] = np.random.default_rng(count).integers(1, 4, n)
    per_ray["skip_instance"], per_ray["skip_id"] = MISS, MISS
    fl = np.zeros(count, np.uint32)
    fl[count - 1] = fr.FLIP_FACING
    for what, flt in (("cull_back", fr.InstanceFilter(fr.CULL_BACK)),
                      ("cull_front + flip + masks", fr.InstanceFilter(fr.CULL_FRONT, 0, fr.instance_filters(
                          count, masks=[3, 1, 2][:count], flags=fl), per_ray))):
        ref, unique = fr.brute_force(cand, inst_of, prim_of, rays, flt)
        assert unique.mean() >= 0.95
        hits, ids, _ = _run(sc, rays, flt)
        got = ids != MISS
        assert not (unique & (got != ref["hit"])).any(), f"{count} instances, {what}: hit / miss"
        m = unique & ref["hit"]
        assert (ids[m] == inst_of[ref["tri"][m]]).all() and (hits["primitive_id"][m] == prim_of[ref["tri"][m]]).all()
        assert (np.abs(hits["t"][m] - ref["t"][m]) <= 1e-5 * np.maximum(1, ref["t"][m])).all()
        assert m.sum() > 20
        a, aid, _ = _run(sc, rays, flt, any_hit=True)
        assert ((aid != MISS) == got).all()


def _combined(comp, n):
    """every part of the filter at once: CULL_BACK, group masks with CULL_DISABLE / FLIP_FACING on some instances, random
    per-ray masks and a skip"""
    rng = np.random.default_rng(5)
    num = comp.inst.size
    fl = np.zeros(num, np.uint32)
    fl[4], fl[fr.MIRROR], fl[1] = fr.CULL_DISABLE, fr.FLIP_FACING, fr.CULL_DISABLE | fr.FLIP_FACING
    per_ray = np.zeros(n, fr.INSTANCE_RAY_FILTER)
    per_ray["mask"] = rng.integers(1, 1 << fr.GROUPS, n)
    per_ray["skip_instance"] = rng.integers(0, num, n)
    per_ray["skip_id"] = rng.integers(0, 1152, n)
    groups = (np.uint32(1) << (np.arange(num, dtype=np.uint32) % fr.GROUPS)).astype(np.uint32)
    return fr.InstanceFilter(fr.CULL_BACK, 0, fr.instance_filters(num, masks=groups, flags=fl), per_ray)


def test_degenerate_rays_batch_edges_and_prefetch(comp):
    import torch
    rt = comp.rt
    sc = comp.scene("bottom_up")
    good = comp.rays[:1000].copy()
    flt = _combined(comp, len(good))
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
    for f in (flt, fr.InstanceFilter(fr.CULL_BACK | fr.CULL_FRONT), fr.InstanceFilter()):
        hits, ids, ctr = _run(sc, deg, f)
        assert (hits["primitive_id"] == MISS).all() and (hits["t"] == np.inf).all() and (ids == MISS).all()
        assert ctr[1] == 0
    ok, oid, _ = _run(sc, good, flt)
    assert 20 < (oid != MISS).sum() < len(good)
    assert (oid[:257] != MISS).sum() > 3
    base, base_id, _ = _run(sc, good, UNFILTERED)
    assert (oid != base_id).sum() > 10
    # the pair-prefetch instantiation gives the same records, filtered
    pf, pid, _ = _run(sc, good, flt, num_primitives=BIG)
    assert pf.tobytes() == ok.tobytes() and (pid == oid).all()
    pa, paid, _ = _run(sc, good, flt, any_hit=True, num_primitives=BIG)
    na, naid, _ = _run(sc, good, flt, any_hit=True)
    assert pa.tobytes() == na.tobytes() and (paid == naid).all()
    assert ((naid != MISS) == (oid != MISS)).all()
    # records past num_rays keep their poison; per_ray is indexed by the ray's index in its batch
    root, count = sc.root
    a = rt._Accel(rt._ptr(sc.tlas.triangles_out), rt._ptr(sc.tlas.nodes_out), root, count)
    hf = _dev_ifilter(rt, flt)
    for n in (1, 63, 65, 257):
        rd = rt.to_device(good[:n])
        hits = torch.full(((n + 64) * 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        idb = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = rt.lib().rt_intersect_rays_instanced_filtered(ctypes.byref(a), rt._ptr(sc.records), sc.n, rt._ptr(sc.table), 2,
                                                           rt._ptr(rd), rt._ptr(hits), rt._ptr(idb), n, 0, 0,
                                                           ctypes.byref(hf._struct(n)), None, rt._stream_ptr(None))
        assert rc == 0
        torch.cuda.synchronize()
        hv, iv = hits.cpu().numpy(), idb.cpu().numpy()
        assert (hv[4 * n:] == 0x5A5A5A5A).all() and (iv[n:] == 0x5A5A5A5A).all(), f"num_rays {n}: records past the batch"
        assert hv[:4 * n].view(np.float32).view(rt.HIT).tobytes() == ok[:n].tobytes(), f"num_rays {n}"
        assert (iv[:n].view(np.uint32) == oid[:n]).all()


def test_short_per_instance_array_and_mask_zero(comp):
    sc = comp.scene("hybrid")
    rays = comp.rays
    num = comp.inst.size
    short = fr.InstanceFilter(0, fr.ALL, fr.instance_filters(3, masks=0))                 # instances 3 .. 6: all ones
    full = fr.InstanceFilter(0, fr.ALL, fr.instance_filters(num, masks=[0, 0, 0] + [fr.ALL] * (num - 3)))
    hs, ids_s, cs = _run(sc, rays, short)
    hf, ids_f, cf = _run(sc, rays, full)
    assert hs.tobytes() == hf.tobytes() and ids_s.tobytes() == ids_f.tobytes() and (cs == cf).all()
    assert not np.isin(ids_s, (0, 1, 2)).any() and (ids_s != MISS).sum() > 100
    assert set(ids_s[ids_s != MISS].tolist()) == {3, 4, 5, 6}
    # num_instance_filters > 0 with a null per_instance: an absent array
    import torch
    rt = comp.rt
    hfilter = rt.InstanceHitFilter()
    st = hfilter._struct(len(rays))
    st.num_instance_filters = 77
    d = rt.to_device(rays).view(torch.float32).view(-1, 8)
    hits = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
    idb = torch.empty(len(rays), dtype=torch.int32, device="cuda")
    root, count = sc.root
    a = rt._Accel(rt._ptr(sc.tlas.triangles_out), rt._ptr(sc.tlas.nodes_out), root, count)
    assert rt.lib().rt_intersect_rays_instanced_filtered(ctypes.byref(a), rt._ptr(sc.records), sc.n, rt._ptr(sc.table), 2, rt._ptr(d),
                                                         rt._ptr(hits), rt._ptr(idb), len(rays), 0, 0, ctypes.byref(st), None,
                                                         rt._stream_ptr(None)) == 0
    torch.cuda.synchronize()
    exp, eid, _ = _run(sc, rays, UNFILTERED)
    assert hits.cpu().numpy().view(rt.HIT).reshape(-1).tobytes() == exp.tobytes() and (idb.cpu().numpy().view(np.uint32) == eid).all()
    # mask 0 on every instance: nothing is entered
    h0, i0, c0 = _run(sc, rays, fr.InstanceFilter(fr.CULL_BACK, fr.ALL, fr.instance_filters(num, masks=0)))
    assert (i0 == MISS).all() and (h0["t"] == np.inf).all() and c0[1] == 0


def test_a_singular_instance_is_never_entered(comp):
    rt = comp.rt
    bad = ir.instance_array([np.zeros((3, 4)), np.eye(3, 4)], [0, 5])                      # singular; a bad BLAS index
    allinst = np.concatenate([comp.inst, bad])
    sc = ti.Instanced(rt, comp.entries, allinst, "bottom_up")
    sc.frame()
    assert rt.instance_status(sc.status) == rt.RT_INSTANCE_SINGULAR | rt.RT_INSTANCE_BAD_BLAS
    rays = comp.rays
    exp, eid, ec = _run(sc, rays, UNFILTERED)
    for flt in (_keep_all_arrays(allinst.size, len(rays)), fr.InstanceFilter()):
        hits, ids, c = _run(sc, rays, flt)
        assert hits.tobytes() == exp.tobytes() and ids.tobytes() == eid.tobytes() and (c == ec).all()
    hits, ids, _ = _run(sc, rays, fr.InstanceFilter(fr.CULL_BACK, fr.ALL, fr.instance_filters(allinst.size, flags=fr.CULL_DISABLE)))
    assert (ids[ids != MISS] < comp.inst.size).all(), "a flagged instance was hit"
    assert hits.tobytes() == exp.tobytes(), "CULL_DISABLE on every instance: nothing is culled"


def test_prepare_build_and_filtered_query_in_a_hip_graph(comp):
    import torch
    rt = comp.rt
    sc = ti.Instanced(rt, comp.entries, comp.inst, "bottom_up")
    rays = rt.to_device(comp.rays[:2000]).view(torch.float32).view(-1, 8)
    n = rays.shape[0]
    num = comp.inst.size
    flt_a = _combined(comp, n)
    flt_b = fr.InstanceFilter(flt_a.flags, 0, flt_a.per_instance.copy(), flt_a.per_ray)
    flt_b.per_instance["mask"] = np.roll(flt_a.per_instance["mask"], 1)
    flt_b.per_instance["flags"] = np.roll(flt_a.per_instance["flags"], 2)
    per_instance = rt.to_device(flt_a.per_instance).view(torch.int32).view(-1, 2)
    per_ray = rt.to_device(flt_a.per_ray).view(torch.int32).view(-1, 4)
    hf = rt.InstanceHitFilter(flt_a.flags, 0, per_instance, per_ray)
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    anyh = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ids_any = torch.empty_like(ids)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    root, count = sc.root

    def one_frame():
        ctr.zero_()
        sc.frame()
        for out, oid, any_hit, c in ((hits, ids, False, ctr), (anyh, ids_any, True, None)):
            rt.IntersectRaysInstancedFiltered(sc.tlas.triangles_out, sc.tlas.nodes_out, root, count, sc.records, sc.n, sc.table,
                                              len(sc.entries), rays, out, oid, hf, any_hit=any_hit, counters=c)

    eager = {}
    for key, flt in (("a", flt_a), ("b", flt_b)):
        per_instance.copy_(rt.to_device(flt.per_instance).view(torch.int32).view(-1, 2))
        one_frame()
        torch.cuda.synchronize()
        eager[key] = [t.clone() for t in (hits, anyh, ids, ids_any, ctr)]
        exp, eid, _ = _run(sc, comp.rays[:2000], flt)
        assert hits.cpu().numpy().view(rt.HIT).reshape(-1).tobytes() == exp.tobytes()
    assert int((eager["a"][2] != -1).sum()) > 100
    assert not torch.equal(eager["a"][2], eager["b"][2]), "the rewritten per_instance must give other answers"

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
        flt = flt_a if key == "a" else flt_b
        per_instance.copy_(rt.to_device(flt.per_instance).view(torch.int32).view(-1, 2))   # rewritten in place: same buffer
        for t in (hits, anyh, ids, ids_any):
            t.fill_(0)
        sc.tlas.nodes_out.zero_()
        sc.records.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip((hits, anyh, ids, ids_any, ctr), eager[key]):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                               exp.view(torch.int32) if exp.dtype == torch.float32 else exp), key
