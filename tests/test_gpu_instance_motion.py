"""GPU tests of instance motion (rt_prepare_motion_instances + a TLAS built over pose 0's proxies and refitted to pose 1's +
rt_intersect_rays_instanced_motion), against tests/instance_motion_ref.py.

1. prepare: both proxy sets byte-equal to the restatement and to rt_prepare_instances run per pose; flags; records; flagged
   instances never hit;
2. identity at both poses, times in {0, 0.25, 0.5, 1}: records byte-equal to rt_intersect_rays, the same triangle tests (grid,
   soup and the deep-stack fractal);
3. exact composition: the minimum over the instances of rt_intersect_rays on the restated float32 object rays, byte for byte,
   with the eight fixed times and with uniformly random ones;
4. float64 brute force per time value (test_gpu_instances._check_world); 5. pose 1 == pose 0; 6. a motion that is singular in
   between; 7. a 65-instance TLAS and rt_motion_validate on it; 8. one to three instances; 9. degenerate rays, bad times, batch
   edges; 10. everything in one HIP graph.
ray_sets() lists the float64-checked ray sets: tests/test_instance_motion_ref_cpu.py holds their unstable share to the cap."""
import numpy as np
import pytest

import instance_motion_ref as imr
import instance_ref as ir
import test_gpu_instances as tgi
import test_gpu_ray_queries as rq

pytestmark = pytest.mark.gpu

TLAS_KINDS = tgi.TLAS_KINDS
F = np.float32
MANY_TIMES = np.array([0.3, 0.77], F)


# ------------------------------------------------------------------ the ray sets (also read by the CPU test)
def _near_rays(world_tris, n, seed):
    """rays aimed at the centroids of random triangles from 30 to 60 units away, within 40 degrees of the triangle's normal,
    half of them with a random t window.  Why not test_gpu_instances._world_rays: the 65 instances lie up to 200 units from
    the origin and their triangles are one unit wide.  The interpolated translation fl(fl(w0 * T0) + fl(tau * T1)) and
    q = fl(o - T) each round at the 1.5e-5 spacing of float32 near 200, so the instance stands up to about 4e-5 away from
    where the float64 reference puts it.  A ray sees that as an error of 4e-5 / (|d| cos(angle to the normal)) in t and of
    4e-5 triangle widths in (u, v).  From outside the whole scene (|o| about 500, three times the spacing) the instancing
    tests' 2e-4 on (u, v) is out of reach for float32 with or without motion, and a grazing ray breaks their 1e-5 on t at
    any distance; |d| >= 30 and cos >= 0.75 towards the aimed-at triangle leave a factor of five under it.  (Measured on an
    MI355X with these rays: t within 3.3e-7 relative, (u, v) within 2.1e-5 of the float64 reference.)"""
    rng = np.random.default_rng(seed)
    V = world_tris.reshape(-1, 3, 3)[rng.integers(0, world_tris.shape[0], n)]
    target = V.mean(axis=1)
    normal = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    g = rng.normal(size=(n, 3))
    g /= np.linalg.norm(g, axis=1)[:, None]
    u = normal * rng.choice([-1.0, 1.0], size=(n, 1)) + 0.6 * g
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = target + u * rng.uniform(30.0, 60.0, size=(n, 1))
    r = np.zeros(n, tgi.RAY)
    r["origin"], r["dir"], r["tmin"], r["tmax"] = o, (target - o) * rng.uniform(1.0, 2.0, size=(n, 1)), 0.0, np.inf
    half = n // 2
    a, b = rng.random(half) * 1.2, rng.random(half) * 1.2
    r["tmin"][:half], r["tmax"][:half] = np.minimum(a, b), np.maximum(a, b)
    return r


def _few(inst, count):
    return inst[[0, 6, 2][:count]]


def _many_rays(blas_tris, many):
    rays, times = [], []
    for k, tau in enumerate(MANY_TIMES):
        rays.append(_near_rays(imr.world_triangles(blas_tris, many, tau)[0], 120, seed=51 + k))
        times.append(np.full(120, tau, F))
    return np.concatenate(rays), np.concatenate(times)


def _half_rays(blas_tris, half):
    return tgi._world_rays(imr.world_triangles(blas_tris, half, 0.25)[0], 400, seed=47)


def ray_sets(blas_tris, inst):
    """(name, instances, rays, times) of every float64-checked run below"""
    rays = tgi._world_rays(imr.union_triangles(blas_tris, inst), 1500, seed=11)
    yield "composition", inst, rays, imr.fixed_times(rays.size, seed=12)
    static = imr.static_instances(inst)
    rays = tgi._world_rays(imr.world_triangles(blas_tris, static, 0.0)[0], 600, seed=13)
    yield "static", static, rays, imr.fixed_times(rays.size, seed=14, values=np.array([0.37], F))
    half = imr.half_turn(inst)
    rays = _half_rays(blas_tris, half)
    yield "half turn", half, rays, np.full(rays.size, 0.25, F)
    many = imr.many_rigid(blas_tris)
    yield ("many",) + (many,) + _many_rays(blas_tris, many)
    for count in (1, 2, 3):
        sub = _few(inst, count)
        rays = tgi._world_rays(imr.union_triangles(blas_tris, sub), 600, seed=23 + count)
        yield f"{count} instances", sub, rays, imr.fixed_times(rays.size, seed=30 + count, values=imr.TIMES[[1, 4, 6]])


# ------------------------------------------------------------------ scene plumbing
class Moving:
    """device buffers of one scene of moving instances: BLAS table, instances, both proxy sets, records, status, both TLAS poses"""

    def __init__(self, rt, blas_entries, instances, tlas="bottom_up"):
        import torch
        self.rt, self.kind = rt, tlas
        self.n = instances.size
        self.entries = list(blas_entries)
        self.table = rt.accel_table(self.entries)
        self.instances = rt.to_device(np.ascontiguousarray(instances))
        self.tlas = rt.BuildInput.allocate(np.zeros((max(self.n, 1), 9), np.float32), sah=tlas == "sah")
        self.tlas.num_triangles = self.n
        self.proxies1 = torch.zeros_like(self.tlas.triangles_in)
        self.pose1 = rt.BuildInput(triangles_in=self.proxies1, triangles_out=torch.zeros_like(self.tlas.triangles_out),
                                   num_triangles=self.n, nodes_out=torch.zeros_like(self.tlas.nodes_out), scratch=self.tlas.scratch)
        self.plan = rt.device_bytes(rt.RefitPlanBytes(max(self.n, 1)))
        self.records = torch.zeros(max(self.n, 1) * 128, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(4, dtype=torch.uint8, device="cuda")

    root = tgi.Instanced.root

    def prepare(self):
        self.rt.PrepareMotionInstances(self.instances, self.n, self.table, len(self.entries), self.tlas.triangles_in,
                                       self.proxies1, self.records, self.status)

    def frame(self):
        """prepare, the TLAS over proxies0, its byte copy, the copy refitted with proxies1 through a plan of its own"""
        rt = self.rt
        self.prepare()
        tgi.Instanced.build(self)
        self.pose1.triangles_out.copy_(self.tlas.triangles_out)
        self.pose1.nodes_out.copy_(self.tlas.nodes_out)
        root, count = self.root
        rt.BuildRefitPlan(self.pose1, root, count, self.plan)
        rt.Refit(self.pose1, root, count, self.plan)

    def query(self, rays, times, hits, ids, any_hit=False, counters=None):
        root, count = self.root
        self.rt.IntersectRaysInstancedMotion(self.tlas, self.pose1, root, count, self.records, self.n, self.table,
                                             len(self.entries), rays, times, hits, ids, any_hit=any_hit, counters=counters)

    def run(self, rays, times, any_hit=False, counters=False):
        """numpy RAY array, float32 times -> (HIT array, instance ids, counters)"""
        import torch
        rt = self.rt
        d = rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)
        n = d.shape[0]
        td = torch.from_numpy(np.broadcast_to(np.asarray(times, F), (n,)).copy()).cuda()
        hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        ids = torch.empty(n, dtype=torch.int32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda") if counters else None
        self.query(d, td, hits, ids, any_hit=any_hit, counters=ctr)
        torch.cuda.synchronize()
        return (hits.cpu().numpy().view(rt.HIT).reshape(-1), ids.cpu().numpy().view(np.uint32),
                ctr.cpu().numpy().astype(np.uint64) if counters else None)

    def at(self, tau):
        return _AtTime(self, tau)

    def host(self, buf, dtype, count):
        return self.rt.to_host(buf, dtype, count)


class _AtTime:
    """a Moving scene with every ray at one time: what test_gpu_instances._check_world drives"""

    def __init__(self, sc, tau):
        self.sc, self.tau = sc, F(tau)

    def run(self, rays, any_hit=False, num_primitives=0, counters=False):
        return self.sc.run(rays, self.tau, any_hit=any_hit, counters=counters)


@pytest.fixture(scope="module")
def world(rt, scenes, ora):
    return rq.World(rt, scenes, ora)


@pytest.fixture(scope="module")
def comp(world):
    """(blas triangles, table entries, root boxes, MOTION_INSTANCE array): test_gpu_instances._composition is pose 0"""
    blas_tris, entries, boxes, inst0 = tgi._composition(world)
    tris, minst = imr.composition(world.scenes)
    assert all((a == b).all() for a, b in zip(blas_tris, tris))
    assert (minst["object_to_world0"] == inst0["object_to_world"]).all() and (minst["blas"] == inst0["blas"]).all()
    return blas_tris, entries, boxes, minst


def _scene(rt, comp, inst, kind):
    sc = Moving(rt, comp[1], inst, kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    assert rt.refit_status(sc.plan, sc.n) == 0
    return sc


def _check_by_time(sc, blas_tris, inst, rays, times, what):
    """check 4: the mixed-time batch equals its per-time parts, and every part passes _check_world at its time"""
    hits, ids, _ = sc.run(rays, times)
    for tau in np.unique(times):
        sel = times == tau
        wt, inst_of, prim_of = imr.world_triangles(blas_tris, inst, tau)
        h, i = tgi._check_world(sc.at(tau), wt, inst_of, prim_of, rays[sel], f"{what} at {tau:g}")
        assert h.tobytes() == hits[sel].tobytes() and (i == ids[sel]).all(), f"{what}: a ray's result depends on its batch"
    return hits, ids


def _set(comp, name):
    return next(s for s in ray_sets(comp[0], comp[3]) if s[0] == name)[1:]


# ------------------------------------------------------------------ 1: prepare
def test_prepare_bit_exact_and_flags(world, comp):
    rt = world.rt
    blas_tris, entries, boxes, inst = comp
    eye, nan, zero, mirror = np.eye(3, 4), np.eye(3, 4), np.zeros((3, 4)), np.diag([-1.0, 1.0, 1.0, 0.0])[:3]
    nan = nan.copy()
    nan[1, 2] = np.nan
    bad = imr.motion_instance_array([eye, eye, eye, nan, eye, zero, eye, mirror], [eye, eye, nan, eye, zero, eye, mirror, eye],
                                    [5, 2, 0, 0, 0, 0, 0, 0])
    allinst = np.concatenate([inst, bad, imr.half_turn(inst)])
    entries = entries + [(entries[0][0], entries[0][1], 0, 0)]     # table entry 2: an empty tree (count 0) -- a bad BLAS
    boxes = boxes + [None]
    prox0, prox1, flags = imr.prepare(allinst, boxes)
    assert flags.tolist() == [0] * inst.size + [1, 1, 2, 2, 2, 2, 2, 2] + [0]
    sc = Moving(rt, entries, allinst)
    sc.frame()
    assert rt.instance_status(sc.status) == rt.RT_INSTANCE_BAD_BLAS | rt.RT_INSTANCE_SINGULAR
    got0 = sc.host(sc.tlas.triangles_in, np.float32, 9 * sc.n).reshape(-1, 9)
    got1 = sc.host(sc.proxies1, np.float32, 9 * sc.n).reshape(-1, 9)
    assert got0.tobytes() == prox0.tobytes() and got1.tobytes() == prox1.tobytes(), "proxies differ from the restatement"
    ok = flags == 0
    for key, got in (("object_to_world0", got0), ("object_to_world1", got1)):
        one = tgi.Instanced(rt, entries, ir.instance_array(list(allinst[key][ok]), list(allinst["blas"][ok])))
        one.prepare()
        assert one.host_proxies().tobytes() == got[ok].tobytes(), f"{key}: proxies differ from rt_prepare_instances's"
    assert (got0[~ok] == 0).all() and (got1[~ok] == 0).all()
    rec = sc.host(sc.records, rt.MOTION_INSTANCE_RECORD, sc.n)
    for key in ("object_to_world0", "object_to_world1"):
        assert rec[key].tobytes() == allinst[key].tobytes()
    assert (rec["flags"] == flags).all() and (rec["blas"] == allinst["blas"]).all() and (rec["spare"] == 0).all()
    # flagged instances are never hit, even by rays aimed straight at the geometry they would place
    rays = tgi._world_rays(imr.union_triangles(blas_tris, inst), 600, seed=7)
    hits, ids, _ = sc.run(rays, imr.fixed_times(rays.size, seed=8))
    hit = ids != 0xFFFFFFFF
    assert ok[ids[hit]].all(), "a flagged instance was hit"
    assert hit.sum() > 50


# ------------------------------------------------------------------ 2: identity at both poses == rt_intersect_rays
@pytest.mark.parametrize("name", ("grid", "soup", "fractal"))
@pytest.mark.parametrize("tree", rq.TREES)
def test_identity_instance_equals_intersect_rays(world, name, tree):
    rt = world.rt
    tris, cam = world.scene(name)
    _, entry, _ = tgi._blas(world, name, tree)
    sets = rq._ray_sets(tris, seed=31)
    cam_rays = rq._camera_rays(rt, cam, rq.W, rq.H, 1, True).cpu().numpy().view(rt.RAY).reshape(-1)
    rays = tgi._positive_zeros(np.concatenate([sets["outside"].astype(rt.RAY), sets["window"].astype(rt.RAY), cam_rays]))
    times = np.array([0, 0.25, 0.5, 1], F)[np.arange(rays.size) % 4]
    exp, ec = rq._query(rt, world.gpu(name, tree), rays, counters=True)
    sc = Moving(rt, [entry], imr.motion_instance_array([np.eye(3, 4)], [np.eye(3, 4)], [0]))
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    hits, ids, c = sc.run(rays, times, counters=True)
    assert hits.tobytes() == exp.tobytes(), f"{name}/{tree}: records differ from rt_intersect_rays"
    assert ((ids == 0) == (exp["primitive_id"] != 0xFFFFFFFF)).all() and ((ids == 0) | (ids == 0xFFFFFFFF)).all()
    assert c[1] == ec[1], f"{name}/{tree}: triangle tests {c[1]} vs {ec[1]}"
    assert c[0] > 0
    a, _, _ = sc.run(rays, times, any_hit=True)
    ea, _ = rq._query(rt, world.gpu(name, tree), rays, any_hit=True)
    assert a.tobytes() == ea.tobytes(), f"{name}/{tree}: any-hit records differ"


# ------------------------------------------------------------------ 3: exact composition
_REF = {}


def _per_instance(rt, entries, inst, rays, times):
    """rt_intersect_rays per instance on the restated float32 object rays: (best HIT, best instance, second-best t)"""
    key = (rays.tobytes(), times.tobytes())
    if key not in _REF:
        best = np.zeros(rays.size, rt.HIT)
        best["t"], best["primitive_id"] = np.inf, 0xFFFFFFFF
        best_id = np.full(rays.size, 0xFFFFFFFF, np.uint32)
        second = np.full(rays.size, np.inf, np.float32)
        for k in range(inst.size):
            e = entries[int(inst["blas"][k])]
            obj, entered = imr.object_rays(rays.astype(rt.RAY), times, inst["object_to_world0"][k], inst["object_to_world1"][k])
            assert entered.all()
            h, _ = rq._query(rt, (tgi.Tree(e[0], e[1]), e[2], e[3]), obj)
            got = h["primitive_id"] != 0xFFFFFFFF
            take = got & (h["t"] < best["t"])
            second = np.where(take, best["t"], np.where(got, np.minimum(second, h["t"]), second))
            best[take], best_id[take] = h[take], k
        _REF[key] = best, best_id, second
    return _REF[key]


def _stable_f64(blas_tris, inst, rays, times, best_id):
    """the rays whose float64 answer at their time is stable and belongs to the instance the per-instance minimum chose"""
    key = ("f64", rays.tobytes(), times.tobytes())
    if key not in _REF:
        out = np.zeros(rays.size, bool)
        for tau in np.unique(times):
            sel = np.nonzero(times == tau)[0]
            wt, inst_of, _ = imr.world_triangles(blas_tris, inst, tau)
            ref = tgi._f64_world(wt, rays[sel])
            out[sel] = ref["stable"] & tgi._window_ok(wt, rays[sel], ref) & \
                np.where(ref["hit"], best_id[sel] == inst_of[np.maximum(ref["tri"], 0)], True)
        _REF[key] = out
    return _REF[key]


@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_exact_composition(world, comp, kind):
    rt = world.rt
    blas_tris, entries, _, inst = comp
    sc = _scene(rt, comp, inst, kind)
    _, rays, times = _set(comp, "composition")
    random_times = np.random.default_rng(15).random(rays.size).astype(F)
    for what, tm in (("fixed times", times), ("random times", random_times)):
        hits, ids, _ = sc.run(rays, tm)
        best, best_id, second = _per_instance(rt, entries, inst, rays, tm)
        if what == "fixed times":
            unique = _stable_f64(blas_tris, inst, rays, tm, best_id)
        else:   # no float64 world per ray: the two nearest instances' t differ by more than 1e-4 relative
            gap = np.where(second == np.inf, np.inf, second) - np.where(best_id != 0xFFFFFFFF, best["t"], 0)
            unique = ~((best_id != 0xFFFFFFFF) & (gap <= 1e-4 * np.maximum(1, best["t"])))
        assert unique.mean() > 0.97, f"{what}: unique fraction {unique.mean():.3f}"
        assert hits[unique].tobytes() == best[unique].tobytes(), \
            f"{kind}, {what}: {np.sum(hits[unique] != best[unique])} records differ from the per-instance minimum"
        assert (ids[unique] == best_id[unique]).all()
        assert (best_id[unique] != 0xFFFFFFFF).sum() > 200 and len(set(best_id[unique].tolist()) - {0xFFFFFFFF}) >= 5


# ------------------------------------------------------------------ 4: float64 brute force, per time value
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_against_float64(world, comp, kind):
    inst, rays, times = _set(comp, "composition")
    sc = _scene(world.rt, comp, inst, kind)
    _check_by_time(sc, comp[0], inst, rays, times, f"composition TLAS {kind}")


# ------------------------------------------------------------------ 5: pose 1 == pose 0
def test_static_scene(world, comp):
    inst, rays, times = _set(comp, "static")
    sc = _scene(world.rt, comp, inst, "bottom_up")
    _check_by_time(sc, comp[0], inst, rays, times, "static scene")


# ------------------------------------------------------------------ 6: singular in between
def test_singular_in_between(world, comp):
    rt = world.rt
    inst, rays, times = _set(comp, "half turn")
    sc = _scene(rt, comp, inst, "bottom_up")            # (status 0: not flagged)
    hits, ids, c = sc.run(rays, 0.5, counters=True)
    assert (ids == rt.MISS).all() and (hits["primitive_id"] == rt.MISS).all() and (hits["t"] == np.inf).all()
    assert c[1] == 0 and c[0] > 0, "at time 0.5 the instance is reached in the TLAS and never entered"
    _check_by_time(sc, comp[0], inst, rays, times, "half turn")


# ------------------------------------------------------------------ 7: a 65-instance TLAS
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_many_instances_and_validate(world, comp, kind):
    import torch
    rt = world.rt
    inst, rays, times = _set(comp, "many")
    sc = _scene(rt, comp, inst, kind)
    _check_by_time(sc, comp[0], inst, rays, times, f"65 instances TLAS {kind}")
    root, count = sc.root
    status = torch.full((1,), 0x77, dtype=torch.int32, device="cuda")
    rt.MotionValidate(sc.tlas, sc.pose1, root, count, sc.n, status)
    assert rt.motion_status(status) == 0
    nodes = sc.pose1.nodes_out.clone()
    nodes.view(torch.uint8)[32 * (root + 1) + 28] ^= 1           # one w28 word of pose 1
    rt.MotionValidate(sc.tlas, (sc.pose1.triangles_out, nodes), root, count, sc.n, status)
    assert rt.motion_status(status) == rt.RT_MOTION_TOPOLOGY_MISMATCH


# ------------------------------------------------------------------ 8: one to three instances
@pytest.mark.parametrize("count", (1, 2, 3))
@pytest.mark.parametrize("kind", TLAS_KINDS)
def test_few_instances(world, comp, count, kind):
    inst, rays, times = _set(comp, f"{count} instances")
    sc = _scene(world.rt, comp, inst, kind)
    _check_by_time(sc, comp[0], inst, rays, times, f"{count} instances TLAS {kind}")


# ------------------------------------------------------------------ 9: edges
def test_degenerate_rays_bad_times_and_batch_edges(world, comp):
    import ctypes
    import torch
    rt = world.rt
    blas_tris, _, _, inst = comp
    sc = _scene(rt, comp, inst, "bottom_up")
    good = tgi._world_rays(imr.union_triangles(blas_tris, inst), 500, seed=29).astype(rt.RAY)
    times = imr.fixed_times(good.size, seed=28)
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
    hits, ids, ctr = sc.run(deg, times[:8], counters=True)
    assert (hits["primitive_id"] == rt.MISS).all() and (hits["t"] == np.inf).all() and (ids == rt.MISS).all()
    assert ctr[1] == 0
    ok, oid, _ = sc.run(good, times)
    assert (oid != rt.MISS).sum() > 100
    # a time that is NaN or outside [0, 1]: a miss, nothing tested -- for rays that hit at a valid time
    hitters = good[oid != rt.MISS][:60]
    for bad in (nan, -0.1, 1.0001, np.inf, -np.inf):
        for any_hit in (False, True):
            h, i, c = sc.run(hitters, F(bad), any_hit=any_hit, counters=True)
            assert (h["primitive_id"] == rt.MISS).all() and (h["t"] == np.inf).all() and (h["u"] == 0).all() and (i == rt.MISS).all()
            assert c[0] == 0 and c[1] == 0, f"time {bad}: tests were counted"
    mixed = np.where(np.arange(hitters.size) % 2 == 0, times[:hitters.size], nan).astype(F)
    h, i, _ = sc.run(hitters, mixed)
    assert (i[1::2] == rt.MISS).all() and (i[0::2] != rt.MISS).sum() > 0
    # records past num_rays keep their poison; a null counters pointer is accepted
    root, count = sc.root
    a = rt._motion_accel(sc.tlas, sc.pose1, root, count)
    for n in (1, 63, 65, 1001):
        reps = (n + good.size - 1) // good.size
        rd = rt.to_device(np.tile(good, reps)[:n])
        td = torch.from_numpy(np.tile(times, reps)[:n].copy()).cuda()
        hits = torch.full(((n + 64) * 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        idb = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = rt.lib().rt_intersect_rays_instanced_motion(ctypes.byref(a), rt._ptr(sc.records), sc.n, rt._ptr(sc.table), 2,
                                                         rt._ptr(rd), rt._ptr(td), rt._ptr(hits), rt._ptr(idb), n, 0, None,
                                                         rt._stream_ptr(None))
        assert rc == 0
        torch.cuda.synchronize()
        hv, iv = hits.cpu().numpy(), idb.cpu().numpy()
        assert (hv[4 * n:] == 0x5A5A5A5A).all() and (iv[n:] == 0x5A5A5A5A).all(), f"num_rays {n}: records past the batch"
        assert hv[:4 * n].view(np.float32).view(rt.HIT).tobytes() == np.tile(ok, reps)[:n].tobytes()
        assert (iv[:n].view(np.uint32) == np.tile(oid, reps)[:n]).all()


# ------------------------------------------------------------------ 10: hipGraph
def test_everything_in_a_hip_graph(world, comp):
    import torch
    rt = world.rt
    blas_tris, _, _, inst = comp
    sc = Moving(rt, comp[1], inst, "bottom_up")
    rays_np = tgi._world_rays(imr.union_triangles(blas_tris, inst), 1000, seed=37).astype(rt.RAY)
    rays = rt.to_device(rays_np).view(torch.float32).view(-1, 8)
    n = rays.shape[0]
    times = torch.from_numpy(imr.fixed_times(n, seed=38)).cuda()
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    anyh = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ids_any = torch.empty_like(ids)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")

    def one_frame():
        ctr.zero_()
        sc.frame()
        sc.query(rays, times, hits, ids, counters=ctr)
        sc.query(rays, times, anyh, ids_any, any_hit=True)

    moved = inst.copy()
    for key in ("object_to_world0", "object_to_world1"):
        moved[key][:, :, 3] += np.float32(0.05) * np.arange(inst.size, dtype=np.float32)[:, None]
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
        sc.pose1.nodes_out.zero_()
        sc.records.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip((hits, anyh, ids, ids_any, ctr), eager[key]):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                               exp.view(torch.int32) if exp.dtype == torch.float32 else exp), key
