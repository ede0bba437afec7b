"""GPU tests of the traversal-stack edges of the motion, sphere and instanced ray queries (rt_intersect_rays_motion, _spheres,
_instanced, _instanced_filtered, _instanced_motion): the LDS / private boundary at level 16, a full 64-entry stack, and -- for
the two-level kernels -- a BLAS entered with the stack bottom above 0, at, across and far above level 16.

Every comparison is against the oracle's ordered per-ray walkers (oracle/rt_oracle.c, ora_walk_rays*), which drop the pushes
trace_ray drops, run on the tree BYTES the kernel was given: records and instance ids bit for bit, counters[0:2] equal to the
walker's sums.  counters[2:4] (vote and leaf-phase counts) depend on wave scheduling and are not compared.  The inputs are
tests/stack_scenes.py's; tests/test_stack_walk_ref_cpu.py checks the walkers and holds every input to the condition that makes
it a test of its level (repeated here on the device's own trees, from the walker's per-ray depth and drop counts)."""
import collections

import numpy as np
import pytest

import instance_filter_ref as ifr
import instance_motion_ref as imr
import instance_ref as ir
import stack_scenes as sc
import test_gpu_instance_filter as tgf
import test_gpu_instance_motion as tgm
import test_gpu_instances as tgi
import test_gpu_ray_queries as rq
import test_gpu_spheres as tgs

pytestmark = pytest.mark.gpu

F = np.float32
DEPTH, DROPPED, LOW, HIGH = 2, 3, 4, 5
TAUS = np.array(sc.TAUS, F)


# ------------------------------------------------------------------ plumbing
def _dev_rays(rt, rays):
    import torch
    return rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)


def _host_tree(rt, inp):
    return rt.to_host(inp.triangles_out, rt.TRIANGLE_PAIR), rt.to_host(inp.nodes_out, rt.NODE)


def _launch(rt, n, call, ids=False):
    """call(hits, counters[, ids]) -> (HIT [n], counters uint64 [4][, instance ids])"""
    import torch
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    idb = torch.empty(n, dtype=torch.int32, device="cuda")
    if ids:
        call(hits, ctr, idb)
    else:
        call(hits, ctr)
    torch.cuda.synchronize()
    out = (hits.cpu().numpy().view(rt.HIT).reshape(-1), ctr.cpu().numpy().astype(np.uint64))
    return out + (idb.cpu().numpy().view(np.uint32),) if ids else out


def _check(got, ctr, exp, st, what, ids=None, exp_ids=None):
    bad = got.view(np.dtype((np.void, 16))) != exp.view(np.dtype((np.void, 16)))
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} records differ from the walker's (first: ray {np.nonzero(bad)[0][:5]})"
    if ids is not None:
        assert (ids == exp_ids).all(), f"{what}: instance ids differ on {(ids != exp_ids).sum()} rays"
    sums = st[:, :2].sum(axis=0, dtype=np.uint64)
    assert (ctr[:2] == sums).all(), f"{what}: counters {ctr[:2]} vs the walker's sums {sums}"


def _report(what, st):
    print(f"{what}: greatest depth {int(st[:, DEPTH].max())}, dropped pushes {int(st[:, DROPPED].sum())}"
          + (f", depth inside instances entered below 16: {int(st[:, LOW].max())}, dropped inside instances entered above 16: "
             f"{int(st[:, HIGH].sum())}" if st.shape[1] > 4 else ""))


def _deep(st):
    return ((st[:, DEPTH] >= 17) & (st[:, DEPTH] <= 63) & (st[:, DROPPED] == 0)).any()


def _over_taus(rays):
    """every ray at every time of TAUS: (rays [4 n], times [4 n])"""
    return np.tile(rays, len(TAUS)), np.repeat(TAUS, len(rays))


Pose = collections.namedtuple("Pose", "triangles_out nodes_out")


def _Pose(rt, leaves, nodes):
    """an uploaded hand-made tree: the (triangles, nodes) pair the queries take, with a BuildInput's names"""
    return Pose(rt.to_device(leaves), rt.to_device(nodes))


@pytest.fixture(scope="module")
def fractals(rt, scenes):
    """name, kind -> (tris, cam, BuildInput, root, count, host leaves, host nodes), built once on the device"""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            tris, cam = sc.fractal(name, scenes)
            inp, root, count = rq._gpu_tree(rt, tris, "sah" if kind == "sah" else "bottom_up")
            cache[name, kind] = (tris, cam, inp, root, count) + _host_tree(rt, inp)
        return cache[name, kind]
    return get


FRACTALS = (("deep", "lbvh"), ("deep", "sah"), ("full", "sah"), ("dense", "sah"))


# ------------------------------------------------------------------ the anchor: rt_intersect_rays, already pinned
def test_anchor_intersect_rays_on_the_full_stack_fractal(rt, ora, fractals):
    tris, cam, inp, root, count, leaves, nodes = fractals("full", "sah")
    w, h = sc.FRAME
    dev = rq._camera_rays(rt, cam, w, h, 1, False)
    rays = dev.cpu().numpy().view(rt.RAY).reshape(-1)
    assert rays.tobytes() == sc.camera_rays_f32(cam, w, h).tobytes(), "the float32 restatement of the ray generator"
    _, oc = ora.trace(leaves, nodes, root, count, cam, w, h)
    for any_hit in (False, True):
        exp, st = ora.walk_rays(leaves, nodes, root, count, rays, any_hit=any_hit)
        got, ctr = rq._query(rt, (inp, root, count), dev, any_hit=any_hit, counters=True)
        _check(got, ctr, exp, st, f"IntersectRays any_hit={any_hit}")
        if not any_hit:
            _report("IntersectRays full/sah", st)
            assert int(st[:, DEPTH].max()) == int(oc[2]) == sc.STACK and int(st[:, DROPPED].sum()) == int(oc[3]) > 0
            assert (st[:, :2].sum(axis=0, dtype=np.uint64) == oc[:2]).all()


# ------------------------------------------------------------------ rt_intersect_rays_motion
def _motion(rt, ora, pose0, pose1, host0, host1, root, count, rays, what):
    """both modes over every time of TAUS -> the closest-hit walker records and stats, one block of len(rays) rows per time"""
    import torch
    r4, t4 = _over_taus(rays)
    d, td = _dev_rays(rt, r4), torch.from_numpy(t4).cuda()
    out = None
    for any_hit in (False, True):
        exp, st = ora.walk_rays_motion(host0[0], host0[1], host1[0], host1[1], root, count, r4, t4, any_hit=any_hit)
        got, ctr = _launch(rt, len(r4), lambda hits, c: rt.IntersectRaysMotion(pose0, pose1, root, count, d, td, hits,
                                                                              any_hit=any_hit, counters=c))
        _check(got, ctr, exp, st, f"IntersectRaysMotion {what} any_hit={any_hit}")
        assert (exp["primitive_id"] != sc.MISS).sum() >= sc.AIMED
        out = (exp, st) if out is None else out
    _report(f"IntersectRaysMotion {what}", out[1])
    return out


@pytest.mark.parametrize("L", sc.COMB_L)
def test_motion_triangle_combs(rt, ora, L):
    c = sc.tri_comb(L)
    _, st = _motion(rt, ora, _Pose(rt, c["leaves0"], c["nodes0"]), _Pose(rt, c["leaves1"], c["nodes1"]), (c["leaves0"], c["nodes0"]),
                    (c["leaves1"], c["nodes1"]), c["root"], c["count"], sc.comb_rays(c["aim"], seed=31 + L), f"comb {L}")
    depth, dropped = sc.expect_comb(L)
    assert (st[:, DEPTH] == depth).all() and (st[:, DROPPED] == dropped).all()


@pytest.mark.parametrize("name,kind", FRACTALS)
def test_motion_fractals(rt, ora, fractals, name, kind):
    import torch
    tris, cam, inp, root, count, leaves, nodes = fractals(name, kind)
    pose1, plan1 = rt.MotionPose(inp, root, count, sc.moved_fractal(tris))
    torch.cuda.synchronize()
    assert rt.refit_status(plan1, inp.num_triangles) == 0
    rays = sc.fractal_rays(name, tris, cam)
    l1, n1 = _host_tree(rt, pose1)
    exp, st = _motion(rt, ora, inp, pose1, (leaves, nodes), (l1, n1), root, count, rays, f"{name}/{kind}")
    for tau, hits, block in zip(TAUS, np.split(exp, len(TAUS)), np.split(st, len(TAUS))):
        if name == "deep":
            assert _deep(block) and (block[:, DROPPED] == 0).all()
            continue
        dropped = block[:, DROPPED] > 0
        assert dropped.any() and block[:, DEPTH].max() == sc.STACK
        if name == "dense":
            # the records the kernel had to match are not the brute-force closest hits: the drop rule is observable
            brute = sc.brute_leaves_t(leaves, rays, l1, tau)
            free, _ = ora.walk_rays_motion(leaves, nodes, l1, n1, root, count, rays, np.full(len(rays), tau, F), stack_limit=1024)
            gone = dropped & (hits["t"] != brute) & (free["t"] == brute)
            print(f"    time {tau}: {dropped.sum()} rays dropped a push, {gone.sum()} of them lost the brute-force hit")
            assert gone.any() and (hits["t"][gone] > brute[gone]).all()


# ------------------------------------------------------------------ rt_intersect_rays_spheres
def _spheres(rt, ora, dev_tree, host_tree, root, count, spheres, rays, what):
    """closest, any-hit and the indexed instantiation -> the closest-hit walker records and stats"""
    import torch
    d = _dev_rays(rt, rays)
    n = len(rays)
    sp = rt.to_device(np.ascontiguousarray(spheres, F))
    query = lambda hits, c, **kw: rt.IntersectRaysSpheres(dev_tree[0], dev_tree[1], root, count, sp, len(spheres), d, hits,
                                                           counters=c, **kw)
    out = None
    for any_hit in (False, True):
        exp, st = ora.walk_rays_spheres(host_tree[0], host_tree[1], root, count, spheres, rays, any_hit=any_hit)
        got, ctr = _launch(rt, n, lambda hits, c: query(hits, c, any_hit=any_hit))
        _check(got, ctr, exp, st, f"IntersectRaysSpheres {what} any_hit={any_hit}")
        out = (exp, st) if out is None else out
    exp, st = out
    assert (exp["primitive_id"] != sc.MISS).sum() >= sc.AIMED
    # indexed: a permutation of two thirds of the rays; the others keep their sentinel
    perm = np.random.default_rng(3).permutation(n)[: 2 * n // 3].astype(np.uint32)
    order = torch.from_numpy(perm.view(np.int32)).cuda()
    hits = torch.full((n, 4), 0, dtype=torch.int32, device="cuda").fill_(0x5A5A5A5A)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    query(hits, ctr, order=order)
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(rt.HIT).reshape(-1)
    listed = np.zeros(n, bool)
    listed[perm] = True
    assert got[listed].tobytes() == exp[listed].tobytes(), f"IntersectRaysSpheres {what}: indexed records differ"
    assert (got[~listed].view(np.uint32) == 0x5A5A5A5A).all(), "unlisted records were written"
    assert (ctr.cpu().numpy().astype(np.uint64)[:2] == st[listed, :2].sum(axis=0, dtype=np.uint64)).all()
    _report(f"IntersectRaysSpheres {what}", st)
    return exp, st


@pytest.mark.parametrize("L", sc.COMB_L)
def test_sphere_combs(rt, ora, L):
    c = sc.sphere_comb(L)
    pose = _Pose(rt, c["leaves"], c["nodes"])
    _, st = _spheres(rt, ora, (pose.triangles_out, pose.nodes_out), (c["leaves"], c["nodes"]), c["root"], c["count"], c["spheres"],
                     sc.comb_rays(c["aim"], seed=37 + L), f"comb {L}")
    depth, dropped = sc.expect_comb(L)
    assert (st[:, DEPTH] == depth).all() and (st[:, DROPPED] == dropped).all()


@pytest.mark.parametrize("name,kind", [("deep", k) for k in tgs.KINDS] + [("full", "sah")])
def test_sphere_fractals(rt, ora, scenes, name, kind):
    """deep: every builder; full: the SAH builder's tree alone fills the stack (tests/test_stack_walk_ref_cpu.py)"""
    tris, cam = sc.fractal(name, scenes)
    spheres = sc.fractal_spheres(tris, name)
    s = tgs.Spheres(rt, spheres, kind).frame()
    assert rt.sphere_status(s.status) == 0
    root, count = s.root
    leaves, nodes = _host_tree(rt, s.tree)
    rays = sc.sphere_rays(name, spheres, cam)
    exp, st = _spheres(rt, ora, (s.tree.triangles_out, s.tree.nodes_out), (leaves, nodes), root, count, spheres, rays, f"{name}/{kind}")
    if name == "deep":
        assert _deep(st) and (st[:, DROPPED] == 0).all()
        return
    dropped = st[:, DROPPED] > 0
    assert dropped.any() and st[:, DEPTH].max() == sc.STACK
    brute = sc.brute_spheres_t(spheres, rays)
    free, _ = ora.walk_rays_spheres(leaves, nodes, root, count, spheres, rays, stack_limit=1024)
    gone = dropped & (exp["t"] != brute) & (free["t"] == brute)
    print(f"    {dropped.sum()} rays dropped a push, {gone.sum()} of them lost the brute-force hit")
    assert gone.any() and (exp["t"][gone] > brute[gone]).all()


# ------------------------------------------------------------------ the two-level kernels
class _TwoLevel:
    """a hand-made comb TLAS over instances of one BLAS (table entry 0; entry 1 is an empty tree: a bad BLAS): the device buffers,
    the device's own records read back, and what the walker needs"""

    def __init__(self, rt, tlas, mats0, mats1, blas_of, blas_dev, blas_host, root, count):
        self.rt, self.tlas, self.K = rt, tlas, len(mats0)
        self.entries = [(blas_dev[0], blas_dev[1], root, count), (blas_dev[0], blas_dev[1], 0, 0)]
        self.counts = [count, 0]
        self.trees = [blas_host + (root, count)] * self.K
        self.pose0, self.pose1 = _Pose(rt, tlas["leaves"], tlas["nodes0"]), _Pose(rt, tlas["leaves"], tlas["nodes1"])
        self.static = tgi.Instanced(rt, self.entries, ir.instance_array(mats0, blas_of))
        self.static.prepare()
        self.moving = tgm.Moving(rt, self.entries, imr.motion_instance_array(mats0, mats1, blas_of))
        self.moving.prepare()
        bad = rt.RT_INSTANCE_BAD_BLAS if np.any(blas_of) else 0
        assert rt.instance_status(self.static.status) == bad and rt.instance_status(self.moving.status) == bad
        self.records = self.static.host_records()
        self.motion_records = rt.to_host(self.moving.records, rt.MOTION_INSTANCE_RECORD, self.K)

    def walk(self, ora, rays, obj, ent, any_hit, times=None, cull=None, stack_limit=64):
        tl = self.tlas
        kw = dict(stack_limit=stack_limit)
        if times is not None:
            kw.update(tlas_nodes1=tl["nodes1"], times=times)
        return ora.walk_rays_instanced(tl["leaves"], tl["nodes0"], tl["root"], tl["count"], self.trees, rays, obj, ent,
                                       any_hit=any_hit, cull=cull, **kw)

    def query(self, d, hits, ids, ctr, any_hit=False, num_primitives=0, flt=None):
        rt, s, tl = self.rt, self.static, self.tlas
        args = (self.pose0.triangles_out, self.pose0.nodes_out, tl["root"], tl["count"], s.records, self.K, s.table, 2, d, hits, ids)
        if flt is None:
            rt.IntersectRaysInstanced(*args, any_hit=any_hit, num_primitives=num_primitives, counters=ctr)
        else:
            rt.IntersectRaysInstancedFiltered(*args, flt, any_hit=any_hit, num_primitives=num_primitives, counters=ctr)

    def query_motion(self, d, td, hits, ids, ctr, any_hit=False):
        m, tl = self.moving, self.tlas
        self.rt.IntersectRaysInstancedMotion(self.pose0, self.pose1, tl["root"], tl["count"], m.records, self.K, m.table, 2, d, td,
                                             hits, ids, any_hit=any_hit, counters=ctr)


def _comb_scene(rt, case):
    b = case["blas"]
    pose = _Pose(rt, b["leaves0"], b["nodes0"])
    return _TwoLevel(rt, case["tlas"], case["mats0"], case["mats1"], case["blas_of"], (pose.triangles_out, pose.nodes_out),
                     (b["leaves0"], b["nodes0"]), b["root"], b["count"])


def _fractal_scene(rt, fractals, name, kind, D):
    tris, cam, inp, root, count, leaves, nodes = fractals(name, kind)
    mats = sc.exact_matrices(D + 1, one_sided=name == "dense")
    tl = sc.tlas_comb(D, half=2.0 ** 50)
    scene = _TwoLevel(rt, tl, mats, mats, np.zeros(D + 1, np.uint32), (inp.triangles_out, inp.nodes_out), (leaves, nodes), root, count)
    return scene, sc.two_level_fractal_rays(name, tris, cam, mats)


def _instanced(rt, ora, scene, rays, what):
    """rt_intersect_rays_instanced, both instantiations and both modes; the filtered call with a pass-all filter and with one
    instance masked under CULL_BACK -> the closest-hit walker stats"""
    d = _dev_rays(rt, rays)
    n = len(rays)
    obj, ent = sc.static_object_rays(rays, scene.records, scene.counts)
    out = None
    for any_hit in (False, True):
        exp, eid, st = scene.walk(ora, rays, obj, ent, any_hit)
        for pf in (0, sc.BIG):
            got, ctr, ids = _launch(rt, n, lambda h, c, i: scene.query(d, h, i, c, any_hit=any_hit, num_primitives=pf), ids=True)
            _check(got, ctr, exp, st, f"IntersectRaysInstanced {what} any_hit={any_hit} pf={pf > 0}", ids, eid)
        got, ctr, ids = _launch(rt, n, lambda h, c, i: scene.query(d, h, i, c, any_hit=any_hit,
                                                                   flt=tgf._dev_ifilter(rt, ifr.InstanceFilter())), ids=True)
        _check(got, ctr, exp, st, f"IntersectRaysInstancedFiltered {what} pass-all any_hit={any_hit}", ids, eid)
        out = (exp, st) if out is None else out
    _report(f"IntersectRaysInstanced {what}", out[1])
    return out + (obj, ent)


def _filtered(rt, ora, scene, rays, obj, ent, masked, plain, what):
    d = _dev_rays(rt, rays)
    masks = np.full(scene.K, ifr.ALL, np.uint32)
    masks[masked] = 0
    flt = ifr.InstanceFilter(ifr.CULL_BACK, ifr.ALL, ifr.instance_filters(scene.K, masks=masks))
    ent = ent.copy()
    ent[:, masked] = False
    cull = sc.cull_back(scene.records)
    assert set(cull.tolist()) == {ifr.CULL_BACK, ifr.CULL_FRONT}, "a mirrored instance swaps the cull bits"
    for any_hit in (False, True):
        exp, eid, st = scene.walk(ora, rays, obj, ent, any_hit, cull=cull)
        for pf in (0, sc.BIG):
            got, ctr, ids = _launch(rt, len(rays), lambda h, c, i: scene.query(d, h, i, c, any_hit=any_hit, num_primitives=pf,
                                                                               flt=tgf._dev_ifilter(rt, flt)), ids=True)
            _check(got, ctr, exp, st, f"IntersectRaysInstancedFiltered {what} masked + CULL_BACK any_hit={any_hit} pf={pf > 0}",
                   ids, eid)
        if not any_hit:
            assert not (eid == masked).any() and (exp["t"] != plain["t"]).any(), "the filter changes answers"
            _report(f"IntersectRaysInstancedFiltered {what}", st)


def _instanced_motion(rt, ora, scene, rays, what):
    import torch
    r4, t4 = _over_taus(rays)
    d, td = _dev_rays(rt, r4), torch.from_numpy(t4).cuda()
    obj, ent = sc.motion_object_rays(r4, t4, scene.motion_records, scene.counts)
    out = None
    for any_hit in (False, True):
        exp, eid, st = scene.walk(ora, r4, obj, ent, any_hit, times=t4)
        got, ctr, ids = _launch(rt, len(r4), lambda h, c, i: scene.query_motion(d, td, h, i, c, any_hit=any_hit), ids=True)
        _check(got, ctr, exp, st, f"IntersectRaysInstancedMotion {what} any_hit={any_hit}", ids, eid)
        out = (st, ent) if out is None else out
    _report(f"IntersectRaysInstancedMotion {what}", out[0])
    return out


@pytest.mark.parametrize("D,B", sc.TWO_LEVEL)
def test_two_level_combs(rt, ora, D, B):
    case = sc.two_level_case(D, B)
    scene = _comb_scene(rt, case)
    rays = case["rays"]
    overflow = D + B >= sc.STACK
    exp, st, obj, ent = _instanced(rt, ora, scene, rays, f"comb ({D}, {B})")
    assert not ent[:, case["bad"]].any() and ent[:, case["masked"]].all()
    want = sc.expect_two_level(D, B, sc.leaf_enter(case, ent[0]))
    assert (st[:, 2:6] == np.array(want, np.uint32)).all(), f"({D}, {B}): {st[0]} vs {want}"
    assert (st[:, LOW] >= 17).any() and overflow == bool((st[:, HIGH] > 0).any())
    _filtered(rt, ora, scene, rays, obj, ent, case["masked"], exp, f"comb ({D}, {B})")
    mst, ment = _instanced_motion(rt, ora, scene, rays, f"comb ({D}, {B})")
    n = len(rays)
    for k, tau in enumerate(TAUS):
        block, e = mst[k * n:(k + 1) * n], ment[k * n:(k + 1) * n]
        assert e[:, case["singular"]].all() == (tau != 0.5) and e[:, case["singular"]].any() == (tau != 0.5), \
            "the instance that is singular in between is not entered at time 0.5, and is at every other time"
        want = sc.expect_two_level(D, B, sc.leaf_enter(case, e[0]))
        assert (block[:, 2:6] == np.array(want, np.uint32)).all(), f"({D}, {B}) time {tau}: {block[0]} vs {want}"


@pytest.mark.parametrize("name,kind,D", sc.TWO_LEVEL_FRACTALS)
def test_fractal_blas_under_a_comb_tlas(rt, ora, fractals, name, kind, D):
    scene, rays = _fractal_scene(rt, fractals, name, kind, D)
    what = f"{name}/{kind} under comb {D}"
    exp, st, obj, ent = _instanced(rt, ora, scene, rays, what)
    assert ent.all() and (st[:, LOW] >= 17).any() and (exp["primitive_id"] != sc.MISS).mean() > 0.3
    if D == 30:
        assert (st[:, HIGH] > 0).any() and st[:, DEPTH].max() == sc.STACK
    else:
        assert (st[:, DROPPED] == 0).all()
    if name == "dense":
        # the records the kernels had to match are not the brute-force closest hits (the brute force, K x m tests per ray, on
        # the rays whose record a walk that keeps every push changes)
        free, _, _ = scene.walk(ora, rays, obj, ent, False, stack_limit=1024)
        sel = np.nonzero((st[:, HIGH] > 0) & (free["t"] != exp["t"]))[0][:40]
        brute = sc.brute_two_level_t([sc.leaf_triangles(scene.trees[0][0])] * scene.K, obj[sel], ent[sel], rays[sel])
        gone = (exp["t"][sel] != brute) & (free["t"][sel] == brute)
        print(f"    of {len(sel)} rays, {gone.sum()} lost the brute-force hit to a push dropped above level 16")
        assert gone.any() and (exp["t"][sel][gone] > brute[gone]).all()
    _filtered(rt, ora, scene, rays, obj, ent, int(scene.tlas["ids"][D - 2]), exp, what)
    mst, _ = _instanced_motion(rt, ora, scene, rays, what)
    assert (mst[:, LOW] >= 17).any()
