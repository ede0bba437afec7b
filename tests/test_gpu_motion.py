"""GPU tests of the motion-blur ray query (rt_intersect_rays_motion, rt_motion_validate, MotionPose) on every tree the builders
make (the eight of test_gpu_ray_queries.TREES) over grid_mesh(24, 5), soup(1500) and cornell34.  Pose 1 is a smooth
displacement (a function of position alone, so pairs stay whole); the times are motion_ref.TIMES = {0, 0.25, 1/3, 0.7, 1}.

1. endpoints: every time 0 (1) gives rt_intersect_rays's records over pose 0 (pose 1) -- primitive_id exactly, t / u / v with ==
   (a zero's sign may differ) -- and its counters [0], [1]; closest-hit and any-hit; also on fractal_corner(4000), whose rays
   reach the private half of the traversal stack;
2. between the poses: one time per ray, the records against motion_ref's float64 brute force per time group with the
   assertions and bounds of test_gpu_ray_queries._check_against_f64; on non-pair trees the record is bit for bit the float32
   Moller-Trumbore of the float32-interpolated triangle;
3. any-hit hits exactly where closest-hit hits, inside the window, never nearer than the closest hit;
4. a moving occluder: a quad crosses a fixed ray between the poses; the ray hits for the times of the covered interval
   (computed in float64, its ends and the quad's diagonal kept away from) and misses outside, and misses in both poses;
5. tiny and degenerate scenes of tests/small_scenes.py (n1, n2, n5, twins, n65, stack, giant; the built n = 0 tree; count = 0)
   with pose 1 = pose 0 translated: the assertions of 1 and 2;
6. degenerate times (NaN, below 0, above 1) are misses with no tests; records past num_rays are not written; pose 1 == pose 0
   with every time 0 is the static query;
7. rt_motion_validate: 0 for a MotionPose pair, RT_MOTION_TOPOLOGY_MISMATCH for two trees of different meshes;
8. refit of pose 1 + validate + query in one HIP graph replay the eager bytes."""
import numpy as np
import pytest

import motion_ref as mr
import small_scenes as ss
import test_gpu_ray_queries as rq

pytestmark = pytest.mark.gpu

F = np.float32
TREES = rq.TREES
SENT = 0x5A5A5A5A
SMALL = ("n1", "n2", "n5", "twins", "n65", "stack", "giant")


# ------------------------------------------------------------------ device calls
def _motion_tree(rt, tris0, tris1, tree):
    """GPU build of pose 0 (a split tree identity-refitted, as rt_abi.h asks) and MotionPose -> (pose0, pose1, plan1, root, count)"""
    import torch
    inp, root, count = rq._gpu_tree(rt, tris0, tree)
    n = inp.num_triangles
    if "splits" in tree:
        plan0 = rt.device_bytes(rt.RefitPlanBytes(n))
        rt.BuildRefitPlan(inp, root, count, plan0)
        rt.Refit(inp, root, count, plan0)
        assert rt.refit_status(plan0, n) == 0
    pose1, plan1 = rt.MotionPose(inp, root, count, tris1)
    torch.cuda.synchronize()
    assert n == 0 or rt.refit_status(plan1, n) == 0, f"{tree}: pose 1's refit status"
    return inp, pose1, plan1, root, count


def _dev_rays(rt, rays):
    import torch
    return rt.to_device(np.ascontiguousarray(rays.astype(rt.RAY))).view(torch.float32).view(-1, 8)


def _mquery(rt, mg, rays, times, any_hit=False, pad=0):
    """-> (HIT [n], counters uint64[4]); `pad` sentinel records behind the n records, checked"""
    import torch
    pose0, pose1, _, root, count = mg
    d = _dev_rays(rt, rays)
    n = d.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(times, F)).cuda()
    hits = torch.full((n + pad, 4), 0, dtype=torch.int32, device="cuda").fill_(SENT)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    rt.IntersectRaysMotion(pose0, pose1, root, count, d, t, hits, any_hit=any_hit, counters=ctr)
    torch.cuda.synchronize()
    hv = hits.cpu().numpy()
    assert (hv[n:] == SENT).all(), "records past num_rays were written"
    return hv[:n].view(F).view(rt.HIT).reshape(-1).copy(), ctr.cpu().numpy().astype(np.uint64)


def _squery(rt, pose, root, count, rays, any_hit=False):
    return rq._query(rt, (pose, root, count), np.ascontiguousarray(rays.astype(rt.RAY)), any_hit=any_hit, counters=True)


def _assert_same_records(got, exp, what, nan_is_nan=False):
    for f in ("primitive_id", "t", "u", "v"):     # (the floats with ==: a zero's sign may differ)
        same = got[f] == exp[f]
        if nan_is_nan and f != "primitive_id":
            # the fractal alone: a ray's determinant against a triangle of size 2^42 overflows (a = inf, f = 0, u = 0 * inf) and
            # Moller-Trumbore's range tests let the NaN through, in the static query as here; there a NaN equals a NaN
            same |= np.isnan(got[f]) & np.isnan(exp[f])
        assert same.all(), f"{what}: {f} differs on {(~same).sum()} rays"


def _check_endpoints(rt, mg, rays, what, nan_is_nan=False):
    pose0, pose1, _, root, count = mg
    for tau, pose in ((0.0, pose0), (1.0, pose1)):
        for any_hit in (False, True):
            got, gc = _mquery(rt, mg, rays, np.full(len(rays), tau, F), any_hit=any_hit)
            exp, ec = _squery(rt, pose, root, count, rays, any_hit=any_hit)
            w = f"{what} time {tau} any_hit={any_hit}"
            _assert_same_records(got, exp, w, nan_is_nan)
            assert (gc[:2] == ec[:2]).all(), f"{w}: counters {gc[:2]} vs the static query's {ec[:2]}"


def _check_f64(rt, rays, hits, ref, tris_all, base, what, tree, bound):
    rq._check_against_f64(tris_all, rays, mr.with_base(hits, base), ref, ref["stable"], what, check_mt="pairs" not in tree,
                          bound=bound)


# ------------------------------------------------------------------ the world: poses, rays and references, computed once
class World:
    def __init__(self, rt, scenes):
        self.rt, self.scenes = rt, scenes
        self._m = {}

    def _memo(self, key, make):
        if key not in self._m:
            self._m[key] = make()
        return self._m[key]

    def poses(self, name):
        return self._memo(("poses", name), lambda: mr.poses(name, self.scenes))

    def cases(self, name):
        """kind -> (rays, times, ref, tris_all, base)"""
        def make():
            t0, t1 = self.poses(name)
            return {kind: (r, tm) + mr.brute(t0, t1, r, tm, window=kind == "window")
                    for kind, (r, tm) in mr.ray_cases(name, t0, t1).items()}
        return self._memo(("cases", name), make)

    def all_rays(self, name):
        """the rays and times of cases(name), without its float64 references"""
        c = self._memo(("rays", name), lambda: mr.ray_cases(name, *self.poses(name)))
        return np.concatenate([c[k][0] for k in c]), np.concatenate([c[k][1] for k in c])

    def gpu(self, name, tree):
        return self._memo(("gpu", name, tree), lambda: _motion_tree(self.rt, *self.poses(name), tree))

    def small(self, name):
        def make():
            t0 = ss.tris(name, self.scenes)
            t1 = mr.translated(t0)
            rays = ss.rays(name, t0)
            times = mr.TIMES[np.arange(len(rays)) % len(mr.TIMES)]
            return (t0, t1, rays, times) + mr.brute(t0, t1, rays, times)
        return self._memo(("small", name), make)


@pytest.fixture(scope="module")
def world(rt, scenes):
    return World(rt, scenes)


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", mr.ENDPOINT_SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_endpoints_are_the_static_query(world, name, tree):
    rays, _ = world.all_rays(name)
    _check_endpoints(world.rt, world.gpu(name, tree), rays, f"{name}/{tree}", nan_is_nan=name == "fractal")


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", mr.SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_between_the_poses_against_float64(world, name, tree):
    mg = world.gpu(name, tree)
    for kind, (rays, times, ref, tris_all, base) in world.cases(name).items():
        hits, ctr = _mquery(world.rt, mg, rays, times)
        assert ctr[1] > 0
        _check_f64(world.rt, rays, hits, ref, tris_all, base, f"{name}/{tree} {kind}", tree, mr.CAP[name])


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", mr.SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_any_hit(world, name, tree):
    rt = world.rt
    rays, times = world.all_rays(name)
    mg = world.gpu(name, tree)
    c, cc = _mquery(rt, mg, rays, times)
    a, ac = _mquery(rt, mg, rays, times, any_hit=True)
    ch, ah = c["primitive_id"] != rt.MISS, a["primitive_id"] != rt.MISS
    assert (ch == ah).all(), f"{name}/{tree}: any-hit hits on {ah.sum()} rays, closest-hit on {ch.sum()}"
    assert ch.sum() > 100
    assert ac[1] <= cc[1] and ac[0] <= cc[0], "any-hit does no more work than closest-hit"
    ra, aa, ca = rays[ah], a[ah], c[ah]
    assert ((aa["t"] >= ra["tmin"]) & (aa["t"] <= ra["tmax"])).all()
    assert (aa["t"] >= ca["t"]).all()


# ------------------------------------------------------------------ 4
def _occluder(c):
    """a quad [c - 1, c + 1] x [-1, 1] at z = 2 (two triangles sharing the diagonal p00 - p11) and six fixed triangles far off
    the ray, so that every builder has a tree to make"""
    p00, p10, p11, p01 = (c - 1, -1, 2), (c + 1, -1, 2), (c + 1, 1, 2), (c - 1, 1, 2)
    quad = [p00 + p10 + p11, p00 + p11 + p01]
    far = [(x, 8.0, z, x + 1, 8.0, z, x, 9.0, z + 0.5) for x in (-6.0, 0.0, 6.0) for z in (1.0, 5.0)]
    return np.array(quad + far, F)


@pytest.mark.parametrize("tree", TREES)
def test_a_moving_occluder(rt, tree):
    tris0, tris1 = _occluder(-3.0), _occluder(3.0)
    mg = _motion_tree(rt, tris0, tris1, tree)
    ox, oy = 0.1, 0.2
    times = np.linspace(0, 1, 257).astype(F)
    # float64: the quad's centre at time tau is the interpolation of -3 and 3; the ray is covered while |ox - c| < 1 and sits on
    # the diagonal where ox - c == oy
    tau = times.astype(np.float64)
    c = (1 - tau) * -3.0 + tau * 3.0
    lo, hi, diag = (ox - 1 + 3) / 6, (ox + 1 + 3) / 6, (ox - oy + 3) / 6
    m = 0.01
    inside = (tau > lo + m) & (tau < hi - m) & (np.abs(tau - diag) > m)
    outside = (tau < lo - m) | (tau > hi + m)
    assert inside.sum() > 60 and outside.sum() > 150 and (np.abs(ox - c[inside]) < 1).all() and (np.abs(ox - c[outside]) > 1).all()
    rays = np.zeros(len(times), rt.RAY)
    rays["origin"], rays["dir"], rays["tmin"], rays["tmax"] = (ox, oy, 0.0), (0.0, 0.0, 1.0), 0.0, np.inf
    for any_hit in (False, True):
        hits, _ = _mquery(rt, mg, rays, times, any_hit=any_hit)
        hit = hits["primitive_id"] != rt.MISS
        assert hit[inside].all(), f"{tree}: {(~hit[inside]).sum()} misses while the quad covers the ray"
        assert not hit[outside].any(), f"{tree}: {hit[outside].sum()} hits while the quad is off the ray"
        assert (np.abs(hits["t"][hit] - 2.0) <= 2e-5).all() and np.isin(hits["primitive_id"][hit], (0, 1)).all()
    for pose in (mg[0], mg[1]):       # neither pose alone sees the occluder
        s, _ = _squery(rt, pose, mg[3], mg[4], rays)
        assert (s["primitive_id"] == rt.MISS).all()


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("tree", TREES)
def test_small_scenes(world, name, tree):
    rt = world.rt
    t0, t1, rays, times, ref, tris_all, base = world.small(name)
    mg = _motion_tree(rt, t0, t1, tree)
    what = f"{name}/{tree}"
    _check_endpoints(rt, mg, rays, what)
    hits, _ = _mquery(rt, mg, rays, times, pad=64)
    assert name not in ss.NO_F64_CAST
    _check_f64(rt, rays, hits, ref, tris_all, base, what, tree, 0.01)
    anyh, _ = _mquery(rt, mg, rays, times, any_hit=True, pad=64)
    assert ((hits["primitive_id"] != rt.MISS) == (anyh["primitive_id"] != rt.MISS)).all(), f"{what}: any-hit and closest-hit disagree"


@pytest.mark.parametrize("tree", ss.N0_TREES)
def test_empty_trees(world, tree):
    rt = world.rt
    rays = world.small("n5")[2]
    times = mr.TIMES[np.arange(len(rays)) % len(mr.TIMES)]
    empty = np.zeros((0, 9), F)
    mg = _motion_tree(rt, empty, empty, tree)          # the builder's own empty tree: a root run of two None slots
    assert mg[4] == 2
    full = world.gpu("grid", "bottom_up")
    for m in (mg, full[:3] + (0, 0)):                  # and count = 0 over a real tree: nothing is read
        for any_hit in (False, True):
            hits, ctr = _mquery(rt, m, rays, times, any_hit=any_hit, pad=64)
            assert (hits["primitive_id"] == rt.MISS).all() and (hits["t"] == np.inf).all() and (hits["u"] == 0).all()
            assert (ctr[:2] == 0).all(), f"count {m[4]}: counters {ctr}"


# ------------------------------------------------------------------ 6
def test_degenerate_times_and_batch_edges(world):
    rt = world.rt
    mg = world.gpu("grid", "bottom_up")
    good, _ = world.cases("grid")["outside"][:2]
    good = good.astype(rt.RAY)
    ok, _ = _mquery(rt, mg, good, np.full(len(good), 0.25, F))
    assert (ok["primitive_id"] != rt.MISS).sum() > 100
    bad = np.array([np.nan, -0.1, 1.5, -np.inf, np.inf, -1e-30, np.nextafter(F(1), F(2)), -np.nan], F)
    hits, ctr = _mquery(rt, mg, good[:len(bad)], bad, pad=64)
    assert (hits["primitive_id"] == rt.MISS).all() and (hits["t"] == np.inf).all() and (hits["u"] == 0).all() and (hits["v"] == 0).all()
    assert (ctr[:2] == 0).all(), "no test is counted for a ray whose time is not in [0, 1]"
    # one bad time among good ones changes nothing else; -0.0 is 0
    times = np.full(len(good), 0.25, F)
    times[5] = np.nan
    mixed, _ = _mquery(rt, mg, good, times)
    keep = np.arange(len(good)) != 5
    assert mixed[keep].tobytes() == ok[keep].tobytes() and mixed["primitive_id"][5] == rt.MISS
    z, _ = _mquery(rt, mg, good, np.full(len(good), -0.0, F))
    _assert_same_records(z, _squery(rt, mg[0], mg[3], mg[4], good)[0], "time -0.0")
    # batch edges: records past num_rays keep their sentinel (checked inside), the others are the big batch's
    for n in (1, 63, 65, 1000):
        h, _ = _mquery(rt, mg, good[:n], np.full(n, 0.25, F), pad=64)
        assert h.tobytes() == ok[:n].tobytes(), f"num_rays {n}"
    # pose 1 == pose 0 byte for byte, every time 0 (and any other time: the interpolation of a value with itself)
    same = (mg[0], mg[0], None, mg[3], mg[4])
    s, sc = _squery(rt, mg[0], mg[3], mg[4], good)
    h, hc = _mquery(rt, same, good, np.zeros(len(good), F))
    _assert_same_records(h, s, "pose 1 == pose 0")
    assert (hc[:2] == sc[:2]).all()


# ------------------------------------------------------------------ 7
def test_validate(world, rt, scenes):
    import torch
    status = torch.full((1,), 0x77, dtype=torch.int32, device="cuda")
    for tree in ("bottom_up", "sah_pairs_splits"):
        pose0, pose1, _, root, count = world.gpu("grid", tree)
        status.fill_(0x77)
        rt.MotionValidate(pose0, pose1, root, count, pose0.num_triangles, status)
        assert rt.motion_status(status) == 0, f"{tree}: a MotionPose pair is one tree"
    a = world.gpu("grid", "bottom_up")[0]
    other = scenes.soup(a.num_triangles, 3, size=0.15)
    b, rb, cb = rq._gpu_tree(rt, other, "bottom_up")
    assert b.num_triangles == a.num_triangles
    status.zero_()
    rt.MotionValidate(a, b, 0, 2, a.num_triangles, status)
    assert rt.motion_status(status) == rt.RT_MOTION_TOPOLOGY_MISMATCH
    # one rotation word changed in a copy
    pose0, pose1, _, root, count = world.gpu("grid", "pairs")
    t = pose1.triangles_out.clone()
    t[7 * 64 + 44] ^= 1
    rt.MotionValidate(pose0, (t, pose1.nodes_out), root, count, pose0.num_triangles, status)
    assert rt.motion_status(status) == rt.RT_MOTION_TOPOLOGY_MISMATCH
    rt.MotionValidate(pose0, pose1, root, count, pose0.num_triangles, status)
    assert rt.motion_status(status) == 0, "the word is cleared"


# ------------------------------------------------------------------ 8
def test_refit_validate_and_query_in_a_hip_graph(rt, scenes):
    import torch
    from test_gpu_refit import _smooth
    tris = scenes.grid_mesh(40, 3)
    pose0, root, count = rq._gpu_tree(rt, tris, "sah")
    pose1, plan1 = rt.MotionPose(pose0, root, count, _smooth(tris))
    n = pose0.num_triangles
    rays = _dev_rays(rt, rq._ray_sets(tris, seed=9)["outside"])
    nr = rays.shape[0]
    times = torch.from_numpy(mr.TIMES[np.arange(nr) % len(mr.TIMES)]).cuda()
    hits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    sets = [_smooth(tris, phase=ph) for ph in (0.0, 0.7, 1.9)]

    def frame():
        rt.Refit(pose1, root, count, plan1)
        rt.MotionValidate(pose0, pose1, root, count, n, status)
        rt.IntersectRaysMotion(pose0, pose1, root, count, rays, times, hits)

    eager = []
    for p in sets:
        pose1.triangles_in.copy_(rt.to_device(p))
        frame()
        torch.cuda.synchronize()
        eager.append((pose1.nodes_out.cpu().numpy().copy(), hits.view(torch.uint8).cpu().numpy().copy()))
    assert len({e[1].tobytes() for e in eager}) == 3, "the three poses give different records"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        frame()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            frame()
    torch.cuda.current_stream().wait_stream(side)
    for p, (en, eh) in zip(sets, eager):
        pose1.triangles_in.copy_(rt.to_device(p))
        hits.fill_(0)
        status.fill_(0x77)
        graph.replay()
        torch.cuda.synchronize()
        assert (pose1.nodes_out.cpu().numpy() == en).all() and (hits.view(torch.uint8).cpu().numpy() == eh).all()
        assert rt.motion_status(status) == 0
    assert rt.refit_status(plan1, n) == 0
