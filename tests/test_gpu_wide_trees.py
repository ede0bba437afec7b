"""GPU tests of the ray-type queries on trees with runs of one to seven slots (tests/wide_trees.py): NONE slots first, in the
middle and last, lone runs below the root, a 7-slot root run.  Every tree is built on the device, downloaded, re-packed on the
host and uploaded; the device is held to a reference run on the WIDE tree's own bytes -- the oracle's ordered walkers
(records and instance ids bit for bit, counters[0:2] equal to the walker's sums), never to its own answer on the binary tree.
tests/test_wide_trees_ref_cpu.py holds the inputs to the conditions that make these cases a test of the run-length logic.

1. rt_intersect_rays (the anchor; both instantiations) and rt_intersect_rays_motion over stack_scenes.TAUS, pose 1 refitted on
   the host by refit_ref: both modes on LBVH, hybrid, SAH, SAH + pairs and SAH + splits trees of the grid and the soup;
2. rt_intersect_rays_filtered: closest / any hit under cull-back, group masks, a skip id and all combined, against
   ray_filter_ref's kept walk, as tests/test_gpu_ray_filter.py;
3. rt_intersect_rays_spheres over the grid's centroid spheres (two leaves hold ids >= the count, one radius is negative),
   direct and indexed, against ora.walk_rays_spheres;
4. rt_intersect_rays_capsules: degenerate capsules byte-equal to the sphere query on the same wide tree, counters included;
   real capsules through test_gpu_capsules' record / closest / any checks;
5. rt_sphere_cast: radius 0 byte-equal to rt_intersect_rays on the wide tree, records and counters; radii > 0 through
   test_gpu_sphere_cast's checks, overlap rows equal to rt_range_count's; rays that miss the root run cost one box test per
   non-NONE root slot (the NONE slot's +-1e30 bounds are not read into root_M), and rays that pass under the scene enter the
   grown root boxes only if the last non-NONE slot's bound, the largest, is part of root_M;
6. rt_intersect_rays_instanced, _filtered and _motion: a TLAS over 24 instances re-packed to a 7-slot root run, BLASes the wide
   grid and the wide soup, stack_scenes.exact_matrices; against ora.walk_rays_instanced; also wide over binary and binary over
   wide, so that a failure points to one level;
7. rt_intersect_rays_instanced_mixed: an all-triangle table byte-equal to rt_intersect_rays_instanced; one identity instance
   over the wide sphere tree byte-equal to the flat sphere query; instance_mixed_ref's half-and-half world, every BLAS and
   the TLAS re-packed, against its float64 brute force;
8. rt_prepare_instances on a table whose root runs have 3, 5 and 7 slots with NONE slots; count = 8 is a bad BLAS;
9. trees of 3, 5 and 7 triangles as one root run of leaf slots and no Box child: rt_intersect_rays (both instantiations), the
   motion query, a keep-all rt_intersect_rays_filtered, the sphere cast of radius 0, the run as a sphere tree (sphere query and
   degenerate capsules), and the run as the one BLAS under a one-leaf TLAS through rt_intersect_rays_instanced, _filtered
   (pass-all and CULL_BACK), _motion and _mixed (all-triangle table; identity instance of the sphere tree).  Real capsules and
   sphere casts of radius > 0 are not run on them: their float64 arms need some hundred stable hits.  The set-valued queries,
   refit and the ray sort on these runs are tests/test_gpu_wide_trees_sets.py's;
10. a device-to-device copy of the wide tree into the buffer the cast reads (the "upload": its source is a staging tensor on
    the device, which is what a capture can hold), the sphere cast and the instanced query captured in one HIP graph, replayed
    after the rays are rewritten in place.

Every walker reports zero dropped pushes here (asserted): a full stack is tests/test_gpu_stack_depths.py's business."""
import numpy as np
import pytest

import capsule_ref as cr
import instance_filter_ref as ifr
import instance_motion_ref as imr
import instance_ref as ir
import ray_filter_ref as rx
import ray_first_ref as rf
import refit_ref
import sphere_cast_ref as scr
import stack_scenes as sc
import test_gpu_capsule_stack as tcs
import test_gpu_capsules as tgc
import instance_mixed_ref as mr
import test_gpu_instance_filter as tgf
import test_gpu_instance_mixed as tgx
import test_gpu_instance_motion as tgm
import test_gpu_instances as tgi
import test_gpu_ray_filter as tgr
import test_gpu_ray_queries as rq
import test_gpu_sphere_cast as tsc
import test_gpu_spheres as tgs
import test_gpu_stack_depths as tsd
import wide_trees as wt

pytestmark = pytest.mark.gpu

F = np.float32
MISS = 0xFFFFFFFF
DROPPED = tsd.DROPPED
TAUS = tsd.TAUS
K_INST = 24


# ------------------------------------------------------------------ the trees
class Wide:
    """one scene on one builder: the device's binary tree (inp, host copy) and its re-packed copy, uploaded"""

    def __init__(self, rt, tris, kind):
        self.rt, self.tris, self.kind = rt, tris, kind
        self.inp, self.root, self.count = rq._gpu_tree(rt, tris, kind)
        self.leaves, self.nodes = tsd._host_tree(rt, self.inp)
        w, wr, wc = wt.repack(self.nodes, self.root, self.count)
        assert len(w) * 32 <= rt.NodesBytes(tris.shape[0]), "the wide tree fits the BuildInput's nodes_out"
        self.tree = wt.Tree(self.leaves, w, wr, wc, rt)
        h = wt.hist(w, wr, wc)
        assert set(h) == set(range(1, 8)) and min(h.values()) >= 2 and wc >= 3, h


@pytest.fixture(scope="module")
def wide(rt, scenes):
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            cache[name, kind] = Wide(rt, wt.tris(name, scenes), kind)
        return cache[name, kind]
    return get


@pytest.fixture(scope="module")
def rays_of(scenes):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = wt.rays(name, wt.tris(name, scenes))
        return cache[name]
    return get


def _clean(st, exp, what, share=0.3):
    assert int(st[:, DROPPED].sum()) == 0, f"{what}: the walker dropped a push"
    got = (exp["primitive_id"] != MISS).mean()
    assert got >= share, f"{what}: the walker finds a hit on {got:.3f} of the rays"


# ------------------------------------------------------------------ 1: the anchor and the motion query
@pytest.mark.parametrize("kind", wt.KINDS)
@pytest.mark.parametrize("name", wt.SCENES)
def test_intersect_rays(rt, ora, wide, rays_of, name, kind):
    w, rays = wide(name, kind), rays_of(name)
    t = w.tree
    d = tsd._dev_rays(rt, rays)
    for any_hit in (False, True):
        exp, st = ora.walk_rays(*t.host, rays, any_hit=any_hit)
        _clean(st, exp, f"{name}/{kind}")
        for pf in (0, sc.BIG):
            got, ctr = rq._query(rt, t.g, d, any_hit=any_hit, num_primitives=pf, counters=True)
            tsd._check(got, ctr, exp, st, f"IntersectRays wide {name}/{kind} any_hit={any_hit} pf={pf > 0}")
    print(f"IntersectRays wide {name}/{kind}: run lengths {wt.hist(t.nodes, t.root, t.count)}")


@pytest.mark.parametrize("kind", wt.KINDS)
@pytest.mark.parametrize("name", wt.SCENES)
def test_intersect_rays_motion(rt, ora, wide, rays_of, name, kind):
    w, rays = wide(name, kind), rays_of(name)
    t = w.tree
    l1, n1, broken = refit_ref.refit_ref(t.leaves, t.nodes, t.root, t.count, wt.moved(w.tris))
    assert not broken
    none = (t.nodes["w28"] >> 29) == wt.NONE
    assert n1[none].tobytes() == t.nodes[none].tobytes() and (n1["min"][~none] != t.nodes["min"][~none]).any()
    pose1 = wt.Tree(l1, n1, t.root, t.count, rt)
    # one ray set per time, aimed at the scene as that time sees it (the soup's small triangles move by half their size)
    import torch
    t1 = wt.moved(w.tris)
    r4 = np.concatenate([wt.rays(name, wt.at_time(w.tris, t1, tau)) for tau in TAUS])
    t4 = np.repeat(TAUS, len(rays))
    d, td = tsd._dev_rays(rt, r4), torch.from_numpy(t4).cuda()
    for any_hit in (False, True):
        exp, st = ora.walk_rays_motion(t.leaves, t.nodes, l1, n1, t.root, t.count, r4, t4, any_hit=any_hit)
        got, ctr = tsd._launch(rt, len(r4), lambda hits, c: rt.IntersectRaysMotion(t.pose, pose1.pose, t.root, t.count, d, td, hits,
                                                                                   any_hit=any_hit, counters=c))
        tsd._check(got, ctr, exp, st, f"IntersectRaysMotion wide {name}/{kind} any_hit={any_hit}")
        for tau, block, bst in zip(TAUS, np.split(exp, len(TAUS)), np.split(st, len(TAUS))):
            # (a quarter of a batch: some hundred hits per time.  The static sets reach 0.71 and 0.33)
            _clean(bst, block, f"motion {name}/{kind} at time {tau}", share=0.25)
    # every ray of time 0 again at time 1: the two poses give other answers
    a, _ = ora.walk_rays_motion(t.leaves, t.nodes, l1, n1, t.root, t.count, rays, np.zeros(len(rays), F))
    b, _ = ora.walk_rays_motion(t.leaves, t.nodes, l1, n1, t.root, t.count, rays, np.ones(len(rays), F))
    assert (a["t"] != b["t"]).any()


# ------------------------------------------------------------------ 2: the filtered query
@pytest.mark.parametrize("kind", ("bottom_up", "sah_pairs", "sah_splits"))
@pytest.mark.parametrize("name", ("grid", "layers"))
def test_intersect_rays_filtered(rt, wide, rays_of, name, kind):
    w, rays = wide(name, kind), rays_of(name)
    t = w.tree
    walk = tgr.Walk(t.nodes, t.leaves, t.root, t.count, rays, w.tris.shape[0])
    n = len(rays)
    for fname in ("cull_back", "groups", "skip_nearest", "combined"):
        flt, frows, _, _ = walk.kept(fname)
        exp = walk.expected(fname, 1)
        empty = np.array([len(r) == 0 for r in frows])
        assert 0 < empty.sum() < n
        for pf in (0, tgr.BIG):
            what = f"wide {name}/{kind}/{fname}, num_primitives {pf}"
            hits, _ = tgr._closest(rt, t.g, rays, flt, num_primitives=pf)
            anyh, _ = tgr._closest(rt, t.g, rays, flt, any_hit=True, num_primitives=pf)
            miss = hits["primitive_id"] == MISS
            assert (miss == empty).all(), f"{what}: a miss holds iff W_f is empty; rays {np.nonzero(miss != empty)[0][:4]}"
            assert hits[miss].tobytes() == rf.miss_records(int(miss.sum())).tobytes()
            assert ((anyh["primitive_id"] == MISS) == miss).all(), f"{what}: any-hit hits iff closest-hit hits"
            for i in np.nonzero(~miss)[0]:
                row = frows[i]
                for h, mode in ((hits[i], "closest"), (anyh[i], "any")):
                    same = (row["t"].view(np.uint32) == h["t"].view(np.uint32)) & (row["u"].view(np.uint32) == h["u"].view(np.uint32)) & \
                           (row["v"].view(np.uint32) == h["v"].view(np.uint32))
                    assert same.any(), f"{what}: ray {i}: the {mode} record {h} is not in W_f in (t, u, v)"
                    assert h["primitive_id"] in row["primitive_id"], f"{what}: ray {i}: the {mode} record {h} carries a filtered id"
                E, decided, _ = exp[i]
                if decided:
                    assert hits["t"][i].view(np.uint32) == E["t"][0].view(np.uint32), \
                        f"{what}: decided ray {i}: t {hits['t'][i]} is not E's {E['t'][0]}"
    # a keep-all filter is the unfiltered call, counters included
    for any_hit in (False, True):
        a, ca = tgr._closest(rt, t.g, rays, rx.Filter(), any_hit=any_hit)
        b, cb = tgr._closest(rt, t.g, rays, tgr.UNFILTERED, any_hit=any_hit)
        assert a.tobytes() == b.tobytes() and (ca[:2] == cb[:2]).all()


# ------------------------------------------------------------------ 3, 4: spheres and capsules
class WideSpheres:
    """the grid's centroid spheres on one builder, the tree re-packed; two leaves hold ids >= the count"""

    def __init__(self, rt, scenes, kind):
        self.spheres, self.rays = wt.sphere_scene("grid", scenes)
        s = tgs.Spheres(rt, self.spheres, kind).frame()
        assert rt.sphere_status(s.status) == rt.RT_SPHERE_BAD, "sphere 5 has a negative radius"
        self.keep = s
        root, count = s.root
        leaves, nodes = tsd._host_tree(rt, s.tree)
        leaves = leaves[:len(self.spheres)].copy()
        n = len(self.spheres)
        leaves["primitive_id_0"][[11, n // 2]] = n + 1, 0xFFFFFFF0
        self.tree = wt.Tree(leaves, *wt.repack(nodes, root, count), rt)
        assert set(wt.hist(self.tree.nodes, self.tree.root, self.tree.count)) == set(range(1, 8))


@pytest.fixture(scope="module")
def wide_spheres(rt, scenes):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = WideSpheres(rt, scenes, kind)
        return cache[kind]
    return get


@pytest.mark.parametrize("kind", tgs.KINDS)
def test_intersect_rays_spheres(rt, ora, wide_spheres, kind):
    s = wide_spheres(kind)
    t = s.tree
    exp, st = tsd._spheres(rt, ora, (t.pose.triangles_out, t.pose.nodes_out), (t.leaves, t.nodes), t.root, t.count, s.spheres, s.rays,
                           f"wide grid/{kind}")
    _clean(st, exp, f"spheres {kind}")
    ids = exp["primitive_id"][exp["primitive_id"] != MISS]
    assert (ids < len(s.spheres)).all() and not (ids == 5).any()


@pytest.mark.parametrize("kind", tgs.KINDS)
def test_degenerate_capsules_equal_the_sphere_query(rt, wide_spheres, kind):
    s = wide_spheres(kind)
    t = s.tree
    tcs._same_as_spheres(rt, t.pose.triangles_out, t.pose.nodes_out, t.root, t.count, s.spheres, s.rays, f"wide grid/{kind}")


@pytest.mark.parametrize("kind", tgs.KINDS)
def test_real_capsules(rt, scenes, kind):
    import torch
    caps, rays = wt.capsule_scene("grid", scenes)
    c = tgc.Capsules(rt, caps, kind).frame()
    torch.cuda.synchronize()
    assert rt.capsule_status(c.status) == rt.RT_CAPSULE_BAD, "capsule 5 has a negative radius"
    root, count = c.root
    leaves, nodes = tsd._host_tree(rt, c.tree)
    t = wt.Tree(leaves, *wt.repack(nodes, root, count), rt)
    assert set(wt.hist(t.nodes, t.root, t.count)) == set(range(1, 8))
    ref = cr.Reference(caps, rays)
    d = tgc._dev_rays(rt, rays)

    def run(**kw):
        hits = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
        rt.IntersectRaysCapsules(t.pose.triangles_out, t.pose.nodes_out, t.root, t.count, c.capsules, c.n, d, hits, **kw)
        torch.cuda.synchronize()
        return hits.cpu().numpy().view(rt.HIT).reshape(-1)

    closest = run()
    tgc._check_closest(closest, ref, f"wide capsules grid/{kind}")
    tgc._check_any(run(any_hit=True), ref, f"wide capsules grid/{kind} any-hit", closest)
    assert (closest["primitive_id"] != MISS).mean() >= 0.3


# ------------------------------------------------------------------ 5: the sphere cast
def _cast(rt, t, rays, radii=None, radius=0.0, **kw):
    import torch
    n = len(rays)
    hits = torch.full((n, 4), 0, dtype=torch.int32, device="cuda").fill_(0x5A5A5A5A).view(torch.float32)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    rd = None if radii is None else rt.to_device(np.ascontiguousarray(radii, F)).view(torch.float32)
    rt.SphereCast(t.pose.triangles_out, t.pose.nodes_out, t.root, t.count, tsd._dev_rays(rt, rays), hits, radii=rd, radius=radius,
                  counters=ctr, **kw)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(rt.HIT).reshape(-1), ctr.cpu().numpy().astype(np.uint64)


@pytest.mark.parametrize("kind", ("bottom_up", "sah", "sah_pairs", "sah_splits"))
@pytest.mark.parametrize("name", wt.SCENES)
def test_sphere_cast_radius_0_equals_intersect_rays(rt, ora, wide, rays_of, name, kind):
    w, rays = wide(name, kind), rays_of(name)
    t = w.tree
    for any_hit in (False, True):
        exp, st = ora.walk_rays(*t.host, rays, any_hit=any_hit)
        ref, rctr = rq._query(rt, t.g, rays, any_hit=any_hit, counters=True)
        for kw in (dict(radius=0.0), dict(radii=np.zeros(len(rays), F))):
            got, ctr = _cast(rt, t, rays, any_hit=any_hit, **kw)
            what = f"SphereCast radius 0 wide {name}/{kind} any_hit={any_hit} {sorted(kw)}"
            assert got.tobytes() == ref.tobytes(), f"{what}: records differ from rt_intersect_rays"
            assert (ctr[:2] == rctr[:2]).all(), f"{what}: counters {ctr[:2]} vs rt_intersect_rays's {rctr[:2]}"
            tsd._check(got, ctr, exp, st, what)


@pytest.mark.parametrize("kind", ("bottom_up", "sah", "sah_pairs", "sah_splits"))
def test_sphere_cast_radii(rt, wide, kind):
    import torch
    w = wide("grid", kind)
    t = w.tree
    rays, radii = wt.cast_rays("grid", w.tris)
    ref = scr.Reference(w.tris, rays, radii)
    assert ref.unstable_share <= wt.cast_cap()
    tr = tsc.Tree(rt, w.tris, kind, built=t.g)
    assert tr.M == scr.root_M(t.nodes, t.root, t.count) and tr.M >= scr.scene_M(w.tris) and tr.M < 1e29
    closest, cf, ctr = tr.cast(rays, radii, counters=True)
    hit = tsc._check_closest(tr, closest, cf, ref, f"wide grid/{kind}")
    assert hit.mean() >= 0.3 and ctr[0] > 0 and ctr[1] >= hit.sum()
    hits, feats, _ = tr.cast(rays, radii, any_hit=True)
    tsc._check_any(tr, hits, feats, ref, closest, f"wide grid/{kind} any-hit")
    # overlap rows are the rows where rt_range_count in sphere shape counts a triangle, on the same wide tree
    n = len(rays)
    q = np.zeros(n, rt.POINT_QUERY)
    q["p"] = rays["origin"] + rays["tmin"][:, None] * rays["dir"]
    q["dist2_max"] = radii * radii
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rt.RangeCount(t.pose.triangles_out, t.pose.nodes_out, t.root, t.count, rt.to_device(q).view(torch.float32), off)
    torch.cuda.synchronize()
    touched = np.diff(off.cpu().numpy()) > 0
    over, pos = cf == scr.OVERLAP, radii > 0
    assert not (over & ~touched).any() and not (over & ~pos).any() and over.sum() >= 10
    st = ref.stable & pos
    assert (over[st] == touched[st]).all(), f"wide grid/{kind}: overlap rows differ from the range query's on stable rays"


def test_sphere_cast_root_run_with_a_none_slot(rt, wide):
    """rays that pass the scene by ten extents: every cast tests the root run's non-NONE slots and nothing else.  A NONE slot
    read into root_M (its bounds are +-1e30) would grow every box by 2^-18 * 1e30 and send every ray through the whole tree."""
    w = wide("grid", "sah")
    t = w.tree
    root = t.nodes[t.root:t.root + t.count]
    live = int(((root["w28"] >> 29) != wt.NONE).sum())
    assert live < t.count == 7
    last = [s for s in range(t.count) if int(root["w28"][s]) >> 29 != wt.NONE][-1]
    mags = np.maximum(np.abs(root["min"]).max(1), np.abs(root["max"]).max(1))
    nodes = t.nodes.copy()
    if mags[last] < mags[(root["w28"] >> 29) != wt.NONE].max():     # the largest bound goes to the last live slot: stretch its box
        nodes["max"][t.root + last] = np.maximum(nodes["max"][t.root + last], F(2.0) * mags[(root["w28"] >> 29) != wt.NONE].max())
    t2 = wt.Tree(t.leaves, nodes, t.root, t.count, rt)
    M = scr.root_M(nodes, t.root, t.count)
    run = nodes[t.root:t.root + t.count]
    assert M == max(np.abs(run["min"][last]).max(), np.abs(run["max"][last]).max()) and M < 100
    _, _, mid, ext = scr.scene_box(w.tris)
    n = 200
    rng = np.random.default_rng(5)
    rays = np.zeros(n, rt.RAY)
    rays["origin"] = mid + np.array([0.0, 10.0 * ext + M, 0.0]) + rng.uniform(-1, 1, (n, 3))
    rays["dir"] = np.array([1.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, (n, 3))
    rays["tmin"], rays["tmax"] = 0.0, np.inf
    radii = rng.uniform(0.01, 0.5 * ext, n).astype(F)
    for any_hit in (False, True):
        got, ctr = _cast(rt, t2, rays, radii=radii, any_hit=any_hit)
        assert (got["primitive_id"] == MISS).all()
        assert ctr[0] == n * live and ctr[1] == 0, f"box tests {ctr[0]} for {n} rays over {live} live root slots; leaf tests {ctr[1]}"


def test_sphere_cast_root_M_includes_the_last_live_slot(rt, wide):
    """the other half of root_M: the largest bound sits in the LAST non-NONE slot of the root run and nowhere else (its box is
    stretched to 2^21 along +x, so that 2^-18 * M is 8).  Rays pass under the scene, level, at a distance d in [1, 4] below the
    lowest root box, with radii of at most 0.1: grown by e(M) = r + 8 every root box they pass under takes them in, grown by
    the e of an M taken over the run less that slot (r + some 1e-5) none does -- both from sphere_cast_ref's grow_e and slab
    test alone.  So a loop that stopped one slot short would leave the counters at one box test per live root slot."""
    w = wide("grid", "sah")
    t = w.tree
    root = t.nodes[t.root:t.root + t.count]
    slots = [s for s in range(t.count) if int(root["w28"][s]) >> 29 != wt.NONE]
    live, last = len(slots), slots[-1]
    assert live < t.count == 7
    nodes = t.nodes.copy()
    nodes["max"][t.root + last][0] = F(2.0 ** 21)
    t2 = wt.Tree(t.leaves, nodes, t.root, t.count, rt)
    run = nodes[t.root:t.root + t.count]
    M = scr.root_M(nodes, t.root, t.count)
    short = run.copy()
    short["w28"][last] = 0                                        # the run as a loop that ends one slot early sees it
    M_short = scr.root_M(short, 0, t.count)
    assert M == F(2.0 ** 21) and M_short < 100
    lo, hi, mid, ext = scr.scene_box(w.tris)
    n = 200
    rng = np.random.default_rng(6)
    rays = np.zeros(n, rt.RAY)
    rays["origin"][:, 0] = lo[0] - 20.0
    rays["origin"][:, 1] = float(run["min"][slots, 1].min()) - rng.uniform(1.0, 4.0, n)
    rays["origin"][:, 2] = mid[2] + rng.uniform(-0.25, 0.25, n) * (hi[2] - lo[2])
    rays["dir"][:, 0] = 1.0
    rays["dir"][:, 2] = rng.uniform(-0.01, 0.01, n)
    rays["tmin"], rays["tmax"] = 0.0, np.inf
    radii = rng.uniform(0.01, 0.1, n).astype(F)

    def entered(Mx):
        e = scr.grow_e(radii, Mx)[:, None]
        return np.array([scr.slab_f32(rays, run["min"][s][None, :] - e, run["max"][s][None, :] + e, rays["tmax"]) for s in slots]).any(0)

    assert entered(M).all() and not entered(M_short).any(), "the reference alone: the grown boxes take every ray in only under the full M"
    for any_hit in (False, True):
        got, ctr = _cast(rt, t2, rays, radii=radii, any_hit=any_hit)
        assert (got["primitive_id"] == MISS).all(), "the balls pass a whole unit under every triangle"
        assert ctr[0] + ctr[1] >= n * live + n, \
            f"tests {ctr[:2]}: {n} rays over {live} live root slots, and every ray goes on below a root slot it entered"


# ------------------------------------------------------------------ 6: the two-level queries
def _mats1(mats):
    """pose 1 of exact_matrices: scaled by 1.25 and moved"""
    out = []
    for M in mats:
        M = np.asarray(M, np.float64).copy()
        M[:, :3] *= 1.25
        M[:, 3] += (0.5, -0.25, 0.125)
        out.append(M)
    return out


def _tlas_host(rt, built, n):
    leaves, nodes = tsd._host_tree(rt, built)
    return leaves[:n].copy(), nodes


class World:
    """24 instances (exact_matrices) of two BLASes (grid: table entry 0, soup: entry 1) under a TLAS built on the device.
    wide_tlas / wide_blas choose which level is re-packed.  Holds what the walker needs and the device calls."""

    def __init__(self, rt, wide, rays_of, wide_tlas, wide_blas, kind="bottom_up"):
        import torch
        self.rt, self.K = rt, K_INST
        ws = [wide("grid", kind), wide("soup", "sah_pairs")]
        blas = [w.tree if wide_blas else wt.Tree(w.leaves, w.nodes, w.root, w.count, rt) for w in ws]
        self.blas = blas
        self.entries = [(b.pose.triangles_out, b.pose.nodes_out, b.root, b.count) for b in blas]
        self.counts = [b.count for b in blas]
        mats0 = sc.exact_matrices(K_INST)
        self.blas_of = np.arange(K_INST, dtype=np.uint32) % 2
        self.trees = [blas[int(b)].host for b in self.blas_of]
        # the static scene
        s = tgi.Instanced(rt, self.entries, ir.instance_array(mats0, self.blas_of))
        s.frame()
        torch.cuda.synchronize()
        assert rt.instance_status(s.status) == 0
        self.static, self.records = s, s.host_records()
        root, count = s.root
        tl, tn = _tlas_host(rt, s.tlas, K_INST)
        self.tlas = self._tlas(tl, (tn,), root, count, wide_tlas)
        # the moving scene: both TLAS poses have one topology, so one re-packing serves both
        m = tgm.Moving(rt, self.entries, imr.motion_instance_array(mats0, _mats1(mats0), self.blas_of))
        m.frame()
        torch.cuda.synchronize()
        assert rt.instance_status(m.status) == 0
        self.moving, self.motion_records = m, rt.to_host(m.records, rt.MOTION_INSTANCE_RECORD, K_INST)
        ml, mn0 = _tlas_host(rt, m.tlas, K_INST)
        _, mn1 = _tlas_host(rt, m.pose1, K_INST)
        self.mtlas = self._tlas(ml, (mn0, mn1), root, count, wide_tlas)
        self.mats0, self.mats1, self.rays_of = mats0, _mats1(mats0), rays_of
        self.rays = self.aimed(0.0)

    def aimed(self, tau):
        """world rays: 16 rays of each instance's BLAS, mapped through the instance's matrix as time tau sees it (tau 0: the
        static matrix itself)"""
        parts = []
        for k in range(K_INST):
            src = self.rays_of("grid" if self.blas_of[k] == 0 else "soup")
            pick = (k * 7 + 24 * np.arange(16)) % len(src)
            parts.append(sc.through_instances(src[pick], [imr.matrix_at(self.mats0[k], self.mats1[k], [tau])[0]]))
        return np.concatenate(parts)[:381]

    def _tlas(self, leaves, poses, root, count, wide_tlas):
        rt = self.rt
        if wide_tlas:
            packed = [wt.repack(n, root, count, none_every=2) for n in poses]
            nodes, root, count = [p[0] for p in packed], packed[0][1], packed[0][2]
            assert all((n["w12"] == nodes[0]["w12"]).all() and (n["w28"] == nodes[0]["w28"]).all() for n in nodes)
            assert count == 7, "the TLAS's root run has 7 slots"
            mid = [s - f for f, k in wt.runs(nodes[0], root, count) for s in range(f, f + k)
                   if k > 2 and f < s < f + k - 1 and int(nodes[0]["w28"][s]) >> 29 == wt.TRI]
            assert len(mid) >= 3, "instance leaves sit in the middle of wide runs"
        else:
            nodes = list(poses)
        return dict(leaves=leaves, nodes=nodes, root=root, count=count, poses=[wt.Tree(leaves, n, root, count, rt).pose for n in nodes])

    def walk(self, ora, rays, obj, ent, any_hit, times=None, cull=None):
        tl = self.tlas if times is None else self.mtlas
        kw = {} if times is None else dict(tlas_nodes1=tl["nodes"][1], times=times)
        return ora.walk_rays_instanced(tl["leaves"], tl["nodes"][0], tl["root"], tl["count"], self.trees, rays, obj, ent,
                                       any_hit=any_hit, cull=cull, **kw)

    def query(self, d, hits, ids, ctr, any_hit=False, num_primitives=0, flt=None, mixed=None):
        rt, s, tl = self.rt, self.static, self.tlas
        p = tl["poses"][0]
        args = (p.triangles_out, p.nodes_out, tl["root"], tl["count"], s.records, self.K, s.table)
        if mixed is not None:
            rt.IntersectRaysInstancedMixed(*args, mixed, 2, d, hits, ids, any_hit=any_hit, counters=ctr)
        elif flt is None:
            rt.IntersectRaysInstanced(*args, 2, d, hits, ids, any_hit=any_hit, num_primitives=num_primitives, counters=ctr)
        else:
            rt.IntersectRaysInstancedFiltered(*args, 2, d, hits, ids, flt, any_hit=any_hit, num_primitives=num_primitives, counters=ctr)

    def query_motion(self, d, td, hits, ids, ctr, any_hit=False):
        m, tl = self.moving, self.mtlas
        self.rt.IntersectRaysInstancedMotion(tl["poses"][0], tl["poses"][1], tl["root"], tl["count"], m.records, self.K, m.table, 2,
                                             d, td, hits, ids, any_hit=any_hit, counters=ctr)


LEVELS = {"wide_over_wide": (True, True), "wide_over_binary": (True, False), "binary_over_wide": (False, True)}


@pytest.fixture(scope="module")
def worlds(rt, wide, rays_of):
    cache = {}

    def get(level):
        if level not in cache:
            cache[level] = World(rt, wide, rays_of, *LEVELS[level])
        return cache[level]
    return get


@pytest.mark.parametrize("level", LEVELS)
def test_intersect_rays_instanced(rt, ora, worlds, level):
    w = worlds(level)
    rays, n = w.rays, len(w.rays)
    d = tsd._dev_rays(rt, rays)
    obj, ent = sc.static_object_rays(rays, w.records, w.counts)
    assert ent.all()
    plain = None
    for any_hit in (False, True):
        exp, eid, st = w.walk(ora, rays, obj, ent, any_hit)
        _clean(st, exp, f"instanced {level}")
        for pf in (0, sc.BIG):
            got, ctr, ids = tsd._launch(rt, n, lambda h, c, i: w.query(d, h, i, c, any_hit=any_hit, num_primitives=pf), ids=True)
            tsd._check(got, ctr, exp, st, f"IntersectRaysInstanced {level} any_hit={any_hit} pf={pf > 0}", ids, eid)
        got, ctr, ids = tsd._launch(rt, n, lambda h, c, i: w.query(d, h, i, c, any_hit=any_hit,
                                                                   flt=tgf._dev_ifilter(rt, ifr.InstanceFilter())), ids=True)
        tsd._check(got, ctr, exp, st, f"IntersectRaysInstancedFiltered {level} pass-all any_hit={any_hit}", ids, eid)
        plain = (exp, eid) if plain is None else plain
    assert len(set(plain[1][plain[1] != MISS].tolist())) >= K_INST // 2, "hits on many instances, of both BLASes"
    # one instance masked out under CULL_BACK
    masked = int(np.bincount(plain[1][plain[1] != MISS]).argmax())
    masks = np.full(w.K, ifr.ALL, np.uint32)
    masks[masked] = 0
    flt = ifr.InstanceFilter(ifr.CULL_BACK, ifr.ALL, ifr.instance_filters(w.K, masks=masks))
    ent2 = ent.copy()
    ent2[:, masked] = False
    cull = sc.cull_back(w.records)
    assert set(cull.tolist()) == {ifr.CULL_BACK, ifr.CULL_FRONT}, "a mirrored instance swaps the cull bits"
    for any_hit in (False, True):
        exp, eid, st = w.walk(ora, rays, obj, ent2, any_hit, cull=cull)
        assert int(st[:, DROPPED].sum()) == 0
        for pf in (0, sc.BIG):
            got, ctr, ids = tsd._launch(rt, n, lambda h, c, i: w.query(d, h, i, c, any_hit=any_hit, num_primitives=pf,
                                                                       flt=tgf._dev_ifilter(rt, flt)), ids=True)
            tsd._check(got, ctr, exp, st, f"IntersectRaysInstancedFiltered {level} masked + CULL_BACK any_hit={any_hit} pf={pf > 0}",
                       ids, eid)
        if not any_hit:
            assert not (eid == masked).any() and (exp["t"] != plain[0]["t"]).any(), "the filter changes answers"


@pytest.mark.parametrize("level", LEVELS)
def test_intersect_rays_instanced_motion(rt, ora, worlds, level):
    import torch
    w = worlds(level)
    # one ray set per time, aimed through every instance's matrix as that time sees it: pose 1 is scaled by 1.25 and moved, and
    # rays aimed at pose 0 would leave the later times nearly without hits
    r4 = np.concatenate([w.aimed(tau) for tau in TAUS])
    t4 = np.repeat(TAUS, len(w.rays))
    d, td = tsd._dev_rays(rt, r4), torch.from_numpy(t4).cuda()
    obj, ent = sc.motion_object_rays(r4, t4, w.motion_records, w.counts)
    assert ent.all()
    for any_hit in (False, True):
        exp, eid, st = w.walk(ora, r4, obj, ent, any_hit, times=t4)
        for tau, block, bid, bst in zip(TAUS, np.split(exp, len(TAUS)), np.split(eid, len(TAUS)), np.split(st, len(TAUS))):
            # (the share test_intersect_rays_motion asks of a time's block; the static world is held to 0.3)
            _clean(bst, block, f"instanced motion {level} at time {tau}", share=0.25)
            assert any_hit or len(set(bid[bid != MISS].tolist())) >= K_INST // 2, f"time {tau}: hits on many instances"
        got, ctr, ids = tsd._launch(rt, len(r4), lambda h, c, i: w.query_motion(d, td, h, i, c, any_hit=any_hit), ids=True)
        tsd._check(got, ctr, exp, st, f"IntersectRaysInstancedMotion {level} any_hit={any_hit}", ids, eid)


# ------------------------------------------------------------------ 7: the mixed query
def test_mixed_all_triangle_table_equals_the_instanced_query(rt, worlds):
    w = worlds("wide_over_wide")
    d, n = tsd._dev_rays(rt, w.rays), len(w.rays)
    table = rt.geometry_table([None, None])
    for any_hit in (False, True):
        exp, ectr, eid = tsd._launch(rt, n, lambda h, c, i: w.query(d, h, i, c, any_hit=any_hit), ids=True)
        got, ctr, ids = tsd._launch(rt, n, lambda h, c, i: w.query(d, h, i, c, any_hit=any_hit, mixed=table), ids=True)
        assert got.tobytes() == exp.tobytes() and (ids == eid).all(), f"any_hit {any_hit}: records differ from rt_intersect_rays_instanced"
        assert (ctr[:2] == ectr[:2]).all(), f"any_hit {any_hit}: tests {ctr[:2]} vs {ectr[:2]}"
        assert (ids != MISS).sum() >= 50


@pytest.mark.parametrize("kind", tgs.KINDS)
def test_mixed_identity_sphere_instance_equals_the_sphere_query(rt, wide_spheres, kind):
    import torch
    s = wide_spheres(kind)
    t = s.tree
    rays = tgi._positive_zeros(s.rays)
    d, n = tsd._dev_rays(rt, rays), len(rays)
    sp = rt.to_device(np.ascontiguousarray(s.spheres, F))
    entries = [(t.pose.triangles_out, t.pose.nodes_out, t.root, t.count)]
    inst = tgi.Instanced(rt, entries, ir.instance_array([np.eye(3, 4)], [0]))
    inst.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(inst.status) == 0
    assert (inst.host_records()["world_to_object"] == np.eye(3, 4, dtype=F)).all()
    table = rt.geometry_table([(sp, len(s.spheres))])
    root, count = inst.root
    for any_hit in (False, True):
        exp, ectr = tsd._launch(rt, n, lambda h, c: rt.IntersectRaysSpheres(t.pose.triangles_out, t.pose.nodes_out, t.root, t.count, sp,
                                                                            len(s.spheres), d, h, any_hit=any_hit, counters=c))
        got, ctr, ids = tsd._launch(rt, n, lambda h, c, i: rt.IntersectRaysInstancedMixed(
            inst.tlas.triangles_out, inst.tlas.nodes_out, root, count, inst.records, 1, inst.table, table, 1, d, h, i, any_hit=any_hit,
            counters=c), ids=True)
        assert got.tobytes() == exp.tobytes(), f"{kind} any_hit {any_hit}: records differ from rt_intersect_rays_spheres"
        assert ctr[1] == ectr[1], f"{kind} any_hit {any_hit}: sphere tests {ctr[1]} vs {ectr[1]}"
        hit = exp["primitive_id"] != MISS
        assert (ids[hit] == 0).all() and (ids[~hit] == MISS).all() and hit.mean() >= 0.3


class _WideMixed(tgx.Mixed):
    """test_gpu_instance_mixed.Mixed whose TLAS is swapped for its re-packed copy after the build"""
    wide_root = None

    @property
    def root(self):
        return self.wide_root or tgi.Instanced.root.fget(self)


def test_mixed_half_and_half_world_against_float64(rt):
    """instance_mixed_ref's world (two triangle and two sphere BLASes, eight instances) with every BLAS and the TLAS re-packed,
    through test_gpu_instance_mixed's float64 check"""
    import torch
    w = mr.world()
    b = tgx.Blases(rt, w.data, w.kinds, mr.BLAS_TREES)
    keep, entries = [], []
    for tri, nod, root, count in b.entries:
        t = wt.Tree(rt.to_host(tri, rt.TRIANGLE_PAIR), *wt.repack(rt.to_host(nod, rt.NODE), root, count), rt)
        assert max(wt.hist(t.nodes, t.root, t.count)) == 7
        keep.append(t)
        entries.append((t.pose.triangles_out, t.pose.nodes_out, t.root, t.count))
    s = _WideMixed(rt, entries, b.geoms, w.instances)
    s.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(s.status) == 0
    tl, tn = _tlas_host(rt, s.tlas, w.n)
    tlas = wt.Tree(tl, *wt.repack(tn, *s.root, none_every=2), rt)
    assert tlas.count >= 3 and ((tlas.nodes["w28"] >> 29) == wt.NONE).any()
    s.tlas, s.wide_root = tlas.pose, (tlas.root, tlas.count)
    tgx._check_f64(s, mr.reference(mr.SEEDS[0]), "wide mixed world")


# ------------------------------------------------------------------ 8: rt_prepare_instances over wide root runs
def test_prepare_instances_over_wide_root_runs(rt, wide):
    import torch
    w = wide("grid", "bottom_up")
    trees, boxes = [], []
    for width in (3, 5, 7):
        nodes, root, count = wt.repack(w.nodes, w.root, w.count, root_width=width)
        run = nodes[root:root + count]
        assert count == width and ((run["w28"] >> 29) == wt.NONE).sum() == 1
        trees.append(wt.Tree(w.leaves, nodes, root, count, rt))
        boxes.append(ir.root_box(nodes, root, count))
        assert np.abs(np.array(boxes[-1])).max() < 100, "the NONE slot's bounds are not in the box"
    entries = [(t.pose.triangles_out, t.pose.nodes_out, t.root, t.count) for t in trees]
    entries.append(entries[2][:3] + (8,))                      # a root run of 8 slots: a bad BLAS
    boxes.append(None)
    mats = sc.exact_matrices(8)
    inst = ir.instance_array(mats, [0, 1, 2, 0, 1, 2, 3, 2])
    s = tgi.Instanced(rt, entries, inst)
    s.status.fill_(0xFF)
    s.prepare()
    torch.cuda.synchronize()
    assert rt.instance_status(s.status) == rt.RT_INSTANCE_BAD_BLAS
    prox, inv, flags = ir.prepare(inst, boxes)
    assert flags.tolist() == [0, 0, 0, 0, 0, 0, ir.BAD_BLAS, 0]
    assert s.host_proxies().tobytes() == prox.tobytes(), "proxies differ from the float32 restatement"
    rec = s.host_records()
    assert (rec["flags"] == flags).all() and (rec["blas"] == inst["blas"]).all() and (rec["spare"] == 0).all()
    ok = flags == 0
    assert (inv[ok].astype(F).astype(np.float64) == inv[ok]).all(), "the inverses of these matrices are exact in float32"
    assert (rec["world_to_object"][ok] == inv[ok].astype(F)).all(), "world_to_object differs from the exact inverse"


# ------------------------------------------------------------------ 9: one root run of 3, 5, 7 leaf slots
def _single_run(rt, scenes, n):
    """-> (name, triangles, rays, leaf records, the tree as one root run of n leaf slots, uploaded)"""
    name = f"tiny{n}"
    tris = wt.tris(name, scenes)
    inp, root, count = rq._gpu_tree(rt, tris, "bottom_up")
    leaves, nodes = tsd._host_tree(rt, inp)
    leaves = leaves[:n].copy()
    t = wt.Tree(leaves, *wt.single_run(nodes, root, count), rt)
    assert t.count == n and wt.hist(t.nodes, t.root, t.count) == {n: 1}
    return name, tris, wt.rays(name, tris), leaves, t


def _single_run_spheres(rt, tris, leaves, t, n):
    """the same run as a sphere tree: leaf k holds sphere k, every slot its sphere's proxy box -> (spheres, rays, tree)"""
    spheres = sc.fractal_spheres(tris, "deep")
    sl = leaves.copy()
    sl["primitive_id_0"] = np.arange(n)
    prox = tgs.sr.prepare_f32(spheres)[0]
    sn = t.nodes.copy()
    order = (sn["w28"] & wt.MASK).astype(np.int64)
    sn["min"], sn["max"] = prox[order, 0:3], prox[order, 3:6]
    return spheres, tgs.sr.make_rays(spheres, 77 + n, wt.N_RAYS, with_radius=True), wt.Tree(sl, sn, t.root, t.count, rt)


@pytest.mark.parametrize("n", wt.TINY)
def test_single_run_trees(rt, ora, scenes, n):
    import torch
    name, tris, rays, leaves, t = _single_run(rt, scenes, n)
    d = tsd._dev_rays(rt, rays)
    l1, n1, _ = refit_ref.refit_ref(leaves, t.nodes, t.root, t.count, wt.moved(tris))
    pose1 = wt.Tree(l1, n1, t.root, t.count, rt)
    tsd._motion(rt, ora, t.pose, pose1.pose, (leaves, t.nodes), (l1, n1), t.root, t.count, rays, f"single run of {n}")
    for any_hit in (False, True):
        exp, st = ora.walk_rays(*t.host, rays, any_hit=any_hit)
        _clean(st, exp, name)
        for pf in (0, sc.BIG):
            got, ctr = rq._query(rt, t.g, d, any_hit=any_hit, num_primitives=pf, counters=True)
            tsd._check(got, ctr, exp, st, f"IntersectRays single run of {n} any_hit={any_hit} pf={pf > 0}")
        got, ctr = tgr._closest(rt, t.g, rays, rx.Filter(), any_hit=any_hit)
        tsd._check(got, ctr, exp, st, f"IntersectRaysFiltered keep-all single run of {n} any_hit={any_hit}")
        got, ctr = _cast(rt, t, rays, radius=0.0, any_hit=any_hit)
        tsd._check(got, ctr, exp, st, f"SphereCast radius 0 single run of {n} any_hit={any_hit}")
    # the same run as a sphere tree (leaf k holds sphere k) and as a one-BLAS world under a one-leaf TLAS
    spheres, srays, stree = _single_run_spheres(rt, tris, leaves, t, n)
    sl, sn = stree.leaves, stree.nodes
    tsd._spheres(rt, ora, (stree.pose.triangles_out, stree.pose.nodes_out), (sl, sn), t.root, t.count, spheres, srays, f"single run of {n}")
    tcs._same_as_spheres(rt, stree.pose.triangles_out, stree.pose.nodes_out, t.root, t.count, spheres, srays, f"single run of {n}")
    inst = tgi.Instanced(rt, [(t.pose.triangles_out, t.pose.nodes_out, t.root, t.count)], ir.instance_array(sc.exact_matrices(3)[2:], [0]))
    inst.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(inst.status) == 0
    rec = inst.host_records()
    tl, tn = _tlas_host(rt, inst.tlas, 1)
    wr = sc.through_instances(rays, sc.exact_matrices(3)[2:])
    obj, ent = sc.static_object_rays(wr, rec, [t.count])
    root1, count1 = inst.root
    dw = tsd._dev_rays(rt, wr)
    for any_hit in (False, True):
        exp, eid, st = ora.walk_rays_instanced(tl, tn, root1, count1, [t.host], wr, obj, ent, any_hit=any_hit)
        got, ctr, ids = tsd._launch(rt, len(wr), lambda h, c, i: inst.query(dw, h, i, any_hit=any_hit, counters=c), ids=True)
        tsd._check(got, ctr, exp, st, f"IntersectRaysInstanced single run of {n} any_hit={any_hit}", ids, eid)
        assert (eid != MISS).mean() >= 0.3


@pytest.mark.parametrize("n", wt.TINY)
def test_single_run_trees_under_instances(rt, ora, scenes, n):
    """the same root run of n leaf slots as the one BLAS of a one-leaf TLAS, through the filtered, the motion and the mixed
    instanced calls: the BLAS's root run is entered from the TLAS leaf with the lane's stack at its base"""
    import torch
    name, tris, rays, leaves, t = _single_run(rt, scenes, n)
    entry = (t.pose.triangles_out, t.pose.nodes_out, t.root, t.count)
    M0 = sc.exact_matrices(3)[2:]
    M1 = _mats1(M0)
    inst = tgi.Instanced(rt, [entry], ir.instance_array(M0, [0]))
    inst.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(inst.status) == 0
    rec = inst.host_records()
    tl, tn = _tlas_host(rt, inst.tlas, 1)
    root1, count1 = inst.root
    wr = sc.through_instances(rays, M0)
    obj, ent = sc.static_object_rays(wr, rec, [t.count])
    dw, nw = tsd._dev_rays(rt, wr), len(wr)
    args = (inst.tlas.triangles_out, inst.tlas.nodes_out, root1, count1, inst.records, 1, inst.table)
    # the filtered call: a pass-all filter is the plain walk, CULL_BACK the walk with the instance's cull word
    cull = sc.cull_back(rec)
    tri_table = rt.geometry_table([None])
    for any_hit in (False, True):
        plain, pid, pst = ora.walk_rays_instanced(tl, tn, root1, count1, [t.host], wr, obj, ent, any_hit=any_hit)
        exp, eid, st = ora.walk_rays_instanced(tl, tn, root1, count1, [t.host], wr, obj, ent, any_hit=any_hit, cull=cull)
        assert int(pst[:, DROPPED].sum()) == 0 and int(st[:, DROPPED].sum()) == 0
        for flt, (e, i, s), what in ((ifr.InstanceFilter(), (plain, pid, pst), "pass-all"),
                                     (ifr.InstanceFilter(ifr.CULL_BACK, ifr.ALL, ifr.instance_filters(1)), (exp, eid, st), "CULL_BACK")):
            for pf in (0, sc.BIG):
                got, ctr, ids = tsd._launch(rt, nw, lambda h, c, k: rt.IntersectRaysInstancedFiltered(
                    *args, 1, dw, h, k, tgf._dev_ifilter(rt, flt), any_hit=any_hit, num_primitives=pf, counters=c), ids=True)
                tsd._check(got, ctr, e, s, f"IntersectRaysInstancedFiltered {what} single run of {n} any_hit={any_hit} pf={pf > 0}", ids, i)
        if not any_hit:
            assert (plain["primitive_id"] != MISS).mean() >= 0.3 and 0 < (eid != MISS).sum() < (pid != MISS).sum(), "the cull drops hits"
        # the mixed call over an all-triangle geometry table is the plain instanced call
        a, actr, aid = tsd._launch(rt, nw, lambda h, c, k: inst.query(dw, h, k, any_hit=any_hit, counters=c), ids=True)
        b, bctr, bid = tsd._launch(rt, nw, lambda h, c, k: rt.IntersectRaysInstancedMixed(
            *args, tri_table, 1, dw, h, k, any_hit=any_hit, counters=c), ids=True)
        assert b.tobytes() == a.tobytes() and (bid == aid).all() and (bctr[:2] == actr[:2]).all(), \
            f"single run of {n} any_hit={any_hit}: the mixed call over triangles differs from rt_intersect_rays_instanced"
    # the motion call: one ray set per time, aimed through the instance's matrix as that time sees it
    mov = tgm.Moving(rt, [entry], imr.motion_instance_array(M0, M1, [0]))
    mov.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(mov.status) == 0
    mrec = rt.to_host(mov.records, rt.MOTION_INSTANCE_RECORD, 1)
    ml, mn0 = _tlas_host(rt, mov.tlas, 1)
    _, mn1 = _tlas_host(rt, mov.pose1, 1)
    mroot, mcount = mov.root
    r4 = np.concatenate([sc.through_instances(rays, [imr.matrix_at(M0[0], M1[0], [tau])[0]]) for tau in TAUS])
    t4 = np.repeat(TAUS, len(rays))
    d4, td = tsd._dev_rays(rt, r4), torch.from_numpy(t4).cuda()
    obj, ent = sc.motion_object_rays(r4, t4, mrec, [t.count])
    assert ent.all()
    for any_hit in (False, True):
        exp, eid, st = ora.walk_rays_instanced(ml, mn0, mroot, mcount, [t.host], r4, obj, ent, any_hit=any_hit, tlas_nodes1=mn1, times=t4)
        for tau, block, bst in zip(TAUS, np.split(exp, len(TAUS)), np.split(st, len(TAUS))):
            _clean(bst, block, f"instanced motion, single run of {n}, at time {tau}", share=0.25)
        got, ctr, ids = tsd._launch(rt, len(r4), lambda h, c, k: mov.query(d4, td, h, k, any_hit=any_hit, counters=c), ids=True)
        tsd._check(got, ctr, exp, st, f"IntersectRaysInstancedMotion single run of {n} any_hit={any_hit}", ids, eid)
    # the mixed call over one identity instance of the run as a sphere tree is the flat sphere query
    spheres, srays, stree = _single_run_spheres(rt, tris, leaves, t, n)
    srays = tgi._positive_zeros(srays)
    sd, sp = tsd._dev_rays(rt, srays), rt.to_device(np.ascontiguousarray(spheres, F))
    sentry = (stree.pose.triangles_out, stree.pose.nodes_out, stree.root, stree.count)
    one = tgi.Instanced(rt, [sentry], ir.instance_array([np.eye(3, 4)], [0]))
    one.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(one.status) == 0
    oroot, ocount = one.root
    sph_table = rt.geometry_table([(sp, n)])
    for any_hit in (False, True):
        exp, ectr = tsd._launch(rt, len(srays), lambda h, c: rt.IntersectRaysSpheres(*sentry, sp, n, sd, h, any_hit=any_hit, counters=c))
        got, ctr, ids = tsd._launch(rt, len(srays), lambda h, c, k: rt.IntersectRaysInstancedMixed(
            one.tlas.triangles_out, one.tlas.nodes_out, oroot, ocount, one.records, 1, one.table, sph_table, 1, sd, h, k,
            any_hit=any_hit, counters=c), ids=True)
        assert got.tobytes() == exp.tobytes(), f"single run of {n} any_hit={any_hit}: records differ from rt_intersect_rays_spheres"
        assert ctr[1] == ectr[1], f"single run of {n} any_hit={any_hit}: sphere tests {ctr[1]} vs {ectr[1]}"
        hit = exp["primitive_id"] != MISS
        assert (ids[hit] == 0).all() and (ids[~hit] == MISS).all() and hit.any()


# ------------------------------------------------------------------ 10: a HIP graph
def test_upload_cast_and_instanced_query_in_a_hip_graph(rt, ora, worlds, rays_of):
    import torch
    w = worlds("wide_over_wide")
    blas = w.blas[0]                                   # the wide grid
    n = len(w.rays)
    sets = {"a": (w.rays, rays_of("grid")), "b": (np.ascontiguousarray(w.rays[::-1]), np.ascontiguousarray(rays_of("grid")[::-1]))}
    host_nodes = rt.to_device(blas.nodes)              # the upload's source: a device-side staging copy
    nodes = torch.zeros_like(host_nodes)
    world_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    cast_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    hits = torch.empty((2, n, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ctr = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    tl = w.tlas

    def one_frame():
        ctr.zero_()
        nodes.copy_(host_nodes)                        # the wide tree is written into the buffer the cast reads
        rt.SphereCast(blas.pose.triangles_out, nodes, blas.root, blas.count, cast_rays, hits[0], radius=0.0, counters=ctr[0])
        p = tl["poses"][0]
        rt.IntersectRaysInstanced(p.triangles_out, p.nodes_out, tl["root"], tl["count"], w.static.records, w.K, w.static.table, 2,
                                  world_rays, hits[1], ids, counters=ctr[1])

    def load(key):
        world_rays.copy_(tsd._dev_rays(rt, sets[key][0]))       # rewritten in place: the same buffers
        cast_rays.copy_(tsd._dev_rays(rt, sets[key][1]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    load("a")
    with torch.cuda.stream(side):
        one_frame()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for key in ("a", "b", "a"):
        load(key)
        hits.fill_(0)
        ids.fill_(0)
        nodes.zero_()
        graph.replay()
        torch.cuda.synchronize()
        wr, cr_ = sets[key]
        exp, st = ora.walk_rays(*blas.host, cr_)
        c = ctr.cpu().numpy().astype(np.uint64)
        tsd._check(hits[0].cpu().numpy().view(rt.HIT).reshape(-1), c[0], exp, st, f"graph replay {key}: SphereCast")
        obj, ent = sc.static_object_rays(wr, w.records, w.counts)
        exp, eid, st = w.walk(ora, wr, obj, ent, False)
        tsd._check(hits[1].cpu().numpy().view(rt.HIT).reshape(-1), c[1], exp, st, f"graph replay {key}: IntersectRaysInstanced",
                   ids.cpu().numpy().view(np.uint32), eid)
