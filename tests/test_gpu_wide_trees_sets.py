"""GPU tests of the set-valued queries, the signed distance, refit and the ray sort on trees with runs of one to seven slots
(tests/wide_trees.py; the ray-type queries are tests/test_gpu_wide_trees.py's).  Every tree is built on the device, downloaded,
re-packed on the host and uploaded, and the device is held to a reference run on the wide tree's own bytes.

1. rt_ray_hits_count / _collect and the filtered pair: offsets, and rows as multisets bit for bit, equal ray_hits_ref.walk (the
   filtered ones ray_filter_ref's kept walk) on the wide tree; counters [0] and [1] equal its box tests and leaf visits.  On
   `layers` at least 10 % of the rays have two or more hits;
2. rt_ray_first_hits, plain and filtered, k in {1, 3, 8}: decided rays are ray_first_ref.expected bit for bit, the envelope
   holds on every ray, the undecided share is under the cap -- the checks of tests/test_gpu_ray_first.py and
   tests/test_gpu_ray_filter.py;
3. rt_signed_distance / rt_occupancy on small_scenes' tetra as one root run of leaf slots, on its box (twelve leaves) under
   a 7-slot root run, and on sdf_ref's box with mixed widths: equal to sdf_ref.compose on the same wide tree, and to the
   analytic solid;
4. rt_build_refit_plan + rt_refit with the wide tree written into the BuildInput's own nodes_out: status 0; after the vertices
   move (twice, through one plan) nodes and leaf records equal refit_ref.refit_ref bit for bit, the NONE slots' bytes
   untouched; rt_intersect_rays on the refitted tree equals the walker on the downloaded bytes; a Box child with count 0 and
   one whose run ends past the slot count give RT_REFIT_BAD_TREE;
5. rt_sort_rays on a 7-slot root run with a NONE slot: order, keys, num_live and root box equal ray_sort_ref.sort; the order
   fed to rt_intersect_rays_indexed gives the unsorted records;
6. items 1, 2, 4 and 5 again on the trees of 3, 5 and 7 triangles as ONE root run of that many leaf slots and no Box child: the
   per-run loops start on the root run with an empty stack, walk_run and the expected-arrival count of the refit see the root
   run alone, and the sort's root box is taken over leaf slots only (item 3 has the tetra's run of four)."""
import numpy as np
import pytest

import ray_first_ref as rf
import ray_hits_ref as rh
import refit_ref
import sdf_ref
import small_scenes as ss
import test_gpu_ray_filter as tgr
import test_gpu_ray_first as tgk
import test_gpu_ray_hits as tgh
import test_gpu_ray_queries as rq
import test_gpu_ray_sort as trs
import test_gpu_refit as tre
import test_gpu_sdf as tgd
import test_gpu_small_scenes as tss
import test_gpu_stack_depths as tsd
import wide_trees as wt
from test_gpu_wide_trees import Wide

pytestmark = pytest.mark.gpu

F = np.float32
MISS = 0xFFFFFFFF
SET_KINDS = ("bottom_up", "sah_pairs", "sah_splits")
SET_SCENES = wt.SCENES + ("layers",)
KS = (1, 3, 8)
FILTERS = ("cull_back", "combined")


@pytest.fixture(scope="module")
def wide(rt, scenes):
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            w = Wide(rt, wt.tris(name, scenes), kind)
            w.rays = wt.rays(name, w.tris)
            cache[name, kind] = w
        return cache[name, kind]
    return get


class Tiny:
    """a scene of wide_trees.TINY on the LBVH builder, its tree re-packed to ONE root run of n leaf slots (no Box child, no NONE
    slot): every per-run loop starts on the root run with an empty stack and ends there.  The attributes of Wide"""

    def __init__(self, rt, scenes, n):
        self.name = f"tiny{n}"
        self.tris = wt.tris(self.name, scenes)
        self.rays = wt.rays(self.name, self.tris)
        self.inp, root, count = rq._gpu_tree(rt, self.tris, "bottom_up")
        leaves, nodes = tsd._host_tree(rt, self.inp)
        self.tree = wt.Tree(leaves[:n].copy(), *wt.single_run(nodes, root, count), rt)
        assert self.tree.count == n and wt.hist(self.tree.nodes, self.tree.root, self.tree.count) == {n: 1}


# ------------------------------------------------------------------ 1: all hits
@pytest.mark.parametrize("kind", SET_KINDS)
@pytest.mark.parametrize("name", SET_SCENES)
def test_ray_hits(rt, wide, name, kind):
    _ray_hits(rt, wide(name, kind), f"wide {name}/{kind}", 0.10 if name == "layers" else 0.0)


@pytest.mark.parametrize("n", wt.TINY)
def test_ray_hits_on_a_single_run(rt, scenes, n):
    _ray_hits(rt, Tiny(rt, scenes, n), f"single run of {n}", 0.05)


def _ray_hits(rt, w, what, many_min):
    t, rays = w.tree, w.rays
    rows, box_tests, leaf_visits = rh.walk(t.nodes, t.leaves, t.root, t.count, rays)
    r = tgh._hits(rt, t.pose.triangles_out, t.pose.nodes_out, t.root, t.count, rays)
    assert r.st_count == 0
    assert (r.offsets == rh.offsets(rows)).all(), f"{what}: offsets differ from the prefix sum of the walk's row lengths"
    tgh._assert_rows_equal(r.rows, rows, what)
    assert r.ctr_count[0] == box_tests and r.ctr_count[1] == leaf_visits, \
        f"{what}: counters {r.ctr_count[:2]} vs the walk's {box_tests}, {leaf_visits}"
    many = np.mean([len(x) >= 2 for x in rows])
    print(f"{what}: {int(r.offsets[-1])} records, {100 * many:.1f} % of the rays with two or more")
    assert r.offsets[-1] > 0 and many >= many_min
    # the filtered pair against the kept walk
    walk = tgr.Walk(t.nodes, t.leaves, t.root, t.count, rays, w.tris.shape[0])
    assert walk.box_tests == box_tests and walk.leaf_visits == leaf_visits
    for fname in FILTERS:
        flt, frows, _, _ = walk.kept(fname)
        f = tgr._hits(rt, t.g, rays, flt)
        assert (f.offsets == rh.offsets(frows)).all(), f"{what}/{fname}: offsets differ from the prefix sum of |W_f|"
        tgr._same_rows(f.rows, frows, f"{what}/{fname}")
        assert (f.ctr_count == r.ctr_count).all(), f"{what}/{fname}: counters {f.ctr_count[:2]}, unfiltered {r.ctr_count[:2]}"
        assert 0 < f.offsets[-1] < r.offsets[-1], f"{what}/{fname}: the filter keeps {f.offsets[-1]} of {r.offsets[-1]} records"


# ------------------------------------------------------------------ 2: the first K
@pytest.mark.parametrize("kind", SET_KINDS)
@pytest.mark.parametrize("name", SET_SCENES)
def test_ray_first_hits(rt, wide, name, kind):
    _ray_first_hits(rt, wide(name, kind), f"wide {name}/{kind}")


@pytest.mark.parametrize("n", wt.TINY)
def test_ray_first_hits_on_a_single_run(rt, scenes, n):
    _ray_first_hits(rt, Tiny(rt, scenes, n), f"single run of {n}")


def _ray_first_hits(rt, w, what):
    t, rays = w.tree, w.rays
    walk = tgk.Walk(t.nodes, t.leaves, t.root, t.count, rays)
    assert walk.nonempty >= len(rays) // 8 and max(len(r) for r in walk.rows) >= 2, "the ray set is not trivial"
    for k in KS:
        exp = walk.expected(k)
        share = rf.undecided_share(exp, walk.rows)                # the reference alone: a condition on the inputs
        assert share <= rf.CAP, f"{what}: k {k}: {100 * share:.2f} % of the rays are undecided"
        rows, ctr, status = tgk._first(rt, t.pose.triangles_out, t.pose.nodes_out, t.root, t.count, rays, k)
        assert status == 0, f"{what}: k {k}: status {status}"
        differ = tgk._check_rows(rows, walk, k, what, exp)
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits
        print(f"{what}: k {k}: {100 * share:.3f} % undecided, {differ} rows differ from E; box tests {int(ctr[0])} of {walk.box_tests}")
    fwalk = tgr.Walk(t.nodes, t.leaves, t.root, t.count, rays, w.tris.shape[0])
    for fname in FILTERS:
        flt, frows, _, _ = fwalk.kept(fname)
        for k in KS:
            exp = fwalk.expected(fname, k)
            share = rf.undecided_share(exp, frows)
            assert share <= rf.CAP, f"{what}/{fname}: k {k}: {100 * share:.2f} % of the rays are undecided"
            rows, ctr, status = tgr._first(rt, t.g, rays, k, flt)
            assert status == 0
            tgr._check_first_rows(rows, fwalk, fname, k, f"{what}/{fname}: k {k}", exp)
            assert ctr[0] <= fwalk.box_tests and ctr[1] <= fwalk.leaf_visits


# ------------------------------------------------------------------ 3: signed distance and occupancy
def _sdf_check(rt, t, tris, p, inside, what):
    """test_gpu_small_scenes.test_signed_distance's checks on one uploaded tree"""
    tree = (t.pose.triangles_out, t.pose.nodes_out, t.root, t.count)
    q = sdf_ref.queries(p)
    b = sdf_ref.brute_f64(tris, p, sdf_ref.DEFAULT_DIRS)              # the reference alone: which points are certain
    sure = b["stable"] & (b["dist"] >= sdf_ref.NEAR)
    assert sure.sum() >= 100 and (sure & inside).sum() >= 8 and (sure & ~inside).sum() >= 50
    assert (sdf_ref.vote(b["counts"])[sure] == inside[sure]).all(), "the float64 reference itself: odd inside, even outside"
    for votes, dirs in tgd.COMBOS:
        w = f"{what}/votes {votes}/{'default' if dirs is None else 'caller'} dirs"
        c = sdf_ref.compose(rt, tree, q, votes, dirs)
        r = tgd._run(rt, tree, q, votes, dirs)
        assert c["status"] == 0 and r.st_sdf == 0 and r.st_occ == 0
        assert (r.prim == c["primitive_id"]).all(), f"{w}: {(r.prim != c['primitive_id']).sum()} primitive ids differ"
        assert (tgd._bits(r.sdist) == tgd._bits(c["sdist"])).all(), f"{w}: sdist differs from the composition"
        assert (r.inside == c["inside"]).all(), f"{w}: occupancy differs from the composition"
        assert (r.ctr_sdf[:2] == c["counters"]).all() and (r.ctr_occ[:2] == c["vote_counters"].sum(0)).all(), \
            f"{w}: counters {r.ctr_sdf[:2]} / {r.ctr_occ[:2]}, the composition {c['counters']} / {c['vote_counters'].sum(0)}"
        if dirs is None:
            assert (r.inside.astype(bool)[sure] == inside[sure]).all(), f"{w}: inside wrong against the analytic solid"
            assert ((r.sdist < 0)[sure] == inside[sure]).all()
            M = max(float(np.abs(p).max()), float(np.abs(tris).max()))
            assert (np.abs(np.abs(r.sdist).astype(np.float64) - b["dist"]) <= 4 * 2.0 ** -23 * M).all(), f"{w}: |sdist| against float64"


@pytest.mark.parametrize("name,kind", (("tetra", "bottom_up"), ("tetra", "sah"), ("box", "bottom_up"), ("box", "sah")))
def test_signed_distance_on_the_widest_runs(rt, scenes, name, kind):
    """tetra: one root run of its four leaf slots.  box: twelve leaves (its triangles do not pair) cannot be one run of at most
    seven slots: a 7-slot root run over whatever runs hold the rest"""
    tris = ss.tris(name, scenes)
    inp, root, count = rq._gpu_tree(rt, tris, kind)
    leaves, nodes = tsd._host_tree(rt, inp)
    if name == "tetra":
        t = wt.Tree(leaves, *wt.single_run(nodes, root, count), rt)
        assert t.count == 4 and wt.hist(t.nodes, t.root, t.count) == {4: 1}
    else:
        t = wt.Tree(leaves, *wt.repack(nodes, root, count, widths=(7,), none_every=0, lone_every=0, root_width=7), rt)
        assert t.count == 7 and max(wt.hist(t.nodes, t.root, t.count)) == 7
    p = tss._sdf_points(name, tris)
    inside = ss.in_tetra(p) if name == "tetra" else sdf_ref._in_box(p.astype(np.float64), sdf_ref.BOX_LO, sdf_ref.BOX_HI)
    _sdf_check(rt, t, tris, p, inside, f"{wt.hist(t.nodes, t.root, t.count)}: {name}/{kind}")


@pytest.mark.parametrize("kind", ("bottom_up", "sah"))
def test_signed_distance_on_mixed_widths(rt, kind):
    tris = np.array(sdf_ref.mesh("box"))
    inp, root, count = rq._gpu_tree(rt, tris, kind)
    leaves, nodes = tsd._host_tree(rt, inp)
    t = wt.Tree(leaves, *wt.repack(nodes, root, count, widths=(3, 1, 2, 4), none_every=2, root_width=4), rt)
    h = wt.hist(t.nodes, t.root, t.count)
    assert len(h) >= 3 and ((t.nodes["w28"] >> 29) == wt.NONE).any(), h
    p = sdf_ref.mixed_points("box", 512)
    _sdf_check(rt, t, tris, p, sdf_ref.analytic_inside("box", p), f"mixed widths {h}: box/{kind}")


# ------------------------------------------------------------------ 4: refit
def _write_wide(rt, w):
    """the wide tree into the BuildInput's own nodes_out (the slots behind it keep the binary tree's bytes) -> (root, count)"""
    import torch
    t = w.tree
    w.inp.nodes_out[:len(t.nodes) * 32].copy_(rt.to_device(t.nodes))
    torch.cuda.synchronize()
    return t.root, t.count


@pytest.mark.parametrize("kind", SET_KINDS)
@pytest.mark.parametrize("name", wt.SCENES)
def test_refit(rt, ora, scenes, name, kind):
    w = Wide(rt, wt.tris(name, scenes), kind)          # a BuildInput of its own: the refit rewrites it
    _refit(rt, ora, w, name, f"wide {name}/{kind}", 3)


@pytest.mark.parametrize("n", wt.TINY)
def test_refit_on_a_single_run(rt, ora, scenes, n):
    """walk_run and the expected-arrival count see the root run alone: n leaf slots, no parent slot to climb to"""
    w = Tiny(rt, scenes, n)
    _refit(rt, ora, w, w.name, f"single run of {n}", 0)


def _refit(rt, ora, w, name, what, least_none):
    root, count = _write_wide(rt, w)
    inp = w.inp
    plan = tre._plan(rt, inp, root, count)             # (asserts status 0)
    before = tre._arrays(inp, rt)
    none = np.zeros(len(before[1]), bool)
    none[wt.reached_slots(before[1], root, count)] = True
    none &= (before[1]["w28"] >> 29) == wt.NONE
    assert none.sum() >= least_none
    where = what
    for step, seed in enumerate((3, 4)):
        moved = wt.moved(w.tris, seed)
        assert tre._refit(rt, inp, root, count, plan, moved) == 0
        after = tre._arrays(inp, rt)
        el, en, broken = refit_ref.refit_ref(before[0], before[1], root, count, moved)
        assert not broken
        what = f"{where}, move {step}"
        assert after[0].tobytes() == el.tobytes(), f"{what}: leaf records differ from the reference refit"
        bad = np.nonzero((after[1].view(np.dtype((np.void, 32))) != en.view(np.dtype((np.void, 32)))).reshape(-1))[0]
        assert bad.size == 0, f"{what}: {bad.size} slots differ from the reference refit (first: {bad[:5]})"
        assert after[1][none].tobytes() == before[1][none].tobytes(), f"{what}: a NONE slot was written"
        assert (after[1]["min"] != before[1]["min"]).any()
        before = after
    # rt_intersect_rays on the refitted wide tree equals the walker on the downloaded bytes (rays aimed at the moved scene)
    rays = wt.rays(name, moved)
    g = (inp, root, count)
    for any_hit in (False, True):
        exp, st = ora.walk_rays(before[0], before[1], root, count, rays, any_hit=any_hit)
        got, ctr = rq._query(rt, g, rays, any_hit=any_hit, counters=True)
        tsd._check(got, ctr, exp, st, f"IntersectRays on the refitted tree, {where}, any_hit={any_hit}")
        assert int(st[:, tsd.DROPPED].sum()) == 0 and (exp["primitive_id"] != MISS).mean() >= 0.3


def test_refit_plan_rejects_malformed_runs(rt, scenes):
    import torch
    w = Wide(rt, wt.tris("grid", scenes), "bottom_up")
    root, count = _write_wide(rt, w)
    inp, n = w.inp, w.tris.shape[0]
    slots = rt.NodesBytes(n) // 32
    good = w.tree.nodes
    box = [s for s in wt.reached_slots(good, root, count) if int(good["w28"][s]) >> 29 == wt.BOX]
    plan = rt.device_bytes(rt.RefitPlanBytes(n))
    for what, w12, w28 in (("a Box child with count 0", lambda v: v & wt.MASK, lambda v: v),
                           ("a Box child whose run ends past the slot count", lambda v: (v & wt.MASK) | (7 << 29),
                            lambda v: (wt.BOX << 29) | (slots - 3))):
        bad = good.copy()
        s = box[len(box) // 2]
        bad["w12"][s], bad["w28"][s] = w12(int(bad["w12"][s])), w28(int(bad["w28"][s]))
        inp.nodes_out[:len(bad) * 32].copy_(rt.to_device(bad))
        rt.BuildRefitPlan(inp, root, count, plan)
        torch.cuda.synchronize()
        assert rt.refit_status(plan, n) & rt.RT_REFIT_BAD_TREE, what
    inp.nodes_out[:len(good) * 32].copy_(rt.to_device(good))
    rt.BuildRefitPlan(inp, root, count, plan)
    torch.cuda.synchronize()
    assert rt.refit_status(plan, n) == 0


# ------------------------------------------------------------------ 5: the ray sort
@pytest.mark.parametrize("name,kind", (("grid", "bottom_up"), ("soup", "sah"), ("layers", "sah_pairs")))
def test_sort_rays_on_a_wide_root_run(rt, wide, name, kind):
    w = wide(name, kind)
    t = w.tree
    run = t.nodes[t.root:t.root + t.count]
    assert t.count == 7 and ((run["w28"] >> 29) == wt.NONE).sum() == 1
    _sort_rays(rt, w, f"wide {name}/{kind}")


@pytest.mark.parametrize("n", wt.TINY)
def test_sort_rays_on_a_single_run(rt, scenes, n):
    """the root box is taken over leaf slots alone"""
    _sort_rays(rt, Tiny(rt, scenes, n), f"single run of {n}")


def _sort_rays(rt, w, what):
    t = w.tree
    rays = w.rays.copy()
    rays["tmin"][5], rays["tmax"][5] = 2.0, 1.0                  # a dead ray
    got, ref = trs._check_sort(rt, t.g, rays, what)
    assert np.abs(np.array(ref["box"])).max() < 100, "the NONE slot's bounds are not in the root box"
    assert ref["num_live"] == len(rays) - 1
    plain, pc = rq._query(rt, t.g, rays, counters=True)
    hits, ctr = trs._indexed(rt, t.g, got["rays_dev"], got["order_dev"], len(rays))
    assert hits.tobytes() == plain.tobytes(), "the sorted order gives other records than the unsorted batch"
    assert (ctr[:2] == pc[:2]).all()
