"""GPU tests of the instanced all-hit ray queries on the trees where a traversal goes wrong first (the calls and their
sentinels: tests/ray_hits_instanced_gpu.py; the reference: the numpy walk of tests/ray_hits_instanced_ref.py on the bytes the
device reads).

1. stack edges: stack_scenes.two_level_case -- a comb TLAS of D pending instance leaves over comb BLASes of B pending leaves.
   One stack of 64 serves both levels: instance leaf j is entered at depth j (15, 16, 17: the last LDS level and the first
   private ones are stack bottoms), its BLAS stacks B entries above that, and a push is dropped iff D + B > 64.  Without a
   dropped push the rows are the walk's; with one, both calls set RT_RAY_HITS_STACK_OVERFLOW, agree with each other, and every
   row is a subset of the walk's row;
2. tiny trees: BLASes of one to five triangles and the degenerate scenes flat / points / giant under TLASes of one to five
   instances;
3. wide trees: wide_trees.repack (runs of 1..7 slots, NONE slots first, in the middle and last) on the BLASes, on the TLAS, and
   on both."""
import numpy as np
import pytest

import instance_ref as ir
import ray_hits_instanced_gpu as g
import ray_hits_instanced_ref as rhi
import ray_hits_instanced_scene as rsc
import ray_hits_ref as rh
import small_scenes as ss
import stack_scenes as sc
import test_gpu_instances as tgi
import test_gpu_stack_depths as tsd
import wide_trees as wt
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

F = np.float32
STACK_CASES = sc.TWO_LEVEL + ((17, 4), (60, 4), (61, 4))       # (60, 4): the stack exactly full; (61, 4): one push too many


# ------------------------------------------------------------------ 1: stack edges
@pytest.mark.parametrize("D,B", STACK_CASES)
def test_two_level_combs(rt, D, B):
    case = sc.two_level_case(D, B)
    tl, b = case["tlas"], case["blas"]
    blas_dev = rt.to_device(b["leaves0"]), rt.to_device(b["nodes0"])
    entries = [(blas_dev[0], blas_dev[1], b["root"], b["count"]), (blas_dev[0], blas_dev[1], 0, 0)]
    inst = tgi.Instanced(rt, entries, ir.instance_array(case["mats0"], case["blas_of"]))
    inst.prepare()                                               # the records; the TLAS is the hand-made comb
    assert rt.instance_status(inst.status) == rt.RT_INSTANCE_BAD_BLAS
    tlas_dev = rt.to_device(tl["leaves"]), rt.to_device(tl["nodes0"])
    trees = [(b["leaves0"], b["nodes0"], b["root"], b["count"]), (b["leaves0"], b["nodes0"], 0, 0)]
    s = g.Scene(rt, tlas_dev, (tl["leaves"], tl["nodes0"], tl["root"], tl["count"]), inst.records, D + 1, inst.table, 2, trees,
                keep=(inst, blas_dev))
    assert s.records["flags"][case["bad"]] == rt.RT_INSTANCE_BAD_BLAS and (np.delete(s.records["flags"], case["bad"]) == 0).all()
    rays = case["rays"].astype(rt.RAY)
    ray, ent, _ = s.entered(rays)
    assert len(ray) == len(rays) * D, "every ray reaches every instance leaf; all but the bad instance are entered"
    ref = s.walk(rays)
    r = g.hits(rt, s.args, rays)                                 # (count and collect agree: asserted inside)
    overflow = D + B > sc.STACK
    what = f"comb ({D}, {B})"
    assert sum(len(x) for x in ref[0]) > len(rays)
    if not overflow:
        g.check_against_walk(r, ref, what)
        return
    assert r.st_count == rt.RT_RAY_HITS_STACK_OVERFLOW == r.st_collect, f"{what}: status {r.st_count}"
    for k in range(len(rays)):
        assert rhi.is_subset(r.rows[k], ref[0][k]), f"{what}: ray {k}: not a subset of the walk's row"
    assert r.ctr_count[0] < ref[1] and r.ctr_count[1] < ref[2], "dropped pushes are subtrees that were not visited"
    assert 0 < r.offsets[-1] < rhi.offsets(ref[0])[-1]


# ------------------------------------------------------------------ 2: tiny trees
def _spread(K, ext, seed):
    """K placements: stack_scenes.comb_matrices (rotations, power-of-two scales, one mirror), the first two left on top of each
    other, the others moved apart along x"""
    mats = [np.array(m) for m in sc.comb_matrices(K, seed=seed)]
    for k in range(2, K):
        mats[k][:, 3] += (0.8 * ext * (k - 1), 0.0, 0.0)
    return mats


@pytest.mark.parametrize("name", ss.TINY[:5] + ("flat", "points", "giant"))
def test_tiny_blases_under_tiny_tlases(rt, scenes, name):
    tris = np.array(ss.tris(name, scenes))
    ext = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    src = ss.all_rays(name, tris).astype(rt.RAY)
    seen = 0
    for K in (1, 2, 3, 4, 5):
        blas_kind = ("bottom_up", "sah_pairs", "sah")[K % 3]
        tlas_kind = tgi.TLAS_KINDS[K % 3]
        inp, root, count = _gpu_tree(rt, tris, blas_kind)
        leaves, nodes = tsd._host_tree(rt, inp)
        mats = _spread(K, ext, seed=100 + K)
        inst = tgi.Instanced(rt, [(inp.triangles_out, inp.nodes_out, root, count)], ir.instance_array(mats, [0] * K), tlas_kind)
        inst.frame()
        assert rt.instance_status(inst.status) == 0
        s = g.from_instanced(rt, inst, [(leaves, nodes, root, count)])
        rays = sc.through_instances(src[K % 2::2], mats).astype(rt.RAY)      # every object ray, seen through every instance
        r = g.hits(rt, s.args, rays)
        g.check_against_walk(r, s.walk(rays), f"{name}: {K} instances, BLAS {blas_kind}, TLAS {tlas_kind}")
        seen += int(r.offsets[-1])
        if r.offsets[-1]:
            assert np.concatenate(r.rows)["instance"].max() < K
    assert seen > 0 or name == "points", f"{name}: no ray crossed anything"


# ------------------------------------------------------------------ 3: wide trees
class _Wide:
    """two BLASes (wide_trees' grid and soup) under 40 placements, framed once; the binary trees' host copies and their re-packed
    copies, uploaded"""

    def __init__(self, rt, scenes):
        self.rt = rt
        self.blas, self.wide_blas = [], []
        tris = [wt.tris("grid", scenes), wt.tris("soup", scenes)]
        for t, kind in zip(tris, ("bottom_up", "sah_pairs")):
            inp, root, count = _gpu_tree(rt, t, kind)
            leaves, nodes = tsd._host_tree(rt, inp)
            self.blas.append((inp, (leaves, nodes, root, count)))
            w = wt.Tree(leaves, *wt.repack(nodes, root, count), rt)
            h = wt.hist(w.nodes, w.root, w.count)
            assert set(h) == set(range(1, 8)), h
            assert set(wt.none_places(w.nodes, w.root, w.count)) >= {"first", "middle", "last"}
            self.wide_blas.append(w)
        rng = np.random.default_rng(41)
        exts = [float(np.ptp(t.reshape(-1, 3), axis=0).max()) for t in tris]
        ext = max(exts)
        mats, blas_of = [], []
        for k in range(40):
            R = ir.rotation(*rng.uniform(-3, 3, 3)) * rng.uniform(0.6, 1.4) * (ext / exts[k % 2])     # both BLASes at one size
            if k % 7 == 3:
                R = R @ np.diag([1.0, -1.0, 1.0])
            at = np.array([k % 4, (k // 4) % 4, k // 16], np.float64) * 0.6 * ext + rng.uniform(-0.2, 0.2, 3) * ext
            mats.append(np.hstack([R, at.reshape(3, 1)]))
            blas_of.append(k % 2)
        self.inst = ir.instance_array(mats, blas_of)
        self.world, _, _ = ir.world_triangles(tris, self.inst)
        self.rays = rsc.scene_rays(self.world, n_world=200, per_kind=96, seed=59).astype(rt.RAY)

    def scene(self, wide_blas, wide_tlas, tlas_kind):
        rt = self.rt
        if wide_blas:
            entries = [(w.pose.triangles_out, w.pose.nodes_out, w.root, w.count) for w in self.wide_blas]
            trees = [w.host for w in self.wide_blas]
        else:
            entries = [(inp.triangles_out, inp.nodes_out, t[2], t[3]) for inp, t in self.blas]
            trees = [t for _, t in self.blas]
        inst = tgi.Instanced(rt, entries, self.inst, tlas_kind)
        inst.frame()
        assert rt.instance_status(inst.status) == 0
        s = g.from_instanced(rt, inst, trees)
        if wide_tlas:
            leaves, nodes, root, count = s.tlas
            w = wt.Tree(leaves, *wt.repack(nodes, root, count, none_every=2), rt)
            h = wt.hist(w.nodes, w.root, w.count)
            assert max(h) == 7 and len(h) >= 4 and ((w.nodes["w28"] >> 29) == wt.NONE).any(), h
            s = g.Scene(rt, (w.pose.triangles_out, w.pose.nodes_out), w.host, inst.records, inst.n, inst.table, len(entries), trees,
                        keep=(inst, w, s))
        return s


@pytest.fixture(scope="module")
def wide(rt, scenes):
    return _Wide(rt, scenes)


@pytest.mark.parametrize("tlas_kind", ("bottom_up", "sah"))
@pytest.mark.parametrize("wide_blas,wide_tlas", ((True, False), (False, True), (True, True)))
def test_wide_trees(wide, wide_blas, wide_tlas, tlas_kind):
    s = wide.scene(wide_blas, wide_tlas, tlas_kind)
    r = g.hits(wide.rt, s.args, wide.rays)
    g.check_against_walk(r, s.walk(wide.rays), f"wide BLAS {wide_blas}, wide TLAS {wide_tlas}, TLAS {tlas_kind}")
    assert r.offsets[-1] > len(wide.rays) // 2 and r.counts.max() >= 4
    assert len(np.unique(np.concatenate(r.rows)["instance"])) >= 20
