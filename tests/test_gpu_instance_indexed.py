"""GPU tests of the indexed forms of the instanced and motion ray queries (rt_intersect_rays_instanced_indexed,
rt_intersect_rays_instanced_motion_indexed, rt_intersect_rays_instanced_mixed_indexed, rt_intersect_rays_motion_indexed).

Every check compares with the sibling call on the same device buffers -- code the indexed arms leave unchanged -- so there is
no tolerance anywhere: records are compared as 32-bit words.  Scenes: the 7-instance composition of test_gpu_instances.py (a
mirrored and a non-uniform instance among them) and its moving twin of test_gpu_instance_motion.py, the mixed world of
test_gpu_instance_mixed.py, the two poses of test_gpu_motion.py's grid.  Batches: a shuffled tiled camera batch, a host-made
diffuse bounce off the camera hits, and the "window" ray set -- a few thousand rays each.

1. identity: each entry point through the sorted order (rt_sort_rays over the TLAS), a random permutation and the identity
   list, closest and any hit, both prefetch arms where there are two: hits and instance ids byte-equal to the sibling,
   counters[0:2] equal under a permutation, all four under the identity list.  The instanced call with filter = NULL against
   rt_intersect_rays_instanced and with a filter of all three rule kinds and distinct per-ray records against
   rt_intersect_rays_instanced_filtered; the motion calls with a distinct time per ray;
2. index lists: test_gpu_ray_sort.py's test_index_lists on the instanced call with BOTH output arrays poisoned, and one subset
   case for each of the other three entry points;
3. batch edges: num_indices in {1, 63, 64, 65, 257} with num_rays = 300, and num_rays = 1;
4. one, two and three instances, and one identity instance over a one-triangle tree;
5. the stack edge: a two-level comb on which the instanced queries fill their 64 entries and drop pushes, through a random
   permutation;
6. coherence as a deterministic count: through the sorted order the shuffled camera batch takes strictly fewer wave steps
   than in its own order (the bounce batch is printed only: nobody has measured whether a sort by the TLAS root box helps it);
7. rt_sort_rays over the TLAS -> the indexed closest-hit call -> the indexed any-hit call captured in one HIP graph (a single
   chain on one stream), replayed with the rays rewritten between replays."""
import importlib
import types

import numpy as np
import pytest

import instance_filter_ref as fr
import instance_mixed_ref as mxr
import instance_motion_ref as imr
import instance_ref as ir
import ray_sort_ref
import small_scenes as ss
import stack_scenes as stk
import test_gpu_instance_filter as tgf
import test_gpu_instance_mixed as tgx
import test_gpu_instance_motion as tgm
import test_gpu_instances as ti
import test_gpu_motion as tmo
import test_gpu_ray_queries as rq
import test_gpu_stack_depths as tsd

pytestmark = pytest.mark.gpu

W, H = rq.W, rq.H
BIG = rq.BIG
F = np.float32
MISS = 0xFFFFFFFF
POISON = 0x5A5A5A5A


# ------------------------------------------------------------------ device plumbing
def _dev_rays(rt, rays):
    import torch
    return rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)


def _dev_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


def _dev_f32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F)).cuda()


class Case:
    """one entry point on one scene and one device ray batch of n rays.  direct(hits, ids, ctr, any_hit, pf) is the sibling
    call, indexed(order, num_indices, hits, ids, ctr, any_hit, pf) the new one; tree = (nodes, root, count) of what
    rt_sort_rays reads; has_ids: the call writes instance ids; has_pf: the call takes the scene-size hint"""

    def __init__(self, rt, name, rays, tree, direct, indexed, has_ids=True, has_pf=False):
        self.rt, self.name, self.rays, self.n, self.tree = rt, name, rays, rays.shape[0], tree
        self.direct, self.indexed, self.has_ids, self.has_pf = direct, indexed, has_ids, has_pf

    def _run(self, call):
        """-> (hit words uint32 [n, 4], id words uint32 [n], counters uint64 [4]); both arrays start as POISON"""
        import torch
        hits = torch.empty((self.n, 4), dtype=torch.float32, device="cuda")
        hits.view(torch.int32).fill_(POISON)
        ids = torch.full((self.n,), POISON, dtype=torch.int32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        call(hits, ids, ctr)
        torch.cuda.synchronize()
        return (hits.cpu().numpy().view(np.uint32).reshape(-1, 4), ids.cpu().numpy().view(np.uint32),
                ctr.cpu().numpy().astype(np.uint64))

    def sibling(self, any_hit=False, pf=0):
        return self._run(lambda h, i, c: self.direct(h, i, c, any_hit, pf))

    def through(self, order, num_indices=None, any_hit=False, pf=0):
        return self._run(lambda h, i, c: self.indexed(order, num_indices, h, i, c, any_hit, pf))

    def sort(self):
        """rt_sort_rays over the case's tree -> (device order, host order, num_live)"""
        import torch
        rt = self.rt
        nodes, root, count = self.tree
        order = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        scratch = rt.device_bytes(rt.RaySortScratchBytes(self.n))
        assert rt.SortRays(nodes, root, count, self.rays, order, scratch) == self.n
        torch.cuda.synchronize()
        return order, order.cpu().numpy().view(np.uint32), rt.ray_sort_live(scratch, self.n)


def _instanced_case(sc, d, flt=None, name="instanced"):
    """rt_intersect_rays_instanced_indexed on a test_gpu_instances.Instanced scene against rt_intersect_rays_instanced
    (flt None) or rt_intersect_rays_instanced_filtered (flt: an rt.InstanceHitFilter)"""
    rt = sc.rt
    root, count = sc.root
    args = (sc.tlas.triangles_out, sc.tlas.nodes_out, root, count, sc.records, sc.n, sc.table, len(sc.entries), d)

    def direct(h, i, c, any_hit, pf):
        if flt is None:
            rt.IntersectRaysInstanced(*args, h, i, any_hit=any_hit, num_primitives=pf, counters=c)
        else:
            rt.IntersectRaysInstancedFiltered(*args, h, i, flt, any_hit=any_hit, num_primitives=pf, counters=c)

    def indexed(o, k, h, i, c, any_hit, pf):
        rt.IntersectRaysInstancedIndexed(*args, o, h, i, num_indices=k, filter=flt, any_hit=any_hit, num_primitives=pf, counters=c)
    return Case(rt, name, d, (sc.tlas.nodes_out, root, count), direct, indexed, has_pf=True)


def _instanced_motion_case(sc, d, td):
    """rt_intersect_rays_instanced_motion_indexed on a test_gpu_instance_motion.Moving scene"""
    rt = sc.rt
    root, count = sc.root
    args = (sc.tlas, sc.pose1, root, count, sc.records, sc.n, sc.table, len(sc.entries), d, td)

    def direct(h, i, c, any_hit, pf):
        rt.IntersectRaysInstancedMotion(*args, h, i, any_hit=any_hit, counters=c)

    def indexed(o, k, h, i, c, any_hit, pf):
        rt.IntersectRaysInstancedMotionIndexed(*args, o, h, i, num_indices=k, any_hit=any_hit, counters=c)
    return Case(rt, "instanced motion", d, (sc.tlas.nodes_out, root, count), direct, indexed)


def _mixed_case(sc, d):
    """rt_intersect_rays_instanced_mixed_indexed on a test_gpu_instance_mixed.Mixed scene"""
    rt = sc.rt
    root, count = sc.root
    args = (sc.tlas.triangles_out, sc.tlas.nodes_out, root, count, sc.records, sc.n, sc.table, sc.geom_table, len(sc.entries), d)

    def direct(h, i, c, any_hit, pf):
        rt.IntersectRaysInstancedMixed(*args, h, i, any_hit=any_hit, counters=c)

    def indexed(o, k, h, i, c, any_hit, pf):
        rt.IntersectRaysInstancedMixedIndexed(*args, o, h, i, num_indices=k, any_hit=any_hit, counters=c)
    return Case(rt, "instanced mixed", d, (sc.tlas.nodes_out, root, count), direct, indexed)


def _motion_case(rt, mg, d, td):
    """rt_intersect_rays_motion_indexed on a test_gpu_motion tree (pose0, pose1, plan1, root, count)"""
    pose0, pose1, _, root, count = mg

    def direct(h, i, c, any_hit, pf):
        rt.IntersectRaysMotion(pose0, pose1, root, count, d, td, h, any_hit=any_hit, counters=c)

    def indexed(o, k, h, i, c, any_hit, pf):
        rt.IntersectRaysMotionIndexed(pose0, pose1, root, count, d, td, o, h, num_indices=k, any_hit=any_hit, counters=c)
    return Case(rt, "motion", d, (pose0.nodes_out, root, count), direct, indexed, has_ids=False)


# ------------------------------------------------------------------ the checks
def _same(case, got, exp, what, rows=None):
    """hit and id words of `rows` (default: all) equal; ids of a call that writes none keep their poison"""
    sel = slice(None) if rows is None else rows
    bad = (got[0][sel] != exp[0][sel]).any(axis=1)
    assert not bad.any(), f"{what}: {bad.sum()} hit records differ from the sibling's (first {np.nonzero(bad)[0][:5]})"
    if case.has_ids:
        assert (got[1][sel] == exp[1][sel]).all(), f"{what}: {(got[1][sel] != exp[1][sel]).sum()} instance ids differ"
    else:
        assert (got[1] == POISON).all(), f"{what}: a call without instance ids wrote some"


def _check_identity(case, what, seed=0, min_hits=50):
    """orders {sorted, random permutation, identity} x {closest, any} x the prefetch arms -> the sibling's closest-hit run"""
    n = case.n
    order_dev, order, _ = case.sort()
    assert sorted(order.tolist()) == list(range(n)), f"{what}: the sorted order is not a permutation"
    rng = np.random.default_rng(seed)
    orders = dict(sorted=order_dev, random=_dev_u32(rng.permutation(n)), identity=_dev_u32(np.arange(n)))
    first = None
    for pf in ((0, BIG) if case.has_pf else (0,)):
        for any_hit in (False, True):
            exp = case.sibling(any_hit=any_hit, pf=pf)
            first = exp if first is None else first
            for oname, o in orders.items():
                got = case.through(o, any_hit=any_hit, pf=pf)
                w = f"{what} {case.name} {oname} any={any_hit} pf={pf >= BIG}"
                _same(case, got, exp, w)
                assert (got[2][:2] == exp[2][:2]).all(), f"{w}: counters {got[2][:2]} vs the sibling's {exp[2][:2]}"
                if oname == "identity":
                    assert (got[2] == exp[2]).all(), f"{w}: the identity list is the sibling, wave steps included"
    hit = first[0][:, 1] != MISS
    assert hit.sum() >= min_hits, f"{what}: {hit.sum()} hits: too few to mean anything"
    if case.has_ids:
        assert ((first[1] != MISS) == hit).all()
    return first


def _check_list(case, exp, idx, what, num_indices=None, order_words=None):
    """test_gpu_ray_sort.py's check: listed records are the sibling's, unlisted ones keep the poison -- in both arrays"""
    n = case.n
    idx = np.asarray(idx, np.uint32)
    words = idx if order_words is None else order_words
    got = case.through(_dev_u32(words), num_indices=num_indices)
    listed = np.zeros(n, bool)
    listed[idx[idx < n].astype(np.int64)] = True
    _same(case, got, exp, f"{what}: listed", rows=listed)
    assert (got[0][~listed] == POISON).all(), f"{what}: {(got[0][~listed] != POISON).any(axis=1).sum()} unlisted hit records written"
    if case.has_ids:
        assert (got[1][~listed] == POISON).all(), f"{what}: {(got[1][~listed] != POISON).sum()} unlisted instance ids written"
    return listed


# ------------------------------------------------------------------ scenes and batches, made once
@pytest.fixture(scope="module")
def world(rt, scenes, ora):
    return rq.World(rt, scenes, ora)


@pytest.fixture(scope="module")
def raygen():
    return importlib.import_module("gpu-raytracing_amd.raygen")


def _flat_hits(hits, ids, blas_tris, inst):
    """instanced HIT records with primitive_id replaced by the index into instance_ref.world_triangles's flat array"""
    offs = np.concatenate([[0], np.cumsum([blas_tris[int(b)].shape[0] for b in inst["blas"]])])
    out = hits.copy()
    ok = ids != MISS
    out["primitive_id"][ok] = (offs[ids[ok]] + hits["primitive_id"][ok]).astype(np.uint32)
    return out


class Comp:
    """the composition: its scenes per TLAS kind and the three batches (numpy RAY arrays), never changed"""

    def __init__(self, world, raygen):
        rt = self.rt = world.rt
        self.blas_tris, self.entries, _, self.inst = ti._composition(world)
        self.wt, self.inst_of, self.prim_of = ir.world_triangles(self.blas_tris, self.inst)
        self._sc = {}
        P = self.wt.reshape(-1, 3)
        # from inside the scene box, looking down at the mirrored and the non-uniform instance past three others: half the
        # pixels hit (float64 brute force of the 67 x 45 frame: 1525 hits in five instances; the bounce hits 552 times)
        cam = world.scenes.camera_for_box(P.min(axis=0), P.max(axis=0), yaw=-0.8, pitch=0.9, back=0.5)
        tiled = rq._camera_rays(rt, cam, W, H, 1, True).cpu().numpy().view(rt.RAY).reshape(-1)
        self.camera_tiled = tiled
        self.camera = tiled[np.random.default_rng(41).permutation(tiled.size)]
        # one diffuse bounce off the row-major camera hits: live and dead rays interleaved, origins all over the scene
        prim = rq._camera_rays(rt, cam, W, H, 1, False).cpu().numpy().view(rt.RAY).reshape(-1)
        self.parent_hits, self.parent_ids, _ = self.scene("bottom_up").run(prim)
        bounce, live = raygen.bounce_rays(prim, _flat_hits(self.parent_hits, self.parent_ids, self.blas_tris, self.inst),
                                          self.wt.astype(F), seed=3)
        assert 500 < live < bounce.size
        self.bounce = bounce.astype(rt.RAY)
        self.window = rq._ray_sets(self.wt, seed=29)["window"].astype(rt.RAY)
        self.batches = dict(camera=self.camera, bounce=self.bounce, window=self.window)

    def scene(self, kind):
        if kind not in self._sc:
            sc = ti.Instanced(self.rt, self.entries, self.inst, kind)
            sc.frame()
            assert self.rt.instance_status(sc.status) == 0
            self._sc[kind] = sc
        return self._sc[kind]

    def all_rays(self):
        return np.concatenate([self.camera, self.bounce, self.window])

    def filter(self, batch):
        """all three rule kinds at once (test_gpu_instance_filter._combined: CULL_BACK with CULL_DISABLE / FLIP_FACING on some
        instances, the mirrored one among them; group masks per instance; a random mask and an (instance, primitive) skip per
        ray) -- on the bounce batch the skip is the ray's own parent hit, the self-hit rule"""
        rays = self.batches[batch]
        flt = tgf._combined(types.SimpleNamespace(inst=self.inst), rays.size)
        if batch == "bounce":
            flt.per_ray["skip_instance"], flt.per_ray["skip_id"] = self.parent_ids, self.parent_hits["primitive_id"]
        per_ray = flt.per_ray.view(np.uint32).reshape(-1, 4)[:, :3]
        # (a bounce ray's skip is its parent's hit: neighbouring pixels share triangles, and every missed parent has RT_MISS)
        assert len(np.unique(per_ray, axis=0)) > rays.size // 4, "the per-ray records must tell the rays apart"
        return flt


@pytest.fixture(scope="module")
def comp(world, raygen):
    return Comp(world, raygen)


# ------------------------------------------------------------------ 1: identity
@pytest.mark.parametrize("batch", ("camera", "bounce", "window"))
@pytest.mark.parametrize("kind", ("bottom_up", "sah"))
def test_instanced_indexed_equals_the_direct_call(comp, kind, batch):
    rt = comp.rt
    sc = comp.scene(kind)
    d = _dev_rays(rt, comp.batches[batch])
    plain = _check_identity(_instanced_case(sc, d), f"{kind} {batch}", seed=1)
    flt = comp.filter(batch)
    case = _instanced_case(sc, d, tgf._dev_ifilter(rt, flt), name="instanced filtered")
    kept = _check_identity(case, f"{kind} {batch}", seed=2, min_hits=20)
    assert (kept[0] != plain[0]).any(axis=1).sum() >= 10, "the filter must change answers"
    # a kernel that read per_ray by launch position gives other bytes: the sibling on per-ray records permuted the way a
    # random order would hand them out
    perm = np.random.default_rng(2).permutation(case.n)
    flt.per_ray = np.ascontiguousarray(flt.per_ray[perm])
    wrong = _instanced_case(sc, d, tgf._dev_ifilter(rt, flt)).sibling()
    assert (wrong[0] != kept[0]).any(axis=1).sum() >= 5, "the per-ray records do not tell ray index from launch position"


@pytest.fixture(scope="module")
def moving(world, comp):
    """the composition with two key transforms per instance (test_gpu_instance_motion's), under a bottom-up TLAS"""
    rt = world.rt
    tris, minst = imr.composition(world.scenes)
    assert (minst["object_to_world0"] == comp.inst["object_to_world"]).all()
    sc = tgm.Moving(rt, comp.entries, minst, "bottom_up")
    sc.frame()
    assert rt.instance_status(sc.status) == 0 and rt.refit_status(sc.plan, sc.n) == 0
    return sc


def _times(n, seed):
    """a distinct time per ray in [0, 1), with the two ends and one value outside mixed in"""
    t = np.random.default_rng(seed).random(n).astype(F)
    t[:3] = (0.0, 1.0, 1.5)
    assert len(np.unique(t)) > n - n // 50
    return t


@pytest.mark.parametrize("batch", ("camera", "bounce", "window"))
def test_instanced_motion_indexed_equals_the_direct_call(comp, moving, batch):
    rt = comp.rt
    rays = comp.batches[batch]
    times = _times(rays.size, seed=5)
    case = _instanced_motion_case(moving, _dev_rays(rt, rays), _dev_f32(times))
    got = _check_identity(case, batch, seed=3)
    # times by launch position would give other bytes
    other = _instanced_motion_case(moving, case.rays, _dev_f32(times[np.random.default_rng(3).permutation(rays.size)])).sibling()
    assert (other[0] != got[0]).any(axis=1).sum() > 20, "the times do not tell ray index from launch position"


@pytest.fixture(scope="module")
def mixed_scene(rt):
    """the mixed world of test_gpu_instance_mixed (triangle and sphere BLASes under one bottom-up TLAS) and its rays"""
    import torch
    w = mxr.world()
    b = tgx.Blases(rt, w.data, w.kinds, mxr.BLAS_TREES)
    sc = tgx.Mixed(rt, b.entries, b.geoms, w.instances, "bottom_up")
    sc.frame()
    torch.cuda.synchronize()
    assert rt.instance_status(sc.status) == 0
    rays = mxr.world_rays(w, 1200, seed=31).astype(rt.RAY)
    return sc, rays[np.random.default_rng(6).permutation(rays.size)], b


def test_instanced_mixed_indexed_equals_the_direct_call(rt, mixed_scene):
    sc, rays, _ = mixed_scene
    case = _mixed_case(sc, _dev_rays(rt, rays))
    got = _check_identity(case, "mixed world", seed=4)
    kinds = np.asarray(mxr.world().kinds)[mxr.world().instances["blas"][got[1][got[1] != MISS]]]
    assert (kinds == mxr.TRIANGLES).sum() > 50 and (kinds == mxr.SPHERES).sum() > 50, "hits in both kinds of BLAS"
    # no table: the call forwards to the instanced indexed one, as the sibling forwards to the instanced one
    import torch
    rt_args = (sc.tlas.triangles_out, sc.tlas.nodes_out) + sc.root + (sc.records, sc.n, sc.table, None, len(sc.entries), case.rays)
    h = torch.zeros((case.n, 4), dtype=torch.float32, device="cuda")
    i = torch.zeros(case.n, dtype=torch.int32, device="cuda")
    eh, ei = torch.zeros_like(h), torch.zeros_like(i)
    rt.IntersectRaysInstancedMixedIndexed(*rt_args, _dev_u32(np.random.default_rng(7).permutation(case.n)), h, i)
    rt.IntersectRaysInstancedMixed(*rt_args, eh, ei)
    torch.cuda.synchronize()
    assert torch.equal(h.view(torch.int32), eh.view(torch.int32)) and torch.equal(i, ei)


@pytest.fixture(scope="module")
def motion_tree(rt, scenes):
    """the grid of test_gpu_motion and its smooth displacement under an SAH tree with pairs; camera and window rays"""
    w = tmo.World(rt, scenes)
    mg = w.gpu("grid", "sah_pairs")
    t0, t1 = w.poses("grid")
    cam = rq._scene("grid", scenes)[1]
    tiled = rq._camera_rays(rt, cam, W, H, 1, True).cpu().numpy().view(rt.RAY).reshape(-1)
    rays = np.concatenate([tiled, rq._ray_sets(np.concatenate([t0, t1]), seed=37)["window"].astype(rt.RAY)])
    return mg, rays[np.random.default_rng(8).permutation(rays.size)]


def test_motion_indexed_equals_the_direct_call(rt, motion_tree):
    mg, rays = motion_tree
    times = _times(rays.size, seed=9)
    case = _motion_case(rt, mg, _dev_rays(rt, rays), _dev_f32(times))
    got = _check_identity(case, "grid/sah_pairs", seed=5)
    other = _motion_case(rt, mg, case.rays, _dev_f32(times[np.random.default_rng(5).permutation(rays.size)])).sibling()
    assert (other[0] != got[0]).any(axis=1).sum() > 20, "the times do not tell ray index from launch position"


# ------------------------------------------------------------------ 2: index lists
def test_index_lists(comp):
    rt = comp.rt
    rays = np.concatenate([comp.bounce, comp.camera])
    n = rays.size
    case = _instanced_case(comp.scene("sah"), _dev_rays(rt, rays))
    exp = case.sibling()
    rng = np.random.default_rng(9)
    check = lambda idx, what, **kw: _check_list(case, exp, idx, what, **kw)

    sub = rng.permutation(n)[:n // 3]
    assert not check(sub, "strict subset").all()
    assert check(sub[:1000 + 37], "not a multiple of 64").sum() == 1037
    assert check(sub[:1], "one index").sum() == 1
    dup = np.concatenate([sub[:500], sub[:500], sub[:500][::-1], np.full(100, sub[0])])
    assert check(dup, "duplicates").sum() == 500
    skip = np.concatenate([sub[:300], [n, n + 1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF], np.full(64, 0xFFFFFFFF), sub[300:600]])
    assert check(rng.permutation(skip), "indices >= num_rays").sum() == 600
    assert check(np.full(200, 0xFFFFFFFF), "nothing but skipped indices").sum() == 0
    longer = np.concatenate([rng.permutation(n), rng.permutation(n)[:n // 2], np.full(77, 0xFFFFFFFF)])
    assert longer.size > n and check(longer, "num_indices > num_rays").all()
    # num_indices limits a longer list: the words past it are not read as indices
    words = np.concatenate([sub[:130], np.setdiff1d(np.arange(n), sub[:130])])
    assert check(sub[:130], "num_indices < len(order)", num_indices=130, order_words=words).sum() == 130
    # the live prefix of a sorted order is the batch's active-ray list
    order_dev, order, live = case.sort()
    alive = ray_sort_ref.live(rays)
    assert live == alive.sum() and 0 < live < n
    got = case.through(order_dev, num_indices=live)
    _same(case, got, exp, "live prefix", rows=alive)
    assert (got[0][~alive] == POISON).all() and (got[1][~alive] == POISON).all(), "live prefix: a dead ray's records were written"
    # the filtered arm through a subset: per-ray records by ray index, unlisted records alone
    fcase = _instanced_case(comp.scene("sah"), case.rays, tgf._dev_ifilter(rt, tgf._combined(types.SimpleNamespace(inst=comp.inst), n)))
    assert not _check_list(fcase, fcase.sibling(), sub, "filtered: strict subset").all()


def test_index_lists_of_the_other_entry_points(rt, comp, moving, mixed_scene, motion_tree):
    rng = np.random.default_rng(10)
    rays = comp.all_rays()
    cases = [_instanced_motion_case(moving, _dev_rays(rt, rays), _dev_f32(_times(rays.size, seed=11)))]
    sc, mrays, _ = mixed_scene
    cases.append(_mixed_case(sc, _dev_rays(rt, mrays)))
    mg, grays = motion_tree
    cases.append(_motion_case(rt, mg, _dev_rays(rt, grays), _dev_f32(_times(grays.size, seed=12))))
    for case in cases:
        n = case.n
        sub = np.concatenate([rng.permutation(n)[:n // 3 + 5], [n, 0xFFFFFFFF]])
        listed = _check_list(case, case.sibling(), sub, f"{case.name}: strict subset")
        assert listed.sum() == n // 3 + 5


# ------------------------------------------------------------------ 3: batch edges
@pytest.mark.parametrize("num_indices", (1, 63, 64, 65, 257))
def test_batch_edges(comp, num_indices):
    rt = comp.rt
    rays = comp.all_rays()[np.random.default_rng(13).permutation(comp.all_rays().size)[:300]]
    case = _instanced_case(comp.scene("bottom_up"), _dev_rays(rt, rays))
    exp = case.sibling()
    assert (exp[1] != MISS).sum() > 30
    idx = np.random.default_rng(num_indices).permutation(300)[:num_indices]
    assert _check_list(case, exp, idx, f"num_indices {num_indices}").sum() == num_indices
    # the same count read from the front of a longer buffer
    words = np.concatenate([idx, np.setdiff1d(np.arange(300), idx)])
    assert _check_list(case, exp, idx, f"num_indices {num_indices} of 300 words", num_indices=num_indices,
                       order_words=words).sum() == num_indices


def test_one_ray(rt, comp, moving):
    hit = comp.window[np.nonzero(comp.scene("bottom_up").run(comp.window)[1] != MISS)[0][:1]]
    assert hit.size == 1
    d = _dev_rays(rt, hit)
    for case in (_instanced_case(comp.scene("bottom_up"), d), _instanced_motion_case(moving, d, _dev_f32([0.0]))):
        exp = case.sibling()
        assert exp[1][0] != MISS
        assert _check_list(case, exp, [0], f"{case.name}: one ray").all()
        assert _check_list(case, exp, [0, 0, 1, 0xFFFFFFFF, 0], f"{case.name}: one ray, five indices").all()
        assert not _check_list(case, exp, [1, 2, 300], f"{case.name}: one ray, no index in range").any()


# ------------------------------------------------------------------ 4: few instances and tiny BLASes
@pytest.mark.parametrize("count", (1, 2, 3))
@pytest.mark.parametrize("kind", ti.TLAS_KINDS)
def test_few_instances(comp, count, kind):
    rt = comp.rt
    sub = comp.inst[[0, 6, 2][:count]]
    sc = ti.Instanced(rt, comp.entries, sub, kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    wt, _, _ = ir.world_triangles(comp.blas_tris, sub)
    rays = ti._world_rays(wt, 800, seed=23 + count).astype(rt.RAY)
    _check_identity(_instanced_case(sc, _dev_rays(rt, rays)), f"{count} instances TLAS {kind}", seed=count)


@pytest.mark.parametrize("kind", ti.TLAS_KINDS)
def test_identity_instance_over_one_triangle(rt, scenes, kind):
    t = ss.tris("n1", scenes)
    inp, root, count = rq._gpu_tree(rt, t, "bottom_up")
    sc = ti.Instanced(rt, [(inp.triangles_out, inp.nodes_out, root, count)], ir.instance_array([np.eye(3, 4)], [0]), kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0
    rays = ss.all_rays("n1", t).astype(rt.RAY)
    got = _check_identity(_instanced_case(sc, _dev_rays(rt, rays)), f"n1 TLAS {kind}", seed=6, min_hits=20)
    assert set(got[1].tolist()) == {0, MISS}


# ------------------------------------------------------------------ 5: the stack edge
def test_full_stack_drops_pushes(rt, ora):
    """tlas_comb(60) over tri_comb(8) BLASes (stack_scenes.TWO_LEVEL): instances entered at stack bottoms >= 56 fill the 64
    entries and drop pushes -- through a random permutation exactly as in the sibling"""
    import torch
    case = stk.two_level_case(60, 8)
    scene = tsd._comb_scene(rt, case)
    rays = case["rays"]
    obj, ent = stk.static_object_rays(rays, scene.records, scene.counts)
    _, _, st = scene.walk(ora, rays, obj, ent, False)
    assert st[:, tsd.DEPTH].max() == stk.STACK and st[:, tsd.DROPPED].sum() > 0, "the scene must fill the stack and drop pushes"
    d = _dev_rays(rt, rays)
    n = len(rays)
    order = _dev_u32(np.random.default_rng(14).permutation(n))
    s, tl = scene.static, scene.tlas
    args = (scene.pose0.triangles_out, scene.pose0.nodes_out, tl["root"], tl["count"], s.records, scene.K, s.table, 2, d)
    flt = tgf._dev_ifilter(rt, fr.InstanceFilter(fr.CULL_BACK))
    static = Case(rt, "instanced", d, None,
                  lambda h, i, c, a, pf: rt.IntersectRaysInstanced(*args, h, i, any_hit=a, num_primitives=pf, counters=c),
                  lambda o, k, h, i, c, a, pf: rt.IntersectRaysInstancedIndexed(*args, o, h, i, num_indices=k, any_hit=a,
                                                                               num_primitives=pf, counters=c))
    culled = Case(rt, "instanced filtered", d, None,
                  lambda h, i, c, a, pf: rt.IntersectRaysInstancedFiltered(*args, h, i, flt, any_hit=a, num_primitives=pf, counters=c),
                  lambda o, k, h, i, c, a, pf: rt.IntersectRaysInstancedIndexed(*args, o, h, i, num_indices=k, filter=flt, any_hit=a,
                                                                               num_primitives=pf, counters=c))
    td = torch.from_numpy(np.resize(np.array(stk.TAUS, F), n)).cuda()
    m = scene.moving
    margs = (scene.pose0, scene.pose1, tl["root"], tl["count"], m.records, scene.K, m.table, 2, d, td)
    motion = Case(rt, "instanced motion", d, None,
                  lambda h, i, c, a, pf: rt.IntersectRaysInstancedMotion(*margs, h, i, any_hit=a, counters=c),
                  lambda o, k, h, i, c, a, pf: rt.IntersectRaysInstancedMotionIndexed(*margs, o, h, i, num_indices=k, any_hit=a,
                                                                                      counters=c))
    for c, pfs in ((static, (0, BIG)), (culled, (0, BIG)), (motion, (0,))):
        for pf in pfs:
            for any_hit in (False, True):
                exp = c.sibling(any_hit=any_hit, pf=pf)
                got = c.through(order, any_hit=any_hit, pf=pf)
                w = f"comb (60, 8) {c.name} any={any_hit} pf={pf >= BIG}"
                _same(c, got, exp, w)
                assert (got[2][:2] == exp[2][:2]).all(), f"{w}: counters {got[2][:2]} vs {exp[2][:2]}"
                assert (exp[1] != MISS).sum() > 10


# ------------------------------------------------------------------ 6: coherence
def _steps(c):
    return int(c[2] + c[3])


def test_sorting_restores_coherence(comp):
    """A deterministic count: through the order rt_sort_rays gives over the TLAS, the shuffled tiled camera batch takes strictly
    fewer wave steps (counters[2] + counters[3]) than in its own order.  The unshuffled batch is printed as the floor.  For
    the bounce batch the two counts are printed and nothing is asserted."""
    rt = comp.rt
    sc = comp.scene("bottom_up")
    floor = _instanced_case(sc, _dev_rays(rt, comp.camera_tiled)).sibling()[2]
    for batch in ("camera", "bounce"):
        case = _instanced_case(sc, _dev_rays(rt, comp.batches[batch]))
        order_dev, _, _ = case.sort()
        own = case.through(_dev_u32(np.arange(case.n)))[2]
        through = case.through(order_dev)[2]
        direct = case.sibling()[2]
        assert (direct == own).all(), "the identity list is the direct call, wave steps included"
        assert (through[:2] == own[:2]).all()
        print(f"composition {batch}: wave steps in the batch's own order {_steps(own)}, sorted {_steps(through)} "
              f"(ratio {_steps(through) / _steps(own):.3f})" + (f", unshuffled {_steps(floor)}" if batch == "camera" else ""))
        if batch == "camera":
            assert _steps(through) < _steps(own)


# ------------------------------------------------------------------ 7: hipGraph
def test_sort_and_indexed_queries_in_a_hip_graph(comp):
    import torch
    rt = comp.rt
    sc = comp.scene("bottom_up")
    root, count = sc.root
    n = comp.bounce.size
    batches = [comp.bounce, comp.all_rays()[-n:], comp.bounce[np.random.default_rng(1).permutation(n)]]
    assert all(b.size == n for b in batches)
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    hits, anyh = (torch.zeros((n, 4), dtype=torch.float32, device="cuda") for _ in range(2))
    ids, ids_any = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    scratch = rt.device_bytes(rt.RaySortScratchBytes(n))
    args = (sc.tlas.triangles_out, sc.tlas.nodes_out, root, count, sc.records, sc.n, sc.table, len(sc.entries), rays)

    def one_frame():
        rt.SortRays(sc.tlas.nodes_out, root, count, rays, order, scratch)
        rt.IntersectRaysInstancedIndexed(*args, order, hits, ids)
        rt.IntersectRaysInstancedIndexed(*args, order, anyh, ids_any, any_hit=True)

    rays.copy_(_dev_rays(rt, batches[0]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()                       # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for b in (batches[1], batches[2], batches[0]):
        rays.copy_(_dev_rays(rt, b))
        order.fill_(-1)
        for t in (hits, anyh):
            t.view(torch.int32).fill_(POISON)
        for t in (ids, ids_any):
            t.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert sorted(order.cpu().numpy().view(np.uint32).tolist()) == list(range(n)), "the replayed sort gives a permutation"
        case = _instanced_case(sc, rays)
        for got_h, got_i, any_hit in ((hits, ids, False), (anyh, ids_any, True)):
            exp = case.sibling(any_hit=any_hit)
            assert (got_h.cpu().numpy().view(np.uint32).reshape(-1, 4) == exp[0]).all(), f"replay any={any_hit}: hits"
            assert (got_i.cpu().numpy().view(np.uint32) == exp[1]).all(), f"replay any={any_hit}: instance ids"
        assert (ids.cpu().numpy().view(np.uint32) != MISS).sum() > 100
