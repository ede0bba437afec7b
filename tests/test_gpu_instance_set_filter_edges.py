"""GPU tests of the FILTERED arms of the instanced all-hit and first-K kernels on the smallest shapes where an arm can go wrong
(the calls and their sentinels: tests/instance_set_filter_gpu.py; the reference: tests/instance_set_filter_ref.py on the bytes
the device reads).

1. one instance of a hand-made one-triangle BLAS, and of a hand-made pair leaf folded so that a ray crosses A from behind and B
   from the front: under CULL_BACK B is kept and A is culled, under an identity and under a mirror;
2. wide trees: wide_trees.repack (runs of 1..7 slots, NONE slots first, in the middle and last) on the BLASes and the TLAS;
3. a TLAS of one instance (the mirror);
4. instances 9 - 11 (singular, bad BLAS, empty tree) together with masks: admitted by the mask they are still never entered;
5. NaN and empty-window rays with per-ray records;
6. num_rays not a multiple of 64, and num_rays = 0;
7. stack edges, one comb scene for the three new arms: stack_scenes.two_level_case at the depth that just fits (status 0, rows
   equal the reference) and at the depth that just overflows (the status flag; every row a subset -- first-K: a sorted subset --
   of the reference row)."""
import numpy as np
import pytest

import instance_filter_ref as ifr
import instance_ref as ir
import instance_set_filter_gpu as ig
import instance_set_filter_ref as isf
import instance_set_filter_scene as fsc
import ray_first_instanced_gpu as fg
import ray_first_instanced_ref as rfi
import ray_hits_instanced_gpu as g
import ray_hits_instanced_ref as rhi
import ray_hits_ref as rh
import stack_scenes as sc
import test_gpu_instances as tgi
import test_gpu_ray_hits_instanced_edges as hie
from test_gpu_ray_first_instanced_edges import _comb_scene
from test_gpu_ray_hits_instanced import World

pytestmark = pytest.mark.gpu

F = np.float32
SENT = g.SENT


def _both(rt, s, rays, flt, what, ks=(1, 4)):
    """the three arms against the reference on a scene without dropped pushes -> (all-hit Result, Walk)"""
    walk = ig.Walk(s, rays, flt)
    hf = ig.dev_filter(rt, flt)
    r = ig.hits(rt, s.args, rays, hf)
    ig.check_hits(r, walk, what)
    for k in ks:
        rows, ctr, status = ig.first(rt, s.args, rays, k, hf)
        assert status == 0, f"{what}: k {k}: status {status}"
        fg.check_rows(rows, walk, k, what)
        assert ctr[0] <= r.ctr_count[0] and ctr[1] <= r.ctr_count[1]
    return r, walk


# ------------------------------------------------------------------ 1: one triangle; a pair leaf with B kept and A culled
def _hand_blas(rt, pair):
    """a BLAS of one leaf record under a one-slot root run.  pair: the folded quad A = (v0, v1, v2), B = (v2, v1, v3); else A only"""
    nodes = np.zeros(2, sc.NODE)
    nodes["min"][0], nodes["max"][0] = (-2, -2, -2), (2, 2, 2)
    nodes["w28"][0] = (sc.TRI << 29) | 0                       # (w12's count 0: a leaf)
    lv = np.zeros(1, sc.TRIANGLE_PAIR)
    lv["v0"], lv["v1"], lv["v2"] = (-1, 0.5, 1), (0, 0, 0), (0, 1, 0)
    lv["v3"] = (1, 0.5, 1) if pair else lv["v2"]
    lv["primitive_id_0"], lv["primitive_id_1"] = 0, 1
    dev = rt.to_device(lv), rt.to_device(nodes)
    return (dev[0], dev[1], 0, 1), (lv, nodes, 0, 1)


@pytest.mark.parametrize("mirror", (False, True))
@pytest.mark.parametrize("pair", (False, True))
def test_one_instance_of_one_leaf(rt, pair, mirror):
    entry, tree = _hand_blas(rt, pair)
    M = np.hstack([np.diag([-1.0, 1.0, 1.0]) if mirror else np.eye(3), np.zeros((3, 1))])
    inst = tgi.Instanced(rt, [entry], ir.instance_array([M], [0]), "bottom_up")
    inst.frame()
    assert rt.instance_status(inst.status) == 0
    s = g.from_instanced(rt, inst, [tree])
    # along +x at z = 0.5: the wing through x = -0.5, then the wing through x = +0.5
    ys = np.linspace(0.35, 0.65, 7)
    rays = np.zeros(len(ys), rt.RAY)
    rays["origin"] = [(-3.0, y, 0.5) for y in ys]
    rays["dir"], rays["tmin"], rays["tmax"] = (1.0, 0.0, 0.0), 0.0, np.inf
    what = f"one leaf (pair {pair}, mirror {mirror})"
    plain, _ = _both(rt, s, rays, isf.keep_all(), what + " keep-all", ks=(1, 2))
    assert (plain.counts == (2 if pair else 1)).all()
    r, walk = _both(rt, s, rays, ifr.InstanceFilter(ifr.CULL_BACK), what + " CULL_BACK", ks=(1, 2))
    # A is crossed from behind and B from the front -- and so are their mirror images, which swap places: B is kept and A is
    # culled, at t = 3.5 (x = +0.5) under the identity and at t = 2.5 (x = -0.5) under the mirror
    kept_t = 2.5 if mirror else 3.5
    for i, row in enumerate(r.rows):
        if not pair:
            assert len(row) == 0, f"{what}: ray {i}: A alone is a back face: {row}"
            continue
        assert len(row) == 1 and abs(float(row["t"][0]) - kept_t) < 1e-5, f"{what}: ray {i}: {row}"
        assert int(row["primitive_id"][0]) == 1, f"{what}: ray {i}: B is kept and A is culled"
    if pair:
        # (identity: the culled wing is the nearer one, and the row starts behind it: it did not shrink the bound)
        rows, _, _ = ig.first(rt, s.args, rays, 1, ig.dev_filter(rt, ifr.InstanceFilter(ifr.CULL_BACK)))
        assert (np.abs(rows["t"][:, 0] - kept_t) < 1e-5).all() and (rows["primitive_id"][:, 0] == 1).all()
        skip = np.zeros(len(rays), ifr.INSTANCE_RAY_FILTER)
        skip["mask"], skip["skip_instance"], skip["skip_id"] = ifr.ALL, 0, (1 if mirror else 0)    # the near wing's id
        r, _ = _both(rt, s, rays, fsc.skip_filter(skip), what + " skip the near wing", ks=(1, 2))
        assert all(len(row) == 1 and abs(float(row["t"][0]) - 3.5) < 1e-5 for row in r.rows)


# ------------------------------------------------------------------ 2: wide trees
@pytest.fixture(scope="module")
def wide(rt, scenes):
    return hie._Wide(rt, scenes)


@pytest.mark.parametrize("name", ("cull_back", "masks"))
@pytest.mark.parametrize("wide_blas,wide_tlas", ((True, False), (False, True), (True, True)))
def test_wide_trees(wide, wide_blas, wide_tlas, name):
    s = wide.scene(wide_blas, wide_tlas, "sah" if wide_blas else "bottom_up")
    flt = ifr.make_arm(name, wide.inst.size, len(wide.rays))
    r, walk = _both(wide.rt, s, wide.rays, flt, f"wide BLAS {wide_blas}, wide TLAS {wide_tlas}, {name}")
    assert r.offsets[-1] > len(wide.rays) // 4 and len(np.unique(np.concatenate(r.rows)["instance"])) >= 10


# ------------------------------------------------------------------ 3, 4, 5, 6 on the 12-instance scene
@pytest.fixture(scope="module")
def world(rt, scenes):
    return World(rt, scenes)


@pytest.mark.parametrize("tlas_kind", ("bottom_up", "sah"))
def test_tlas_of_one_instance(world, tlas_kind):
    rt = world.rt
    s = world.make(tlas_kind, "sah_pairs", world.inst[[fsc.MIRROR]])
    rays = world.rays[::2]
    plain, _ = _both(rt, s, rays, isf.keep_all(), "one instance, keep-all")
    r, _ = _both(rt, s, rays, ifr.InstanceFilter(ifr.CULL_BACK), "one instance, CULL_BACK")
    assert 0 < r.offsets[-1] < plain.offsets[-1]
    r, _ = _both(rt, s, rays, fsc.none_admitted(1), "one instance, masked")
    assert r.offsets[-1] == 0 and r.ctr_count[1] == 0 and r.ctr_count[0] > 0


def test_never_entered_instances_with_masks(world):
    rt = world.rt
    s = world.scene("bottom_up", "sah_pairs")
    num = world.inst.size
    # only 9, 10, 11 admitted: singular, bad BLAS, the empty tree -- nothing is entered
    im = np.where(np.isin(np.arange(num), fsc.NEVER), 1, 2).astype(np.uint32)
    flt = ifr.InstanceFilter(ifr.CULL_FRONT, 1, ifr.instance_filters(num, masks=im))
    r, walk = _both(rt, s, world.rays, flt, "only the never-entered instances admitted")
    assert r.offsets[-1] == 0 and r.ctr_count[1] == 0 and walk.leaf_visits == 0
    # 9, 10, 11 and the even instances admitted, with flags on the never-entered ones
    im = np.where(np.isin(np.arange(num), fsc.NEVER) | (np.arange(num) % 2 == 0), 1, 2).astype(np.uint32)
    fl = np.where(np.isin(np.arange(num), fsc.NEVER), ifr.FLIP_FACING | ifr.CULL_DISABLE, 0).astype(np.uint32)
    flt = ifr.InstanceFilter(ifr.CULL_BACK, 1, ifr.instance_filters(num, masks=im, flags=fl))
    r, _ = _both(rt, s, world.rays, flt, "the never-entered and the even instances admitted")
    seen = np.unique(np.concatenate(r.rows)["instance"]).tolist()
    assert seen and all(k % 2 == 0 and k < 9 for k in seen)


def test_dead_rays_with_per_ray_records(world):
    rt = world.rt
    s = world.scene("sah", "bottom_up")
    nan = F(np.nan)
    rays = world.rays[:200].copy()
    dead = np.arange(5, 200, 23)
    for j, i in enumerate(dead):
        if j % 4 == 0:
            rays["tmin"][i], rays["tmax"][i] = 5.0, 1.0
        elif j % 4 == 1:
            rays["origin"][i, j % 3] = nan
        elif j % 4 == 2:
            rays["dir"][i] = nan
        else:
            rays["tmax"][i] = nan
    assert (~rh.live(rays)).sum() == len(dead)
    flt = ifr.make_arm("masks", world.inst.size, len(rays))
    flt.flags = ifr.CULL_BACK
    r, _ = _both(rt, s, rays, flt, "dead rays")
    assert (r.counts[dead] == 0).all() and r.counts.sum() > 0
    rows, _, _ = ig.first(rt, s.args, rays, 3, ig.dev_filter(rt, flt))
    assert rows[dead].tobytes() == rfi.pad_items(len(dead) * 3).tobytes()
    r = ig.hits(rt, s.args, rays[dead], ig.dev_filter(rt, ifr.InstanceFilter(ifr.CULL_BACK, ifr.ALL, None, flt.per_ray[dead])))
    assert (r.offsets == 0).all() and (r.ctr_count == 0).all()


def test_batch_ends_and_the_empty_batch(world):
    import torch
    rt = world.rt
    s = world.scene("hybrid", "sah_pairs")
    rays = world.rays[:300]
    flt = ifr.make_arm("masks", world.inst.size, len(rays))
    flt.flags = ifr.CULL_FRONT
    full = ig.hits(rt, s.args, rays, ig.dev_filter(rt, flt))
    first, _, _ = ig.first(rt, s.args, rays, 3, ig.dev_filter(rt, flt))
    assert full.offsets[-1] > 0
    for n in (1, 63, 65, 257):
        hf = ig.dev_filter(rt, ifr.InstanceFilter(flt.flags, flt.ray_mask, flt.per_instance, flt.per_ray[:n]))
        r = ig.hits(rt, s.args, rays[:n], hf)                    # (sentinels: checked inside)
        assert (r.offsets == full.offsets[:n + 1]).all(), f"batch of {n}"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r.rows, full.rows[:n])), f"batch of {n}: rows differ"
        rows, _, _ = ig.first(rt, s.args, rays[:n], 3, hf)
        assert rows.tobytes() == np.ascontiguousarray(first[:n]).tobytes(), f"batch of {n}: first-K rows differ"
    # num_rays = 0: nothing runs, nothing is written
    hf = ig.dev_filter(rt, ifr.InstanceFilter(ifr.CULL_BACK))
    off = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    empty = torch.empty((0, 8), dtype=torch.float32, device="cuda")
    hits = torch.full((8, 2, 4), 7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((8, 2), 7, dtype=torch.int32, device="cuda")
    assert rt.RayHitsCountInstancedFiltered(*s.args, empty, hf, off[:1]) == 0
    assert rt.RayHitsCollectInstancedFiltered(*s.args, empty, hf, off[:1], hits.view(-1, 4), ids.view(-1)) == 0
    assert rt.RayFirstHitsInstancedFiltered(*s.args, empty, 2, hf, hits[:0], ids[:0]) == 0
    torch.cuda.synchronize()
    assert off.cpu().numpy().tolist() == [SENT] * 4 and bool((hits == 7.0).all()) and bool((ids == 7).all())
    o, h, i = rt.RayHitsInstancedFiltered(*s.args, empty, hf)
    assert o.cpu().numpy().tolist() == [0] and tuple(h.shape) == (0, 4) and tuple(i.shape) == (0,)


# ------------------------------------------------------------------ 7: stack edges
@pytest.mark.parametrize("D,B", ((60, 4), (61, 4)))
def test_comb_at_the_stack_edge(rt, D, B):
    case = sc.two_level_case(D, B)
    s = _comb_scene(rt, case)
    rays = case["rays"].astype(rt.RAY)
    n, num = len(rays), D + 1
    # the instance the case sets aside for masking is masked; every ray skips primitive 0 of the instance of TLAS leaf D
    im = np.full(num, 1, np.uint32)
    im[case["masked"]] = 2
    per_ray = np.zeros(n, ifr.INSTANCE_RAY_FILTER)
    per_ray["mask"], per_ray["skip_instance"], per_ray["skip_id"] = 1, int(case["tlas"]["ids"][D]), 0
    flt = ifr.InstanceFilter(0, 0, ifr.instance_filters(num, masks=im), per_ray)
    hf = ig.dev_filter(rt, flt)
    walk = ig.Walk(s, rays, flt)
    what = f"comb ({D}, {B})"
    assert sum(len(x) for x in walk.rows) > n
    assert not any((row["instance"] == case["masked"]).any() for row in walk.rows)
    # what the definition needs, by the sequential model in the shipped order on the device's records
    need = [isf.model(s.tlas, s.records, s.trees, rays[i], i, flt, 1).max_depth for i in (0, n - 1)]
    assert need[0] == need[1] == D + B, f"{what}: the model needs {need} entries"
    fits = D + B <= sc.STACK
    r = ig.hits(rt, s.args, rays, hf)
    if fits:
        ig.check_hits(r, walk, what)
    else:
        assert r.st_count == rt.RT_RAY_HITS_STACK_OVERFLOW == r.st_collect, f"{what}: status {r.st_count}"
        for i in range(n):
            assert rhi.is_subset(r.rows[i], walk.rows[i]), f"{what}: ray {i}: not a subset of the reference row"
        assert r.ctr_count[0] < walk.box_tests and r.ctr_count[1] < walk.leaf_visits
    for k in (1, 3):
        rows, ctr, status = ig.first(rt, s.args, rays, k, hf)
        if fits:
            assert status == 0 and fg.check_rows(rows, walk, k, what) == 0
            assert ctr[0] == walk.box_tests and ctr[1] == walk.leaf_visits, "no bound prunes a comb"
            continue
        assert status == rt.RT_RAY_FIRST_STACK_OVERFLOW, f"{what}: k {k}: status {status}"
        for i in range(n):
            assert fg.is_sorted_subset(rows[i], walk.rows[i]), f"{what}: k {k}: ray {i}: not a sorted subset of the reference row"
        for i in (0, n - 1):
            run = isf.model(s.tlas, s.records, s.trees, rays[i], i, flt, k, limit=sc.STACK)
            assert run.overflow and run.row.tobytes() == rows[i].tobytes(), f"{what}: k {k}: ray {i}: {rows[i]} != the model's"
