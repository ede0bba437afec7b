"""GPU tests of the filtered instanced all-hit ray queries (rt_ray_hits_count_instanced_filtered /
rt_ray_hits_collect_instanced_filtered; rt_abi.h, instanced set-filter block) on the 12-instance scene of
tests/test_gpu_ray_hits_instanced.py: device-built LBVH and SAH BLASes (the scene's grid of 1,152, soup of 1,500 and Cornell
box of 34 triangles), the device's own records, about 2,000 rays.  Every output buffer carries sentinels behind it
(tests/instance_set_filter_gpu.py).  The reference is tests/instance_set_filter_ref.py on the DEVICE's own bytes.

1. count = collect = the reference walk for the arms of instance_filter_ref.make_arm, "skip" on a bounce batch and a half-masked
   scene: rows as sorted 20-byte items, offsets, counts, counters[0..1] exact;
2. contract (a): both keep-all forms and filter = NULL give the unfiltered sibling's offsets, counts, counters and status byte
   for byte and the same items;
3. contract (b): row i = the union over the admitted instances of rt_ray_hits_collect_filtered on that BLAS with the numpy object
   ray under instance_filter_ref.effective, tagged with the instance -- GPU against GPU;
4. contract (c): rt_intersect_rays_instanced_filtered's closest hit is in the row; a miss there is an empty row;
5. contract (d): masks that admit no instance: empty rows, no leaf visit, exactly the TLAS slots examined;
6. contract (e): one identity instance equals rt_ray_hits_collect_filtered on the BLAS with {mask, skip_id};
7. fixed K = 2 under a filter: exact counts, RT_RAY_HITS_TRUNCATED, nothing past a segment;
8. the twins 5 / 6: skipping (5, id) leaves (6, id) in the row at the same t;
9. the mirror, instance 4: CULL_BACK keeps what the float64 world-space facing calls front; CULL_DISABLE and FLIP_FACING on it;
10. per_instance shorter than num_instances; a null per_instance with num_instance_filters > 0;
11. the convenience call RayHitsInstancedFiltered, plain and sorted."""
import numpy as np
import pytest

import instance_filter_ref as ifr
import instance_ref as ir
import instance_set_filter_gpu as ig
import instance_set_filter_ref as isf
import instance_set_filter_scene as fsc
import ray_filter_ref as rx
import ray_hits_instanced_gpu as g
import ray_hits_instanced_ref as rhi
import ray_hits_ref as rh
import test_gpu_ray_filter as tgr
from test_gpu_instance_filter import _run as closest_filtered
from test_gpu_ray_hits_instanced import World

pytestmark = pytest.mark.gpu

F = np.float32
SENT = g.SENT
COMBOS = (("bottom_up", "bottom_up"), ("sah", "sah_pairs"), ("hybrid", "sah_splits"))     # (TLAS kind, BLAS kind)
WALK_ARMS = fsc.ARMS + ("skip", "half")


class Tree:
    """what test_gpu_ray_filter's calls take for a built tree"""

    def __init__(self, entry):
        self.triangles_out, self.nodes_out = entry[0], entry[1]


class FWorld(World):
    """test_gpu_ray_hits_instanced.World (the scene, its rays, the unfiltered device rows) plus, per (combo, arm), the ray set, the
    filter, the reference and the device result -- everything computed once"""

    def __init__(self, rt, scenes):
        super().__init__(rt, scenes)
        self._arm, self._walk, self._res = {}, {}, {}

    def arm(self, combo, name):
        """-> (rays, host filter)"""
        if (combo, name) not in self._arm:
            n, num = len(self.rays), self.inst.size
            if name == "skip":
                rays, per_ray = fsc.bounce(self.rays, self.rows(*combo)[0].rows)
                out = rays.astype(self.rt.RAY), fsc.skip_filter(per_ray)
            elif name == "half":
                out = self.rays, fsc.half_masked(num)
            elif name == "none":
                out = self.rays, fsc.none_admitted(num)
            else:
                out = self.rays, fsc.arm(name, num, n)
            self._arm[combo, name] = out
        return self._arm[combo, name]

    def walk(self, combo, name):
        if (combo, name) not in self._walk:
            rays, flt = self.arm(combo, name)
            self._walk[combo, name] = ig.Walk(self.scene(*combo), rays, flt)
        return self._walk[combo, name]

    def result(self, combo, name):
        if (combo, name) not in self._res:
            rays, flt = self.arm(combo, name)
            self._res[combo, name] = ig.hits(self.rt, self.scene(*combo).args, rays, ig.dev_filter(self.rt, flt))
        return self._res[combo, name]


@pytest.fixture(scope="module")
def world(rt, scenes):
    return FWorld(rt, scenes)


# ------------------------------------------------------------------ 1: rows against the walk
@pytest.mark.parametrize("name", WALK_ARMS)
@pytest.mark.parametrize("combo", COMBOS)
def test_rows_equal_the_walk(world, combo, name):
    r, walk = world.result(combo, name), world.walk(combo, name)
    plain, _ = world.rows(*combo)
    what = f"TLAS {combo[0]} / BLAS {combo[1]} / {name}"
    ig.check_hits(r, walk, what)
    assert (r.counts == [len(x) for x in walk.rows]).all()
    assert 0 < r.offsets[-1], f"{what}: nothing kept"
    if name != "skip":
        assert r.offsets[-1] < plain.offsets[-1], f"{what}: nothing rejected"
        assert r.ctr_count[0] <= plain.ctr_count[0] and r.ctr_count[1] <= plain.ctr_count[1]
    if name in ("masks", "half"):
        assert r.ctr_count[0] < plain.ctr_count[0] and r.ctr_count[1] < plain.ctr_count[1], "a masked instance saves its descent"
    print(f"{what}: {int(r.offsets[-1])} records, box tests {int(r.ctr_count[0])}, leaf visits {int(r.ctr_count[1])}")


# ------------------------------------------------------------------ 2: (a) keep-all
@pytest.mark.parametrize("combo", COMBOS)
def test_keep_all_is_the_unfiltered_call(world, combo):
    rt = world.rt
    s = world.scene(*combo)
    plain, _ = world.rows(*combo)
    n = len(world.rays)
    for what, flt in (("null arrays", isf.keep_all()), ("all-ones arrays", isf.keep_all(n, world.inst.size)), ("NULL", None)):
        r = ig.hits(rt, s.args, world.rays, ig.dev_filter(rt, flt))
        assert r.offsets.tobytes() == plain.offsets.tobytes() and r.counts.tobytes() == plain.counts.tobytes(), what
        assert r.ctr_count.tobytes() == plain.ctr_count.tobytes() and r.st_count == plain.st_count == 0, what
        rhi.assert_rows_equal(r.rows, plain.rows, what)


# ------------------------------------------------------------------ 3: (b) composition, GPU against GPU
@pytest.mark.parametrize("name", ("cull_back", "cull_disable", "skip"))
@pytest.mark.parametrize("combo", COMBOS[:2])
def test_composition_of_per_blas_filtered_rows(world, combo, name):
    rt = world.rt
    s = world.scene(*combo)
    rays, flt = world.arm(combo, name)
    r = world.result(combo, name)
    n = len(rays)
    ray, inst, _ = s.entered(rays)
    ok = isf.rule1(flt, ray, inst, n)
    ray, inst = ray[ok], inst[ok]
    entries, _ = world.blas(combo[1])
    exp = [[] for _ in rays]
    for k in np.unique(inst):
        sel = ray[inst == k]
        W = s.records["world_to_object"][k]
        obj = ir.object_rays(rays[sel], W)
        eff, _ = ifr.effective(flt, int(k), W, n)
        one = rx.Filter(eff.flags, eff.ray_mask, None, None if eff.per_ray is None else eff.per_ray[sel])
        e = entries[int(s.records["blas"][k])]
        per = tgr._hits(rt, (Tree(e), e[2], e[3]), obj, one)      # rt_ray_hits_count_filtered + _collect_filtered on the BLAS
        for i, row in zip(sel, per.rows):
            exp[i].append(rhi.items(k, row))
    exp = [np.concatenate(x) if x else np.zeros(0, rhi.ITEM) for x in exp]
    rhi.assert_rows_equal(r.rows, exp, f"composition {combo} / {name}")
    assert sum(len(x) for x in exp) == int(r.offsets[-1]) > 0


# ------------------------------------------------------------------ 4: (c) the closest-hit relation
@pytest.mark.parametrize("name", ("cull_back", "masks", "skip"))
@pytest.mark.parametrize("combo", COMBOS)
def test_closest_hit_is_a_member(world, combo, name):
    rt = world.rt
    s = world.scene(*combo)
    rays, flt = world.arm(combo, name)
    r = world.result(combo, name)
    assert r.st_count == 0
    c, ids, _ = closest_filtered(s.keep[0], rays, flt)
    hit = c["primitive_id"] != rt.MISS
    assert ((ids != rt.MISS) == hit).all()
    assert (hit == (r.counts > 0)).all(), f"closest hit and the row disagree on {(hit != (r.counts > 0)).sum()} rays"
    assert hit.sum() > len(rays) // 8
    for k in np.nonzero(hit)[0]:
        row = r.rows[k]
        same = (row["instance"] == ids[k]) & (row["t"].view(np.uint32) == c["t"][k:k + 1].view(np.uint32)) & \
               (row["u"].view(np.uint32) == c["u"][k:k + 1].view(np.uint32)) & \
               (row["v"].view(np.uint32) == c["v"][k:k + 1].view(np.uint32))
        assert same.any(), f"ray {k}: the closest hit {c[k]} in instance {ids[k]} is not in the row {row}"
        assert row["t"].min() <= c["t"][k]


# ------------------------------------------------------------------ 5: (d) masks that admit no instance
@pytest.mark.parametrize("combo", COMBOS)
def test_no_instance_admitted(world, combo):
    s = world.scene(*combo)
    r = world.result(combo, "none")
    _, _, tlas_slots = s.entered(world.rays)
    assert (r.offsets == 0).all() and (r.counts == 0).all() and r.st_count == 0
    assert r.ctr_count[1] == 0 and r.ctr_count[0] == tlas_slots > 0, f"counters {r.ctr_count}, TLAS slots examined {tlas_slots}"
    # per-ray masks of zero do the same
    per_ray = np.zeros(len(world.rays), ifr.INSTANCE_RAY_FILTER)
    per_ray["skip_instance"], per_ray["skip_id"] = isf.MISS, isf.MISS
    z = ig.hits(world.rt, s.args, world.rays, ig.dev_filter(world.rt, ifr.InstanceFilter(0, ifr.ALL, None, per_ray)))
    assert (z.offsets == 0).all() and z.ctr_count[1] == 0 and z.ctr_count[0] == tlas_slots


# ------------------------------------------------------------------ 6: (e) one identity instance
@pytest.mark.parametrize("which,blas_kind", ((0, "bottom_up"), (1, "sah_pairs"), (2, "sah_splits")))
def test_identity_instance_equals_the_single_tree_filtered_call(world, which, blas_kind):
    rt = world.rt
    entries, _ = world.blas(blas_kind)
    e = entries[which]
    tree = (Tree(e), e[2], e[3])
    rays = rh.ray_sets(world.blas_tris[which], 11 + which, per_kind=160).astype(rt.RAY)
    for f in ("origin", "dir"):
        rays[f] = rays[f] + F(0)                         # no -0 component
    n = len(rays)
    plain = tgr._hits(rt, tree, rays, tgr.UNFILTERED)
    one = np.zeros(n, rx.RAY_FILTER)
    one["mask"] = 1 + (np.arange(n) % 3 == 0)            # 1 or 2
    one["skip_id"] = rx.nearest_ids(plain.rows)
    per_ray = np.zeros(n, ifr.INSTANCE_RAY_FILTER)
    per_ray["mask"], per_ray["skip_instance"], per_ray["skip_id"] = one["mask"], 0, one["skip_id"]
    exp = tgr._hits(rt, tree, rays, rx.Filter(rx.CULL_BACK, 0, None, one))
    assert 0 < exp.offsets[-1] < plain.offsets[-1]
    for tlas_kind in ("bottom_up", "sah"):
        s = world.make(tlas_kind, blas_kind, ir.instance_array([np.eye(3, 4)], [which]))
        r = ig.hits(rt, s.args, rays, ig.dev_filter(rt, ifr.InstanceFilter(ifr.CULL_BACK, 0, None, per_ray)))
        what = f"identity over BLAS {which} ({blas_kind}), TLAS {tlas_kind}"
        assert r.st_count == 0 and (r.offsets == exp.offsets).all(), what
        rhi.assert_rows_equal(r.rows, [rhi.items(0, row) for row in exp.rows], what)
        assert r.ctr_count[1] == exp.ctr_count[1], what


# ------------------------------------------------------------------ 7: fixed K
@pytest.mark.parametrize("combo", COMBOS[:2])
def test_fixed_k_under_a_filter(world, combo):
    import torch
    rt = world.rt
    K = 2
    s = world.scene(*combo)
    rays, flt = world.arm(combo, "cull_front")
    full = world.result(combo, "cull_front")
    n = len(rays)
    assert (full.counts > K).any() and (full.counts == K).any() and (full.counts < K).any()
    rd = g.dev_rays(rt, rays)
    hf = ig.dev_filter(rt, flt)
    off = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
    recs, cnt, ctr, st = ig.collect(rt, s.args, rd, hf, off, n * K)
    assert (cnt == full.counts).all(), "counts must be exact beyond the room"
    assert (ctr == full.ctr_count).all() and st == rt.RT_RAY_HITS_TRUNCATED
    seg = recs.reshape(n, K)
    for k in range(n):
        m = min(int(cnt[k]), K)
        assert (seg[k, :m]["instance"] != SENT).all() and rhi.is_subset(seg[k, :m], full.rows[k]), f"ray {k}: not of the exact row"
        assert (seg[k, m:]["instance"] == SENT).all() and (seg[k, m:]["primitive_id"] == SENT).all(), f"ray {k} wrote past its records"
    short = np.nonzero(full.counts <= K)[0]              # no row longer than K: no flag
    per = None if flt.per_ray is None else flt.per_ray[short]
    hf = ig.dev_filter(rt, ifr.InstanceFilter(flt.flags, flt.ray_mask, flt.per_instance, per))
    off = (torch.arange(len(short) + 1, dtype=torch.int64) * K).cuda()
    recs, cnt, _, st = ig.collect(rt, s.args, g.dev_rays(rt, rays[short]), hf, off, len(short) * K)
    assert st == 0 and (cnt == full.counts[short]).all()


# ------------------------------------------------------------------ 8: the twins
@pytest.mark.parametrize("combo", COMBOS)
def test_skipping_one_twin_leaves_the_other(world, combo):
    rt = world.rt
    a, b = fsc.TWINS
    s = world.scene(*combo)
    plain, _ = world.rows(*combo)
    per_ray = fsc.skip_nearest(plain.rows, only=a)
    flt = fsc.skip_filter(per_ray)
    r = ig.hits(rt, s.args, world.rays, ig.dev_filter(rt, flt))
    ig.check_hits(r, ig.Walk(s, world.rays, flt), f"{combo}: skip the nearest of instance {a}")
    seen = 0
    for i in np.nonzero(per_ray["skip_instance"] == a)[0]:
        pid = per_ray["skip_id"][i]
        was = plain.rows[i][(plain.rows[i]["instance"] == a) & (plain.rows[i]["primitive_id"] == pid)]
        row = r.rows[i]
        assert not ((row["instance"] == a) & (row["primitive_id"] == pid)).any(), f"ray {i}: ({a}, {pid}) was not skipped"
        twin = row[(row["instance"] == b) & (row["primitive_id"] == pid)]
        assert len(twin) == len(was) >= 1, f"ray {i}: ({b}, {pid}) is missing"
        assert sorted(twin["t"].view(np.uint32).tolist()) == sorted(was["t"].view(np.uint32).tolist()), f"ray {i}: another t"
        assert len(row) == len(plain.rows[i]) - len(was)
        seen += 1
    assert seen > 20


# ------------------------------------------------------------------ 9: the mirror
def _facing(world, rays, i, items):
    """float64 world-space facing (the signed cosine between the ray and the normal side) of ray i on its items' triangles"""
    if not hasattr(world, "_where"):
        world._where = {(int(a), int(b)): j for j, (a, b) in enumerate(zip(world.inst_of, world.prim_of))}
    where = world._where
    V = np.asarray(world.world, np.float64).reshape(-1, 3, 3)
    d = rays["dir"][i].astype(np.float64)
    out = []
    for it in items:
        T = V[where[int(it["instance"]), int(it["primitive_id"])]]
        e1, e2 = T[1] - T[0], T[2] - T[0]
        nrm = np.cross(e1, e2)
        out.append(float(np.dot(e1, np.cross(d, e2)) / (np.linalg.norm(d) * np.linalg.norm(nrm))))
    return np.array(out)


@pytest.mark.parametrize("combo", COMBOS[:2])               # (not the split BLASes: a placed triangle once per row)
def test_mirror_instance_is_culled_by_its_world_space_side(world, combo):
    rt = world.rt
    m = fsc.MIRROR
    s = world.scene(*combo)
    plain, _ = world.rows(*combo)
    assert ifr.det_f32(s.records["world_to_object"][m]) < 0
    num = world.inst.size
    flip = np.zeros(num, np.uint32)
    flip[m] = ifr.FLIP_FACING
    disable = np.zeros(num, np.uint32)
    disable[m] = ifr.CULL_DISABLE
    arms = {"cull_back": ifr.InstanceFilter(ifr.CULL_BACK),
            "flip": ifr.InstanceFilter(ifr.CULL_BACK, ifr.ALL, ifr.instance_filters(num, flags=flip)),
            "disable": ifr.InstanceFilter(ifr.CULL_BACK, ifr.ALL, ifr.instance_filters(num, flags=disable))}
    for name, flt in arms.items():
        r = ig.hits(rt, s.args, world.rays, ig.dev_filter(rt, flt))
        ig.check_hits(r, ig.Walk(s, world.rays, flt), f"{combo}: mirror / {name}")
        kept = dropped = 0
        for i in range(len(world.rays)):
            before = plain.rows[i][plain.rows[i]["instance"] == m]
            if not len(before):
                continue
            after = r.rows[i][r.rows[i]["instance"] == m]
            if name == "disable":
                rhi.assert_rows_equal([after], [before], f"ray {i}: CULL_DISABLE on the mirror")
                kept += len(after)
                continue
            sign = -1.0 if name == "flip" else 1.0
            gone = before[~np.isin(before["primitive_id"], after["primitive_id"])]
            assert (sign * _facing(world, world.rays, i, after) > -isf.FACE_MARGIN).all(), f"{name}: ray {i} kept a back face"
            assert (sign * _facing(world, world.rays, i, gone) < isf.FACE_MARGIN).all(), f"{name}: ray {i} dropped a front face"
            kept, dropped = kept + len(after), dropped + len(gone)
        assert kept > 20 and (dropped > 20 or name == "disable"), f"{name}: {kept} kept, {dropped} dropped"


# ------------------------------------------------------------------ 10: short and absent per_instance arrays
@pytest.mark.parametrize("combo", COMBOS[:2])
def test_short_and_absent_per_instance(world, combo):
    rt = world.rt
    s = world.scene(*combo)
    plain, _ = world.rows(*combo)
    short = ifr.InstanceFilter(ifr.CULL_BACK, 1, ifr.instance_filters(3, masks=[1, 2, 1], flags=[0, 0, ifr.CULL_DISABLE]))
    r = ig.hits(rt, s.args, world.rays, ig.dev_filter(rt, short))
    ig.check_hits(r, ig.Walk(s, world.rays, short), f"{combo}: per_instance of 3 records")
    seen = np.unique(np.concatenate(r.rows)["instance"]).tolist()
    assert 1 not in seen and {0, 2, 3, 8} <= set(seen), "instance 1 is masked; instances beyond the array have all-ones masks"

    class Lying(rt.InstanceHitFilter):                   # num_instance_filters > 0 with a null per_instance: an absent array
        def _struct(self, num_rays):
            st = super()._struct(num_rays)
            st.num_instance_filters = 77
            return st

    r = ig.hits(rt, s.args, world.rays, Lying())
    assert r.offsets.tobytes() == plain.offsets.tobytes() and r.ctr_count.tobytes() == plain.ctr_count.tobytes()
    rhi.assert_rows_equal(r.rows, plain.rows, "a null per_instance with num_instance_filters = 77")


# ------------------------------------------------------------------ 11: the convenience call
def test_ray_hits_instanced_filtered_convenience_sorted(world):
    import torch
    rt = world.rt
    combo = COMBOS[2]
    s = world.scene(*combo)
    rays, flt = world.arm(combo, "masks")
    want = world.result(combo, "masks")
    rd = g.dev_rays(rt, rays)
    hf = ig.dev_filter(rt, flt)
    off, hits, ids = rt.RayHitsInstancedFiltered(*s.args, rd, hf)
    assert off.dtype == torch.int64 and tuple(hits.shape) == (int(want.offsets[-1]), 4) and tuple(ids.shape) == (int(want.offsets[-1]),)
    got = rhi.items(ids.cpu().numpy().view(np.uint32), hits.cpu().numpy().view(rh.HIT).reshape(-1))
    assert (off.cpu().numpy() == want.offsets).all() and got.tobytes() == np.concatenate(want.rows).tobytes()
    off, hits, ids = rt.RayHitsInstancedFiltered(*s.args, rd, hf, sort=True)
    o = off.cpu().numpy()
    got = rhi.items(ids.cpu().numpy().view(np.uint32), hits.cpu().numpy().view(rh.HIT).reshape(-1))
    rows = [got[o[k]:o[k + 1]] for k in range(len(rays))]
    rhi.assert_rows_equal(rows, want.rows, "sorted")
    for k, row in enumerate(rows):
        key = list(zip(row["t"].tolist(), row["instance"].tolist(), row["primitive_id"].tolist()))
        assert key == sorted(key), f"ray {k}: not ascending in (t, instance, primitive_id): {key}"
    o2, h2, i2 = rt.RayHitsInstancedFiltered(*s.args, rd, None)
    plain, _ = world.rows(*combo)
    assert (o2.cpu().numpy() == plain.offsets).all()
