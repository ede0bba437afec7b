"""CPU tests of the instance-filter reference (tests/instance_filter_ref.py), the yardstick of
tests/test_gpu_instance_filter.py, on the 7-instance composition of test_gpu_instances._composition (a rotation, a non-uniform
scale, a mirror, a shear, a translation, a copy overlapping the first, and a second BLAS of another kind), rebuilt from the
oracle's trees:
1. det_f32 and the effective per-instance filter are the values known by construction;
2. the two halves of the reference agree: composing ray_filter_ref.walk_gated_det + keep per instance on
   instance_ref.object_rays (the float32 restatement of the kernel's rule: object-space determinant, cull bits swapped by the
   sign of det_f32), the per-ray minimum agrees in instance and primitive with the float64 brute force over the kept WORLD
   triangles (world-space facing, the mirror handled by the geometry) on every unique ray, for every filter arm -- and the
   unique share of every arm, a condition on the inputs the GPU test rests on, is at least 0.95.  Measured (seed 11, 2 x 1500
   rays; the skip arm on its bounce batch of 714 rays): keep-all 0.9997, cull_back 0.9997, cull_front 1.0000, cull_disable
   0.9997, flip_facing 0.9997, masks 1.0000, skip 0.9986; 336 bounce rays have the triangle they start on as their unfiltered
   nearest record, and 85 unique ones report the skipped primitive id in the OTHER overlapping copy of the same BLAS;
   on the bounce batch t agrees within 1e-5 * max(1, t) on the 176 of 308 unique hits whose float32 start point resolves that
   bound (instance_filter_ref.t_resolved; worst 0.28 of the bound there, 1.77 over all 308);
3. the mirrored instance loses the opposite half of its records to CULL_BACK from the half it would lose without the mirror."""
import numpy as np
import pytest

import instance_filter_ref as fr
import instance_ref as ir
import ray_filter_ref as rx
from test_gpu_ray_queries import _ora_tree

F = np.float32


class Scene:
    def __init__(self, scenes, ora):
        self.blas_tris = [scenes.grid_mesh(24, 5), scenes.grid_mesh(16, 9)]
        self.trees = [_ora_tree(ora, self.blas_tris[0], "bottom_up"), _ora_tree(ora, self.blas_tris[1], "sah_pairs")]
        self.inst = fr.composition_instances(self.blas_tris[0])
        boxes = [ir.root_box(nodes, root, count) for _, nodes, root, count in self.trees]
        _, inv, flags = ir.prepare(self.inst, boxes)
        assert (flags == 0).all()
        self.W = inv.astype(F)                                    # the record's float32 world_to_object
        self.wt, self.inst_of, self.prim_of = ir.world_triangles(self.blas_tris, self.inst)
        self.rays = fr.world_rays(self.wt, fr.RAYS, fr.SEED)
        self.walks = fr.walk_instances(self.trees, self.inst, self.W, self.rays)
        self.cand = fr.candidates(self.rays, self.wt)


@pytest.fixture(scope="module")
def scene(scenes, ora):
    return Scene(scenes, ora)


# ------------------------------------------------------------------ 1: known values
def test_det_and_effective_filter_known_values():
    eye = np.eye(3, 4, dtype=F)
    mirror = np.diag([-1.0, 1.0, 1.0]).astype(F) @ eye
    assert fr.det_f32(eye) == F(1) and fr.det_f32(mirror) == F(-1)
    assert fr.det_f32(np.array([[2, 0, 0, 9], [0, 3, 0, 9], [0, 0, 4, 9]], F)) == F(24)
    assert fr.det_f32(np.array([[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], F)) == F(-1)        # a swap of two axes mirrors
    # the operation order: c0, c1, c2 are rounded products of rounded differences, summed ((c0 - c1) + c2)
    w = np.array([[1.1, 2.3, -0.7, 0], [0.9, -1.9, 3.3, 0], [-2.1, 0.4, 1.7, 0]], F)
    c0 = F(w[0, 0] * F(F(w[1, 1] * w[2, 2]) - F(w[1, 2] * w[2, 1])))
    c1 = F(w[0, 1] * F(F(w[1, 0] * w[2, 2]) - F(w[1, 2] * w[2, 0])))
    c2 = F(w[0, 2] * F(F(w[1, 0] * w[2, 1]) - F(w[1, 1] * w[2, 0])))
    assert fr.det_f32(w) == F(F(c0 - c1) + c2)
    assert abs(float(fr.det_f32(w)) - np.linalg.det(w[:, :3].astype(np.float64))) < 1e-5
    nan = eye.copy()
    nan[1, 1] = np.nan
    B, Fr = fr.CULL_BACK, fr.CULL_FRONT
    # (flags, instance flags, W) -> effective cull bits
    for flags, ifl, W, want in ((B, 0, eye, B), (B, 0, mirror, Fr), (Fr, 0, mirror, B), (B | Fr, 0, mirror, B | Fr),
                                (B, fr.FLIP_FACING, eye, Fr), (B, fr.FLIP_FACING, mirror, B), (B, fr.CULL_DISABLE, eye, 0),
                                (B | Fr, fr.CULL_DISABLE | fr.FLIP_FACING, mirror, 0), (B, 0, nan, B), (0, fr.FLIP_FACING, mirror, 0),
                                (B, 0x80, mirror, Fr)):
        flt = fr.InstanceFilter(flags, fr.ALL, fr.instance_filters(3, flags=[0, ifl, 0]))
        eff, entered = fr.effective(flt, 1, W, 4)
        assert eff.flags == want and entered.all() and eff.per_ray is None, (flags, ifl, want)
        assert fr.effective(flt, 0, W, 4)[0].flags == fr.effective(fr.InstanceFilter(flags), 1, W, 4)[0].flags
    # the instance rule: per-ray masks against instance masks; instances beyond the array are all ones
    per_ray = np.zeros(4, fr.INSTANCE_RAY_FILTER)
    per_ray["mask"], per_ray["skip_instance"], per_ray["skip_id"] = [1, 2, 3, 0], [1, 0, fr.MISS, 1], [7, 7, 7, fr.MISS]
    flt = fr.InstanceFilter(0, 0, fr.instance_filters(2, masks=[1, 2]), per_ray)
    assert fr.effective(flt, 0, eye, 4)[1].tolist() == [True, False, True, False]
    assert fr.effective(flt, 1, eye, 4)[1].tolist() == [False, True, True, False]
    assert fr.effective(flt, 2, eye, 4)[1].tolist() == [True, True, True, False]
    assert fr.effective(fr.InstanceFilter(0, 2, fr.instance_filters(2, masks=[1, 2])), 0, eye, 4)[1].tolist() == [False] * 4
    # the skip id acts only inside skip_instance
    assert fr.effective(flt, 1, eye, 4)[0].per_ray["skip_id"].tolist() == [7, fr.MISS, fr.MISS, fr.MISS]
    assert fr.effective(flt, 0, eye, 4)[0].per_ray["skip_id"].tolist() == [fr.MISS, 7, fr.MISS, fr.MISS]
    assert (fr.effective(flt, 1, eye, 4)[0].per_ray["mask"] == fr.ALL).all()


def test_the_composition_is_the_gpu_tests_composition(scene):
    inst = scene.inst
    assert inst.size == 7 and inst["blas"].tolist() == [0, 0, 0, 0, 0, 0, 1]
    dets = [float(fr.det_f32(w)) for w in scene.W]
    assert [d < 0 for d in dets] == [k == fr.MIRROR for k in range(7)], "exactly the mirror has a negative determinant"
    assert (inst["object_to_world"][fr.OVERLAP[0]][:, :3] == inst["object_to_world"][fr.OVERLAP[1]][:, :3]).all()


# ------------------------------------------------------------------ 2: the two halves agree; the unique shares
def _agree(scene, rays, walks, cand, flt, what):
    n = len(rays)
    best, best_id = fr.compose(walks, scene.W, flt, n)
    ref, unique = fr.brute_force(cand, scene.inst_of, scene.prim_of, rays, flt)
    share = unique.mean()
    print(f"{what}: unique share {share:.4f}, hits {ref['hit'].mean():.2f}")
    assert share >= 0.95, f"{what}: unique share {share:.3f}"
    got = best_id != fr.MISS
    bad = unique & (got != ref["hit"])
    assert not bad.any(), f"{what}: hit / miss differs on {bad.sum()} unique rays (first {np.nonzero(bad)[0][:5]})"
    m = unique & ref["hit"]
    assert (best_id[m] == scene.inst_of[ref["tri"][m]]).all(), f"{what}: instance"
    assert (best["primitive_id"][m] == scene.prim_of[ref["tri"][m]]).all(), f"{what}: primitive"
    assert m.sum() > 200
    return best, best_id, ref, unique


@pytest.mark.parametrize("arm", ("keep_all",) + fr.ARMS)
def test_composition_agrees_with_float64(scene, arm):
    n = len(scene.rays)
    flt = fr.InstanceFilter() if arm == "keep_all" else fr.make_arm(arm, scene.inst.size, n)
    best, best_id, ref, unique = _agree(scene, scene.rays, scene.walks, scene.cand, flt, arm)
    base, base_id = fr.compose(scene.walks, scene.W, fr.InstanceFilter(), n)
    if arm == "keep_all":
        return
    assert (best_id != base_id).sum() > 20, f"{arm}: the filter changes too few answers to mean anything"
    if arm == "flip_facing":                    # FLIP_FACING on the mirror: equal to culling on the object-space side
        for k in range(scene.inst.size):
            assert fr.effective(flt, k, scene.W[k], n)[0].flags == fr.CULL_BACK
    if arm == "cull_disable":
        cb = fr.compose(scene.walks, scene.W, fr.make_arm("cull_back", scene.inst.size, n), n)[1]
        assert (best_id != cb).sum() > 5, "CULL_DISABLE must bring back hits that cull_back loses"
    if arm == "masks":
        group = np.uint32(1) << (best_id[best_id != fr.MISS] % fr.GROUPS)
        assert ((group & flt.per_ray["mask"][best_id != fr.MISS]) != 0).all()


def test_skip_on_the_bounce_batch(scene):
    n = len(scene.rays)
    first, first_inst = fr.compose(scene.walks, scene.W, fr.InstanceFilter(), n)
    rays, per_ray = fr.bounce_batch(scene.rays, first, first_inst, scene.wt, scene.inst_of, scene.prim_of, fr.BOUNCE_SEED)
    assert 300 < len(rays) <= 3000
    walks = fr.walk_instances(scene.trees, scene.inst, scene.W, rays)
    cand = fr.candidates(rays, scene.wt)
    flt = fr.InstanceFilter(0, 0, None, per_ray)
    best, best_id, ref, unique = _agree(scene, rays, walks, cand, flt, "skip")
    # t: on the hits whose float32 start point resolves test_gpu_instances._check_world's bound the two halves agree within it
    bound = 1e-5 * np.maximum(1, ref["t"])
    ok = unique & ref["hit"] & fr.t_resolved(cand, ref, rays, bound)
    err = np.abs(best["t"] - ref["t"])
    allhits = unique & ref["hit"]
    print(f"skip: t is checked on {ok.sum()} of {allhits.sum()} unique hits; worst error / bound there "
          f"{(err[ok] / bound[ok]).max():.3f}, on all unique hits {(err[allhits] / bound[allhits]).max():.3f}")
    assert ok.sum() > 100 and (err[ok] <= bound[ok]).all()
    # the unfiltered nearest record of a bounce ray is often the triangle it starts on: the batch tests what it is for
    base, base_id = fr.compose(walks, scene.W, fr.InstanceFilter(), len(rays))
    own = (base_id == per_ray["skip_instance"]) & (base["primitive_id"] == per_ray["skip_id"])
    assert own.sum() > 50
    assert not ((best_id == per_ray["skip_instance"]) & (best["primitive_id"] == per_ray["skip_id"])).any()
    # the skipped primitive id, met in the other overlapping copy of the same BLAS, is reported there
    other = unique & (best["primitive_id"] == per_ray["skip_id"]) & (best_id != per_ray["skip_instance"]) & (best_id != fr.MISS)
    print(f"skip: {own.sum()} rays start on their unfiltered nearest record; {other.sum()} unique rays report the skipped id in "
          f"the other copy")
    assert other.sum() >= 10
    assert set(best_id[other].tolist()) <= set(fr.OVERLAP)


# ------------------------------------------------------------------ 3: the mirror loses the other half
def test_mirror_loses_the_opposite_half(scene):
    n = len(scene.rays)
    k = fr.MIRROR
    rows, dets = scene.walks[k]
    eff = fr.effective(fr.InstanceFilter(fr.CULL_BACK), k, scene.W[k], n)[0]
    assert eff.flags == fr.CULL_FRONT, "the mirror swaps the cull bits"
    plain = rx.Filter(fr.CULL_BACK)                                # what the instance would lose without the mirror
    total = lost_mirror = lost_plain = 0
    for i in range(n):
        if not len(rows[i]):
            continue
        with np.errstate(invalid="ignore"):
            sided = ~np.isnan(dets[i]) & (dets[i] != 0)
        km, kp = rx.keep(rows[i], dets[i], i, eff), rx.keep(rows[i], dets[i], i, plain)
        assert (km[sided] != kp[sided]).all(), "a sided record is lost to exactly one of the two"
        total += int(sided.sum()); lost_mirror += int((~km[sided]).sum()); lost_plain += int((~kp[sided]).sum())
    assert lost_mirror + lost_plain == total and lost_mirror > 10 and lost_plain > 10
    # and the float64 world-space facing says the same about the mirrored copy: the records CULL_BACK loses there are the
    # ones whose WORLD determinant is negative, i.e. whose object determinant is positive
    sel = scene.inst_of[scene.cand["tri"]] == k
    kept, _ = fr.kept_masks(scene.cand, scene.inst_of, scene.prim_of, fr.InstanceFilter(fr.CULL_BACK), n)
    assert (kept[sel] == (scene.cand["face"][sel] >= 0)).all() and 0 < kept[sel].sum() < sel.sum()
