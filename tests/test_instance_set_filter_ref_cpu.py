"""CPU tests of the references of the filtered instanced all-hit / first-K queries (tests/instance_set_filter_ref.py), the
yardstick of the GPU tests, on oracle-built trees, the 12 instances of tests/ray_hits_instanced_scene.py and the arms of
instance_filter_ref.make_arm plus "skip" on a bounce batch:

1. the filtered walk equals the float64 brute force over the kept world triangles on every stable pair, none missing and none
   extra, and at most 1 % of the in-window pairs of admitted instances are unstable (the shares are printed; the module
   docstring of the reference quotes them);
2. the sequential model equals the numpy head on decided rays in all four orders and satisfies claims 1 and 3 on every ray;
   a rejected nearest crossing never moves the model's bound;
3. keep-all, in both of its forms, equals the unfiltered references: rows, gates and counts."""
import numpy as np
import pytest

import instance_filter_ref as ifr
import instance_ref as ir
import instance_set_filter_ref as isf
import instance_set_filter_scene as fsc
import range_sets as rs
import ray_first_instanced_ref as rfi
import ray_hits_instanced_ref as rhi
import ray_hits_instanced_scene as rsc
import wide_trees as wt

F = np.float32
BLAS_KINDS = ("bottom_up", "sah", "hybrid")
ORDERS = ((False, False), (True, False), (False, True), (True, True))     # (reverse, recull); the first is the kernel's
MODEL_KS = (1, 2, 5)


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(scenes, ora):
    s = Scene()
    s.blas_tris = [rs.scene_tris(name, scenes) for name in rsc.BLAS_SCENES]
    s.trees = [wt.ora_tree(ora, t, kind) for t, kind in zip(s.blas_tris, BLAS_KINDS)]
    s.trees.append((s.trees[0][0], s.trees[0][1], 0, 0))                 # table entry 3: an empty tree
    s.inst = rsc.scene_instances(s.blas_tris)
    s.prox, s.rec = rsc.host_scene(s.inst, s.trees)
    s.tlas = wt.ora_tree(ora, s.prox, "bottom_up")
    s.world, s.inst_of, s.prim_of = ir.world_triangles(s.blas_tris, s.inst[:9])
    s.rays = rsc.scene_rays(s.world)
    s.args = (s.tlas[1], s.tlas[0], s.tlas[2], s.tlas[3], s.rec, s.trees)
    s.plain = rfi.walk_gated(*s.args, s.rays)
    s.bounce_rays, s.bounce_per_ray = fsc.bounce(s.rays, s.plain[0])
    s.brute = {"main": isf.Brute(s.world, s.inst_of, s.prim_of, s.rays),
               "bounce": isf.Brute(s.world, s.inst_of, s.prim_of, s.bounce_rays)}
    s.walks = {}
    return s


def arm_of(s, name):
    """-> (ray set name, rays, filter)"""
    n = len(s.rays)
    if name == "keep_all":
        return "main", s.rays, isf.keep_all()
    if name == "skip":
        return "bounce", s.bounce_rays, fsc.skip_filter(s.bounce_per_ray)
    return "main", s.rays, fsc.arm(name, s.inst.size, n)


def walk_of(s, name):
    if name not in s.walks:
        _, rays, flt = arm_of(s, name)
        s.walks[name] = isf.walk_gated(*s.args, rays, flt)
    return s.walks[name]


ALL_ARMS = ("keep_all",) + fsc.ARMS + ("skip",)


def test_the_arms_reject_something(scene):
    s = scene
    total = sum(len(r) for r in s.plain[0])
    assert len(s.bounce_rays) > 500 and total > len(s.rays) // 2
    for name in fsc.ARMS:
        kept = sum(len(r) for r in walk_of(s, name)[0])
        assert 0 < kept < total, f"{name}: {kept} of {total} items kept"
    rows = walk_of(s, "skip")[0]
    for i, row in enumerate(rows):
        pr = s.bounce_per_ray[i]
        assert not ((row["instance"] == pr["skip_instance"]) & (row["primitive_id"] == pr["skip_id"])).any()
    # the mask arm: a masked pair costs its TLAS slot and nothing else
    _, _, bt, lv = walk_of(s, "masks")
    assert bt < s.plain[2] and lv < s.plain[3]


@pytest.mark.parametrize("name", ALL_ARMS)
def test_walk_agrees_with_float64_on_stable_pairs(scene, name):
    s = scene
    which, rays, flt = arm_of(s, name)
    rows = walk_of(s, name)[0]
    got, twice = rhi.got_matrix(rows, s.inst_of, s.prim_of, len(rays))
    assert not twice
    b = s.brute[which].under(flt)
    missing = b["stable"] & b["expected"] & ~got
    extra = b["stable"] & ~b["expected"] & got
    share = float((b["in_window"] & ~b["stable"]).sum()) / float(b["in_window"].sum())
    print(f"{name}: {int(b['in_window'].sum())} in-window pairs of admitted instances, unstable share {100 * share:.4f} %, "
          f"stable expected {int((b['stable'] & b['expected']).sum())}, missing {int(missing.sum())}, extra {int(extra.sum())}")
    assert not missing.any(), f"{name}: {missing.sum()} stable kept pairs are not in their row: {np.argwhere(missing)[:4]}"
    assert not extra.any(), f"{name}: {extra.sum()} stable rejected pairs are in a row: {np.argwhere(extra)[:4]}"
    assert (b["stable"] & b["expected"]).sum() > len(rays) // 8
    assert share <= isf.CAP, f"{name}: {100 * share:.3f} % of the in-window pairs are unstable"


def test_margins_are_the_projects_own():
    assert isf.MARGIN == rhi.MARGIN == 1e-4 and isf.FACE_MARGIN == ifr.FACE_MARGIN == 1e-3 and isf.CAP == 0.01


@pytest.mark.parametrize("name", ("cull_back", "masks", "skip"))
def test_model_equals_the_head_in_all_four_orders(scene, name):
    s = scene
    _, rays, flt = arm_of(s, name)
    rows, gates, _, _ = walk_of(s, name)
    hit = [i for i in range(len(rays)) if len(rows[i]) > 0]
    picks = hit[::20] + [i for i in range(len(rays)) if len(rows[i]) == 0][:4]
    tlas = (s.tlas[0], s.tlas[1], s.tlas[2], s.tlas[3])
    decided = 0
    for k in MODEL_KS:
        exp = rfi.expected(rows, gates, k, rays["tmax"])
        for reverse, recull in ORDERS:
            for i in picks:
                run = isf.model(tlas, s.rec, s.trees, rays[i], i, flt, k, reverse=reverse, recull=recull)
                why = rfi.envelope_violation(run.row, rows[i], gates[i], k, rays["tmax"][i])
                assert why is None, f"{name}: k {k}, reverse {reverse}, recull {recull}, ray {i}: {why}"
                E, dec, _ = exp[i]
                if dec:
                    want = rfi.pad_items(k)
                    want[:len(E)] = E
                    assert run.row.tobytes() == want.tobytes(), \
                        f"{name}: k {k}, reverse {reverse}, recull {recull}, decided ray {i}: {run.row} is not E = {E}"
                    decided += 1
    assert decided >= len(MODEL_KS) * len(ORDERS) * len(picks) * 0.9


def test_model_bound_moves_only_on_kept_items(scene):
    """rays whose nearest crossing is skipped: at k = 1 every value the model's bound takes is the t of a kept item -- never
    the skipped one's, which is nearer than all of them"""
    s = scene
    per_ray = fsc.skip_nearest(s.plain[0])
    flt = fsc.skip_filter(per_ray)
    rows, gates, _, _ = isf.walk_gated(*s.args, s.rays, flt)
    tlas = (s.tlas[0], s.tlas[1], s.tlas[2], s.tlas[3])
    seen = 0
    for i in [i for i in range(len(s.rays)) if len(s.plain[0][i]) > 1][::6]:
        skipped = rfi.sorted_row(s.plain[0][i])[0]
        run = isf.model(tlas, s.rec, s.trees, s.rays[i], i, flt, 1)
        kept_t = set(rows[i]["t"].tolist())
        assert all(float(b) in kept_t for b in run.bounds), f"ray {i}: bounds {run.bounds}"
        if len(rows[i]) and skipped["t"] < rfi.sorted_row(rows[i])[0]["t"]:
            assert all(b > skipped["t"] for b in run.bounds)
            seen += 1
    assert seen > 10


def test_keep_all_equals_the_unfiltered_references(scene):
    s = scene
    ref_rows, ref_gates, bt, lv = s.plain
    hits_rows, hbt, hlv = rhi.walk(*s.args, s.rays)
    for flt in (isf.keep_all(), isf.keep_all(len(s.rays), s.inst.size), isf.keep_all(len(s.rays), 3)):
        rows, gates, b, l = isf.walk_gated(*s.args, s.rays, flt)
        rhi.assert_rows_equal(rows, ref_rows, "keep-all against the unfiltered walk")
        assert (b, l) == (bt, lv)
        for (ws, g), (rws, rg) in zip(rfi.dedup_all(rows, gates), rfi.dedup_all(ref_rows, ref_gates)):
            assert ws.tobytes() == rws.tobytes() and g.tobytes() == rg.tobytes()
        arows, ab, al = isf.walk(*s.args, s.rays, flt)
        rhi.assert_rows_equal(arows, hits_rows, "keep-all against the unfiltered all-hit walk")
        assert (ab, al) == (hbt, hlv)
    run = isf.model((s.tlas[0], s.tlas[1], s.tlas[2], s.tlas[3]), s.rec, s.trees, s.rays[3], 3, isf.keep_all(), 32)
    one = rfi.walk_gated(*s.args, s.rays[3:4])
    assert (run.box_tests, run.leaf_visits) == (one[2], one[3])
