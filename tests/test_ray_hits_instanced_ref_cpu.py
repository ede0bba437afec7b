"""CPU test of the two references of the instanced all-hit ray queries (tests/ray_hits_instanced_ref.py) on the scene the GPU
tests use, built here with the oracle's builders: three BLASes (range_sets.scene_tris "grid", "soup", "cornell") and 12
instances (rotations, a non-uniform scale, a mirror, two instances of one BLAS in the same place, one nested inside another's
box, a singular one, a bad-BLAS one, one of an empty tree).

1. the numpy walk agrees with the float64 brute force over the placed triangles on every stable pair, accepted and rejected,
   at the reference's MARGIN (the all-hit tests' 1e-4: nothing wider was needed); at most 1 % of the in-window (ray, instance,
   triangle) pairs are left out as unstable, and the never-entered instances contribute nothing;
2. an identity placement reproduces ray_hits_ref.walk: the same records, instance 0, the same leaf visits."""
import numpy as np
import pytest

import instance_ref as ir
import range_sets as rs
import ray_hits_instanced_ref as rhi
import ray_hits_instanced_scene as rsc
import ray_hits_ref as rh
import wide_trees as wt

BLAS_KINDS = ("bottom_up", "sah", "hybrid")      # of "grid", "soup", "cornell": no pairs, no splits -- one leaf per triangle


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(scenes, ora):
    s = Scene()
    s.blas_tris = [rs.scene_tris(name, scenes) for name in rsc.BLAS_SCENES]
    s.trees = [wt.ora_tree(ora, t, kind) for t, kind in zip(s.blas_tris, BLAS_KINDS)]
    s.trees.append((s.trees[0][0], s.trees[0][1], 0, 0))                 # table entry 3: an empty tree
    assert len(s.trees) == rsc.NUM_BLAS
    s.inst = rsc.scene_instances(s.blas_tris)
    s.prox, s.rec = rsc.host_scene(s.inst, s.trees)
    assert s.rec["flags"].tolist() == [0] * 9 + [ir.SINGULAR, ir.BAD_BLAS, ir.BAD_BLAS]
    s.tlas = wt.ora_tree(ora, s.prox, "bottom_up")
    s.world, s.inst_of, s.prim_of = ir.world_triangles(s.blas_tris, s.inst[:9])
    s.rays = rsc.scene_rays(s.world)
    s.rows, s.box_tests, s.leaf_visits = rhi.walk(s.tlas[1], s.tlas[0], s.tlas[2], s.tlas[3], s.rec, s.trees, s.rays)
    s.got, s.twice = rhi.got_matrix(s.rows, s.inst_of, s.prim_of, len(s.rays))
    return s


def test_scene_is_what_the_issue_asks_for(scene):
    s = scene
    assert s.inst.size == 12 and 1900 <= len(s.rays) <= 2100
    M = s.inst["object_to_world"].astype(np.float64)
    dets = [np.linalg.det(m[:, :3]) for m in M]
    assert dets[4] < 0 and dets[9] == 0 and all(d > 0 for k, d in enumerate(dets) if k not in (4, 9))
    assert (s.inst["object_to_world"][5] == s.inst["object_to_world"][6]).all() and s.inst["blas"][5] == s.inst["blas"][6]
    # instance 7's proxy box lies inside instance 2's
    assert (s.prox[7, :3] >= s.prox[2, :3]).all() and (s.prox[7, 3:6] <= s.prox[2, 3:6]).all()
    assert int(s.inst["blas"][10]) >= rsc.NUM_BLAS and int(s.inst["blas"][11]) == rsc.EMPTY_BLAS
    # every enterable instance is crossed by some ray; the others by none
    seen = np.unique(np.concatenate(s.rows)["instance"])
    assert seen.tolist() == list(range(9))
    lens = np.array([len(r) for r in s.rows])
    assert lens.max() >= 4 and (lens > 0).mean() > 0.25 and s.leaf_visits > 0 and s.box_tests > 0
    # the twins report the same records under both ids
    for row in s.rows:
        a, b = row[row["instance"] == 5], row[row["instance"] == 6]
        assert rh.canon([a[["t", "primitive_id", "u", "v"]].astype(rh.HIT)])[0].tolist() == \
            rh.canon([b[["t", "primitive_id", "u", "v"]].astype(rh.HIT)])[0].tolist()


def test_walk_agrees_with_float64_on_stable_pairs(scene):
    s, margin = scene, rhi.MARGIN
    assert not s.twice, "no pairs, no splits: a placed triangle is in a row at most once"
    b = rhi.brute_f64(s.world, s.rays, margin)
    missing = b["stable"] & b["accepted"] & ~s.got
    extra = b["stable"] & ~b["accepted"] & s.got
    share = float((b["in_window"] & ~b["stable"]).sum()) / float(b["in_window"].sum())
    print(f"margin {margin:g}: {int(b['in_window'].sum())} in-window pairs, unstable share {100 * share:.4f} %, "
          f"stable accepted {int((b['stable'] & b['accepted']).sum())}, missing {int(missing.sum())}, extra {int(extra.sum())}")
    assert not missing.any(), f"{missing.sum()} stable accepted pairs are not in their row: {np.argwhere(missing)[:4]}"
    assert not extra.any(), f"{extra.sum()} stable rejected pairs are in a row: {np.argwhere(extra)[:4]}"
    assert (b["stable"] & b["accepted"]).sum() > len(s.rays) // 2
    assert share <= 0.01, f"{100 * share:.3f} % of the in-window pairs are unstable at margin {margin}"


def test_margin_is_the_all_hit_tests_own():
    assert rhi.MARGIN == rh.MARGIN == 1e-4


@pytest.mark.parametrize("which", (0, 1, 2))
def test_identity_placement_reproduces_the_all_hit_walk(scene, ora, which):
    s = scene
    leaves, nodes, root, count = s.trees[which]
    inst = ir.instance_array([np.eye(3, 4)], [which])
    prox, rec = rsc.host_scene(inst, s.trees)
    assert (rec["world_to_object"][0] == np.eye(3, 4, dtype=np.float32)).all() and rec["flags"][0] == 0
    rays = rh.ray_sets(s.blas_tris[which], 11 + which, per_kind=96).astype(rh.RAY)
    for f in ("origin", "dir"):
        rays[f] = rays[f] + np.float32(0)            # no -0 component: the identity then reproduces every bit
    ref_rows, _, ref_leaf = rh.walk(nodes, leaves, root, count, rays)
    for kind in ("bottom_up", "sah"):
        tl = wt.ora_tree(ora, prox, kind)
        rows, box_tests, leaf_visits = rhi.walk(tl[1], tl[0], tl[2], tl[3], rec, s.trees, rays)
        assert all((r["instance"] == 0).all() for r in rows)
        rhi.assert_rows_equal(rows, [rhi.items(0, r) for r in ref_rows], f"identity over BLAS {which}, TLAS {kind}")
        assert leaf_visits == ref_leaf and box_tests > 0
    assert sum(len(r) for r in ref_rows) > len(rays) // 4
