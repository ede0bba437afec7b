"""CPU tests of the all-hit references (tests/ray_hits_ref.py): the tree walk on a hand-made tree whose rows are known by
construction, and the condition the GPU test's float64 comparison rests on -- on the grid and soup scenes with the ray sets
used there, at most 1 % of the (ray, triangle) pairs whose t lies inside the window are unstable."""
import numpy as np
import pytest

import range_sets as rs
import ray_hits_ref as rh

F = np.float32
SEEDS = rh.SEEDS      # the GPU test uses the same sets


def hand_tree(rt):
    """slot 0: the root run (one BOX slot) -> the run [2, 5): a single-triangle leaf, a NONE slot, a pair leaf.
    leaf 0: triangle 7 in the plane z = 1, stored with rotation 1; leaf 1: the unit quad in z = 2 as the pair (10, 11),
    A = (v0, v1, v2), B = (v2, v1, v3), B stored with rotation 2"""
    nodes = np.zeros(5, rt.NODE)
    leaves = np.zeros(2, rt.TRIANGLE_PAIR)
    leaves["v0"][0], leaves["v1"][0], leaves["v2"][0] = (0, 0, 1), (1, 0, 1), (0, 1, 1)
    leaves["v3"][0] = leaves["v2"][0]
    leaves["primitive_id_0"][0], leaves["rotations"][0] = 7, (1, 0)
    leaves["v0"][1], leaves["v1"][1], leaves["v2"][1], leaves["v3"][1] = (0, 0, 2), (1, 0, 2), (0, 1, 2), (1, 1, 2)
    leaves["primitive_id_0"][1], leaves["primitive_id_1"][1], leaves["rotations"][1] = 10, 11, (0, 2)
    nodes["min"][0], nodes["max"][0] = (0, 0, 1), (1, 1, 2)
    nodes["w12"][0], nodes["w28"][0] = 3 << 29, (rt.CHILD_BOX << 29) | 2
    nodes["min"][2], nodes["max"][2] = (0, 0, 1), (1, 1, 1)
    nodes["w12"][2], nodes["w28"][2] = 1 << 29, (rt.CHILD_TRI << 29) | 0
    nodes["min"][3], nodes["max"][3] = (-9, -9, -9), (9, 9, 9)                   # NONE: never examined, whatever its box
    nodes["w12"][3], nodes["w28"][3] = 0, (rt.CHILD_NONE << 29) | 1
    nodes["min"][4], nodes["max"][4] = (0, 0, 2), (1, 1, 2)
    nodes["w12"][4], nodes["w28"][4] = 2 << 29, (rt.CHILD_TRI << 29) | 1
    return nodes, leaves


def hand_rays():
    r = np.zeros(7, rh.RAY)
    r["dir"] = (0.01, 0.02, 1.0)
    r["tmin"], r["tmax"] = 0.0, np.inf
    r["origin"][:] = (0.2, 0.2, 0.0)
    r["origin"][1] = (0.8, 0.8, 0.0)
    r["tmax"][2] = 1.5
    r["tmin"][3] = 1.5
    r["origin"][4] = (5.0, 5.0, 0.0)
    r["tmin"][5], r["tmax"][5] = 2.0, 1.0                     # dead: tmin > tmax
    r["dir"][6, 1] = np.nan                                   # dead: a NaN direction
    return r


def test_walk_on_a_hand_made_tree(rt):
    nodes, leaves = hand_tree(rt)
    rows, box_tests, leaf_visits = rh.walk(nodes, leaves, 0, 1, hand_rays())
    ids = [sorted(r["primitive_id"].tolist()) for r in rows]
    assert ids == [[7, 10], [11], [7], [10], [], [], []]
    # rays 0-3: the root slot and the two non-NONE slots of the run; ray 4 fails the root slot; dead rays count nothing
    assert box_tests == 4 * 3 + 1
    # ray 0 and 1 enter both leaves, ray 2 (tmax 1.5) only the z = 1 leaf, ray 3 (tmin 1.5) only the z = 2 leaf
    assert leaf_visits == 2 + 2 + 1 + 1
    r0 = {int(x["primitive_id"]): x for x in rows[0]}
    # triangle 7 at (0.21, 0.22, 1): stored weights (bu, bv) = (0.21, 0.22), rotation 1 -> (u, v) = (bv, 1 - bu - bv)
    assert abs(r0[7]["t"] - 1) < 1e-6 and abs(r0[7]["u"] - 0.22) < 1e-6 and abs(r0[7]["v"] - 0.57) < 1e-6
    # triangle 10 at (0.22, 0.24, 2): rotation 0 -> the stored weights
    assert abs(r0[10]["t"] - 2) < 1e-6 and abs(r0[10]["u"] - 0.22) < 1e-6 and abs(r0[10]["v"] - 0.24) < 1e-6
    # ray 1 meets B = ((0,1,2), (1,0,2), (1,1,2)) at (0.82, 0.84, 2): (bu, bv) = (0.16, 0.66), rotation 2 -> (1 - bu - bv, bu)
    b = rows[1][0]
    assert abs(b["t"] - 2) < 1e-6 and abs(b["u"] - 0.18) < 1e-6 and abs(b["v"] - 0.16) < 1e-6
    assert (rh.offsets(rows) == [0, 2, 3, 4, 5, 5, 5, 5]).all()
    # an empty tree: every row empty, nothing counted
    rows, bt, lv = rh.walk(nodes, leaves, 0, 0, hand_rays())
    assert all(len(r) == 0 for r in rows) and bt == 0 and lv == 0


def test_walk_agrees_with_float64_on_the_hand_made_tree(rt):
    nodes, leaves = hand_tree(rt)
    tris = np.zeros((12, 3, 3), F)                            # the caller's triangles 7, 10, 11 (the others: far away)
    tris[:] = ((100, 100, 100), (101, 100, 100), (100, 101, 100))
    tris[7] = ((1, 0, 1), (0, 1, 1), (0, 0, 1))               # stored rotated by 1: (v2, v0, v1) of the caller's
    tris[10] = ((0, 0, 2), (1, 0, 2), (0, 1, 2))
    tris[11] = ((1, 1, 2), (0, 1, 2), (1, 0, 2))              # stored rotated by 2: (v1, v2, v0) of the caller's
    rays = hand_rays()
    rows, _, _ = rh.walk(nodes, leaves, 0, 1, rays)
    b = rh.brute_f64(tris.reshape(-1, 9), rays)
    assert b["stable"].all()
    for i, row in enumerate(rows):
        assert sorted(row["primitive_id"].tolist()) == np.nonzero(b["accepted"][i])[0].tolist()
        for rec in row:                                       # the caller-corner weights: o + t d = (1-u-v) v0 + u v1 + v v2
            T = tris[int(rec["primitive_id"])].astype(np.float64)
            p = rays["origin"][i].astype(np.float64) + float(rec["t"]) * rays["dir"][i].astype(np.float64)
            q = (1 - float(rec["u"]) - float(rec["v"])) * T[0] + float(rec["u"]) * T[1] + float(rec["v"]) * T[2]
            assert np.abs(p - q).max() < 1e-5


@pytest.mark.parametrize("name", ("grid", "soup"))
def test_stable_share_of_the_ray_sets(scenes, name):
    tris = rs.scene_tris(name, scenes)
    rays = rh.ray_sets(tris, SEEDS[name])
    assert len(rays) == 2048 and rh.live(rays).all()
    d = rays["dir"]
    assert (np.abs(d) > 1e-6 * np.abs(d).max(1)[:, None]).all(), "no axis-aligned ray"
    b = rh.brute_f64(tris, rays)
    inw = b["in_window"]
    share = (inw & ~b["stable"]).sum() / inw.sum()
    print(f"{name}: {inw.sum()} pairs with t inside the window, {100 * share:.3f} % unstable, "
          f"{b['accepted'].sum()} accepted, longest row {b['accepted'].sum(1).max()}")
    assert share <= 0.01
    assert b["accepted"].sum() >= len(rays) // 2 and b["accepted"].sum(1).max() >= 2      # the sets are not trivial
