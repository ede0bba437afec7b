"""CPU tests of the hit-filter reference (tests/ray_filter_ref.py), the yardstick of tests/test_gpu_ray_filter.py:
1. on test_ray_first_ref_cpu.py's hand-made tree the determinants and the kept rows are the values known by construction;
   walk_gated_det's rows, gates and counts are ray_first_ref.walk_gated's;
2. the partition laws on oracle-built trees: cull-back and cull-front rows are disjoint and their union is W without the
   NaN-determinant records; the rows of a per-ray mask m and of ~m partition W; the skip row is W without that id;
3. the condition the GPU test rests on: on the oracle-built trees of the four scenes, with the ray sets and the five filters
   used there, at most ray_first_ref.CAP of the rays with a non-empty W_f are undecided on W_f, for every k the GPU test uses;
4. the self-hit batch: on a non-zero number of the bounce rays the unfiltered nearest record is the triangle the ray starts on."""
import numpy as np
import pytest

import range_sets as rs
import ray_filter_ref as rx
import ray_first_ref as rf
import ray_hits_ref as rh
from test_gpu_ray_queries import _ora_tree
from test_ray_first_ref_cpu import ORACLE_TREES, hand_rays, hand_tree

F = np.float32


def _ids(rows):
    return [sorted(int(x) for x in r["primitive_id"]) for r in rows]


# ------------------------------------------------------------------ 1: known values
def test_kept_rows_on_the_hand_made_tree(rt):
    nodes, leaves = hand_tree(rt)
    rays = hand_rays()
    rows, gates, dets, bt, lv = rx.walk_gated_det(nodes, leaves, 0, 1, rays)
    ref_rows, ref_gates, rbt, rlv = rf.walk_gated(nodes, leaves, 0, 1, rays)
    assert (bt, lv) == (rbt, rlv)
    for a, b, ga, gb in zip(rows, ref_rows, gates, ref_gates):
        assert a.tobytes() == b.tobytes() and ga.tobytes() == gb.tobytes(), "walk_gated_det's rows and gates are walk_gated's"
    assert _ids(rows) == [[7, 10], [11], [7], [10], [], [], [], [7, 10]]
    # every triangle of the tree is counter-clockwise seen from +z (normal (0, 0, 1)) and every ray has dir.z = 1:
    # a = -dir . n = -1 exactly (unit legs, B = (v2, v1, v3) = ((0,1,2), (1,0,2), (1,1,2)) included): all back faces
    assert all((d == F(-1.0)).all() for d in dets)
    assert _ids(rx.filtered(rows, gates, dets, rx.Filter(rx.CULL_BACK))[0]) == [[]] * 8
    assert _ids(rx.filtered(rows, gates, dets, rx.Filter(rx.CULL_FRONT))[0]) == _ids(rows)
    assert _ids(rx.filtered(rows, gates, dets, rx.Filter())[0]) == _ids(rows)
    # the same rays from the other side (origin.z = 3, dir.z = -1) meet the fronts: a = +1
    back = rays.copy()
    back["origin"][:, 2], back["dir"][:, 2] = 3.0, -1.0
    back["origin"][:, :2] += 3 * back["dir"][:, :2]
    back["dir"][:, :2] *= -1                                   # the same line, walked backwards
    brows, bgates, bdets, _, _ = rx.walk_gated_det(nodes, leaves, 0, 1, back)
    assert sum(len(r) for r in brows) > 0 and all((d == F(1.0)).all() for d in bdets)
    assert _ids(rx.filtered(brows, bgates, bdets, rx.Filter(rx.CULL_FRONT))[0]) == [[]] * 8
    assert _ids(rx.filtered(brows, bgates, bdets, rx.Filter(rx.CULL_BACK))[0]) == _ids(brows)
    # skip ids: per ray, MISS skips nothing, without per_ray nothing is skipped
    per_ray = np.zeros(8, rx.RAY_FILTER)
    per_ray["mask"], per_ray["skip_id"] = rx.ALL, [7, 11, rx.MISS, 10, 7, 7, 7, 10]
    kept, kgates = rx.filtered(rows, gates, dets, rx.Filter(0, 0, None, per_ray))
    assert _ids(kept) == [[10], [], [7], [], [], [], [], [7]]
    assert [g.tolist() for g in kgates] == [[2.0], [], [1.0], [], [], [], [], [1.0]], "a kept record keeps its gate"
    # masks: ids 7 and 10 have masks of their own, 11 lies beyond the array and is all ones
    pm = np.zeros(11, np.uint32)
    pm[7], pm[10] = 1, 2
    assert _ids(rx.filtered(rows, gates, dets, rx.Filter(0, 1, pm))[0]) == [[7], [11], [7], [], [], [], [], [7]]
    assert _ids(rx.filtered(rows, gates, dets, rx.Filter(0, 2, pm))[0]) == [[10], [11], [], [10], [], [], [], [10]]
    assert _ids(rx.filtered(rows, gates, dets, rx.Filter(0, 0, pm))[0]) == [[]] * 8, "mask 0 keeps nothing"
    assert _ids(rx.filtered(rows, gates, dets, rx.Filter(0, 4, pm))[0]) == [[], [11], [], [], [], [], [], []]
    per_ray["mask"], per_ray["skip_id"] = [1, 4, 2, 3, 3, 3, 3, 2], rx.MISS
    assert _ids(rx.filtered(rows, gates, dets, rx.Filter(0, 0, pm, per_ray))[0]) == [[7], [11], [], [10], [], [], [], [10]]
    # a NaN determinant is neither front nor back: it survives both bits
    rec = np.zeros(3, rx.HIT)
    assert rx.keep(rec, np.array([1.0, -1.0, np.nan], F), 0, rx.Filter(rx.CULL_BACK | rx.CULL_FRONT)).tolist() == [False, False, True]


# ------------------------------------------------------------------ 2: partition laws
@pytest.mark.parametrize("tree", ("pairs", "sah_pairs_splits"))
def test_partition_laws_on_an_oracle_built_tree(scenes, ora, tree):
    tris = scenes.soup(300, 5, size=0.5)
    leaves, nodes, root, count = _ora_tree(ora, tris, tree)
    rays = rf.ray_sets(tris, 77, per_kind=64)
    rows, gates, dets, _, _ = rx.walk_gated_det(nodes, leaves, root, count, rays)
    assert sum(len(r) for r in rows) > len(rays) and max(len(r) for r in rows) >= 4, "the ray set is not trivial"
    n = len(rays)
    back = rx.filtered(rows, gates, dets, rx.Filter(rx.CULL_BACK))[0]
    front = rx.filtered(rows, gates, dets, rx.Filter(rx.CULL_FRONT))[0]
    assert sum(len(r) for r in back) > 0 and sum(len(r) for r in front) > 0
    per_ray = np.zeros(n, rx.RAY_FILTER)
    per_ray["mask"] = np.random.default_rng(3).integers(1, 7, n)
    per_ray["skip_id"] = rx.MISS
    pm = rx.group_masks(len(tris))
    inv = per_ray.copy()
    inv["mask"] = ~per_ray["mask"]
    m_rows = rx.filtered(rows, gates, dets, rx.Filter(0, 0, pm, per_ray))[0]
    i_rows = rx.filtered(rows, gates, dets, rx.Filter(0, 0, pm, inv))[0]
    skip = per_ray.copy()
    skip["mask"], skip["skip_id"] = rx.ALL, rx.nearest_ids(rows)
    s_rows = rx.filtered(rows, gates, dets, rx.Filter(0, 0, None, skip))[0]
    for i in range(n):
        with np.errstate(invalid="ignore"):
            sided = rows[i][~np.isnan(dets[i])]
        assert (rh.canon([np.concatenate([back[i], front[i]])])[0] == rh.canon([sided])[0]).all()
        assert (rh.canon([np.concatenate([m_rows[i], i_rows[i]])])[0] == rh.canon([rows[i]])[0]).all()
        assert (rh.canon([s_rows[i]])[0] == rh.canon([rows[i][rows[i]["primitive_id"] != skip["skip_id"][i]]])[0]).all()
        assert len(s_rows[i]) < len(rows[i]) or len(rows[i]) == 0


# ------------------------------------------------------------------ 3: the cap, on W_f
@pytest.mark.parametrize("name", ("grid", "soup", "cornell", "fractal"))
def test_undecided_share_of_the_filtered_rows(scenes, ora, name):
    tris = rs.scene_tris(name, scenes)
    rays = rf.ray_sets(tris, rf.SEEDS[name])
    assert len(rays) == 2048
    for tree in ORACLE_TREES:
        leaves, nodes, root, count = _ora_tree(ora, tris, tree)
        rows, gates, dets, _, _ = rx.walk_gated_det(nodes, leaves, root, count, rays)
        for fname in rx.FILTERS:
            frows, fgates = rx.filtered(rows, gates, dets, rx.make_filter(fname, rows, len(tris)))
            dedup = rf.dedup_all(frows, fgates)
            for k in rx.KS:
                share = rf.undecided_share(rf.expected(frows, fgates, k, rays["tmax"], dedup=dedup), frows)
                print(f"{name}/{tree}/{fname}: k {k}: {100 * share:.3f} % of {sum(len(r) > 0 for r in frows)} rays undecided")
                assert share <= rf.CAP, f"{name}/{tree}/{fname}: k {k}: {100 * share:.2f} % undecided"


# ------------------------------------------------------------------ 4: the self-hit batch hits itself
BOUNCE_SEED = 23


@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs"))
def test_bounce_rays_meet_their_own_triangle(scenes, ora, tree):
    tris = rs.scene_tris("grid", scenes)
    rays = rf.ray_sets(tris, rf.SEEDS["grid"])
    leaves, nodes, root, count = _ora_tree(ora, tris, tree)
    rows, gates, _, _, _ = rx.walk_gated_det(nodes, leaves, root, count, rays)
    first = rf.padded(rf.expected(rows, gates, 1, rays["tmax"]), 1)[:, 0]
    bounce, per_ray = rx.bounce_rays(rays, first, BOUNCE_SEED)
    assert len(bounce) > len(rays) // 8
    brows, bgates, _, _, _ = rx.walk_gated_det(nodes, leaves, root, count, bounce)
    exp = rf.expected(brows, bgates, 1, bounce["tmax"])
    own = sum(1 for e, s in zip(exp, per_ray["skip_id"]) if e[1] and len(e[0]) and e[0]["primitive_id"][0] == s)
    print(f"grid/{tree}: {own} of {len(bounce)} bounce rays have their own triangle as the decided nearest record")
    assert own > 0
