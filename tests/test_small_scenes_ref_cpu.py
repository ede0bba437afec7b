"""CPU tests of the references on the small scenes (tests/small_scenes.py), before any kernel sees them: what
tests/test_gpu_small_scenes.py asserts of the device rests on the conditions checked here, on the oracle's trees.

1. the walks against float64: on every oracle tree of every scene ray_hits_ref.walk and ray_first_ref.walk_gated give the same
   rows, every stable accepted (ray, triangle) pair of ray_hits_ref.brute_f64 is in its row and no stable rejected pair is,
   and the nearest record of every row passes test_gpu_ray_queries._check_against_f64 against shade_ref.cast -- the assertion
   the GPU test makes of rt_intersect_rays, made here of the walk;
2. the caps, unchanged: at most 1 % of the (ray, triangle) pairs with t inside the window are unstable
   (test_ray_hits_ref_cpu.py), at most 1 % of the rays (_check_against_f64), at most ray_first_ref.CAP of the rays with a
   non-empty row undecided for k in 1, 2, 8 (test_gpu_ray_first.py).  Every share is printed;
3. points: point_ref.brute_force within 8 ulps of the largest coordinate of point_ref.brute_force_f64
   (test_point_ref_cpu.py's tolerance) on EVERY scene -- scaled_up included: its largest squared distance is about 1e11, far
   inside float32's range;
4. ties: knn_ref.brute_force_knn lists the 64 copies of `stack` and the 2 of `twins` by ascending id at one dist2;
   range_ref.sphere keeps all of them at the exact radius and none one float below it.

Scenes without a float64 arm (small_scenes.NO_F64_PAIRS / NO_F64_CAST), held to the bit-exact arms only:
  points       every Moller-Trumbore determinant is exactly 0: float64 calls every pair unstable, whatever the ray set;
  scaled_down  shade_ref.cast rejects |det| <= 1e-12, the kernel (as the reference tracer) |det| < 1e-9: with edges of 1e-4 and
               directions of 1e-3 every determinant is about 1e-11, so cast sees hits where the documented rule has none.
               ray_hits_ref.brute_f64 restates the kernel's epsilon, so the pairs arm holds there (every row is empty);
  flat's in-plane rays and scaled_down's long rays (small_scenes.exact_rays) are outside both arms for the reasons given there."""
import numpy as np
import pytest

import knn_ref as kr
import point_ref as pr
import range_ref as rr
import ray_first_ref as rf
import ray_hits_ref as rh
import sdf_ref
import small_scenes as ss
import test_gpu_ray_queries as rq

F = np.float32
ORACLE_TREES = tuple(t for t in rq.TREES if t != "hybrid_pairs")       # (hybrid + pairs has no oracle builder)
PAIR_CAP = 0.01           # test_ray_hits_ref_cpu.py
RAY_CAP = 0.01            # test_gpu_ray_queries._check_against_f64's default bound
POINT_ULPS = 8            # test_point_ref_cpu.py


def nearest_records(rows):
    """the closest-hit record of every all-hit row: smallest t, then smallest id; a miss is (inf, MISS, 0, 0)"""
    out = rf.miss_records(len(rows))
    for i, row in enumerate(rows):
        if len(row):
            out[i] = row[rf.key_order(row)[0]]
    return out


@pytest.mark.parametrize("name", ss.OPEN)
def test_walks_against_float64(scenes, ora, name):
    tris = ss.tris(name, scenes)
    n = tris.shape[0]
    rays = ss.rays(name, tris)
    m = len(rays)
    every = ss.all_rays(name, tris)
    pairs_arm, cast_arm = name not in ss.NO_F64_PAIRS, name not in ss.NO_F64_CAST
    b = rh.brute_f64(tris, rays)
    inw = b["in_window"]
    share = float((inw & ~b["stable"]).sum()) / max(int(inw.sum()), 1)
    ref = rq._f64(tris, rays)
    print(f"{name}: {n} triangles, {m} rays (+{len(every) - m} exact-only): {100 * share:.3f} % of {int(inw.sum())} pairs unstable"
          f"{'' if pairs_arm else ' (no pairs arm)'}, {100 * (1 - ref['stable'].mean()):.3f} % of the rays unstable"
          f"{'' if cast_arm else ' (no cast arm)'}, {int(b['accepted'].sum())} accepted pairs")
    if pairs_arm:
        assert share <= PAIR_CAP, f"{name}: {100 * share:.2f} % of the pairs are unstable"
    if pairs_arm and name != "scaled_down":
        assert b["accepted"].sum() >= 32, f"{name}: the rays hardly hit anything"
    if name == "flat":                  # what the overlap filter of small_scenes.rays leaves of the 32 axis-aligned rays
        axis = (rays["dir"][:, 0] == 0) & (rays["dir"][:, 1] == 0)
        print(f"flat: {int(axis.sum())} axis-aligned rays, {int(b['accepted'][axis].any(1).sum())} of them cross a triangle")
        assert axis.sum() >= 8 and b["accepted"][axis].any(1).sum() >= 8, "flat: too few axis-aligned rays survive"
    for tree in ORACLE_TREES:
        leaves, nodes, root, count = rq._ora_tree(ora, tris, tree)
        what = f"{name}/{tree}"
        rows, box_tests, leaf_visits = rh.walk(nodes, leaves, root, count, every)
        if len(every) > m:                                            # the exact-only rays are not there to miss
            hit = sum(len(r) > 0 for r in rows[m:])
            print(f"{what}: {hit} of {len(every) - m} exact-only rays have a non-empty row")
            assert name != "scaled_down" or hit >= 16, f"{what}: {hit} exact-only rays hit anything"
        grows, gates, gb, gl = rf.walk_gated(nodes, leaves, root, count, every)
        assert (gb, gl) == (box_tests, leaf_visits), f"{what}: the two walks count differently"
        for i, (x, y) in enumerate(zip(rh.canon(rows), rh.canon(grows))):
            assert x.shape == y.shape and (x == y).all(), f"{what}: ray {i}: walk and walk_gated differ"
        dedup = rf.dedup_all(grows, gates)
        for k in (1, 2, 8):
            exp = rf.expected(grows, gates, k, every["tmax"], dedup=dedup)
            und = rf.undecided_share(exp, grows)
            print(f"{what}: k {k}: {100 * und:.3f} % undecided")
            assert und <= rf.CAP, f"{what}: k {k}: {100 * und:.2f} % of the rays are undecided"
        if pairs_arm:
            got = np.zeros((m, n), bool)
            for i, row in enumerate(rows[:m]):
                ids = row["primitive_id"].astype(np.int64)
                assert (ids < n).all()
                assert "splits" in tree or len(np.unique(ids)) == len(ids), f"{what}: ray {i}: a triangle twice in a row"
                got[i, ids] = True
            missing, extra = b["stable"] & b["accepted"] & ~got, b["stable"] & ~b["accepted"] & got
            assert not missing.any(), f"{what}: {missing.sum()} stable accepted pairs are not in their row: {np.argwhere(missing)[:4]}"
            assert not extra.any(), f"{what}: {extra.sum()} stable rejected pairs are in a row: {np.argwhere(extra)[:4]}"
        if cast_arm:
            rq._check_against_f64(tris, rays, nearest_records(rows[:m]), ref, ref["stable"], what, check_mt="pairs" not in tree,
                                  bound=RAY_CAP)


@pytest.mark.parametrize("name", ss.OPEN)
def test_points_against_float64(scenes, name):
    tris = ss.tris(name, scenes)
    for kind, p in ss.points(name, tris).items():
        d32 = pr.brute_force(p, np.inf, tris)[0]
        d64 = pr.brute_force_f64(p, tris)
        assert np.isfinite(d32).all() and float(d32.max()) < 1e30, "squared distances inside float32's range"
        M = max(float(np.abs(tris).max()), float(np.abs(p).max()))
        err = np.abs(np.sqrt(d32.astype(np.float64)) - d64) / (M * 2.0 ** -23)
        print(f"{name}/{kind}: {len(p)} points, {err.max():.2f} ulps of the largest coordinate")
        assert err.max() <= POINT_ULPS, f"{name}/{kind}: {err.max():.1f} ulps of the largest coordinate against float64"


@pytest.mark.parametrize("name,copies", (("stack", 64), ("twins", 2)))
def test_ties_are_ordered_by_id(scenes, name, copies):
    tris = ss.tris(name, scenes)
    p = ss.all_points(name, tris)
    rows = kr.brute_force_knn(p, np.inf, tris, 32)
    k = min(32, copies)
    assert (rows["primitive_id"][:, :k] == np.arange(k)[None, :]).all(), "equal dist2: ascending id"
    assert (rows["dist2"][:, :k] == rows["dist2"][:, :1]).all() and (rows["primitive_id"][:, k:] == kr.MISS).all()
    assert kr.ascending(rows)
    d2 = rows["dist2"][:, 0].copy()
    lists, counts = rr.sphere(p, d2, tris)
    assert (counts == copies).all() and all((x == np.arange(copies)).all() for x in lists), "exactly at the radius: all of them"
    off = d2 > 0
    assert off.sum() >= 64
    _, counts = rr.sphere(p[off], np.nextafter(d2[off], F(0)), tris)
    assert (counts == 0).all(), "one float below the shared distance: none"
    if name == "stack":
        q = ss.range_queries(name, tris)
        assert (rr.sphere(q["sphere", "at_the_distance"]["p"], q["sphere", "at_the_distance"]["dist2_max"], tris)[1] == 64).all()
        assert (rr.sphere(q["sphere", "one_float_below"]["p"], q["sphere", "one_float_below"]["dist2_max"], tris)[1] == 0).all()


def test_the_scenes_are_what_they_say(scenes):
    """sizes, the degeneracies the names promise, determinism, and query sets of at most 256"""
    sizes = {name: ss.tris(name, scenes).shape[0] for name in ss.OPEN + ss.CLOSED}
    assert [sizes[k] for k in ss.TINY] == [1, 2, 3, 4, 5, 2, 63, 64, 65]
    assert [sizes[k] for k in ss.DEGENERATE] == [40, 65, 64, 257, 129, 200, 200] and sizes["tetra"] == 4 and sizes["box"] == 12
    T = ss.tris("points", scenes).reshape(-1, 3, 3).astype(np.float64)
    assert (np.linalg.norm(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]), axis=1) <= 1e-6).all(), "points: zero area"
    assert (ss.tris("flat", scenes).reshape(-1, 3)[:, 2] == ss.FLAT_Z).all()
    s = ss.tris("stack", scenes)
    assert (s.view(np.uint32) == s.view(np.uint32)[:1]).all()
    t = ss.tris("twins", scenes)
    assert t[0].tobytes() == t[1].tobytes()
    assert float(np.abs(ss.tris("scaled_up", scenes)).max()) > 4e3 and float(np.abs(ss.tris("scaled_down", scenes)).max()) < 6e-4
    g = ss.tris("giant", scenes).reshape(-1, 3, 3)
    assert np.ptp(g[0], axis=0).max() == 1100 and np.ptp(g[1:], axis=1).max() < 0.05
    for name in ss.OPEN:
        a = ss.tris(name, scenes)
        assert a.tobytes() == ss.tris(name, scenes).tobytes() and ss.all_rays(name, a).tobytes() == ss.all_rays(name, a).tobytes()
        assert all(len(q) <= 256 for q in ss.range_queries(name, a).values())
        assert all(len(p) <= 256 for p in ss.points(name, a).values())
        assert len(ss.overlap_queries(name, a)) == 32
    # the closed meshes are closed and face outwards: the signed volume is the solid's
    for name, volume in (("tetra", None), ("box", float(np.prod(sdf_ref.BOX_HI - sdf_ref.BOX_LO)))):
        T = ss.tris(name, scenes).reshape(-1, 3, 3).astype(np.float64)
        v = (T[:, 0] * np.cross(T[:, 1], T[:, 2])).sum() / 6
        assert v > 0 and (volume is None or abs(v - volume) < 1e-6)
    assert ss.in_tetra(ss.tris("tetra", scenes).reshape(-1, 3).astype(np.float64).mean(0)[None])[0]
