"""GPU tests of EVERY query on the small scenes of tests/small_scenes.py: trees of one to five triangles, of two equal
triangles and of 63 / 64 / 65, whose root runs hold Tri and None slots directly, and degenerate or badly scaled geometry
(zero-area triangles, one flat axis, 64 identical triangles, far-apart clusters, one huge triangle, coordinates at 1e4 and
1e-3).  The per-query files draw their trees from five scenes of 800 to 4000 triangles; tests/test_gpu_fuzz.py pushes scenes
like these through the builders and rt_trace only.  Nothing here is random at run time and no tolerance is new: every
assertion is the one the query's own file makes on the big scenes, through that file's helpers, and the conditions the
float64 arms rest on are checked on the CPU first (tests/test_small_scenes_ref_cpu.py).

Every test is parametrised by (scene, tree kind) over all sixteen open scenes and all eight tree kinds, so each (query, tree
kind) pair below runs on the nine TINY and the seven DEGENERATE scenes:

  test                          calls                                                     reference
  test_closest_and_any_hit      IntersectRays (closest, any)                              walk rows (bit), shade_ref.cast (f64)
  test_sorted_and_indexed       SortRays, IntersectRaysIndexed                            ray_sort_ref.sort, the unsorted call
  test_all_hit                  RayHitsCount / RayHitsCollect                             ray_hits_ref.walk (bit), brute_f64
  test_first_k                  RayFirstHits, k = 1, 2, 8                                 ray_first_ref.expected / envelope
  test_filtered                 IntersectRaysFiltered, RayHitsCount/CollectFiltered,      ray_filter_ref.filtered on the walk
                                RayFirstHitsFiltered
  test_closest_point_and_knn    ClosestPoints, KNearest k = 1, 7, 32                      point_ref / knn_ref brute force (bit)
  test_range                    RangeQuery's count + collect, spheres and boxes           range_ref.sphere / box (sets)
  test_tri_overlaps             TriOverlapsCount / Collect, self_pairs on and off         tri_overlap_ref.brute_force (sets)
  test_signed_distance (*)      SignedDistance, Occupancy                                 sdf_ref.compose (bit), analytic inside
  test_instanced (**)           PrepareInstances, IntersectRaysInstanced(+Filtered)       walks of the BLAS on object rays (bit),
                                                                                          instance_filter_ref.brute_force (f64)
  test_every_query_on_the_tree_built_from_nothing: all of the above on n0, the bottom-up builder's tree of zero triangles.
  (*) on the two closed meshes (tetra, box) x eight tree kinds.  (**) on three BLAS tables (one instance of the one-triangle
  BLAS, two instances of the two-triangle BLAS, a `stack` BLAS) x eight BLAS tree kinds, the TLAS kind cycling.

The walk is the numpy tree walk over the DOWNLOADED node and leaf bytes, so it exists for hybrid + pairs, which has no oracle
builder; that kind is also held to its sibling `pairs` (same leaves, another top) record for record.  Split trees get the
arms their own files give them: real, distinct, sorted and within the documented bound (points), true matches (sets),
|sdist| (signed distance).  `stack`'s first-K tie order: ascending ids within every sub-run of equal t on all eight kinds; the
k lowest ids outright on the four kinds without pairs only, where all 64 t are one value.  Arms a scene does not get, with the reason, are listed in tests/small_scenes.py
(NO_F64_PAIRS, NO_F64_CAST, exact_rays).  Every output buffer has sentinels behind it."""
import numpy as np
import pytest

import instance_filter_ref as fr
import instance_ref as ir
import knn_ref as kr
import point_ref as pr
import ray_filter_ref as rx
import ray_first_ref as rf
import ray_hits_ref as rh
import sdf_ref as sr
import small_scenes as ss
import test_gpu_instance_filter as tif
import test_gpu_instances as ti
import test_gpu_knn as tk
import test_gpu_point_queries as tp
import test_gpu_range_queries as tg
import test_gpu_ray_filter as tf
import test_gpu_ray_first as t1
import test_gpu_ray_hits as th
import test_gpu_ray_queries as rq
import test_gpu_ray_sort as tsort
import test_gpu_sdf as tsd
import test_gpu_tri_overlaps as tov
import tri_overlap_ref as tr

pytestmark = pytest.mark.gpu

F = np.float32
TREES = rq.TREES
SENT, PAD = th.SENT, th.PAD
MISS = 0xFFFFFFFF
CASES = [(name, tree) for name in ss.OPEN for tree in TREES]
KS = (1, 2, 8)


def _split(tree):
    return "splits" in tree


def _one_slot(name, tree):
    """the root run of the one-triangle tree holds ONE slot that is not None (the Tri slot; the LBVH puts a None slot next to
    it), so every traced query counts exactly one box test.  (The hybrid kinds put a box run above it.)"""
    return name == "n1" and "hybrid" not in tree


# ------------------------------------------------------------------ the world: scenes, trees and references, computed once
class World:
    def __init__(self, rt, scenes):
        self.rt, self.scenes = rt, scenes
        self._m = {}

    def _memo(self, key, make):
        if key not in self._m:
            self._m[key] = make()
        return self._m[key]

    def tris(self, name):
        return self._memo(("tris", name), lambda: ss.tris(name, self.scenes))

    def rays(self, name):
        """-> (all rays as rt.RAY, the number of leading rays that have float64 arms)"""
        def make():
            t = self.tris(name)
            r = np.ascontiguousarray(ss.all_rays(name, t).astype(self.rt.RAY))
            r.setflags(write=False)
            return r, len(ss.rays(name, t))
        return self._memo(("rays", name), make)

    def gpu(self, name, tree):
        return self._memo(("gpu", name, tree), lambda: rq._gpu_tree(self.rt, self.tris(name), tree))

    def bytes(self, name, tree):
        return self._memo(("bytes", name, tree), lambda: th._download(self.rt, self.gpu(name, tree)[0]))

    def walk(self, name, tree):
        """test_gpu_ray_filter.Walk over the downloaded bytes: rows, gates, dets, box_tests, leaf_visits"""
        def make():
            nodes, leaves = self.bytes(name, tree)
            _, root, count = self.gpu(name, tree)
            return tf.Walk(nodes, leaves, root, count, self.rays(name)[0], self.tris(name).shape[0])
        return self._memo(("walk", name, tree), make)

    def cast(self, name):
        return self._memo(("cast", name), lambda: rq._f64(self.tris(name), self.rays(name)[0][:self.rays(name)[1]]))

    def brute(self, name):
        return self._memo(("brute", name), lambda: rh.brute_f64(self.tris(name), self.rays(name)[0][:self.rays(name)[1]]))

    def points(self, name):
        return self._memo(("points", name), lambda: ss.all_points(name, self.tris(name)))

    def closest_exp(self, name):
        return self._memo(("closest", name), lambda: tp._expected(self.points(name), np.inf, self.tris(name)))

    def knn_exp(self, name):
        return self._memo(("knn", name), lambda: kr.brute_force_knn(self.points(name), np.inf, self.tris(name), 32))

    def range_sets(self, name):
        def make():
            t = self.tris(name)
            return {k: (q, tg._expected(q, t)) for k, q in ss.range_queries(name, t).items()}
        return self._memo(("range", name), make)

    def overlap_sets(self, name):
        def make():
            t = self.tris(name)
            shifted = ss.overlap_queries(name, t)
            return {"self": (t, True, tr.brute_force(t, t, self_pairs=True)),
                    "own": (t[:256], False, tr.brute_force(t[:256], t)),
                    "shifted": (shifted, False, tr.brute_force(shifted, t))}
        return self._memo(("overlap", name), make)


@pytest.fixture(scope="module")
def world(rt, scenes):
    return World(rt, scenes)


def _in_row(rec, row):
    return bool((np.ascontiguousarray(row).view(np.uint32).reshape(-1, 4) == np.frombuffer(rec.tobytes(), np.uint32)[None, :]).all(1).any())


def _check_member_of_rows(hits, rows, what, nearest=True):
    """a hit record is a record of the ray's all-hit row, bit for bit, at the row's smallest t when `nearest`; a miss is
    (inf, MISS, 0, 0) and has an empty row"""
    miss = rf.miss_records(1)[0]
    for i, (h, row) in enumerate(zip(hits, rows)):
        if h["primitive_id"] == MISS:
            assert h.tobytes() == miss.tobytes(), f"{what}: ray {i}: a miss record is {h}"
            assert len(row) == 0, f"{what}: ray {i}: a miss, the walk's row has {len(row)} records"
            continue
        assert len(row) and _in_row(h, row), f"{what}: ray {i}: {h} is not in the walk's row {row}"
        with np.errstate(invalid="ignore"):
            assert not nearest or np.isnan(h["t"]) or h["t"] == np.fmin.reduce(row["t"]), f"{what}: ray {i}: not the nearest of its row"


# ------------------------------------------------------------------ closest and any hit
@pytest.mark.parametrize("name,tree", CASES)
def test_closest_and_any_hit(world, name, tree):
    rt = world.rt
    tris, (rays, m), g, walk = world.tris(name), world.rays(name), world.gpu(name, tree), world.walk(name, tree)
    what = f"{name}/{tree}"
    hits, _ = tf._closest(rt, g, rays, tf.UNFILTERED)                   # (sentinels behind the records: checked inside)
    anyh, _ = tf._closest(rt, g, rays, tf.UNFILTERED, any_hit=True)
    _check_member_of_rows(hits, walk.rows, what)
    _check_member_of_rows(anyh, walk.rows, f"{what} any-hit", nearest=False)
    assert ((hits["primitive_id"] != MISS) == (anyh["primitive_id"] != MISS)).all(), f"{what}: any-hit and closest-hit disagree"
    if name not in ss.NO_F64_CAST:
        ref = world.cast(name)
        rq._check_against_f64(tris, rays[:m], hits[:m], ref, ref["stable"], what, check_mt="pairs" not in tree)
    if tree == "hybrid_pairs":          # no oracle builder: the same leaves under another top give the same records
        sib, _ = tf._closest(rt, world.gpu(name, "pairs"), rays, tf.UNFILTERED)
        same = sib["primitive_id"] == hits["primitive_id"]              # (equal triangles tie on t: either id is right)
        assert (sib["t"].view(np.uint32) == hits["t"].view(np.uint32)).all() and hits[same].tobytes() == sib[same].tobytes()


# ------------------------------------------------------------------ sorted and indexed
def _indexed(rt, g, rays_dev, order_dev, n, any_hit=False):
    import torch
    inp, root, count = g
    buf = torch.full(((n + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    hits = buf[:n * 4].view(torch.float32).view(n, 4)
    rt.IntersectRaysIndexed(inp.triangles_out, inp.nodes_out, root, count, rays_dev, order_dev, hits, any_hit=any_hit)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[n * 4:] == SENT).all(), "the indexed call wrote past the last record"
    return h[:n * 4].view(rt.HIT).reshape(n)


@pytest.mark.parametrize("name,tree", CASES)
def test_sorted_and_indexed(world, name, tree):
    rt = world.rt
    tris, (rays, _), g = world.tris(name), world.rays(name), world.gpu(name, tree)
    what = f"{name}/{tree}"
    got, ref = tsort._check_sort(rt, g, rays, what)                    # order, keys, num_live and the root box, bit for bit
    assert ref["num_live"] == len(rays)
    V = tris.reshape(-1, 3)
    lo, hi = got["box"]
    assert (lo <= V.min(0)).all() and (hi >= V.max(0)).all(), f"{what}: the root box {lo} .. {hi} does not hold the scene"
    if tree == "bottom_up":             # (LBVH slot boxes are the vertex boxes below them, unpadded)
        assert (lo == V.min(0)).all() and (hi == V.max(0)).all(), f"{what}: the root box {lo} .. {hi} is not the scene's"
    for any_hit in (False, True):
        exp, _ = tf._closest(rt, g, rays, tf.UNFILTERED, any_hit=any_hit)
        idx = _indexed(rt, g, got["rays_dev"], got["order_dev"], len(rays), any_hit=any_hit)
        assert idx.tobytes() == exp.tobytes(), f"{what} any_hit={any_hit}: {(idx != exp).sum()} records differ from the unsorted call's"


# ------------------------------------------------------------------ all-hit
@pytest.mark.parametrize("name,tree", CASES)
def test_all_hit(world, name, tree):
    rt = world.rt
    tris, (rays, m), (inp, root, count), walk = world.tris(name), world.rays(name), world.gpu(name, tree), world.walk(name, tree)
    what = f"{name}/{tree}"
    r = th._hits(rt, inp.triangles_out, inp.nodes_out, root, count, rays)       # count and collect agree, sentinels: inside
    assert r.st_count == 0
    assert (r.offsets == rh.offsets(walk.rows)).all(), f"{what}: offsets differ from the prefix sum of the walk's lengths"
    assert (r.counts == [len(x) for x in walk.rows]).all()
    th._assert_rows_equal(r.rows, walk.rows, what)
    assert r.ctr_count[0] == walk.box_tests and r.ctr_count[1] == walk.leaf_visits, \
        f"{what}: counters {r.ctr_count[:2]}, the walk counts {walk.box_tests}, {walk.leaf_visits}"
    closest = th._closest(rt, (inp, root, count), rays)
    _check_member_of_rows(closest, r.rows, f"{what}: closest hit against the device's rows")
    if name not in ss.NO_F64_PAIRS and not _split(tree):
        b = world.brute(name)
        nt = tris.shape[0]
        got = np.zeros((m, nt), bool)
        for i, row in enumerate(r.rows[:m]):
            ids = row["primitive_id"].astype(np.int64)
            assert (ids < nt).all() and len(np.unique(ids)) == len(ids), f"{what}: ray {i}: a triangle twice in a row"
            got[i, ids] = True
        missing, extra = b["stable"] & b["accepted"] & ~got, b["stable"] & ~b["accepted"] & got
        assert not missing.any(), f"{what}: {missing.sum()} stable accepted pairs are not in their row: {np.argwhere(missing)[:4]}"
        assert not extra.any(), f"{what}: {extra.sum()} stable rejected pairs are in a row: {np.argwhere(extra)[:4]}"


# ------------------------------------------------------------------ first-K
def _check_first(rows, frows, fgates, rays, k, what):
    """decided rays are E bit for bit, the envelope (records of the row, ascending, padded with misses, nothing owed) holds on
    every ray.  -> (undecided share, number of hit rays)"""
    exp = rf.expected(frows, fgates, k, rays["tmax"])
    share = rf.undecided_share(exp, frows)
    assert share <= rf.CAP, f"{what}: k {k}: {100 * share:.2f} % of the rays are undecided"
    want = rf.padded(exp, k)
    n = len(rays)
    equal = (rows.view(np.uint32).reshape(n, -1) == want.view(np.uint32).reshape(n, -1)).all(1)
    decided = np.array([e[1] for e in exp], bool)
    wrong = np.nonzero(decided & ~equal)[0]
    assert len(wrong) == 0, f"{what}: k {k}: {len(wrong)} decided rays differ from E; ray {wrong[0]}: {rows[wrong[0]]} != {want[wrong[0]]}"
    for i in range(n):
        why = rf.envelope_violation(rows[i], frows[i], fgates[i], k, rays["tmax"][i])
        assert why is None, f"{what}: k {k}: ray {i}: {why}"
    return share, decided


@pytest.mark.parametrize("name,tree", CASES)
def test_first_k(world, name, tree):
    rt = world.rt
    (rays, _), (inp, root, count), walk = world.rays(name), world.gpu(name, tree), world.walk(name, tree)
    what = f"{name}/{tree}"
    for k in KS:                                                      # (8 exceeds the tree on n1 .. n5 and twins)
        rows, ctr, status = t1._first(rt, inp.triangles_out, inp.nodes_out, root, count, rays, k)    # sentinels: inside
        assert status == 0, f"{what}: k {k}: status {status}"
        share, decided = _check_first(rows, walk.rows, walk.gates, rays, k, what)
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits
        if name == "stack":             # ties on t come out by ascending id, on every tree: within each sub-run of equal t ...
            for i in np.nonzero(np.array([len(r) > 0 for r in walk.rows]))[0]:
                live = rows[i][rows[i]["primitive_id"] != MISS]
                same_t = live["t"][1:] == live["t"][:-1]
                assert (live["t"][1:] >= live["t"][:-1]).all() and (live["primitive_id"][1:] > live["primitive_id"][:-1])[same_t].all(), \
                    f"{what}: k {k}: ray {i}: ties out of order: {live}"
        if name == "stack" and "pairs" not in tree:     # ... and without pairs all 64 t are ONE value, so the k lowest ids
            # (a pair leaf stores its second triangle rotated, and a rotated Moller-Trumbore rounds t differently)
            hit = np.array([len(r) > 0 for r in walk.rows]) & decided
            assert hit.sum() >= 64 and (rows["primitive_id"][hit] == np.arange(k)[None, :]).all(), f"{what}: k {k}: ties out of order"
            assert (rows["t"][hit] == rows["t"][hit][:, :1]).all()
        if name in ("n1", "n2", "twins") and k == 8:
            assert (rows["primitive_id"][:, 2:] == MISS).all(), f"{what}: more records than triangles"
    print(f"{what}: k {KS[-1]}: {100 * share:.3f} % undecided")


# ------------------------------------------------------------------ filtered ray queries
def _filters(walk, num_triangles):
    """cull back faces; a mask that removes triangle 0; skip id 0 on every ray (the ONLY triangle of n1); make_filter's skip of
    each ray's own nearest hit; make_filter's combination of all three mechanisms"""
    n = len(walk.rays)
    pm = np.ones(num_triangles, np.uint32)
    pm[0] = 2
    skip0 = np.zeros(n, rx.RAY_FILTER)
    skip0["mask"], skip0["skip_id"] = rx.ALL, 0
    return {"cull_back": rx.Filter(rx.CULL_BACK), "mask_without_0": rx.Filter(0, 1, pm, None),
            "skip_0": rx.Filter(0, 0, None, skip0),
            "skip_nearest": rx.make_filter("skip_nearest", walk.rows, num_triangles),
            "combined": rx.make_filter("combined", walk.rows, num_triangles)}


@pytest.mark.parametrize("name,tree", CASES)
def test_filtered(world, name, tree):
    rt = world.rt
    tris, (rays, _), g, walk = world.tris(name), world.rays(name), world.gpu(name, tree), world.walk(name, tree)
    for fname, flt in _filters(walk, tris.shape[0]).items():
        what = f"{name}/{tree}/{fname}"
        frows, fgates = rx.filtered(walk.rows, walk.gates, walk.dets, flt)
        r = tf._hits(rt, g, rays, flt)                                # count and collect agree, sentinels: inside
        assert (r.offsets == rh.offsets(frows)).all(), f"{what}: offsets differ from the prefix sum of |W_f|"
        tf._same_rows(r.rows, frows, what)
        assert r.ctr_count[0] == walk.box_tests and r.ctr_count[1] == walk.leaf_visits, f"{what}: counters are the unfiltered walk's"
        if fname in ("mask_without_0", "skip_0"):
            assert not any((row["primitive_id"] == 0).any() for row in r.rows), f"{what}: triangle 0 reported"
            if tris.shape[0] == 1:
                assert r.offsets[-1] == 0, f"{what}: the only triangle is filtered out"
        hits, _ = tf._closest(rt, g, rays, flt)
        anyh, _ = tf._closest(rt, g, rays, flt, any_hit=True)
        _check_member_of_rows(hits, frows, what)
        _check_member_of_rows(anyh, frows, f"{what} any-hit", nearest=False)
        if fname in ("cull_back", "mask_without_0", "skip_0"):
            for k in (1, 8):
                rows, _, status = tf._first(rt, g, rays, k, flt)
                assert status == 0
                _check_first(rows, frows, fgates, rays, k, what)


# ------------------------------------------------------------------ closest point and k-nearest
def _bound_ok(got_d2, bf_d2, tris, p, what):
    assert (got_d2 >= bf_d2).all(), what
    M = max(float(np.abs(tris).max()), float(np.abs(p).max()))
    excess = np.sqrt(got_d2.astype(np.float64)) - np.sqrt(bf_d2.astype(np.float64))
    assert excess.max() <= 2.0 ** -20 * M, f"{what}: {excess.max()} beyond 2^-20 * {M}"


@pytest.mark.parametrize("name,tree", CASES)
def test_closest_point_and_knn(world, name, tree):
    rt = world.rt
    tris, p, g = world.tris(name), world.points(name), world.gpu(name, tree)
    T = tris.reshape(-1, 3, 3)
    n = len(p)
    q = tp._queries(p)
    what = f"{name}/{tree}"
    exp = world.closest_exp(name)
    got, ctr, st = tp._query_tree(rt, g, q, counters=True, status=True, n_alloc=n + PAD)
    assert (got[n:].view(np.float32) == 7.0).all(), f"{what}: records past num_queries were written"
    got = got[:n]
    assert st == 0 and ctr[0] > 0 and ctr[1] >= n and ctr[2] == 0 and ctr[3] == 0
    assert not _one_slot(name, tree) or (ctr[0] == n and ctr[1] == n), f"{what}: counters {ctr[:2]} for {n} queries of one slot"
    if not _split(tree):
        tp._assert_records_equal(got, exp, what)
    else:
        ids = got["primitive_id"]
        assert (ids < T.shape[0]).all(), f"{what}: a miss with an infinite radius"
        d, u, v = pr.d2(p, T[ids, 0], T[ids, 1], T[ids, 2])
        assert (got["dist2"].view(np.uint32) == d.view(np.uint32)).all()
        assert (got["u"].view(np.uint32) == u.view(np.uint32)).all() and (got["v"].view(np.uint32) == v.view(np.uint32)).all()
        _bound_ok(got["dist2"], exp["dist2"], tris, p, what)
    exp32 = world.knn_exp(name)
    for k in (1, 7, 32):                                              # (7 and 32 exceed the tree on the tiny scenes)
        rows, ctr, st = tk._knn_tree(rt, g, q, k, counters=True, status=True, n_alloc=n + PAD)
        assert (rows[n:].view(np.float32) == 7.0).all(), f"{what}: k {k}: rows past num_queries were written"
        rows = rows[:n]
        assert st == 0 and ctr[2] == 0 and ctr[3] == 0
        assert not _one_slot(name, tree) or (ctr[0] == n and ctr[1] == n), f"{what}: k {k}: counters {ctr[:2]} for {n} queries"
        if not _split(tree):
            tk._assert_rows_equal(rows, exp32[:, :k], f"{what}/k={k}")
        else:
            full = min(k, T.shape[0])
            assert (rows["primitive_id"][:, :full] < T.shape[0]).all() and (rows["primitive_id"][:, full:] == MISS).all()
            tk._assert_real_distinct_sorted(rows, p, tris, f"{what}/k={k}")
            _bound_ok(rows["dist2"][:, :full], exp32["dist2"][:, :full], tris, p, f"{what}/k={k}")


# ------------------------------------------------------------------ range
@pytest.mark.parametrize("name,tree", CASES)
def test_range(world, name, tree):
    rt = world.rt
    g = world.gpu(name, tree)
    for key, (q, exp) in world.range_sets(name).items():
        what = f"{name}/{tree}/{key}"
        r = tg._range(rt, g, q)                                       # count and collect agree, sentinels: inside
        assert r.st_count == 0
        assert (r.offsets == np.concatenate([[0], np.cumsum(r.counts.astype(np.int64))])).all(), f"{what}: offsets"
        assert not _one_slot(name, tree) or r.ctr_count[0] == len(q), f"{what}: {r.ctr_count[0]} box tests for {len(q)} queries"
        if not _split(tree):
            tg._assert_exact(r, exp, what)
        else:
            assert all(np.isin(got, e).all() for got, e in zip(r.lists, exp[0])), f"{what}: a false match"


# ------------------------------------------------------------------ triangle overlap
@pytest.mark.parametrize("name,tree", CASES)
def test_tri_overlaps(world, name, tree):
    rt = world.rt
    g = world.gpu(name, tree)
    for key, (q, self_pairs, exp) in world.overlap_sets(name).items():
        what = f"{name}/{tree}/{key}"
        r = tov._overlaps(rt, g, q, self_pairs=self_pairs)            # count and collect agree, sentinels: inside
        assert r.st_count == 0
        assert not _one_slot(name, tree) or r.ctr_count[0] == len(q), f"{what}: {r.ctr_count[0]} box tests for {len(q)} queries"
        if not _split(tree):
            tov._assert_exact(r, exp, what)
        else:
            assert all(np.isin(got, e).all() for got, e in zip(r.lists, exp[0])), f"{what}: a false match"


# ------------------------------------------------------------------ signed distance and occupancy
def _sdf_points(name, tris):
    """256 points: 96 uniform in 1.5 x the mesh box, 32 inside the (convex) mesh, 64 near the surface, 64 exactly on it
    (corners, edge midpoints, face points as float32)"""
    rng = np.random.default_rng(ss.SEED[name] + 7)
    T = tris.reshape(-1, 3, 3).astype(np.float64)
    V = T.reshape(-1, 3)
    c, half = (V.min(0) + V.max(0)) / 2, (V.max(0) - V.min(0)) / 2
    uni = rng.uniform(c - 1.5 * half, c + 1.5 * half, (96, 3))
    uni = np.concatenate([uni, (rng.dirichlet(np.ones(len(V)), 32)[:, :, None] * V[None]).sum(1)])
    t = T[rng.integers(0, len(T), 96)]
    surf = (rng.dirichlet((1, 1, 1), 96)[:, :, None] * t).sum(1)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    near = surf[:64] + nrm[:64] * (10 ** rng.uniform(-5, -2, 64) * rng.choice([-1, 1], 64))[:, None]
    t3 = T[rng.integers(0, len(T), 32)]
    on = np.concatenate([surf[64:80], t3[:8, 0], (t3[8:, 0] + t3[8:, 1]) / 2])
    return np.ascontiguousarray(np.concatenate([uni, near, on]).astype(F))


@pytest.mark.parametrize("name", ss.CLOSED)
@pytest.mark.parametrize("kind", TREES)
def test_signed_distance(world, name, kind):
    rt = world.rt
    tris = world.tris(name)
    inp, root, count = world.gpu(name, kind)
    tree = (inp.triangles_out, inp.nodes_out, root, count)
    p = _sdf_points(name, tris)
    q = sr.queries(p)
    b = sr.brute_f64(tris, p, sr.DEFAULT_DIRS)                        # the reference alone: which points are certain
    sure = b["stable"] & (b["dist"] >= sr.NEAR)
    inside = ss.in_tetra(p) if name == "tetra" else sr._in_box(p.astype(np.float64), sr.BOX_LO, sr.BOX_HI)
    assert sure.sum() >= 100 and (sure & inside).sum() >= 8 and (sure & ~inside).sum() >= 50
    assert (sr.vote(b["counts"])[sure] == inside[sure]).all(), "the float64 reference itself: odd inside, even outside"
    for votes, dirs in tsd.COMBOS:
        what = f"{name}/{kind}/votes {votes}/{'default' if dirs is None else 'caller'} dirs"
        c = sr.compose(rt, tree, q, votes, dirs)
        r = tsd._run(rt, tree, q, votes, dirs)                        # sentinels behind both outputs: inside
        assert c["status"] == 0 and r.st_sdf == 0 and r.st_occ == 0
        assert (r.prim == c["primitive_id"]).all(), f"{what}: {(r.prim != c['primitive_id']).sum()} primitive ids differ"
        if _split(kind):
            assert (tsd._bits(np.abs(r.sdist)) == tsd._bits(np.abs(c["sdist"]))).all(), f"{what}: |sdist| differs"
            continue
        assert (tsd._bits(r.sdist) == tsd._bits(c["sdist"])).all(), f"{what}: sdist differs from the composition"
        assert (r.inside == c["inside"]).all(), f"{what}: occupancy differs from the composition"
        assert (r.ctr_sdf[:2] == c["counters"]).all() and (r.ctr_occ[:2] == c["vote_counters"].sum(0)).all()
        if dirs is None:
            assert (r.inside.astype(bool)[sure] == inside[sure]).all(), f"{what}: inside wrong against the analytic solid"
            assert ((r.sdist < 0)[sure] == inside[sure]).all()
            M = max(float(np.abs(p).max()), float(np.abs(tris).max()))
            assert (np.abs(np.abs(r.sdist).astype(np.float64) - b["dist"]) <= 4 * 2.0 ** -23 * M).all(), f"{what}: |sdist| against float64"


# ------------------------------------------------------------------ instanced
TABLES = ("one", "two_pairs", "stack")
TLAS = ti.TLAS_KINDS


def _table(name):
    """-> (scene of the BLAS, object_to_world matrices)"""
    if name == "one":
        return "n1", [ti._affine(ir.rotation(0.3, -0.5, 0.9) * 1.25, (0.5, -1.0, 2.0))]
    if name == "two_pairs":
        return "n2", [ti._affine(np.eye(3), (0, 0, 0)), ti._affine(ir.rotation(0.2, 0.4, -0.3) @ np.diag([1.0, -1.0, 1.5]), (0.3, 0.2, 0.4))]
    return "stack", [ti._affine(ir.rotation(-0.4, 0.1, 0.6) @ np.diag([1.5, 0.7, 1.0]), (0.1, 0.2, -0.3))]


def _instanced(sc, rays, flt, any_hit=False):
    """tif._run with sentinels behind both outputs -> (HIT array, instance ids)"""
    import torch
    rt = sc.rt
    d = rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)
    n = d.shape[0]
    hbuf = torch.full(((n + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    ibuf = torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")
    hits, ids = hbuf[:n * 4].view(torch.float32).view(n, 4), ibuf[:n]
    if flt is tif.UNFILTERED:
        sc.query(d, hits, ids, any_hit=any_hit)
    else:
        root, count = sc.root
        rt.IntersectRaysInstancedFiltered(sc.tlas.triangles_out, sc.tlas.nodes_out, root, count, sc.records, sc.n, sc.table,
                                          len(sc.entries), d, hits, ids, tif._dev_ifilter(rt, flt), any_hit=any_hit)
    torch.cuda.synchronize()
    h, i = hbuf.cpu().numpy().view(np.uint32), ibuf.cpu().numpy().view(np.uint32)
    assert (h[n * 4:] == SENT).all() and (i[n:] == SENT).all(), "the instanced call wrote past num_rays"
    return h[:n * 4].view(rt.HIT).reshape(n), i[:n]


def _instance_filters(num_instances, n):
    per_inst = fr.instance_filters(num_instances)
    per_inst["mask"][0] = 2                                           # ray_mask 1: instance 0 is never entered
    skip = np.zeros(n, fr.INSTANCE_RAY_FILTER)
    skip["mask"], skip["skip_instance"], skip["skip_id"] = fr.ALL, 0, 0     # primitive 0 of instance 0: the ONLY triangle of `one`
    return {"unfiltered": tif.UNFILTERED, "keep_all": fr.InstanceFilter(), "cull_back": fr.InstanceFilter(fr.CULL_BACK),
            "without_instance_0": fr.InstanceFilter(0, 1, per_inst, None), "skip_0_of_0": fr.InstanceFilter(0, 0, None, skip)}


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("tree", TREES)
def test_instanced(world, table, tree):
    rt = world.rt
    scene, mats = _table(table)
    tris = world.tris(scene)
    inp, root, count = world.gpu(scene, tree)
    nodes, leaves = world.bytes(scene, tree)
    inst = ir.instance_array(mats, [0] * len(mats))
    kind = TLAS[(TABLES.index(table) + TREES.index(tree)) % len(TLAS)]
    what = f"{table}/{tree}/TLAS {kind}"
    sc = ti.Instanced(rt, [(inp.triangles_out, inp.nodes_out, root, count)], inst, kind)
    sc.frame()
    assert rt.instance_status(sc.status) == 0, f"{what}: PrepareInstances status"
    W = sc.host_records()["world_to_object"]
    wt, inst_of, prim_of = ir.world_triangles([tris], inst)
    rays = ss.rays(scene, np.ascontiguousarray(wt.astype(F))).astype(rt.RAY)      # (the scene's ray recipe, on the world triangles)
    n = len(rays)
    walks = fr.walk_instances([(leaves, nodes, root, count)], inst, W, rays)
    cand = fr.candidates(rays, wt)
    for fname, flt in _instance_filters(inst.size, n).items():
        f = fr.InstanceFilter() if flt is tif.UNFILTERED else flt
        hits, ids = _instanced(sc, rays, flt)
        anyh, aids = _instanced(sc, rays, flt, any_hit=True)
        # bit for bit: the record is a kept record of the entered instance `ids`, at the smallest kept t over all instances
        kept = []
        for k, (rows, dets) in enumerate(walks):
            eff, entered = fr.effective(f, k, W[k], n)
            kept.append([row[rx.keep(row, det, i, eff)] if entered[i] else row[:0] for i, (row, det) in enumerate(zip(rows, dets))])
        for i in range(n):
            tmin = min([np.fmin.reduce(k_[i]["t"]) for k_ in kept if len(k_[i])], default=None)
            for h, hid, nearest in ((hits[i], ids[i], True), (anyh[i], aids[i], False)):
                w = f"{what}/{fname}: ray {i}"
                assert (h["primitive_id"] == MISS) == (hid == MISS) == (tmin is None), f"{w}: hit / miss: {h}, instance {hid}"
                if tmin is None:
                    assert h.tobytes() == rf.miss_records(1)[0].tobytes(), f"{w}: a miss record is {h}"
                    continue
                assert hid < inst.size and _in_row(h, kept[hid][i]), f"{w}: {h} is not a kept record of instance {hid}"
                assert not nearest or h["t"] == tmin, f"{w}: t {h['t']}, the nearest kept record has {tmin}"
        if fname == "without_instance_0":
            assert not (ids == 0).any() and (inst.size > 1 or (ids == MISS).all())
        if fname == "skip_0_of_0":
            assert not ((ids == 0) & (hits["primitive_id"] == 0)).any() and (table != "one" or (ids == MISS).all())
        # float64 over the kept world triangles, as test_gpu_instance_filter._check_f64 compares
        ref, unique = fr.brute_force(cand, inst_of, prim_of, rays, f)
        got = ids != MISS
        assert not (unique & (got != ref["hit"])).any(), f"{what}/{fname}: hit / miss differs on unique rays"
        sel = unique & ref["hit"]
        k = ref["tri"][sel]
        assert (ids[sel] == inst_of[k]).all() and (hits["primitive_id"][sel] == prim_of[k]).all(), f"{what}/{fname}: instance / primitive"
        assert (np.abs(hits["t"][sel] - ref["t"][sel]) <= 1e-5 * np.maximum(1, ref["t"][sel])).all(), f"{what}/{fname}: t"
        if fname == "unfiltered" and table != "stack":            # (64 rivals at one t: float64 calls no hit of `stack` unique)
            assert sel.sum() >= 32, f"{what}: {sel.sum()} unique hits: not a test"


# ------------------------------------------------------------------ the tree built from zero triangles
@pytest.mark.parametrize("tree", ss.N0_TREES)
def test_every_query_on_the_tree_built_from_nothing(world, tree):
    """n0: the builder's own empty tree, a root run of two None slots -- every slot of the run fails `type != None`, which
    n1's run (a Tri slot beside one None slot) never shows.  Every query: all records miss, every CSR row is empty, status 0,
    NOTHING is counted (a box test is a slot that is not None), sentinels intact (inside the helpers)."""
    import torch
    rt = world.rt
    name = ss.EMPTY
    g = world.gpu(name, tree)
    inp, root, count = g
    tri, nod = inp.triangles_out, inp.nodes_out
    assert count == 2
    run = rt.to_host(nod, rt.NODE, 2)
    assert ((run["w28"] >> 29) == 0).all() and ((run["w12"] >> 29) == 0).all(), f"n0/{tree}: the root run is not two None slots"
    P = ss.proxy()
    rays = np.ascontiguousarray(ss.all_rays(name, P).astype(rt.RAY))
    n = len(rays)
    miss = rf.miss_records(n)
    what = f"n0/{tree}"
    skip0 = np.zeros(n, rx.RAY_FILTER)
    skip0["mask"], skip0["skip_id"] = rx.ALL, 0
    flt = {"unfiltered": tf.UNFILTERED, "cull_back": rx.Filter(rx.CULL_BACK), "skip_0": rx.Filter(0, 0, None, skip0)}
    for fname, f in flt.items():
        for any_hit in (False, True):
            hits, ctr = tf._closest(rt, g, rays, f, any_hit=any_hit)
            # ([2] and [3] count the waves' phases, not tests: the waves do run over the run of two slots)
            assert hits.tobytes() == miss.tobytes() and (ctr[:2] == 0).all(), f"{what}/{fname} any_hit={any_hit}: {ctr}"
        r = tf._hits(rt, g, rays, f)                                  # status 0 and count == collect: asserted inside
        assert (r.offsets == 0).all() and (r.counts == 0).all() and (r.ctr_count == 0).all(), f"{what}/{fname}: all-hit"
        for k in KS:
            rows, ctr, status = tf._first(rt, g, rays, k, f)
            assert status == 0 and (ctr == 0).all() and rows.tobytes() == rf.miss_records(n * k).tobytes(), f"{what}/{fname}: k {k}"
    got, ref = tsort._check_sort(rt, g, rays, what)                   # the box of a run without a slot is the point 0
    assert ref["num_live"] == n and (got["box"][0] == 0).all() and (got["box"][1] == 0).all()
    assert _indexed(rt, g, got["rays_dev"], got["order_dev"], n).tobytes() == miss.tobytes()
    p = ss.all_points(name, P)
    q = tp._queries(p)
    hits, ctr, st = tp._closest(rt, tri, nod, root, count, q, counters=True, status=True, n_alloc=len(p) + PAD)
    assert (hits[len(p):].view(np.float32) == 7.0).all() and st == 0 and (ctr == 0).all()
    h = hits[:len(p)]
    assert (h["primitive_id"] == MISS).all() and (h["dist2"] == np.inf).all() and (h["u"] == 0).all() and (h["v"] == 0).all()
    for k in (1, 7, 32):
        rows, ctr, st = tk._knn(rt, tri, nod, root, count, q, k, counters=True, status=True, n_alloc=len(p) + PAD)
        assert (rows[len(p):].view(np.float32) == 7.0).all() and st == 0 and (ctr == 0).all()
        assert (rows[:len(p)]["primitive_id"] == MISS).all() and (rows[:len(p)]["dist2"] == np.inf).all()
    for key, rq_ in ss.range_queries(name, P).items():
        r = tg._range(rt, g, rq_)
        assert r.st_count == 0 and (r.offsets == 0).all() and (r.ctr_count == 0).all(), f"{what}/{key}"
    for key, oq in (("proxy", P), ("shifted", ss.overlap_queries(name, P))):
        r = tov._overlaps(rt, g, oq)
        assert r.st_count == 0 and (r.offsets == 0).all() and (r.ctr_count == 0).all(), f"{what}/{key}"
    for votes, dirs in tsd.COMBOS:
        r = tsd._run(rt, (tri, nod, root, count), sr.queries(p), votes, dirs)
        assert r.st_sdf == 0 and r.st_occ == 0 and (r.ctr_sdf == 0).all() and (r.ctr_occ == 0).all()
        assert (r.prim == MISS).all() and (r.sdist == np.inf).all() and (r.inside == 0).all(), f"{what}: votes {votes}"
    # instanced: a BLAS whose root run has no box is a bad BLAS -- flagged by PrepareInstances, never entered
    for kind in TLAS:
        sc = ti.Instanced(rt, [(tri, nod, root, count)], ir.instance_array([np.eye(3, 4)], [0]), kind)
        sc.frame()
        assert rt.instance_status(sc.status) == rt.RT_INSTANCE_BAD_BLAS, f"{what}: TLAS {kind}: status"
        for f in (tif.UNFILTERED, fr.InstanceFilter(fr.CULL_BACK)):
            for any_hit in (False, True):
                hits, ids = _instanced(sc, rays, f, any_hit=any_hit)
                assert hits.tobytes() == miss.tobytes() and (ids == MISS).all(), f"{what}: TLAS {kind}: a flagged instance was hit"
    torch.cuda.synchronize()
