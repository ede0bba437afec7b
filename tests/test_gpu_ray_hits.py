"""GPU tests of the all-hit ray queries (rt_ray_hits_count / rt_ray_hits_collect) on every tree the builders make.

1. rows against the walk: on all eight tree kinds the row of every ray equals the numpy tree walk over the tree's own bytes
   (tests/ray_hits_ref.py) as a multiset of 16-byte records, bit for bit; offsets, counts and both calls' counters agree;
2. rows against float64 on the six non-split trees: every stable accepted (ray, triangle) pair of the brute force over the
   caller's triangles is in the row, no stable rejected pair is; on non-pair trees each record is the kernel's own float32
   Moller-Trumbore of its triangle, bit for bit;
3. the closest-hit relation on all eight trees: rt_intersect_rays's (t, u, v) bits are in the row, min t of the row is at most
   it, a miss has an empty row and the other way round;
4. dead rays and the empty tree; 5. batch ends and sentinels; 6. fixed-K collection and truncation; 7. parity on a closed
   mesh; 8. stack overflow; 9. refit; 10. hipGraph; 11. RayHits(..., sort=True)."""
import numpy as np
import pytest

import range_sets as rs
import ray_hits_ref as rh
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

TREES = ("bottom_up", "pairs", "hybrid", "hybrid_pairs", "sah", "sah_pairs", "sah_splits", "sah_pairs_splits")
EXACT_TREES = TREES[:6]
SCENES = ("grid", "soup", "cornell", "fractal")
F = np.float32
SENT = 0x5EA7BEEF        # sentinel word of every output buffer
PAD = 64                 # sentinel words / records behind every output buffer


# ------------------------------------------------------------------ helpers
class Result:
    pass


def _dev_rays(rt, rays):
    import torch
    return rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)


def _count(rt, tri, nod, root, count, rd):
    """-> (offsets int64[n+1] numpy, counters uint64[4], status, the device offsets)"""
    import torch
    n = rd.shape[0]
    off = torch.full((n + 1 + PAD,), SENT, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert rt.RayHitsCount(tri, nod, root, count, rd, off[:n + 1], counters=ctr, status=st) == n
    torch.cuda.synchronize()
    o = off.cpu().numpy()
    assert (o[n + 1:] == SENT).all(), "RayHitsCount wrote past offsets[n]"
    return o[:n + 1], ctr.cpu().numpy().astype(np.uint64), rt.ray_hits_status(st), off


def _collect(rt, tri, nod, root, count, rd, off_dev, capacity):
    """-> (HIT records [capacity] with untouched ones left as sentinel words, counts uint32[n], counters, status)"""
    import torch
    n = rd.shape[0]
    hits = torch.full(((capacity + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    rt.RayHitsCollect(tri, nod, root, count, rd, off_dev[:n + 1], hits, counts=cnt[:n], counters=ctr, status=st)
    torch.cuda.synchronize()
    h, c = hits.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert (h[capacity * 4:] == SENT).all(), "RayHitsCollect wrote past the last segment"
    assert (c[n:] == SENT).all(), "RayHitsCollect wrote counts past num_rays"
    return h[:capacity * 4].view(rh.HIT), c[:n], ctr.cpu().numpy().astype(np.uint64), rt.ray_hits_status(st)


def _hits(rt, tri, nod, root, count, rays):
    """count, then collect into exactly offsets[n] records.  Asserts what must hold on ANY tree: count and collect agree."""
    r = Result()
    rd = _dev_rays(rt, rays)
    n = len(rays)
    r.offsets, r.ctr_count, r.st_count, off = _count(rt, tri, nod, root, count, rd)
    assert r.offsets[0] == 0 and (np.diff(r.offsets) >= 0).all()
    total = int(r.offsets[n])
    recs, r.counts, r.ctr_collect, r.st_collect = _collect(rt, tri, nod, root, count, rd, off, total)
    assert (r.counts.astype(np.int64) == np.diff(r.offsets)).all(), "collect's counts differ from the differences of offsets"
    assert (recs.view(np.uint32).reshape(-1, 4) != SENT).any(1).all(), "a segment was not filled"
    assert (r.ctr_count == r.ctr_collect).all(), f"counters differ: count {r.ctr_count}, collect {r.ctr_collect}"
    assert r.ctr_count[2] == 0 and r.ctr_count[3] == 0
    assert r.st_count == r.st_collect and not (r.st_collect & rt.RT_RAY_HITS_TRUNCATED)
    r.rows = [recs[r.offsets[k]:r.offsets[k + 1]] for k in range(n)]
    return r


def _download(rt, inp):
    n = inp.num_triangles
    return rt.to_host(inp.nodes_out, rt.NODE, rt.NodesBytes(n) // 32), rt.to_host(inp.triangles_out, rt.TRIANGLE_PAIR, n)


def _closest(rt, g, rays):
    import torch
    inp, root, count = g
    hits = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
    rt.IntersectRays(inp.triangles_out, inp.nodes_out, root, count, _dev_rays(rt, rays), hits)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(rt.HIT).reshape(-1)


def _assert_rows_equal(rows, ref_rows, what):
    for k, (a, b) in enumerate(zip(rh.canon(rows), rh.canon(ref_rows))):
        assert a.shape == b.shape and (a == b).all(), f"{what}: ray {k}: {len(a)} records, the walk has {len(b)}"


class World:
    """scenes, their ray sets, built trees and, per (scene, tree), the device rows and the walk's rows -- computed once"""
    def __init__(self, rt, scenes):
        self.rt, self.scenes = rt, scenes
        self._sc, self._g, self._rows, self._b = {}, {}, {}, {}

    def scene(self, name):
        if name not in self._sc:
            tris = rs.scene_tris(name, self.scenes)
            self._sc[name] = tris, rh.ray_sets(tris, rh.SEEDS[name]).astype(self.rt.RAY)
        return self._sc[name]

    def gpu(self, name, tree):
        if (name, tree) not in self._g:
            self._g[name, tree] = _gpu_tree(self.rt, self.scene(name)[0], tree)
        return self._g[name, tree]

    def rows(self, name, tree):
        """-> (device Result, (walk rows, box tests, leaf visits))"""
        if (name, tree) not in self._rows:
            inp, root, count = self.gpu(name, tree)
            rays = self.scene(name)[1]
            nodes, leaves = _download(self.rt, inp)
            self._rows[name, tree] = (_hits(self.rt, inp.triangles_out, inp.nodes_out, root, count, rays),
                                      rh.walk(nodes, leaves, root, count, rays))
        return self._rows[name, tree]

    def brute(self, name):
        if name not in self._b:
            self._b[name] = rh.brute_f64(*self.scene(name))
        return self._b[name]


@pytest.fixture(scope="module")
def world(rt, scenes):
    return World(rt, scenes)


# ------------------------------------------------------------------ 1: rows against the walk
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_rows_equal_the_walk(world, name, tree):
    r, (ref_rows, box_tests, leaf_visits) = world.rows(name, tree)
    what = f"{name}/{tree}"
    assert r.st_count == 0, f"{what}: status {r.st_count}"
    assert (r.offsets == rh.offsets(ref_rows)).all(), f"{what}: offsets differ from the prefix sum of the walk's lengths"
    assert (r.counts == [len(x) for x in ref_rows]).all()
    _assert_rows_equal(r.rows, ref_rows, what)
    assert r.ctr_count[0] == box_tests and r.ctr_count[1] == leaf_visits, \
        f"{what}: counters {r.ctr_count[:2]}, the walk counts {box_tests}, {leaf_visits}"
    assert r.offsets[-1] >= len(ref_rows) // 8 and max(len(x) for x in ref_rows) >= 2, "the ray set is not trivial"
    print(f"{what}: {int(r.offsets[-1])} records, longest row {int(r.counts.max())}, box tests {int(r.ctr_count[0])}, "
          f"leaf visits {int(r.ctr_count[1])}")


# ------------------------------------------------------------------ 2: rows against float64
def _mt_f32_of(tris, rays, ray_idx, prim):
    """the kernel's float32 Moller-Trumbore of caller triangle `prim` for ray `ray_idx` (unrotated leaves): (t, u, v)"""
    T = tris.reshape(-1, 3, 3)[prim.astype(np.int64)]
    r = rays[ray_idx]
    _, t, u, v = rh.mt_f32(T[:, 0], T[:, 1], T[:, 2], r["origin"], r["dir"], r["tmin"], r["tmax"])
    return t, u, v


# (the fractal spans 2^-10 .. 2^45: its float32 products overflow, so float32 and float64 decisions differ by more than any
# margin there -- as in the ray-query tests it is held to the walk and to closest hit only)
@pytest.mark.parametrize("name", ("grid", "soup", "cornell"))
@pytest.mark.parametrize("tree", EXACT_TREES)
def test_rows_against_float64(world, name, tree):
    tris, rays = world.scene(name)
    b = world.brute(name)
    r, _ = world.rows(name, tree)
    n, nt = len(rays), tris.shape[0]
    got = np.zeros((n, nt), bool)
    ray_idx = np.repeat(np.arange(n), r.counts.astype(np.int64))
    recs = np.concatenate(r.rows)
    prim = recs["primitive_id"].astype(np.int64)
    assert (prim < nt).all()
    assert not got[ray_idx, prim].any() and len(np.unique(ray_idx * nt + prim)) == len(prim), "a triangle twice in a row"
    got[ray_idx, prim] = True
    missing = b["stable"] & b["accepted"] & ~got
    extra = b["stable"] & ~b["accepted"] & got
    assert not missing.any(), f"{name}/{tree}: {missing.sum()} stable accepted pairs are not in their row: {np.argwhere(missing)[:4]}"
    assert not extra.any(), f"{name}/{tree}: {extra.sum()} stable rejected pairs are in a row: {np.argwhere(extra)[:4]}"
    assert (b["stable"] & b["accepted"]).sum() > n // 8
    if "pairs" not in tree:
        t, u, v = _mt_f32_of(tris, rays, ray_idx, prim)
        for f, x in (("t", t), ("u", u), ("v", v)):
            assert (recs[f].view(np.uint32) == x.view(np.uint32)).all(), f"{name}/{tree}: {f} is not the kernel's own MT"


# ------------------------------------------------------------------ 3: the closest-hit relation
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_closest_hit_is_a_member(world, name, tree):
    rt = world.rt
    rays = world.scene(name)[1]
    r, _ = world.rows(name, tree)
    c = _closest(rt, world.gpu(name, tree), rays)
    hit = c["primitive_id"] != rt.MISS
    assert (hit == (r.counts > 0)).all(), f"{name}/{tree}: closest hit and the row disagree on {(hit != (r.counts > 0)).sum()} rays"
    assert hit.sum() > len(rays) // 8
    for k in np.nonzero(hit)[0]:
        row = r.rows[k]
        same = (row["t"].view(np.uint32) == c["t"][k:k + 1].view(np.uint32)) & \
               (row["u"].view(np.uint32) == c["u"][k:k + 1].view(np.uint32)) & \
               (row["v"].view(np.uint32) == c["v"][k:k + 1].view(np.uint32))
        assert same.any(), f"{name}/{tree}: ray {k}: the closest hit {c[k]} is not in the row {row}"
        with np.errstate(invalid="ignore"):
            assert np.isnan(c["t"][k]) or np.fmin.reduce(row["t"]) <= c["t"][k]


# ------------------------------------------------------------------ 4: dead rays, the empty tree
def test_dead_rays_and_the_empty_tree(world):
    import torch
    rt = world.rt
    rays = world.scene("grid")[1]
    inp, root, count = world.gpu("grid", "sah_pairs")
    cam = rt.to_device(world.scenes.camera_b(24))
    off_frame = torch.empty((rt.CameraRayCount(9, 9, 1, True), 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, 9, 9, off_frame, tiled=True)
    torch.cuda.synchronize()
    cam_rays = off_frame.cpu().numpy().view(rt.RAY).reshape(-1)
    off = cam_rays[cam_rays["tmax"] == -1][:1]
    assert len(off) == 1, "an edge tile has off-frame lanes"
    nan = F(np.nan)
    deg = rays[:9].copy()
    deg["tmin"][0], deg["tmax"][0] = 5.0, 1.0                 # tmin > tmax
    deg["origin"][1, 0] = nan
    deg["dir"][2, 1] = nan
    deg["tmin"][3] = nan
    deg["tmax"][4] = nan
    deg["dir"][5] = nan
    deg["origin"][6] = nan
    deg["tmin"][7], deg["tmax"][7] = 1e-5, 0.0
    deg[8] = off[0]
    assert not rh.live(deg).any()
    r = _hits(rt, inp.triangles_out, inp.nodes_out, root, count, deg)
    assert (r.offsets == 0).all() and (r.counts == 0).all() and (r.ctr_count == 0).all() and (r.ctr_collect == 0).all()
    # dead rays among live ones: their rows are empty, the others' rows are the batch's own
    mixed = rays[:300].copy()
    mixed[10:300:29] = deg[:10][np.arange(len(mixed[10:300:29])) % 9]
    full, _ = world.rows("grid", "sah_pairs")
    r = _hits(rt, inp.triangles_out, inp.nodes_out, root, count, mixed)
    dead = ~rh.live(mixed)
    assert dead.sum() == 10 and (r.counts[dead] == 0).all()
    _assert_rows_equal([x for x, d in zip(r.rows, dead) if not d], [x for x, d in zip(full.rows[:300], dead) if not d], "mixed")
    # an empty tree (count = 0): every row empty, nothing counted
    r = _hits(rt, inp.triangles_out, inp.nodes_out, 0, 0, rays[:300])
    assert (r.offsets == 0).all() and (r.ctr_count == 0).all() and r.st_count == 0


# ------------------------------------------------------------------ 5: batch ends
def test_batch_ends_and_sentinels(world):
    import torch
    rt = world.rt
    rays = world.scene("soup")[1]
    inp, root, count = world.gpu("soup", "hybrid_pairs")
    full, _ = world.rows("soup", "hybrid_pairs")
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        r = _hits(rt, inp.triangles_out, inp.nodes_out, root, count, rays[:n])         # (sentinels: checked inside)
        assert (r.offsets == full.offsets[:n + 1]).all(), f"batch of {n}"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r.rows, full.rows[:n])), f"batch of {n}: rows differ"
    # an empty batch still writes offsets[0] = 0, and nothing else
    off = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    empty = torch.empty((0, 8), dtype=torch.float32, device="cuda")
    assert rt.RayHitsCount(inp.triangles_out, inp.nodes_out, root, count, empty, off[:1]) == 0
    hits = torch.full((8, 4), 7.0, dtype=torch.float32, device="cuda")
    assert rt.RayHitsCollect(inp.triangles_out, inp.nodes_out, root, count, empty, off[:1], hits) == 0
    torch.cuda.synchronize()
    assert off.cpu().numpy().tolist() == [0, SENT, SENT, SENT] and bool((hits == 7.0).all())


# ------------------------------------------------------------------ 6: fixed K
def _quad_stack(layers=8):
    """parallel unit quads at z = 0 .. layers-1, two triangles each that share the diagonal (pairs merge them)"""
    tris = np.zeros((2 * layers, 3, 3), F)
    for k in range(layers):
        a, b, c, d = (0, 0, k), (1, 0, k), (1, 1, k), (0, 1, k)
        tris[2 * k], tris[2 * k + 1] = (a, b, c), (a, c, d)
    return np.ascontiguousarray(tris.reshape(-1, 9))


@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs"))
def test_fixed_k_truncation(rt, tree):
    import torch
    layers = 8
    tris = _quad_stack(layers)
    inp, root, count = _gpu_tree(rt, tris, tree)
    rng = np.random.default_rng(6)
    n = 300
    rays = np.zeros(n, rt.RAY)
    rays["origin"][:, :2] = rng.uniform(0.1, 0.9, (n, 2))
    rays["origin"][:, 2] = -1.0
    rays["dir"] = (0.003, -0.002, 1.0)
    rays["tmin"] = 0.0
    rays["tmax"] = rng.choice([1.5, 3.5, 4.5, 7.5, np.inf], n)            # rows of 1, 3, 4, 7 and 8 records
    full = _hits(rt, inp.triangles_out, inp.nodes_out, root, count, rays)
    assert full.counts.max() >= 6 and set(full.counts.tolist()) == {1, 3, 4, 7, 8}
    rd = _dev_rays(rt, rays)
    for K in (1, 2, 4):
        off = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
        recs, cnt, ctr, st = _collect(rt, inp.triangles_out, inp.nodes_out, root, count, rd, off, n * K)    # (sentinels behind)
        assert (cnt == full.counts).all(), "counts must be exact beyond the room"
        assert (ctr == full.ctr_count).all()
        assert bool(st & rt.RT_RAY_HITS_TRUNCATED) == bool((cnt > K).any()) and not (st & rt.RT_RAY_HITS_STACK_OVERFLOW)
        seg = recs.reshape(n, K)
        for k in range(n):
            m = min(int(cnt[k]), K)
            assert seg[k, :m].tobytes() == full.rows[k][:m].tobytes(), f"K {K}: ray {k}: not the head of the full row"
            assert (seg[k, m:].view(np.uint32) == SENT).all(), f"K {K}: ray {k} wrote past its records"
    # room everywhere: no flag
    K = int(full.counts.max())
    off = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
    _, _, _, st = _collect(rt, inp.triangles_out, inp.nodes_out, root, count, rd, off, n * K)
    assert st == 0
    # a segment with offsets[i+1] < offsets[i] gets nothing; its neighbours are served as usual
    K = 4
    o = np.arange(n + 1, dtype=np.int64) * K
    o[1::2] += 2 * K + 1                         # odd entries ahead of their successors: even rays get K+... room, odd rays none
    off = torch.from_numpy(o).cuda()
    cap = int(o.max()) + 16
    recs, cnt, _, st = _collect(rt, inp.triangles_out, inp.nodes_out, root, count, rd, off, cap)
    assert (cnt == full.counts).all() and st & rt.RT_RAY_HITS_TRUNCATED
    written = (recs.view(np.uint32).reshape(-1, 4) != SENT).any(1)
    expect = np.zeros(cap, bool)
    for k in range(n):
        room = max(int(o[k + 1] - o[k]), 0)
        m = min(int(cnt[k]), room)
        if k % 2 == 1:
            assert room == 0
        assert recs[o[k]:o[k] + m].tobytes() == full.rows[k][:m].tobytes()
        expect[o[k]:o[k] + m] = True
    assert (written == expect).all(), "a record outside the segments' rooms was written (or one inside was not)"


# ------------------------------------------------------------------ 7: parity on a closed mesh
def _box_mesh(lo, hi):
    """the 12 triangles of the box [lo, hi]: closed and convex"""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    c = np.array([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], F)
    quads = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    tris = [(c[a], c[b], c[cc]) for a, b, cc, d in quads] + [(c[a], c[cc], c[d]) for a, b, cc, d in quads]
    return np.ascontiguousarray(np.array(tris, F).reshape(-1, 9))


def test_parity_on_a_closed_mesh(rt):
    lo, hi = np.array((-0.7, -0.4, -0.9)), np.array((0.6, 0.8, 0.5))
    tris = _box_mesh(lo, hi)
    assert tris.shape[0] == 12
    rng = np.random.default_rng(12)
    cand = rng.uniform(-1.0, 1.0, (4000, 3))
    # signed distance bound: inside, the distance to the nearest face; outside, at least the largest face excess
    g = np.maximum(lo - cand, cand - hi).max(1)
    cand = cand[np.abs(g) >= 1e-2]
    d = np.array((0.577, 0.211, 0.789))
    d /= np.linalg.norm(d)
    rays = np.zeros(len(cand), rt.RAY)
    rays["origin"], rays["dir"], rays["tmin"], rays["tmax"] = cand, d, 0.0, np.inf
    b = rh.brute_f64(tris, rays)
    keep = np.nonzero(b["stable"].all(1))[0][:512]            # chosen by the reference alone
    assert len(keep) == 512
    rays, acc = rays[keep], b["accepted"][keep]
    inside = (np.maximum(lo - cand[keep], cand[keep] - hi).max(1) < 0)
    assert inside.sum() > 50 and (~inside).sum() > 50
    assert b["stable"][keep].all()
    assert ((acc.sum(1) % 2 == 1) == inside).all(), "the float64 reference itself: odd inside, even outside"
    for tree in EXACT_TREES:
        inp, root, count = _gpu_tree(rt, tris, tree)
        r = _hits(rt, inp.triangles_out, inp.nodes_out, root, count, rays)
        assert r.st_count == 0
        assert ((r.counts % 2 == 1) == inside).all(), f"{tree}: parity wrong on {(((r.counts % 2) == 1) != inside).sum()} points"
        assert (r.counts == acc.sum(1)).all()


# ------------------------------------------------------------------ 8: stack overflow
def _comb(rt, L, rng):
    """a comb of L two-slot nodes: node k = (box child k+1, leaf k) in slots (2k, 2k+1), the last node = (leaf L, leaf L-1).
    Every box spans [-50, 50]^3, so a ray that starts inside enters every slot: every node pushes its leaf and descends, and
    L entries are pending before the first pop.  Triangles: L + 1 large ones around the origin at radius 2 .. 8."""
    tris = np.zeros((L + 1, 3, 3), F)
    for k in range(L + 1):
        c = rng.normal(size=3)
        c /= np.linalg.norm(c)
        e1 = np.cross(c, (0.3, 0.5, 0.8))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(c, e1)
        r = 2.0 + k % 7
        tris[k] = (c * r - 2 * e1 - 2 * e2, c * r + 3 * e1 - 2 * e2, c * r - 2 * e1 + 3 * e2)
    nodes = np.zeros(2 * L, rt.NODE)
    for k in range(L):
        last = k == L - 1
        for s in (2 * k, 2 * k + 1):
            nodes["min"][s], nodes["max"][s] = (-50, -50, -50), (50, 50, 50)
        nodes["w12"][2 * k] = 1 << 29 if last else 2 << 29
        nodes["w28"][2 * k] = (2 << 29) | L if last else (1 << 29) | (2 * (k + 1))
        nodes["w12"][2 * k + 1] = 1 << 29
        nodes["w28"][2 * k + 1] = (2 << 29) | k
    leaves = np.zeros(L + 1, rt.TRIANGLE_PAIR)
    leaves["v0"], leaves["v1"], leaves["v2"], leaves["v3"] = tris[:, 0], tris[:, 1], tris[:, 2], tris[:, 2]
    leaves["primitive_id_0"] = np.arange(L + 1)
    return nodes, leaves


def test_stack_overflow_is_flagged_and_rows_are_subsets(rt):
    L = 80
    rng = np.random.default_rng(5)
    nodes, leaves = _comb(rt, L, rng)
    n = 70                                        # ends inside the second wave
    rays = np.zeros(n, rt.RAY)
    rays["origin"] = rng.uniform(-0.05, 0.05, (n, 3))
    rays["dir"] = rng.normal(size=(n, 3))
    rays["tmin"], rays["tmax"] = 0.0, np.inf
    ref_rows, box_tests, _ = rh.walk(nodes, leaves, 0, 2, rays)
    assert sum(len(x) for x in ref_rows) > n
    r = _hits(rt, rt.to_device(leaves), rt.to_device(nodes), 0, 2, rays)        # (count and collect agree: asserted inside)
    assert r.st_count & rt.RT_RAY_HITS_STACK_OVERFLOW and r.st_collect & rt.RT_RAY_HITS_STACK_OVERFLOW
    kept = np.concatenate([np.arange(64), [L]])  # the 64 kept pushes and the bottom leaf
    for k in range(n):
        got, ref = rh.canon([r.rows[k]])[0], rh.canon([ref_rows[k]])[0]
        assert np.isin(got, ref).all() and len(np.unique(got)) == len(got), f"ray {k}: not a subset of the walk's row"
        exp = ref_rows[k][np.isin(ref_rows[k]["primitive_id"], kept)]
        assert (got == rh.canon([exp])[0]).all()
    assert r.ctr_count[0] == box_tests == n * 2 * L and r.ctr_count[1] == n * 65


# ------------------------------------------------------------------ 9: refit
def _move(tris, t):
    """a smooth deformation applied per vertex: shared vertices stay shared (pairs stay pairs)"""
    v = tris.reshape(-1, 3).astype(np.float64)
    out = v.copy()
    out[:, 1] += 0.3 * np.sin(0.7 * v[:, 0] + t) * np.cos(0.5 * v[:, 2])
    out[:, 0] += 0.1 * np.cos(0.3 * v[:, 2] + t)
    return np.ascontiguousarray(out.astype(F).reshape(-1, 9))


@pytest.mark.parametrize("tree", ("bottom_up", "sah_pairs"))
def test_refit_then_rows_equal_the_walk(rt, scenes, tree):
    import torch
    tris = rs.scene_tris("grid", scenes)
    inp, root, count = _gpu_tree(rt, tris, tree)
    plan = rt.device_bytes(rt.RefitPlanBytes(inp.num_triangles))
    rt.BuildRefitPlan(inp, root, count, plan)
    moved = _move(tris, 1.0)
    inp.triangles_in.copy_(rt.to_device(moved))
    rt.Refit(inp, root, count, plan)
    torch.cuda.synchronize()
    assert rt.refit_status(plan, inp.num_triangles) == 0
    rays = rh.ray_sets(moved, 91).astype(rt.RAY)
    nodes, leaves = _download(rt, inp)
    ref_rows, box_tests, leaf_visits = rh.walk(nodes, leaves, root, count, rays)
    r = _hits(rt, inp.triangles_out, inp.nodes_out, root, count, rays)
    assert r.st_count == 0 and (r.offsets == rh.offsets(ref_rows)).all() and r.offsets[-1] > len(rays) // 4
    _assert_rows_equal(r.rows, ref_rows, f"refit {tree}")
    assert r.ctr_count[0] == box_tests and r.ctr_count[1] == leaf_visits


# ------------------------------------------------------------------ 10: hipGraph
def test_count_and_collect_in_a_hip_graph(world):
    import torch
    rt = world.rt
    all_rays = world.scene("grid")[1]
    inp, root, count = world.gpu("grid", "hybrid")
    n, K = 700, 24
    batches = [all_rays[:n], all_rays[1024:1024 + n], all_rays[300:300 + n]]
    rd = _dev_rays(rt, batches[0]).clone()
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    fixed = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
    hits = torch.empty((n * K, 4), dtype=torch.float32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    scratch = rt.device_bytes(rt.RayHitsScratchBytes(n))
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        hits.view(torch.int32).fill_(SENT)
        rt.RayHitsCount(inp.triangles_out, inp.nodes_out, root, count, rd, off, scratch=scratch, counters=ctr, status=st)
        rt.RayHitsCollect(inp.triangles_out, inp.nodes_out, root, count, rd, fixed, hits, counts=cnt, counters=ctr, status=st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()                       # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for rays in batches[1:]:
        rd.copy_(_dev_rays(rt, rays))
        for t in (off, cnt):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        direct = _hits(rt, inp.triangles_out, inp.nodes_out, root, count, rays)
        assert direct.counts.max() <= K and direct.offsets[-1] > n // 4
        assert (off.cpu().numpy() == direct.offsets).all() and (cnt.cpu().numpy().view(np.uint32) == direct.counts).all()
        seg = hits.cpu().numpy().view(rh.HIT).reshape(n, K)
        for k in range(n):
            m = int(direct.counts[k])
            assert seg[k, :m].tobytes() == direct.rows[k].tobytes(), f"replay: ray {k}"
            assert (seg[k, m:].view(np.uint32) == SENT).all()
        assert (ctr.cpu().numpy().astype(np.uint64) == 2 * direct.ctr_count).all() and int(st.item()) == 0


# ------------------------------------------------------------------ 11: the convenience call
@pytest.mark.parametrize("tree", ("sah_pairs", "sah_splits"))
def test_ray_hits_convenience_sorted(world, tree):
    import torch
    rt = world.rt
    rays = world.scene("soup")[1]
    inp, root, count = world.gpu("soup", tree)
    plain, _ = world.rows("soup", tree)
    rd = _dev_rays(rt, rays)
    off, hits = rt.RayHits(inp.triangles_out, inp.nodes_out, root, count, rd)
    assert off.dtype == torch.int64 and hits.dtype == torch.float32 and tuple(hits.shape) == (int(plain.offsets[-1]), 4)
    assert (off.cpu().numpy() == plain.offsets).all()
    assert hits.cpu().numpy().tobytes() == np.concatenate(plain.rows).tobytes()
    off, hits = rt.RayHits(inp.triangles_out, inp.nodes_out, root, count, rd, sort=True)
    o, h = off.cpu().numpy(), hits.cpu().numpy().view(rh.HIT).reshape(-1)
    assert (o == plain.offsets).all()
    rows = [h[o[k]:o[k + 1]] for k in range(len(rays))]
    _assert_rows_equal(rows, plain.rows, f"sorted {tree}")
    for k, row in enumerate(rows):
        key = list(zip(row["t"].tolist(), row["primitive_id"].tolist()))
        assert key == sorted(key), f"ray {k}: not ascending in (t, primitive_id): {key}"
    assert max(len(x) for x in rows) >= 3


# ------------------------------------------------------------------ the shared scan through a second caller
def test_count_scan_chunk_loop(rt):
    """1025 workgroups of rays: the scan over the block sums runs its chunk loop for RayHitsCount as for RangeCount
    (range_ref.py: the same four triangles, the same pattern).  A ray from (0.2, 0.2, 0) along +z with window
    [0, tmax] crosses the planes z = 1 .. 4 that lie below tmax = 0.5, 1.5 .. 4.5."""
    import range_ref as rr
    n = rr.SCAN_CHUNK_N[1]
    inp, root, count = _gpu_tree(rt, rr.scan_tiny_tris(), "bottom_up")
    rays = np.zeros(n, rh.RAY)
    rays["origin"], rays["dir"], rays["tmax"] = F([0.2, 0.2, 0.0]), F([0.0, 0.0, 1.0]), rr.scan_reach_pattern(n)
    counts = (F([1, 2, 3, 4])[None, :] <= rays["tmax"][:, None]).sum(axis=1)
    assert set(np.unique(counts)) == {0, 1, 2, 3, 4}
    offsets, _, status, _ = _count(rt, inp.triangles_out, inp.nodes_out, root, count, _dev_rays(rt, rays))
    exp = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    assert status == 0
    assert (offsets == exp).all(), f"first wrong offset at ray {int(np.argmax(offsets != exp))}"
