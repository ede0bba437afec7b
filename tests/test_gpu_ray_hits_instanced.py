"""GPU tests of the instanced all-hit ray queries (rt_ray_hits_count_instanced / rt_ray_hits_collect_instanced; rt_abi.h,
instanced all-hit block) on the scene of tests/test_ray_hits_instanced_ref_cpu.py: three BLASes, 12
instances (three of them never entered), about 2,000 rays (test_gpu_instances._world_rays plus ray_hits_ref.ray_sets on the
world triangles).  Every output buffer carries sentinels behind it (tests/ray_hits_instanced_gpu.py).

1. rows against the numpy walk on the device's own bytes, TLAS kinds x BLAS kinds: multisets of 20-byte items bit for bit,
   offsets, counts, both calls' counters equal to each other and to the walk's, counters[2:4] untouched;
2. composition, GPU against GPU: row i = the union over the walk's entered instances of rt_ray_hits_collect on that BLAS
   with the numpy object ray, tagged with the instance;
3. the closest-hit relation: rt_intersect_rays_instanced's (instance, t, u, v) is in the row; a miss there is an empty row;
4. an identity instance: rt_ray_hits_collect's rows on the BLAS, ids 0, the same leaf visits;
5. float64 brute force on the non-split BLAS kinds, stable pairs only (the reference's margin, fixed on the CPU);
6. edge inputs: dead rays, num_instances = 0, an empty TLAS, all instances flagged, batch sizes around a wave and a workgroup,
   1, 2 and 3 instances;
7. fixed K = 2: exact counts, written records a subset, RT_RAY_HITS_TRUNCATED iff a row is longer, nothing past a segment;
8. parity on closed meshes placed three times under rotation and mirror;
9. prepare + TLAS build + count + fixed-K collect captured in one HIP graph, replayed after the matrices were rewritten;
10. the convenience call RayHitsInstanced, plain and sorted."""
import numpy as np
import pytest

import instance_ref as ir
import range_sets as rs
import ray_hits_instanced_gpu as g
import ray_hits_instanced_ref as rhi
import ray_hits_instanced_scene as rsc
import ray_hits_ref as rh
import sdf_ref
import small_scenes as ss
import test_gpu_instances as tgi
import test_gpu_ray_hits as tgh
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

TLAS_KINDS = ("bottom_up", "hybrid", "sah")
BLAS_KINDS = ("bottom_up", "pairs", "sah", "sah_pairs", "sah_splits")
EXACT_BLAS_KINDS = BLAS_KINDS[:4]                 # every triangle in one leaf
F = np.float32
SENT = g.SENT


def _download(rt, inp):
    n = inp.num_triangles
    return rt.to_host(inp.triangles_out, rt.TRIANGLE_PAIR, n), rt.to_host(inp.nodes_out, rt.NODE, rt.NodesBytes(n) // 32)


class World:
    """the scene, its rays, built BLASes and framed scenes, and per (TLAS kind, BLAS kind) the device rows and the walk's rows
    -- everything computed once"""

    def __init__(self, rt, scenes):
        self.rt, self.scenes = rt, scenes
        self.blas_tris = [rs.scene_tris(name, scenes) for name in rsc.BLAS_SCENES]
        self.inst = rsc.scene_instances(self.blas_tris)
        self.world, self.inst_of, self.prim_of = ir.world_triangles(self.blas_tris, self.inst[:9])
        self.rays = rsc.scene_rays(self.world).astype(rt.RAY)
        self._blas, self._scene, self._rows, self._brute = {}, {}, {}, None

    def blas(self, kind):
        """-> (table entries, host trees) of the three BLASes built as `kind`, plus entry 3: an empty tree"""
        if kind not in self._blas:
            entries, trees, keep = [], [], []
            for tris in self.blas_tris:
                inp, root, count = _gpu_tree(self.rt, tris, kind)
                leaves, nodes = _download(self.rt, inp)
                entries.append((inp.triangles_out, inp.nodes_out, root, count))
                trees.append((leaves, nodes, root, count))
                keep.append(inp)
            entries.append((entries[0][0], entries[0][1], 0, 0))
            trees.append((trees[0][0], trees[0][1], 0, 0))
            self._blas[kind] = entries, trees, keep
        return self._blas[kind][:2]

    def make(self, tlas_kind, blas_kind, inst):
        entries, trees = self.blas(blas_kind)
        sc = tgi.Instanced(self.rt, entries, inst, tlas_kind)
        sc.frame()
        return g.from_instanced(self.rt, sc, trees)

    def scene(self, tlas_kind, blas_kind):
        if (tlas_kind, blas_kind) not in self._scene:
            s = self.make(tlas_kind, blas_kind, self.inst)
            assert self.rt.instance_status(s.keep[0].status) == self.rt.RT_INSTANCE_BAD_BLAS | self.rt.RT_INSTANCE_SINGULAR
            assert s.records["flags"].tolist() == [0] * 9 + [ir.SINGULAR, ir.BAD_BLAS, ir.BAD_BLAS]
            self._scene[tlas_kind, blas_kind] = s
        return self._scene[tlas_kind, blas_kind]

    def rows(self, tlas_kind, blas_kind):
        """-> (device Result, (walk rows, box tests, leaf visits))"""
        if (tlas_kind, blas_kind) not in self._rows:
            s = self.scene(tlas_kind, blas_kind)
            self._rows[tlas_kind, blas_kind] = g.hits(self.rt, s.args, self.rays), s.walk(self.rays)
        return self._rows[tlas_kind, blas_kind]

    def brute(self):
        if self._brute is None:
            self._brute = rhi.brute_f64(self.world, self.rays)
        return self._brute


@pytest.fixture(scope="module")
def world(rt, scenes):
    return World(rt, scenes)


# ------------------------------------------------------------------ 1: rows against the walk
@pytest.mark.parametrize("blas_kind", BLAS_KINDS)
@pytest.mark.parametrize("tlas_kind", TLAS_KINDS)
def test_rows_equal_the_walk(world, tlas_kind, blas_kind):
    r, ref = world.rows(tlas_kind, blas_kind)
    what = f"TLAS {tlas_kind} / BLAS {blas_kind}"
    g.check_against_walk(r, ref, what)
    assert (r.counts == [len(x) for x in ref[0]]).all()
    seen = np.unique(np.concatenate(r.rows)["instance"])
    assert seen.tolist() == list(range(9)), f"{what}: instances in the rows: {seen}"
    assert r.offsets[-1] >= len(world.rays) // 8 and r.counts.max() >= 4, "the ray set is not trivial"
    print(f"{what}: {int(r.offsets[-1])} records, longest row {int(r.counts.max())}, box tests {int(r.ctr_count[0])}, "
          f"leaf visits {int(r.ctr_count[1])}")


# ------------------------------------------------------------------ 2: composition, GPU against GPU
@pytest.mark.parametrize("tlas_kind,blas_kind", (("bottom_up", "sah_splits"), ("hybrid", "bottom_up"), ("sah", "pairs"),
                                                 ("sah", "sah_pairs")))
def test_composition_of_per_blas_rows(world, tlas_kind, blas_kind):
    rt = world.rt
    s = world.scene(tlas_kind, blas_kind)
    r, _ = world.rows(tlas_kind, blas_kind)
    ray, inst, _ = s.entered(world.rays)
    entries, _ = world.blas(blas_kind)
    exp = [[] for _ in world.rays]
    for k in np.unique(inst):
        sel = ray[inst == k]
        obj = ir.object_rays(world.rays[sel], s.records["world_to_object"][k])
        e = entries[int(s.records["blas"][k])]
        per = tgh._hits(rt, e[0], e[1], e[2], e[3], obj)          # rt_ray_hits_count + rt_ray_hits_collect on the BLAS
        assert per.st_count == 0
        for i, row in zip(sel, per.rows):
            exp[i].append(rhi.items(k, row))
    exp = [np.concatenate(x) if x else np.zeros(0, rhi.ITEM) for x in exp]
    rhi.assert_rows_equal(r.rows, exp, f"composition TLAS {tlas_kind} / BLAS {blas_kind}")
    assert len(np.unique(inst)) == 9 and sum(len(x) for x in exp) == int(r.offsets[-1])


# ------------------------------------------------------------------ 3: the closest-hit relation
@pytest.mark.parametrize("blas_kind", BLAS_KINDS)
@pytest.mark.parametrize("tlas_kind", TLAS_KINDS)
def test_closest_hit_is_a_member(world, tlas_kind, blas_kind):
    rt = world.rt
    s = world.scene(tlas_kind, blas_kind)
    r, _ = world.rows(tlas_kind, blas_kind)
    assert r.st_count == 0                               # no ray dropped a push
    c, ids, _ = s.keep[0].run(world.rays)
    hit = c["primitive_id"] != rt.MISS
    assert ((ids != rt.MISS) == hit).all()
    assert (hit == (r.counts > 0)).all(), f"closest hit and the row disagree on {(hit != (r.counts > 0)).sum()} rays"
    assert hit.sum() > len(world.rays) // 8
    for k in np.nonzero(hit)[0]:
        row = r.rows[k]
        same = (row["instance"] == ids[k]) & (row["t"].view(np.uint32) == c["t"][k:k + 1].view(np.uint32)) & \
               (row["u"].view(np.uint32) == c["u"][k:k + 1].view(np.uint32)) & \
               (row["v"].view(np.uint32) == c["v"][k:k + 1].view(np.uint32))
        assert same.any(), f"ray {k}: the closest hit {c[k]} in instance {ids[k]} is not in the row {row}"
        assert row["t"].min() <= c["t"][k]


# ------------------------------------------------------------------ 4: an identity instance
@pytest.mark.parametrize("which,blas_kind", ((0, "bottom_up"), (1, "sah_pairs"), (2, "pairs"), (1, "sah_splits")))
def test_identity_instance_equals_ray_hits(world, which, blas_kind):
    rt = world.rt
    entries, trees = world.blas(blas_kind)
    e = entries[which]
    rays = rh.ray_sets(world.blas_tris[which], 11 + which, per_kind=160).astype(rt.RAY)
    for f in ("origin", "dir"):
        rays[f] = rays[f] + F(0)                         # no -0 component
    assert not (np.signbit(rays["origin"]) & (rays["origin"] == 0)).any() and not (np.signbit(rays["dir"]) & (rays["dir"] == 0)).any()
    exp = tgh._hits(rt, e[0], e[1], e[2], e[3], rays)
    assert exp.offsets[-1] > len(rays) // 4
    for tlas_kind in TLAS_KINDS:
        s = world.make(tlas_kind, blas_kind, ir.instance_array([np.eye(3, 4)], [which]))
        assert (s.records["world_to_object"] == np.eye(3, 4, dtype=F)).all() and s.records["flags"][0] == 0
        r = g.hits(rt, s.args, rays)
        what = f"identity over BLAS {which} ({blas_kind}), TLAS {tlas_kind}"
        assert r.st_count == 0 and (r.offsets == exp.offsets).all(), what
        assert all((row["instance"] == 0).all() for row in r.rows), what
        rhi.assert_rows_equal(r.rows, [rhi.items(0, row) for row in exp.rows], what)
        assert r.ctr_count[1] == exp.ctr_count[1], f"{what}: leaf visits {r.ctr_count[1]} vs {exp.ctr_count[1]}"


# ------------------------------------------------------------------ 5: float64 on non-split BLASes
@pytest.mark.parametrize("blas_kind", EXACT_BLAS_KINDS)
@pytest.mark.parametrize("tlas_kind", TLAS_KINDS)
def test_rows_against_float64(world, tlas_kind, blas_kind):
    b = world.brute()
    r, _ = world.rows(tlas_kind, blas_kind)
    got, twice = rhi.got_matrix(r.rows, world.inst_of, world.prim_of, len(world.rays))
    assert not twice, "a placed triangle twice in a row"
    missing = b["stable"] & b["accepted"] & ~got
    extra = b["stable"] & ~b["accepted"] & got
    assert not missing.any(), f"{missing.sum()} stable accepted pairs are not in their row: {np.argwhere(missing)[:4]}"
    assert not extra.any(), f"{extra.sum()} stable rejected pairs are in a row: {np.argwhere(extra)[:4]}"
    assert (b["stable"] & b["accepted"]).sum() > len(world.rays) // 2


# ------------------------------------------------------------------ 6: edge inputs
def _dead(rays):
    nan = F(np.nan)
    deg = rays[:8].copy()
    deg["tmin"][0], deg["tmax"][0] = 5.0, 1.0                 # tmin > tmax
    deg["origin"][1, 0] = nan
    deg["dir"][2, 1] = nan
    deg["tmin"][3] = nan
    deg["tmax"][4] = nan
    deg["dir"][5] = nan
    deg["origin"][6] = nan
    deg["tmin"][7], deg["tmax"][7] = 1e-5, 0.0
    assert not rh.live(deg).any()
    return deg


def test_dead_rays(world):
    rt = world.rt
    s = world.scene("bottom_up", "sah_pairs")
    full, _ = world.rows("bottom_up", "sah_pairs")
    deg = _dead(world.rays)
    r = g.hits(rt, s.args, deg)
    assert (r.offsets == 0).all() and (r.counts == 0).all() and (r.ctr_count == 0).all() and r.st_count == 0
    mixed = world.rays[:300].copy()
    mixed[10:300:29] = deg[np.arange(len(mixed[10:300:29])) % 8]
    r = g.hits(rt, s.args, mixed)
    dead = ~rh.live(mixed)
    assert dead.sum() == 10 and (r.counts[dead] == 0).all()
    rhi.assert_rows_equal([x for x, d in zip(r.rows, dead) if not d], [x for x, d in zip(full.rows[:300], dead) if not d], "mixed")


def test_no_instances_empty_tlas_all_flagged(world):
    import torch
    rt = world.rt
    s = world.scene("sah", "bottom_up")
    rays = world.rays[:600]
    # num_instances = 0 over the same TLAS: no id is below it, nothing is entered; the TLAS's slots are still examined
    a = s.args
    none = g.Scene(rt, s.tlas_dev, s.tlas, s.records_dev, 0, None, 0, [], keep=(s,))
    r = g.hits(rt, none.args, rays)
    _, box_tests, leaf_visits = none.walk(rays)
    assert (r.offsets == 0).all() and r.ctr_count[0] == box_tests > 0 and r.ctr_count[1] == leaf_visits == 0 and r.st_count == 0
    # an empty TLAS (count 0, no arrays): nothing is examined
    empty = (None, None, 0, 0) + a[4:]
    r = g.hits(rt, empty, rays)
    assert (r.offsets == 0).all() and (r.ctr_count == 0).all() and r.st_count == 0
    # every instance flagged (singular): the proxies are points at the origin, the TLAS is walked, nothing is entered
    entries, trees = world.blas("bottom_up")
    flagged = world.make("bottom_up", "bottom_up", ir.instance_array([np.zeros((3, 4))] * 3, [0, 1, 2]))
    assert (flagged.records["flags"] == ir.SINGULAR).all()
    through = rays.copy()
    through["dir"] = -through["origin"]                   # through the origin, where the point proxies sit
    through["tmin"], through["tmax"] = 0.0, np.inf
    r = g.hits(rt, flagged.args, through)
    _, box_tests, _ = flagged.walk(through)
    assert (r.offsets == 0).all() and r.ctr_count[0] == box_tests > 0 and r.ctr_count[1] == 0
    torch.cuda.synchronize()


def test_batch_ends(world):
    rt = world.rt
    s = world.scene("hybrid", "pairs")
    full, _ = world.rows("hybrid", "pairs")
    for n in (1, 63, 64, 65, 255, 256, 257):
        r = g.hits(rt, s.args, world.rays[:n])                # (sentinels: checked inside)
        assert (r.offsets == full.offsets[:n + 1]).all(), f"batch of {n}"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r.rows, full.rows[:n])), f"batch of {n}: rows differ"


def test_empty_batch_runs_nothing(world):
    import torch
    rt = world.rt
    s = world.scene("hybrid", "pairs")
    off = torch.full((4,), SENT, dtype=torch.int64, device="cuda")
    empty = torch.empty((0, 8), dtype=torch.float32, device="cuda")
    hits = torch.full((8, 4), 7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    assert rt.RayHitsCountInstanced(*s.args, empty, off[:1]) == 0
    assert rt.RayHitsCollectInstanced(*s.args, empty, off[:1], hits, ids) == 0
    torch.cuda.synchronize()
    assert off.cpu().numpy().tolist() == [SENT] * 4 and bool((hits == 7.0).all()) and bool((ids == 7).all())
    o, h, i = rt.RayHitsInstanced(*s.args, empty)
    assert o.cpu().numpy().tolist() == [0] and tuple(h.shape) == (0, 4) and tuple(i.shape) == (0,)


@pytest.mark.parametrize("n", (1, 2, 3))
@pytest.mark.parametrize("tlas_kind", TLAS_KINDS)
def test_few_instances(world, tlas_kind, n):
    rt = world.rt
    s = world.make(tlas_kind, "sah_pairs", world.inst[[0, 4, 7][:n]])
    rays = world.rays
    r = g.hits(rt, s.args, rays)
    g.check_against_walk(r, s.walk(rays), f"{n} instances, TLAS {tlas_kind}")
    assert np.unique(np.concatenate(r.rows)["instance"]).tolist() == list(range(n))


# ------------------------------------------------------------------ 7: fixed K
def test_fixed_k(world):
    import torch
    rt = world.rt
    K = 2
    s = world.scene("bottom_up", "sah")
    full, _ = world.rows("bottom_up", "sah")
    n = len(world.rays)
    assert (full.counts > K).any() and (full.counts == K).any() and (full.counts < K).any()
    rd = g.dev_rays(rt, world.rays)
    off = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
    recs, cnt, ctr, st = g.collect(rt, s.args, rd, off, n * K)          # (sentinels behind: checked inside)
    assert (cnt == full.counts).all(), "counts must be exact beyond the room"
    assert (ctr == full.ctr_count).all()
    assert st == rt.RT_RAY_HITS_TRUNCATED
    seg = recs.reshape(n, K)
    for k in range(n):
        m = min(int(cnt[k]), K)
        assert (seg[k, :m]["instance"] != SENT).all() and rhi.is_subset(seg[k, :m], full.rows[k]), f"ray {k}: not of the exact row"
        assert (seg[k, m:]["instance"] == SENT).all() and (seg[k, m:]["primitive_id"] == SENT).all(), f"ray {k} wrote past its records"
    # no row longer than K: no flag
    short = np.nonzero(full.counts <= K)[0]
    rd = g.dev_rays(rt, world.rays[short])
    off = (torch.arange(len(short) + 1, dtype=torch.int64) * K).cuda()
    recs, cnt, _, st = g.collect(rt, s.args, rd, off, len(short) * K)
    assert st == 0 and (cnt == full.counts[short]).all() and cnt.max() == K
    seg = recs.reshape(len(short), K)
    for j, k in enumerate(short):
        rhi.assert_rows_equal([seg[j, :int(cnt[j])]], [full.rows[k]], f"short ray {k}")


# ------------------------------------------------------------------ 8: parity on placed closed meshes
def _inside_object(name, p):
    if name == "tetra":
        return ss.in_tetra(p)
    return ((p > sdf_ref.BOX_LO) & (p < sdf_ref.BOX_HI)).all(axis=1)


@pytest.mark.parametrize("name", ss.CLOSED)
def test_parity_on_placed_closed_meshes(rt, scenes, name):
    tris = np.array(ss.tris(name, scenes))
    cen = tris.reshape(-1, 3).astype(np.float64).mean(axis=0)
    R1, R2 = ir.rotation(0.4, -0.8, 0.3), ir.rotation(-1.0, 0.5, 0.7)
    mirror = np.diag([1.0, -1.0, 1.0])
    lin = [R1, mirror, R2 @ mirror * 1.25]
    at = [(-2.5, 0.0, 0.0), (0.0, 0.3, 0.0), (2.5, -0.2, 0.4)]            # apart: the placed boxes do not touch
    mats = [np.hstack([A, (np.asarray(t) - A @ cen).reshape(3, 1)]) for A, t in zip(lin, at)]
    inst = ir.instance_array(mats, [0, 0, 0])
    world_tris, inst_of, prim_of = ir.world_triangles([tris], inst)
    rng = np.random.default_rng(ss.SEED[name])
    ext = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    o = np.concatenate([np.asarray(t) + rng.uniform(-0.5 * ext, 0.5 * ext, (500, 3)) for t in at])
    d = rng.normal(size=o.shape)
    rays = np.zeros(len(o), rt.RAY)
    rays["origin"], rays["dir"], rays["tmin"], rays["tmax"] = o, d, 0.0, np.inf
    b = rhi.brute_f64(world_tris, rays)
    keep = np.nonzero(b["stable"].all(1))[0]                           # chosen by the reference alone
    assert len(keep) > 1200
    rays, acc = rays[keep], b["accepted"][keep]
    inside = np.zeros((len(rays), 3), bool)
    for k, M in enumerate(inst["object_to_world"].astype(np.float64)):
        W = np.linalg.inv(M[:, :3])
        inside[:, k] = _inside_object(name, (rays["origin"].astype(np.float64) - M[:, 3]) @ W.T)
    par = np.stack([acc[:, inst_of == k].sum(1) % 2 == 1 for k in range(3)], axis=1)
    assert (par == inside).all(), "the float64 reference itself: odd inside, even outside, per placed copy"
    assert (inside.sum(0) > 20).all() and (~inside).sum() > 100 and inside.sum(1).max() == 1
    for blas_kind in ("bottom_up", "sah_pairs"):
        inp, root, count = _gpu_tree(rt, tris, blas_kind)
        leaves, nodes = _download(rt, inp)
        for tlas_kind in ("bottom_up", "sah"):
            sc = tgi.Instanced(rt, [(inp.triangles_out, inp.nodes_out, root, count)], inst, tlas_kind)
            sc.frame()
            assert rt.instance_status(sc.status) == 0
            s = g.from_instanced(rt, sc, [(leaves, nodes, root, count)])
            r = g.hits(rt, s.args, rays)
            assert r.st_count == 0
            got = np.stack([[int((row["instance"] == k).sum()) for k in range(3)] for row in r.rows])
            assert ((got % 2 == 1) == inside).all(), f"{name} {blas_kind}/{tlas_kind}: parity wrong on {((got % 2 == 1) != inside).sum()}"
            assert (got == np.stack([acc[:, inst_of == k].sum(1) for k in range(3)], axis=1)).all()


# ------------------------------------------------------------------ 9: hipGraph
def test_prepare_build_count_and_collect_in_a_hip_graph(world):
    import torch
    rt = world.rt
    K = 6
    entries, trees = world.blas("sah_pairs")
    sc = tgi.Instanced(rt, entries, world.inst, "bottom_up")
    rays = world.rays[:900]
    n = len(rays)
    rd = g.dev_rays(rt, rays)
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    fixed = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
    hits = torch.empty((n * K, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(n * K, dtype=torch.int32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    scratch = rt.device_bytes(rt.RayHitsScratchBytes(n))
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        hits.view(torch.int32).fill_(SENT)
        ids.fill_(SENT)
        sc.frame()
        root, count = sc.root
        a = (sc.tlas.triangles_out, sc.tlas.nodes_out, root, count, sc.records, sc.n, sc.table, len(sc.entries))
        rt.RayHitsCountInstanced(*a, rd, off, scratch=scratch, counters=ctr, status=st)
        rt.RayHitsCollectInstanced(*a, rd, fixed, hits, ids, counts=cnt, counters=ctr, status=st)

    moved = world.inst.copy()
    moved["object_to_world"][:9, :, 3] += F(0.07) * (1 + np.arange(9, dtype=F))[:, None]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()                       # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    totals = []
    for instances in (moved, world.inst):
        sc.instances.copy_(rt.to_device(instances))                       # rewritten in place: the same buffer
        for t in (off, cnt):
            t.fill_(-7)
        sc.tlas.nodes_out.zero_()
        sc.records.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        s = g.from_instanced(rt, sc, trees)
        ref_rows, box_tests, leaf_visits = s.walk(rays)
        lens = np.array([len(x) for x in ref_rows])
        assert (off.cpu().numpy() == rhi.offsets(ref_rows)).all() and (cnt.cpu().numpy().view(np.uint32) == lens).all()
        seg = rhi.items(ids.cpu().numpy().view(np.uint32), hits.cpu().numpy().view(rh.HIT).reshape(-1)).reshape(n, K)
        for k in range(n):
            m = min(int(lens[k]), K)
            if lens[k] <= K:
                rhi.assert_rows_equal([seg[k, :m]], [ref_rows[k]], f"replay: ray {k}")
            else:
                assert rhi.is_subset(seg[k, :m], ref_rows[k]), f"replay: ray {k}"
            assert (seg[k, m:]["instance"] == SENT).all()
        assert (ctr.cpu().numpy().astype(np.uint64)[:2] == 2 * np.array([box_tests, leaf_visits], np.uint64)).all()
        assert int(st.item()) == (rt.RT_RAY_HITS_TRUNCATED if (lens > K).any() else 0)
        totals.append(int(lens.sum()))
        assert lens.sum() > n // 4 and (lens <= K).mean() > 0.9
    assert totals[0] != totals[1], "the moved scene must give other rows"


# ------------------------------------------------------------------ 10: the convenience call
def test_ray_hits_instanced_convenience_sorted(world):
    import torch
    rt = world.rt
    s = world.scene("sah", "sah_splits")
    plain, _ = world.rows("sah", "sah_splits")
    rd = g.dev_rays(rt, world.rays)
    off, hits, ids = rt.RayHitsInstanced(*s.args, rd)
    assert off.dtype == torch.int64 and hits.dtype == torch.float32 and ids.dtype == torch.int32
    assert tuple(hits.shape) == (int(plain.offsets[-1]), 4) and tuple(ids.shape) == (int(plain.offsets[-1]),)
    assert (off.cpu().numpy() == plain.offsets).all()
    got = rhi.items(ids.cpu().numpy().view(np.uint32), hits.cpu().numpy().view(rh.HIT).reshape(-1))
    assert got.tobytes() == np.concatenate(plain.rows).tobytes()
    off, hits, ids = rt.RayHitsInstanced(*s.args, rd, sort=True)
    o = off.cpu().numpy()
    got = rhi.items(ids.cpu().numpy().view(np.uint32), hits.cpu().numpy().view(rh.HIT).reshape(-1))
    assert (o == plain.offsets).all()
    rows = [got[o[k]:o[k + 1]] for k in range(len(world.rays))]
    rhi.assert_rows_equal(rows, plain.rows, "sorted")
    for k, row in enumerate(rows):
        key = list(zip(row["t"].tolist(), row["instance"].tolist(), row["primitive_id"].tolist()))
        assert key == sorted(key), f"ray {k}: not ascending in (t, instance, primitive_id): {key}"
    assert max(len(x) for x in rows) >= 4


def test_ray_hits_instanced_on_a_side_stream(world):
    """the convenience call with stream=: everything it launches, torch's own work included, goes to that stream -- nothing of it
    may sit on the current stream behind work that is still queued there and land after the count and collect"""
    import torch
    rt = world.rt
    s = world.scene("sah", "sah_splits")
    plain, _ = world.rows("sah", "sah_splits")
    rd = g.dev_rays(rt, world.rays)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())            # the rays are uploaded
    busy = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
    for _ in range(40):                                      # some milliseconds of work queued on the current stream
        busy = busy @ busy * 0.0 + 1.0
    off, hits, ids = rt.RayHitsInstanced(*s.args, rd, stream=side)
    side.synchronize()
    o = off.cpu().numpy()                                    # (this copy waits for the current stream too)
    torch.cuda.synchronize()
    assert (o == plain.offsets).all() and (off.cpu().numpy() == plain.offsets).all(), "offsets were overwritten off the stream"
    got = rhi.items(ids.cpu().numpy().view(np.uint32), hits.cpu().numpy().view(rh.HIT).reshape(-1))
    assert got.tobytes() == np.concatenate(plain.rows).tobytes()
    assert float(busy[0, 0]) == 1.0
