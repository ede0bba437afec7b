"""GPU tests of the instanced first-K ray query (rt_ray_first_hits_instanced; rt_abi.h, instanced first-K block; DESIGN section
30) on the two scenes of tests/ray_first_instanced_scene.py: three BLASes, 12 instances (three of them never entered), about
2,000 rays.  Both output buffers carry sentinels behind them (tests/ray_first_instanced_gpu.py).  The reference is
tests/ray_first_instanced_ref.py on the DEVICE's own bytes: the instanced all-hit walk with the gate of every item, from which E
(the row of a decided ray), the decided flag and the envelope (claims 1 and 3, which hold on every ray) follow with no kernel
involved.

1. main scene, k in {1, 2, 4, 32}, 3 TLAS kinds x 5 BLAS kinds: the undecided share of the reference alone is at most the cap
   (asserted before the kernel's rows are looked at); rows equal E bit for bit, 20 bytes an item, on decided rays (on split
   BLASes E comes from Ws); claims 1 and 3 on every ray;
2. k = 32, above the longest row: the rows are the sorted rows of rt_ray_hits_collect_instanced, GPU against GPU, and both
   counters equal rt_ray_hits_count_instanced's;
3. counters at most the all-hit ones for k in {1, 4};
4. k = 1 against rt_intersect_rays_instanced: on decided rays the first t is at most the closest-hit t; a closest-hit miss is a
   row of pads and the other way round;
5. an identity instance over each BLAS gives rt_ray_first_hits's row on that tree on rays decided for both, instance ids 0;
6. twins: every row that holds an item of instance 5 at t holds instance 6's at the same t right behind it, or ends there;
7. edge inputs: dead rays, num_instances = 0, an empty TLAS, all instances flagged, batch sizes 1, 63, 64, 65 and 257, 1 to 3
   instances, a window that excludes the first layers;
8. the Cornell-twins scene, the undecided case: claims 1 and 3 on every ray, claim 2 on its decided rays, an undecided share
   above zero at k = 1;
9. prepare -> TLAS build -> query captured in one HIP graph, replayed after the matrices were rewritten;
10. the call on a side stream behind work queued on the current one."""
import numpy as np
import pytest

import instance_ref as ir
import range_sets as rs
import ray_first_instanced_gpu as fg
import ray_first_instanced_ref as rfi
import ray_first_instanced_scene as fsc
import ray_first_ref as rf
import ray_hits_instanced_gpu as g
import ray_hits_ref as rh
import test_gpu_instances as tgi
import test_gpu_ray_first as tgf
from test_gpu_ray_queries import _gpu_tree

pytestmark = pytest.mark.gpu

TLAS_KINDS = ("bottom_up", "hybrid", "sah")
BLAS_KINDS = ("bottom_up", "pairs", "sah", "sah_pairs", "sah_splits")   # the instanced all-hit test's
KS = (1, 2, 4, 32)
F = np.float32
SENT = g.SENT


def _download(rt, inp):
    n = inp.num_triangles
    return rt.to_host(inp.triangles_out, rt.TRIANGLE_PAIR, n), rt.to_host(inp.nodes_out, rt.NODE, rt.NodesBytes(n) // 32)


class World:
    """the two scenes, their rays, built BLASes, framed scenes, per (scene, TLAS kind, BLAS kind) the reference and per k the
    device rows -- everything computed once"""

    def __init__(self, rt, scenes):
        self.rt = rt
        self.blas_tris = [rs.scene_tris(name, scenes) for name in fsc.BLAS_SCENES]
        self.inst = {"main": fsc.main_instances(self.blas_tris), "twins": fsc.twins_instances(self.blas_tris)}
        self.rays = {}
        for name, inst in self.inst.items():
            world, _, _ = ir.world_triangles(self.blas_tris, inst[:9])
            self.rays[name] = fsc.scene_rays(world).astype(rt.RAY)
        self._blas, self._scene, self._walk, self._rows, self._all = {}, {}, {}, {}, {}

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

    def scene(self, name, tlas_kind, blas_kind):
        key = name, tlas_kind, blas_kind
        if key not in self._scene:
            s = self.make(tlas_kind, blas_kind, self.inst[name])
            assert s.records["flags"].tolist() == [0] * 9 + [ir.SINGULAR, ir.BAD_BLAS, ir.BAD_BLAS]
            self._scene[key] = s
        return self._scene[key]

    def walk(self, name, tlas_kind, blas_kind):
        key = name, tlas_kind, blas_kind
        if key not in self._walk:
            self._walk[key] = fg.Walk(self.scene(*key), self.rays[name])
        return self._walk[key]

    def rows(self, name, tlas_kind, blas_kind, k):
        """-> (rows ITEM [n, k], counters, status) of the device"""
        key = name, tlas_kind, blas_kind, k
        if key not in self._rows:
            self._rows[key] = fg.first(self.rt, self.scene(name, tlas_kind, blas_kind).args, self.rays[name], k)
        return self._rows[key]

    def all_hits(self, name, tlas_kind, blas_kind):
        """rt_ray_hits_count_instanced + rt_ray_hits_collect_instanced on the same scene and rays"""
        key = name, tlas_kind, blas_kind
        if key not in self._all:
            self._all[key] = g.hits(self.rt, self.scene(*key).args, self.rays[name])
        return self._all[key]


@pytest.fixture(scope="module")
def world(rt, scenes):
    return World(rt, scenes)


# ------------------------------------------------------------------ 1: decided rays are E, every ray is inside the envelope
@pytest.mark.parametrize("blas_kind", BLAS_KINDS)
@pytest.mark.parametrize("tlas_kind", TLAS_KINDS)
def test_rows_against_the_gated_walk(world, tlas_kind, blas_kind):
    walk = world.walk("main", tlas_kind, blas_kind)
    what = f"main: TLAS {tlas_kind} / BLAS {blas_kind}"
    assert walk.nonempty > len(walk.rays) // 4 and 5 <= walk.longest < 32, "the ray set is not trivial"
    assert np.unique(np.concatenate(walk.rows)["instance"]).tolist() == list(range(9))
    for k in KS:
        share = walk.share(k)                        # of the device's own bytes, by the reference alone
        print(f"{what}: k {k}: {100 * share:.3f} % of {walk.nonempty} rays undecided")
        assert share <= rfi.CAP, f"{what}: k {k}: {100 * share:.2f} % undecided"
    for k in KS:
        rows, ctr, status = world.rows("main", tlas_kind, blas_kind, k)
        assert status == 0
        differ = fg.check_rows(rows, walk, k, what)
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits
        print(f"{what}: k {k}: {differ} rows differ from E, box tests {int(ctr[0])} of {walk.box_tests}, "
              f"leaf visits {int(ctr[1])} of {walk.leaf_visits}")


# ------------------------------------------------------------------ 2: k above the longest row, GPU against GPU
@pytest.mark.parametrize("tlas_kind,blas_kind", (("bottom_up", "sah_pairs"), ("hybrid", "sah"), ("sah", "pairs"),
                                                 ("sah", "bottom_up")))
def test_k_above_the_longest_row_is_the_sorted_collect_row(world, tlas_kind, blas_kind):
    k = 32
    allh = world.all_hits("main", tlas_kind, blas_kind)
    assert allh.st_count == 0 and 5 <= allh.counts.max() < k
    rows, ctr, status = world.rows("main", tlas_kind, blas_kind, k)
    assert status == 0
    for i, r in enumerate(allh.rows):
        want = rfi.pad_items(k)
        want[:len(r)] = rfi.sorted_row(r)
        assert rows[i].tobytes() == want.tobytes(), f"TLAS {tlas_kind} / BLAS {blas_kind}: ray {i}: {rows[i][:len(r) + 1]} != {want[:len(r) + 1]}"
    assert (ctr == allh.ctr_count).all(), f"counters {ctr}, rt_ray_hits_count_instanced's {allh.ctr_count}"


# ------------------------------------------------------------------ 3: the bound shrinks
@pytest.mark.parametrize("tlas_kind,blas_kind", (("bottom_up", "sah_splits"), ("hybrid", "pairs"), ("sah", "sah")))
def test_counters_are_at_most_the_all_hit_ones(world, tlas_kind, blas_kind):
    allh = world.all_hits("main", tlas_kind, blas_kind)
    for k in (1, 4):
        _, ctr, status = world.rows("main", tlas_kind, blas_kind, k)
        assert status == 0 and ctr[0] <= allh.ctr_count[0] and ctr[1] <= allh.ctr_count[1], f"k {k}: {ctr} vs {allh.ctr_count}"
        assert ctr[0] > 0 and ctr[1] > 0
    _, c1, _ = world.rows("main", tlas_kind, blas_kind, 1)
    assert c1[0] < allh.ctr_count[0], "k = 1 on rays with several layers must save box tests"


# ------------------------------------------------------------------ 4: k = 1 against closest hit
@pytest.mark.parametrize("blas_kind", BLAS_KINDS)
@pytest.mark.parametrize("tlas_kind", TLAS_KINDS)
def test_k1_against_closest_hit(world, tlas_kind, blas_kind):
    rt = world.rt
    s = world.scene("main", tlas_kind, blas_kind)
    walk = world.walk("main", tlas_kind, blas_kind)
    rows, _, status = world.rows("main", tlas_kind, blas_kind, 1)
    assert status == 0
    c, ids, _ = s.keep[0].run(world.rays["main"])
    hit = c["primitive_id"] != rt.MISS
    pads = rows["primitive_id"][:, 0] == rfi.MISS
    assert (hit == ~pads).all(), f"closest hit and the k = 1 row disagree on {(hit == pads).sum()} rays"
    assert rows[pads, 0].tobytes() == rfi.pad_items(int(pads.sum())).tobytes()
    decided = np.array([e[1] for e in walk.expected(1)], bool)
    sel = hit & decided
    assert sel.sum() > len(hit) // 8
    assert (rows["t"][sel, 0] <= c["t"][sel]).all()


# ------------------------------------------------------------------ 5: an identity instance
@pytest.mark.parametrize("which,blas_kind", ((0, "bottom_up"), (1, "sah_pairs"), (2, "pairs"), (1, "sah_splits")))
def test_identity_instance_equals_ray_first_hits(world, which, blas_kind):
    rt = world.rt
    entries, trees = world.blas(blas_kind)
    e = entries[which]
    leaves, nodes, root, count = trees[which]
    rays = rh.ray_sets(world.blas_tris[which], 11 + which, per_kind=160).astype(rt.RAY)
    for f in ("origin", "dir"):
        rays[f] = rays[f] + F(0)                         # no -0 component
    flat = tgf.Walk(nodes, leaves, root, count, rays)
    for tlas_kind in TLAS_KINDS:
        s = world.make(tlas_kind, blas_kind, ir.instance_array([np.eye(3, 4)], [which]))
        assert (s.records["world_to_object"] == np.eye(3, 4, dtype=F)).all() and s.records["flags"][0] == 0
        walk = fg.Walk(s, rays)
        for k in (1, 4):
            both = np.array([a[1] and b[1] for a, b in zip(walk.expected(k), flat.expected(k))], bool)
            assert both.mean() > 0.9
            want, _, st0 = tgf._first(rt, e[0], e[1], e[2], e[3], rays, k)
            rows, _, st1 = fg.first(rt, s.args, rays, k)
            what = f"identity over BLAS {which} ({blas_kind}), TLAS {tlas_kind}, k {k}"
            assert st0 == 0 and st1 == 0, what
            live = rows["primitive_id"] != rfi.MISS
            assert (rows["instance"][live] == 0).all() and (rows["instance"][~live] == rfi.MISS).all(), what
            got = np.ascontiguousarray(rows[["t", "primitive_id", "u", "v"]]).astype(rh.HIT)
            assert got[both].tobytes() == np.ascontiguousarray(want[both]).tobytes(), what
            assert live[:, 0].sum() > len(rays) // 4


# ------------------------------------------------------------------ 6: twins
@pytest.mark.parametrize("tlas_kind,blas_kind", (("bottom_up", "bottom_up"), ("hybrid", "sah_pairs"), ("sah", "sah_splits")))
def test_twins_report_side_by_side(world, tlas_kind, blas_kind):
    a, b = fsc.TWINS
    seen = 0
    for k in KS:
        rows, _, _ = world.rows("main", tlas_kind, blas_kind, k)
        for i, row in enumerate(rows):
            m = int((row["primitive_id"] != rfi.MISS).sum())
            assert not (row["instance"][:m] == b).any() or (row["instance"][:m] == a).any(), f"k {k}: ray {i}: twin {b} without {a}"
            for j in np.nonzero(row["instance"][:m] == a)[0]:
                seen += 1
                if j + 1 == m == k:
                    continue                             # the row is full and ends on the lower twin
                nxt = row[j + 1]
                assert j + 1 < m and nxt["instance"] == b and nxt["t"].tobytes() == row["t"][j].tobytes() and \
                    nxt["primitive_id"] == row["primitive_id"][j] and nxt["u"] == row["u"][j] and nxt["v"] == row["v"][j], \
                    f"k {k}: ray {i}: {row[j]} is not followed by its twin: {row[:m]}"
    assert seen > 50


# ------------------------------------------------------------------ 7: edge inputs
def _dead(rays):
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
    deg["tmin"][8], deg["tmax"][8] = 0.0, -1.0
    assert not rh.live(deg).any()
    return deg


def test_dead_rays(world):
    rt = world.rt
    k = 3
    s = world.scene("main", "bottom_up", "sah_pairs")
    rays = world.rays["main"]
    full, _, _ = fg.first(rt, s.args, rays[:300], k)
    deg = _dead(rays)
    rows, ctr, status = fg.first(rt, s.args, deg, k)
    assert rows.tobytes() == rfi.pad_items(9 * k).tobytes() and (ctr == 0).all() and status == 0
    mixed = rays[:300].copy()
    mixed[10:300:29] = deg[np.arange(len(mixed[10:300:29])) % 9]
    dead = ~rh.live(mixed)
    assert dead.sum() == 10
    rows, _, _ = fg.first(rt, s.args, mixed, k)
    assert rows[dead].tobytes() == rfi.pad_items(10 * k).tobytes()
    assert rows[~dead].tobytes() == full[~dead].tobytes()


def test_no_instances_empty_tlas_all_flagged(world):
    rt = world.rt
    k = 3
    s = world.scene("main", "sah", "bottom_up")
    rays = world.rays["main"][:600]
    # num_instances = 0 over the same TLAS: k pads for every ray, nothing counted
    none = g.Scene(rt, s.tlas_dev, s.tlas, s.records_dev, 0, None, 0, [], keep=(s,))
    rows, ctr, status = fg.first(rt, none.args, rays, k)
    assert rows.tobytes() == rfi.pad_items(600 * k).tobytes() and (ctr == 0).all() and status == 0
    # an empty TLAS (count 0, no arrays): the same
    rows, ctr, status = fg.first(rt, (None, None, 0, 0) + s.args[4:], rays, k)
    assert rows.tobytes() == rfi.pad_items(600 * k).tobytes() and (ctr == 0).all() and status == 0
    # every instance flagged (singular): the proxies are points at the origin, the TLAS is walked, nothing is entered
    flagged = world.make("bottom_up", "bottom_up", ir.instance_array([np.zeros((3, 4))] * 3, [0, 1, 2]))
    assert (flagged.records["flags"] == ir.SINGULAR).all()
    through = rays.copy()
    through["dir"] = -through["origin"]                   # through the origin, where the point proxies sit
    through["tmin"], through["tmax"] = 0.0, np.inf
    rows, ctr, status = fg.first(rt, flagged.args, through, k)
    walk = fg.Walk(flagged, through)
    assert rows.tobytes() == rfi.pad_items(600 * k).tobytes() and status == 0
    assert ctr[0] == walk.box_tests > 0 and ctr[1] == walk.leaf_visits == 0


def test_batch_ends(world):
    rt = world.rt
    s = world.scene("main", "hybrid", "pairs")
    rays = world.rays["main"]
    for k in (1, 3):
        full, _, _ = fg.first(rt, s.args, rays[:300], k)
        for n in (1, 63, 64, 65, 257):
            rows, _, _ = fg.first(rt, s.args, rays[:n], k)            # (sentinels: checked inside)
            assert rows.tobytes() == np.ascontiguousarray(full[:n]).tobytes(), f"batch of {n}, k {k}"


def test_empty_batch_runs_nothing(world):
    import torch
    rt = world.rt
    s = world.scene("main", "hybrid", "pairs")
    empty = torch.empty((0, 8), dtype=torch.float32, device="cuda")
    hits = torch.full((8, 2, 4), 7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((8, 2), 7, dtype=torch.int32, device="cuda")
    assert rt.RayFirstHitsInstanced(*s.args, empty, 2, hits[:0], ids[:0]) == 0
    torch.cuda.synchronize()
    assert bool((hits == 7.0).all()) and bool((ids == 7).all())


@pytest.mark.parametrize("n", (1, 2, 3))
@pytest.mark.parametrize("tlas_kind", TLAS_KINDS)
def test_few_instances(world, tlas_kind, n):
    rt = world.rt
    s = world.make(tlas_kind, "sah_pairs", world.inst["main"][[0, 4, 7][:n]])
    rays = world.rays["main"]
    walk = fg.Walk(s, rays)
    assert np.unique(np.concatenate(walk.rows)["instance"]).tolist() == list(range(n))
    for k in (1, 4):
        assert walk.share(k) <= rfi.CAP
        rows, ctr, status = fg.first(rt, s.args, rays, k)
        assert status == 0
        fg.check_rows(rows, walk, k, f"{n} instances, TLAS {tlas_kind}")
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits


def test_a_window_that_excludes_the_first_layers(world):
    """tmin between the second and the third distinct t of a ray's row: what lies in front is not reported, the rest is"""
    rt = world.rt
    s = world.scene("main", "sah", "sah_pairs")
    base = world.walk("main", "sah", "sah_pairs")
    picked, tmins = [], []
    for i, (ws, _) in enumerate(base.dedup):
        t = np.unique(ws["t"][np.isfinite(ws["t"])])
        if len(t) >= 4 and t[2] - t[1] > 1e-3 * max(1.0, abs(float(t[2]))):
            picked.append(i)
            tmins.append(F(0.5) * (t[1] + t[2]))
    assert len(picked) > 60
    rays = world.rays["main"][picked].copy()
    rays["tmin"] = np.array(tmins, F)
    assert rh.live(rays).all()
    walk = fg.Walk(s, rays)
    for k in (1, 2, 32):
        assert walk.share(k) <= rfi.CAP
        rows, _, status = fg.first(rt, s.args, rays, k)
        assert status == 0
        fg.check_rows(rows, walk, k, "window")
        assert (rows["primitive_id"][:, 0] != rfi.MISS).all() and (rows["t"][:, 0] >= rays["tmin"]).all()
        assert all(len(full[0]) > len(cut[0]) >= 2 for full, cut in zip([base.dedup[i] for i in picked], walk.dedup))


# ------------------------------------------------------------------ 8: the Cornell-twins scene
@pytest.mark.parametrize("tlas_kind,blas_kind", (("bottom_up", "bottom_up"), ("hybrid", "sah"), ("sah", "sah_pairs"),
                                                 ("sah", "sah_splits")))
def test_cornell_twins_scene_is_held_to_the_envelope(world, tlas_kind, blas_kind):
    walk = world.walk("twins", tlas_kind, blas_kind)
    what = f"twins: TLAS {tlas_kind} / BLAS {blas_kind}"
    share = walk.share(1)
    print(f"{what}: k 1: {100 * share:.3f} % of {walk.nonempty} rays undecided")
    assert share > 0, f"{what}: no undecided ray at k = 1: the envelope is not exercised"
    for k in KS:
        rows, ctr, status = world.rows("twins", tlas_kind, blas_kind, k)
        assert status == 0
        differ = fg.check_rows(rows, walk, k, what)                # claim 2 on decided rays, claims 1 and 3 on every ray
        assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits
        print(f"{what}: k {k}: {100 * walk.share(k):.3f} % undecided, {differ} rows differ from E")


# ------------------------------------------------------------------ 9: hipGraph
def test_prepare_build_and_query_in_a_hip_graph(world):
    import torch
    rt = world.rt
    k = 4
    entries, trees = world.blas("sah_pairs")
    inst0 = world.inst["main"]
    sc = tgi.Instanced(rt, entries, inst0, "bottom_up")
    rays = world.rays["main"][:900]
    n = len(rays)
    rd = g.dev_rays(rt, rays)
    hits = torch.empty((n, k, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty((n, k), dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        ctr.zero_()
        st.zero_()
        sc.frame()
        root, count = sc.root
        rt.RayFirstHitsInstanced(sc.tlas.triangles_out, sc.tlas.nodes_out, root, count, sc.records, sc.n, sc.table,
                                 len(sc.entries), rd, k, hits, ids, counters=ctr, status=st)

    moved = inst0.copy()
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
    seen = []
    for instances in (moved, inst0):
        sc.instances.copy_(rt.to_device(instances))                       # rewritten in place: the same buffer
        hits.view(torch.int32).fill_(SENT)
        ids.fill_(SENT)
        ctr.fill_(-1)
        sc.tlas.nodes_out.zero_()
        sc.records.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        got = rfi.items(ids.cpu().numpy().view(np.uint32).reshape(-1), hits.cpu().numpy().view(rh.HIT).reshape(-1)).reshape(n, k)
        got_ctr = ctr.cpu().numpy().astype(np.uint64)
        s = g.from_instanced(rt, sc, trees)
        walk = fg.Walk(s, rays)
        assert walk.share(k) <= rfi.CAP and int(st.item()) == 0
        fg.check_rows(got, walk, k, "replay")
        assert 0 < got_ctr[0] <= walk.box_tests and 0 < got_ctr[1] <= walk.leaf_visits
        eager, eager_ctr, _ = fg.first(rt, s.args, rays, k)
        assert got.tobytes() == eager.tobytes() and (got_ctr[:2] == eager_ctr).all()
        assert walk.nonempty > n // 4
        seen.append(got.tobytes())
    assert seen[0] != seen[1], "the moved scene must give other rows"


# ------------------------------------------------------------------ 10: a side stream
def test_on_a_side_stream_behind_queued_work(world):
    import torch
    rt = world.rt
    k = 4
    s = world.scene("main", "sah", "sah_splits")
    rays = world.rays["main"]
    want, want_ctr, _ = world.rows("main", "sah", "sah_splits", k)
    rd = g.dev_rays(rt, rays)
    n = len(rays)
    hits = torch.full((n, k, 4), 7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((n, k), 7, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())            # the rays are uploaded, the buffers filled
    busy = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")
    for _ in range(40):                                      # some milliseconds of work queued on the current stream
        busy = busy @ busy * 0.0 + 1.0
    assert rt.RayFirstHitsInstanced(*s.args, rd, k, hits, ids, counters=ctr, status=st, stream=side) == n
    side.synchronize()                                       # the side stream alone: the rows are complete
    got = rfi.items(ids.cpu().numpy().view(np.uint32).reshape(-1), hits.cpu().numpy().view(rh.HIT).reshape(-1)).reshape(n, k)
    torch.cuda.synchronize()
    assert got.tobytes() == want.tobytes()
    assert (ctr.cpu().numpy().astype(np.uint64)[:2] == want_ctr).all() and int(st.item()) == 0
    assert float(busy[0, 0]) == 1.0
