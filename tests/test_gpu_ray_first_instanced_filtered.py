"""GPU tests of the filtered instanced first-K ray query (rt_ray_first_hits_instanced_filtered; rt_abi.h, instanced set-filter
block) on the main scene of tests/ray_first_instanced_scene.py: device-built LBVH and SAH BLASes, 12 instances
(three of them never entered), the device's own records, about 2,000 rays.  Both output buffers carry sentinels behind them
(tests/instance_set_filter_gpu.py).  The reference is tests/instance_set_filter_ref.py on the DEVICE's own bytes: the FILTERED
instanced all-hit walk with the gate of every item, from which E (the row of a decided ray), the decided flag and the envelope
(claims 1 and 3, which hold on every ray) follow with no kernel involved.

1. k in {1, 4, 32} x arms: on every decided ray the row is the head of the filtered W bit for bit in all 20 bytes, claims 1 and
   3 on every ray, claim 4 against rt_ray_hits_count_instanced_filtered under the same filter (equal above the longest row);
2. contract (a): both keep-all forms and filter = NULL give the unfiltered sibling's rows, counters and status byte for byte;
3. a ray whose nearest crossing is rejected by cull, by skip and by mask in turn: the row starts at the nearest KEPT crossing,
   which lies beyond the rejected one (the bound did not shrink on it), and k = 1 equals rt_intersect_rays_instanced_filtered;
4. contract (c): k = 1 on decided rays is at most the filtered closest-hit t; a miss there is a row of pads and back;
5. contract (d): masks that admit no instance: rows of pads, no leaf visit, exactly the TLAS slots examined;
6. contract (e): one identity instance equals rt_ray_first_hits_filtered on the BLAS with {mask, skip_id};
7. the twins: skipping (5, id) leaves (6, id) at the same t; the mirror: CULL_BACK rows hold no world-space back face of it;
8. per_instance shorter than num_instances; a null per_instance with num_instance_filters > 0;
9. one linear hipGraph capture of the call, replayed twice: rows equal to the eager call."""
import numpy as np
import pytest

import instance_filter_ref as ifr
import instance_ref as ir
import instance_set_filter_gpu as ig
import instance_set_filter_ref as isf
import instance_set_filter_scene as fsc
import ray_filter_ref as rx
import ray_first_instanced_gpu as fg
import ray_first_instanced_ref as rfi
import ray_hits_instanced_gpu as g
import ray_hits_ref as rh
import test_gpu_ray_filter as tgr
from test_gpu_instance_filter import _run as closest_filtered
from test_gpu_ray_first_instanced import World
from test_gpu_ray_hits_instanced_filtered import Tree, _facing

pytestmark = pytest.mark.gpu

F = np.float32
SENT = g.SENT
COMBOS = (("bottom_up", "bottom_up"), ("sah", "sah_pairs"), ("hybrid", "sah_splits"))     # (TLAS kind, BLAS kind)
KS = (1, 4, 32)
ARMS = ("cull_back", "cull_disable", "masks", "skip", "half")


class FWorld(World):
    """test_gpu_ray_first_instanced.World (the main scene, its rays, the unfiltered reference and rows) plus, per (combo, arm),
    the ray set, the filter and the reference -- everything computed once"""

    def __init__(self, rt, scenes):
        super().__init__(rt, scenes)
        self._arm, self._fwalk, self._frows = {}, {}, {}
        self.world_tris, self.inst_of, self.prim_of = ir.world_triangles(self.blas_tris, self.inst["main"][:9])
        self.world = self.world_tris

    def arm(self, combo, name):
        """-> (rays, host filter)"""
        if (combo, name) not in self._arm:
            rays = self.rays["main"]
            n, num = len(rays), self.inst["main"].size
            if name == "skip":
                b, per_ray = fsc.bounce(rays, self.walk("main", *combo).rows)
                out = b.astype(self.rt.RAY), fsc.skip_filter(per_ray)
            elif name == "half":
                out = rays, fsc.half_masked(num)
            elif name == "none":
                out = rays, fsc.none_admitted(num)
            else:
                out = rays, fsc.arm(name, num, n)
            self._arm[combo, name] = out
        return self._arm[combo, name]

    def fwalk(self, combo, name):
        if (combo, name) not in self._fwalk:
            rays, flt = self.arm(combo, name)
            self._fwalk[combo, name] = ig.Walk(self.scene("main", *combo), rays, flt)
        return self._fwalk[combo, name]

    def frows(self, combo, name, k):
        if (combo, name, k) not in self._frows:
            rays, flt = self.arm(combo, name)
            self._frows[combo, name, k] = ig.first(self.rt, self.scene("main", *combo).args, rays, k, ig.dev_filter(self.rt, flt))
        return self._frows[combo, name, k]


@pytest.fixture(scope="module")
def world(rt, scenes):
    return FWorld(rt, scenes)


# ------------------------------------------------------------------ 1: decided rays are E, every ray is inside the envelope
@pytest.mark.parametrize("name", ARMS)
@pytest.mark.parametrize("combo", COMBOS)
def test_rows_against_the_filtered_gated_walk(world, combo, name):
    rt = world.rt
    walk = world.fwalk(combo, name)
    rays, flt = world.arm(combo, name)
    what = f"TLAS {combo[0]} / BLAS {combo[1]} / {name}"
    assert walk.nonempty > len(rays) // 8 and walk.longest < 32, "the ray set is not trivial"
    allh = ig.hits(rt, world.scene("main", *combo).args, rays, ig.dev_filter(rt, flt))
    ig.check_hits(allh, walk, what)
    for k in KS:
        share = walk.share(k)                        # of the device's own bytes, by the reference alone
        print(f"{what}: k {k}: {100 * share:.3f} % of {walk.nonempty} rays undecided")
        assert share < 0.5, f"{what}: k {k}: most rays are undecided: the bit-for-bit check would hold on too few"
        rows, ctr, status = world.frows(combo, name, k)
        assert status == 0
        differ = fg.check_rows(rows, walk, k, what)  # claim 2 on decided rays, claims 1 and 3 on every ray
        # claim 4, against rt_ray_hits_count_instanced_filtered under the same filter
        assert ctr[0] <= allh.ctr_count[0] and ctr[1] <= allh.ctr_count[1], f"{what}: k {k}: {ctr} vs {allh.ctr_count}"
        if k > walk.longest:
            assert (ctr == allh.ctr_count).all(), f"{what}: k {k} above the longest row: {ctr} vs {allh.ctr_count}"
            # (a split BLAS repeats a triangle once per reference reached in the all-hit row; the list holds it once)
            for i, r in enumerate(allh.rows if "splits" not in combo[1] else ()):
                want = rfi.pad_items(k)
                want[:len(r)] = rfi.sorted_row(r)
                assert rows[i].tobytes() == want.tobytes(), f"{what}: ray {i}: not the sorted filtered all-hit row"
        print(f"{what}: k {k}: {differ} rows differ from E, box tests {int(ctr[0])} of {int(allh.ctr_count[0])}")


# ------------------------------------------------------------------ 2: (a) keep-all
@pytest.mark.parametrize("combo", COMBOS)
def test_keep_all_is_the_unfiltered_call(world, combo):
    rt = world.rt
    s = world.scene("main", *combo)
    rays = world.rays["main"]
    for k in (1, 4):
        want, want_ctr, want_st = world.rows("main", *combo, k)
        for what, flt in (("null arrays", isf.keep_all()), ("all-ones arrays", isf.keep_all(len(rays), 12)), ("NULL", None)):
            rows, ctr, st = ig.first(rt, s.args, rays, k, ig.dev_filter(rt, flt))
            assert rows.tobytes() == want.tobytes(), f"{combo}: k {k}: {what}: rows differ from the unfiltered call's"
            assert ctr.tobytes() == want_ctr.tobytes() and st == want_st == 0, f"{combo}: k {k}: {what}"


# ------------------------------------------------------------------ 3: the nearest crossing rejected
def _rejecting_filters(world, combo):
    """per way of rejecting -> (filter, bool [n]: rays whose nearest unfiltered crossing it rejects by that way)"""
    rays = world.rays["main"]
    n, num = len(rays), world.inst["main"].size
    base = world.walk("main", *combo)
    near = fsc.nearest_items(base.rows)
    has = np.array([it is not None for it in near])
    out = {}
    # skip: the nearest (instance, primitive) itself
    out["skip"] = fsc.skip_filter(fsc.skip_nearest(base.rows)), has.copy()
    # mask: per-ray masks that leave out the group (instance % 3) of the nearest crossing's instance
    per_ray = np.zeros(n, ifr.INSTANCE_RAY_FILTER)
    per_ray["skip_instance"], per_ray["skip_id"] = isf.MISS, isf.MISS
    group = np.array([int(it["instance"]) % 3 if it is not None else 0 for it in near])
    per_ray["mask"] = 7 & ~(1 << group)
    im = (np.uint32(1) << (np.arange(num, dtype=np.uint32) % 3)).astype(np.uint32)
    out["mask"] = ifr.InstanceFilter(0, 0, ifr.instance_filters(num, masks=im), per_ray), has.copy()
    # cull: CULL_BACK; the rays whose nearest crossing the reference's CULL_BACK walk does not keep
    flt = ifr.InstanceFilter(ifr.CULL_BACK)
    kept = ig.Walk(world.scene("main", *combo), rays, flt)
    gone = np.zeros(n, bool)
    for i, it in enumerate(near):
        if it is not None:
            gone[i] = not ((kept.rows[i]["instance"] == it["instance"]) & (kept.rows[i]["primitive_id"] == it["primitive_id"])).any()
    out["cull"] = flt, gone
    return out, near


@pytest.mark.parametrize("combo", COMBOS)
def test_nearest_crossing_rejected_by_cull_skip_and_mask(world, combo):
    rt = world.rt
    s = world.scene("main", *combo)
    rays = world.rays["main"]
    filters, near = _rejecting_filters(world, combo)
    for way, (flt, rejected) in filters.items():
        walk = ig.Walk(s, rays, flt)
        hf = ig.dev_filter(rt, flt)
        exp = walk.expected(1)
        rows, _, status = ig.first(rt, s.args, rays, 1, hf)
        assert status == 0
        fg.check_rows(rows, walk, 1, f"{combo}: nearest rejected by {way}")
        c, ids, _ = closest_filtered(s.keep[0], rays, flt)
        beyond = 0
        for i in np.nonzero(rejected)[0]:
            E, decided, _ = exp[i]
            first = rows[i, 0]
            gone = near[i]
            assert not (first["instance"] == gone["instance"] and first["primitive_id"] == gone["primitive_id"]), \
                f"{way}: ray {i}: the rejected crossing {gone} is in the row"
            if not decided:
                continue
            if len(E) == 0:
                assert first["primitive_id"] == rfi.MISS and c["primitive_id"][i] == rt.MISS
                continue
            # the nearest KEPT crossing: the head of the reference, and the filtered closest hit's bits
            assert first.tobytes() == E[0].tobytes(), f"{way}: ray {i}: {first} is not the nearest kept crossing {E[0]}"
            # (the t alone: among crossings at one t the closest-hit query keeps the first it meets, this one the lowest key)
            assert first["t"].tobytes() == c["t"][i].tobytes(), f"{way}: ray {i}: k = 1 {first} vs the filtered closest hit {c[i]}"
            if first["t"] > gone["t"]:
                beyond += 1                              # found beyond the rejected t: the bound never shrank to it
        assert rejected.sum() > 30 and beyond > 20, f"{way}: {int(rejected.sum())} rays rejected, {beyond} kept items beyond"


# ------------------------------------------------------------------ 4: (c) k = 1 against the filtered closest hit
@pytest.mark.parametrize("name", ("cull_back", "masks", "skip"))
@pytest.mark.parametrize("combo", COMBOS)
def test_k1_against_the_filtered_closest_hit(world, combo, name):
    rt = world.rt
    s = world.scene("main", *combo)
    rays, flt = world.arm(combo, name)
    walk = world.fwalk(combo, name)
    rows, _, status = world.frows(combo, name, 1)
    assert status == 0
    c, ids, _ = closest_filtered(s.keep[0], rays, flt)
    hit = c["primitive_id"] != rt.MISS
    pads = rows["primitive_id"][:, 0] == rfi.MISS
    assert (hit == ~pads).all(), f"closest hit and the k = 1 row disagree on {(hit == pads).sum()} rays"
    assert rows[pads, 0].tobytes() == rfi.pad_items(int(pads.sum())).tobytes()
    decided = np.array([e[1] for e in walk.expected(1)], bool)
    sel = hit & decided
    assert sel.sum() > len(hit) // 8
    assert (rows["t"][sel, 0] <= c["t"][sel]).all()


# ------------------------------------------------------------------ 5: (d) masks that admit no instance
@pytest.mark.parametrize("combo", COMBOS)
def test_no_instance_admitted(world, combo):
    rt = world.rt
    s = world.scene("main", *combo)
    rays, flt = world.arm(combo, "none")
    _, _, tlas_slots = s.entered(rays)
    for k in (1, 4):
        rows, ctr, status = ig.first(rt, s.args, rays, k, ig.dev_filter(rt, flt))
        assert rows.tobytes() == rfi.pad_items(len(rays) * k).tobytes() and status == 0
        assert ctr[1] == 0 and ctr[0] == tlas_slots > 0, f"counters {ctr}, TLAS slots examined {tlas_slots}"


# ------------------------------------------------------------------ 6: (e) one identity instance
@pytest.mark.parametrize("which,blas_kind", ((0, "bottom_up"), (1, "sah_pairs"), (2, "sah_splits")))
def test_identity_instance_equals_the_single_tree_filtered_call(world, which, blas_kind):
    rt = world.rt
    entries, trees = world.blas(blas_kind)
    e = entries[which]
    tree = (Tree(e), e[2], e[3])
    leaves, nodes, root, count = trees[which]
    rays = rh.ray_sets(world.blas_tris[which], 11 + which, per_kind=160).astype(rt.RAY)
    for f in ("origin", "dir"):
        rays[f] = rays[f] + F(0)                         # no -0 component
    n = len(rays)
    flat = tgr.Walk(nodes, leaves, root, count, rays, len(world.blas_tris[which]))
    one = np.zeros(n, rx.RAY_FILTER)
    one["mask"] = 1 + (np.arange(n) % 3 == 0)
    one["skip_id"] = rx.nearest_ids(flat.rows)
    single = rx.Filter(rx.CULL_FRONT, 0, None, one)
    frows, fgates = rx.filtered(flat.rows, flat.gates, flat.dets, single)
    import ray_first_ref as rf
    per_ray = np.zeros(n, ifr.INSTANCE_RAY_FILTER)
    per_ray["mask"], per_ray["skip_instance"], per_ray["skip_id"] = one["mask"], 0, one["skip_id"]
    flt = ifr.InstanceFilter(ifr.CULL_FRONT, 0, None, per_ray)
    s = world.make("sah", blas_kind, ir.instance_array([np.eye(3, 4)], [which]))
    walk = ig.Walk(s, rays, flt)
    for k in (1, 4):
        both = np.array([a[1] and b[1] for a, b in zip(walk.expected(k), rf.expected(frows, fgates, k, rays["tmax"]))], bool)
        assert both.mean() > 0.9
        want, _, st0 = tgr._first(rt, tree, rays, k, single)
        rows, _, st1 = ig.first(rt, s.args, rays, k, ig.dev_filter(rt, flt))
        what = f"identity over BLAS {which} ({blas_kind}), k {k}"
        assert st0 == 0 and st1 == 0, what
        live = rows["primitive_id"] != rfi.MISS
        assert (rows["instance"][live] == 0).all() and (rows["instance"][~live] == rfi.MISS).all(), what
        got = np.ascontiguousarray(rows[["t", "primitive_id", "u", "v"]]).astype(rh.HIT)
        assert got[both].tobytes() == np.ascontiguousarray(want[both]).tobytes(), what
        assert live[:, 0].sum() == walk.nonempty > 30, "a row starts with a live item iff the filtered W is not empty"


# ------------------------------------------------------------------ 7: the twins and the mirror
@pytest.mark.parametrize("combo", COMBOS)
def test_skipping_one_twin_leaves_the_other(world, combo):
    rt = world.rt
    a, b = fsc.TWINS
    s = world.scene("main", *combo)
    rays = world.rays["main"]
    base = world.walk("main", *combo)
    per_ray = fsc.skip_nearest(base.rows, only=a)
    flt = fsc.skip_filter(per_ray)
    walk = ig.Walk(s, rays, flt)
    k = 32
    rows, _, status = ig.first(rt, s.args, rays, k, ig.dev_filter(rt, flt))
    assert status == 0 and fg.check_rows(rows, walk, k, f"{combo}: skip the nearest of instance {a}") == 0
    seen = 0
    for i in np.nonzero(per_ray["skip_instance"] == a)[0]:
        pid = per_ray["skip_id"][i]
        was = rfi.sorted_row(base.rows[i][(base.rows[i]["instance"] == a) & (base.rows[i]["primitive_id"] == pid)])[0]
        row = rows[i]
        assert not ((row["instance"] == a) & (row["primitive_id"] == pid)).any(), f"ray {i}: ({a}, {pid}) was not skipped"
        twin = row[(row["instance"] == b) & (row["primitive_id"] == pid)]
        assert len(twin) >= 1 and was["t"].tobytes() in [t.tobytes() for t in twin["t"]], f"ray {i}: ({b}, {pid}) at t {was['t']} is missing"
        seen += 1
    assert seen > 20


@pytest.mark.parametrize("combo", COMBOS[:2])
def test_mirror_rows_hold_no_world_space_back_face(world, combo):
    m = fsc.MIRROR
    rays, _ = world.arm(combo, "cull_back")
    rows, _, _ = world.frows(combo, "cull_back", 4)
    plain, _, _ = world.rows("main", *combo, 4)
    kept = before = 0
    for i in range(len(rays)):
        live = rows[i][(rows[i]["primitive_id"] != rfi.MISS) & (rows[i]["instance"] == m)]
        assert (_facing(world, rays, i, live) > -isf.FACE_MARGIN).all(), f"ray {i}: a back face of the mirror in the row"
        kept += len(live)
        before += int(((plain[i]["primitive_id"] != rfi.MISS) & (plain[i]["instance"] == m)).sum())
    assert 10 < kept < before


# ------------------------------------------------------------------ 8: short and absent per_instance arrays
@pytest.mark.parametrize("combo", COMBOS[:2])
def test_short_and_absent_per_instance(world, combo):
    rt = world.rt
    s = world.scene("main", *combo)
    rays = world.rays["main"]
    short = ifr.InstanceFilter(ifr.CULL_BACK, 1, ifr.instance_filters(3, masks=[1, 2, 1], flags=[0, 0, ifr.CULL_DISABLE]))
    walk = ig.Walk(s, rays, short)
    for k in (1, 4):
        rows, _, status = ig.first(rt, s.args, rays, k, ig.dev_filter(rt, short))
        assert status == 0
        fg.check_rows(rows, walk, k, f"{combo}: per_instance of 3 records")
        live = rows["primitive_id"] != rfi.MISS
        assert not (rows["instance"][live] == 1).any() and (rows["instance"][live] >= 3).any()

    class Lying(rt.InstanceHitFilter):                   # num_instance_filters > 0 with a null per_instance: an absent array
        def _struct(self, num_rays):
            st = super()._struct(num_rays)
            st.num_instance_filters = 77
            return st

    want, want_ctr, _ = world.rows("main", *combo, 4)
    rows, ctr, status = ig.first(rt, s.args, rays, 4, Lying())
    assert rows.tobytes() == want.tobytes() and ctr.tobytes() == want_ctr.tobytes() and status == 0


# ------------------------------------------------------------------ 9: hipGraph
def test_one_linear_hip_graph_capture_replayed_twice(world):
    import torch
    rt = world.rt
    k = 4
    combo = COMBOS[1]
    s = world.scene("main", *combo)
    rays, flt = world.arm(combo, "masks")
    want, want_ctr, _ = world.frows(combo, "masks", k)
    n = len(rays)
    rd = g.dev_rays(rt, rays)
    hf = ig.dev_filter(rt, flt)
    hits = torch.empty((n, k, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty((n, k), dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call():
        rt.RayFirstHitsInstancedFiltered(*s.args, rd, k, hf, hits, ids, counters=ctr, status=st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call()                            # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            call()                        # one kernel node: a linear graph
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        hits.view(torch.int32).fill_(SENT)
        ids.fill_(SENT)
        ctr.zero_()
        st.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = rfi.items(ids.cpu().numpy().view(np.uint32).reshape(-1), hits.cpu().numpy().view(rh.HIT).reshape(-1)).reshape(n, k)
        assert got.tobytes() == want.tobytes(), "a replay's rows differ from the eager call's"
        assert (ctr.cpu().numpy().astype(np.uint64)[:2] == want_ctr).all() and int(st.item()) == 0
