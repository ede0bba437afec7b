"""GPU tests of the hit filters of the ray queries (rt_intersect_rays_filtered, rt_ray_hits_count_filtered /
rt_ray_hits_collect_filtered, rt_ray_first_hits_filtered) on every tree the builders make, against tests/ray_filter_ref.py: the
gated all-hit walk over the tree's own bytes with the stored-corner determinant of every record, from which W_f (the kept
records), and on it E, the decided flag and the envelope of the first-K contract, follow with no kernel involved.

1. all-hit rows equal W_f as multisets of 16-byte records on all eight trees of four scenes, for five filters (cull back, cull
   front, three groups against per-ray masks, skip the nearest, all combined); count and collect agree; counters [0] and [1]
   are the unfiltered call's;
2. the partition laws on device output alone;
3. first-K filtered, k in {1, 3, 8, 32}: decided rays are E on W_f bit for bit, the envelope holds on every ray, the undecided
   share of the reference is under the cap;
4. closest / any filtered, both instantiations: the record is in W_f, a miss iff W_f is empty, any-hit iff closest-hit, t = E's
   t on k=1-decided rays;
5. keep-all filters (both spellings) and filter = NULL give the unfiltered entry points' bytes and counters;
6. winding on pair trees against a float64 brute force on the caller's corners;
7. self-hit-free bounce rays through skip_id;
8. batch ends, dead rays, the empty tree, mask 0, per_ray indexed by the ray's index;
9. one hipGraph capture and replay of a filtered closest-hit plus a filtered first-K call."""
import numpy as np
import pytest

import range_sets as rs
import ray_filter_ref as rx
import ray_first_ref as rf
import ray_hits_ref as rh
import sdf_ref
from test_gpu_ray_hits import PAD, SENT, TREES, _dev_rays, _download
from test_gpu_ray_queries import _gpu_tree
from test_ray_filter_ref_cpu import BOUNCE_SEED

pytestmark = pytest.mark.gpu

SCENES = ("grid", "soup", "cornell", "fractal")
F = np.float32
BIG = 16 << 20            # num_primitives hint that selects the pair-prefetch instantiation
UNFILTERED = "unfiltered"  # in the place of a filter: the unfiltered entry point


# ------------------------------------------------------------------ helpers
def _dev_filter(rt, flt):
    """rx.Filter (host arrays) -> rt.HitFilter (device arrays); None stays None (filter = NULL)"""
    import torch
    if flt is None:
        return None
    pm = None if flt.prim_masks is None else rt.to_device(flt.prim_masks).view(torch.int32)
    pr = None if flt.per_ray is None else rt.to_device(flt.per_ray).view(torch.int32).view(-1, 2)
    return rt.HitFilter(flt.flags, flt.ray_mask, pm, pr)


class Result:
    pass


def _hits(rt, g, rays, flt):
    """count, then collect into exactly offsets[n] records, both through `flt` (UNFILTERED: the unfiltered entry points).
    Sentinels lie behind every buffer.  Asserts what holds for ANY filter: count and collect agree."""
    import torch
    inp, root, count = g
    tri, nod = inp.triangles_out, inp.nodes_out
    r = Result()
    rd = _dev_rays(rt, rays)
    n = len(rays)
    hf = None if flt is UNFILTERED else _dev_filter(rt, flt)
    off = torch.full((n + 1 + PAD,), SENT, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    if flt is UNFILTERED:
        rt.RayHitsCount(tri, nod, root, count, rd, off[:n + 1], counters=ctr, status=st)
    else:
        rt.RayHitsCountFiltered(tri, nod, root, count, rd, hf, off[:n + 1], counters=ctr, status=st)
    torch.cuda.synchronize()
    o = off.cpu().numpy()
    assert (o[n + 1:] == SENT).all(), "the count call wrote past offsets[n]"
    r.offsets, r.ctr_count, r.st_count = o[:n + 1], ctr.cpu().numpy().astype(np.uint64), rt.ray_hits_status(st)
    assert r.offsets[0] == 0 and (np.diff(r.offsets) >= 0).all()
    total = int(r.offsets[n])
    hits = torch.full(((total + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")
    ctr.zero_()
    st.zero_()
    if flt is UNFILTERED:
        rt.RayHitsCollect(tri, nod, root, count, rd, off[:n + 1], hits, counts=cnt[:n], counters=ctr, status=st)
    else:
        rt.RayHitsCollectFiltered(tri, nod, root, count, rd, hf, off[:n + 1], hits, counts=cnt[:n], counters=ctr, status=st)
    torch.cuda.synchronize()
    h, c = hits.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert (h[total * 4:] == SENT).all(), "the collect call wrote past the last segment"
    assert (c[n:] == SENT).all(), "the collect call wrote counts past num_rays"
    recs, r.counts = h[:total * 4].view(rh.HIT), c[:n]
    r.ctr_collect, r.st_collect = ctr.cpu().numpy().astype(np.uint64), rt.ray_hits_status(st)
    assert (r.counts.astype(np.int64) == np.diff(r.offsets)).all(), "collect's counts differ from the differences of offsets"
    assert (recs.view(np.uint32).reshape(-1, 4) != SENT).any(1).all(), "a segment was not filled"
    assert (r.ctr_count == r.ctr_collect).all() and r.ctr_count[2] == 0 and r.ctr_count[3] == 0
    assert r.st_count == r.st_collect == 0
    r.rows = [recs[r.offsets[k]:r.offsets[k + 1]] for k in range(n)]
    r.raw = recs
    return r


def _first(rt, g, rays, k, flt):
    """-> (rows: HIT [n, k], counters uint64[4], status); sentinels behind the rows, every record written"""
    import torch
    inp, root, count = g
    rd = _dev_rays(rt, rays)
    n = rd.shape[0]
    buf = torch.full(((n * k + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    out = buf[:n * k * 4].view(torch.float32).view(n, k, 4)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    if flt is UNFILTERED:
        assert rt.RayFirstHits(inp.triangles_out, inp.nodes_out, root, count, rd, k, out, counters=ctr, status=st) == n
    else:
        assert rt.RayFirstHitsFiltered(inp.triangles_out, inp.nodes_out, root, count, rd, k, _dev_filter(rt, flt), out,
                                       counters=ctr, status=st) == n
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[n * k * 4:] == SENT).all(), "the first-K call wrote past the last row"
    assert (h[:n * k * 4].reshape(-1, 4) != SENT).any(1).all(), "a record of a row was not written"
    c = ctr.cpu().numpy().astype(np.uint64)
    assert c[2] == 0 and c[3] == 0
    return h[:n * k * 4].view(rf.HIT).reshape(n, k), c, rt.ray_first_status(st)


def _closest(rt, g, rays, flt, any_hit=False, num_primitives=0):
    """-> (HIT [n], counters uint64[4]); sentinels behind the records, every record written"""
    import torch
    inp, root, count = g
    rd = _dev_rays(rt, rays)
    n = rd.shape[0]
    buf = torch.full(((n + PAD) * 4,), SENT, dtype=torch.int32, device="cuda")
    hits = buf[:n * 4].view(torch.float32).view(n, 4)
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    if flt is UNFILTERED:
        rt.IntersectRays(inp.triangles_out, inp.nodes_out, root, count, rd, hits, any_hit=any_hit, num_primitives=num_primitives,
                         counters=ctr)
    else:
        rt.IntersectRaysFiltered(inp.triangles_out, inp.nodes_out, root, count, rd, hits, _dev_filter(rt, flt), any_hit=any_hit,
                                 num_primitives=num_primitives, counters=ctr)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[n * 4:] == SENT).all(), "the closest-hit call wrote past the last record"
    assert (h[:n * 4].reshape(-1, 4) != SENT).any(1).all(), "a record was not written"
    return h[:n * 4].view(rf.HIT).reshape(n), ctr.cpu().numpy().astype(np.uint64)


def _same_rows(rows, ref_rows, what):
    for i, (a, b) in enumerate(zip(rh.canon(rows), rh.canon(ref_rows))):
        assert a.shape == b.shape and (a == b).all(), f"{what}: ray {i}: {len(a)} records, the reference has {len(b)}"


def _join(*parts):
    return [np.concatenate(p) for p in zip(*parts)]


class Walk:
    """the reference of one (tree, ray set): W with gates and determinants and its counters -- computed once, never changed --
    and, per filter, W_f with its gates and Ws"""
    def __init__(self, nodes, leaves, root, count, rays, num_triangles):
        self.rays, self.num_triangles = rays, num_triangles
        self.rows, self.gates, self.dets, self.box_tests, self.leaf_visits = rx.walk_gated_det(nodes, leaves, root, count, rays)
        self._f = {}

    def filter(self, name):
        return self.kept(name)[0]

    def kept(self, name):
        """-> (the rx.Filter `name`, W_f rows, gates, dedup)"""
        if name not in self._f:
            flt = rx.make_filter(name, self.rows, self.num_triangles)
            frows, fgates = rx.filtered(self.rows, self.gates, self.dets, flt)
            self._f[name] = flt, frows, fgates, rf.dedup_all(frows, fgates)
        return self._f[name]

    def expected(self, name, k):
        _, frows, fgates, dedup = self.kept(name)
        return rf.expected(frows, fgates, k, self.rays["tmax"], dedup=dedup)


class World:
    """scenes, their ray sets, built trees and, per (scene, tree), the reference over the downloaded bytes -- computed once"""
    def __init__(self, rt, scenes):
        self.rt, self.scenes = rt, scenes
        self._sc, self._g, self._w, self._u = {}, {}, {}, {}

    def scene(self, name):
        if name not in self._sc:
            tris = rs.scene_tris(name, self.scenes)
            self._sc[name] = tris, rh.ray_sets(tris, rh.SEEDS[name]).astype(self.rt.RAY)
        return self._sc[name]

    def gpu(self, name, tree):
        if (name, tree) not in self._g:
            self._g[name, tree] = _gpu_tree(self.rt, self.scene(name)[0], tree)
        return self._g[name, tree]

    def walk(self, name, tree):
        if (name, tree) not in self._w:
            inp, root, count = self.gpu(name, tree)
            nodes, leaves = _download(self.rt, inp)
            tris, rays = self.scene(name)
            self._w[name, tree] = Walk(nodes, leaves, root, count, rays, tris.shape[0])
        return self._w[name, tree]

    def unfiltered(self, name, tree):
        """the device's unfiltered all-hit result"""
        if (name, tree) not in self._u:
            self._u[name, tree] = _hits(self.rt, self.gpu(name, tree), self.scene(name)[1], UNFILTERED)
        return self._u[name, tree]


@pytest.fixture(scope="module")
def world(rt, scenes):
    return World(rt, scenes)


# ------------------------------------------------------------------ 1: all-hit rows equal W_f
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_all_hit_rows_equal_the_kept_walk(world, name, tree):
    rt = world.rt
    g, rays, walk = world.gpu(name, tree), world.scene(name)[1], world.walk(name, tree)
    plain = world.unfiltered(name, tree)
    assert len(rays) == 2048
    assert plain.ctr_count[0] == walk.box_tests and plain.ctr_count[1] == walk.leaf_visits
    for fname in rx.FILTERS:
        what = f"{name}/{tree}/{fname}"
        flt, frows, _, _ = walk.kept(fname)
        r = _hits(rt, g, rays, flt)
        assert (r.offsets == rh.offsets(frows)).all(), f"{what}: offsets differ from the prefix sum of |W_f|"
        _same_rows(r.rows, frows, what)
        assert (r.ctr_count == plain.ctr_count).all(), f"{what}: counters {r.ctr_count[:2]}, unfiltered {plain.ctr_count[:2]}"
        kept, total = int(r.offsets[-1]), int(plain.offsets[-1])
        assert 0 < kept < total, f"{what}: the filter keeps {kept} of {total} records: not a test of it"
        print(f"{what}: {kept} of {total} records kept")


# ------------------------------------------------------------------ 2: partition laws on device output alone
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", ("bottom_up", "hybrid_pairs", "sah_pairs_splits"))
def test_partition_laws_on_device_output(world, name, tree):
    rt = world.rt
    g, (tris, rays) = world.gpu(name, tree), world.scene(name)
    plain = world.unfiltered(name, tree)
    n = len(rays)
    back = _hits(rt, g, rays, rx.Filter(rx.CULL_BACK))
    front = _hits(rt, g, rays, rx.Filter(rx.CULL_FRONT))
    both = _hits(rt, g, rays, rx.Filter(rx.CULL_BACK | rx.CULL_FRONT))          # what is neither: the NaN determinants
    _same_rows(_join(back.rows, front.rows, both.rows), plain.rows, f"{name}/{tree}: back + front + neither")
    for i in range(n):
        b, f = (set(x.tobytes() for x in r.rows[i]) for r in (back, front))
        assert not (b & f), f"{name}/{tree}: ray {i}: a record both front and back"
    assert back.offsets[-1] > 0 and front.offsets[-1] > 0
    assert both.offsets[-1] == 0 or name == "fractal", "only overflowed products give a NaN determinant"
    per_ray = np.zeros(n, rx.RAY_FILTER)
    per_ray["mask"], per_ray["skip_id"] = np.random.default_rng(5).integers(1, 1 << rx.GROUPS, n), rx.MISS
    inv = per_ray.copy()
    inv["mask"] = ~per_ray["mask"]
    pm = rx.group_masks(tris.shape[0])
    m_rows, i_rows = (_hits(rt, g, rays, rx.Filter(0, 0, pm, p)) for p in (per_ray, inv))
    _same_rows(_join(m_rows.rows, i_rows.rows), plain.rows, f"{name}/{tree}: mask m + mask ~m")
    assert 0 < m_rows.offsets[-1] < plain.offsets[-1]
    skip = per_ray.copy()
    skip["mask"], skip["skip_id"] = rx.ALL, rx.nearest_ids(plain.rows)
    s = _hits(rt, g, rays, rx.Filter(0, 0, None, skip))
    _same_rows(s.rows, [r[r["primitive_id"] != sid] for r, sid in zip(plain.rows, skip["skip_id"])], f"{name}/{tree}: skip")
    assert s.offsets[-1] < plain.offsets[-1]


# ------------------------------------------------------------------ 3: first-K on W_f
def _check_first_rows(rows, walk, fname, k, what, exp):
    """decided rays are E bit for bit; claims 1 and 3 on every ray, against W_f"""
    _, frows, fgates, _ = walk.kept(fname)
    n = len(walk.rays)
    want = rf.padded(exp, k)
    equal = (rows.view(np.uint32).reshape(n, -1) == want.view(np.uint32).reshape(n, -1)).all(1)
    decided = np.array([e[1] for e in exp], bool)
    wrong = np.nonzero(decided & ~equal)[0]
    assert len(wrong) == 0, f"{what}: {len(wrong)} decided rays differ from E; ray {wrong[0]}: {rows[wrong[0]]} != {want[wrong[0]]}"
    misses = rf.miss_records(k).tobytes()
    for i in range(n):
        if len(frows[i]) == 0:                                # (the envelope of an empty W_f: a row of misses)
            assert rows[i].tobytes() == misses, f"{what}: ray {i}: W_f is empty and the row is {rows[i]}"
            continue
        why = rf.envelope_violation(rows[i], frows[i], fgates[i], k, walk.rays["tmax"][i])
        assert why is None, f"{what}: ray {i}: {why}"
    return int((~equal).sum())


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_first_k_rows_against_the_kept_walk(world, name, tree):
    rt = world.rt
    g, rays, walk = world.gpu(name, tree), world.scene(name)[1], world.walk(name, tree)
    for fname in rx.FILTERS:
        flt, frows, _, _ = walk.kept(fname)
        for k in rx.KS:
            what = f"{name}/{tree}/{fname}: k {k}"
            exp = walk.expected(fname, k)
            share = rf.undecided_share(exp, frows)             # the reference alone: a condition on the inputs
            assert share <= rf.CAP, f"{what}: {100 * share:.2f} % of the rays are undecided"
            rows, ctr, status = _first(rt, g, rays, k, flt)
            assert status == 0, f"{what}: status {status}"
            differ = _check_first_rows(rows, walk, fname, k, what, exp)
            assert ctr[0] <= walk.box_tests and ctr[1] <= walk.leaf_visits, f"{what}: counters {ctr[:2]} exceed the all-hit walk's"
            print(f"{what}: {100 * share:.3f} % undecided, {differ} rows differ from E, box tests {int(ctr[0])} of {walk.box_tests}")


# ------------------------------------------------------------------ 4: closest / any
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tree", TREES)
def test_closest_and_any_hit_against_the_kept_walk(world, name, tree):
    rt = world.rt
    g, rays, walk = world.gpu(name, tree), world.scene(name)[1], world.walk(name, tree)
    n = len(rays)
    for fname in rx.FILTERS:
        flt, frows, _, _ = walk.kept(fname)
        exp = walk.expected(fname, 1)
        empty = np.array([len(r) == 0 for r in frows])
        for pf in (0, BIG):
            what = f"{name}/{tree}/{fname}, num_primitives {pf}"
            hits, _ = _closest(rt, g, rays, flt, num_primitives=pf)
            anyh, _ = _closest(rt, g, rays, flt, any_hit=True, num_primitives=pf)
            miss = hits["primitive_id"] == rf.MISS
            assert (miss == empty).all(), f"{what}: a miss holds iff W_f is empty; rays {np.nonzero(miss != empty)[0][:4]}"
            assert hits[miss].tobytes() == rf.miss_records(int(miss.sum())).tobytes()
            assert ((anyh["primitive_id"] == rf.MISS) == miss).all(), f"{what}: any-hit hits iff closest-hit hits"
            for i in np.nonzero(~miss)[0]:
                w = frows[i]
                for h, kind in ((hits[i], "closest"), (anyh[i], "any")):
                    same = (w["t"].view(np.uint32) == h["t"].view(np.uint32)) & (w["u"].view(np.uint32) == h["u"].view(np.uint32)) & \
                           (w["v"].view(np.uint32) == h["v"].view(np.uint32))
                    assert same.any(), f"{what}: ray {i}: the {kind} record {h} is not in W_f in (t, u, v)"
                    assert h["primitive_id"] in w["primitive_id"], f"{what}: ray {i}: the {kind} record {h} carries a filtered id"
                E, decided, _ = exp[i]
                if decided:
                    assert hits["t"][i].view(np.uint32) == E["t"][0].view(np.uint32), \
                        f"{what}: decided ray {i}: t {hits['t'][i]} is not E's {E['t'][0]}"
        assert 0 < empty.sum() < n


# ------------------------------------------------------------------ 5: keep-all filters and filter = NULL
@pytest.mark.parametrize("name,tree", (("grid", "hybrid_pairs"), ("soup", "sah_splits"), ("fractal", "sah")))
def test_keep_all_filters_are_the_unfiltered_calls(world, name, tree):
    rt = world.rt
    g, (tris, rays) = world.gpu(name, tree), world.scene(name)
    n = len(rays)
    per_ray = np.zeros(n, rx.RAY_FILTER)
    per_ray["mask"], per_ray["skip_id"] = rx.ALL, rx.MISS
    spellings = {"flags 0, null arrays": rx.Filter(), "all-ones arrays": rx.Filter(0, 0, np.full(tris.shape[0], rx.ALL, np.uint32), per_ray),
                 "filter = NULL": None}
    plain = world.unfiltered(name, tree)
    plain_first = {k: _first(rt, g, rays, k, UNFILTERED) for k in (1, 8)}
    plain_closest = {(a, pf): _closest(rt, g, rays, UNFILTERED, any_hit=a, num_primitives=pf) for a in (False, True) for pf in (0, BIG)}
    for what, flt in spellings.items():
        r = _hits(rt, g, rays, flt)
        assert (r.offsets == plain.offsets).all() and r.raw.tobytes() == plain.raw.tobytes(), f"{what}: all-hit bytes"
        assert (r.ctr_count == plain.ctr_count).all() and (r.counts == plain.counts).all(), f"{what}: all-hit counters"
        for k, (rows, ctr, status) in plain_first.items():
            frows, fctr, fstatus = _first(rt, g, rays, k, flt)
            assert frows.tobytes() == rows.tobytes() and (fctr == ctr).all() and fstatus == status, f"{what}: first-K, k {k}"
        for (a, pf), (hits, ctr) in plain_closest.items():
            fhits, fctr = _closest(rt, g, rays, flt, any_hit=a, num_primitives=pf)
            assert fhits.tobytes() == hits.tobytes() and (fctr == ctr).all(), f"{what}: closest / any {a}, num_primitives {pf}"


# ------------------------------------------------------------------ 6: winding on pair trees
@pytest.mark.parametrize("mesh", ("icosphere", "torus"))
@pytest.mark.parametrize("tree", ("pairs", "sah_pairs", "bottom_up"))
def test_facing_is_the_callers_winding(rt, mesh, tree):
    tris = sdf_ref.mesh(mesh)                                  # closed, outward-wound
    rays = rh.ray_sets(tris, 11)[:512].astype(rt.RAY)          # the first kind: from outside, towards interior points
    g = _gpu_tree(rt, tris, tree)
    b = rh.brute_f64(tris, rays)
    T = tris.reshape(-1, 3, 3).astype(np.float64)
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    # float64 facing on the CALLER's corners: a = e1 . (dir x e2) = -dir . n; brute_f64's `stable` keeps |a| away from 0
    a64 = np.einsum("tj,rtj->rt", e1, np.cross(rays["dir"].astype(np.float64)[:, None, :], e2[None]))
    plain = _hits(rt, g, rays, UNFILTERED)
    culled = _hits(rt, g, rays, rx.Filter(rx.CULL_BACK))
    got = np.zeros(b["accepted"].shape, bool)
    for i, row in enumerate(culled.rows):
        got[i, row["primitive_id"].astype(np.int64)] = True
    want_kept = b["stable"] & b["accepted"] & (a64 > 0)
    want_dropped = b["stable"] & (~b["accepted"] | (a64 < 0))
    assert want_kept.sum() > len(rays) // 4 and (b["stable"] & b["accepted"] & (a64 < 0)).sum() > len(rays) // 4
    assert not (want_kept & ~got).any(), f"{mesh}/{tree}: stable front crossings were culled: {np.argwhere(want_kept & ~got)[:4]}"
    assert not (want_dropped & got).any(), f"{mesh}/{tree}: stable back crossings were kept: {np.argwhere(want_dropped & got)[:4]}"
    all_stable = b["stable"].all(1)
    lens, culled_lens = np.diff(plain.offsets), np.diff(culled.offsets)
    assert all_stable.sum() > len(rays) // 2 and (lens[all_stable] > 0).sum() > len(rays) // 8
    assert (2 * culled_lens[all_stable] == lens[all_stable]).all(), "a ray from outside a closed mesh enters as often as it leaves"


# ------------------------------------------------------------------ 7: self-hit
@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_pairs"))
def test_bounce_rays_skip_their_own_triangle(world, tree):
    rt = world.rt
    g, rays = world.gpu("grid", tree), world.scene("grid")[1]
    primary, _ = _closest(rt, g, rays, UNFILTERED)
    bounce, per_ray = rx.bounce_rays(rays, primary, BOUNCE_SEED)
    bounce = bounce.astype(rt.RAY)
    assert len(bounce) > len(rays) // 8
    own, _ = _closest(rt, g, bounce, UNFILTERED)
    self_hits = int((own["primitive_id"] == per_ray["skip_id"]).sum())
    print(f"grid/{tree}: {self_hits} of {len(bounce)} unfiltered bounce rays report the triangle they start on")
    assert self_hits > 0, "no bounce ray meets its own triangle: not a test of skip_id"
    flt = rx.Filter(0, 0, None, per_ray)
    skip = per_ray["skip_id"]
    for any_hit in (False, True):
        hits, _ = _closest(rt, g, bounce, flt, any_hit=any_hit)
        assert (hits["primitive_id"] != skip).all(), f"closest / any {any_hit}: a skipped id is reported"
    r = _hits(rt, g, bounce, flt)
    plain = _hits(rt, g, bounce, UNFILTERED)
    assert all((row["primitive_id"] != s).all() for row, s in zip(r.rows, skip))
    _same_rows(r.rows, [row[row["primitive_id"] != s] for row, s in zip(plain.rows, skip)], f"grid/{tree}: bounce rows")
    for k in (1, 4):
        rows, _, status = _first(rt, g, bounce, k, flt)
        assert status == 0 and (rows["primitive_id"] != skip[:, None]).all(), f"first-K, k {k}: a skipped id is listed"
    # what the filter is for: the filtered nearest hit lies past the surface the ray starts on, never at t ~ 0 on it
    fhits, _ = _closest(rt, g, bounce, flt)
    assert (fhits["primitive_id"] != own["primitive_id"])[own["primitive_id"] == skip].all()


# ------------------------------------------------------------------ 8: batch ends, dead rays, the empty tree, mask 0
def test_batch_ends_dead_rays_empty_tree_and_mask_zero(world):
    rt = world.rt
    name, tree = "soup", "hybrid_pairs"
    g, (tris, rays), walk = world.gpu(name, tree), world.scene(name), world.walk(name, tree)
    flt = walk.filter("combined")
    k = 3
    full = _hits(rt, g, rays, flt)
    full_first, _, _ = _first(rt, g, rays, k, flt)
    full_closest, _ = _closest(rt, g, rays, flt)
    # batch ends: a sub-batch with the matching per_ray records gives the batch's own rows (sentinels checked inside)
    for n in (1, 63, 257):
        sub = flt.sliced(slice(0, n))
        r = _hits(rt, g, rays[:n], sub)
        assert (r.offsets == full.offsets[:n + 1]).all() and r.raw.tobytes() == full.raw[:full.offsets[n]].tobytes(), f"batch of {n}"
        rows, _, _ = _first(rt, g, rays[:n], k, sub)
        assert rows.tobytes() == full_first[:n].tobytes(), f"first-K, batch of {n}"
        hits, _ = _closest(rt, g, rays[:n], sub)
        assert hits.tobytes() == full_closest[:n].tobytes(), f"closest, batch of {n}"
    # per_ray is indexed by the ray's index: rays and records permuted together give the permuted results
    perm = np.random.default_rng(8).permutation(300)
    sub = flt.sliced(perm)
    r = _hits(rt, g, rays[perm], sub)
    _same_rows(r.rows, [full.rows[j] for j in perm], "permuted batch")
    rows, _, _ = _first(rt, g, rays[perm], k, sub)
    assert rows.tobytes() == full_first[perm].tobytes()
    hits, _ = _closest(rt, g, rays[perm], sub)
    assert hits.tobytes() == full_closest[perm].tobytes()
    assert (full_closest[:300].tobytes() != hits.tobytes()), "the permutation must change something"
    # dead rays: empty rows, rows of misses, nothing counted
    nan = F(np.nan)
    dead = rays[:5].copy()
    dead["tmin"][0], dead["tmax"][0] = 5.0, 1.0
    dead["origin"][1, 0] = nan
    dead["dir"][2, 1] = nan
    dead["tmin"][3] = nan
    dead["tmax"][4] = nan
    assert not rf.live(dead).any()
    sub = flt.sliced(slice(0, 5))
    r = _hits(rt, g, dead, sub)
    assert r.offsets[-1] == 0 and (r.ctr_count == 0).all()
    rows, ctr, status = _first(rt, g, dead, k, sub)
    assert rows.tobytes() == rf.miss_records(5 * k).tobytes() and (ctr == 0).all() and status == 0
    hits, ctr = _closest(rt, g, dead, sub)
    assert hits.tobytes() == rf.miss_records(5).tobytes() and (ctr[:2] == 0).all()
    # the empty tree (count = 0): nothing is read through it
    inp, _, _ = g
    empty = (inp, 0, 0)
    sub = flt.sliced(slice(0, 300))
    r = _hits(rt, empty, rays[:300], sub)
    assert r.offsets[-1] == 0 and (r.ctr_count == 0).all()
    rows, ctr, _ = _first(rt, empty, rays[:300], k, sub)
    assert rows.tobytes() == rf.miss_records(300 * k).tobytes() and (ctr == 0).all()
    hits, _ = _closest(rt, empty, rays[:300], sub)
    assert hits.tobytes() == rf.miss_records(300).tobytes()
    # mask 0: the ray is traced (the unfiltered counters) and keeps nothing
    plain = world.unfiltered(name, tree)
    for zero in (rx.Filter(0, 0), rx.Filter(0, rx.ALL, np.zeros(tris.shape[0], np.uint32))):
        r = _hits(rt, g, rays, zero)
        assert r.offsets[-1] == 0 and (r.ctr_count == plain.ctr_count).all() and plain.ctr_count[1] > 0
        rows, ctr, _ = _first(rt, g, rays, k, zero)
        assert rows.tobytes() == rf.miss_records(len(rays) * k).tobytes() and (ctr == plain.ctr_count).all()
        for any_hit in (False, True):
            hits, ctr = _closest(rt, g, rays, zero, any_hit=any_hit)
            assert hits.tobytes() == rf.miss_records(len(rays)).tobytes() and ctr[1] > 0
    # a prim_masks array shorter than the ids: ids beyond it are all ones
    short = np.zeros(tris.shape[0] // 2, np.uint32)
    r = _hits(rt, g, rays, rx.Filter(0, rx.ALL, short))
    _same_rows(r.rows, [row[row["primitive_id"] >= len(short)] for row in plain.rows], "a short prim_masks array")
    assert 0 < r.offsets[-1] < plain.offsets[-1]


# ------------------------------------------------------------------ 9: hipGraph
def test_filtered_calls_in_a_hip_graph(world):
    import torch
    rt = world.rt
    name, tree = "grid", "sah_pairs"
    g, rays, walk = world.gpu(name, tree), world.scene(name)[1], world.walk(name, tree)
    inp, root, count = g
    flt = walk.filter("combined")
    n, k = 700, 4
    hf = _dev_filter(rt, flt.sliced(slice(0, n)))
    rd = _dev_rays(rt, rays[:n]).clone()
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    out = torch.empty((n, k, 4), dtype=torch.float32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def one_frame():
        st.zero_()
        rt.IntersectRaysFiltered(inp.triangles_out, inp.nodes_out, root, count, rd, hits, hf)
        rt.RayFirstHitsFiltered(inp.triangles_out, inp.nodes_out, root, count, rd, k, hf, out, status=st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()                       # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for lo in (0, 900):                   # (the per-ray records stay those of rays[:n]: the graph holds their pointer)
        batch = rays[lo:lo + n]
        rd.copy_(_dev_rays(rt, batch))
        hits.fill_(0)
        out.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        got_hits = hits.cpu().numpy().view(rf.HIT).reshape(n)
        got_rows = out.cpu().numpy().view(rf.HIT).reshape(n, k)
        sub = flt.sliced(slice(0, n))
        eager_hits, _ = _closest(rt, g, batch, sub)
        eager_rows, _, eager_st = _first(rt, g, batch, k, sub)
        assert got_hits.tobytes() == eager_hits.tobytes() and got_rows.tobytes() == eager_rows.tobytes()
        assert int(st.item()) == eager_st == 0
        assert (eager_hits["primitive_id"] != rf.MISS).sum() > n // 8
