"""GPU tests of the sphere cast (rt_sphere_cast) against tests/sphere_cast_ref.py, the numpy restatement of the header
(tests/test_sphere_cast_ref_cpu.py checks that reference on its own).

A tree stores a triangle's corners in an order of its own (a rotation per leaf triangle; in a split tree one triangle may sit
in several leaves), and the float32 test runs on the stored corners.  So every tree is copied back and walked on the host for
its stored triangles, and a device record is held to the restatement on SOME stored instance of the reported triangle.

1. closest hit, per scene x seed x {LBVH, SAH, SAH + pairs, SAH + splits}: every record and its feature word are the
   restatement's for the reported triangle and the ray's original window, bit for bit; on float64-stable rays hit / miss and
   overlap / travel are float64's, the triangle is one within the gap of float64's least t, t is the least float32 t over the
   stored instances of those triangles bit for bit, and within GPU_TOL_FACTOR x sphere_cast_ref.T_TOL of float64's;
2. any hit: hits exactly where closest hits, a genuine float32 contact; re-casting a closest travelling hit under
   tmax = nextafter(t, 0) finds nothing;
3. overlap rows are the rows where rt_range_count in sphere shape on (o + tmin*d, r*r) counts a triangle;
4. a uniform `radius` equals a filled `radii` array byte for byte; features = None works;
5. counters add across launches and are invariant under a permutation; partial index lists with out-of-range entries;
   rt_sort_rays's order;
6. trees of 1, 2, 3 and 5 triangles, one pair leaf, a ball larger than the whole scene;
7. invalid radii inside a batch, degenerate rays, batch sizes 1 to 257 with poison behind them, the empty tree;
8. a cast after rt_refit;
9. build plus both modes in one HIP graph, replayed after `radii` is rewritten in place."""
import numpy as np
import pytest

import sphere_cast_ref as sc
import test_gpu_ray_queries as rq

pytestmark = pytest.mark.gpu

F = np.float32
TREES = ("bottom_up", "sah", "sah_pairs", "sah_splits")
POISON = 0x5A5A5A5A


# ------------------------------------------------------------------ plumbing
def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def stored_instances(leaves, nodes, root, count):
    """walk the tree: (prim ids, stored corners float32 [m, 9], rotations) of every leaf triangle the cast would test"""
    prims, stored, rots = [], [], []
    stack = [(root, count)]
    seen = set()
    while stack:
        idx, cnt = stack.pop()
        for k in range(idx, idx + cnt):
            w12, w28 = int(nodes["w12"][k]), int(nodes["w28"][k])
            kind, child, c = w28 >> 29, w28 & 0x1FFFFFFF, w12 >> 29
            if kind == 1:
                stack.append((child, c))
            elif kind == 2 and child not in seen:
                seen.add(child)
                lf = leaves[child]
                prims.append(int(lf["primitive_id_0"]))
                stored.append(np.concatenate([lf["v0"], lf["v1"], lf["v2"]]))
                rots.append(int(lf["rotations"][0]))
                if c > 0 and lf["v3"].tobytes() != lf["v2"].tobytes():
                    prims.append(int(lf["primitive_id_1"]))
                    stored.append(np.concatenate([lf["v2"], lf["v1"], lf["v3"]]))
                    rots.append(int(lf["rotations"][1]))
    return np.array(prims, np.int64), np.array(stored, F).reshape(-1, 9), np.array(rots, np.uint32)


class Tree:
    """one built tree, its stored triangles on the host and the device calls on it"""

    def __init__(self, rt, tris, tree, built=None):
        self.rt, self.tris, self.kind = rt, np.ascontiguousarray(tris, F).reshape(-1, 9), tree
        self.inp, self.root, self.count = built if built else rq._gpu_tree(rt, self.tris, tree)
        self.read_back()

    def read_back(self):
        rt = self.rt
        leaves, nodes = rt.to_host(self.inp.triangles_out, rt.TRIANGLE_PAIR), rt.to_host(self.inp.nodes_out, rt.NODE)
        self.prims, self.stored, self.rots = stored_instances(leaves, nodes, self.root, self.count)
        order = np.argsort(self.prims, kind="stable")
        self.prims, self.stored, self.rots = self.prims[order], self.stored[order], self.rots[order]
        n = self.tris.shape[0]
        self.first = np.searchsorted(self.prims, np.arange(n))
        self.copies = np.searchsorted(self.prims, np.arange(n), side="right") - self.first
        self.M = sc.root_M(nodes, self.root, self.count)

    def launch(self, rays, hits, **kw):
        self.rt.SphereCast(self.inp.triangles_out, self.inp.nodes_out, self.root, self.count, rays, hits, **kw)

    def cast(self, rays, radii=None, radius=0.0, counters=False, features=True, **kw):
        """numpy RAY array (+ numpy radii) -> (HIT array, feature words or None, counters or None)"""
        import torch
        rt = self.rt
        d = _dev_rays(rt, rays)
        n = d.shape[0]
        hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        feats = torch.full((n,), POISON, dtype=torch.int32, device="cuda") if features else None
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda") if counters else None
        rd = None if radii is None else rt.to_device(np.ascontiguousarray(radii, F)).view(torch.float32)
        self.launch(d, hits, radii=rd, radius=radius, features=feats, counters=ctr, **kw)
        torch.cuda.synchronize()
        return (hits.cpu().numpy().view(rt.HIT).reshape(-1), feats.cpu().numpy().view(np.uint32) if features else None,
                ctr.cpu().numpy().astype(np.uint64) if counters else None)


def _dev_rays(rt, rays):
    import torch
    return rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)


def _best_over_instances(tree, rays, radii, ri, ti):
    """the restatement of ray ri[k] on every stored instance of triangle ti[k]: per pair the least t (NaN: none) and whether
    some instance gives exactly `want` (t, u, v, feature) when that is given"""
    out = []
    for k in range(int(tree.copies[ti].max(initial=0))):
        sel = np.flatnonzero(tree.copies[ti] > k)
        j = tree.first[ti[sel]] + k
        out.append((sel, sc.pairs_f32(rays, radii, ri[sel], tree.stored[j], tree.rots[j])))
    return out


def _check_records(tree, hits, feats, rays, radii, what):
    """every record is the miss record or the restatement's record of some stored instance of the reported triangle in the
    ray's original window, feature word included"""
    hit = hits["primitive_id"] != sc.MISS
    miss = hits[~hit]
    assert (miss["t"] == np.inf).all() and (_bits(miss["u"]) == 0).all() and (_bits(miss["v"]) == 0).all(), what
    assert (feats[~hit] == sc.NONE).all(), what
    assert not (hit & ~sc.traced(rays, radii)).any(), f"{what}: a ray that is not traced hit"
    ri = np.flatnonzero(hit)
    ti = hits["primitive_id"][hit].astype(np.int64)
    assert (ti < tree.tris.shape[0]).all() and (tree.copies[ti] > 0).all(), what
    ok = np.zeros(ri.size, bool)
    for sel, (t, u, v, f) in _best_over_instances(tree, rays, radii, ri, ti):
        h = hits[ri[sel]]
        ok[sel] |= (_bits(t) == _bits(h["t"])) & (_bits(u) == _bits(h["u"])) & (_bits(v) == _bits(h["v"])) & (f == feats[ri[sel]])
    assert ok.all(), f"{what}: {int((~ok).sum())} records are not the float32 formula's for the reported triangle (first: ray " \
                     f"{ri[~ok][:5]}, features {feats[ri[~ok][:5]]})"
    return hit


def _check_closest(tree, hits, feats, ref, what, name=None):
    hit = _check_records(tree, hits, feats, ref.rays, ref.radii, what)
    st = ref.stable
    over = feats == sc.OVERLAP
    assert (hit[st] == ref.f64["hit"][st]).all(), f"{what}: hit / miss differs from float64 on a stable ray"
    assert (over[st] == ref.f64["over"][st]).all(), f"{what}: overlap / travel differs from float64 on a stable ray"
    assert (_bits(hits["t"][over]) == _bits(ref.rays["tmin"][over])).all(), what
    both = np.flatnonzero(st & hit)
    ids = hits["primitive_id"][both].astype(np.int64)
    trav = ~over[both]
    assert ref.cand[both[trav], ids[trav]].all(), f"{what}: a triangle outside the gap of float64's least t"
    err = sc.t_error(hits["t"][both], ref.f64["t"][both]).max(initial=0.0)
    # t is the least float32 t over the stored instances of the triangles within the gap
    rows = both[trav]
    rr, tt = np.nonzero(ref.cand[rows])
    least = np.full(rows.size, np.inf, F)
    for sel, (t, u, v, f) in _best_over_instances(tree, ref.rays, ref.radii, rows[rr], tt):
        np.minimum.at(least, rr[sel], np.where(np.isnan(t), F(np.inf), t))
    assert (_bits(least) == _bits(hits["t"][rows])).all(), f"{what}: t is not the least float32 t of the nearest triangles"
    kinds = np.bincount(feats[both], minlength=5)
    print(f"{what}: {int(hit.sum())} hits of {hit.size}, unstable {100 * ref.unstable_share:.3f} %, face / edge / corner / "
          f"overlap {kinds[1:].tolist()}, max t error {err:.3g}")
    if name:
        assert ref.unstable_share <= sc.CAP[name], what
        assert (kinds[1:] > 20).all(), what
        assert err <= sc.GPU_TOL_FACTOR * sc.T_TOL[name], f"{what}: t is {err:.3g} from float64's"
    return hit


def _check_any(tree, hits, feats, ref, closest, what):
    hit = _check_records(tree, hits, feats, ref.rays, ref.radii, what)
    assert (hit == (closest["primitive_id"] != sc.MISS)).all(), f"{what}: any-hit and closest-hit differ on hit / miss"
    assert (hits["t"][hit] >= closest["t"][hit]).all(), what
    st = ref.stable
    assert (hit[st] == ref.f64["hit"][st]).all(), what


@pytest.fixture(scope="module")
def built(rt):
    """the three scenes on the four trees, built and read back once"""
    cache = {}

    def get(name, tree):
        if (name, tree) not in cache:
            cache[name, tree] = Tree(rt, sc.scene(name), tree)
        return cache[name, tree]
    return get


# ------------------------------------------------------------------ 1: closest hit
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("seed", sc.SEEDS)
@pytest.mark.parametrize("name", sc.SCENES)
def test_closest_hit(built, name, seed, tree):
    tr = built(name, tree)
    ref = sc.reference(name, seed)
    assert tr.M >= sc.scene_M(ref.tris), "the root run bounds the scene's vertices"
    hits, feats, ctr = tr.cast(ref.rays, ref.radii, counters=True)
    hit = _check_closest(tr, hits, feats, ref, f"{name} {tree} seed {seed}", name)
    assert ctr[0] > 0 and ctr[1] >= hit.sum()


# ------------------------------------------------------------------ 2: any hit
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", sc.SCENES)
def test_any_hit(built, name, tree):
    tr = built(name, tree)
    ref = sc.reference(name, sc.SEEDS[0])
    closest, cf, _ = tr.cast(ref.rays, ref.radii)
    hits, feats, _ = tr.cast(ref.rays, ref.radii, any_hit=True)
    _check_any(tr, hits, feats, ref, closest, f"{name} {tree} any-hit")
    # a window that ends one ulp before a travelling closest hit holds no contact at all
    pick = np.flatnonzero((closest["primitive_id"] != sc.MISS) & (cf != sc.OVERLAP) & (closest["t"] > ref.rays["tmin"]))
    assert pick.size > 500
    cut = ref.rays[pick].copy()
    cut["tmax"] = np.nextafter(closest["t"][pick], F(0))
    for any_hit in (False, True):
        again, af, _ = tr.cast(cut, ref.radii[pick], any_hit=any_hit)
        assert (again["primitive_id"] == sc.MISS).all() and (af == sc.NONE).all(), \
            f"{name} {tree}: a contact before the closest one under tmax = nextafter(t, 0)"


# ------------------------------------------------------------------ 3: overlap rows against the range query
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", sc.SCENES)
def test_overlap_rows_are_the_range_querys(rt, built, name, tree):
    import torch
    tr = built(name, tree)
    ref = sc.reference(name, sc.SEEDS[1])
    n = ref.rays.shape[0]
    q = np.zeros(n, rt.POINT_QUERY)
    q["p"] = ref.rays["origin"] + ref.rays["tmin"][:, None] * ref.rays["dir"]
    q["dist2_max"] = ref.radii * ref.radii
    assert q["p"].dtype == F and q["dist2_max"].dtype == F
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rt.RangeCount(tr.inp.triangles_out, tr.inp.nodes_out, tr.root, tr.count, rt.to_device(q).view(torch.float32), off)
    torch.cuda.synchronize()
    touched = np.diff(off.cpu().numpy()) > 0
    for any_hit in (False, True):
        hits, feats, _ = tr.cast(ref.rays, ref.radii, any_hit=any_hit)
        over = feats == sc.OVERLAP
        pos = ref.radii > 0
        assert not (over & ~touched).any(), "an overlap record where the range query counts no triangle"
        assert not (over & ~pos).any(), "a ray of radius 0 never overlaps"
        assert over.sum() > 300
        if any_hit:        # (an any-hit ray may end at a travelling contact of a triangle it meets before the one it overlaps)
            continue
        st = ref.stable & pos
        assert (over[st] == touched[st]).all(), f"{name} {tree}: overlap rows differ from the range query's on stable rays"
        # (an unstable ray may touch at tmin and still report a travelling contact at the same t: ties go to the later part)
        assert ((over != touched) & pos).sum() <= (~ref.stable).sum()


# ------------------------------------------------------------------ 4: uniform radius, no feature buffer
def test_uniform_radius_and_no_features(built):
    tr = built("sheet", "sah_pairs")
    ref = sc.reference("sheet", sc.SEEDS[0])
    n = ref.rays.shape[0]
    for radius in (0.0, 0.03125, 0.7, 40.0):
        for any_hit in (False, True):
            a, fa, ca = tr.cast(ref.rays, np.full(n, radius, F), counters=True, any_hit=any_hit)
            b, fb, cb = tr.cast(ref.rays, None, radius=radius, counters=True, any_hit=any_hit)
            assert a.tobytes() == b.tobytes() and fa.tobytes() == fb.tobytes() and (ca[:2] == cb[:2]).all(), radius
            c, fc, _ = tr.cast(ref.rays, None, radius=radius, features=False, any_hit=any_hit)
            assert fc is None and c.tobytes() == a.tobytes()
            _check_records(tr, a, fa, ref.rays, np.full(n, radius, F), f"uniform radius {radius}")
        assert (a["primitive_id"] != sc.MISS).sum() > 100


# ------------------------------------------------------------------ 5: counters and index lists
def test_counters_and_index_list(rt, built):
    import torch
    tr = built("soup", "bottom_up")
    ref = sc.reference("soup", sc.SEEDS[0])
    n = ref.rays.shape[0]
    rays = _dev_rays(rt, ref.rays)
    radii = rt.to_device(ref.radii).view(torch.float32)
    for any_hit in (False, True):
        plain, pf, c1 = tr.cast(ref.rays, ref.radii, counters=True, any_hit=any_hit)
        again, af, c2 = tr.cast(ref.rays, ref.radii, counters=True, any_hit=any_hit)
        assert plain.tobytes() == again.tobytes() and pf.tobytes() == af.tobytes()
        assert (c1[:2] == c2[:2]).all() and c1[0] > 0 and c1[1] > 0
        # counters are added to: two launches into one buffer give the sum
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        hits = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
        feats = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
        tr.launch(rays, hits, radii=radii, features=feats, counters=ctr, any_hit=any_hit)
        tr.launch(rays, hits, radii=radii, features=feats, counters=ctr, any_hit=any_hit)
        torch.cuda.synchronize()
        both = ctr.cpu().numpy().astype(np.uint64)
        assert (both[:2] == 2 * c1[:2]).all() and (both[2:] > c1[2:]).all()
        perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
        order = rt.to_device(perm).view(torch.int32)
        hits.fill_(-7.0)
        ctr.zero_()
        tr.launch(rays, hits, radii=radii, features=feats, order=order, counters=ctr, any_hit=any_hit)
        torch.cuda.synchronize()
        assert hits.cpu().numpy().view(rt.HIT).reshape(-1).tobytes() == plain.tobytes()
        assert feats.cpu().numpy().view(np.uint32).tobytes() == pf.tobytes()
        assert (ctr.cpu().numpy().astype(np.uint64)[:2] == c1[:2]).all()
        # a partial list with out-of-range entries, and num_indices shorter than the list
        lst = perm[:1000].copy()
        lst[::7] = np.uint32(n) + np.arange(lst[::7].size, dtype=np.uint32) * np.uint32(1 << 20)
        lst[3] = 0xFFFFFFFF
        order = rt.to_device(lst).view(torch.int32)
        hits.fill_(-7.0)
        feats.fill_(POISON)
        tr.launch(rays, hits, radii=radii, features=feats, order=order, num_indices=900, any_hit=any_hit)
        torch.cuda.synchronize()
        got = hits.cpu().numpy().view(rt.HIT).reshape(-1)
        gf = feats.cpu().numpy().view(np.uint32)
        listed = np.zeros(n, bool)
        listed[lst[:900][lst[:900] < n]] = True
        assert got[listed].tobytes() == plain[listed].tobytes() and (gf[listed] == pf[listed]).all()
        assert (got[~listed].view(F) == F(-7.0)).all() and (gf[~listed] == POISON).all(), "an unlisted record was written"


@pytest.mark.parametrize("tree", ("bottom_up", "sah_splits"))
def test_sorted_order_gives_the_same_records(rt, built, tree):
    import torch
    tr = built("far", tree)
    ref = sc.reference("far", sc.SEEDS[1])
    n = ref.rays.shape[0]
    rays = _dev_rays(rt, ref.rays)
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    scratch = rt.device_bytes(rt.RaySortScratchBytes(n))
    assert rt.SortRays(tr.inp.nodes_out, tr.root, tr.count, rays, order, scratch) == n
    assert sorted(order.cpu().numpy().view(np.uint32).tolist()) == list(range(n))
    plain, pf, c1 = tr.cast(ref.rays, ref.radii, counters=True)
    hits = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    feats = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    tr.launch(rays, hits, radii=rt.to_device(ref.radii).view(torch.float32), features=feats, order=order, counters=ctr)
    torch.cuda.synchronize()
    assert hits.cpu().numpy().view(rt.HIT).reshape(-1).tobytes() == plain.tobytes()
    assert feats.cpu().numpy().view(np.uint32).tobytes() == pf.tobytes()
    assert (ctr.cpu().numpy().astype(np.uint64)[:2] == c1[:2]).all()


# ------------------------------------------------------------------ 6: small trees, a pair leaf, a huge ball
SMALL = np.array([[0.1, -0.2, 0.3, 0.9, 0.4, 0.3, 0.2, 0.7, -0.1], [1.2, 0.1, -0.1, 1.6, 0.5, 0.2, 1.1, 0.6, 0.4],
                  [-0.9, 0.8, 0.2, -0.2, 1.4, -0.5, -0.6, 0.3, 0.6], [0.3, 0.3, 1.5, 0.9, -0.3, 1.1, 0.2, -0.4, 1.3],
                  [0.2, -1.1, -0.4, -0.6, -1.3, 0.2, 0.1, -0.7, 0.5]], F)


def _small_ref(tris, seed, n=768):
    return sc.Reference(tris, *sc.make_rays(tris, seed, n))


@pytest.mark.parametrize("tree", TREES)
def test_few_triangles(rt, tree):
    for count in (1, 2, 3, 5):
        tris = SMALL[:count]
        tr = Tree(rt, tris, tree)
        ref = _small_ref(tris, 40 + count)
        closest, cf, _ = tr.cast(ref.rays, ref.radii)
        hit = _check_closest(tr, closest, cf, ref, f"{count} triangles {tree}")
        assert hit.sum() > 20
        hits, feats, _ = tr.cast(ref.rays, ref.radii, any_hit=True)
        _check_any(tr, hits, feats, ref, closest, f"{count} triangles {tree} any-hit")


class _Buffers:
    def __init__(self, triangles_out, nodes_out):
        self.triangles_out, self.nodes_out = triangles_out, nodes_out


@pytest.mark.parametrize("rots", ((0, 0), (1, 2), (2, 1)))
def test_one_pair_leaf(rt, rots):
    """a hand-made tree: one root slot, one leaf holding A = (v0, v1, v2) and B = (v2, v1, v3) with the given rotations"""
    v = np.array([[0, 0, 0], [1, 0, 0.1], [0, 1, 0.05], [1, 1, 0.3]], F)
    stored = [v[[0, 1, 2]], v[[2, 1, 3]]]
    # the caller's corners: the stored ones un-rotated (rotation 1: (c0, c1, c2) = (s1, s2, s0); 2: (s2, s0, s1))
    caller = [s[{0: [0, 1, 2], 1: [1, 2, 0], 2: [2, 0, 1]}[r]] for s, r in zip(stored, rots)]
    quad = np.ascontiguousarray(np.array(caller, F).reshape(2, 9))
    leaves = np.zeros(1, rt.TRIANGLE_PAIR)
    leaves["v0"], leaves["v1"], leaves["v2"], leaves["v3"] = v
    leaves["primitive_id_0"], leaves["primitive_id_1"], leaves["rotations"] = 0, 1, rots
    nodes = np.zeros(2, rt.NODE)
    nodes["min"][0], nodes["max"][0] = v.min(axis=0), v.max(axis=0)
    nodes["w12"][0], nodes["w28"][0] = 1 << 29, 2 << 29          # count 1: triangle B is there; type 2: a leaf, index 0
    tr = Tree(rt, quad, "hand", built=(_Buffers(rt.to_device(leaves), rt.to_device(nodes)), 0, 1))
    assert tr.prims.tolist() == [0, 1] and tr.rots.tolist() == list(rots)
    ref = _small_ref(quad, 61)
    closest, cf, ctr = tr.cast(ref.rays, ref.radii, counters=True)
    hit = _check_closest(tr, closest, cf, ref, f"pair leaf {rots}")
    assert hit.sum() > 50 and set(closest["primitive_id"][hit].tolist()) == {0, 1}
    assert ctr[1] <= sc.traced(ref.rays, ref.radii).sum(), "one test per leaf visited"
    hits, feats, _ = tr.cast(ref.rays, ref.radii, any_hit=True)
    _check_any(tr, hits, feats, ref, closest, f"pair leaf {rots} any-hit")


@pytest.mark.parametrize("tree", ("bottom_up", "sah_pairs"))
def test_a_ball_larger_than_the_scene(built, tree):
    tr = built("soup", tree)
    ref = sc.reference("soup", sc.SEEDS[0])
    rays = ref.rays[:512].copy()
    _, _, mid, ext = sc.scene_box(ref.tris)
    # from far outside, towards the scene: the ball (ten scene sizes) meets the scene's hull; and from inside: overlap
    rays["origin"][:256] = (mid + 100.0 * ext * np.array([0.6, -0.64, 0.48])).astype(F)
    rays["dir"][:256] = (mid - rays["origin"][:256].astype(np.float64)) / 50.0
    rays["tmin"], rays["tmax"] = 0, np.inf
    radii = np.full(512, 10.0 * ext, F)
    small = sc.Reference(ref.tris, rays, radii)
    hits, feats, _ = tr.cast(rays, radii)
    _check_closest(tr, hits, feats, small, f"huge ball {tree}")
    assert (feats[:256] != sc.NONE).all() and (feats[:256] != sc.OVERLAP).all() and (feats[256:] == sc.OVERLAP).all()
    assert (np.abs(hits["t"][:256] - 45.0) < 1.0).all()


# ------------------------------------------------------------------ 7: invalid radii, degenerate rays, batch edges, the empty tree
def test_invalid_radii_inside_a_batch(built):
    tr = built("soup", "sah")
    ref = sc.reference("soup", sc.SEEDS[0])
    radii = ref.radii.copy()
    bad = np.arange(5, radii.size, 11)
    radii[bad] = np.resize(np.array([-1.0, np.nan, np.inf, -np.inf, -1e-30], F), bad.size)
    good = np.ones(radii.size, bool)
    good[bad] = False
    for any_hit in (False, True):
        full, ff, cf = tr.cast(ref.rays, ref.radii, counters=True, any_hit=any_hit)
        hits, feats, ctr = tr.cast(ref.rays, radii, counters=True, any_hit=any_hit)
        assert hits[good].tobytes() == full[good].tobytes() and (feats[good] == ff[good]).all()
        assert (hits["primitive_id"][bad] == sc.MISS).all() and (hits["t"][bad] == np.inf).all() and (feats[bad] == sc.NONE).all()
        only, _, cb = tr.cast(ref.rays[bad], radii[bad], counters=True, any_hit=any_hit)
        assert cb[0] == 0 and cb[1] == 0 and (only["primitive_id"] == sc.MISS).all(), "a ray that is not traced counts no test"
        rest, _, cg = tr.cast(ref.rays[good], ref.radii[good], counters=True, any_hit=any_hit)
        assert (ctr[:2] == cg[:2]).all() and rest.tobytes() == full[good].tobytes()


def test_degenerate_rays_and_batch_edges(rt, built):
    import torch
    tr = built("sheet", "bottom_up")
    ref = sc.reference("sheet", sc.SEEDS[0])
    nan = F(np.nan)
    deg = ref.rays[:7].copy()
    deg["origin"][0, 0] = nan
    deg["dir"][1, 1] = nan
    deg["tmin"][2], deg["tmax"][2] = 5.0, 1.0
    deg["tmin"][3], deg["tmax"][3] = 1e-5, 0.0
    deg["tmin"][4] = nan
    deg["tmax"][5] = nan
    deg["dir"][6] = nan
    for any_hit in (False, True):
        for radius in (0.0, 0.5, 100.0):
            hits, feats, ctr = tr.cast(deg, None, radius=radius, counters=True, any_hit=any_hit)
            assert (hits["primitive_id"] == sc.MISS).all() and (hits["t"] == np.inf).all() and (feats == sc.NONE).all()
            assert ctr[0] == 0 and ctr[1] == 0, "a ray that is not traced counts no test"
    # a ray without a direction is traced: it touches what it overlaps and nothing else
    still = ref.rays[2048:2112].copy()          # (origins inside the scene's box)
    still["dir"] = 0
    still["tmin"], still["tmax"] = 0, np.inf
    radii = np.resize(np.array([0, 0.01, 0.5, 3.0], F), 64)
    hits, feats, _ = tr.cast(still, radii)
    _check_records(tr, hits, feats, still, radii, "rays without a direction")
    assert set(feats.tolist()) == {sc.NONE, sc.OVERLAP}

    # batch sizes around the wave and the workgroup; records past num_rays are not written
    full, ff, _ = tr.cast(ref.rays, ref.radii)
    d = _dev_rays(rt, ref.rays)
    rd = rt.to_device(ref.radii).view(torch.float32)
    for n in (1, 2, 63, 64, 65, 255, 256, 257):
        hits = torch.full((n + 64, 4), -7.0, dtype=torch.float32, device="cuda")
        feats = torch.full((n + 64,), POISON, dtype=torch.int32, device="cuda")
        tr.launch(d[:n], hits, radii=rd[:n], features=feats)
        torch.cuda.synchronize()
        got, gf = hits.cpu().numpy(), feats.cpu().numpy().view(np.uint32)
        assert got[:n].view(rt.HIT).reshape(-1).tobytes() == full[:n].tobytes() and (gf[:n] == ff[:n]).all(), n
        assert (got[n:] == F(-7.0)).all() and (gf[n:] == POISON).all(), f"num_rays {n}: records past the batch"
    # an empty batch and an empty index list run nothing
    hits = torch.full((4, 4), -7.0, dtype=torch.float32, device="cuda")
    tr.launch(d[:0], hits, radius=1.0)
    tr.launch(d[:4], hits, radius=1.0, order=torch.zeros(4, dtype=torch.int32, device="cuda"), num_indices=0)
    torch.cuda.synchronize()
    assert (hits.cpu().numpy() == F(-7.0)).all()


def test_empty_tree(rt):
    import torch
    rays = sc.reference("sheet", sc.SEEDS[0]).rays[:100]
    for any_hit in (False, True):
        hits = torch.full((100, 4), -7.0, dtype=torch.float32, device="cuda")
        feats = torch.full((100,), POISON, dtype=torch.int32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        rt.SphereCast(None, None, 0, 0, _dev_rays(rt, rays), hits, radius=2.0, features=feats, counters=ctr, any_hit=any_hit)
        torch.cuda.synchronize()
        got = hits.cpu().numpy().view(rt.HIT).reshape(-1)
        assert (got["primitive_id"] == sc.MISS).all() and (got["t"] == np.inf).all() and (feats.cpu().numpy() == 0).all()
        assert (ctr.cpu().numpy()[:2] == 0).all()


# ------------------------------------------------------------------ 8: after a refit
@pytest.mark.parametrize("tree", ("bottom_up", "sah_pairs"))
def test_cast_after_refit(rt, tree):
    import torch
    tris = sc.scene("sheet")
    tr = Tree(rt, tris, tree)
    n = tris.shape[0]
    plan = rt.device_bytes(rt.RefitPlanBytes(n))
    rt.BuildRefitPlan(tr.inp, tr.root, tr.count, plan)
    assert rt.refit_status(plan, n) == 0
    # every grid vertex moved (shared vertices stay shared: the displacement is a function of the position)
    p = tris.reshape(-1, 3).astype(np.float64)
    moved = p + 0.3 * np.stack([np.sin(1.7 * p[:, 2]), np.cos(1.3 * p[:, 0] + 0.5 * p[:, 2]), np.sin(0.9 * p[:, 0])], axis=1)
    moved = np.ascontiguousarray(moved.reshape(-1, 9), F)
    tr.inp.triangles_in.copy_(rt.to_device(moved))
    rt.Refit(tr.inp, tr.root, tr.count, plan)
    torch.cuda.synchronize()
    assert rt.refit_status(plan, n) == 0
    tr.tris = moved
    tr.read_back()
    ref = sc.Reference(moved, *sc.make_rays(moved, 71, 2048))
    closest, cf, _ = tr.cast(ref.rays, ref.radii)
    hit = _check_closest(tr, closest, cf, ref, f"sheet {tree} refitted")
    assert hit.sum() > 800
    hits, feats, _ = tr.cast(ref.rays, ref.radii, any_hit=True)
    _check_any(tr, hits, feats, ref, closest, f"sheet {tree} refitted any-hit")


# ------------------------------------------------------------------ 9: hipGraph
def test_build_and_cast_in_a_hip_graph(rt):
    import torch
    ref = sc.reference("soup", sc.SEEDS[0])
    n = sc.NUM_RAYS
    sets = {"a": ref.radii, "b": np.ascontiguousarray(ref.radii[::-1] * F(0.5))}
    inp = rt.BuildInput.allocate(ref.tris)
    rays = _dev_rays(rt, ref.rays)
    radii = torch.empty(n, dtype=torch.float32, device="cuda")
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    anyh = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    feats = torch.empty((2, n), dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")

    def one_frame():
        ctr.zero_()
        rt.RunBottomUpBuild(inp)
        rt.SphereCast(inp.triangles_out, inp.nodes_out, 0, 2, rays, hits, radii=radii, features=feats[0], counters=ctr)
        rt.SphereCast(inp.triangles_out, inp.nodes_out, 0, 2, rays, anyh, radii=radii, features=feats[1], any_hit=True)

    def load(key):
        radii.copy_(rt.to_device(sets[key]).view(torch.float32))      # rewritten in place: the same buffer

    eager = {}
    for key in ("a", "b"):
        load(key)
        one_frame()
        torch.cuda.synchronize()
        eager[key] = [t.clone() for t in (hits, anyh, feats, ctr)]
    assert not torch.equal(eager["a"][0], eager["b"][0]), "other radii must give other records"

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    tr = None
    for key in ("a", "b", "a"):
        load(key)
        hits.fill_(0)
        anyh.fill_(0)
        feats.fill_(0)
        inp.nodes_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, e in zip((hits, anyh, feats, ctr), eager[key]):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                               e.view(torch.int32) if e.dtype == torch.float32 else e), key
        if tr is None:
            tr = Tree(rt, ref.tris, "bottom_up", built=(inp, 0, 2))
        got = hits.cpu().numpy().view(rt.HIT).reshape(-1)
        gf = feats.cpu().numpy().view(np.uint32)
        if key == "a":
            _check_closest(tr, got, gf[0], ref, f"graph replay {key}", "soup")
            _check_any(tr, anyh.cpu().numpy().view(rt.HIT).reshape(-1), gf[1], ref, got, f"graph replay {key} any-hit")
        else:
            _check_records(tr, got, gf[0], ref.rays, sets[key], f"graph replay {key}")
