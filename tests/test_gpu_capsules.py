"""GPU tests of capsule primitives (rt_prepare_capsules + any builder over the proxies + rt_intersect_rays_capsules) against
tests/capsule_ref.py, the numpy restatement of the header (tests/test_capsule_ref_cpu.py checks that reference on its own).

1. prepare: proxies bit-exact against the reference, denormal and 1e30 inputs included; every kind of invalid capsule flagged
   and given the point proxy;
2. closest hit, per scene x seed x {bottom_up, hybrid, sah}: every hit's t, u and v equal the float32 formula for the reported capsule
   and the ray's original window bit for bit; t is never below the dense float32 minimum; on float64-stable rays hit / miss and
   the (canonical) capsule are float64's and t is within GPU_TOL_FACTOR x capsule_ref.T_TOL of float64's (rays only the gap rule
   calls unstable are held to t too); the unstable share is within the cap; the invalid capsules placed in every scene are
   never hit;
3. any hit: hits exactly where the closest-hit query hits, a genuine float32 record; tmax = nextafter(t, 0) of a near-root
   closest hit misses that capsule;
4. counters and the index list: sums equal across launches and across a permutation, indexed records equal unindexed ones,
   unlisted records untouched, an index >= num_rays does nothing;
5. rt_sort_rays's order on the capsule tree, fed to `order`: the same records;
6. moving capsules: prepare into the same proxies, refit through a plan built once (and a rebuild), check 2 again;
7. small and degenerate cases;
8. prepare + LBVH build + query in one HIP graph, replayed after the capsule buffer is rewritten in place."""
import numpy as np
import pytest

import capsule_ref as cr

pytestmark = pytest.mark.gpu

KINDS = ("bottom_up", "hybrid", "sah")
F = np.float32


# ------------------------------------------------------------------ plumbing
class Capsules:
    """device buffers of one capsule scene: capsules, proxies (the build input), status, the tree"""

    def __init__(self, rt, capsules, kind="bottom_up"):
        import torch
        self.rt, self.kind = rt, kind
        self.n = capsules.shape[0]
        self.capsules = rt.to_device(np.ascontiguousarray(capsules, F)) if self.n else rt.device_bytes(64)
        self.tree = rt.BuildInput.allocate(np.zeros((max(self.n, 1), 9), F), sah=kind == "sah")
        self.tree.num_triangles = self.n
        self.status = torch.zeros(4, dtype=torch.uint8, device="cuda")

    def upload(self, capsules):
        assert capsules.shape[0] == self.n
        self.capsules.copy_(self.rt.to_device(np.ascontiguousarray(capsules, F)))   # in place: the same buffer

    def prepare(self, stream=None):
        self.rt.PrepareCapsules(self.capsules, self.n, self.tree.triangles_in, self.status, stream=stream)

    def build(self, stream=None):
        rt = self.rt
        if self.kind == "sah":
            rt.RunSahBuild(self.tree, rt.Arguments(build_type=rt.kSAH), stream=stream)
        else:
            hyb = self.kind == "hybrid"
            rt.RunBottomUpBuild(self.tree, rt.Arguments(build_type=rt.kHybrid if hyb else rt.kBottomUp), hybrid=hyb,
                                stream=stream)

    @property
    def root(self):
        if self.kind == "sah":
            return 0, 1
        return (2 * max(self.n, 1) + 1 if self.kind == "hybrid" else 0), 2

    def frame(self, stream=None):
        self.prepare(stream)
        self.build(stream)
        return self

    def query(self, rays, hits, num_capsules=None, **kw):
        root, count = self.root
        self.rt.IntersectRaysCapsules(self.tree.triangles_out, self.tree.nodes_out, root, count, self.capsules,
                                      self.n if num_capsules is None else num_capsules, rays, hits, **kw)

    def run(self, rays, counters=False, **kw):
        """numpy RAY array -> (HIT array, counters)"""
        import torch
        rt = self.rt
        d = _dev_rays(rt, rays)
        hits = torch.empty((d.shape[0], 4), dtype=torch.float32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda") if counters else None
        self.query(d, hits, counters=ctr, **kw)
        torch.cuda.synchronize()
        h = hits.cpu().numpy().view(rt.HIT).reshape(-1)
        return (h, ctr.cpu().numpy().astype(np.uint64)) if counters else h

    def host_proxies(self):
        return self.rt.to_host(self.tree.triangles_in, F, 9 * self.n).reshape(-1, 9)


def _dev_rays(rt, rays):
    import torch
    return rt.to_device(np.ascontiguousarray(rays, rt.RAY)).view(torch.float32).view(-1, 8)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _check_records(hits, ref, what, rays=None):
    """every record is the miss record or a genuine float32 hit of the reported capsule in the ray's original window"""
    rays = ref.rays if rays is None else rays
    caps = ref.capsules
    hit = hits["primitive_id"] != cr.MISS
    miss = hits[~hit]
    assert (miss["t"] == np.inf).all() and (_bits(miss["u"]) == 0).all() and (_bits(miss["v"]) == 0).all(), what
    ids = hits["primitive_id"][hit].astype(np.int64)
    assert (ids < caps.shape[0]).all(), what
    assert cr.valid(caps)[ids].all(), f"{what}: an invalid capsule was hit"
    t, far, v = cr.pair_f32(rays[hit], caps, ids)
    assert not np.isnan(t).any(), f"{what}: a reported capsule is not hit by its ray in float32"
    assert (_bits(hits["t"][hit]) == _bits(t)).all(), f"{what}: t is not the float32 formula's"
    assert (_bits(hits["u"][hit]) == _bits(far.astype(F))).all(), f"{what}: u is not the far-root flag"
    assert (_bits(hits["v"][hit]) == _bits(v)).all(), f"{what}: v is not the float32 formula's"
    return hit


def _check_closest(hits, ref, what, name=None):
    hit = _check_records(hits, ref, what)
    assert (hits["t"] >= ref.t32).all(), f"{what}: a t below the dense float32 minimum"
    st = ref.stable
    held = ref.same & hit & ref.f64["hit"]          # stable, or unstable by the gap rule alone: held to t
    err = cr.t_error(hits["t"][held], ref.f64["t"][held]).max(initial=0.0)
    print(f"{what}: {int(hit.sum())} hits of {hit.size}, unstable {100 * ref.unstable_share:.3f} %, "
          f"far roots {int((hits['u'] == 1).sum())}, body {int(((hits['v'] > 0) & (hits['v'] < 1)).sum())}, max t error {err:.3g}")
    assert ref.unstable_share <= (cr.CAP[name] if name else 0.01), what
    assert (hit[st] == ref.f64["hit"][st]).all(), f"{what}: hit / miss differs from float64 on a stable ray"
    both = st & hit
    assert (ref.canon[hits["primitive_id"][both]] == ref.f64["id"][both]).all(), f"{what}: another capsule than float64's"
    assert ((hits["u"][both] == 1) == ref.f64["far"][both]).all(), f"{what}: another root than float64's"
    if name:
        assert err <= cr.GPU_TOL_FACTOR * cr.T_TOL[name], f"{what}: t is {err:.3g} from float64's"


def _check_any(hits, ref, what, closest=None):
    hit = _check_records(hits, ref, what)
    st = ref.stable
    assert (hit[st] == ref.f64["hit"][st]).all(), f"{what}: any-hit differs from float64 on a stable ray"
    assert (hit <= (ref.t32 < np.inf)).all(), f"{what}: any-hit hits where no capsule is hit in float32"
    if closest is not None:
        assert (hit == (closest["primitive_id"] != cr.MISS)).all(), f"{what}: any-hit and closest-hit differ on hit / miss"
        assert (hits["t"][hit] >= closest["t"][hit]).all(), what


@pytest.fixture(scope="module")
def built(rt):
    """the three scenes on the three builders, prepared and built once"""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            cache[name, kind] = Capsules(rt, cr.gpu_scene(name), kind).frame()
        return cache[name, kind]
    return get


# ------------------------------------------------------------------ 1: prepare
def test_prepare_is_bit_exact(rt):
    extreme = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [-1, -2, -3, 0, 1, 2, 3, 0], [1e30, -1e30, 3e29, 1e30, -1e30, 1e30, 0, 0],
                        [1e-30, 2e-30, -1e-30, 1e-31, 3e-30, -2e-30, 1e-30, 0], [1e-40, -1e-41, 0, 1e-42, 2e-40, 1e-41, 1e-44, 0],
                        [1e-35, 0, 0, 1e-36, 0, 1e-35, 0, 0], [5, 5, 5, 1e30, 6, 6, 6, 0], [3e38, 0, 0, 1, -3e38, 0, 0, 0],
                        [1, 2, 3, 1e-45, 1, 2, 3, 0], [123456.789, -0.001, 77.7, 0.5, 123456.5, 0.001, 77.9, 0]], F)
    for name, c in [(n, cr.gpu_scene(n)) for n in cr.SCENES] + [("extreme", extreme)]:
        sc = Capsules(rt, c)
        sc.status.fill_(0xFF)
        sc.prepare()
        exp, ok, status = cr.prepare_f32(c)
        got = sc.host_proxies()
        assert np.isfinite(exp).all(), name
        assert (_bits(got) == _bits(exp)).all(), f"{name}: proxies differ from the reference"
        assert rt.capsule_status(sc.status) == status == (cr.RT_CAPSULE_BAD if name != "extreme" else 0)
        assert (got[~ok] == 0).all()
    # every kind of invalid capsule on its own; the pad word is never read
    for bad in ((np.nan, 0, 0, 1, 1, 0, 0, 0), (0, np.inf, 0, 1, 1, 0, 0, 0), (0, 0, 0, 1, np.nan, 0, 0, 0),
                (0, 0, 0, 1, 0, 0, -np.inf, 0), (0, 0, 0, -1e-30, 1, 0, 0, 0), (0, 0, 0, np.nan, 1, 0, 0, 0),
                (0, 0, 0, np.inf, 1, 0, 0, 0), (0, 0, 0, -np.inf, 1, 0, 0, 0)):
        c = np.array([[1, 2, 3, 0.5, 2, 2, 2, np.nan], bad, [4, 5, 6, 0.25, 4, 5, 7, np.inf]], F)
        sc = Capsules(rt, c)
        sc.prepare()
        got = sc.host_proxies()
        assert rt.capsule_status(sc.status) == rt.RT_CAPSULE_BAD, bad
        assert (_bits(got) == _bits(cr.prepare_f32(c)[0])).all() and (_bits(got[1]) == 0).all(), bad
        assert (got[0] != 0).any() and (got[2] != 0).any()
    # an empty batch still clears the word
    sc = Capsules(rt, np.zeros((0, 8), F))
    sc.status.fill_(0xFF)
    sc.prepare()
    assert rt.capsule_status(sc.status) == 0


# ------------------------------------------------------------------ 2: closest hit
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", cr.SEEDS)
@pytest.mark.parametrize("name", cr.SCENES)
def test_closest_hit(built, name, seed, kind):
    sc = built(name, kind)
    ref = cr.reference(name, seed)
    hits, ctr = sc.run(ref.rays, counters=True)
    _check_closest(hits, ref, f"{name} {kind} seed {seed}", name)
    assert ctr[0] > 0 and ctr[1] >= (hits["primitive_id"] != cr.MISS).sum()


# ------------------------------------------------------------------ 3: any hit
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", cr.SCENES)
def test_any_hit(built, name, kind):
    sc = built(name, kind)
    ref = cr.reference(name, cr.SEEDS[0])
    closest = sc.run(ref.rays)
    _check_any(sc.run(ref.rays, any_hit=True), ref, f"{name} {kind} any-hit", closest)
    # a window that ends one ulp before a near-root hit misses that capsule
    pick = np.flatnonzero((closest["primitive_id"] != cr.MISS) & (closest["u"] == 0) & (closest["t"] > 0))
    assert pick.size > 500
    cut = ref.rays[pick].copy()
    cut["tmax"] = np.nextafter(closest["t"][pick], F(0))
    for any_hit in (False, True):
        again = sc.run(cut, any_hit=any_hit)
        same = again["primitive_id"] == closest["primitive_id"][pick]
        assert not same.any(), f"{name} {kind}: a capsule hit at t is hit again under tmax = nextafter(t, 0)"
        _check_records(again, ref, f"{name} {kind} cut window", rays=cut)


# ------------------------------------------------------------------ 4: counters and the index list
def test_counters_and_index_list(rt, built):
    import torch
    sc = built("fibres", "bottom_up")
    ref = cr.reference("fibres", cr.SEEDS[0])
    n = ref.rays.shape[0]
    rays = _dev_rays(rt, ref.rays)
    for any_hit in (False, True):
        plain, c1 = sc.run(ref.rays, counters=True, any_hit=any_hit)
        again, c2 = sc.run(ref.rays, counters=True, any_hit=any_hit)
        assert plain.tobytes() == again.tobytes() and (c1[:2] == c2[:2]).all() and c1[0] > 0 and c1[1] > 0
        # counters are added to: two launches into one buffer give the sum
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        hits = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
        sc.query(rays, hits, counters=ctr, any_hit=any_hit)
        sc.query(rays, hits, counters=ctr, any_hit=any_hit)
        torch.cuda.synchronize()
        both = ctr.cpu().numpy().astype(np.uint64)
        assert (both[:2] == 2 * c1[:2]).all() and (both[2:] > c1[2:]).all()
        perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
        order = rt.to_device(perm).view(torch.int32)
        hits.fill_(-7.0)
        ctr.zero_()
        sc.query(rays, hits, order=order, counters=ctr, any_hit=any_hit)
        torch.cuda.synchronize()
        assert hits.cpu().numpy().view(rt.HIT).reshape(-1).tobytes() == plain.tobytes()
        assert (ctr.cpu().numpy().astype(np.uint64)[:2] == c1[:2]).all()
        # a partial list with out-of-range entries, and num_indices shorter than the list
        lst = perm[:1000].copy()
        lst[::7] = np.uint32(n) + np.arange(lst[::7].size, dtype=np.uint32) * np.uint32(1 << 20)
        lst[3] = 0xFFFFFFFF
        order = rt.to_device(lst).view(torch.int32)
        hits.fill_(-7.0)
        sc.query(rays, hits, order=order, num_indices=900, any_hit=any_hit)
        torch.cuda.synchronize()
        got = hits.cpu().numpy().view(rt.HIT).reshape(-1)
        listed = np.zeros(n, bool)
        listed[lst[:900][lst[:900] < n]] = True
        assert got[listed].tobytes() == plain[listed].tobytes()
        assert (got[~listed].view(F) == F(-7.0)).all(), "an unlisted record was written"


# ------------------------------------------------------------------ 5: rt_sort_rays's order
@pytest.mark.parametrize("kind", KINDS)
def test_sorted_order_gives_the_same_records(rt, built, kind):
    import torch
    sc = built("far", kind)
    ref = cr.reference("far", cr.SEEDS[1])
    n = ref.rays.shape[0]
    rays = _dev_rays(rt, ref.rays)
    root, count = sc.root
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    scratch = rt.device_bytes(rt.RaySortScratchBytes(n))
    assert rt.SortRays(sc.tree.nodes_out, root, count, rays, order, scratch) == n
    live = rt.ray_sort_live(scratch, n)
    assert live == n and sorted(order.cpu().numpy().view(np.uint32).tolist()) == list(range(n))
    plain, c1 = sc.run(ref.rays, counters=True)
    hits = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    sc.query(rays, hits, order=order, counters=ctr)
    torch.cuda.synchronize()
    assert hits.cpu().numpy().view(rt.HIT).reshape(-1).tobytes() == plain.tobytes()
    assert (ctr.cpu().numpy().astype(np.uint64)[:2] == c1[:2]).all()


# ------------------------------------------------------------------ 6: moving capsules
@pytest.mark.parametrize("kind", KINDS)
def test_moving_capsules_refit_and_rebuild(rt, kind):
    import torch
    seed = cr.SEEDS[0]
    sc = Capsules(rt, cr.gpu_scene("fibres"), kind).frame()
    root, count = sc.root
    plan = rt.device_bytes(rt.RefitPlanBytes(sc.n))
    rt.BuildRefitPlan(sc.tree, root, count, plan)
    assert rt.refit_status(plan, sc.n) == 0
    for step in (1, 2):
        ref = cr.reference("fibres", seed, step)
        sc.upload(ref.capsules)
        sc.prepare()
        rt.Refit(sc.tree, root, count, plan)
        torch.cuda.synchronize()
        assert rt.refit_status(plan, sc.n) == 0 and rt.capsule_status(sc.status) == rt.RT_CAPSULE_BAD
        closest = sc.run(ref.rays)
        _check_closest(closest, ref, f"fibres {kind} refit step {step}", "fibres")
        _check_any(sc.run(ref.rays, any_hit=True), ref, f"fibres {kind} refit step {step} any-hit", closest)
    ref = cr.reference("fibres", seed, 2)
    sc.build()
    _check_closest(sc.run(ref.rays), ref, f"fibres {kind} rebuilt", "fibres")


# ------------------------------------------------------------------ 7: small and degenerate cases
def _small_ref(capsules, seed, n=768):
    return cr.Reference(capsules, cr.make_rays(capsules, seed, n, with_radius=True))


@pytest.mark.parametrize("kind", KINDS)
def test_few_capsules(rt, kind):
    base = np.array([[0.1, -0.2, 0.3, 0.5, 0.6, 0.4, 0.3, 0], [1.2, 0.1, -0.1, 0.4, 1.2, 0.1, -0.1, 0],
                     [-0.9, 0.8, 0.2, 0.3, -0.2, 1.4, -0.5, 0], [0.3, 0.3, 1.5, 0.0, 0.9, -0.3, 1.1, 0],
                     [0.2, -1.1, -0.4, 0.3, -0.6, -1.3, 0.2, 0]], F)
    for count in (1, 2, 3, 5):
        c = base[:count]
        sc = Capsules(rt, c, kind).frame()
        assert rt.capsule_status(sc.status) == 0
        ref = _small_ref(c, 40 + count)
        closest = sc.run(ref.rays)
        _check_closest(closest, ref, f"{count} capsules {kind}")
        _check_any(sc.run(ref.rays, any_hit=True), ref, f"{count} capsules {kind} any-hit", closest)


HAND_CAPSULE = (0, 0, 0, 1, 4, 0, 0, 0)      # axis (0,0,0)-(4,0,0), r = 1
#            origin, direction, (t, u, v) or None for a miss: tests/test_capsule_ref_cpu.py's hand cases, exact in float32
HAND_RAYS = [((2, -5, 0), (0, 1, 0), (4.0, 0.0, 0.5)), ((1, -5, 0), (0, 2, 0), (2.0, 0.0, 0.25)),
             ((3, 0, 0), (0, 0, 1), (1.0, 1.0, 0.75)), ((-5, 0, 0), (1, 0, 0), (4.0, 0.0, 0.0)),
             ((9, 0, 0), (-1, 0, 0), (4.0, 0.0, 1.0)), ((-5, 2, 0), (1, 0, 0), None), ((2, 0, 0), (1, 0, 0), (3.0, 1.0, 1.0)),
             ((2, 0, 0), (-1, 0, 0), (3.0, 1.0, 0.0)), ((0, -5, 0), (0, 1, 0), (4.0, 0.0, 0.0)),
             ((4, -5, 0), (0, 1, 0), (4.0, 0.0, 1.0)), ((-1.5, -5, 0), (0, 1, 0), None)]


@pytest.mark.parametrize("kind", KINDS)
def test_hand_cases(rt, kind):
    # a far second capsule keeps the tree a tree of two leaves
    c = np.array([HAND_CAPSULE, (50, 50, 50, 0.5, 51, 50, 50, 0)], F)
    sc = Capsules(rt, c, kind).frame()
    rays = np.zeros(len(HAND_RAYS) + 1, cr.RAY)
    rays["origin"][:-1] = [r[0] for r in HAND_RAYS]
    rays["dir"][:-1] = [r[1] for r in HAND_RAYS]
    rays["origin"][-1], rays["dir"][-1] = (-5, 0.5, 0), (1, 0, 0)      # parallel at offset 0.5: p0's cap (t is not exact)
    rays["tmax"] = np.inf
    for any_hit in (False, True):
        hits = sc.run(rays, any_hit=any_hit)
        for h, (_, _, want) in zip(hits, HAND_RAYS):
            if want is None:
                assert h["primitive_id"] == cr.MISS and h["t"] == np.inf
            else:
                assert h["primitive_id"] == 0 and (float(h["t"]), float(h["u"]), float(h["v"])) == want
        last = hits[-1]
        assert last["primitive_id"] == 0 and last["u"] == 0 and last["v"] == 0 and abs(last["t"] - (5 - np.sqrt(0.75))) < 1e-6
        t, far, v = cr.pair_f32(rays, c, np.zeros(rays.shape[0], np.int64))
        hit = hits["primitive_id"] == 0
        assert (hit == ~np.isnan(t)).all() and (_bits(hits["t"][hit]) == _bits(t[hit])).all()


@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_scenes(rt, kind):
    # r = 0: hit only by a line through the segment, exactly.  Rays in the z = 0 plane across the x axis, every number of a few
    # bits: each operation of the test is exact.
    c = np.array([[0, 0, 0, 0, 4, 0, 0, 0], [8, 1, 1, 0.5, 8, 2, 1, 0], [0, 5, 0, 0.25, 0, 5, 0, 0]], F)
    sc = Capsules(rt, c, kind).frame()
    rays = np.zeros(4, cr.RAY)
    rays["origin"] = [(1, -2, 0), (3, 1, 0), (1, -2, 0.5), (5, -2, 0)]
    rays["dir"] = [(0, 1, 0), (0, -0.5, 0), (0, 1, 0), (0, 1, 0)]
    rays["tmax"] = np.inf
    hits = sc.run(rays)
    assert hits["primitive_id"].tolist() == [0, 0, cr.MISS, cr.MISS] and hits["t"].tolist()[:2] == [2.0, 2.0]
    assert (hits["u"] == 0).all() and hits["v"].tolist() == [0.25, 0.75, 0, 0]
    ref = _small_ref(c, 51)
    _check_closest(sc.run(ref.rays), ref, f"r = 0 {kind}")

    # two identical capsules (and a third): either copy is the answer
    c = np.array([[0.5, 0.5, 0.5, 0.4, 0.9, 0.1, 0.7, 0], [-1, 0, 0, 0.3, -1.2, 0.4, 0.1, 0], [0.5, 0.5, 0.5, 0.4, 0.9, 0.1, 0.7, 0]], F)
    ref = _small_ref(c, 52)
    sc = Capsules(rt, c, kind).frame()
    closest = sc.run(ref.rays)
    _check_closest(closest, ref, f"identical capsules {kind}")
    _check_any(sc.run(ref.rays, any_hit=True), ref, f"identical capsules {kind} any-hit", closest)

    # one capsule containing all others: rays from inside the big one reach it through a far root
    rng = np.random.default_rng(53)
    p0 = rng.uniform(-1, 1, (40, 3))
    small = cr.pack(p0, rng.uniform(0.05, 0.2, 40), p0 + rng.uniform(-0.3, 0.3, (40, 3)))
    c = np.vstack([small, cr.pack([(-2, 0, 0)], 10, [(2, 0, 0)])]).astype(F)
    ref = cr.Reference(c, cr.make_rays(small, 54, 768))        # (the end-point box: every ray begins inside the big capsule)
    sc = Capsules(rt, c, kind).frame()
    hits = sc.run(ref.rays)
    _check_closest(hits, ref, f"enclosing capsule {kind}")
    far = (hits["primitive_id"] == 40) & (hits["u"] == 1)
    assert far.sum() > 50 and (hits["primitive_id"][ref.stable & (ref.rays["tmax"] == np.inf)] != cr.MISS).all()

    # every capsule invalid: point proxies at the origin, nothing is ever hit
    c = np.array([[np.nan, 0, 0, 1, 1, 0, 0, 0], [0, 0, 0, -1, 1, 0, 0, 0], [0, 0, 0, np.nan, 1, 0, 0, 0],
                  [0, 0, 0, np.inf, 1, 0, 0, 0], [0, 0, 0, 1, np.inf, 0, 0, 0]], F)
    sc = Capsules(rt, c, kind).frame()
    assert rt.capsule_status(sc.status) == rt.RT_CAPSULE_BAD
    rays = np.zeros(64, cr.RAY)
    rays["origin"] = rng.uniform(-1, 1, (64, 3))
    rays["dir"] = -rays["origin"]
    rays["tmax"] = np.inf
    hits, ctr = sc.run(rays, counters=True)
    assert (hits["primitive_id"] == cr.MISS).all() and (hits["t"] == np.inf).all()
    assert ctr[1] <= 2 * 64, "only the two capsules with a non-finite end point pass the radius rule and are tested"


@pytest.mark.parametrize("kind", KINDS)
def test_num_capsules_below_the_leaf_ids(rt, built, kind):
    sc = built("fibres", kind)
    full = cr.reference("fibres", cr.SEEDS[0])
    rays = full.rays[:1024].copy()
    for keep in (700, 1, 0):
        hits, ctr = sc.run(rays, counters=True, num_capsules=keep)
        if keep == 0:
            assert (hits["primitive_id"] == cr.MISS).all() and ctr[1] == 0 and ctr[0] > 0
            continue
        ref = cr.Reference(full.capsules[:keep].copy(), rays)
        assert (hits["primitive_id"][hits["primitive_id"] != cr.MISS] < keep).all()
        _check_closest(hits, ref, f"fibres {kind} num_capsules {keep}")


def test_degenerate_rays_and_batch_edges(rt, built):
    import torch
    sc = built("strand", "bottom_up")
    ref = cr.reference("strand", cr.SEEDS[0])
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
        hits, ctr = sc.run(deg, counters=True, any_hit=any_hit)
        assert (hits["primitive_id"] == cr.MISS).all() and (hits["t"] == np.inf).all() and (hits["u"] == 0).all()
        assert ctr[0] == 0 and ctr[1] == 0, "a ray that is not traced counts no test"
    # a ray without a direction is traced and hits nothing, even from inside a capsule
    still = ref.rays[:4].copy()
    still["origin"] = ref.capsules[:4, :3]
    still["dir"] = 0
    still["tmin"], still["tmax"] = 0, np.inf
    hits = sc.run(still)
    assert (hits["primitive_id"] == cr.MISS).all() and (hits["t"] == np.inf).all()

    # batch sizes around the wave and the workgroup; records past num_rays are not written
    full = sc.run(ref.rays)
    d = _dev_rays(rt, ref.rays)
    for n in (1, 63, 64, 65, 257):
        hits = torch.full((n + 64, 4), -7.0, dtype=torch.float32, device="cuda")
        sc.query(d[:n], hits)
        torch.cuda.synchronize()
        got = hits.cpu().numpy()
        assert got[:n].view(rt.HIT).reshape(-1).tobytes() == full[:n].tobytes(), n
        assert (got[n:] == F(-7.0)).all(), f"num_rays {n}: records past the batch"
    # an empty batch and an empty index list run nothing
    hits = torch.full((4, 4), -7.0, dtype=torch.float32, device="cuda")
    sc.query(d[:0], hits)
    sc.query(d[:4], hits, order=torch.zeros(4, dtype=torch.int32, device="cuda"), num_indices=0)
    torch.cuda.synchronize()
    assert (hits.cpu().numpy() == F(-7.0)).all()


def test_empty_tree(rt):
    import torch
    sc = Capsules(rt, np.zeros((0, 8), F))
    sc.prepare()
    rays = cr.reference("strand", cr.SEEDS[0]).rays[:100]
    hits = torch.full((100, 4), -7.0, dtype=torch.float32, device="cuda")
    rt.IntersectRaysCapsules(None, None, 0, 0, None, 0, _dev_rays(rt, rays), hits)      # count = 0: the empty tree
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(rt.HIT).reshape(-1)
    assert (got["primitive_id"] == cr.MISS).all() and (got["t"] == np.inf).all()


# ------------------------------------------------------------------ 8: hipGraph
def test_prepare_build_and_query_in_a_hip_graph(rt):
    import torch
    seed = cr.SEEDS[0]
    refs = {"a": cr.reference("fibres", seed), "b": cr.reference("fibres", seed, 1)}
    sc = Capsules(rt, refs["a"].capsules, "bottom_up")
    n = cr.NUM_RAYS
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    anyh = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")

    def one_frame():
        ctr.zero_()
        sc.frame()
        sc.query(rays, hits, counters=ctr)
        sc.query(rays, anyh, any_hit=True)

    def load(key):
        sc.upload(refs[key].capsules)                   # rewritten in place: the same buffers
        rays.copy_(_dev_rays(rt, refs[key].rays))

    eager = {}
    for key in ("a", "b"):
        load(key)
        one_frame()
        torch.cuda.synchronize()
        eager[key] = [t.clone() for t in (hits, anyh, ctr)]
    assert not torch.equal(eager["a"][0], eager["b"][0]), "the moved scene must give other records"

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        one_frame()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            one_frame()
    torch.cuda.current_stream().wait_stream(side)
    for key in ("a", "b", "a"):
        load(key)
        hits.fill_(0)
        anyh.fill_(0)
        sc.tree.nodes_out.zero_()
        sc.status.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        got = hits.cpu().numpy().view(rt.HIT).reshape(-1)
        _check_closest(got, refs[key], f"graph replay {key}", "fibres")
        _check_any(anyh.cpu().numpy().view(rt.HIT).reshape(-1), refs[key], f"graph replay {key} any-hit", got)
        assert rt.capsule_status(sc.status) == rt.RT_CAPSULE_BAD
        for g, e in zip((hits, anyh, ctr), eager[key]):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                               e.view(torch.int32) if e.dtype == torch.float32 else e), key
