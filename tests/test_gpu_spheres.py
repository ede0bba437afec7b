"""GPU tests of sphere primitives (rt_prepare_spheres + any builder over the proxies + rt_intersect_rays_spheres) against
tests/sphere_ref.py, the numpy restatement of the header (tests/test_sphere_ref_cpu.py checks that reference on its own).

1. prepare: proxies bit-exact against the reference; NaN-centre, negative-, NaN- and infinite-radius spheres flagged, point proxies;
2. closest hit, per scene x {bottom_up, hybrid, sah}: every hit's t equals the float32 formula for the reported sphere and the
   ray's original window bit for bit, u is the far-root flag and v is 0; t is never below the dense float32 minimum; on
   float64-stable rays hit / miss and the (canonical) sphere are float64's; the unstable share is within the cap; the invalid
   spheres placed in every scene are never hit;
3. any hit: hits where float64 has a stable hit in the window, misses where it has a stable miss, a genuine float32 record;
   tmax = nextafter(t, 0) of a near-root closest hit misses that sphere;
4. counters and the index list: sums equal across launches and across a permutation, indexed records equal unindexed ones,
   unlisted records untouched, an index >= num_rays does nothing;
5. rt_sort_rays's order on the sphere tree, fed to `order`: the same records;
6. moving spheres: prepare into the same proxies, refit through a plan built once (and a rebuild), check 2 again;
7. small and degenerate cases;
8. prepare + LBVH build + query in one HIP graph, replayed after the sphere buffer is rewritten in place."""
import numpy as np
import pytest

import sphere_ref as sr

pytestmark = pytest.mark.gpu

KINDS = ("bottom_up", "hybrid", "sah")
F = np.float32


# ------------------------------------------------------------------ plumbing
class Spheres:
    """device buffers of one sphere scene: spheres, proxies (the build input), status, the tree"""

    def __init__(self, rt, spheres, kind="bottom_up"):
        import torch
        self.rt, self.kind = rt, kind
        self.n = spheres.shape[0]
        self.spheres = rt.to_device(np.ascontiguousarray(spheres, F)) if self.n else rt.device_bytes(64)
        self.tree = rt.BuildInput.allocate(np.zeros((max(self.n, 1), 9), F), sah=kind == "sah")
        self.tree.num_triangles = self.n
        self.status = torch.zeros(4, dtype=torch.uint8, device="cuda")

    def upload(self, spheres):
        assert spheres.shape[0] == self.n
        self.spheres.copy_(self.rt.to_device(np.ascontiguousarray(spheres, F)))   # in place: the same buffer

    def prepare(self, stream=None):
        self.rt.PrepareSpheres(self.spheres, self.n, self.tree.triangles_in, self.status, stream=stream)

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

    def query(self, rays, hits, num_spheres=None, **kw):
        root, count = self.root
        self.rt.IntersectRaysSpheres(self.tree.triangles_out, self.tree.nodes_out, root, count, self.spheres,
                                     self.n if num_spheres is None else num_spheres, rays, hits, **kw)

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


def _check_records(hits, ref, what):
    """every record is the miss record or a genuine float32 hit of the reported sphere in the ray's original window"""
    rays, spheres = ref.rays, ref.spheres
    hit = hits["primitive_id"] != sr.MISS
    miss = hits[~hit]
    assert (miss["t"] == np.inf).all() and (miss["u"] == 0).all() and (miss["v"] == 0).all(), what
    ids = hits["primitive_id"][hit].astype(np.int64)
    assert (ids < spheres.shape[0]).all(), what
    assert sr.valid(spheres)[ids].all(), f"{what}: an invalid sphere was hit"
    t, far = sr.pair_f32(rays[hit], spheres, ids)
    assert not np.isnan(t).any(), f"{what}: a reported sphere is not hit by its ray in float32"
    assert (_bits(hits["t"][hit]) == _bits(t)).all(), f"{what}: t is not the float32 formula's"
    assert (hits["u"][hit] == far.astype(F)).all() and (_bits(hits["v"][hit]) == 0).all(), what
    return hit


def _check_closest(hits, ref, what):
    hit = _check_records(hits, ref, what)
    assert (hits["t"] >= ref.t32).all(), f"{what}: a t below the dense float32 minimum"
    print(f"{what}: {int(hit.sum())} hits of {hit.size}, unstable {100 * ref.unstable_share:.3f} %, "
          f"far roots {int((hits['u'] == 1).sum())}")
    assert ref.unstable_share <= sr.CAP, what
    st = ref.stable
    assert (hit[st] == ref.f64["hit"][st]).all(), f"{what}: hit / miss differs from float64 on a stable ray"
    both = st & hit
    assert (ref.canon[hits["primitive_id"][both]] == ref.f64["id"][both]).all(), f"{what}: another sphere than float64's"


def _check_any(hits, ref, what):
    hit = _check_records(hits, ref, what)
    st = ref.stable
    assert (hit[st] == ref.f64["hit"][st]).all(), f"{what}: any-hit differs from float64 on a stable ray"
    assert (hit <= (ref.t32 < np.inf)).all(), f"{what}: any-hit hits where no sphere is hit in float32"


@pytest.fixture(scope="module")
def built(rt):
    """the three scenes on the three builders, prepared and built once"""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            cache[name, kind] = Spheres(rt, sr.gpu_scene(name), kind).frame()
        return cache[name, kind]
    return get


# ------------------------------------------------------------------ 1: prepare
def test_prepare_is_bit_exact(rt):
    extreme = np.array([[0, 0, 0, 0], [-0.0, -0.0, -0.0, 0], [1e30, -1e30, 3e29, 1e30], [1e-30, 2e-30, -1e-30, 1e-31],
                        [1e-40, -1e-41, 0, 1e-42], [1e-35, 0, 0, 1e-36], [5, 5, 5, 1e30], [3e38, 0, 0, 1], [1, 2, 3, 1e-45],
                        [123456.789, -0.001, 77.7, 0.5]], F)
    for name, s in [(n, sr.gpu_scene(n)) for n in sr.SCENES] + [("extreme", extreme)]:
        sc = Spheres(rt, s)
        sc.status.fill_(0xFF)
        sc.prepare()
        exp, ok, status = sr.prepare_f32(s)
        got = sc.host_proxies()
        assert np.isfinite(exp).all(), name
        assert (_bits(got) == _bits(exp)).all(), f"{name}: proxies differ from the reference"
        assert rt.sphere_status(sc.status) == status == (sr.RT_SPHERE_BAD if name != "extreme" else 0)
        assert (got[~ok] == 0).all()
    # every kind of invalid sphere on its own
    for bad in ((np.nan, 0, 0, 1), (0, np.inf, 0, 1), (0, 0, -np.inf, 1), (0, 0, 0, -1e-30), (0, 0, 0, np.nan), (0, 0, 0, np.inf),
                (0, 0, 0, -np.inf)):
        s = np.array([[1, 2, 3, 0.5], bad, [4, 5, 6, 0.25]], F)
        sc = Spheres(rt, s)
        sc.prepare()
        got = sc.host_proxies()
        assert rt.sphere_status(sc.status) == rt.RT_SPHERE_BAD, bad
        assert (_bits(got) == _bits(sr.prepare_f32(s)[0])).all() and (_bits(got[1]) == 0).all(), bad
    # an empty batch still clears the word
    sc = Spheres(rt, np.zeros((0, 4), F))
    sc.status.fill_(0xFF)
    sc.prepare()
    assert rt.sphere_status(sc.status) == 0


# ------------------------------------------------------------------ 2: closest hit
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sr.SCENES)
def test_closest_hit(built, name, kind):
    sc = built(name, kind)
    for seed in sr.SEEDS:
        ref = sr.reference(name, seed)
        hits, ctr = sc.run(ref.rays, counters=True)
        _check_closest(hits, ref, f"{name} {kind} seed {seed}")
        assert ctr[0] > 0 and ctr[1] >= (hits["primitive_id"] != sr.MISS).sum()


# ------------------------------------------------------------------ 3: any hit
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sr.SCENES)
def test_any_hit(built, name, kind):
    sc = built(name, kind)
    ref = sr.reference(name, sr.SEEDS[0])
    _check_any(sc.run(ref.rays, any_hit=True), ref, f"{name} {kind} any-hit")
    # a window that ends one ulp before a near-root hit misses that sphere
    closest = sc.run(ref.rays)
    pick = np.flatnonzero((closest["primitive_id"] != sr.MISS) & (closest["u"] == 0) & (closest["t"] > 0))
    assert pick.size > 500
    cut = ref.rays[pick].copy()
    cut["tmax"] = np.nextafter(closest["t"][pick], F(0))
    for any_hit in (False, True):
        again = sc.run(cut, any_hit=any_hit)
        same = again["primitive_id"] == closest["primitive_id"][pick]
        assert not same.any(), f"{name} {kind}: a sphere hit at t is hit again under tmax = nextafter(t, 0)"
        hit = again["primitive_id"] != sr.MISS
        t, far = sr.pair_f32(cut[hit], ref.spheres, again["primitive_id"][hit].astype(np.int64))
        assert (_bits(again["t"][hit]) == _bits(t)).all() and (again["u"][hit] == far.astype(F)).all()


# ------------------------------------------------------------------ 4: counters and the index list
def test_counters_and_index_list(rt, built):
    import torch
    sc = built("cloud", "bottom_up")
    ref = sr.reference("cloud", sr.SEEDS[0])
    n = ref.rays.shape[0]
    rays = _dev_rays(rt, ref.rays)
    for any_hit in (False, True):
        plain, c1 = sc.run(ref.rays, counters=True, any_hit=any_hit)
        again, c2 = sc.run(ref.rays, counters=True, any_hit=any_hit)
        assert plain.tobytes() == again.tobytes() and (c1[:2] == c2[:2]).all() and c1[0] > 0 and c1[1] > 0
        perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
        order = rt.to_device(perm).view(torch.int32)
        hits = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
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
    sc = built("shell", kind)
    ref = sr.reference("shell", sr.SEEDS[1])
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


# ------------------------------------------------------------------ 6: moving spheres
@pytest.mark.parametrize("kind", KINDS)
def test_moving_spheres_refit_and_rebuild(rt, kind):
    import torch
    seed = sr.SEEDS[0]
    sc = Spheres(rt, sr.gpu_scene("cloud"), kind).frame()
    root, count = sc.root
    plan = rt.device_bytes(rt.RefitPlanBytes(sc.n))
    rt.BuildRefitPlan(sc.tree, root, count, plan)
    assert rt.refit_status(plan, sc.n) == 0
    for step in (1, 2):
        ref = sr.reference("cloud", seed, step)
        sc.upload(ref.spheres)
        sc.prepare()
        rt.Refit(sc.tree, root, count, plan)
        torch.cuda.synchronize()
        assert rt.refit_status(plan, sc.n) == 0 and rt.sphere_status(sc.status) == rt.RT_SPHERE_BAD
        _check_closest(sc.run(ref.rays), ref, f"cloud {kind} refit step {step}")
        _check_any(sc.run(ref.rays, any_hit=True), ref, f"cloud {kind} refit step {step} any-hit")
    ref = sr.reference("cloud", seed, 2)
    sc.build()
    _check_closest(sc.run(ref.rays), ref, f"cloud {kind} rebuilt")


# ------------------------------------------------------------------ 7: small and degenerate cases
def _small_ref(spheres, seed, n=768):
    return sr.Reference(spheres, sr.make_rays(spheres, seed, n, with_radius=True))


@pytest.mark.parametrize("kind", KINDS)
def test_few_spheres(rt, kind):
    base = np.array([[0.1, -0.2, 0.3, 0.5], [1.2, 0.1, -0.1, 0.4], [-0.9, 0.8, 0.2, 0.7], [0.3, 0.3, 1.5, 0.0],
                     [0.2, -1.1, -0.4, 0.3]], F)
    for count in (1, 2, 3, 5):
        s = base[:count]
        sc = Spheres(rt, s, kind).frame()
        assert rt.sphere_status(sc.status) == 0
        ref = _small_ref(s, 40 + count)
        _check_closest(sc.run(ref.rays), ref, f"{count} spheres {kind}")
        _check_any(sc.run(ref.rays, any_hit=True), ref, f"{count} spheres {kind} any-hit")


@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_scenes(rt, kind):
    # r = 0: hit only by a line through the centre, exactly.  o = c - k * d with d of a few bits: every operation of the test is
    # exact, s = k and the offset p is 0.  (Skew directions: a ray that lies IN a face plane of a box is the slab test's own
    # edge case, the tracer's, and not the subject here.)
    s = np.array([[1, 2, 3, 0], [4, 0, 0, 0.5], [0, 5, 0, 0.25]], F)
    sc = Spheres(rt, s, kind).frame()
    rays = np.zeros(3, sr.RAY)
    rays["origin"] = [(-1, 1, -1), (3, 1, 2.5), (-1 + 1e-3, 1, -1)]
    rays["dir"] = [(0.5, 0.25, 1), (-1, 0.5, 0.25), (0.5, 0.25, 1)]
    rays["tmax"] = np.inf
    hits = sc.run(rays)
    assert hits["primitive_id"].tolist() == [0, 0, sr.MISS] and hits["t"].tolist()[:2] == [4.0, 2.0]
    assert (hits["u"] == 0).all() and (hits["v"] == 0).all()
    ref = _small_ref(s, 51)
    _check_closest(sc.run(ref.rays), ref, f"r = 0 {kind}")

    # two identical spheres (and a third): either copy is the answer
    s = np.array([[0.5, 0.5, 0.5, 0.6], [-1, 0, 0, 0.3], [0.5, 0.5, 0.5, 0.6]], F)
    ref = _small_ref(s, 52)
    sc = Spheres(rt, s, kind).frame()
    _check_closest(sc.run(ref.rays), ref, f"identical spheres {kind}")
    _check_any(sc.run(ref.rays, any_hit=True), ref, f"identical spheres {kind} any-hit")

    # one sphere containing all others: rays from inside the big one reach it through the far root
    rng = np.random.default_rng(53)
    s = np.vstack([np.hstack([rng.uniform(-1, 1, (40, 3)), rng.uniform(0.05, 0.2, (40, 1))]), [[0, 0, 0, 10]]]).astype(F)
    ref = sr.Reference(s, sr.make_rays(s, 54, 768))        # (the centre box: every ray begins inside the big sphere)
    sc = Spheres(rt, s, kind).frame()
    hits = sc.run(ref.rays)
    _check_closest(hits, ref, f"enclosing sphere {kind}")
    far = (hits["primitive_id"] == 40) & (hits["u"] == 1)
    assert far.sum() > 50 and (hits["primitive_id"][ref.stable & (ref.rays["tmax"] == np.inf)] != sr.MISS).all()

    # every sphere invalid: point proxies at the origin, nothing is ever hit
    s = np.array([[np.nan, 0, 0, 1], [0, 0, 0, -1], [0, 0, 0, np.nan], [0, 0, 0, np.inf], [np.inf, 0, 0, 1]], F)
    sc = Spheres(rt, s, kind).frame()
    assert rt.sphere_status(sc.status) == rt.RT_SPHERE_BAD
    rays = np.zeros(64, sr.RAY)
    rays["origin"] = rng.uniform(-1, 1, (64, 3))
    rays["dir"] = -rays["origin"]
    rays["tmax"] = np.inf
    hits, ctr = sc.run(rays, counters=True)
    assert (hits["primitive_id"] == sr.MISS).all() and (hits["t"] == np.inf).all()
    assert ctr[1] <= 2 * 64, "only the NaN- and the inf-centre sphere pass the radius rule and are tested"


@pytest.mark.parametrize("kind", KINDS)
def test_num_spheres_below_the_leaf_ids(rt, built, kind):
    sc = built("cloud", kind)
    full = sr.reference("cloud", sr.SEEDS[0])
    rays = full.rays[:1024].copy()
    for keep in (700, 1, 0):
        hits, ctr = sc.run(rays, counters=True, num_spheres=keep)
        if keep == 0:
            assert (hits["primitive_id"] == sr.MISS).all() and ctr[1] == 0 and ctr[0] > 0
            continue
        ref = sr.Reference(full.spheres[:keep].copy(), rays)
        assert (hits["primitive_id"][hits["primitive_id"] != sr.MISS] < keep).all()
        _check_closest(hits, ref, f"cloud {kind} num_spheres {keep}")


def test_degenerate_rays_and_batch_edges(rt, built):
    import torch
    sc = built("lattice", "bottom_up")
    ref = sr.reference("lattice", sr.SEEDS[0])
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
        assert (hits["primitive_id"] == sr.MISS).all() and (hits["t"] == np.inf).all() and (hits["u"] == 0).all()
        assert ctr[0] == 0 and ctr[1] == 0, "a ray that is not traced counts no test"
    # a ray without a direction is traced and hits nothing, even from inside a sphere
    still = ref.rays[:4].copy()
    still["origin"] = ref.spheres[:4, :3]
    still["dir"] = 0
    still["tmin"], still["tmax"] = 0, np.inf
    hits = sc.run(still)
    assert (hits["primitive_id"] == sr.MISS).all() and (hits["t"] == np.inf).all()

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
    sc = Spheres(rt, np.zeros((0, 4), F))
    sc.prepare()
    rays = sr.reference("lattice", sr.SEEDS[0]).rays[:100]
    hits = torch.full((100, 4), -7.0, dtype=torch.float32, device="cuda")
    rt.IntersectRaysSpheres(None, None, 0, 0, None, 0, _dev_rays(rt, rays), hits)      # count = 0: the empty tree
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(rt.HIT).reshape(-1)
    assert (got["primitive_id"] == sr.MISS).all() and (got["t"] == np.inf).all()


# ------------------------------------------------------------------ 8: hipGraph
def test_prepare_build_and_query_in_a_hip_graph(rt):
    import torch
    seed = sr.SEEDS[0]
    refs = {"a": sr.reference("cloud", seed), "b": sr.reference("cloud", seed, 1)}
    sc = Spheres(rt, refs["a"].spheres, "bottom_up")
    n = sr.NUM_RAYS
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
        sc.upload(refs[key].spheres)                    # rewritten in place: the same buffers
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
        _check_closest(got, refs[key], f"graph replay {key}")
        _check_any(anyh.cpu().numpy().view(rt.HIT).reshape(-1), refs[key], f"graph replay {key} any-hit")
        assert rt.sphere_status(sc.status) == rt.RT_SPHERE_BAD
        for g, e in zip((hits, anyh, ctr), eager[key]):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                               e.view(torch.int32) if e.dtype == torch.float32 else e), key
