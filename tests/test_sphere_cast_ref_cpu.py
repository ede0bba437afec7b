"""CPU test of tests/sphere_cast_ref.py alone, on every scene and seed tests/test_gpu_sphere_cast.py uses: what the GPU checks
rest on.

  * the unstable share of every batch is within sphere_cast_ref.CAP; every feature kind and overlap occur among the stable hits;
  * on stable rays the float32 restatement (over the pair list, caller's corner order) and the float64 brute force agree on
    hit / miss and on overlap / travel; the float32 triangle is one whose own float64 t lies within the gap of the least; t is
    within sphere_cast_ref.T_TOL (the figures measured here: the test prints them);
  * the contact point of a stable travelling hit lies, in float64, at distance r from the centre o + t*d, and is the closest
    point of the hit triangle to that centre, within CONTACT_TOL of the scene's size;
  * no stable hit is culled by the float32 slab test of its triangle's vertex box grown by e, with tmax already shrunk to the
    hit -- the check that justifies the pad;
  * a sample of the pairs the pair list dropped is rejected by the float32 test too;
  * radius 0 rows are ray_filter_ref's Moller-Trumbore, bit for bit;
  * the formula on hand cases in exactly representable numbers.

The contact tolerance, per ray: the centre moves by the error of t times |dir| (4 * T_TOL * max(1, |t|) * |dir|: T_TOL with the
GPU test's factor), and the contact point comes from float32 weights and float32 corners (16 ulps of the scene's largest
coordinate)."""
import numpy as np
import pytest

import point_ref as pr
import ray_filter_ref as rf
import sphere_cast_ref as sc

F = np.float32
CASES = [(name, seed) for name in sc.SCENES for seed in sc.SEEDS]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name,seed", CASES)
def test_reference_is_sound(name, seed):
    ref = sc.reference(name, seed)
    rays, radii, tris = ref.rays, ref.radii, ref.tris
    assert rays.shape[0] == sc.NUM_RAYS and ref.traced.all()
    t32, id32, u32, v32, f32 = ref.dense32
    st = ref.stable
    hit32 = id32 >= 0
    both = st & hit32
    err = sc.t_error(t32[both], ref.f64["t"][both])
    kinds = np.bincount(f32[both], minlength=5)
    print(f"{name} seed {seed}: unstable {100 * ref.unstable_share:.3f} %, hits {100 * hit32.mean():.1f} %, overlap "
          f"{100 * ref.f64['over'].mean():.1f} %, face / edge / corner / overlap among stable hits {kinds[1:].tolist()}, "
          f"pairs {ref.ri.size} (dropped {ref.dropped}), max t error {err.max():.3g}")
    assert ref.unstable_share <= sc.CAP[name]
    assert (hit32[st] == ref.f64["hit"][st]).all(), "float32 and float64 disagree on hit / miss of a stable ray"
    assert ((f32 == sc.OVERLAP)[st] == ref.f64["over"][st]).all(), "float32 and float64 disagree on overlap / travel"
    assert (st & ~hit32).sum() > 20, "the batch must hold misses"
    assert ref.cand[np.flatnonzero(both), id32[both]].all(), "the float32 triangle is not within the gap of float64's least t"
    assert err.max() <= sc.T_TOL[name]
    assert (kinds[1:] > 20).all(), "every feature kind and overlap must occur"
    assert (_bits(t32[f32 == sc.OVERLAP]) == _bits(rays["tmin"][f32 == sc.OVERLAP])).all()

    # the contact point: at distance r from the centre, and the triangle's closest point to it
    trav = both & (f32 != sc.OVERLAP) & (radii > 0)
    T = tris.astype(np.float64).reshape(-1, 3, 3)[id32[trav]]
    u, v = u32[trav].astype(np.float64)[:, None], v32[trav].astype(np.float64)[:, None]
    contact = (1 - u - v) * T[:, 0] + u * T[:, 1] + v * T[:, 2]
    centre = rays["origin"][trav].astype(np.float64) + t32[trav].astype(np.float64)[:, None] * rays["dir"][trav].astype(np.float64)
    tol = 4 * sc.T_TOL[name] * np.maximum(1.0, np.abs(t32[trav])) * np.linalg.norm(rays["dir"][trav].astype(np.float64), axis=1) \
        + 16 * 2.0 ** -24 * float(np.abs(tris).max())
    dist = np.linalg.norm(centre - contact, axis=1)
    near = pr.closest_f64(centre, T[:, 0], T[:, 1], T[:, 2])
    print(f"  contact: |dist - r| <= {np.abs(dist - radii[trav]).max():.3g}, dist - closest <= {(dist - near).max():.3g}, "
          f"least tol {tol.min():.3g}")
    assert trav.sum() > 1000
    assert (np.abs(dist - radii[trav]) <= tol).all(), "the contact point is not at distance r from the centre"
    assert (dist - near <= tol).all(), "the contact point is not the triangle's closest point to the centre"

    # the grown vertex box of the hit triangle, under tmax = the float32 t of the hit
    P = tris.reshape(-1, 3, 3)[id32[both]]
    e = sc.grow_e(radii[both], sc.scene_M(tris))[:, None]
    assert (e[radii[both] == 0] == 0).all()
    assert sc.slab_f32(rays[both], P.min(axis=1) - e, P.max(axis=1) + e, t32[both]).all(), "a stable hit is culled by its box"


@pytest.mark.parametrize("name", sc.SCENES)
def test_dropped_pairs_are_rejected_in_float32(name):
    ref = sc.reference(name, sc.SEEDS[0])
    n, m = ref.rays.shape[0], ref.tris.shape[0]
    kept = np.zeros((n, m), bool)
    kept[ref.ri, ref.ti] = True
    rng = np.random.default_rng(3)
    ri, ti = rng.integers(0, n, size=200_000), rng.integers(0, m, size=200_000)
    sel = ~kept[ri, ti]
    ri, ti = ri[sel], ti[sel]
    assert ri.size > 100_000
    t, u, v, feat = sc.pairs_f32(ref.rays, ref.radii, ri, ref.tris[ti], np.zeros(ti.size, np.uint32))
    assert np.isnan(t).all() and (feat == sc.NONE).all()


@pytest.mark.parametrize("name", sc.SCENES)
def test_radius_zero_is_moller_trumbore_bit_for_bit(name):
    ref = sc.reference(name, sc.SEEDS[1])
    # every radius set to 0, against each ray's float64-nearest triangles and a random one
    rng = np.random.default_rng(5)
    n = ref.rays.shape[0]
    ids = np.where(ref.f64["id"] >= 0, ref.f64["id"], rng.integers(0, ref.tris.shape[0], size=n))
    tri = ref.tris[ids].reshape(-1, 3, 3)
    zero = np.zeros(n, F)
    for rot in (0, 1, 2):                      # the stored corners of a rotated leaf triangle
        stored = {0: tri, 1: tri[:, [2, 0, 1]], 2: tri[:, [1, 2, 0]]}[rot]     # un-rotating these gives the caller's corners back
        t, u, v, feat = sc.pairs_f32(ref.rays, zero, np.arange(n), stored.reshape(-1, 9), np.full(n, rot, np.uint32))
        ok, mt, bu, bv, _ = rf.mt_det_f32(stored[:, 0], stored[:, 1], stored[:, 2], ref.rays["origin"], ref.rays["dir"],
                                          ref.rays["tmin"], ref.rays["tmax"])
        assert ok.sum() > 200
        assert (~np.isnan(t) == ok).all() and (feat == np.where(ok, sc.FACE, sc.NONE)).all()
        assert (_bits(t[ok]) == _bits(mt[ok])).all()
        with np.errstate(invalid="ignore"):
            w0 = (F(1) - bu - bv).astype(F)
        eu, ev = {0: (bu, bv), 1: (bv, w0), 2: (w0, bu)}[rot]
        assert (_bits(u[ok]) == _bits(eu[ok])).all() and (_bits(v[ok]) == _bits(ev[ok])).all()
    assert (sc.grow_e(zero, 100.0) == 0).all()


def _one(origin, direction, r, tri, tmin=0.0, tmax=np.inf, rot=0):
    rays = np.zeros(1, sc.RAY)
    rays["origin"], rays["dir"], rays["tmin"], rays["tmax"] = origin, direction, tmin, tmax
    t, u, v, f = sc.pairs_f32(rays, np.array([r], F), np.zeros(1, np.int64), np.array([tri], F).reshape(1, 9),
                              np.array([rot], np.uint32))
    return float(t[0]), float(u[0]), float(v[0]), int(f[0])


def test_the_formula_on_hand_cases():
    tri = ((0, 0, 0), (4, 0, 0), (0, 4, 0))      # in the plane z = 0, normal +z
    # head-on onto the face, from either side, in units of |dir|
    assert _one((1, 1, 5), (0, 0, -1), 1, tri) == (4.0, 0.25, 0.25, sc.FACE)
    assert _one((1, 1, -5), (0, 0, 2), 1, tri) == (2.0, 0.25, 0.25, sc.FACE)
    # the same contact through the rotations of the stored corners: the record speaks of the caller's corners
    assert _one((2, 1, 5), (0, 0, -1), 1, ((0, 4, 0), (0, 0, 0), (4, 0, 0)), rot=1) == (4.0, 0.5, 0.25, sc.FACE)
    assert _one((2, 1, 5), (0, 0, -1), 1, ((4, 0, 0), (0, 4, 0), (0, 0, 0)), rot=2) == (4.0, 0.5, 0.25, sc.FACE)
    # onto an edge's body: in the plane, towards edge v0-v1 from below it
    assert _one((2, -5, 0), (0, 1, 0), 1, tri) == (4.0, 0.5, 0.0, sc.EDGE)
    assert _one((-5, 1, 0), (1, 0, 0), 1, tri) == (4.0, 0.0, 0.25, sc.EDGE)        # edge v2-v0
    # onto a corner
    assert _one((-5, 0, 0), (1, 0, 0), 1, tri) == (4.0, 0.0, 0.0, sc.CORNER)       # along edge v0-v1: parallel to an edge
    assert _one((9, 0, 0), (-1, 0, 0), 1, tri) == (4.0, 1.0, 0.0, sc.CORNER)
    assert _one((0, 9, 0), (0, -1, 0), 1, tri) == (4.0, 0.0, 1.0, sc.CORNER)
    assert _one((-3, -4, 0), (3, 4, 0), 1, tri)[1:] == (0.0, 0.0, sc.CORNER)       # diagonally onto v0
    assert abs(_one((-3, -4, 0), (3, 4, 0), 1, tri)[0] - 0.8) < 1e-6
    # grazing at exactly r: parallel to edge v0-v1 at distance 1 below it, and over the face at height 1
    assert _one((-5, -1, 0), (1, 0, 0), 1, tri) == (5.0, 0.0, 0.0, sc.CORNER)
    assert np.isnan(_one((-5, -1.5, 0), (1, 0, 0), 1, tri)[0])
    # starting in contact: overlap at tmin, the closest point's weights
    assert _one((1, 1, 0.5), (0, 0, -1), 1, tri) == (0.0, 0.25, 0.25, sc.OVERLAP)
    assert _one((1, 1, 1), (0, 0, 1), 1, tri) == (0.0, 0.25, 0.25, sc.OVERLAP)     # touching exactly, moving away
    assert _one((1, 1, 5), (0, 0, -1), 1, tri, tmin=4.5) == (4.5, 0.25, 0.25, sc.OVERLAP)
    assert _one((2, -0.5, 0), (1, 0, 0), 1, tri) == (0.0, 0.5, 0.0, sc.OVERLAP)
    # starting inside the prism between the offset faces, outside the sum: only the rim can be met
    assert _one((-5, 1, 0.5), (1, 0, 0), 1, tri)[1:] == (0.0, 0.25, sc.EDGE)
    assert abs(_one((-5, 1, 0.5), (1, 0, 0), 1, tri)[0] - (5 - np.sqrt(0.75))) < 1e-6
    # moving away, behind the window, past the window
    assert np.isnan(_one((1, 1, 5), (0, 0, 1), 1, tri)[0])
    assert np.isnan(_one((1, 1, 5), (0, 0, -1), 1, tri, tmax=3.5)[0])
    # a zero-area triangle: no face, the edges and corners still stop the ball
    sliver = ((0, 0, 0), (4, 0, 0), (4, 0, 0))
    assert _one((2, 0, 5), (0, 0, -1), 1, sliver)[0] == 4.0 and _one((2, 0, 5), (0, 0, -1), 1, sliver)[3] == sc.EDGE
    point = ((1, 1, 1), (1, 1, 1), (1, 1, 1))
    # (three degenerate edges at one t: the tie goes to the last part, edge s2-s0 at v = 0, which is corner s2)
    assert _one((1, 1, 6), (0, 0, -1), 2, point) == (3.0, 0.0, 1.0, sc.CORNER)
    assert np.isnan(_one((2, 0, 5), (0, 0, -1), 0, sliver)[0])                     # radius 0: Moller-Trumbore rejects it
    # radius 0 is the ray query
    assert _one((1, 1, 5), (0, 0, -1), 0, tri) == (5.0, 0.25, 0.25, sc.FACE)
    assert np.isnan(_one((2, -5, 0), (0, 1, 0), 0, tri)[0])
    # a ray without a direction touches nothing unless it overlaps
    assert np.isnan(_one((1, 1, 5), (0, 0, 0), 1, tri)[0])
    assert _one((1, 1, 0.5), (0, 0, 0), 1, tri)[3] == sc.OVERLAP


def test_the_e_rule():
    r = np.array([0, 1e-3, 1, 100], F)
    e = sc.grow_e(r, 8.0)
    assert e[0] == 0 and e.dtype == F
    assert e[1] == F(F(1e-3) + F(F(2.0 ** -18) * F(8.0))) and e[2] == F(F(1) + F(2.0 ** -15))
    assert e[3] == F(F(100) + F(F(100) * F(2.0 ** -18)))                           # max(r, M) = r
    nodes = np.zeros(4, [("min", "<f4", 3), ("w12", "<u4"), ("max", "<f4", 3), ("w28", "<u4")])
    nodes["min"][1], nodes["max"][1], nodes["w28"][1] = (-3, 1, 2), (5, 2, 2.5), 1 << 29
    nodes["min"][2], nodes["max"][2], nodes["w28"][2] = (-9, 0, 0), (1, 1, 1), 2 << 29
    nodes["min"][3], nodes["max"][3], nodes["w28"][3] = (-99, 0, 0), (99, 0, 0), 0     # type "none": not read
    assert sc.root_M(nodes, 1, 3) == 9 and sc.root_M(nodes, 1, 1) == 5 and sc.root_M(nodes, 3, 1) == 0
