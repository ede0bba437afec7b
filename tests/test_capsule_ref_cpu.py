"""CPU test of tests/capsule_ref.py alone, on every scene and seed tests/test_gpu_capsules.py uses: what the GPU checks rest on.

  * the unstable share of every batch is within capsule_ref.CAP; each scene gives at least half the hit, far-root and body
    shares it was designed for;
  * on stable rays the float32 formula (dense rays x capsules) and the float64 brute force agree on hit / miss, capsule and
    far flag; t is within capsule_ref.T_TOL (the figures measured here: the test prints them) -- on `strand` also on the rays
    that only the gap rule calls unstable, which are held to t and not to the id;
  * no stable hit is culled by its capsule's padded box, tested with the float32 slab test under tmax already shrunk to the hit;
  * every prepared box contains both end spheres in float64, invalid capsules get the point proxy and the status flag;
  * degenerate capsules are sphere_ref's spheres, bit for bit, in prepare and in the test;
  * the formula on hand cases in exactly representable numbers."""
import numpy as np
import pytest

import capsule_ref as cr
import sphere_ref as sr

F = np.float32
CASES = [(name, seed, 0) for name in cr.SCENES for seed in cr.SEEDS] + [("fibres", cr.SEEDS[0], 1), ("fibres", cr.SEEDS[0], 2)]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name,seed,step", CASES)
def test_reference_is_sound(name, seed, step):
    ref = cr.reference(name, seed, step)
    rays, caps = ref.rays, ref.capsules
    n = rays.shape[0]
    assert n == cr.NUM_RAYS
    st = ref.stable
    hit32 = ref.id32 >= 0
    both = st & hit32
    body = (ref.v32[both] > 0) & (ref.v32[both] < 1)
    err = cr.t_error(ref.t32[both], ref.f64["t"][both])
    print(f"{name} seed {seed} step {step}: unstable {100 * ref.unstable_share:.3f} % (without the gap rule "
          f"{100 * (1 - ref.same.mean()):.3f} %), hits {100 * hit32.mean():.1f} %, far roots {100 * ref.far32.mean():.2f} %, "
          f"body {100 * body.mean():.1f} % of stable hits, max t error {err.max():.3g}")
    assert ref.unstable_share <= cr.CAP[name]

    assert (hit32[st] == ref.f64["hit"][st]).all(), "float32 and float64 disagree on hit / miss of a stable ray"
    assert (ref.canon[ref.id32[both]] == ref.f64["id"][both]).all(), "float32 and float64 disagree on the capsule of a stable ray"
    assert (ref.far32[both] == ref.f64["far"][both]).all()
    assert (st & ~hit32).sum() > 20, "the batch must hold misses"
    # t: the step-0 figures are the ones T_TOL records; a moved scene gets the factor of 2 the GPU test grants it
    assert err.max() <= cr.T_TOL[name] * (2.0 if step else 1.0)
    # rays only the gap rule calls unstable (two capsules cross within 1e-4): t is still the nearest crossing's
    near_tie = ref.same & ~st & hit32 & ref.f64["hit"]
    assert cr.t_error(ref.t32[near_tie], ref.f64["t"][near_tie]).max(initial=0.0) <= 2.0 * cr.T_TOL[name]

    # the padded box of the hit capsule, under tmax = the float32 t of the hit
    prox, ok, status = cr.prepare_f32(caps)
    ids = ref.id32[both]
    assert ok[ids].all()
    assert cr.slab_f32(rays[both], prox[ids, 0:3], prox[ids, 3:6], ref.t32[both]).all(), "a stable hit is culled by its box"

    if step == 0:
        assert hit32.mean() >= cr.MIN_HIT[name]
        assert ref.far32.mean() >= cr.MIN_FAR[name]
        assert body.mean() >= cr.MIN_BODY[name]
        assert (ref.v32[both] == 0).any() and (ref.v32[both] == 1).any(), "both caps must be hit"


@pytest.mark.parametrize("name", cr.SCENES)
def test_prepared_boxes(name):
    for step in (0, 1):
        c = cr.gpu_scene(name)
        if step:
            c = cr.moved(c, step)
        prox, ok, status = cr.prepare_f32(c)
        assert prox.dtype == np.float32 and prox.shape == (c.shape[0], 9)
        assert status == cr.RT_CAPSULE_BAD and (~ok).sum() == 4 and not ok[-4:].any()
        assert (prox[~ok] == 0).all()
        r = c[ok, 3:4].astype(np.float64)
        lo, hi = prox[ok, 0:3].astype(np.float64), prox[ok, 3:6].astype(np.float64)
        for p in (c[ok, 0:3].astype(np.float64), c[ok, 4:7].astype(np.float64)):
            assert (lo <= p - r).all() and (hi >= p + r).all()
        assert (lo < hi).all()
        mid = prox[ok, 6:9].astype(np.float64)
        assert (lo <= mid).all() and (mid <= hi).all()
        # the pad is a few 2^-18 of the largest bound, not more
        big = np.abs(np.concatenate([lo, hi], axis=1)).max(axis=1, keepdims=True)
        pmin = np.minimum(c[ok, 0:3], c[ok, 4:7]).astype(np.float64)
        pmax = np.maximum(c[ok, 0:3], c[ok, 4:7]).astype(np.float64)
        assert ((pmin - r) - lo <= big * 2.0 ** -17).all() and (hi - (pmax + r) <= big * 2.0 ** -17).all()


def test_degenerate_capsules_are_spheres_bit_for_bit():
    for name in sr.SCENES:
        s = sr.gpu_scene(name)
        c = cr.pack(s[:, 0:3], s[:, 3], s[:, 0:3])
        c[:, 0:4] = s           # (the NaN and infinite entries as they are)
        c[:, 4:7] = s[:, 0:3]
        ps, oks, sts = sr.prepare_f32(s)
        pc, okc, stc = cr.prepare_f32(c)
        assert (_bits(ps) == _bits(pc)).all() and (oks == okc).all() and sts == stc
        rays = sr.reference(name, sr.SEEDS[0]).rays[:512]
        ids = np.random.default_rng(3).integers(0, s.shape[0], size=512)
        ts, fs = sr.pair_f32(rays, s, ids)
        tc, fc, vc = cr.pair_f32(rays, c, ids)
        assert (_bits(ts) == _bits(tc)).all() and (fs == fc).all() and (_bits(vc) == 0).all()
        assert (~np.isnan(ts)).sum() > 0
        td, idd, fd = sr.dense_f32(rays, s)
        tcd, idc, fcd, vcd = cr.dense_f32(rays, c)
        assert (_bits(td) == _bits(tcd)).all() and (idd == idc).all() and (fd == fcd).all() and (_bits(vcd) == 0).all()


def _one(origin, direction, capsule, tmin=0.0, tmax=np.inf):
    rays = np.zeros(1, cr.RAY)
    rays["origin"], rays["dir"], rays["tmin"], rays["tmax"] = origin, direction, tmin, tmax
    t, far, v = cr.pair_f32(rays, np.array([capsule], F), np.zeros(1, np.int64))
    return float(t[0]), bool(far[0]), float(v[0])


def test_the_formula_on_hand_cases():
    cap = (0, 0, 0, 1, 4, 0, 0, 0)      # axis (0,0,0)-(4,0,0), r = 1
    assert _one((2, -5, 0), (0, 1, 0), cap) == (4.0, False, 0.5)         # perpendicular through the body's middle
    assert _one((1, -5, 0), (0, 2, 0), cap) == (2.0, False, 0.25)        # in units of |dir|
    assert _one((3, 0, 0), (0, 0, 1), cap) == (1.0, True, 0.75)          # from inside: the far root, on the body
    assert _one((-5, 0, 0), (1, 0, 0), cap) == (4.0, False, 0.0)         # along the axis (A == 0): p0's cap at distance - 1
    assert _one((9, 0, 0), (-1, 0, 0), cap) == (4.0, False, 1.0)         # and from the other end: p1's cap
    assert _one((-5, 0.5, 0), (1, 0, 0), cap)[1:] == (False, 0.0)        # parallel at offset 0.5: the cap
    assert abs(_one((-5, 0.5, 0), (1, 0, 0), cap)[0] - (5 - np.sqrt(0.75))) < 1e-6
    assert np.isnan(_one((-5, 2, 0), (1, 0, 0), cap)[0])                 # parallel at offset 2: a miss
    assert _one((2, 0, 0), (1, 0, 0), cap) == (3.0, True, 1.0)           # parallel from inside: out through p1's cap
    assert _one((2, 0, 0), (-1, 0, 0), cap) == (3.0, True, 0.0)
    assert _one((0, -5, 0), (0, 1, 0), cap) == (4.0, False, 0.0)         # at the seam, y1 == -nn/2 exactly: a hit, p0's cap
    assert _one((4, -5, 0), (0, 1, 0), cap) == (4.0, False, 1.0)         # the other seam
    assert _one((-1, -5, 0), (0, 1, 0), cap) == (5.0, False, 0.0)        # tangent to p0's cap at its pole
    assert np.isnan(_one((-1.5, -5, 0), (0, 1, 0), cap)[0])              # past the cap
    assert np.isnan(_one((2, -5, 0), (0, 1, 0), cap, tmax=3.5)[0])       # the window ends before the capsule
    assert _one((2, -5, 0), (0, 1, 0), cap, tmin=4.5) == (6.0, True, 0.5)
    seg = (0, 0, 0, 0, 4, 0, 0, 0)      # r = 0: a segment only a ray through it hits
    assert _one((1, -2, 0), (0, 1, 0), seg) == (2.0, False, 0.25)
    assert np.isnan(_one((1, -2, 0.5), (0, 1, 0), seg)[0])
    assert np.isnan(_one((5, -2, 0), (0, 1, 0), seg)[0])
    # not valid for the query: never hit
    for bad in ((0, 0, 0, -1, 4, 0, 0, 0), (0, 0, 0, np.nan, 4, 0, 0, 0), (0, 0, 0, np.inf, 4, 0, 0, 0),
                (np.nan, 0, 0, 1, 4, 0, 0, 0), (0, 0, 0, 1, 4, np.inf, 0, 0)):
        assert np.isnan(_one((2, -5, 0), (0, 1, 0), bad)[0]), bad
    # a ray without a direction hits nothing, even from inside
    assert np.isnan(_one((2, 0, 0), (0, 0, 0), cap)[0])
    # a small capsule far away: re-basing the ray keeps the digits the textbook discriminant loses
    t, far, v = _one((0, 0, 0), (1, 0, 0), (4096, 0.001, -1, 0.002, 4096, 0.001, 1, 0))
    exact = 4096 - np.sqrt(np.float64(F(0.002)) ** 2 - np.float64(F(0.001)) ** 2)
    assert abs(t - exact) <= 4096 * 2.0 ** -22 and not far and v == 0.5
    # identical capsules share one canonical index
    assert cr.canonical(np.array([cap, seg, cap], F)).tolist() == [0, 1, 0]
