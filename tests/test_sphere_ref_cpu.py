"""CPU test of tests/sphere_ref.py alone, on every scene and seed tests/test_gpu_spheres.py uses: what the GPU checks rest on.

  * the unstable share of every batch is within sphere_ref.CAP (1 %);
  * on stable rays the float32 formula (dense rays x spheres) and the float64 brute force agree on hit / miss and sphere;
  * no stable hit is culled by its sphere's padded box, tested with the float32 slab test under tmax already shrunk to the hit;
  * every scene exercises the far root (rays that begin inside a sphere);
  * every prepared box contains c +- r in float64, and invalid spheres get the point proxy and the status flag."""
import numpy as np
import pytest

import sphere_ref as sr

CASES = [(name, seed, 0) for name in sr.SCENES for seed in sr.SEEDS] + [("cloud", sr.SEEDS[0], 1), ("cloud", sr.SEEDS[0], 2)]
# the least share of a batch that must take a far root: the scenes are built so that rays begin inside spheres (lattice: the
# spheres fill pi / 6 of the box the second half of the rays starts in; shell: every ray begins inside the outer sphere and
# those that meet no small sphere leave through it; cloud: about 1500 * 4/3 pi E[r^3] / 8 = 4 % of the box is inside a sphere)
MIN_FAR = {"cloud": 0.01, "lattice": 0.10, "shell": 0.10}


@pytest.mark.parametrize("name,seed,step", CASES)
def test_reference_is_sound(name, seed, step):
    ref = sr.reference(name, seed, step)
    rays, spheres = ref.rays, ref.spheres
    n = rays.shape[0]
    assert n == sr.NUM_RAYS
    print(f"{name} seed {seed} step {step}: unstable {100 * ref.unstable_share:.3f} %, hits {int(ref.f64['hit'].sum())}, "
          f"far roots {100 * ref.far32.mean():.1f} %")
    assert ref.unstable_share <= sr.CAP

    st = ref.stable
    hit32 = ref.id32 >= 0
    assert (hit32[st] == ref.f64["hit"][st]).all(), "float32 and float64 disagree on hit / miss of a stable ray"
    both = st & hit32
    assert (ref.canon[ref.id32[both]] == ref.f64["id"][both]).all(), "float32 and float64 disagree on the sphere of a stable ray"
    assert (ref.far32[both] == ref.f64["far"][both]).all()
    assert both.sum() > n // 4 and (st & ~hit32).sum() > 20, "the batch must hold hits and misses"

    # the padded box of the hit sphere, under tmax = the float32 t of the hit
    prox, ok, status = sr.prepare_f32(spheres)
    ids = ref.id32[both]
    assert ok[ids].all()
    assert sr.slab_f32(rays[both], prox[ids, 0:3], prox[ids, 3:6], ref.t32[both]).all(), "a stable hit is culled by its box"

    if step == 0:
        assert ref.far32.mean() >= MIN_FAR[name]


@pytest.mark.parametrize("name", sr.SCENES)
def test_prepared_boxes(name):
    for step in (0, 1):
        s = sr.gpu_scene(name)
        if step:
            s = sr.moved(s, step)
        prox, ok, status = sr.prepare_f32(s)
        assert prox.dtype == np.float32 and prox.shape == (s.shape[0], 9)
        assert status == sr.RT_SPHERE_BAD and (~ok).sum() == 4 and not ok[-4:].any()
        assert (prox[~ok] == 0).all()
        c, r = s[ok, :3].astype(np.float64), s[ok, 3:4].astype(np.float64)
        lo, hi = prox[ok, 0:3].astype(np.float64), prox[ok, 3:6].astype(np.float64)
        assert (lo <= c - r).all() and (hi >= c + r).all()
        assert (lo < hi).all()
        mid = prox[ok, 6:9].astype(np.float64)
        assert (lo <= mid).all() and (mid <= hi).all()
        # the pad is a few 2^-18 of the largest bound, not more
        big = np.abs(np.concatenate([lo, hi], axis=1)).max(axis=1, keepdims=True)
        assert ((c - r) - lo <= big * 2.0 ** -17).all() and (hi - (c + r) <= big * 2.0 ** -17).all()


def test_the_formula_on_hand_cases():
    F = np.float32
    rays = np.zeros(4, sr.RAY)
    rays["origin"] = [(0, 0, -5), (0, 0, 0), (0, 0, -5), (0, 3, -5)]
    rays["dir"] = [(0, 0, 2), (0, 0, 2), (0, 0, 2), (0, 0, 2)]
    rays["tmax"] = [np.inf, np.inf, 1.0, np.inf]
    t, far = sr.pair_f32(rays, np.array([[0, 0, 0, 1]], F), np.zeros(4, np.int64))
    assert t[0] == F(2.0) and not far[0]          # from outside: the near root, in units of |dir|
    assert t[1] == F(0.5) and far[1]              # from inside: the far root
    assert np.isnan(t[2]) and np.isnan(t[3])      # the window ends before the sphere; the line passes it by
    # a small sphere far away: the perpendicular offset keeps the digits the textbook discriminant loses
    rays = np.zeros(1, sr.RAY)
    rays["dir"], rays["tmax"] = (1, 0, 0), np.inf
    s = np.array([[4096, 0.001, 0, 0.002]], F)
    t, far = sr.pair_f32(rays, s, np.zeros(1, np.int64))
    exact = 4096 - np.sqrt(np.float64(s[0, 3]) ** 2 - np.float64(s[0, 1]) ** 2)
    assert abs(float(t[0]) - exact) <= 4096 * 2.0 ** -22
    # not valid for the query: never hit
    for bad in ((0, 0, 0, -1), (0, 0, 0, np.nan), (0, 0, 0, np.inf), (np.nan, 0, 0, 1)):
        t, _ = sr.pair_f32(rays, np.array([bad], F), np.zeros(1, np.int64))
        assert np.isnan(t[0]), bad
    # a ray without a direction hits nothing, even from inside
    rays["dir"] = 0
    t, _ = sr.pair_f32(rays, np.array([[0, 0, 0, 1]], F), np.zeros(1, np.int64))
    assert np.isnan(t[0])
    # identical spheres share one canonical index
    assert sr.canonical(np.array([[1, 2, 3, 4], [0, 0, 0, 1], [1, 2, 3, 4]], F)).tolist() == [0, 1, 0]
