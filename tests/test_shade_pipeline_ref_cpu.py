"""Self-checks of tests/shade_pipeline_ref.py, the numpy float32 restatement the GPU tests of the deferred-shading calls
compare against: the properties include/rt_abi.h promises for the shadow ray and the depth byte."""
import numpy as np

import shade_pipeline_ref as ref

LIGHT = (20.0, 3.0, -10.0)
N_TRI = 50


def _batch(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, ref.RAY)
    rays["origin"] = rng.uniform(-5, 5, (n, 3))
    d = rng.normal(size=(n, 3))
    rays["dir"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays["tmin"], rays["tmax"] = 1e-5, 120.0
    hits = np.zeros(n, ref.HIT)
    hits["t"] = rng.uniform(0.5, 60, n)
    hits["primitive_id"] = rng.integers(0, N_TRI, n)
    hits["u"], hits["v"] = 0.25, 0.5
    return rays, hits


def test_a_miss_gives_the_dead_ray():
    rays, hits = _batch()
    hits["primitive_id"][::3] = ref.MISS
    hits["t"][::3] = np.inf
    hits["primitive_id"][1::9] = N_TRI              # the first id that is no triangle
    hits["t"][2::11] = np.nan                       # (still a hit record: the NaN goes through)
    rays["tmax"][5::13] = -1.0                      # dead primary rays, whatever their record says
    rays["dir"][6::17, 1] = np.nan
    out = ref.shadow_rays(rays, hits, N_TRI, LIGHT)
    dead = (hits["primitive_id"] >= N_TRI) | ~ref.live(rays)
    assert dead.sum() > 1000 and (~dead).sum() > 1000
    for f in ("origin", "dir"):
        assert (out[f][dead] == 0).all() and not np.signbit(out[f][dead]).any()
    assert (out["tmin"][dead] == 0).all() and (out["tmax"][dead] == -1).all()
    assert not ref.live(out[dead]).any(), "rt_intersect_rays does not trace the dead ray"
    assert (out["tmin"][~dead] == np.float32(0.001)).all()


def test_direction_is_unit_and_tmax_is_the_light_distance():
    rays, hits = _batch()
    out = ref.shadow_rays(rays, hits, N_TRI, LIGHT)
    assert out["origin"].dtype == np.float32
    hp = rays["origin"].astype(np.float64) + rays["dir"].astype(np.float64) * hits["t"].astype(np.float64)[:, None]
    l = np.asarray(LIGHT) - hp
    dist = np.linalg.norm(l, axis=1)
    assert np.abs(out["tmax"] - dist).max() <= 1e-5 * dist.max()
    norm = np.linalg.norm(out["dir"].astype(np.float64), axis=1)
    assert np.abs(norm - 1).max() < 4 * np.finfo(np.float32).eps, "unit length to within float rounding"
    assert (out["tmax"] > 0.001).all() and ref.live(out).all()


def test_a_scaled_light_distance_scales_tmax():
    """the scene scaled by a power of two about the origin (origin, t and light: exact in float32) scales the shadow ray's
    origin and tmax by the same factor and leaves its direction alone, bit for bit"""
    rays, hits = _batch()
    base = ref.shadow_rays(rays, hits, N_TRI, LIGHT)
    for s in (0.25, 2.0, 1024.0):
        r2, h2 = rays.copy(), hits.copy()
        r2["origin"] = rays["origin"] * np.float32(s)
        h2["t"] = hits["t"] * np.float32(s)
        out = ref.shadow_rays(r2, h2, N_TRI, tuple(np.float32(x) * np.float32(s) for x in np.float32(LIGHT)))
        assert (out["tmax"] == base["tmax"] * np.float32(s)).all()
        assert (out["origin"] == base["origin"] * np.float32(s)).all()
        assert out["dir"].tobytes() == base["dir"].tobytes()


def test_depth_byte():
    hits = np.zeros(8, ref.HIT)
    hits["t"] = [0.0, 60.0, 120.0, 500.0, np.inf, 30.0, np.nan, 119.9]
    hits["primitive_id"] = [0, 1, 2, 3, ref.MISS, N_TRI, 4, N_TRI - 1]
    b = ref.depth_byte(hits, 120.0, N_TRI)
    assert b.dtype == np.uint8
    assert b.tolist() == [0, 127, 255, 255, 0, 0, 255, 254]      # 60/120*255 = 127.5 truncates; fminf(1, NaN) = 1
