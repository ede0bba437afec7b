"""Reference of the motion-blur ray query (rt_intersect_rays_motion), restated from include/rt_abi.h with no code shared with
the kernels, and the inputs its CPU and GPU tests share.

lerp32(a, b, tau)             the defined interpolation in float32: w0 = 1 - tau; fl(fl(w0 * a) + fl(tau * b))
lerp_tris(tris0, tris1, tau)  the caller's triangles as a ray of time tau sees them
brute(tris0, tris1, rays, times)
    float64 brute force per time group: shade_ref.cast over the float32-interpolated triangles of each distinct time.
    Returns (ref, tris_all, base): ref as shade_ref.cast's dict over all rays, with ref["tri"] an index into tris_all -- the
    interpolated triangles of every group one after the other, group k at [k n, (k + 1) n) -- mapped to the first exact copy
    as test_gpu_ray_queries._canonical does; base[i] = k n for ray i.  A hit record of ray i names triangle
    base[i] + primitive_id of tris_all, so test_gpu_ray_queries._check_against_f64 applies to (tris_all, records with base
    added) unchanged.
poses(name, scenes), ray_cases(name, tris0)
    the scenes, key poses, ray sets and per-ray times of tests/test_gpu_motion.py; tests/test_motion_ref_cpu.py holds the
    unstable fraction of exactly these against the GPU test's cap."""
import numpy as np

import shade_ref

F = np.float32
TIMES = np.array([0.0, 0.25, 1.0 / 3.0, 0.7, 1.0], F)
SCENES = ("grid", "soup", "cornell")
ENDPOINT_SCENES = SCENES + ("fractal",)   # the endpoint test also runs the deep-stack scene (levels 26..48 of the traversal stack)
CAP = {"grid": 0.01, "soup": 0.01, "cornell": 0.05}     # the unstable fraction _check_against_f64 allows (cornell: shared planes)


def lerp32(a, b, tau):
    a, b, tau = np.asarray(a, F), np.asarray(b, F), F(tau)
    w0 = F(F(1) - tau)
    return ((w0 * a).astype(F) + (tau * b).astype(F)).astype(F)


def lerp_tris(tris0, tris1, tau):
    return lerp32(np.asarray(tris0, F).reshape(-1, 9), np.asarray(tris1, F).reshape(-1, 9), tau)


def canonical(tris):
    """index of the first exact copy of every triangle, and the sorted first copies"""
    _, first, inv = np.unique(np.ascontiguousarray(tris, F).view(np.dtype((np.void, 36))).reshape(-1), return_index=True,
                              return_inverse=True)
    return first[inv.reshape(-1)], np.sort(first)


def _cast(rays, tris, keep, lo, hi):
    r = shade_ref.cast(rays["origin"].astype(np.float64), rays["dir"].astype(np.float64), tris[keep], lo, hi)
    r["tri"] = np.where(r["hit"], keep[np.maximum(r["tri"], 0)], -1)
    return r


def brute(tris0, tris1, rays, times, window=False):
    """window: rays whose hit lies near an end of [tmin, tmax] may go either way in float32 and count as unstable (the rule of
    test_gpu_ray_queries._window_stable)"""
    times = np.asarray(times, F)
    groups = np.unique(times)
    n = np.asarray(tris0).reshape(-1, 9).shape[0]
    tris_all = np.concatenate([lerp_tris(tris0, tris1, g) for g in groups])
    gi = np.searchsorted(groups, times)
    canon, _ = canonical(tris_all)
    N = len(rays)
    ref = dict(hit=np.zeros(N, bool), t=np.full(N, np.inf), tri=np.full(N, -1, np.int64), u=np.zeros(N), v=np.zeros(N),
               stable=np.ones(N, bool))
    for k in range(len(groups)):
        sel = np.nonzero(gi == k)[0]
        if not sel.size:
            continue
        tg, r = tris_all[k * n:(k + 1) * n], rays[sel]
        _, keep = canonical(tg)
        lo, hi = r["tmin"].astype(np.float64), r["tmax"].astype(np.float64)
        c = _cast(r, tg, keep, lo, hi)
        stable = c["stable"]
        if window:
            loose = _cast(r, tg, keep, lo * (1 - 1e-4) - 1e-9, hi * (1 + 1e-4))
            tight = _cast(r, tg, keep, lo * (1 + 1e-4) + 1e-9, hi * (1 - 1e-4))
            stable = stable & (loose["hit"] == tight["hit"]) & (loose["tri"] == tight["tri"]) & (loose["tri"] == c["tri"])
        ref["hit"][sel], ref["t"][sel], ref["u"][sel], ref["v"][sel], ref["stable"][sel] = c["hit"], c["t"], c["u"], c["v"], stable
        ref["tri"][sel] = np.where(c["hit"], canon[k * n + np.maximum(c["tri"], 0)], -1)
    return ref, tris_all, gi * n


def with_base(hits, base):
    """the records with every hit's primitive_id turned into its index in brute()'s tris_all"""
    out = hits.copy()
    hit = out["primitive_id"] != 0xFFFFFFFF
    out["primitive_id"][hit] = (out["primitive_id"][hit].astype(np.int64) + base[hit]).astype(np.uint32)
    return out


# ------------------------------------------------------------------ the inputs of the GPU test
def poses(name, scenes):
    """(tris0, tris1): a scene of test_gpu_ray_queries and its smooth displacement (a function of position alone: shared
    corners stay shared, so pairs stay whole)"""
    import test_gpu_ray_queries as rq
    from test_gpu_refit import _smooth
    tris0 = np.ascontiguousarray(rq._scene(name, scenes)[0], F).reshape(-1, 9)
    return tris0, _smooth(tris0)


def ray_cases(name, tris0, tris1):
    """kind -> (rays, times): test_gpu_ray_queries._ray_sets aimed at the union of both poses (1200 rays per kind: outside,
    axis, window), each ray with one of TIMES"""
    import test_gpu_ray_queries as rq
    sets = rq._ray_sets(np.concatenate([tris0, tris1]), seed=ENDPOINT_SCENES.index(name) + 301)
    rng = np.random.default_rng(ENDPOINT_SCENES.index(name) + 77)
    return {kind: (r, TIMES[rng.integers(0, len(TIMES), len(r))]) for kind, r in sets.items()}


def translated(tris):
    """pose 1 of the tiny and degenerate scenes: pose 0 moved by a tenth of its extent (at least 0.01) along (1, -0.5, 0.25)"""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    ext = float(np.ptp(t.reshape(-1, 3), axis=0).max()) if t.size else 1.0
    d = (max(0.1 * ext, 0.01) * np.array([1.0, -0.5, 0.25])).astype(F)
    return (t + d).astype(F).reshape(-1, 9)
