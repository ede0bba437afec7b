"""Seeded secondary-ray generators on the host (numpy): what the measurement tools and the ray-sort tests trace after the
camera rays.  Inputs and outputs are RAY / HIT record arrays (see the package's dtypes); nothing here touches the GPU."""
import numpy as np

RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
MISS = 0xFFFFFFFF


def _hit_frame(rays, hits, tris):
    """(ok, hit point, unit normal facing the incoming ray) per ray; rows of missed rays are filled from triangle 0"""
    ok = hits["primitive_id"] != MISS
    V = tris.reshape(-1, 3, 3)[np.where(ok, hits["primitive_id"], 0).astype(np.int64)].astype(np.float32)
    n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1), 1e-30)[:, None]
    n *= -np.sign((n * rays["dir"]).sum(axis=1))[:, None]
    P = rays["origin"] + rays["dir"] * np.where(ok, hits["t"], 0)[:, None]
    return ok, P, n


def bounce_rays(rays, hits, tris, seed=1):
    """One diffuse bounce: origins on the hits of `rays` (offset 1e-3 along the normal facing the ray), uniform hemisphere
    directions, tmax = +inf; the ray of a missed (or dead) parent gets tmax = -1 < tmin, so it is not traced -- live and dead
    rays stay interleaved as the parents' hits and misses are.  Returns (RAY array, number of live rays)."""
    ok, P, n = _hit_frame(rays, hits, tris)
    d = np.random.default_rng(seed).normal(size=P.shape).astype(np.float32)
    d /= np.linalg.norm(d, axis=1)[:, None]
    d *= np.sign((d * n).sum(axis=1))[:, None]
    out = np.zeros(rays.size, RAY)
    out["origin"], out["dir"] = P + n * np.float32(1e-3), d
    out["tmin"], out["tmax"] = np.float32(1e-5), np.where(ok, np.float32(np.inf), np.float32(-1))
    return out, int(ok.sum())


def occlusion_rays(rays, hits, tris, per_hit=4, length=1.0, seed=2):
    """Short ambient-occlusion rays: `per_hit` rays per parent, consecutive (ray per_hit * i + k belongs to parent i), from
    the hit point into the hemisphere, tmax = `length` (unit directions); dead where the parent missed."""
    ok, P, n = _hit_frame(rays, hits, tris)
    P, n, ok = np.repeat(P, per_hit, axis=0), np.repeat(n, per_hit, axis=0), np.repeat(ok, per_hit)
    d = np.random.default_rng(seed).normal(size=P.shape).astype(np.float32)
    d /= np.linalg.norm(d, axis=1)[:, None]
    d *= np.sign((d * n).sum(axis=1))[:, None]
    out = np.zeros(P.shape[0], RAY)
    out["origin"], out["dir"] = P + n * np.float32(1e-3), d
    out["tmin"], out["tmax"] = np.float32(1e-5), np.where(ok, np.float32(length), np.float32(-1))
    return out, int(ok.sum())
