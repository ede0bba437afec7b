"""numpy float32 restatement of the record-level recipes of the deferred-shading calls (include/rt_abi.h):
rt_generate_shadow_rays's ray and RT_RENDER_DEPTH's byte of rt_shade_frame.  Every operation is a float32 array
operation, so it is rounded on its own, as the kernels' are (no fused multiply-add; IEEE division and square root)."""
import numpy as np

RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
HIT = np.dtype([("t", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])
MISS = 0xFFFFFFFF
SHADOW_TMIN = np.float32(0.001)


def live(rays):
    """the rays rt_intersect_rays traces: tmin <= tmax (false for NaN) and no NaN in origin or direction"""
    with np.errstate(invalid="ignore"):
        return (rays["tmin"] <= rays["tmax"]) & ~np.isnan(rays["origin"]).any(axis=1) & ~np.isnan(rays["dir"]).any(axis=1)


def shadow_rays(rays, hits, num_triangles, light):
    """shadow_rays[i] of rt_generate_shadow_rays"""
    light = np.asarray(light, np.float32)
    out = np.zeros(rays.shape[0], RAY)
    out["tmax"] = -1.0                                            # the dead ray: origin 0, dir 0, tmin 0, tmax -1
    sel = live(rays) & (hits["primitive_id"] < np.uint32(min(num_triangles, MISS)))
    o, d, t = rays["origin"][sel], rays["dir"][sel], hits["t"][sel]
    with np.errstate(all="ignore"):
        hp = o + d * t[:, None]
        l = light[None, :] - hp
        to_light = np.sqrt((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2])
        linv = np.float32(1.0) / to_light
        direction = l * linv[:, None]
    for a in (hp, l, to_light, linv, direction):
        assert a.dtype == np.float32
    out["origin"][sel], out["dir"][sel], out["tmin"][sel], out["tmax"][sel] = hp, direction, SHADOW_TMIN, to_light
    return out


def depth_byte(hits, max_depth, num_triangles):
    """RT_RENDER_DEPTH: u8(fminf(1, t / max_depth) * 255) of a hit record, 0 of anything else (the float -> u8 conversion
    truncates; NaN -> 0)"""
    hit = hits["primitive_id"] < np.uint32(min(num_triangles, MISS))
    with np.errstate(all="ignore"):
        q = hits["t"] / np.asarray(max_depth, np.float32)
        v = np.where(np.isnan(q), np.float32(1.0), np.minimum(np.float32(1.0), q)) * np.float32(255.0)   # fminf drops a NaN
    assert v.dtype == np.float32
    b = np.where(v > 0, np.where(v >= 255, 255, np.nan_to_num(v, nan=0.0, posinf=255.0).astype(np.int64)), 0)
    return np.where(hit, b, 0).astype(np.uint8)
