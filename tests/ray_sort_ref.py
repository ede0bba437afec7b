"""numpy restatement of rt_sort_rays (include/rt_abi.h, "ray sorting"): liveness, the root-run box and the 27-bit key as
shipped, every float32 operation in the documented order -- the library is built without FMA contraction, so the keys match
bit for bit.  Expected order = np.argsort(keys, kind="stable")."""
import numpy as np

KEY_BITS = 30
DEAD = np.uint32(1 << 29)
ORIGIN_BITS, DIR_BITS = 7, 2
F = np.float32


def live(rays):
    """the rays rt_intersect_rays traces: tmin <= tmax (false for a NaN) and no NaN in origin or direction"""
    with np.errstate(invalid="ignore"):
        return (rays["tmin"] <= rays["tmax"]) & ~np.isnan(rays["origin"]).any(axis=1) & ~np.isnan(rays["dir"]).any(axis=1)


def _ordered(f):
    i = np.ascontiguousarray(f, F).view(np.int32)
    return i ^ ((i >> 31) & 0x7FFFFFFF)


def _unordered(i):
    i = np.asarray(i, np.int32)
    return (i ^ ((i >> 31) & 0x7FFFFFFF)).view(F)


def root_box(nodes, root, count):
    """(lo[3], hi[3]) float32: ordered min / max over the non-NONE slots of [root, root + count); the point 0 without one"""
    run = nodes[(root & 0x1FFFFFFF):(root & 0x1FFFFFFF) + count]
    run = run[(run["w28"] >> 29) != 0]
    if run.size == 0:
        return np.zeros(3, F), np.zeros(3, F)
    return _unordered(_ordered(run["min"]).min(axis=0)), _unordered(_ordered(run["max"]).max(axis=0))


def _cell(q, cells):
    """(q > 0) ? (q >= cells - 1 ? cells - 1 : trunc(q)) : 0 -- by selects, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        pos, top = q > 0, q >= F(cells - 1)
    inner = np.where(pos & ~top, q, F(0)).astype(np.int64).astype(np.uint32)
    return np.where(pos, np.where(top, np.uint32(cells - 1), inner), np.uint32(0)).astype(np.uint32)


def _spread3(v):
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def morton3(c):
    return (_spread3(c[:, 0]) << np.uint32(2)) | (_spread3(c[:, 1]) << np.uint32(1)) | _spread3(c[:, 2])


def cells(rays, lo, hi):
    """(origin cells [N, 3], direction cells [N, 3]) of every ray, dead ones included"""
    o, d = rays["origin"].astype(F), rays["dir"].astype(F)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    OC, DC = 1 << ORIGIN_BITS, 1 << DIR_BITS
    with np.errstate(all="ignore"):
        e = (hi - lo).astype(F)
        oc = _cell((((o - lo).astype(F) / e).astype(F) * F(OC)).astype(F), OC)
        ad = np.abs(d)
        m = ad[:, 0].copy()
        m = np.where(ad[:, 1] > m, ad[:, 1], m)
        m = np.where(ad[:, 2] > m, ad[:, 2], m)
        dc = _cell((((d / m[:, None]).astype(F) * F(DC // 2)).astype(F) + F(DC // 2)).astype(F), DC)
    return oc, dc


def keys(rays, lo, hi):
    oc, dc = cells(rays, lo, hi)
    k = (morton3(oc) << np.uint32(3 * DIR_BITS)) | morton3(dc)
    return np.where(live(rays), k, DEAD).astype(np.uint32)


def sort(rays, nodes, root, count):
    """-> dict(box=(lo, hi), keys (unsorted), order, num_live)"""
    lo, hi = root_box(nodes, root, count)
    k = keys(rays, lo, hi)
    return dict(box=(lo, hi), keys=k, order=np.argsort(k, kind="stable").astype(np.uint32), num_live=int(live(rays).sum()))
