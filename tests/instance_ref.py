"""numpy restatement of instancing (rt_abi.h, instancing block): rt_prepare_instances's float32 arithmetic bit for bit, the
object-space rays of the query, and the float64 world-space triangles of an instanced scene (for a brute-force check)."""
from __future__ import annotations

import numpy as np

PAD = np.float32(2.0 ** -12)
BAD_BLAS, SINGULAR = 1, 2


def _ordered(f):
    i = np.asarray(f, np.float32).view(np.int32)
    return i ^ ((i >> 31) & 0x7FFFFFFF)


def _unordered(i):
    i = np.asarray(i, np.int32)
    return (i ^ ((i >> 31) & 0x7FFFFFFF)).view(np.float32)


def root_box(nodes, root, count):
    """ordered min / max over the non-NONE slots of the run [root, root + count) of a NODE array; None if there is none"""
    run = nodes[root:root + count]
    run = run[(run["w28"] >> 29) != 0]
    if run.size == 0:
        return None
    return _unordered(_ordered(run["min"]).min(axis=0)), _unordered(_ordered(run["max"]).max(axis=0))


def affine_f32(m, p):
    """rows ((m0*x + m1*y) + m2*z) + m3 in float32; m [..., 3, 4], p [..., 3]"""
    f = np.float32
    m, p = np.asarray(m, f), np.asarray(p, f)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    out = [((m[..., k, 0] * x + m[..., k, 1] * y) + m[..., k, 2] * z) + m[..., k, 3] for k in range(3)]
    return np.stack(out, axis=-1).astype(f)


def linear_f32(m, d):
    f = np.float32
    m, d = np.asarray(m, f), np.asarray(d, f)
    out = [(m[..., k, 0] * d[..., 0] + m[..., k, 1] * d[..., 1]) + m[..., k, 2] * d[..., 2] for k in range(3)]
    return np.stack(out, axis=-1).astype(f)


def prepare(instances, boxes):
    """instances: INSTANCE array; boxes[b] = root_box(...) of BLAS b, or None for an unusable table entry.
    Returns (proxies float32 [n, 9], world_to_object float64 [n, 3, 4] (the exact inverse), flags uint32 [n])."""
    n = instances.size
    prox = np.zeros((n, 9), np.float32)
    inv = np.zeros((n, 3, 4))
    flags = np.zeros(n, np.uint32)
    for i in range(n):
        M = instances["object_to_world"][i].astype(np.float32)
        b = int(instances["blas"][i])
        box = boxes[b] if b < len(boxes) else None
        if box is None:
            flags[i] |= BAD_BLAS
        M64 = M.astype(np.float64)
        if not np.isfinite(M).all() or np.linalg.det(M64[:, :3]) == 0.0:
            flags[i] |= SINGULAR
        else:
            W3 = np.linalg.inv(M64[:, :3])
            inv[i, :, :3], inv[i, :, 3] = W3, -W3 @ M64[:, 3]
            if not np.isfinite(inv[i].astype(np.float32)).all():
                flags[i] |= SINGULAR
        if flags[i]:
            continue
        lo, hi = box
        corners = np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]] for c in range(8)],
                           np.float32)
        w = affine_f32(M[None], corners)
        wlo, whi = _unordered(_ordered(w).min(axis=0)), _unordered(_ordered(w).max(axis=0))
        e = np.float32(max(np.abs(wlo).max(), np.abs(whi).max()))
        pad = np.float32(e * PAD)
        wlo, whi = (wlo - pad).astype(np.float32), (whi + pad).astype(np.float32)
        mid = (wlo * np.float32(0.5) + whi * np.float32(0.5)).astype(np.float32)
        prox[i] = np.concatenate([wlo, whi, mid])
    return prox, inv, flags


def object_rays(rays, W):
    """the query's object-space rays: o' = W*(o, 1), d' = W3x3*d in float32 (W: float32 [3, 4], a record's world_to_object)"""
    out = rays.copy()
    out["origin"] = affine_f32(W[None], rays["origin"])
    out["dir"] = linear_f32(W[None], rays["dir"])
    return out


def world_triangles(blas_tris, instances):
    """float64 world-space triangles of every instance: ([sum T, 9], instance index, primitive index)"""
    out, inst, prim = [], [], []
    for i in range(instances.size):
        M = instances["object_to_world"][i].astype(np.float64)
        T = blas_tris[int(instances["blas"][i])].reshape(-1, 3, 3).astype(np.float64)
        out.append((T @ M[:, :3].T + M[:, 3]).reshape(-1, 9))
        inst.append(np.full(T.shape[0], i))
        prim.append(np.arange(T.shape[0]))
    return np.concatenate(out), np.concatenate(inst), np.concatenate(prim)


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def instance_array(mats, blas):
    """INSTANCE records from 3x4 matrices and BLAS indices"""
    a = np.zeros(len(mats), np.dtype([("object_to_world", "<f4", (3, 4)), ("blas", "<u4"), ("pad", "<u4", 3)]))
    for k, (m, b) in enumerate(zip(mats, blas)):
        a["object_to_world"][k] = np.asarray(m, np.float32)
        a["blas"][k] = b
    return a
