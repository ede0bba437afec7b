"""numpy restatement of instance motion (rt_abi.h, instance-motion block): the per-ray interpolated matrix, its float32
inverse and the object-space rays of rt_intersect_rays_instanced_motion, vectorised over rays; rt_prepare_motion_instances's
two proxy sets (instance_ref.prepare, pose by pose) and flags; the float64 world triangles of a moving scene at a time; and the
scenes, rays and times the CPU and GPU tests share."""
from __future__ import annotations

import numpy as np

import instance_ref as ir

BAD_BLAS, SINGULAR = ir.BAD_BLAS, ir.SINGULAR
MOTION_INSTANCE = np.dtype([("object_to_world0", "<f4", (3, 4)), ("object_to_world1", "<f4", (3, 4)), ("blas", "<u4"),
                            ("pad", "<u4", 7)])
TIMES = np.array([0, 0.25, 0.5, 1, 0.3, 0.77, 0.93, 1e-3], np.float32)   # the eight times of the GPU tests
F = np.float32


# ------------------------------------------------------------------ the query's arithmetic
def matrix_at(M0, M1, tau):
    """m[k] = fl(fl(w0 * M0[k]) + fl(tau * M1[k])), w0 = fl(1 - tau): float32 [N, 3, 4] for tau [N] (M0, M1 [3, 4] or [N, 3, 4])"""
    tau = np.asarray(tau, F).reshape(-1, 1, 1)
    w0 = (F(1) - tau).astype(F)
    return ((w0 * np.asarray(M0, F)).astype(F) + (tau * np.asarray(M1, F)).astype(F)).astype(F)


def inverse_f32(m):
    """the query's float32 inverse of the 3x3 part of m [N, 3, 4]: (W [N, 3, 3], det [N], entered [N]) -- cofactors and
    det = (a00*c00 + a01*c01) + a02*c02 as rt_prepare_instances writes them, inv_det = 1 / det, W = adj * inv_det"""
    a = np.asarray(m, F)
    a00, a01, a02 = a[:, 0, 0], a[:, 0, 1], a[:, 0, 2]
    a10, a11, a12 = a[:, 1, 0], a[:, 1, 1], a[:, 1, 2]
    a20, a21, a22 = a[:, 2, 0], a[:, 2, 1], a[:, 2, 2]
    with np.errstate(all="ignore"):
        c00, c01, c02 = a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20
        det = ((a00 * c00 + a01 * c01) + a02 * c02).astype(F)
        inv_det = (F(1) / det).astype(F)
        adj = np.stack([np.stack([c00, a02 * a21 - a01 * a22, a01 * a12 - a02 * a11], axis=-1),
                        np.stack([c01, a00 * a22 - a02 * a20, a02 * a10 - a00 * a12], axis=-1),
                        np.stack([c02, a01 * a20 - a00 * a21, a00 * a11 - a01 * a10], axis=-1)], axis=1).astype(F)
        W = (adj * inv_det[:, None, None]).astype(F)
    entered = (det != 0) & np.isfinite(det) & np.isfinite(inv_det)
    return W, det, entered


def object_rays(rays, times, M0, M1):
    """the query's object-space rays of one instance: (rays with o' = W * (o - T), d' = W * d, each row (w0*x + w1*y) + w2*z in
    float32; entered [N]: False where the interpolated matrix cannot be inverted)"""
    m = matrix_at(M0, M1, times)
    W, _, entered = inverse_f32(m)
    with np.errstate(all="ignore"):
        q = (rays["origin"].astype(F) - m[:, :, 3]).astype(F)
        out = rays.copy()
        out["origin"] = ir.linear_f32(W, q)
        out["dir"] = ir.linear_f32(W, rays["dir"])
    return out, entered


# ------------------------------------------------------------------ prepare
def flags(instances, boxes):
    n = instances.size
    fl = np.zeros(n, np.uint32)
    for i in range(n):
        b = int(instances["blas"][i])
        if (boxes[b] if b < len(boxes) else None) is None:
            fl[i] |= BAD_BLAS
        M0, M1 = instances["object_to_world0"][i], instances["object_to_world1"][i]
        if not (np.isfinite(M0).all() and np.isfinite(M1).all()):
            fl[i] |= SINGULAR
            continue
        d0, d1 = (_det64(M) for M in (M0, M1))
        if d0 == 0.0 or d1 == 0.0 or (d0 < 0) != (d1 < 0):
            fl[i] |= SINGULAR
    return fl


def _det64(M):
    """the kernel's double determinant, term for term"""
    a = np.asarray(M, np.float64)
    c00, c01, c02 = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
    return a[0, 0] * c00 + a[0, 1] * c01 + a[0, 2] * c02


def prepare(instances, boxes):
    """(proxies0, proxies1 float32 [n, 9], flags uint32 [n]): instance_ref.prepare per pose; a flagged instance has the point
    proxy at the origin in both"""
    fl = flags(instances, boxes)
    out = []
    for key in ("object_to_world0", "object_to_world1"):
        one = ir.instance_array(list(instances[key]), list(instances["blas"]))
        prox = np.zeros((instances.size, 9), np.float32)
        ok = fl == 0
        if ok.any():
            prox[ok] = ir.prepare(one[ok], boxes)[0]
        out.append(prox)
    return out[0], out[1], fl


def motion_instance_array(mats0, mats1, blas):
    a = np.zeros(len(mats0), MOTION_INSTANCE)
    for k, (m0, m1, b) in enumerate(zip(mats0, mats1, blas)):
        a["object_to_world0"][k], a["object_to_world1"][k], a["blas"][k] = np.asarray(m0, F), np.asarray(m1, F), b
    return a


# ------------------------------------------------------------------ float64 world
def matrices_f64(instances, t):
    """(1 - t) * M0 + t * M1 in float64 on the float32 inputs: [n, 3, 4]"""
    t = float(F(t))
    return (1.0 - t) * instances["object_to_world0"].astype(np.float64) + t * instances["object_to_world1"].astype(np.float64)


def world_triangles(blas_tris, instances, t):
    """float64 world-space triangles of every instance at time t: ([sum T, 9], instance index, primitive index)"""
    M = matrices_f64(instances, t)
    out, inst, prim = [], [], []
    for i in range(instances.size):
        T = blas_tris[int(instances["blas"][i])].reshape(-1, 3, 3).astype(np.float64)
        out.append((T @ M[i][:, :3].T + M[i][:, 3]).reshape(-1, 9))
        inst.append(np.full(T.shape[0], i))
        prim.append(np.arange(T.shape[0]))
    return np.concatenate(out), np.concatenate(inst), np.concatenate(prim)


def interpolated_proxy_box(prox0, prox1, tau):
    """the box the query sees for every proxy at time tau: float32 lo, hi [n, 3] (the motion query's interpolation)"""
    tau = F(tau)
    w0 = F(1) - tau
    lerp = lambda a, b: ((w0 * a).astype(F) + (tau * b).astype(F)).astype(F)
    return lerp(prox0[:, 0:3], prox1[:, 0:3]), lerp(prox0[:, 3:6], prox1[:, 3:6])


# ------------------------------------------------------------------ the scenes of the tests
def axis_rotation(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis`"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def composition_pose0(ext):
    """the seven matrices of test_gpu_instances._composition (the GPU test asserts they are the same) and their BLAS indices"""
    aff = lambda R, t: np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)])
    R = ir.rotation(0.3, -0.5, 0.9)
    mats = [aff(R, (0, 0, 0)), aff(np.diag([1.5, 0.6, 2.0]), (1.3 * ext, 0, 0)), aff(np.diag([-1.0, 1.0, 1.0]), (0, 1.3 * ext, 0)),
            aff([[1, 0.4, 0], [0, 1, 0.3], [0.2, 0, 1]], (0, 0, 1.3 * ext)), aff(np.eye(3), (-1.2 * ext, 0.5 * ext, 0.2 * ext)),
            aff(R, (0.07 * ext, 0.05 * ext, -0.03 * ext)), aff(ir.rotation(0.1, 0.2, 0.3) * 1.2, (-0.3 * ext, -1.2 * ext, 0))]
    return mats, [0, 0, 0, 0, 0, 0, 1]


def moved_pose(mats0, blas, blas_tris, ext, seed, max_angle=0.4, max_shift=0.3):
    """pose 1: every instance turned by at most max_angle rad about a random axis through the centre of its own world box and
    shifted by at most max_shift * ext along every axis"""
    rng = np.random.default_rng(seed)
    out = []
    for M, b in zip(mats0, blas):
        M = np.asarray(M, np.float64)
        P = blas_tris[b].reshape(-1, 3).astype(np.float64)
        c = M[:, :3] @ ((P.min(axis=0) + P.max(axis=0)) / 2) + M[:, 3]
        R = axis_rotation(rng.normal(size=3), rng.uniform(-max_angle, max_angle))
        shift = rng.uniform(-max_shift, max_shift, 3) * ext
        out.append(np.hstack([R @ M[:, :3], (c + R @ (M[:, 3] - c) + shift)[:, None]]))
    return out


def composition(scenes):
    """(blas triangles [grid_mesh(24, 5), grid_mesh(16, 9)], MOTION_INSTANCE array of the seven moving instances)"""
    blas_tris = [scenes.grid_mesh(24, 5), scenes.grid_mesh(16, 9)]
    ext = float(np.ptp(blas_tris[0].reshape(-1, 3), axis=0).max())
    mats0, blas = composition_pose0(ext)
    return blas_tris, motion_instance_array(mats0, moved_pose(mats0, blas, blas_tris, ext, seed=41), blas)


def many_rigid(blas_tris, count=65, seed=3):
    """random rigid poses as test_tlas_over_proxies_matches_oracle's, with a moved pose 1"""
    rng = np.random.default_rng(seed)
    aff = lambda R, t: np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)])
    mats0 = [aff(ir.rotation(*rng.uniform(-1, 1, 3)), rng.uniform(-200, 200, 3)) for _ in range(count)]
    blas = rng.integers(0, 2, count).tolist()
    ext = float(np.ptp(blas_tris[0].reshape(-1, 3), axis=0).max())
    return motion_instance_array(mats0, moved_pose(mats0, blas, blas_tris, ext, seed=seed + 1), blas)


def union_triangles(blas_tris, instances):
    """the float64 world triangles of both key poses together: what the test rays are aimed at"""
    return np.concatenate([world_triangles(blas_tris, instances, 0.0)[0], world_triangles(blas_tris, instances, 1.0)[0]])


def fixed_times(n, seed, values=TIMES):
    return values[np.random.default_rng(seed).integers(0, values.size, n)]


def static_instances(instances):
    """pose 1 := pose 0"""
    s = instances.copy()
    s["object_to_world1"] = s["object_to_world0"]
    return s


def half_turn(instances, k=0):
    """instance k alone, pose 1 = pose 0 turned by pi about z through the world origin: the interpolated matrix at time 0.5 has
    a singular 3x3 part, while both determinants have one sign"""
    s = instances[[k]].copy()
    Rz = np.diag([-1.0, -1.0, 1.0])
    s["object_to_world1"][0] = (Rz @ s["object_to_world0"][0].astype(np.float64)).astype(F)
    return s
