"""The numpy reference of the filtered instanced ray query (rt_intersect_rays_instanced_filtered), restated from
include/rt_abi.h (instance-filter block) with no code shared with the kernels.

InstanceFilter: the host image of rt_instance_hit_filter -- flags, ray_mask, per_instance (INSTANCE_FILTER array or None),
    per_ray (INSTANCE_RAY_FILTER array or None).
det_f32(W): the 3x3 determinant of a float32 world_to_object in the header's operation order.
effective(flt, k, W, n): the filter as it acts inside instance k -- a ray_filter_ref.Filter on the OBJECT-space determinant
    (the cull bits swapped by `flip`, cleared by CULL_DISABLE; skip_id only where skip_instance == k) plus the "entered" mask
    of the instance rule.  Composed with ray_filter_ref.walk_gated_det + keep on instance_ref.object_rays it restates the kernel
    (compose); handed to rt_intersect_rays_filtered it is the GPU test's per-instance reference.
candidates / cast_kept / brute_force: a float64 brute force over the KEPT world triangles of an instanced scene
    (instance_ref.world_triangles): facing is the sign of the WORLD-space determinant on the float64 world corners, so a mirror
    is handled by the geometry itself (the mirrored copy's corners wind the other way in world space) and nothing of det_f32,
    the cull-bit swap or the object-space rays is shared with what it checks.
The composition (the 7 instances of test_gpu_instances._composition), the filter arms and the ray batches the CPU and GPU tests
share are at the end."""
import numpy as np

import instance_ref as ir
import ray_filter_ref as rx
from shade_ref import BARY_MARGIN, SHADOW_T_MARGIN, T_REL_MARGIN

F = np.float32
MISS, ALL = 0xFFFFFFFF, 0xFFFFFFFF
CULL_BACK, CULL_FRONT = 1, 2
CULL_DISABLE, FLIP_FACING = 1, 2
INSTANCE_FILTER = np.dtype([("mask", "<u4"), ("flags", "<u4")])
INSTANCE_RAY_FILTER = np.dtype([("mask", "<u4"), ("skip_instance", "<u4"), ("skip_id", "<u4"), ("pad", "<u4")])
FACE_MARGIN = 1e-3      # |cos| of the angle between ray and triangle plane below which the facing counts as undecided


class InstanceFilter:
    def __init__(self, flags=0, ray_mask=ALL, per_instance=None, per_ray=None):
        self.flags, self.ray_mask = int(flags), int(ray_mask)
        self.per_instance = None if per_instance is None else np.ascontiguousarray(per_instance, INSTANCE_FILTER)
        self.per_ray = None if per_ray is None else np.ascontiguousarray(per_ray, INSTANCE_RAY_FILTER)

    def ray_masks(self, n):
        return np.full(n, self.ray_mask, np.uint32) if self.per_ray is None else self.per_ray["mask"].astype(np.uint32)

    def instance(self, k):
        """(mask, flags) of instance k: the array's record, or all ones and no flags beyond it or without it"""
        if self.per_instance is None or k >= len(self.per_instance):
            return ALL, 0
        return int(self.per_instance["mask"][k]), int(self.per_instance["flags"][k])


def det_f32(W):
    """(w0.x*(w1.y*w2.z - w1.z*w2.y) - w0.y*(w1.x*w2.z - w1.z*w2.x)) + w0.z*(w1.x*w2.y - w1.y*w2.x), every operation float32"""
    w = np.asarray(W, F)
    with np.errstate(all="ignore"):
        c0 = F(w[0, 0] * F(F(w[1, 1] * w[2, 2]) - F(w[1, 2] * w[2, 1])))
        c1 = F(w[0, 1] * F(F(w[1, 0] * w[2, 2]) - F(w[1, 2] * w[2, 0])))
        c2 = F(w[0, 2] * F(F(w[1, 0] * w[2, 1]) - F(w[1, 1] * w[2, 0])))
        return F(F(c0 - c1) + c2)


def effective(flt, k, W, n):
    """-> (ray_filter_ref.Filter acting on the object-space determinant inside instance k, entered bool [n])"""
    im, iflags = flt.instance(k)
    entered = (flt.ray_masks(n) & np.uint32(im)) != 0
    cull = flt.flags & (CULL_BACK | CULL_FRONT)
    if cull:
        flip = bool(det_f32(W) < 0) != bool(iflags & FLIP_FACING)          # a NaN det compares false: not mirrored
        if flip:
            cull = (CULL_FRONT if cull & CULL_BACK else 0) | (CULL_BACK if cull & CULL_FRONT else 0)
        if iflags & CULL_DISABLE:
            cull = 0
    per_ray = None
    if flt.per_ray is not None:
        per_ray = np.zeros(n, rx.RAY_FILTER)
        per_ray["mask"] = ALL
        # rule 2c: the skip acts inside skip_instance only; skip_id = MISS is "none" (ray_filter_ref.keep's convention too)
        per_ray["skip_id"] = np.where(flt.per_ray["skip_instance"] == k, flt.per_ray["skip_id"], MISS)
    return rx.Filter(cull, ALL, None, per_ray), entered


def walk_instances(trees, inst, W, rays):
    """the unfiltered all-hit rows of every instance on its float32 object rays: [(rows, dets)] per instance.
    trees[b] = (leaves, nodes, root, count) of BLAS b; W float32 [n_inst, 3, 4]"""
    out = []
    for k in range(inst.size):
        leaves, nodes, root, count = trees[int(inst["blas"][k])]
        rows, _, dets, _, _ = rx.walk_gated_det(nodes, leaves, root, count, ir.object_rays(rays, W[k]))
        out.append((rows, dets))
    return out


def compose(walks, W, flt, n):
    """per ray the minimum-t kept record over the entered instances -> (HIT array, instance ids).  `walks`: walk_instances"""
    best = np.zeros(n, rx.HIT)
    best["t"], best["primitive_id"] = np.inf, MISS
    best_id = np.full(n, MISS, np.uint32)
    for k, (rows, dets) in enumerate(walks):
        eff, entered = effective(flt, k, W[k], n)
        for i in np.nonzero(entered)[0]:
            row = rows[i]
            if not len(row):
                continue
            row = row[rx.keep(row, dets[i], i, eff)]
            if len(row):
                j = int(np.argmin(row["t"]))
                if row["t"][j] < best["t"][i]:
                    best[i], best_id[i] = row[j], k
    return best, best_id


# ------------------------------------------------------------------ float64 brute force over the kept world triangles
def candidates(rays, world_tris, chunk=256):
    """float64 Moller-Trumbore of every ray against every world triangle, kept sparse: the (ray, triangle) pairs that lie
    within BARY_MARGIN of the triangle, whatever their t -> dict(ray, tri, t, edge, face), sorted by ray.  face = the
    determinant e1 . (dir x e2) over |dir| |n|: the signed cosine between the ray and the plane's normal side (> 0: front)"""
    V = np.asarray(world_tris, np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = V[:, 0], V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    nlen = np.linalg.norm(np.cross(e1, e2), axis=1)
    o, d = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    out = {k: [] for k in ("ray", "tri", "t", "edge", "face")}
    for c0 in range(0, len(rays), chunk):
        dd, oo = d[c0:c0 + chunk, None, :], o[c0:c0 + chunk, None, :]
        h = np.cross(dd, e2[None])
        a = (e1[None] * h).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 / a
            s = oo - v0[None]
            u = f * (s * h).sum(-1)
            q = np.cross(s, e1[None])
            v = f * (dd * q).sum(-1)
            t = f * (e2[None] * q).sum(-1)
            edge = np.minimum(np.minimum(u, v), 1.0 - u - v)
            face = a / (np.linalg.norm(dd, axis=-1) * nlen[None])
            ok = (np.abs(a) > 1e-12) & (edge >= -BARY_MARGIN)
        r, k = np.nonzero(ok)
        out["ray"].append(r + c0); out["tri"].append(k)
        out["t"].append(t[r, k]); out["edge"].append(edge[r, k]); out["face"].append(face[r, k])
    return {k: np.concatenate(v) for k, v in out.items()}


def kept_masks(cand, inst_of, prim_of, flt, n):
    """the header's rules on the candidates, in world space -> (kept, maybe kept): `maybe` also keeps a candidate whose facing
    is within FACE_MARGIN of edge-on, where float32 may decide the other way"""
    ci, cp = inst_of[cand["tri"]], prim_of[cand["tri"]]
    im = np.array([flt.instance(k)[0] for k in range(int(inst_of.max()) + 1)], np.uint32)
    ifl = np.array([flt.instance(k)[1] for k in range(int(inst_of.max()) + 1)], np.uint32)
    ok = (im[ci] & flt.ray_masks(n)[cand["ray"]]) != 0
    if flt.per_ray is not None:
        pr = flt.per_ray[cand["ray"]]
        ok &= ~((pr["skip_instance"] == ci) & (pr["skip_id"] == cp) & (pr["skip_id"] != MISS))
    facing = np.where((ifl[ci] & FLIP_FACING) != 0, -cand["face"], cand["face"])
    culling = (ifl[ci] & CULL_DISABLE) == 0
    culled = culling & ((bool(flt.flags & CULL_BACK) & (facing < 0)) | (bool(flt.flags & CULL_FRONT) & (facing > 0)))
    surely = culling & ((bool(flt.flags & CULL_BACK) & (facing < -FACE_MARGIN)) | (bool(flt.flags & CULL_FRONT) & (facing > FACE_MARGIN)))
    return ok & ~culled, ok & ~surely


def _first_two(ray, t, mask, n):
    """per ray: the index (into the candidate arrays) of the masked candidate with the smallest t (-1: none), and the t of
    the runner-up (inf: none)"""
    idx = np.nonzero(mask)[0]
    idx = idx[np.lexsort((t[idx], ray[idx]))]
    r = ray[idx]
    lo, hi = np.searchsorted(r, np.arange(n), "left"), np.searchsorted(r, np.arange(n), "right")
    first = np.full(n, -1, np.int64)
    first[hi > lo] = idx[lo[hi > lo]]
    second = np.full(n, np.inf)
    second[hi > lo + 1] = t[idx[lo[hi > lo + 1] + 1]]
    return first, second


def cast_kept(cand, n, tmin, tmax, kept, maybe):
    """shade_ref.cast on the kept candidates -> dict(hit, t, tri, stable); stable as there: the nearest loosely tested
    (margins on the barycentrics, the window and the facing) candidate is the exact hit, BARY_MARGIN inside, no rival within
    T_REL_MARGIN -- or nothing is hit even loosely"""
    ray, t, edge = cand["ray"], cand["t"], cand["edge"]
    lo, hi = np.asarray(tmin, np.float64)[ray], np.asarray(tmax, np.float64)[ray]
    tm = SHADOW_T_MARGIN + T_REL_MARGIN * np.abs(t)
    exact = kept & (edge >= 0) & (t >= lo) & (t <= hi)
    loose = maybe & (t >= lo - tm) & (t <= hi + tm)
    k, _ = _first_two(ray, t, exact, n)
    kl, second = _first_two(ray, t, loose, n)
    hit = k >= 0
    out = dict(hit=hit, t=np.where(hit, t[k], np.inf), tri=np.where(hit, cand["tri"][k], -1))
    first = np.where(kl >= 0, t[kl], np.inf)
    out["stable"] = np.where(hit, (kl == k) & (edge[k] >= BARY_MARGIN) & (second > first * (1 + T_REL_MARGIN) + 1e-12), kl < 0)
    return out


def brute_force(cand, inst_of, prim_of, rays, flt):
    """-> (cast_kept's dict on the rays' windows, unique): unique = stable and the decision does not move when [tmin, tmax] is
    loosened or tightened by 1e-4 (relative) -- test_gpu_instances._window_ok's rule"""
    n = len(rays)
    kept, maybe = kept_masks(cand, inst_of, prim_of, flt, n)
    lo, hi = rays["tmin"].astype(np.float64), rays["tmax"].astype(np.float64)
    ref = cast_kept(cand, n, lo, hi, kept, maybe)
    loose = cast_kept(cand, n, lo * (1 - 1e-4) - 1e-9, hi * (1 + 1e-4), kept, maybe)
    tight = cast_kept(cand, n, lo * (1 + 1e-4) + 1e-9, hi * (1 - 1e-4), kept, maybe)
    window_ok = (loose["hit"] == tight["hit"]) & (loose["tri"] == tight["tri"]) & (loose["tri"] == ref["tri"])
    return ref, ref["stable"] & window_ok


START_ROUNDINGS = 3


def t_resolved(cand, ref, rays, bound):
    """For rays that START on a surface (a bounce batch): is the float32 start point fine enough for `bound`, the tolerance on
    t (an array, per ray)?  The start point has coordinates of magnitude |o|, far larger than the distances the ray travels.
    The kernel's object-space origin carries START_ROUNDINGS roundings of that magnitude -- the record's world_to_object
    entries (a float64 inverse rounded to float32), the products and the sums of o' = W (o, 1) -- so it is off by up to
    3 ulp(|o|) along the surface normal, which moves t by that over |cos| |dir|, cos the angle to the normal of the surface
    met.  Where that exceeds the bound the float64 t is not what float32 arithmetic on these inputs can be held to: a condition
    on the inputs, from the reference alone.  -> bool [n], true on misses"""
    n = len(rays)
    face = np.ones(n)
    sel = cand["tri"] == ref["tri"][cand["ray"]]
    face[cand["ray"][sel]] = np.abs(cand["face"][sel])
    o = np.abs(rays["origin"].astype(F)).max(axis=1)
    dlen = np.linalg.norm(rays["dir"].astype(np.float64), axis=1)
    with np.errstate(all="ignore"):
        moved = START_ROUNDINGS * np.spacing(o).astype(np.float64) / (face * dlen)
    return ~ref["hit"] | (moved <= bound)


# ------------------------------------------------------------------ the scene, filters and rays the CPU and GPU tests share
MIRROR, SECOND = 2, 6                   # the mirrored instance and the instance of the second BLAS
OVERLAP = (0, 5)                        # two overlapping copies of the first BLAS
DISABLED = (MIRROR, 4)                  # the instances that carry CULL_DISABLE in the cull_disable arm
GROUPS = 3
ARMS = ("cull_back", "cull_front", "cull_disable", "flip_facing", "masks")     # (+ "skip", on the bounce batch)
SEED, RAYS, MASK_SEED, BOUNCE_SEED = 11, 1500, 97, 23


def composition_instances(grid_tris):
    """the 7 INSTANCE records of test_gpu_instances._composition, rebuilt: six placements of BLAS 0 = grid_mesh(24) (rotation,
    non-uniform scale, mirror, shear, translation, a copy overlapping the first) and one of BLAS 1 = grid_mesh(16)"""
    ext = float(np.ptp(grid_tris.reshape(-1, 3), axis=0).max())
    R = ir.rotation(0.3, -0.5, 0.9)

    def affine(M, t=(0, 0, 0)):
        return np.hstack([np.asarray(M, np.float64), np.asarray(t, np.float64).reshape(3, 1)])
    mats = [affine(R), affine(np.diag([1.5, 0.6, 2.0]), (1.3 * ext, 0, 0)), affine(np.diag([-1.0, 1.0, 1.0]), (0, 1.3 * ext, 0)),
            affine([[1, 0.4, 0], [0, 1, 0.3], [0.2, 0, 1]], (0, 0, 1.3 * ext)), affine(np.eye(3), (-1.2 * ext, 0.5 * ext, 0.2 * ext)),
            affine(R, (0.07 * ext, 0.05 * ext, -0.03 * ext)), affine(ir.rotation(0.1, 0.2, 0.3) * 1.2, (-0.3 * ext, -1.2 * ext, 0))]
    return ir.instance_array(mats, [0, 0, 0, 0, 0, 0, 1])


def instance_filters(num, masks=None, flags=None):
    a = np.zeros(num, INSTANCE_FILTER)
    a["mask"] = ALL if masks is None else masks
    a["flags"] = 0 if flags is None else flags
    return a


def make_arm(name, num_instances, n):
    """the filter of arm `name` of ARMS for a batch of n rays"""
    if name == "cull_back":
        return InstanceFilter(CULL_BACK)
    if name == "cull_front":
        return InstanceFilter(CULL_FRONT)
    if name == "cull_disable":
        fl = np.zeros(num_instances, np.uint32)
        fl[list(DISABLED)] = CULL_DISABLE | 0x80        # (an unknown bit in a device-side flags word is ignored)
        return InstanceFilter(CULL_BACK, ALL, instance_filters(num_instances, flags=fl))
    if name == "flip_facing":
        fl = np.zeros(num_instances, np.uint32)
        fl[MIRROR] = FLIP_FACING
        return InstanceFilter(CULL_BACK, ALL, instance_filters(num_instances, flags=fl))
    if name == "masks":
        per_ray = np.zeros(n, INSTANCE_RAY_FILTER)
        per_ray["mask"] = np.random.default_rng(MASK_SEED).integers(1, 1 << GROUPS, n)      # 1 .. 7: never empty
        per_ray["skip_instance"], per_ray["skip_id"] = MISS, MISS
        im = (np.uint32(1) << (np.arange(num_instances, dtype=np.uint32) % GROUPS)).astype(np.uint32)
        return InstanceFilter(0, 0, instance_filters(num_instances, masks=im), per_ray)     # (ray_mask 0: per_ray must win)
    raise KeyError(name)


def world_rays(world_tris, n, seed):
    """test_gpu_instances._world_rays: n rays from outside the scene box at interior points, and the same n with random
    [tmin, tmax] windows"""
    rng = np.random.default_rng(seed)
    P = world_tris.reshape(-1, 3)
    lo, hi = P.min(axis=0), P.max(axis=0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = c + u * ext * 1.2
    d = (lo + rng.random((n, 3)) * (hi - lo) - o) * rng.uniform(0.3, 2.0, size=(n, 1))
    r = np.zeros(n, rx.RAY)
    r["origin"], r["dir"], r["tmin"], r["tmax"] = o, d, 0.0, np.inf
    w = r.copy()
    a, b = rng.random(n) * 1.2, rng.random(n) * 1.2
    w["tmin"], w["tmax"] = np.minimum(a, b), np.maximum(a, b)
    return np.concatenate([r, w])


def bounce_batch(rays, first, first_inst, world_tris, inst_of, prim_of, seed):
    """the self-hit batch, ray_filter_ref.bounce_rays's shape: for every ray with a primary hit (first[i] a HIT record in
    instance first_inst[i]) a ray that starts AT the hit point o + t d (float32) with tmin = 0 and its per-ray record (all-ones
    mask, skip = the primary (instance, primitive)).  Directions: random -- except that a ray whose primary lies in one of the
    two OVERLAP copies is aimed at the centroid of the SAME primitive in the other copy, where that primitive id must be
    reported.  Rays without a primary hit are dropped.  -> (RAY array, INSTANCE_RAY_FILTER array)"""
    hit = first["primitive_id"] != MISS
    with np.errstate(invalid="ignore"):
        hit &= np.isfinite(first["t"])
    r, h, hi = rays[hit], first[hit], first_inst[hit]
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(len(r), 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    out = np.zeros(len(r), rx.RAY)
    with np.errstate(all="ignore"):
        out["origin"] = r["origin"].astype(F) + (h["t"].astype(F)[:, None] * r["dir"].astype(F)).astype(F)
    flat = {(int(i), int(p)): j for j, (i, p) in enumerate(zip(inst_of, prim_of))}
    cent = world_tris.reshape(-1, 3, 3).mean(axis=1)
    for j in range(len(r)):
        if int(hi[j]) in OVERLAP:
            other = OVERLAP[1] if int(hi[j]) == OVERLAP[0] else OVERLAP[0]
            d[j] = cent[flat[(other, int(h["primitive_id"][j]))]] - out["origin"][j].astype(np.float64)
    out["dir"] = d
    out["tmin"], out["tmax"] = 0.0, np.inf
    ok = np.isfinite(out["origin"]).all(1) & np.isfinite(out["dir"]).all(1) & (np.abs(out["dir"]).sum(1) > 0)
    per_ray = np.zeros(len(r), INSTANCE_RAY_FILTER)
    per_ray["mask"], per_ray["skip_instance"], per_ray["skip_id"] = ALL, hi, h["primitive_id"]
    return out[ok], per_ray[ok]
