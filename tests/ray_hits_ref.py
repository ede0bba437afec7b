"""Two numpy references for the all-hit ray queries (rt_ray_hits_count / rt_ray_hits_collect), restated from include/rt_abi.h
with no code shared with the kernel, plus the ray sets the CPU and GPU tests share.

(a) walk(nodes, leaves, root, count, rays): the row of every ray as the header defines it -- the accepted triangles of the
    leaves reached through entered slots -- over the node and leaf BYTES of a tree.  float32 slab test (np.fmin / np.fmax drop
    a NaN like fminf / fmaxf), float32 Moller-Trumbore in the kernel's operation order with its acceptance rule and the
    rotation map.  The window is fixed, so a breadth-first frontier of (ray, run) pairs visits exactly the slots any other
    order visits; there is no 64-entry limit.  Returns per-ray HIT arrays and the two test counts.
(b) brute_f64(tris, rays): float64 Moller-Trumbore of every (ray, triangle) pair over the CALLER's triangles: accepted, and
    stable -- u, v, 1-u-v and t at least 1e-4 away from their acceptance limits and |a| away from epsilon -- so that a float32
    evaluation must decide a stable pair the same way."""
import numpy as np

F = np.float32
RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
HIT = np.dtype([("t", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])
INDEX_MASK = 0x1FFFFFFF
NONE, BOX, TRI = 0, 1, 2
EPS = F(0.000000001)
MARGIN = 1e-4
SEEDS = {"grid": 431, "soup": 457, "cornell": 760, "fractal": 736}      # ray_sets seeds of the CPU and GPU tests


def live(rays):
    """rt_intersect_rays's rule: tmin <= tmax (false for a NaN) and no NaN in origin or direction"""
    with np.errstate(invalid="ignore"):
        return (rays["tmin"] <= rays["tmax"]) & ~np.isnan(rays["origin"]).any(1) & ~np.isnan(rays["dir"]).any(1)


def _slab(lo, hi, o, inv):
    """front / back of boxes [lo, hi] for rays (o, inv), all float32 [k, 3]"""
    with np.errstate(invalid="ignore", over="ignore"):
        t1 = ((lo - o).astype(F) * inv).astype(F)
        t2 = ((hi - o).astype(F) * inv).astype(F)
    near, far = np.fmin(t1, t2), np.fmax(t1, t2)
    front = np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2])
    back = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
    return front, back


def mt_f32(c0, c1, c2, o, d, tmin, tmax):
    """the kernel's Moller-Trumbore in float32, operation for operation -> (accepted, t, bu, bv) on the given corners"""
    c0, c1, c2, o, d = (np.asarray(x, F) for x in (c0, c1, c2, o, d))
    with np.errstate(all="ignore"):
        e1, e2 = (c1 - c0).astype(F), (c2 - c0).astype(F)
        hx = d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1]
        hy = d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2]
        hz = d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]
        a = e1[:, 0] * hx + e1[:, 1] * hy + e1[:, 2] * hz
        ok = ~((a > -EPS) & (a < EPS))
        f = F(1.0) / a
        s = (o - c0).astype(F)
        u = f * (s[:, 0] * hx + s[:, 1] * hy + s[:, 2] * hz)
        ok &= ~((u < 0) | (u > 1))
        qx = s[:, 1] * e1[:, 2] - s[:, 2] * e1[:, 1]
        qy = s[:, 2] * e1[:, 0] - s[:, 0] * e1[:, 2]
        qz = s[:, 0] * e1[:, 1] - s[:, 1] * e1[:, 0]
        v = f * (d[:, 0] * qx + d[:, 1] * qy + d[:, 2] * qz)
        ok &= ~((v < 0) | ((u + v) > 1))
        t = f * (e2[:, 0] * qx + e2[:, 1] * qy + e2[:, 2] * qz)
        ok &= ~((t < tmin) | (t > tmax))
    return ok, t.astype(F), u.astype(F), v.astype(F)


def _records(t, prim, bu, bv, rot):
    """HIT records with (u, v) mapped back to the caller's corners: rot 1 -> (bv, w0), 2 -> (w0, bu), else (bu, bv)"""
    with np.errstate(all="ignore"):
        w0 = (F(1) - bu).astype(F) - bv
    out = np.zeros(len(t), HIT)
    out["t"], out["primitive_id"] = t, prim
    out["u"] = np.where(rot == 1, bv, np.where(rot == 2, w0, bu))
    out["v"] = np.where(rot == 1, w0, np.where(rot == 2, bu, bv))
    return out


def walk(nodes, leaves, root, count, rays):
    """-> (rows: list of HIT arrays, one per ray, in no particular order; box_tests; leaf_visits)"""
    n = len(rays)
    o, d = rays["origin"].astype(F), rays["dir"].astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1.0) / d).astype(F)
    tmin, tmax = rays["tmin"].astype(F), rays["tmax"].astype(F)
    alive = np.nonzero(live(rays))[0] if count > 0 else np.zeros(0, np.int64)
    fr_ray = alive.astype(np.int64)
    fr_first = np.full(len(alive), root & INDEX_MASK, np.int64)
    fr_cnt = np.full(len(alive), count, np.int64)
    box_tests = leaf_visits = 0
    got_ray, got_rec = [], []
    while len(fr_ray):
        nr, nf, nc, lr, li = [], [], [], [], []
        for k in range(int(fr_cnt.max())):
            sel = fr_cnt > k
            r, slot = fr_ray[sel], fr_first[sel] + k
            nd = nodes[slot]
            typ = nd["w28"] >> 29
            valid = typ != NONE
            box_tests += int(valid.sum())
            front, back = _slab(nd["min"], nd["max"], o[r], inv[r])
            with np.errstate(invalid="ignore"):
                inn = valid & (back >= front) & (front <= tmax[r]) & (back >= tmin[r])
            child = (nd["w28"] & INDEX_MASK).astype(np.int64)
            is_leaf = inn & (typ == TRI)
            ccount = (nd["w12"] >> 29).astype(np.int64)
            is_box = inn & (typ != TRI) & (ccount > 0)
            lr.append(r[is_leaf]); li.append(child[is_leaf])
            nr.append(r[is_box]); nf.append(child[is_box]); nc.append(ccount[is_box])
        lr, li = np.concatenate(lr), np.concatenate(li)
        leaf_visits += len(lr)
        if len(lr):
            L = leaves[li]
            prim0, prim1 = L["primitive_id_0"], L["primitive_id_1"]
            rot = L["rotations"]
            ok, t, bu, bv = mt_f32(L["v0"], L["v1"], L["v2"], o[lr], d[lr], tmin[lr], tmax[lr])
            got_ray.append(lr[ok]); got_rec.append(_records(t[ok], prim0[ok], bu[ok], bv[ok], rot[ok, 0]))
            two = (L["v3"].view(np.uint32) != L["v2"].view(np.uint32)).any(1)          # B = (v2, v1, v3) iff v3 != v2 bit for bit
            ok, t, bu, bv = mt_f32(L["v2"], L["v1"], L["v3"], o[lr], d[lr], tmin[lr], tmax[lr])
            ok &= two
            got_ray.append(lr[ok]); got_rec.append(_records(t[ok], prim1[ok], bu[ok], bv[ok], rot[ok, 1]))
        fr_ray, fr_first, fr_cnt = np.concatenate(nr), np.concatenate(nf), np.concatenate(nc)
    rows = [np.zeros(0, HIT)] * n
    if got_ray:
        gr, rec = np.concatenate(got_ray), np.concatenate(got_rec)
        order = np.argsort(gr, kind="stable")
        gr, rec = gr[order], rec[order]
        cuts = np.searchsorted(gr, np.arange(n + 1))
        rows = [rec[cuts[i]:cuts[i + 1]] for i in range(n)]
    return rows, box_tests, leaf_visits


def canon(rows):
    """a row as a sorted array of 16-byte records: equal arrays <=> equal multisets, bit for bit"""
    return [np.sort(np.ascontiguousarray(r).view(np.dtype((np.void, 16))).reshape(-1)) for r in rows]


def offsets(rows):
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)


def brute_f64(tris, rays, chunk=256):
    """-> dict of [rays, triangles] arrays: accepted (float64 decision), stable, in_window (t inside [tmin, tmax]), t"""
    T = np.asarray(tris, F).reshape(-1, 3, 3).astype(np.float64)
    m, n = len(rays), T.shape[0]
    out = {k: np.zeros((m, n), bool) for k in ("accepted", "stable", "in_window")}
    out["t"] = np.zeros((m, n))
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    le = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    alive = live(rays)
    for s in range(0, m, chunk):
        r = rays[s:s + chunk]
        o, d = r["origin"].astype(np.float64)[:, None, :], r["dir"].astype(np.float64)[:, None, :]
        lo, hi = r["tmin"].astype(np.float64)[:, None], r["tmax"].astype(np.float64)[:, None]
        with np.errstate(all="ignore"):
            h = np.cross(d, e2[None])
            a = (e1[None] * h).sum(2)
            f = 1.0 / a
            sv = o - T[None, :, 0]
            u = f * (sv * h).sum(2)
            q = np.cross(sv, e1[None])
            v = f * (d * q).sum(2)
            t = f * (e2[None] * q).sum(2)
            scale = np.maximum(1.0, np.abs(t))
            # signed margins of every acceptance condition (>= 0: it holds)
            marg = np.stack([u, 1 - u, v, 1 - u - v, (t - lo) / scale, (hi - t) / scale])
            marg = np.where(np.isnan(marg), np.inf, marg)             # inf - inf on an open window: no limit there
            grazing = np.abs(a) < MARGIN * le[None] * np.linalg.norm(d, axis=2)
            acc = (np.abs(a) >= float(EPS)) & (marg >= 0).all(0)
            stab = (np.abs(marg) >= MARGIN).all(0) & ~grazing & np.isfinite(t)
            inw = np.isfinite(t) & (t >= lo) & (t <= hi)
        ok = alive[s:s + chunk, None]
        out["accepted"][s:s + chunk] = acc & ok
        out["stable"][s:s + chunk] = stab | ~ok                       # a dead ray's empty row is certain
        out["in_window"][s:s + chunk] = inw & ok
        out["t"][s:s + chunk] = t
    return out


def ray_sets(tris, seed, per_kind=512):
    """The rays of the tests on one scene, four kinds of per_kind rays each, concatenated: from outside towards interior points,
    from inside the scene box in random directions, the outside rays with a random [tmin, tmax] window, and the inside rays
    with tmax = +inf and a positive tmin.  Origins are jittered and directions random, so no ray is axis-aligned or aimed at
    a vertex.  -> RAY array"""
    rng = np.random.default_rng(seed)
    V = np.asarray(tris, F).reshape(-1, 3).astype(np.float64)
    lo, hi = V.min(0), V.max(0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())
    span = np.maximum(hi - lo, 0.05 * ext)
    n = per_kind
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = c + u * ext * 1.5
    target = c + (rng.random((n, 3)) - 0.5) * span
    outside = np.zeros(n, RAY)
    outside["origin"], outside["dir"] = o, (target - o) * rng.uniform(0.3, 2.0, (n, 1))
    outside["tmin"], outside["tmax"] = 0.0, 1e30
    inside = np.zeros(n, RAY)
    dirs = rng.normal(size=(n, 3))
    inside["origin"], inside["dir"] = c + (rng.random((n, 3)) - 0.5) * span * 0.9, dirs * rng.uniform(0.5, 2.0, (n, 1))
    inside["tmin"], inside["tmax"] = 0.0, 1e30
    window = outside.copy()
    a, b = rng.random(n) * 1.2, rng.random(n) * 1.2
    window["tmin"], window["tmax"] = np.minimum(a, b), np.maximum(a, b)
    inf = inside.copy()
    inf["dir"] = -inside["dir"]
    inf["tmin"], inf["tmax"] = 1e-3, np.inf
    return np.concatenate([outside, inside, window, inf])
