"""Reference closest-point queries in numpy: what rt_closest_points must return, restated from include/rt_abi.h with no code
shared with the kernel.

d2(p, a, b, c) is the float32 routine of the header, line for line: Ericson's ClosestPtPointTriangle (vertex regions, then the
regions of the edges that have a length, then the face point where s stands clear of the rounding noise of its products, else
the nearest of the three edge points unless the face point is a point of the triangle and none of them is strictly nearer;
dots (x*x' + y*y') + z*z'; every division guarded, every edge weight clamped to [0, 1] by selects), then the clamp of the
point into the triangle's vertex box (np.fmax then np.fmin: they drop NaN as fmaxf / fminf do), then dist2 = (dx*dx + dy*dy) +
dz*dz.  numpy float32 arithmetic is IEEE single with round-to-nearest and no contraction: the kernel's -ffp-contract=off
arithmetic.

brute_force(points, dist2_max, tris) is the lexicographic minimum of (dist2, id) over the triangles with dist2 <= dist2_max, the
record every exact tree must return.  closest_f64 is an independent float64 closest point for accuracy checks."""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
FACE_NOISE = F(2.0 ** -20)      # s at or below this share of the sum of its products' magnitudes is rounding noise


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _guard(num, den):
    with np.errstate(all="ignore"):
        q = num / np.where(den > 0, den, F(1))
    return np.where(den > 0, q, F(0)).astype(F)


def _clamp01(t):
    t = np.where(t > 0, t, F(0))
    return np.where(t < 1, t, F(1)).astype(F)


def _clamped_d2(p, q, lo, hi):
    """dist2 of p to q after q is clamped into [lo, hi] componentwise (fmaxf, then fminf)"""
    d = [p[k] - np.fmin(np.fmax(q[k], lo[k]), hi[k]) for k in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def d2(p, a, b, c):
    """p, a, b, c: float32 arrays [..., 3] (broadcast).  Returns (dist2, u, v) float32 arrays: u, v = weights of b and c."""
    p, a, b, c = (np.asarray(x, F) for x in (p, a, b, c))
    P = [p[..., k] for k in range(3)]
    A = [a[..., k] for k in range(3)]
    B = [b[..., k] for k in range(3)]
    C = [c[..., k] for k in range(3)]
    with np.errstate(all="ignore"):
        ab = [B[k] - A[k] for k in range(3)]
        ac = [C[k] - A[k] for k in range(3)]
        bc = [C[k] - B[k] for k in range(3)]
        ap = [P[k] - A[k] for k in range(3)]
        bp = [P[k] - B[k] for k in range(3)]
        cp = [P[k] - C[k] for k in range(3)]
        d1, d2_ = _dot(*ab, *ap), _dot(*ac, *ap)
        d3, d4 = _dot(*ab, *bp), _dot(*ac, *bp)
        d5, d6 = _dot(*ab, *cp), _dot(*ac, *cp)
        vc = d1 * d4 - d3 * d2_
        vb = d5 * d2_ - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        t_ab = _clamp01(_guard(d1, d1 - d3))
        t_ac = _clamp01(_guard(d2_, d2_ - d6))
        t_bc = _clamp01(_guard(e43, e43 + e56))
        q_ab = [A[k] + t_ab * ab[k] for k in range(3)]
        q_ac = [A[k] + t_ac * ac[k] for k in range(3)]
        q_bc = [B[k] + t_bc * bc[k] for k in range(3)]
        s = (va + vb) + vc
        fv = _guard(vb, s)            # (only used where s > 0: the guard is the plain division there)
        fw = _guard(vc, s)
        q_f = [(A[k] + ab[k] * fv) + ac[k] * fw for k in range(3)]
        lo = [np.fmin(np.fmin(A[k], B[k]), C[k]) for k in range(3)]
        hi = [np.fmax(np.fmax(A[k], B[k]), C[k]) for k in range(3)]

        # the nearest of the three edge points by the clamped float dist2, ties to AB, then AC
        g_ab, g_ac, g_bc = (_clamped_d2(P, q, lo, hi) for q in (q_ab, q_ac, q_bc))
        fb_d = g_ab
        fb_u, fb_v = t_ab, np.zeros_like(t_ab)
        take = g_ac < fb_d
        fb_d = np.where(take, g_ac, fb_d)
        fb_u, fb_v = np.where(take, F(0), fb_u), np.where(take, t_ac, fb_v)
        take = g_bc < fb_d
        fb_d = np.where(take, g_bc, fb_d)
        fb_u, fb_v = np.where(take, F(1) - t_bc, fb_u), np.where(take, t_bc, fb_v)

        # region selection in Ericson's order (the first region whose test holds)
        regions = [
            ((d1 <= 0) & (d2_ <= 0), A, F(0), F(0)),
            ((d3 >= 0) & (d4 <= d3), B, F(1), F(0)),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0) & ((d1 - d3) > 0), q_ab, t_ab, F(0)),
            ((d6 >= 0) & (d5 <= d6), C, F(0), F(1)),
            ((vb <= 0) & (d2_ >= 0) & (d6 <= 0) & ((d2_ - d6) > 0), q_ac, F(0), t_ac),
            ((va <= 0) & (e43 >= 0) & (e56 >= 0) & ((e43 + e56) > 0), q_bc, F(1) - t_bc, t_bc),
        ]
        shape = np.broadcast(d1, P[0]).shape
        q = [np.zeros(shape, F) for _ in range(3)]
        u = np.zeros(shape, F)
        v = np.zeros(shape, F)
        done = np.zeros(shape, bool)
        for cond, qq, uu, vv in regions:
            sel = cond & ~done
            for k in range(3):
                q[k] = np.where(sel, qq[k], q[k])
            u, v = np.where(sel, uu, u), np.where(sel, vv, v)
            done |= sel
        dist = _clamped_d2(P, q, lo, hi)
        # no vertex or edge region.  s is the squared area (times 4) as a sum of six products; where it stands clear of their
        # rounding noise the face point is taken as Ericson takes it.  Where it does not (a collinear triangle: va, vb, vc are
        # rounding residues) the face point only if its weights are those of a point of the triangle and no edge point is
        # strictly nearer, else the nearest edge point
        noise = ((np.abs(d1 * d4) + np.abs(d3 * d2_)) + (np.abs(d5 * d2_) + np.abs(d1 * d6))) + (np.abs(d3 * d6) + np.abs(d5 * d4))
        clear = s > FACE_NOISE * noise                         # (false for a NaN)
        g_f = _clamped_d2(P, q_f, lo, hi)
        face = (s > 0) & (clear | ((fv >= 0) & (fw >= 0) & ((fv + fw) <= 1) & ~(fb_d < g_f)))
        dist = np.where(done, dist, np.where(face, g_f, fb_d)).astype(F)
        u = np.where(done, u, np.where(face, fv, fb_u)).astype(F) + F(0)       # + 0: -0 becomes +0, as in the kernel
        v = np.where(done, v, np.where(face, fw, fb_v)).astype(F) + F(0)
    return dist, u, v


def box_d2(p, lo, hi):
    """the pruning bound of a slot box: g = max(lo - p, p - hi, 0) per axis, (gx*gx + gy*gy) + gz*gz in float32"""
    p, lo, hi = (np.asarray(x, F) for x in (p, lo, hi))
    with np.errstate(all="ignore"):
        g = np.fmax(np.fmax(lo - p, p - hi), F(0))
        return ((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]).astype(F)


def traced(points, dist2_max):
    """queries the call traces: finite p, dist2_max not NaN and not negative"""
    points = np.asarray(points, F)
    dist2_max = np.asarray(dist2_max, F)
    return np.isfinite(points).all(axis=-1) & ~np.isnan(dist2_max) & (dist2_max >= 0)


def brute_force(points, dist2_max, tris, chunk=1 << 22):
    """(dist2, id, u, v) per query: the lexicographic minimum of (dist2, id) over the triangles with dist2 <= dist2_max;
    a miss (and an untraced query) is (+inf, MISS, 0, 0).  tris: float32 [n, 9]."""
    P = np.asarray(points, F).reshape(-1, 3)
    R = np.broadcast_to(np.asarray(dist2_max, F), (P.shape[0],))
    T = np.asarray(tris, F).reshape(-1, 3, 3)
    n, m = T.shape[0], P.shape[0]
    out_d = np.full(m, np.inf, F)
    out_i = np.full(m, MISS, np.uint32)
    out_u = np.zeros(m, F)
    out_v = np.zeros(m, F)
    ok = traced(P, R)
    step = max(1, chunk // max(n, 1))
    for s in range(0, m, step):
        idx = np.nonzero(ok[s:s + step])[0] + s
        if idx.size == 0 or n == 0:
            continue
        d, u, v = d2(P[idx, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])
        within = d <= R[idx, None]
        dd = np.where(within, d, np.inf)
        best = dd.min(axis=1)
        # the lowest id among the triangles at the minimum (argmax of the first True)
        at = (dd == best[:, None]) & within
        j = np.argmax(at, axis=1)
        hit = at.any(axis=1)
        rows = np.arange(idx.size)
        out_d[idx] = np.where(hit, best, np.inf)
        out_i[idx] = np.where(hit, j, MISS).astype(np.uint32)
        out_u[idx] = np.where(hit, u[rows, j], 0)
        out_v[idx] = np.where(hit, v[rows, j], 0)
    return out_d, out_i, out_u, out_v


def closest_f64(p, a, b, c):
    """float64 distance from p to triangle abc (independent of d2: face projection when it falls inside, else the nearest
    point of the three edge segments).  Arrays [..., 3]; returns the distance (not squared)."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))

    def seg(p, a, b):
        ab = b - a
        den = (ab * ab).sum(-1)
        with np.errstate(all="ignore"):
            t = np.where(den > 0, ((p - a) * ab).sum(-1) / np.where(den > 0, den, 1), 0)
        t = np.clip(t, 0, 1)
        q = a + t[..., None] * ab
        return np.sqrt(((p - q) ** 2).sum(-1))

    best = np.minimum(np.minimum(seg(p, a, b), seg(p, a, c)), seg(p, b, c))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        h = ((p - a) * n).sum(-1) / np.where(nn > 0, nn, 1)
        f = p - h[..., None] * n                       # projection onto the plane
        # inside test by the signs of the sub-triangle normals
        s0 = (np.cross(b - a, f - a) * n).sum(-1)
        s1 = (np.cross(c - b, f - b) * n).sum(-1)
        s2 = (np.cross(a - c, f - c) * n).sum(-1)
        inside = (nn > 0) & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
        face = np.abs(h) * np.sqrt(nn)
    return np.where(inside, np.minimum(face, best), best)


def brute_force_f64(points, tris):
    """float64 minimum distance per point over all triangles"""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    T = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    out = np.empty(P.shape[0])
    step = max(1, (1 << 21) // max(T.shape[0], 1))
    for s in range(0, P.shape[0], step):
        d = closest_f64(P[s:s + step, None, :], T[None, :, 0], T[None, :, 1], T[None, :, 2])
        out[s:s + step] = d.min(axis=1)
    return out
