"""numpy restatement of the capsule block of include/rt_abi.h (rt_prepare_capsules, rt_intersect_rays_capsules), written from
the header alone and sharing no code with the kernels:

  * prepare_f32       the prepare arithmetic, bit for bit (valid mask, padded boxes, proxy triangles);
  * capsule_test_f32  the float32 capsule test, every operation rounded on its own, on anything that broadcasts -- dense_f32
                      runs it as a rays x capsules evaluation; a degenerate capsule goes through sphere_ref.sphere_test_f32;
  * brute64           a float64 brute force over the union of the body and the two end spheres: the entry is the least and the
                      exit the greatest crossing of the three solids' surfaces (the union is convex); nearest and second
                      nearest candidate, identical capsules canonicalised;
  * slab_f32          the float32 slab test of the box phase (sphere_ref's);
  * scenes, rays and the shared, cached Reference of every (scene, seed) the tests use.

Stability of a ray is sphere_ref's, from float64 alone (E = 1e-4): the brute force with a loosened (tmin(1-E), tmax(1+E),
r(1+E)) and a tightened (tmin(1+E), tmax(1-E), r(1-E)) problem agrees with the plain one on hit / miss and capsule (`same`),
and the nearest t lies more than 1e-4 * max(1, |t|) below the second nearest (`gap`).  CAP: the share of a batch that may be
unstable -- conditions on the scenes, not measurements (strand: neighbours share their joint sphere, so at a joint the two
nearest crossings coincide by construction and the gap rule alone takes 3 to 4 % of the rays; those rays are still held to t).

T_TOL: |t32 - t64| / max(1, |t64|) of this restatement against brute64 on the stable hits of each scene, the maximum over the
seeds, measured by tests/test_capsule_ref_cpu.py on the CPU (never on GPU output) and rounded up to two digits; the GPU test
allows GPU_TOL_FACTOR times that: one factor of 2 for scenes x seeds not being the whole input space, one for the moved()
steps.  On `far` an ulp of the coordinates is 7.6e-6."""
import functools

import numpy as np

import sphere_ref as sr

F = np.float32
RAY, HIT, MISS = sr.RAY, sr.HIT, sr.MISS
RT_CAPSULE_BAD = 1
PAD = F(2.0 ** -18)
E = 1e-4
CAP = {"fibres": 0.01, "strand": 0.06, "far": 0.01}
SCENES = ("fibres", "strand", "far")
SEEDS = (21, 22)
NUM_RAYS = 4096
# lower bounds on what the batches exercise: half of the shares the scenes were designed to give
MIN_HIT = {"fibres": 0.29, "strand": 0.215, "far": 0.435}
MIN_FAR = {"fibres": 0.0055, "strand": 0.0055, "far": 0.11}
MIN_BODY = {"fibres": 0.415, "strand": 0.49, "far": 0.19}     # of the stable hits: 0 < v < 1
T_TOL = {"fibres": 1.6e-6, "strand": 2.8e-6, "far": 4.9e-5}   # measured: 1.55e-6, 2.76e-6, 4.89e-5
GPU_TOL_FACTOR = 4.0

slab_f32 = sr.slab_f32


# ------------------------------------------------------------------ scenes
def pack(p0, r, p1):
    """float32 [n, 8]: p0, radius, p1, pad (zero bits)"""
    p0, p1 = np.asarray(p0, np.float64).reshape(-1, 3), np.asarray(p1, np.float64).reshape(-1, 3)
    out = np.zeros((p0.shape[0], 8), F)
    out[:, 0:3], out[:, 4:7] = p0, p1
    out[:, 3] = r
    return out


def scene(name):
    if name == "fibres":
        rng = np.random.default_rng(7)
        n = 1500
        mid = rng.uniform(-1.0, 1.0, size=(n, 3))
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        half = 0.5 * rng.uniform(0.05, 0.4, size=n)[:, None]
        r = np.exp(rng.uniform(np.log(0.005), np.log(0.04), size=n))
        return pack(mid - half * u, r, mid + half * u)
    if name == "strand":      # one chain: neighbours share their joint sphere
        s = np.linspace(0.0, 1.0, 1001)
        rad = 0.3 + 0.7 * s
        p = np.stack([rad * np.cos(40 * np.pi * s), rad * np.sin(40 * np.pi * s), 2 * s - 1], axis=1).astype(F)
        return pack(p[:-1], 0.03, p[1:])
    if name == "far":         # large coordinates; every tenth a sphere; two enclosing capsules: inside rays leave by far roots
        rng = np.random.default_rng(11)
        n = 800
        c = np.array([60.0, -35.0, 20.0])
        mid = c + rng.uniform(-0.5, 0.5, size=(n, 3))
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        half = 0.5 * rng.uniform(0.02, 0.3, size=n)[:, None]
        half[::10] = 0.0
        r = rng.uniform(0.01, 0.05, size=n)
        caps = pack(mid - half * u, r, mid + half * u)
        big = pack([c - (1, 0, 0), c], [3.0, 0.5], [c + (1, 0, 0), c + (0, 0.3, 0)])
        return np.ascontiguousarray(np.vstack([caps, big]), F)
    raise KeyError(name)


def invalid_capsules(mid, extent):
    """four capsules no query may hit, placed where every ray would: a NaN end point, a negative, NaN and infinite radius"""
    c = pack(np.tile(mid - 0.1 * extent, (4, 1)), extent, np.tile(mid + 0.1 * extent, (4, 1)))
    c[0, 5] = np.nan
    c[1, 3] = -extent
    c[2, 3] = np.nan
    c[3, 3] = np.inf
    return c


def end_points(capsules):
    """the end points of the valid capsules as sphere_ref spheres of radius r: float32 [2m, 4]"""
    c = np.asarray(capsules, F).reshape(-1, 8)
    c = c[valid(c)]
    return np.ascontiguousarray(np.vstack([c[:, 0:4], np.hstack([c[:, 4:7], c[:, 3:4]])]), F)


def gpu_scene(name):
    """the scene the tests run: scene(name) plus the four invalid capsules in its middle"""
    c = scene(name)
    _, _, mid, ext = sr.centre_box(end_points(c))
    return np.ascontiguousarray(np.vstack([c, invalid_capsules(mid, ext)]), F)


def moved(capsules, step):
    """the scene after `step` frames of motion: both ends displaced, radii scaled (float32 in, float32 out)"""
    rng = np.random.default_rng(2000 + step)
    out = capsules.copy()
    n = capsules.shape[0]
    out[:, 0:3] += (rng.uniform(-0.05, 0.05, size=(n, 3)) * step).astype(F)
    out[:, 4:7] += (rng.uniform(-0.05, 0.05, size=(n, 3)) * step).astype(F)
    out[:, 3] *= rng.uniform(0.7, 1.3, size=n).astype(F)
    return np.ascontiguousarray(out, F)


def make_rays(capsules, seed, n=NUM_RAYS, with_radius=False):
    """sphere_ref.make_rays over the box of the end points (with_radius: of the end spheres)"""
    return sr.make_rays(end_points(capsules), seed, n, with_radius)


# ------------------------------------------------------------------ prepare
def valid(capsules):
    c = np.asarray(capsules, F).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(c[:, 0:3]).all(axis=1) & np.isfinite(c[:, 4:7]).all(axis=1) & (c[:, 3] >= 0) & (c[:, 3] < np.inf)


def prepare_f32(capsules):
    """(proxies float32 [n, 9] = {lo, hi, lo*0.5 + hi*0.5}, valid mask, status word)"""
    c = np.asarray(capsules, F).reshape(-1, 8)
    ok = valid(c)
    with np.errstate(all="ignore"):
        p0, r, p1 = c[:, 0:3], c[:, 3:4], c[:, 4:7]
        lo, hi = np.minimum(p0 - r, p1 - r), np.maximum(p0 + r, p1 + r)
        e = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
        pad = e * PAD
        lo, hi = lo - pad, hi + pad
        mid = lo * F(0.5) + hi * F(0.5)
    assert lo.dtype == F and hi.dtype == F and mid.dtype == F
    prox = np.hstack([lo, hi, mid])
    prox[~ok] = 0
    return np.ascontiguousarray(prox, F), ok, (0 if ok.all() else RT_CAPSULE_BAD)


# ------------------------------------------------------------------ the float32 test
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _cap(gx, gy, gz, dx, dy, dz, a, r):
    """the header's cap(g): (near, far, ok)"""
    bg = -_dot(gx, gy, gz, dx, dy, dz)
    sg = bg / a
    px, py, pz = gx + sg * dx, gy + sg * dy, gz + sg * dz
    l2 = _dot(px, py, pz, px, py, pz)
    disc = r * r - l2
    hh = np.sqrt(disc / a)
    return sg - hh, sg + hh, disc >= 0


def _crossing(far, tau, y, nn, hn, n, q, d, a, r):
    """the header's entry (far = False) or exit (far = True): (root, v, ok)"""
    body = (y > -hn) & (y < hn)
    p0side = y <= -hn
    side = np.where(p0side, F(0.5), F(-0.5))
    cn, cf, cok = _cap(q[0] + side * n[0], q[1] + side * n[1], q[2] + side * n[2], *d, a, r)
    root = np.where(body, tau, cf if far else cn)
    v = np.where(body, y / nn + F(0.5), np.where(p0side, F(0.0), F(1.0)))
    return root, v, body | cok


def capsule_test_f32(ox, oy, oz, dx, dy, dz, tmin, tmax, ax, ay, az, r, bx, by, bz):
    """the header's test on float32 arrays that broadcast (a = p0, b = p1): (t, far, v) -- t is NaN where the capsule is
    rejected or not valid"""
    args = [np.asarray(v) for v in (ox, oy, oz, dx, dy, dz, tmin, tmax, ax, ay, az, r, bx, by, bz)]
    assert all(v.dtype == F for v in args)
    ox, oy, oz, dx, dy, dz, tmin, tmax, ax, ay, az, r, bx, by, bz = args
    half = F(0.5)
    with np.errstate(all="ignore"):
        n = (bx - ax, by - ay, bz - az)
        degenerate = (n[0] == 0) & (n[1] == 0) & (n[2] == 0)
        if degenerate.any():
            ts, fars = sr.sphere_test_f32(ox, oy, oz, dx, dy, dz, tmin, tmax, ax, ay, az, r)
        else:
            ts, fars = F(np.nan), False

        d = (dx, dy, dz)
        fx, fy, fz = ox - (ax * half + bx * half), oy - (ay * half + by * half), oz - (az * half + bz * half)
        a = _dot(*d, *d)
        b = -_dot(fx, fy, fz, *d)
        s = b / a
        q = (fx + s * dx, fy + s * dy, fz + s * dz)
        nn, nd, nq, qd, qq = _dot(*n, *n), _dot(*n, *d), _dot(*n, *q), _dot(*q, *d), _dot(*q, *q)
        A = nn * a - nd * nd
        C = nn * (qq - r * r) - nq * nq
        hn = nn * half
        # A > 0
        B = nn * qd - nq * nd
        h = B * B - A * C
        sq = np.sqrt(h)
        tau1, tau2 = (-B - sq) / A, (-B + sq) / A
        y1, y2 = nq + tau1 * nd, nq + tau2 * nd
        e_np, ve_np, ok1 = _crossing(False, tau1, y1, nn, hn, n, q, d, a, r)
        x_np, vx_np, ok2 = _crossing(True, tau2, y2, nn, hn, n, q, d, a, r)
        ok_np = (h >= 0) & ok1 & ok2
        # !(A > 0)
        fwd = nd > 0
        side = np.where(fwd, half, -half)
        en, _, eok = _cap(q[0] + side * n[0], q[1] + side * n[1], q[2] + side * n[2], *d, a, r)
        _, xf, xok = _cap(q[0] - side * n[0], q[1] - side * n[1], q[2] - side * n[2], *d, a, r)
        ok_p = ~(C > 0) & eok & xok
        ve_p, vx_p = np.where(fwd, F(0), F(1)), np.where(fwd, F(1), F(0))

        skew = A > 0
        entry, exit_ = np.where(skew, e_np, en), np.where(skew, x_np, xf)
        ve, vx = np.where(skew, ve_np, ve_p), np.where(skew, vx_np, vx_p)
        ok = np.where(skew, ok_np, ok_p) & (r >= 0) & (r != np.inf)
        tn, tf = s + entry, s + exit_
        assert tn.dtype == F and tf.dtype == F and ve.dtype == F and vx.dtype == F
        near = ok & (tn >= tmin) & (tn <= tmax)
        far = ok & ~near & (tf >= tmin) & (tf <= tmax)
        t = np.where(near, tn, np.where(far, tf, F(np.nan)))
        v = np.where(near, ve, np.where(far, vx, F(0)))

        t = np.where(degenerate, ts, t).astype(F)
        far = np.where(degenerate, fars, far)
        v = np.where(degenerate | np.isnan(t), F(0), v).astype(F)
    return t, far, v


_cols = sr._cols


def _ccols(c):
    return [np.ascontiguousarray(c[..., k]) for k in (0, 1, 2, 3, 4, 5, 6)]


def pair_f32(rays, capsules, ids):
    """the test of ray i against capsules[ids[i]] in the ray's own window: (t, far, v)"""
    c = np.asarray(capsules, F).reshape(-1, 8)[ids]
    return capsule_test_f32(*_cols(rays), *_ccols(c))


def dense_f32(rays, capsules, chunk=256):
    """rays x capsules: per ray the minimum t over all capsules (+inf: none) and the capsule, root and v that give it"""
    c = np.asarray(capsules, F).reshape(-1, 8)
    n = rays.shape[0]
    tmin = np.full(n, np.inf, F)
    arg = np.full(n, -1, np.int64)
    far = np.zeros(n, bool)
    vv = np.zeros(n, F)
    for i in range(0, n, chunk):
        sl = slice(i, min(i + chunk, n))
        t, f, v = capsule_test_f32(*[x[:, None] for x in _cols(rays, sl)], *[x[None, :] for x in _ccols(c)])
        t = np.where(np.isnan(t), F(np.inf), t)
        k = t.argmin(axis=1)
        row = np.arange(t.shape[0])
        tmin[sl] = t[row, k]
        hit = t[row, k] < np.inf
        arg[sl] = np.where(hit, k, -1)
        far[sl] = f[row, k] & hit
        vv[sl] = np.where(hit, v[row, k], F(0))
    return tmin, arg, far, vv


# ------------------------------------------------------------------ float64
def canonical(capsules):
    """index of the first exact copy of every capsule"""
    _, first, inv = np.unique(np.ascontiguousarray(capsules, F).view(np.dtype((np.void, 32))).reshape(-1), return_index=True,
                              return_inverse=True)
    return first[inv.reshape(-1)]


def _interval_union(starts, ends):
    """[least start, greatest end] over the non-empty intervals (start <= end); (+inf, -inf) when all are empty"""
    lo, hi = np.full(starts[0].shape, np.inf), np.full(starts[0].shape, -np.inf)
    for s, e in zip(starts, ends):
        ok = s <= e
        lo = np.where(ok & (s < lo), s, lo)
        hi = np.where(ok & (e > hi), e, hi)
    return lo, hi


def brute64(rays, capsules, lo=None, hi=None, rscale=1.0, chunk=256):
    """float64 brute force over the valid first copies: dict(hit, id (canonical index, -1: miss), t, t2 (the nearest candidate
    of any OTHER capsule, +inf: none), far)"""
    c = np.asarray(capsules, F).reshape(-1, 8)
    keep = np.flatnonzero(valid(c) & (canonical(c) == np.arange(c.shape[0])))
    p0, p1 = c[keep, 0:3].astype(np.float64), c[keep, 4:7].astype(np.float64)
    r = c[keep, 3].astype(np.float64) * rscale
    o, d = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    lo = rays["tmin"].astype(np.float64) if lo is None else lo
    hi = rays["tmax"].astype(np.float64) if hi is None else hi
    nr = o.shape[0]
    out = dict(hit=np.zeros(nr, bool), id=np.full(nr, -1, np.int64), t=np.full(nr, np.inf), t2=np.full(nr, np.inf),
               far=np.zeros(nr, bool))
    if keep.size == 0:
        return out
    axis, m = (p1 - p0)[None], (0.5 * (p0 + p1))[None]
    nn = (axis * axis).sum(axis=2)
    for i in range(0, nr, chunk):
        sl = slice(i, min(i + chunk, nr))
        with np.errstate(all="ignore"):
            dd = d[sl, None, :]
            a = (dd * dd).sum(axis=2)
            f = o[sl, None, :] - m
            s = -(f * dd).sum(axis=2) / a
            q = f + s[..., None] * dd          # all roots in tau = t - s

            def sphere(g):
                sg = -(g * dd).sum(axis=2) / a
                p = g + sg[..., None] * dd
                disc = r[None, :] ** 2 - (p * p).sum(axis=2)
                hh = np.sqrt(disc / a)
                return np.where(disc >= 0, sg - hh, np.inf), np.where(disc >= 0, sg + hh, -np.inf)
            a0, b0 = sphere(q + 0.5 * axis)
            a1, b1 = sphere(q - 0.5 * axis)
            # the finite cylinder: the infinite one cut by the slab |y| <= nn / 2
            nd, nq = (axis * dd).sum(axis=2), (axis * q).sum(axis=2)
            A = nn * a - nd * nd
            B = nn * (q * dd).sum(axis=2) - nq * nd
            C = nn * ((q * q).sum(axis=2) - r[None, :] ** 2) - nq * nq
            h = B * B - A * C
            skew = A > 1e-12 * nn * a
            sq = np.sqrt(h)
            c_lo = np.where(skew, np.where(h >= 0, (-B - sq) / A, np.inf), np.where(C <= 0, -np.inf, np.inf))
            c_hi = np.where(skew, np.where(h >= 0, (-B + sq) / A, -np.inf), np.where(C <= 0, np.inf, -np.inf))
            ta, tb = (-0.5 * nn - nq) / nd, (0.5 * nn - nq) / nd
            moving = nd != 0
            inside = np.abs(nq) <= 0.5 * nn
            s_lo = np.where(moving, np.minimum(ta, tb), np.where(inside, -np.inf, np.inf))
            s_hi = np.where(moving, np.maximum(ta, tb), np.where(inside, np.inf, -np.inf))
            body = np.broadcast_to(nn > 0, A.shape)
            c_lo = np.where(body, np.maximum(c_lo, s_lo), np.inf)
            c_hi = np.where(body, np.minimum(c_hi, s_hi), -np.inf)
            entry, exit_ = _interval_union((a0, a1, c_lo), (b0, b1, c_hi))
            tn, tf = s + entry, s + exit_
            l, u = lo[sl, None], hi[sl, None]
            any_ = entry <= exit_
            near = any_ & (tn >= l) & (tn <= u)
            far = any_ & ~near & (tf >= l) & (tf <= u)
            t = np.where(near, tn, np.where(far, tf, np.inf))
        k = t.argmin(axis=1)
        row = np.arange(t.shape[0])
        best = t[row, k]
        hit = best < np.inf
        t[row, k] = np.inf
        out["hit"][sl] = hit
        out["id"][sl] = np.where(hit, keep[k], -1)
        out["t"][sl] = best
        out["t2"][sl] = t.min(axis=1)
        out["far"][sl] = far[row, k] & hit
    return out


def stability(rays, capsules):
    """(plain brute force, same mask, stable mask = same & gap)"""
    lo, hi = rays["tmin"].astype(np.float64), rays["tmax"].astype(np.float64)
    plain = brute64(rays, capsules)
    loose = brute64(rays, capsules, lo * (1 - E), hi * (1 + E), 1 + E)
    tight = brute64(rays, capsules, lo * (1 + E), hi * (1 - E), 1 - E)
    same = (plain["hit"] == loose["hit"]) & (plain["hit"] == tight["hit"]) & (plain["id"] == loose["id"]) & \
           (plain["id"] == tight["id"])
    with np.errstate(invalid="ignore"):
        gap = ~plain["hit"] | (plain["t2"] - plain["t"] > 1e-4 * np.maximum(1.0, np.abs(plain["t"])))
    return plain, same, same & gap


def t_error(t32, t64):
    """|t32 - t64| / max(1, |t64|)"""
    t64 = np.asarray(t64, np.float64)
    return np.abs(np.asarray(t32, np.float64) - t64) / np.maximum(1.0, np.abs(t64))


class Reference:
    """everything the checks need about one (capsules, rays) problem, computed once and never written to"""

    def __init__(self, capsules, rays):
        self.capsules, self.rays = capsules, rays
        self.canon = canonical(capsules)
        self.f64, self.same, self.stable = stability(rays, capsules)
        self.t32, self.id32, self.far32, self.v32 = dense_f32(rays, capsules)
        for a in (self.capsules, self.rays, self.canon, self.same, self.stable, self.t32, self.id32, self.far32, self.v32,
                  *self.f64.values()):
            a.setflags(write=False)

    @property
    def unstable_share(self):
        return 1.0 - float(self.stable.mean())


@functools.lru_cache(maxsize=None)
def reference(name, seed, step=0):
    """the shared reference of gpu_scene(name) (after `step` frames of moved()) under make_rays(.., seed)"""
    c = gpu_scene(name)
    if step:
        c = moved(c, step)
    return Reference(c, make_rays(c, seed))
