"""numpy restatement of the sphere block of include/rt_abi.h (rt_prepare_spheres, rt_intersect_rays_spheres), written from the
header alone and sharing no code with the kernels:

  * prepare_f32      the prepare arithmetic, bit for bit (valid mask, padded boxes, proxy triangles);
  * sphere_test_f32  the float32 sphere test, every operation rounded on its own, on anything that broadcasts -- dense_f32 runs
                     it as a rays x spheres evaluation;
  * brute64          a float64 brute force (nearest and second nearest candidate, identical spheres canonicalised);
  * slab_f32         the float32 slab test of the box phase (for the padded-box check);
  * scenes, rays and the shared, cached Reference of every (scene, seed) the tests use.

Stability of a ray comes from float64 alone (E = 1e-4): the brute force with a loosened (tmin(1-E), tmax(1+E), r(1+E)) and a
tightened (tmin(1+E), tmax(1-E), r(1-E)) problem agrees with the plain one on hit / miss and sphere, and the nearest t lies
more than 1e-4 * max(1, |t|) below the second nearest.  CAP: at most 1 % of a batch may be unstable -- a condition on the
scenes (motion_ref.CAP's figure for its non-planar scenes), not a measurement."""
import functools

import numpy as np

F = np.float32
RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
HIT = np.dtype([("t", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])
MISS = 0xFFFFFFFF
RT_SPHERE_BAD = 1
PAD = F(2.0 ** -18)
E = 1e-4
CAP = 0.01
SCENES = ("cloud", "lattice", "shell")
SEEDS = (21, 22)
NUM_RAYS = 4096


# ------------------------------------------------------------------ scenes
def scene(name):
    """float32 [n, 4]: centre, radius"""
    if name == "cloud":
        rng = np.random.default_rng(7)
        c = rng.uniform(-1.0, 1.0, size=(1500, 3))
        r = np.exp(rng.uniform(np.log(0.01), np.log(0.08), size=1500))
    elif name == "lattice":   # every neighbour is tangent
        g = (np.arange(10) - 4.5) * 0.2
        c = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        r = np.full(c.shape[0], 0.1)
    elif name == "shell":     # large coordinates; two concentric spheres around everything: every inside ray exits through a far root
        rng = np.random.default_rng(11)
        mid = np.array([60.0, -35.0, 20.0])
        c = mid + rng.uniform(-0.5, 0.5, size=(800, 3))
        r = rng.uniform(0.02, 0.1, size=800)
        c = np.vstack([c, mid, mid])
        r = np.concatenate([r, [3.0, 0.5]])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.hstack([c, r[:, None]]), F)


def invalid_spheres(mid, extent):
    """four spheres no query may hit, placed where every ray would: NaN centre, negative, NaN and infinite radius"""
    s = np.zeros((4, 4), F)
    s[:, :3] = mid
    s[:, 3] = extent
    s[0, 1] = np.nan
    s[1, 3] = -extent
    s[2, 3] = np.nan
    s[3, 3] = np.inf
    return s


def centre_box(spheres, with_radius=False):
    """(lo, hi, middle, extent) of the box of the valid centres (with_radius: of the valid spheres)"""
    ok = valid(spheres)
    c = spheres[ok, :3].astype(np.float64)
    r = spheres[ok, 3:4].astype(np.float64) if with_radius else 0.0
    lo, hi = (c - r).min(axis=0), (c + r).max(axis=0)
    return lo, hi, (lo + hi) / 2, max(float((hi - lo).max()), 1e-3)


def gpu_scene(name):
    """the scene the tests run: scene(name) plus the four invalid spheres in its middle"""
    s = scene(name)
    _, _, mid, ext = centre_box(s)
    return np.ascontiguousarray(np.vstack([s, invalid_spheres(mid, ext)]), F)


def moved(spheres, step):
    """the scene after `step` frames of motion: centres displaced, radii scaled (float32 in, float32 out)"""
    rng = np.random.default_rng(1000 + step)
    out = spheres.copy()
    out[:, :3] += (rng.uniform(-0.05, 0.05, size=(spheres.shape[0], 3)) * step).astype(F)
    out[:, 3] *= rng.uniform(0.7, 1.3, size=spheres.shape[0]).astype(F)
    return np.ascontiguousarray(out, F)


def make_rays(spheres, seed, n=NUM_RAYS, with_radius=False):
    """first half: from a sphere of twice the scene's extent around its middle at random points of the centre box; second
    half: from random points of the box in random directions; |dir| in [0.3, 3]; the last quarter has a finite window.
    with_radius: the box of the spheres instead of the box of their centres (scenes of a few spheres)"""
    rng = np.random.default_rng(seed)
    lo, hi, mid, ext = centre_box(spheres, with_radius)
    h = n // 2
    u = rng.normal(size=(h, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o1 = mid + 2.0 * ext * u
    d1 = lo + rng.random((h, 3)) * (hi - lo) - o1
    o2 = lo + rng.random((n - h, 3)) * (hi - lo)
    d2 = rng.normal(size=(n - h, 3))
    o, d = np.vstack([o1, o2]), np.vstack([d1, d2])
    d *= (rng.uniform(0.3, 3.0, size=n) / np.linalg.norm(d, axis=1))[:, None]
    r = np.zeros(n, RAY)
    r["origin"], r["dir"], r["tmin"], r["tmax"] = o, d, 0.0, np.inf
    q = n - n // 4
    tmax = rng.uniform(0.05, 1.0, size=n - q) * ext
    r["tmax"][q:] = tmax
    r["tmin"][q:] = rng.uniform(0.0, 0.3, size=n - q) * tmax
    return r


# ------------------------------------------------------------------ prepare
def valid(spheres):
    s = np.asarray(spheres, F).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return np.isfinite(s[:, :3]).all(axis=1) & (s[:, 3] >= 0) & (s[:, 3] < np.inf)


def prepare_f32(spheres):
    """(proxies float32 [n, 9] = {lo, hi, lo*0.5 + hi*0.5}, valid mask, status word)"""
    s = np.asarray(spheres, F).reshape(-1, 4)
    ok = valid(s)
    with np.errstate(all="ignore"):
        c, r = s[:, :3], s[:, 3:4]
        lo, hi = c - r, c + r
        e = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True)
        pad = e * PAD
        lo, hi = lo - pad, hi + pad
        mid = lo * F(0.5) + hi * F(0.5)
    assert lo.dtype == F and hi.dtype == F and mid.dtype == F
    prox = np.hstack([lo, hi, mid])
    prox[~ok] = 0
    return np.ascontiguousarray(prox, F), ok, (0 if ok.all() else RT_SPHERE_BAD)


# ------------------------------------------------------------------ the float32 test
def sphere_test_f32(ox, oy, oz, dx, dy, dz, tmin, tmax, cx, cy, cz, r):
    """the header's test on float32 arrays that broadcast: (t, far) -- t is NaN where the sphere is rejected or not valid"""
    args = [np.asarray(v) for v in (ox, oy, oz, dx, dy, dz, tmin, tmax, cx, cy, cz, r)]
    assert all(v.dtype == F for v in args)
    ox, oy, oz, dx, dy, dz, tmin, tmax, cx, cy, cz, r = args
    with np.errstate(all="ignore"):
        fx, fy, fz = ox - cx, oy - cy, oz - cz
        a = (dx * dx + dy * dy) + dz * dz
        b = -((fx * dx + fy * dy) + fz * dz)
        s = b / a
        px, py, pz = fx + s * dx, fy + s * dy, fz + s * dz
        l2 = (px * px + py * py) + pz * pz
        disc = r * r - l2
        ok = (disc >= 0) & (r >= 0) & (r != np.inf)
        h = np.sqrt(disc / a)
        tn, tf = s - h, s + h
        assert tn.dtype == F and tf.dtype == F
        near = ok & (tn >= tmin) & (tn <= tmax)
        far = ok & ~near & (tf >= tmin) & (tf <= tmax)
        t = np.where(near, tn, np.where(far, tf, F(np.nan))).astype(F)
    return t, far


def _cols(rays, sl=slice(None)):
    o, d = rays["origin"][sl], rays["dir"][sl]
    return [np.ascontiguousarray(v, F) for v in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], rays["tmin"][sl],
                                                 rays["tmax"][sl])]


def pair_f32(rays, spheres, ids):
    """the test of ray i against spheres[ids[i]] in the ray's own window: (t, far)"""
    s = np.asarray(spheres, F).reshape(-1, 4)[ids]
    return sphere_test_f32(*_cols(rays), *[np.ascontiguousarray(s[:, k]) for k in range(4)])


def dense_f32(rays, spheres, chunk=512):
    """rays x spheres: per ray the minimum t over all spheres (+inf: none) and the sphere and root that give it"""
    s = np.asarray(spheres, F).reshape(-1, 4)
    n = rays.shape[0]
    tmin = np.full(n, np.inf, F)
    arg = np.full(n, -1, np.int64)
    far = np.zeros(n, bool)
    for i in range(0, n, chunk):
        sl = slice(i, min(i + chunk, n))
        t, f = sphere_test_f32(*[v[:, None] for v in _cols(rays, sl)], *[s[None, :, k] for k in range(4)])
        t = np.where(np.isnan(t), F(np.inf), t)
        k = t.argmin(axis=1)
        row = np.arange(t.shape[0])
        tmin[sl] = t[row, k]
        hit = t[row, k] < np.inf
        arg[sl] = np.where(hit, k, -1)
        far[sl] = f[row, k] & hit
    return tmin, arg, far


def slab_f32(rays, lo, hi, tmax):
    """the box phase's test of ray i against box i (float32 [n, 3] bounds) under tmax[i]: hit mask"""
    o, d = np.ascontiguousarray(rays["origin"], F), np.ascontiguousarray(rays["dir"], F)
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
        t1, t2 = (lo - o) * inv, (hi - o) * inv
        assert t1.dtype == F
        front = np.fmax(np.fmax(np.fmin(t1[:, 0], t2[:, 0]), np.fmin(t1[:, 1], t2[:, 1])), np.fmin(t1[:, 2], t2[:, 2]))
        back = np.fmin(np.fmin(np.fmax(t1[:, 0], t2[:, 0]), np.fmax(t1[:, 1], t2[:, 1])), np.fmax(t1[:, 2], t2[:, 2]))
        return (back >= front) & (front <= tmax) & (back >= rays["tmin"])


# ------------------------------------------------------------------ float64
def canonical(spheres):
    """index of the first exact copy of every sphere"""
    _, first, inv = np.unique(np.ascontiguousarray(spheres, F).view(np.dtype((np.void, 16))).reshape(-1), return_index=True,
                              return_inverse=True)
    return first[inv.reshape(-1)]


def brute64(rays, spheres, lo=None, hi=None, rscale=1.0, chunk=512):
    """float64 brute force over the valid first copies: dict(hit, id (canonical index, -1: miss), t, t2 (the nearest candidate
    of any OTHER sphere, +inf: none), far)"""
    s = np.asarray(spheres, F).reshape(-1, 4)
    keep = np.flatnonzero(valid(s) & (canonical(s) == np.arange(s.shape[0])))
    c, r = s[keep, :3].astype(np.float64), s[keep, 3].astype(np.float64) * rscale
    o, d = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    lo = rays["tmin"].astype(np.float64) if lo is None else lo
    hi = rays["tmax"].astype(np.float64) if hi is None else hi
    n = o.shape[0]
    out = dict(hit=np.zeros(n, bool), id=np.full(n, -1, np.int64), t=np.full(n, np.inf), t2=np.full(n, np.inf),
               far=np.zeros(n, bool))
    if keep.size == 0:
        return out
    for i in range(0, n, chunk):
        sl = slice(i, min(i + chunk, n))
        with np.errstate(all="ignore"):
            f = o[sl, None, :] - c[None, :, :]
            dd = d[sl, None, :]
            a = (dd * dd).sum(axis=2)
            b = -(f * dd).sum(axis=2)
            sp = b / a
            p = f + sp[..., None] * dd
            disc = r[None, :] ** 2 - (p * p).sum(axis=2)
            h = np.sqrt(disc / a)
            tn, tf = sp - h, sp + h
            l, u = lo[sl, None], hi[sl, None]
            near = (disc >= 0) & (tn >= l) & (tn <= u)
            far = (disc >= 0) & ~near & (tf >= l) & (tf <= u)
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


def stability(rays, spheres):
    """(plain brute force, stable mask)"""
    lo, hi = rays["tmin"].astype(np.float64), rays["tmax"].astype(np.float64)
    plain = brute64(rays, spheres)
    loose = brute64(rays, spheres, lo * (1 - E), hi * (1 + E), 1 + E)
    tight = brute64(rays, spheres, lo * (1 + E), hi * (1 - E), 1 - E)
    same = (plain["hit"] == loose["hit"]) & (plain["hit"] == tight["hit"]) & (plain["id"] == loose["id"]) & \
           (plain["id"] == tight["id"])
    with np.errstate(invalid="ignore"):
        gap = ~plain["hit"] | (plain["t2"] - plain["t"] > 1e-4 * np.maximum(1.0, np.abs(plain["t"])))
    return plain, same & gap


class Reference:
    """everything the checks need about one (spheres, rays) problem, computed once and never written to"""

    def __init__(self, spheres, rays):
        self.spheres, self.rays = spheres, rays
        self.canon = canonical(spheres)
        self.f64, self.stable = stability(rays, spheres)
        self.t32, self.id32, self.far32 = dense_f32(rays, spheres)
        for a in (self.spheres, self.rays, self.canon, self.stable, self.t32, self.id32, self.far32, *self.f64.values()):
            a.setflags(write=False)

    @property
    def unstable_share(self):
        return 1.0 - float(self.stable.mean())


@functools.lru_cache(maxsize=None)
def reference(name, seed, step=0):
    """the shared reference of gpu_scene(name) (after `step` frames of moved()) under make_rays(.., seed)"""
    s = gpu_scene(name)
    if step:
        s = moved(s, step)
    return Reference(s, make_rays(s, seed))
