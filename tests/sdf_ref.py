"""Reference for the signed-distance and occupancy queries (rt_signed_distance / rt_occupancy, include/rt_abi.h), numpy only.

compose      the DEFINITION through public calls: ClosestPoints gives (dist2, id), RayHitsCount per vote direction gives the
             crossing counts, the vote and the float32 square root follow.  The GPU-side oracle: the fused kernel must equal it
             bit for bit.
brute_f64    float64 truth over the caller's triangles: unsigned distance, crossing counts per direction, a stability flag per
             point (tests/ray_hits_ref.py's notion: every acceptance quantity at least MARGIN from its limit).
meshes       closed test meshes with an inside test that casts no ray: an axis box, an icosphere (320 triangles), a torus (512,
             genus 1), a shell (a box inside a box, the inner one flipped: the cavity is outside the solid).
truth_set    the stable points of a mesh with their analytic inside bit and float64 distance -- chosen by the reference alone.
lattice      rt_generate_grid_points in numpy, both layouts.
"""
import functools

import numpy as np

import point_ref as pr
import ray_hits_ref as rh

F = np.float32
MISS = 0xFFFFFFFF
MARGIN = rh.MARGIN
SDF_HIT = np.dtype([("sdist", "<f4"), ("primitive_id", "<u4")])
POINT_QUERY = np.dtype([("p", "<f4", 3), ("dist2_max", "<f4")])
DEFAULT_DIRS = np.array([[0.577, 0.211, 0.789], [-0.683, 0.619, 0.387], [0.259, -0.857, 0.446]], F)
# caller directions of the tests: one axis-aligned (a zero component twice over: 1/0 = inf in the slab test), two oblique
CALLER_DIRS = np.array([[0.0, 0.0, 1.0], [0.31, -0.77, 0.52], [-0.45, 0.12, -0.83]], F)
MESHES = ("box", "icosphere", "torus", "shell")
SEEDS = {"box": 1201, "icosphere": 1202, "torus": 1203, "shell": 1204}     # candidate seeds of the CPU and GPU tests
NUM_CANDIDATES = 4000
NEAR = 1e-2                  # candidates closer than this to the surface are dropped before the stable filter
STABLE_SHARE = 0.95          # the stable filter must keep this share of the NUM_CANDIDATES candidates


# ------------------------------------------------------------------ meshes
def _box_tris(lo, hi, flip=False):
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    c = np.array([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)])
    # outward quads
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]
    tris = [(c[a], c[b], c[cc]) for a, b, cc, d in quads] + [(c[a], c[cc], c[d]) for a, b, cc, d in quads]
    t = np.array(tris)
    if flip:
        t = t[:, ::-1]
    return t


BOX_LO, BOX_HI = np.array((-0.7, -0.4, -0.9)), np.array((0.6, 0.8, 0.5))
SHELL_LO, SHELL_HI = np.array((-0.3, -0.1, -0.4)), np.array((0.2, 0.4, 0.1))     # the cavity of the shell


def _icosphere(level=2, radius=0.9, centre=(0.1, -0.05, 0.2)):
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    verts = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid = {}

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        nf = []
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    V = np.array(verts) * radius + np.array(centre)
    return V[np.array(faces)]


def _torus(nu=16, nv=16, R=1.0, r=0.4):
    u = np.arange(nu) * 2 * np.pi / nu
    v = np.arange(nv) * 2 * np.pi / nv
    U, W = np.meshgrid(u, v, indexing="ij")
    P = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1)
    # a generic rotation: no facet is parallel to an axis or to a vote direction by construction of the lattice
    a, b = 0.37, 0.91
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    P = P @ (Rz @ Rx).T + np.array((0.05, -0.1, 0.02))
    tris = []
    for i in range(nu):
        for j in range(nv):
            i1, j1 = (i + 1) % nu, (j + 1) % nv
            tris += [(P[i, j], P[i1, j], P[i1, j1]), (P[i, j], P[i1, j1], P[i, j1])]
    return np.array(tris)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> float32 [n, 9], the caller's triangles.  Shared vertices are bit-identical (built once in float64, then rounded)."""
    if name == "box":
        t = _box_tris(BOX_LO, BOX_HI)
    elif name == "icosphere":
        t = _icosphere()
    elif name == "torus":
        t = _torus()
    elif name == "shell":
        t = np.concatenate([_box_tris(BOX_LO, BOX_HI), _box_tris(SHELL_LO, SHELL_HI, flip=True)])
    else:
        raise KeyError(name)
    out = np.ascontiguousarray(t.astype(F).reshape(-1, 9))
    out.setflags(write=False)
    return out


def winding_f64(tris, points, chunk=512):
    """float64 winding number per point: the sum of the signed solid angles of the triangles (Van Oosterom & Strackee) / 4 pi"""
    T = np.asarray(tris, F).reshape(-1, 3, 3).astype(np.float64)
    P = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.empty(len(P))
    for s in range(0, len(P), chunk):
        a, b, c = (T[None, :, k] - P[s:s + chunk, None, :] for k in range(3))
        la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(2)
        den = la * lb * lc + (a * b).sum(2) * lc + (b * c).sum(2) * la + (c * a).sum(2) * lb
        out[s:s + chunk] = (2 * np.arctan2(num, den)).sum(1) / (4 * np.pi)
    return out


def _in_box(p, lo, hi):
    return np.maximum(lo - p, p - hi).max(1) < 0


def analytic_inside(name, points):
    """inside the SOLID, without casting a ray.  The float32 corners of the boxes are the rounded constants, and every test
    point keeps at least NEAR from the surface, so the float64 constants decide the same way."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if name == "box":
        return _in_box(p, BOX_LO, BOX_HI)
    if name == "shell":
        return _in_box(p, BOX_LO, BOX_HI) & ~_in_box(p, SHELL_LO, SHELL_HI)
    return np.abs(winding_f64(mesh(name), p)) > 0.5


def in_cavity(points):
    return _in_box(np.asarray(points, np.float64).reshape(-1, 3), SHELL_LO, SHELL_HI)


# ------------------------------------------------------------------ float64 truth
def brute_f64(tris, points, dirs, chunk=256):
    """-> dict: dist (float64 unsigned distance), counts [votes, points] (float64 crossing counts of the rays (p, 0, D[j], inf)),
    stable [points]: every (ray, triangle) decision of every direction is certain -- accepted with every acceptance quantity
    (u, 1 - u, v, 1 - u - v, t) at least MARGIN inside its limit, or rejected with one of them at least MARGIN outside, and a
    grazing pair (|det| < MARGIN * |e1| |e2| |d|) only when it is rejected whatever the sign of det (|u| or |v| beyond
    1 + MARGIN)."""
    T = np.asarray(tris, F).reshape(-1, 3, 3).astype(np.float64)
    P = np.asarray(points, F).reshape(-1, 3).astype(np.float64)
    D = np.asarray(dirs, F).reshape(-1, 3).astype(np.float64)
    m = len(P)
    counts = np.zeros((len(D), m), np.int64)
    stable = np.ones(m, bool)
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    le = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    for j, d in enumerate(D):
        h = np.cross(d[None], e2)
        a = (e1 * h).sum(1)
        grazing = np.abs(a) < MARGIN * le * np.linalg.norm(d)
        for s in range(0, m, chunk):
            with np.errstate(all="ignore"):
                f = 1.0 / a[None]
                sv = P[s:s + chunk, None, :] - T[None, :, 0]
                u = f * (sv * h[None]).sum(2)
                q = np.cross(sv, e1[None])
                v = f * (q * d[None, None]).sum(2)
                t = f * (e2[None] * q).sum(2)
                marg = np.stack([u, 1 - u, v, 1 - u - v, t / np.maximum(1.0, np.abs(t))])
                marg = np.where(np.isnan(marg), -np.inf, marg)
                acc = (np.abs(a[None]) >= float(rh.EPS)) & (marg >= 0).all(0)
                sure_in = (marg >= MARGIN).all(0) & ~grazing[None]
                sure_out = np.where(grazing[None], (np.abs(u) > 1 + MARGIN) | (np.abs(v) > 1 + MARGIN) | np.isnan(u),
                                    (marg <= -MARGIN).any(0))
            counts[j, s:s + chunk] = acc.sum(1)
            stable[s:s + chunk] &= (sure_in | sure_out).all(1)
    return {"dist": pr.brute_force_f64(P, np.asarray(tris, F)), "counts": counts, "stable": stable}


def vote(counts):
    """inside = (number of odd counts) * 2 > votes"""
    counts = np.asarray(counts)
    return (counts % 2 == 1).sum(0) * 2 > counts.shape[0]


@functools.lru_cache(maxsize=None)
def truth_set(name, seed=None):
    """The truth points of mesh `name`: NUM_CANDIDATES points drawn uniformly in 1.5 x the mesh box, those closer than NEAR to
    the surface dropped, then the stable ones under the three default directions.  -> dict: points (float32), inside (analytic),
    dist (float64), counts, candidates (how many were drawn), near (how many were dropped)"""
    tris = mesh(name)
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    V = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = V.min(0), V.max(0)
    c, half = (lo + hi) / 2, (hi - lo) / 2
    cand = rng.uniform(c - 1.5 * half, c + 1.5 * half, (NUM_CANDIDATES, 3)).astype(F)
    b = brute_f64(tris, cand, DEFAULT_DIRS)
    far = b["dist"] >= NEAR
    keep = far & b["stable"]
    pts = np.ascontiguousarray(cand[keep])
    return {"points": pts, "inside": analytic_inside(name, pts), "dist": b["dist"][keep], "counts": b["counts"][:, keep],
            "candidates": NUM_CANDIDATES, "near": int((~far).sum())}


# ------------------------------------------------------------------ query sets of the GPU tests
def queries(points, dist2_max=np.inf):
    q = np.zeros(len(points), POINT_QUERY)
    q["p"], q["dist2_max"] = points, dist2_max
    return q


def mixed_points(name, n=2048, seed=7):
    """n float32 points for the composition test: uniform around the mesh, near the surface (1e-5 .. 1e-2 off a random surface
    point), and EXACTLY on it: vertices, edge midpoints and face points as float32."""
    tris = mesh(name).reshape(-1, 3, 3)
    rng = np.random.default_rng(SEEDS[name] + seed)
    V = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = V.min(0), V.max(0)
    c, half = (lo + hi) / 2, (hi - lo) / 2
    k = n // 4                                  # k near the surface, k on it, the other n - 2k uniform
    uni = rng.uniform(c - 1.5 * half, c + 1.5 * half, (n - 2 * k, 3))
    t = tris[rng.integers(0, len(tris), 2 * k)].astype(np.float64)
    w = rng.dirichlet((1, 1, 1), 2 * k)
    surf = (w[:, :, None] * t).sum(1)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    near = surf[:k] + nrm[:k] * (10 ** rng.uniform(-5, -2, k) * rng.choice([-1, 1], k))[:, None]
    on_face = surf[k:]
    t3 = tris[rng.integers(0, len(tris), k)]
    kind = rng.integers(0, 2, k)
    on_edge = np.where(kind[:, None] == 0, t3[:, 0], (t3[:, 0].astype(np.float64) + t3[:, 1]) / 2)
    on = np.concatenate([on_face[:k // 2], on_edge[:k - k // 2]])
    out = np.ascontiguousarray(np.concatenate([uni, near, on]).astype(F))
    assert out.shape == (n, 3)
    return out


# ------------------------------------------------------------------ the composition (GPU, through public calls)
def _rays(q, d, cast):
    """the vote ray of every query: (p, 0, d, +inf); a query that is not cast gets a dead ray (tmin > tmax)"""
    r = np.zeros(len(q), rh.RAY)
    r["origin"], r["dir"] = np.where(cast[:, None], q["p"], 0), d
    r["tmin"], r["tmax"] = np.where(cast, F(0), F(1)), np.where(cast, F(np.inf), F(-1))
    return r


def compose(rt, tree, q, votes=3, dirs=None, distance=True):
    """The definition of rt_signed_distance / rt_occupancy through rt_closest_points and rt_ray_hits_count.
    tree: (triangles, nodes, root, count) device handles; q: POINT_QUERY array.  The third direction is launched for the
    queries whose first two votes disagree only (the others get dead rays), as the fused call casts it.
    -> dict: sdist (float32), primitive_id, inside (uint8), counts [votes, n] (row lengths; 0 where a vote was not cast),
    cast [votes, n], status (all status words ORed), counters (uint64[2]: every traversal that ran; with distance=False
    without the closest-point call's), vote_counters [votes, 2]"""
    import torch
    tri, nod, root, count = tree
    n = len(q)
    D = np.asarray(DEFAULT_DIRS if dirs is None else dirs, F).reshape(-1, 3)[:votes]
    qd = rt.to_device(np.ascontiguousarray(q)).view(torch.float32).view(-1, 4)
    status = 0
    total = np.zeros(2, np.uint64)
    dist2 = np.full(n, np.inf, F)
    prim = np.full(n, MISS, np.uint32)
    if distance:
        hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        rt.ClosestPoints(tri, nod, root, count, qd, hits, counters=ctr, status=st)
        h = hits.cpu().numpy().view(rt.POINT_HIT).reshape(-1)
        dist2, prim = h["dist2"].copy(), h["primitive_id"].copy()
        status |= rt.point_status(st)
        total += ctr.cpu().numpy().astype(np.uint64)[:2]
    traced = pr.traced(q["p"], q["dist2_max"])
    counts = np.zeros((votes, n), np.int64)
    cast = np.zeros((votes, n), bool)
    vote_ctr = np.zeros((votes, 2), np.uint64)
    odd = np.zeros(n, np.int64)
    for j in range(votes):
        cast[j] = traced & ((odd == 1) if j == 2 else True)
        rd = rt.to_device(_rays(q, D[j], cast[j])).view(torch.float32).view(-1, 8)
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        rt.RayHitsCount(tri, nod, root, count, rd, off, counters=ctr, status=st)
        counts[j] = np.diff(off.cpu().numpy())
        status |= rt.ray_hits_status(st)
        vote_ctr[j] = ctr.cpu().numpy().astype(np.uint64)[:2]
        odd += counts[j] % 2
    total += vote_ctr.sum(0)
    inside = odd * 2 > votes
    with np.errstate(invalid="ignore"):
        sd = np.where(prim == MISS, F(np.inf), np.sqrt(dist2, dtype=F)).astype(F)
    sd = np.where(inside & (sd != 0), -sd, sd).astype(F)
    return {"sdist": sd, "primitive_id": prim, "inside": inside.astype(np.uint8), "counts": counts, "cast": cast,
            "status": int(status), "counters": total, "vote_counters": vote_ctr}


# ------------------------------------------------------------------ the lattice
def lattice(origin, spacing, dims, bricks=False, dist2_max=np.inf):
    """rt_generate_grid_points in numpy -> POINT_QUERY array.  float32: one multiplication, then one addition."""
    o, s = np.asarray(origin, F), np.asarray(spacing, F)
    dx, dy, dz = (int(v) for v in dims)
    if min(dx, dy, dz) <= 0:
        return np.zeros(0, POINT_QUERY)
    if bricks:
        nbx, nby, nbz = (dx + 3) // 4, (dy + 3) // 4, (dz + 3) // 4
        t = np.arange(nbx * nby * nbz * 64, dtype=np.int64)
        lane, brick = t & 63, t >> 6
        bx, by, bz = brick % nbx, (brick // nbx) % nby, brick // (nbx * nby)
        i = 4 * bx + ((lane & 1) | ((lane >> 2) & 2))
        j = 4 * by + (((lane >> 1) & 1) | ((lane >> 3) & 2))
        k = 4 * bz + (((lane >> 2) & 1) | ((lane >> 4) & 2))
    else:
        t = np.arange(dx * dy * dz, dtype=np.int64)
        i, j, k = t % dx, (t // dx) % dy, t // (dx * dy)
    on = (i < dx) & (j < dy) & (k < dz)
    q = np.zeros(len(t), POINT_QUERY)
    idx = np.stack([i, j, k], 1).astype(F)
    p = (o[None, :] + (idx * s[None, :]).astype(F)).astype(F)
    q["p"] = np.where(on[:, None], p, F(0))
    q["dist2_max"] = np.where(on, F(dist2_max), F(-1))
    return q


def brick_index(dims):
    """for the brick layout of `dims`: the brick-layout index of every row-major point -> int64 [dx*dy*dz]"""
    dx, dy, dz = (int(v) for v in dims)
    nbx, nby = (dx + 3) // 4, (dy + 3) // 4
    t = np.arange(dx * dy * dz, dtype=np.int64)
    i, j, k = t % dx, (t // dx) % dy, t // (dx * dy)
    lx, ly, lz = i & 3, j & 3, k & 3
    lane = (lx & 1) | ((ly & 1) << 1) | ((lz & 1) << 2) | ((lx >> 1) << 3) | ((ly >> 1) << 4) | ((lz >> 1) << 5)
    return (((k >> 2) * nby + (j >> 2)) * nbx + (i >> 2)) * 64 + lane
