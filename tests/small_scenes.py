"""The scenes and query sets of the small-scene tests (tests/test_small_scenes_ref_cpu.py on the CPU,
tests/test_gpu_small_scenes.py on the GPU): trees below the sizes at which the builders take their special paths, and
degenerate or badly scaled geometry.  Everything here is a pure function of its arguments: the generators are seeded per
scene by SEED[name], no generator state is shared with another file, and nothing reads the environment.

TINY        n1 .. n5: the first n triangles of scenes.grid_mesh(4, 1) (n1: the one-triangle tree with a Tri slot and a None
            slot in the root run; n2: the pairs builder merges the two triangles of cell 0 into one leaf); twins: triangle 0
            twice (equal Morton codes, equal boxes); n63, n64, n65: one under, exactly and one over a wave's worth -- the first
            n triangles of scenes.grid_mesh(6, 1), because grid_mesh(4, 1) has 32 triangles only.
DEGENERATE  points (40 zero-area triangles: points, repeated-vertex segments, collinear triples, the recipe of
            edge_scenes.signed_zero_mesh's `deg` block), flat (65 soup triangles with z = FLAT_Z), stack (64 bit-identical
            copies of one triangle), clusters (257 triangles of size 0.005 in five clusters about 100 apart), giant (one
            triangle spanning +-500 and 128 of size 0.01), scaled_up / scaled_down (a 200-triangle soup centred on the origin,
            times 1e4 / 1e-3).
CLOSED      tetra (4 triangles) and box (sdf_ref._box_tris, 12 triangles), oriented outwards, for the signed-distance queries.

EMPTY       n0: a tree BUILT from zero triangles, for the bottom-up builder only (N0_TREES): lbvh_tiny_kernel writes a root
            run of two None slots, the all-empty run.  BuildInput.allocate takes n = 0 and test_gpu_parity.test_tiny_builds
            builds and traces that tree; the pairs, hybrid and SAH builders have never been launched with n = 0 by any test,
            so they stay out.  n0 has no box of its own: its query sets are those of proxy(), the twelve triangles of the
            unit cube, so they cover the place where a scene would be.  (The queries' own files pass count = 0 for "empty".)

Query sets, at most 256 queries each (the tests run a scene's ray sets as one batch of at most 384):
rays(name)            ray_hits_ref.ray_sets(tris, seed, per_kind=64) (256 rays), aimed_rays (64 rays at points of triangles,
                      near and steep), and for flat 32 axis-aligned rays through the plane.  Dropped from them by the float64
                      reference alone: flat's rays that cross two of its overlapping coplanar triangles at one t, and giant's
                      aimed rays that meet the huge triangle first
exact_rays(name)      rays without a float64 arm, held to the bit-exact arms only: 32 rays lying exactly in flat's plane (every
                      determinant is 0 or a rounding residue); scaled_down's rays from inside (unit directions: every t is below
                      the float64 reference's absolute margin) and its aimed rays with the direction times 2^20 (at the
                      scene's own scale every determinant is below the kernel's epsilon of 1e-9 and nothing is hit)
points(name)          test_gpu_point_queries._point_sets, 64 per kind; for flat 32 points exactly in the plane more; for stack the
                      triangle's vertices and edge midpoints more
spheres / boxes(name) range_sets.query_sets, 40 per set; for flat boxes with a face exactly in the plane; for stack spheres whose
                      dist2_max is the shared float32 distance exactly, and one float below it
overlap_queries(name) 32 shifted copies of scene triangles (the scene's own triangles, with self_pairs on and off, are taken
                      by the tests directly)"""
import zlib

import numpy as np

import point_ref as pr
import range_sets as rs
import ray_hits_ref as rh
import sdf_ref
from test_gpu_point_queries import _point_sets

F = np.float32
TINY = ("n1", "n2", "n3", "n4", "n5", "twins", "n63", "n64", "n65")
DEGENERATE = ("points", "flat", "stack", "clusters", "giant", "scaled_up", "scaled_down")
OPEN = TINY + DEGENERATE
CLOSED = ("tetra", "box")
EMPTY = "n0"
N0_TREES = ("bottom_up",)     # the builders known to take n = 0 (test_gpu_parity.test_tiny_builds)
SEED = {name: zlib.crc32(name.encode()) % 100000 for name in OPEN + CLOSED + ("scaled", EMPTY)}
FLAT_Z = F(0.375)
LONG = F(2.0 ** 20)           # scaled_down: the factor on the directions of the second half of its rays
NO_F64_PAIRS = ("points",)                # no float64 arm at all: every Moller-Trumbore determinant of `points` is exactly 0
NO_F64_CAST = ("points", "scaled_down")   # no shade_ref.cast arm: its |det| > 1e-12 is not the kernel's |det| >= 1e-9
PER_KIND = 64
TETRA = np.array([(0.1, 0.2, -0.3), (1.3, 0.1, 0.0), (0.4, 1.2, 0.2), (0.5, 0.4, 1.1)])     # the corners of `tetra`


def _soup(scenes, n, name, size):
    return scenes.soup(n, SEED[name], dup_fraction=0.0, size=size).astype(F)


def tris(name, scenes):
    """-> float32 [n, 9], C-contiguous, read-only"""
    if name == EMPTY:
        return np.zeros((0, 9), F)
    if name in ("n1", "n2", "n3", "n4", "n5"):
        t = scenes.grid_mesh(4, 1)[:int(name[1:])]
    elif name in ("n63", "n64", "n65"):
        t = scenes.grid_mesh(6, 1)[:int(name[1:])]
    elif name == "twins":
        t = np.repeat(scenes.grid_mesh(4, 1)[:1], 2, axis=0)
    elif name == "points":
        src = scenes.grid_mesh(6, 3).reshape(-1, 3, 3)
        k = src.shape[0]
        deg = np.empty((40, 3, 3), F)
        for i in range(40):
            a, b = src[(i * 37) % k, 0], src[(i * 53 + 11) % k, 2]
            deg[i] = (np.stack([a, a, a]), np.stack([a, b, b]), np.stack([a, b, (a + b) * F(0.5)]))[i % 3]
        t = deg
    elif name == "flat":
        t = _soup(scenes, 65, name, 0.15).reshape(-1, 3, 3).copy()
        t[:, :, 2] = FLAT_Z
    elif name == "stack":
        t = np.repeat(_soup(scenes, 1, name, 0.3)[:1], 64, axis=0)
    elif name == "clusters":
        rng = np.random.default_rng(SEED[name])
        t = _soup(scenes, 257, name, 0.01).reshape(-1, 3, 3)
        centres = (np.array([[0, 0, 0], [100, 0, 0], [0, 100, 0], [0, 0, 100], [-70, -70, -70]]) + rng.uniform(-5, 5, (5, 3)))
        t = t * F(0.5) + centres.astype(F)[np.arange(257) % 5][:, None, :]
    elif name == "giant":
        t = _soup(scenes, 129, name, 0.01).copy()
        t[0] = np.array([-500, -500, -500, 500, -500, 500, 0, 600, 0], F)
    elif name in ("scaled_up", "scaled_down"):
        t = (_soup(scenes, 200, "scaled", 0.1) - F(0.5)) * F(1e4 if name == "scaled_up" else 1e-3)
    elif name == "tetra":
        a, b, c, d = TETRA
        t = np.array([(a, c, b), (a, b, d), (b, c, d), (a, d, c)])          # outward: the volume (b-a, c-a, d-a) is positive
    elif name == "box":
        t = sdf_ref._box_tris(sdf_ref.BOX_LO, sdf_ref.BOX_HI)
    else:
        raise KeyError(name)
    out = np.ascontiguousarray(np.asarray(t).astype(F).reshape(-1, 9))
    assert np.isfinite(out).all() and out.shape[0] <= 300
    out.setflags(write=False)
    return out


def proxy():
    """the triangles n0's query sets are derived from: the unit cube"""
    out = np.ascontiguousarray(sdf_ref._box_tris((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)).astype(F).reshape(-1, 9))
    out.setflags(write=False)
    return out


def in_tetra(points):
    """inside the tetrahedron of tris("tetra"), by the signs of the four plane distances in float64"""
    a, b, c, d = TETRA.astype(F).astype(np.float64)
    p = np.asarray(points, np.float64)
    faces = ((a, c, b), (a, b, d), (b, c, d), (a, d, c))
    return np.all([((p - f[0]) @ np.cross(f[1] - f[0], f[2] - f[0])) < 0 for f in faces], axis=0)


# ------------------------------------------------------------------ rays
def _ray_array(o, d, tmin=0.0, tmax=np.inf):
    r = np.zeros(len(o), rh.RAY)
    r["origin"], r["dir"], r["tmin"], r["tmax"] = o, d, tmin, tmax
    return r


def aimed_rays(name, t, n=64):
    """n rays at random points of random triangles, from four of the triangle's own sizes away and within about 70 degrees of
    its normal.  The ray sets of ray_hits_ref aim at the scene BOX, which tiny triangles in a wide box (clusters, giant,
    scaled_up) hardly ever fill.  Near and steep by construction: the float32 error of Moller-Trumbore's (t, u, v) grows with
    distance / size and with 1 / cos, and the float64 arms keep the tolerances of the big scenes.  giant's huge triangle is
    not aimed at (edges of 1000 against rays of 0.04: its hits come from the ray_sets rays)."""
    rng = np.random.default_rng(SEED[name] + 6)
    T = t.reshape(-1, 3, 3).astype(np.float64)
    ext = float(np.ptp(T.reshape(-1, 3), axis=0).max())
    k = rng.integers(1 if name == "giant" else 0, len(T), n)
    on = (rng.dirichlet((2, 2, 2), n)[:, :, None] * T[k]).sum(1)
    size = np.ptp(T[k], axis=1).max(1)
    size = np.where(size > 0, size, 1e-3 * ext)
    nrm = np.cross(T[k, 1] - T[k, 0], T[k, 2] - T[k, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    g = rng.normal(size=(n, 3))
    u = nrm * rng.choice([-1.0, 1.0], (n, 1)) + 0.5 * g / np.linalg.norm(g, axis=1)[:, None]
    u /= np.linalg.norm(u, axis=1)[:, None]
    dist = 4 * size
    return _ray_array(on - u * dist[:, None], u * (dist * rng.uniform(0.5, 2.0, n))[:, None], 0.0, np.inf)


def _box_rays(name, t):
    """ray_sets' 256 rays -> (those with a float64 arm, the others).  scaled_down keeps the two kinds from outside only: the
    two kinds from inside have directions of length about 1 whatever the scene's size, so in a scene of 1e-3 every t is below
    the ABSOLUTE margin of 1e-4 that the float64 reference keeps around the ends of a window"""
    r = rh.ray_sets(t, SEED[name], per_kind=PER_KIND)
    if name != "scaled_down":
        return r, r[:0]
    kind = np.arange(len(r)) // PER_KIND
    outside = (kind == 0) | (kind == 2)
    return r[outside], r[~outside]


def rays(name, t):
    """the rays that have a float64 arm where the scene has one: ray_sets (256), aimed_rays (64), and for flat 32 axis-aligned
    rays through the plane"""
    aimed = aimed_rays(name, t)
    if name == "giant":
        # an aimed ray is 0.04 long; where it crosses the huge triangle first, t = distance / 0.04 carries the rounding of
        # coordinates of 500 (3e-5) forty times over.  Such rays are dropped by the float64 reference alone
        b = rh.brute_f64(t, aimed)
        aimed = aimed[~(b["accepted"][:, 0] | (b["in_window"][:, 0] & ~b["stable"][:, 0]))]
    r = np.concatenate([_box_rays(name, t)[0], aimed])
    if name == "flat":
        # +-z exactly, the other components +0 or -0, aimed at points inside triangles
        rng = np.random.default_rng(SEED[name] + 1)
        T = t.reshape(-1, 3, 3).astype(np.float64)
        k = rng.integers(0, len(T), 32)
        on = (rng.dirichlet((1, 1, 1), 32)[:, :, None] * T[k]).sum(1)
        sg = np.where(np.arange(32) % 2 == 0, 1.0, -1.0)
        o = on.copy()
        o[:, 2] = float(FLAT_Z) - sg * rng.uniform(0.5, 2.0, 32)
        d = np.where(rng.random((32, 3)) < 0.5, 0.0, -0.0)
        d[:, 2] = sg * rng.uniform(0.5, 4.0, 32)
        r = np.concatenate([r, _ray_array(o, d)])
        # flat's triangles overlap in their common plane: a ray through an overlap crosses two triangles at ONE t, which no
        # float32 evaluation orders.  Such rays are dropped by the float64 reference alone: a ray stays if at most one
        # triangle is, or within the margins could be, crossed inside its window
        b = rh.brute_f64(t, r)
        r = r[(b["accepted"] | (b["in_window"] & ~b["stable"])).sum(1) <= 1]
    assert rh.live(r).all()
    return r


def exact_rays(name, t):
    """rays WITHOUT a float64 arm, held to the bit-exact arms only: for flat the 32 rays lying in its plane; for scaled_down
    ray_sets' two kinds from inside (see _box_rays) and its aimed rays with the direction times 2^20 (so that determinants
    pass the kernel's epsilon: t is then about 1e-6, far below the absolute margin the float64 reference keeps around a
    window's ends).  Empty for every other scene."""
    if name == "flat":
        return plane_rays(t)
    if name == "scaled_down":
        far = aimed_rays(name, t)
        far["dir"] = far["dir"] * LONG
        return np.concatenate([_box_rays(name, t)[1], far])
    return np.zeros(0, rh.RAY)


def all_rays(name, t):
    return np.concatenate([rays(name, t), exact_rays(name, t)])


def plane_rays(t):
    """32 rays lying exactly in flat's plane (origin.z = FLAT_Z, dir.z = +-0): from outside the scene box across it"""
    rng = np.random.default_rng(SEED["flat"] + 2)
    V = t.reshape(-1, 3).astype(np.float64)
    lo, hi = V.min(0), V.max(0)
    c, ext = (lo + hi) / 2, float((hi - lo).max())
    a = rng.uniform(0, 2 * np.pi, 32)
    u = np.stack([np.cos(a), np.sin(a), np.zeros(32)], 1)
    o = c + u * ext * 1.5
    target = c + (rng.random((32, 3)) - 0.5) * (hi - lo)
    d = (target - o) * rng.uniform(0.3, 2.0, (32, 1))
    o[:, 2] = float(FLAT_Z)
    d[:, 2] = np.where(np.arange(32) % 2 == 0, 0.0, -0.0)
    return _ray_array(o, d, 0.0, 1e30)


# ------------------------------------------------------------------ points
def points(name, t):
    """-> {kind: float32 [k, 3]}"""
    out = {k: np.ascontiguousarray(p[:PER_KIND]) for k, p in _point_sets(t, SEED[name]).items()}
    T = t.reshape(-1, 3, 3)
    if name == "flat":
        rng = np.random.default_rng(SEED[name] + 3)
        V = t.reshape(-1, 3).astype(np.float64)
        lo, hi = V.min(0), V.max(0)
        p = (lo + hi) / 2 + rng.uniform(-0.75, 0.75, (32, 3)) * (hi - lo)
        p[:, 2] = float(FLAT_Z)
        out["in_plane"] = np.ascontiguousarray(p, F)
    if name == "stack":
        a, b, c = (T[0, k].astype(np.float64) for k in range(3))
        out["corners_mids"] = np.ascontiguousarray([a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2], F)
    return out


def all_points(name, t):
    return np.ascontiguousarray(np.concatenate(list(points(name, t).values())), F)


# ------------------------------------------------------------------ spheres and boxes
RANGE_PER_SET = 40


def range_queries(name, t):
    """-> {(shape, kind): queries}, as range_sets.query_sets"""
    out = {k: np.ascontiguousarray(q[:RANGE_PER_SET]) for k, q in rs.query_sets(t, SEED[name]).items()}
    if name == "flat":
        # boxes with one z face exactly in the plane (the other above or below it), and boxes of zero thickness in it
        rng = np.random.default_rng(SEED[name] + 4)
        p = out["box", "near"]["lo"].astype(np.float64)
        half = rng.uniform(0.05, 0.3, (len(p), 3))
        lo, hi = p - half, p + half
        lo[:, 2] = np.where(np.arange(len(p)) % 3 == 0, float(FLAT_Z), float(FLAT_Z) - 0.1)
        hi[:, 2] = np.where(np.arange(len(p)) % 3 == 1, float(FLAT_Z) + 0.1, float(FLAT_Z))
        out["box", "face_in_plane"] = rs.box_queries(lo.astype(F), hi.astype(F))
    if name == "stack":
        # the float32 distance every copy shares, as the radius; then one float below
        T = t.reshape(-1, 3, 3)
        p = out["sphere", "uniform"]["p"].copy()
        d2, _, _ = pr.d2(p, T[:1, 0], T[:1, 1], T[:1, 2])
        d2 = np.asarray(d2, F).reshape(-1)
        at = np.zeros(len(p), out["sphere", "uniform"].dtype)
        at["p"], at["dist2_max"] = p, d2
        below = at.copy()
        below["dist2_max"] = np.where(d2 > 0, np.nextafter(d2, F(0)), F(-1))
        out["sphere", "at_the_distance"], out["sphere", "one_float_below"] = at, below
    return out


# ------------------------------------------------------------------ query triangles
def overlap_queries(name, t):
    """32 copies of scene triangles with every corner moved by a fraction of the triangle's size (a rigid shift of a triangle
    is parallel to it and cuts nothing) -> float32 [32, 9]"""
    rng = np.random.default_rng(SEED[name] + 5)
    T = t.reshape(-1, 3, 3).astype(np.float64)
    k = rng.integers(0, len(T), 32)
    size = np.maximum(np.ptp(T[k], axis=1).max(1), 1e-3 * max(float(np.abs(T).max()), 1e-30))
    q = T[k] + rng.normal(size=(32, 3, 3)) * 0.3 * size[:, None, None]
    return np.ascontiguousarray(q.astype(F).reshape(-1, 9))
