"""The query sets of the range-query tests, shared by the CPU test that proves them non-trivial (tests/test_range_ref_cpu.py)
and the GPU test that runs them (tests/test_gpu_range_queries.py).  Points come from the point-query tests' generator
(near-surface, uniform in the 1.5x box, exactly on vertices / edge midpoints); radii and box sizes are fractions of each
triangle-neighbourhood's own scale, fixed here on the CPU so that every set returns something for at least a quarter of its
queries and at least NQ ids in total."""
import numpy as np

from test_gpu_point_queries import _point_sets
from test_gpu_ray_queries import _scene

F = np.float32
NQ = 512
SCENES = ("grid", "soup", "cornell", "signed_zero", "fractal")


def scene_tris(name, scenes):
    return np.ascontiguousarray(_scene(name, scenes)[0], F).reshape(-1, 9)


def _local_scale(points, tris):
    """per point: the distance to the 8th nearest triangle centroid (float64) -- a radius that finds a handful of triangles
    whatever the scene's scale (the fractal spans 2^-10 .. 2^45)"""
    c = tris.reshape(-1, 3, 3).astype(np.float64).mean(1)
    d = np.sqrt(((points[:, None, :].astype(np.float64) - c[None]) ** 2).sum(2))
    k = min(8, c.shape[0]) - 1
    return np.partition(d, k, axis=1)[:, k]


def sphere_queries(points, radius):
    q = np.zeros(len(points), dtype=[("p", "<f4", 3), ("dist2_max", "<f4")])
    q["p"] = points
    with np.errstate(over="ignore"):
        q["dist2_max"] = (np.asarray(radius, np.float64) ** 2).astype(F)
    return q


def box_queries(lo, hi):
    q = np.zeros(len(lo), dtype=[("lo", "<f4", 3), ("pad0", "<u4"), ("hi", "<f4", 3), ("pad1", "<u4")])
    q["lo"], q["hi"] = lo, hi
    q["pad0"], q["pad1"] = 0xDEADBEEF, 0x7FC00000          # the pad words are not read
    return q


def query_sets(tris, seed):
    """{(shape, kind): queries}: shape "sphere" -> POINT_QUERY records, "box" -> RANGE_BOX records"""
    pts = {k: v[:NQ] for k, v in _point_sets(tris, seed).items()}
    rng = np.random.default_rng(seed + 1000)
    out = {}
    for kind in ("near", "uniform"):
        p = pts[kind]
        s = _local_scale(p, tris)
        out["sphere", kind] = sphere_queries(p, s * rng.uniform(0.3, 2.0, NQ))
        half = s[:, None] * rng.uniform(0.1, 1.5, (NQ, 3))
        out["box", kind] = box_queries((p - half).astype(F), (p + half).astype(F))
    # exactly on vertices and edge midpoints: a radius of 0 (a vertex is at d2 = 0 of every triangle that shares it) for half
    # of the queries, a small one for the rest; boxes that are flat on one axis, through the point
    p = pts["on_vertex_edge"]
    s = _local_scale(p, tris)
    out["sphere", "on_vertex_edge"] = sphere_queries(p, np.where(np.arange(NQ) % 2 == 0, 0.0, s * 0.5))
    half = s[:, None] * rng.uniform(0.1, 1.0, (NQ, 3))
    half[np.arange(NQ), rng.integers(0, 3, NQ)] = 0.0
    out["box", "on_vertex_edge"] = box_queries((p - half).astype(F), (p + half).astype(F))
    return out


def seed_of(name):
    return sum(name.encode())
