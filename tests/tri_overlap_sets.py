"""The query sets of the triangle-overlap tests, shared by the CPU test that proves them non-trivial
(tests/test_tri_overlap_ref_cpu.py) and the GPU test that runs them (tests/test_gpu_tri_overlaps.py), over the scenes of
tests/range_sets.py.  Each set holds NQ query triangles (float32 [NQ, 9]); sizes and displacements are fractions of each
neighbourhood's own scale (range_sets._local_scale), fixed here on the CPU so that every set returns something for at least a
quarter of its queries and at least NQ ids in total.
  moved       scene triangles, every corner displaced by 0.05 .. 0.5 of the local scale in a random direction of its own (a
              rigid step leaves a triangle parallel to its original, which it then never cuts: too few matches on the soup)
  small       random triangles of 0.75 .. 4 local scales, centred at near-surface points
  coincident  exact copies of scene triangles (the coplanar axes; each matches at least itself)
  degenerate  points on vertices and segments through edge midpoints"""
import numpy as np

from range_sets import NQ, SCENES, _local_scale, scene_tris, seed_of  # noqa: F401  (re-exported for the tests)

F = np.float32
KINDS = ("moved", "small", "coincident", "degenerate")


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def query_sets(tris, seed):
    """{kind: float32 [NQ, 9]}"""
    rng = np.random.default_rng(seed + 2000)
    T = np.asarray(tris, F).reshape(-1, 3, 3)
    T64 = T.astype(np.float64)
    n = T.shape[0]
    out = {}
    # moved: a scene triangle with each corner displaced on its own
    k = rng.integers(0, n, NQ)
    s = _local_scale(T64[k].mean(1), tris)
    step = _unit(rng, 3 * NQ).reshape(NQ, 3, 3) * (s[:, None] * rng.uniform(0.05, 0.5, (NQ, 3)))[:, :, None]
    out["moved"] = (T64[k] + step).astype(F).reshape(NQ, 9)
    # small: three random corners around a near-surface point -- a point of a scene triangle, moved off its plane by up to
    # 0.3 of the local scale (the point tests' near-surface set moves by a fraction of the SCENE's extent: on the fractal,
    # which spans 2^-10 .. 2^45, that is far from every small triangle)
    k = rng.integers(0, n, NQ)
    on = (rng.dirichlet((1, 1, 1), NQ)[:, :, None] * T64[k]).sum(1)
    s = _local_scale(on, tris)
    p = on + _unit(rng, NQ) * (s * rng.uniform(0.0, 0.3, NQ))[:, None]
    size = s * rng.uniform(0.75, 4.0, NQ)
    out["small"] = (p[:, None, :] + rng.uniform(-0.5, 0.5, (NQ, 3, 3)) * size[:, None, None]).astype(F).reshape(NQ, 9)
    # coincident: the scene's own triangles, bit for bit
    out["coincident"] = T[rng.integers(0, n, NQ)].reshape(NQ, 9).copy()
    # degenerate: a point on a vertex (even queries), a segment through an edge midpoint along a random direction (odd ones)
    k = rng.integers(0, n, NQ)
    j = rng.integers(0, 3, NQ)
    vert = T64[k, j]
    mid = (T64[k, j] + T64[k, (j + 1) % 3]) * 0.5
    s = _local_scale(mid, tris)
    half = _unit(rng, NQ) * (s * rng.uniform(0.2, 1.0, NQ))[:, None]
    seg = np.stack([mid - half, mid + half, mid + half], axis=1)
    pt = np.repeat(vert[:, None, :], 3, axis=1)
    out["degenerate"] = np.where((np.arange(NQ) % 2 == 0)[:, None, None], pt, seg).astype(F).reshape(NQ, 9)
    return out
