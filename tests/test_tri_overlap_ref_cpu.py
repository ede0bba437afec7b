"""CPU tests of the triangle-overlap restatement (tests/tri_overlap_ref.py) that the GPU tests hold the kernels to:
1. every (scene, query set) the GPU test runs returns something for at least a quarter of its queries and at least NQ ids in
   total, by the reference alone -- a GPU test over empty sets cannot pass; SELF on the soup returns at least 64 pairs, SELF on
   the grid is recorded;
2. the predicate's properties: symmetric where it should be, coincident triangles match, two triangles that touch in one shared
   point match, crossing and separated configurations, coplanar ones (the six in-plane axes), the SELF exclusions;
3. float32 against float64 on the soup and the cornell box: the two predicates agree on every box-overlapping pair whose float64
   gap is at least 1e-4 of the pair's extent (the all-hit tests' margin), and at most 2 % of the pairs are nearer than that."""
import numpy as np
import pytest

import tri_overlap_ref as tr
import tri_overlap_sets as ts

F = np.float32
STABLE = 1e-4           # |sep| >= STABLE * extent: a float64 verdict float32 must reproduce
UNSTABLE_MAX = 0.02     # at most this fraction of the box-overlapping pairs may be nearer than that


# ------------------------------------------------------------------ 1: the GPU query sets are not empty
@pytest.mark.parametrize("name", ts.SCENES)
def test_the_gpu_query_sets_are_not_empty(scenes, name):
    tris = ts.scene_tris(name, scenes)
    sets = ts.query_sets(tris, ts.seed_of(name))
    assert tuple(sets) == ts.KINDS
    for kind, q in sets.items():
        assert q.shape == (ts.NQ, 9) and q.dtype == F and np.isfinite(q).all()
        lists, counts = tr.brute_force(q, tris)
        print(f"{name}/{kind}: non-empty {int((counts > 0).sum())}/{ts.NQ}, ids {int(counts.sum())}, largest {int(counts.max())}")
        assert (counts > 0).sum() * 4 >= ts.NQ, f"{name}/{kind}: only {(counts > 0).sum()} non-empty rows"
        assert counts.sum() >= ts.NQ, f"{name}/{kind}: only {counts.sum()} ids"
        if kind == "coincident":            # a copy of a scene triangle matches at least that triangle
            T = tris.reshape(-1, 9)
            for k in range(0, ts.NQ, 37):
                same = np.nonzero((T.view(np.uint32) == q[k].view(np.uint32)).all(axis=1))[0]
                assert same.size and np.isin(same, lists[k]).all()
    lists, counts = tr.brute_force(tris, tris, self_pairs=True)
    print(f"{name}/SELF: pairs {int(counts.sum())}, rows {int((counts > 0).sum())}/{len(counts)}, largest {int(counts.max())}")
    assert all((x > i).all() for i, x in enumerate(lists))
    if name == "soup":
        assert counts.sum() >= 64


# ------------------------------------------------------------------ 2: properties of the predicate
def _tri(*c):
    return np.array(c, F).reshape(3, 3)


def test_predicate_basics():
    A = _tri((0, 0, 0), (1, 0, 0), (0, 1, 0))
    through = _tri((0.2, 0.2, -1), (0.2, 0.2, 1), (0.9, 0.9, 1))            # pierces A
    above = _tri((0, 0, 0.5), (1, 0, 0.5), (0, 1, 0.5))                    # parallel, boxes apart
    near_miss = _tri((2, 2, -1), (2, 2, 1), (0.6, 0.6, 1))                 # boxes overlap, the triangles do not meet
    for Q, exp in ((through, True), (above, False), (near_miss, False), (A, True)):
        assert bool(tr.cuts(A, Q)) == exp and bool(tr.cuts(Q, A)) == exp
    assert tr.boxes(A, near_miss) and not tr.boxes(A, above)
    # coplanar: only the six in-plane axes can separate (the two normals are parallel, the nine edge crosses too)
    apart = _tri((0.6, 0.6, 0), (1.6, 0.6, 0), (0.6, 1.6, 0))              # same plane, boxes overlap, disjoint
    lapped = _tri((0.25, 0.25, 0), (1.25, 0.25, 0), (0.25, 1.25, 0))       # same plane, overlapping
    assert tr.boxes(A, apart) and not tr.cuts(A, apart) and not tr.cuts(apart, A)
    assert tr.cuts(A, lapped) and tr.cuts(lapped, A)
    ax = tr.axes(A, apart)
    assert (ax[2:11] [:, :2] == 0).all()                                   # the edge crosses all point along z: useless here
    # touching in one shared point matches (strict comparisons): a shared corner, and a corner on the other's interior
    corner = _tri((1, 0, 0), (2, 0, 1), (2, 1, -1))
    tip = _tri((0.25, 0.25, 0), (0.25, 0.25, 1), (1, 1, 1))
    assert tr.cuts(A, corner) and tr.cuts(corner, A) and tr.cuts(A, tip) and tr.cuts(tip, A)
    # degenerate queries are traced: a point on A, a point off A, a segment through A
    on, off = _tri(*[(0.25, 0.25, 0)] * 3), _tri(*[(0.25, 0.25, 0.1)] * 3)
    seg = _tri((0.25, 0.25, -1), (0.25, 0.25, 1), (0.25, 0.25, 1))
    assert tr.cuts(on, A) and tr.cuts(A, on) and not tr.cuts(off, A) and tr.cuts(seg, A) and tr.cuts(A, seg)
    # a NaN corner of Q is dropped by the box fold and never separates
    nanq = A.copy()
    nanq[2, 1] = np.nan
    assert tr.cuts(A, nanq)
    # overflow: a match as long as the boxes overlap
    big = _tri((-3e38, -3e38, -3e38), (3e38, 3e38, 3e38), (3e38, -3e38, 3e38))
    assert tr.cuts(A, big)


def test_symmetry_on_random_pairs():
    """cuts(P, Q) and cuts(Q, P) evaluate different roundings (the corners are taken relative to P's first corner), so they are
    held equal where the float64 verdict is stable, and the box condition is symmetric always"""
    rng = np.random.default_rng(77)
    P = rng.uniform(-1, 1, (4000, 3, 3)).astype(F)
    Q = (P.mean(1, keepdims=True) + rng.uniform(-1, 1, (4000, 3, 3)) * 0.8).astype(F)
    assert (tr.boxes(P, Q) == tr.boxes(Q, P)).all()
    sep, ext = tr.cuts64(P, Q)
    stable = (np.abs(sep) >= STABLE * ext) & tr.boxes(P, Q)
    a, b = tr.cuts(P, Q), tr.cuts(Q, P)
    assert stable.sum() > 1000 and a[stable].any() and not a[stable].all()
    assert (a[stable] == b[stable]).all() and (a[stable] == (sep[stable] <= 0)).all()
    sep2, _ = tr.cuts64(Q, P)
    assert np.allclose(sep, sep2, rtol=0, atol=1e-9)


def test_self_exclusions_and_untraced():
    A = _tri((0, 0, 0), (1, 0, 0), (0, 1, 0))
    B = _tri((0.2, 0.2, -1), (0.2, 0.2, 1), (0.9, 0.9, 1))                  # pierces A, no shared corner
    C = _tri((-0.0, 0.0, -0.0), (0.5, 0.5, 1), (0.5, 0.5, -1))              # pierces A and shares A's corner 0 as -0 / +0
    tris = np.stack([A, B, C]).reshape(-1, 9)
    lists, counts = tr.brute_force(tris, tris, self_pairs=True)
    assert [x.tolist() for x in lists] == [[1], [2], []]                    # (A, C) share a corner; (B, C) cross; j > i only
    lists, _ = tr.brute_force(tris, tris)
    assert [x.tolist() for x in lists] == [[0, 1, 2], [0, 1, 2], [0, 1, 2]]
    assert tr.shares_corner(A, C) and not tr.shares_corner(A, B)
    bad = tris.copy()
    bad[0, 4], bad[1, 8] = np.nan, np.inf
    lists, counts = tr.brute_force(bad, tris)
    assert counts.tolist() == [0, 0, 3]


# ------------------------------------------------------------------ 3: float32 against float64
@pytest.mark.parametrize("name", ("soup", "cornell"))
def test_float32_agrees_with_float64_on_stable_pairs(scenes, name):
    tris = ts.scene_tris(name, scenes)
    T = tris.reshape(-1, 3, 3)
    sets = ts.query_sets(tris, ts.seed_of(name))
    total = unstable = 0
    for kind in ("moved", "small"):
        P = sets[kind].reshape(-1, 3, 3)
        qi, ti = np.nonzero(tr.boxes(P[:, None], T[None]))
        sep, ext = tr.cuts64(P[qi], T[ti])
        stable = np.abs(sep) >= STABLE * ext
        got = tr.no_separating_axis(P[qi], T[ti])
        print(f"{name}/{kind}: box-overlapping pairs {len(qi)}, unstable {int((~stable).sum())}, "
              f"intersecting {int((sep <= 0).sum())}, float32 differs on {int((got != (sep <= 0)).sum())} (all unstable)")
        assert (got[stable] == (sep[stable] <= 0)).all()
        assert (sep[stable] <= 0).any() and (sep[stable] > 0).any()
        total += len(qi)
        unstable += int((~stable).sum())
    assert total >= 1000 and unstable <= UNSTABLE_MAX * total, f"{name}: {unstable} of {total} pairs are unstable"
