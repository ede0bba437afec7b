"""Reference refit in numpy: what rt_refit must write, restated from the rules in include/rt_abi.h with no code shared with the
kernels.

refit_ref(leaves, nodes, root, count, tris) walks the tree top-down from (root, count), rebuilds every reachable leaf record
from `tris` (the new positions) and recomputes every reachable slot's box bottom-up:
  - a single record (primitive_id_1 == 0): v0..v2 = triangle primitive_id_0, v3 = v2;
  - a pair record (primitive_id_1 == primitive_id_0 + 1): A rotated by rotations[0], v3 = B's corner picked by rotations[1];
    the pair is broken when B's edge named by rotations[1] no longer equals (v2, v1) of the rotated A;
  - a leaf slot's box: ordered min / max over A's corners, plus B's for a pair;
  - a box slot's box: ordered union of the boxes of the non-NONE slots of its child run.
Ordered min / max compare the monotone integer image of the floats (-0 below +0).  Every other byte stays as it is.
Returns (leaves, nodes, pair_broken)."""
import numpy as np

NONE, BOX, TRI = 0, 1, 2
MASK = 0x1FFFFFFF


def ordered(f):
    """float32 -> int64 whose order is the order of the bit patterns read as signed magnitudes (-0 < +0)"""
    i = np.asarray(f, np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7FFFFFFF)


def omin(a, b):
    return np.where(ordered(a) <= ordered(b), a, b).astype(np.float32)


def omax(a, b):
    return np.where(ordered(a) >= ordered(b), a, b).astype(np.float32)


def _corners(leaf, tris):
    """the record rebuilt from `tris`: (v0, v1, v2, v3, corners that bound it, pair broken?)"""
    T = tris.reshape(-1, 3, 3)
    id0, id1 = int(leaf["primitive_id_0"]), int(leaf["primitive_id_1"])
    A = T[id0]
    if id1 == 0:
        return A[0], A[1], A[2], A[2], A, False
    assert id1 == id0 + 1, f"record ids ({id0}, {id1}) are neither a single nor a pair"
    B = T[id1]
    ra, rb = int(leaf["rotations"][0]), int(leaf["rotations"][1])
    r = {0: (A[0], A[1], A[2]), 1: (A[2], A[0], A[1]), 2: (A[1], A[2], A[0])}[ra]
    v3 = {2: B[0], 1: B[1]}.get(rb, B[2])
    # the shared edge: r2 -> r1 is B's edge rb (0: B0 B1, 2: B1 B2, 1: B2 B0), compared as the pairing test compares corners
    # (float ==: -0 and +0 match, as they did when the builder paired the two)
    e = {0: (B[0], B[1]), 2: (B[1], B[2]), 1: (B[2], B[0])}.get(rb, (B[0], B[1]))
    broken = not ((r[2] == e[0]).all() and (r[1] == e[1]).all())
    return r[0], r[1], r[2], v3, np.concatenate([A, B]), broken


def walk(nodes, root, count):
    """reachable runs in top-down order: list of (first slot, length, parent slot or None)"""
    runs, seen = [(root, count, None)], {root}
    i = 0
    while i < len(runs):
        f, k, _ = runs[i]
        for s in range(f, f + k):
            if int(nodes["w28"][s]) >> 29 == BOX:
                c, kc = int(nodes["w28"][s]) & MASK, int(nodes["w12"][s]) >> 29
                assert c not in seen, f"run {c} reached twice"
                seen.add(c)
                runs.append((c, kc, s))
        i += 1
    return runs


def refit_ref(leaves, nodes, root, count, tris):
    leaves, nodes = leaves.copy(), nodes.copy()
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    runs = walk(nodes, root, count) if count else []
    broken = False
    # leaves first (any order: a record shared by several slots gets the same bytes each time)
    for f, k, _ in runs:
        for s in range(f, f + k):
            if int(nodes["w28"][s]) >> 29 != TRI:
                continue
            rec = int(nodes["w28"][s]) & MASK
            v0, v1, v2, v3, C, b = _corners(leaves[rec], tris)
            broken |= b
            leaves["v0"][rec], leaves["v1"][rec], leaves["v2"][rec], leaves["v3"][rec] = v0, v1, v2, v3
            lo, hi = C[0], C[0]
            for c in C[1:]:
                lo, hi = omin(lo, c), omax(hi, c)
            nodes["min"][s], nodes["max"][s] = lo, hi
    # box slots bottom-up: a run's parent after the run
    for f, k, parent in reversed(runs):
        if parent is None:
            continue
        lo = hi = None
        for s in range(f, f + k):
            if int(nodes["w28"][s]) >> 29 == NONE:
                continue
            lo = nodes["min"][s] if lo is None else omin(lo, nodes["min"][s])
            hi = nodes["max"][s] if hi is None else omax(hi, nodes["max"][s])
        assert lo is not None, f"run {f} has no non-NONE slot"
        nodes["min"][parent], nodes["max"][parent] = lo, hi
    return leaves, nodes, broken
