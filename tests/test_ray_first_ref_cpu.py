"""CPU tests of the first-K reference (tests/ray_first_ref.py), the yardstick of tests/test_gpu_ray_first.py:
1. on test_ray_hits_ref_cpu.py's hand-made tree (restated here) the gates and E for k = 1, 2, 3 are the values known by
   construction;
2. a sequential pure-Python model of the header's definition (a bound, a stack of (entry, front), a sorted list) gives E on every
   decided ray and satisfies claims 1 and 3 on every ray -- in the kernel's order (nearest front first, ties to the lower slot)
   and in the opposite one (farthest first, ties to the higher slot, triangle B before A), with and without re-testing a pending
   entry when it is popped;
3. the condition the GPU test rests on: on the oracle-built trees of the four scenes with the ray sets used there, at most 2 %
   of the live rays with a non-empty all-hit row are undecided, for every k the GPU test uses."""
import numpy as np
import pytest

import range_sets as rs
import ray_first_ref as rf
from test_gpu_ray_queries import _ora_tree

F = np.float32
KS = (1, 2, 3, 8, 32)
ORACLE_TREES = ("bottom_up", "pairs", "hybrid", "sah", "sah_pairs", "sah_splits", "sah_pairs_splits")   # (no oracle builder for hybrid + pairs)


def hand_tree(rt):
    """slot 0: the root run (one BOX slot) -> the run [2, 5): a single-triangle leaf, a NONE slot, a pair leaf.
    leaf 0: triangle 7 in the plane z = 1, stored with rotation 1; leaf 1: the unit quad in z = 2 as the pair (10, 11),
    A = (v0, v1, v2), B = (v2, v1, v3), B stored with rotation 2"""
    nodes = np.zeros(5, rt.NODE)
    leaves = np.zeros(2, rt.TRIANGLE_PAIR)
    leaves["v0"][0], leaves["v1"][0], leaves["v2"][0] = (0, 0, 1), (1, 0, 1), (0, 1, 1)
    leaves["v3"][0] = leaves["v2"][0]
    leaves["primitive_id_0"][0], leaves["rotations"][0] = 7, (1, 0)
    leaves["v0"][1], leaves["v1"][1], leaves["v2"][1], leaves["v3"][1] = (0, 0, 2), (1, 0, 2), (0, 1, 2), (1, 1, 2)
    leaves["primitive_id_0"][1], leaves["primitive_id_1"][1], leaves["rotations"][1] = 10, 11, (0, 2)
    nodes["min"][0], nodes["max"][0] = (0, 0, 1), (1, 1, 2)
    nodes["w12"][0], nodes["w28"][0] = 3 << 29, (rt.CHILD_BOX << 29) | 2
    nodes["min"][2], nodes["max"][2] = (0, 0, 1), (1, 1, 1)
    nodes["w12"][2], nodes["w28"][2] = 1 << 29, (rt.CHILD_TRI << 29) | 0
    nodes["min"][3], nodes["max"][3] = (-9, -9, -9), (9, 9, 9)                   # NONE: never examined, whatever its box
    nodes["w12"][3], nodes["w28"][3] = 0, (rt.CHILD_NONE << 29) | 1
    nodes["min"][4], nodes["max"][4] = (0, 0, 2), (1, 1, 2)
    nodes["w12"][4], nodes["w28"][4] = 2 << 29, (rt.CHILD_TRI << 29) | 1
    return nodes, leaves


def hand_rays():
    r = np.zeros(8, rf.RAY)
    r["dir"] = (0.01, 0.02, 1.0)
    r["tmin"], r["tmax"] = 0.0, np.inf
    r["origin"][:] = (0.2, 0.2, 0.0)
    r["origin"][1] = (0.8, 0.8, 0.0)
    r["tmax"][2] = 1.5
    r["tmin"][3] = 1.5
    r["origin"][4] = (5.0, 5.0, 0.0)
    r["tmin"][5], r["tmax"][5] = 2.0, 1.0                     # dead: tmin > tmax
    r["dir"][6, 1] = np.nan                                   # dead: a NaN direction
    r["origin"][7] = (0.3, 0.6, 0.0)                          # (0.31, 0.62) at z = 1: A of leaf 0; (0.32, 0.64) at z = 2: A of leaf 1
    return r


# ------------------------------------------------------------------ the sequential model of the definition
def model_row(nodes, leaves, root, count, ray, k, *, reverse=False, recull=True):
    """one ray through the header's definition, one step at a time -> a row of k HIT records"""
    if count == 0 or not rf.live(np.array([ray], rf.RAY))[0]:
        return rf.miss_records(k)
    o, d = ray["origin"].astype(F)[None], ray["dir"].astype(F)[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1.0) / d).astype(F)
    tmin, tmax = F(ray["tmin"]), F(ray["tmax"])
    bound = tmax
    lst = []                                                  # HIT scalars, ascending in (t, id)
    stack = []                                                # (is_leaf, index, slot count, front)
    cur = (False, root & rf.INDEX_MASK, count, F(-np.inf))

    def offer(rec):
        nonlocal bound
        if len(lst) == k and not rf.below(rec, lst[-1]):
            return
        if any(rf.same_key(np.array([e], rf.HIT), np.array([rec], rf.HIT))[0] for e in lst):
            return
        pos = sum(1 for e in lst if rf.below(e, rec))
        lst.insert(pos, rec)
        del lst[k:]
        if len(lst) == k:
            bound = tmax if np.isnan(lst[-1]["t"]) else F(lst[-1]["t"])

    while cur is not None:
        is_leaf, index, cnt, _ = cur
        if is_leaf:
            L = leaves[index:index + 1]
            tests = [(("v0", "v1", "v2"), "primitive_id_0", 0, True),
                     (("v2", "v1", "v3"), "primitive_id_1", 1, bool((L["v3"].view(np.uint32) != L["v2"].view(np.uint32)).any()))]
            for corners, pid, which, wanted in (tests[::-1] if reverse else tests):
                if not wanted:
                    continue
                ok, t, bu, bv = rf.mt_f32(L[corners[0]], L[corners[1]], L[corners[2]], o, d, tmin, bound)
                if ok[0]:
                    offer(rf.records(t, L[pid], bu, bv, L["rotations"][:, which])[0])
        else:
            survivors = []
            for s in range(index, index + cnt):
                nd = nodes[s:s + 1]
                typ = int(nd["w28"][0] >> 29)
                if typ == rf.NONE:
                    continue
                front, back = rf.slab(nd["min"], nd["max"], o, inv)
                front, back = front[0], back[0]
                with np.errstate(invalid="ignore"):
                    if not (back >= front and front <= bound and back >= tmin):
                        continue
                child, ccount = int(nd["w28"][0] & rf.INDEX_MASK), int(nd["w12"][0] >> 29)
                if typ != rf.TRI and ccount == 0:
                    continue
                survivors.append((typ == rf.TRI, child, ccount, front))
            if survivors:
                fronts = [x[3] for x in survivors]
                if reverse:                                   # farthest first, ties to the higher slot
                    pick = max(range(len(survivors)), key=lambda j: (fronts[j], j))
                    rest = [x for j, x in enumerate(survivors) if j != pick][::-1]
                else:                                         # nearest first, ties to the lower slot
                    pick = min(range(len(survivors)), key=lambda j: (fronts[j], j))
                    rest = [x for j, x in enumerate(survivors) if j != pick]
                stack.extend(rest)
                cur = survivors[pick]
                continue
        cur = None
        while stack:
            e = stack.pop()
            if recull and e[3] > bound:
                continue
            cur = e
            break
    row = rf.miss_records(k)
    row[:len(lst)] = lst
    return row


def check_model(nodes, leaves, root, count, rays, ks, what):
    rows, gates, _, _ = rf.walk_gated(nodes, leaves, root, count, rays)
    decided_rays = 0
    for k in ks:
        exp = rf.expected(rows, gates, k, rays["tmax"])
        for reverse, recull in ((False, True), (True, True), (False, False), (True, False)):
            for i, ray in enumerate(rays):
                row = model_row(nodes, leaves, root, count, ray, k, reverse=reverse, recull=recull)
                why = rf.envelope_violation(row, rows[i], gates[i], k, ray["tmax"])
                assert why is None, f"{what}: k {k}, reverse {reverse}, recull {recull}, ray {i}: {why}"
                E, decided, _ = exp[i]
                if decided:
                    want = rf.miss_records(k)
                    want[:len(E)] = E
                    assert row.tobytes() == want.tobytes(), \
                        f"{what}: k {k}, reverse {reverse}, recull {recull}, decided ray {i}: {row} is not E = {E}"
        decided_rays += sum(e[1] for e in exp)
    return rows, decided_rays


# ------------------------------------------------------------------ 1: known values
def test_gates_and_expected_rows_on_the_hand_made_tree(rt):
    nodes, leaves = hand_tree(rt)
    rays = hand_rays()
    rows, gates, box_tests, leaf_visits = rf.walk_gated(nodes, leaves, 0, 1, rays)
    import ray_hits_ref as rh
    ref_rows, bt, lv = rh.walk(nodes, leaves, 0, 1, rays)
    assert (box_tests, leaf_visits) == (bt, lv) == (5 * 3 + 1, 2 + 2 + 1 + 1 + 2)
    for a, b in zip(rh.canon(rows), rh.canon(ref_rows)):
        assert (a == b).all(), "walk_gated's rows are the all-hit walk's"
    # the root slot's box starts at z = 1, leaf slot 2 is the plane z = 1, leaf slot 4 the plane z = 2; the rays have
    # dir.z = 1 and origin.z = 0, so the slab fronts are exactly 1, 1 and 2: gate 1 for triangle 7, gate 2 for 10 and 11
    by_id = [{int(r["primitive_id"]): float(g) for r, g in zip(row, gate)} for row, gate in zip(rows, gates)]
    assert by_id == [{7: 1.0, 10: 2.0}, {11: 2.0}, {7: 1.0}, {10: 2.0}, {}, {}, {}, {7: 1.0, 10: 2.0}]
    want = {1: [[7], [11], [7], [10], [], [], [], [7]],
            2: [[7, 10], [11], [7], [10], [], [], [], [7, 10]],
            3: [[7, 10], [11], [7], [10], [], [], [], [7, 10]]}
    for k in (1, 2, 3):
        exp = rf.expected(rows, gates, k, rays["tmax"])
        assert [e[0]["primitive_id"].tolist() for e in exp] == want[k]
        assert all(e[1] for e in exp), "every ray of the hand-made tree is decided"
        # T1: the t of the (k+1)-th record (triangle 10 at t = 2 behind triangle 7), else the ray's tmax
        t1 = [float(e[2]) for e in exp]
        assert t1[1:7] == [np.inf, 1.5, np.inf, np.inf, 1.0, np.inf]
        assert (abs(t1[0] - 2) < 1e-6 and abs(t1[7] - 2) < 1e-6) if k == 1 else (t1[0] == np.inf and t1[7] == np.inf)
    e0 = rf.expected(rows, gates, 2, rays["tmax"])[0][0]
    assert abs(e0["t"][0] - 1) < 1e-6 and abs(e0["t"][1] - 2) < 1e-6 and abs(e0["u"][0] - 0.22) < 1e-6


def test_expected_and_envelope_on_made_up_rows():
    """the bookkeeping alone: duplicates, ties, NaN, an undecided ray, and rows the envelope must refuse"""
    W = np.zeros(6, rf.HIT)
    W["t"] = [3.0, 1.0, 2.0, 2.0, 1.0, np.nan]
    W["primitive_id"] = [5, 9, 8, 4, 9, 1]
    W["u"] = [0.1, 0.2, 0.3, 0.4, 0.2, 0.5]
    g = np.array([0.5, 1.5, 0.2, 0.3, 0.9, 0.1], F)            # (1.0, 9) twice: the smaller gate 0.9 counts
    ws, gs = rf.dedup_sorted(W, g)
    assert ws["primitive_id"].tolist() == [9, 4, 8, 5, 1] and gs.tolist() == [F(0.9), F(0.3), F(0.2), F(0.5), F(0.1)]
    (E, decided, t1), = rf.expected([W], [g], 2, [F(10)])
    assert E["primitive_id"].tolist() == [9, 4] and decided and t1 == 2.0      # gates 0.9, 0.3 <= T1 = 2 (the tie's partner)
    (E, decided, t1), = rf.expected([W], [np.array([0.5, 2.5, 0.2, 0.3, 2.5, 0.1], F)], 2, [F(10)])
    assert not decided                                        # (1.0, 9) lies behind a front of 2.5 > T1 = 2
    (E, decided, t1), = rf.expected([W], [g], 5, [F(10)])
    assert len(E) == 5 and decided and t1 == 10.0 and np.isnan(E["t"][4])
    (E, decided, t1), = rf.expected([W], [g], 4, [F(10)])
    assert len(E) == 4 and not decided and np.isnan(t1)       # a NaN T1 decides nothing

    def row_of(idx, k):
        r = rf.miss_records(k)
        r[:len(idx)] = ws[idx]
        return r
    assert rf.envelope_ok(row_of([0, 1], 2), W, g, 2, F(10))
    assert not rf.envelope_ok(row_of([1, 0], 2), W, g, 2, F(10))               # not ascending
    assert not rf.envelope_ok(row_of([0, 2], 2), W, g, 2, F(10))               # (2, 4) has gate 0.3 <= 2 and is below (2, 8)
    assert not rf.envelope_ok(row_of([0], 2), W, g, 2, F(10))                  # a short row that is not all of W
    assert rf.envelope_ok(row_of([0, 1, 2, 3, 4], 7), W, g, 7, F(10))
    bad = row_of([0, 1], 2)
    bad["u"][1] = 0.75
    assert not rf.envelope_ok(bad, W, g, 2, F(10))                             # not a record of W bit for bit
    # a full row may lack what lies behind a front beyond its final bound, and nothing else
    g2 = np.array([0.5, 2.5, 0.2, 0.3, 2.5, 0.1], F)
    assert rf.envelope_ok(row_of([1, 2], 2), W, g2, 2, F(10))                  # (1, 9): gate 2.5 > final bound 2
    assert not rf.envelope_ok(row_of([2, 3], 2), W, g2, 2, F(10))              # (1, 9): gate 2.5 <= final bound 3


# ------------------------------------------------------------------ 2: the model
def test_model_on_the_hand_made_tree(rt):
    nodes, leaves = hand_tree(rt)
    _, decided = check_model(nodes, leaves, 0, 1, hand_rays(), (1, 2, 3), "hand-made tree")
    assert decided == 3 * 8


@pytest.mark.parametrize("tree", ("pairs", "sah_splits"))
def test_model_on_an_oracle_built_tree(scenes, ora, tree):
    tris = scenes.soup(300, 5, size=0.5)                      # a quarter are exact copies: ties on t; splits: duplicates
    leaves, nodes, root, count = _ora_tree(ora, tris, tree)
    rays = rf.ray_sets(tris, 77, per_kind=24)
    rows, decided = check_model(nodes, leaves, root, count, rays, (1, 2, 5), f"soup/{tree}")
    lens = [len(r) for r in rows]
    assert max(lens) >= 6 and sum(n > 0 for n in lens) >= len(rays) // 3, "the ray set is not trivial"
    assert decided >= 3 * len(rays) * 0.9
    with np.errstate(invalid="ignore"):
        assert any((np.diff(np.sort(r["t"])) == 0).any() for r in rows), "the copies must show as ties on t"


# ------------------------------------------------------------------ 3: the cap
@pytest.mark.parametrize("name", ("grid", "soup", "cornell", "fractal"))
def test_undecided_share_of_the_ray_sets(scenes, ora, name):
    tris = rs.scene_tris(name, scenes)
    rays = rf.ray_sets(tris, rf.SEEDS[name])
    assert len(rays) == 2048 and rf.live(rays).all()
    for tree in ORACLE_TREES:
        leaves, nodes, root, count = _ora_tree(ora, tris, tree)
        rows, gates, _, _ = rf.walk_gated(nodes, leaves, root, count, rays)
        for k in KS:
            share = rf.undecided_share(rf.expected(rows, gates, k, rays["tmax"]), rows)
            print(f"{name}/{tree}: k {k}: {100 * share:.3f} % of {sum(len(r) > 0 for r in rows)} rays undecided")
            assert share <= rf.CAP, f"{name}/{tree}: k {k}: {100 * share:.2f} % undecided"
