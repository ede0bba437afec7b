"""The numpy reference of the instanced first-K ray query (rt_ray_first_hits_instanced), restated from include/rt_abi.h with no
code shared with the kernel.  The contract is stated on the instanced all-hit row W of a ray (20-byte ITEMs) and on the GATE of
each of its items, so the reference is the instanced all-hit walk of tests/ray_hits_instanced_ref.py carrying one more number,
put together from existing pieces:

entered_gated(): ray_hits_instanced_ref.entered's breadth-first TLAS frontier with the running maximum of the slab `front`
    carried down: every entered (ray, instance) pair comes with the largest world-ray front on the path to the instance's
    leaf slot, that slot included.
walk_gated(): instance_ref.object_rays on the record's own bytes, ray_first_ref.walk_gated on each BLAS for the object rays
    (records and BLAS gates), the TLAS gate folded in by fmax.  -> (rows of ITEMs, gates, box tests, leaf visits); the rows and
    counts are ray_hits_instanced_ref.walk's.
dedup_sorted / expected / envelope_violation / padded: ray_first_ref's on ITEMs with the key (t, instance, primitive_id): t
    as floats (-0 equals +0), a NaN t above every number and equal to any other NaN, then the instance, then the id."""
import numpy as np

import instance_ref as ir
import ray_first_ref as rf
import ray_hits_ref as rh
from ray_hits_instanced_ref import ITEM, RECORD, items  # noqa: F401  (the tests take them from here)

F = np.float32
MISS = rf.MISS
MAX_K = rf.MAX_K
CAP = rf.CAP             # the project's own 2 %


def pad_items(n):
    out = np.zeros(n, ITEM)
    out["instance"], out["t"], out["primitive_id"] = MISS, np.inf, MISS
    return out


def entered_gated(tlas_nodes, tlas_leaves, root, count, records, blas_counts, rays):
    """-> (ray index, instance id, TLAS gate) arrays of the entered pairs, in no particular order, and the TLAS's box tests"""
    o, d = rays["origin"].astype(F), rays["dir"].astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1.0) / d).astype(F)
    tmin, tmax = rays["tmin"].astype(F), rays["tmax"].astype(F)
    alive = np.nonzero(rh.live(rays))[0] if count > 0 and len(records) else np.zeros(0, np.int64)
    fr_ray = alive.astype(np.int64)
    fr_first = np.full(len(alive), root & rf.INDEX_MASK, np.int64)
    fr_cnt = np.full(len(alive), count, np.int64)
    fr_gate = np.full(len(alive), -np.inf, F)
    box_tests = 0
    got_ray, got_leaf, got_gate = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, F)]
    while len(fr_ray):
        nr, nf, nc, ng = [], [], [], []
        for s in range(int(fr_cnt.max())):
            sel = fr_cnt > s
            r, slot = fr_ray[sel], fr_first[sel] + s
            nd = tlas_nodes[slot]
            typ = nd["w28"] >> 29
            valid = typ != rf.NONE
            box_tests += int(valid.sum())
            front, back = rf.slab(nd["min"], nd["max"], o[r], inv[r])
            with np.errstate(invalid="ignore"):
                inn = valid & (back >= front) & (front <= tmax[r]) & (back >= tmin[r])
            gate = np.fmax(fr_gate[sel], front)
            child = (nd["w28"] & rf.INDEX_MASK).astype(np.int64)
            ccount = (nd["w12"] >> 29).astype(np.int64)
            is_leaf = inn & (typ == rf.TRI)
            is_box = inn & (typ != rf.TRI) & (ccount > 0)
            got_ray.append(r[is_leaf]); got_leaf.append(child[is_leaf]); got_gate.append(gate[is_leaf])
            nr.append(r[is_box]); nf.append(child[is_box]); nc.append(ccount[is_box]); ng.append(gate[is_box])
        fr_ray, fr_first, fr_cnt, fr_gate = np.concatenate(nr), np.concatenate(nf), np.concatenate(nc), np.concatenate(ng)
    ray, leaf, gate = np.concatenate(got_ray), np.concatenate(got_leaf), np.concatenate(got_gate).astype(F)
    inst = tlas_leaves["primitive_id_0"][leaf].astype(np.int64)
    ok = inst < len(records)
    safe = np.where(ok, inst, 0)
    if len(records):
        blas = records["blas"][safe].astype(np.int64)
        ok &= (records["flags"][safe] == 0) & (blas < len(blas_counts))
        cnt = np.asarray(list(blas_counts) + [0], np.int64)[np.where(blas < len(blas_counts), blas, len(blas_counts))]
        ok &= (cnt >= 1) & (cnt <= 7)
    return ray[ok], inst[ok], gate[ok], box_tests


def walk_gated(tlas_nodes, tlas_leaves, root, count, records, blas_trees, rays):
    """blas_trees[b] = (leaves, nodes, root, count) of table entry b.  -> (rows: one ITEM array per ray, gates: one float32
    array per ray, box tests of both levels, BLAS leaf visits).  A scene without records counts nothing (the header)."""
    n = len(rays)
    ray, inst, tgate, box_tests = entered_gated(tlas_nodes, tlas_leaves, root, count, records, [t[3] for t in blas_trees], rays)
    leaf_visits = 0
    got_ray, got_item, got_gate = [], [], []
    for k in np.unique(inst):
        which = inst == k
        sel = ray[which]
        obj = ir.object_rays(rays[sel], records["world_to_object"][k])
        assert rh.live(obj).all(), "an object ray has a NaN: outside what this reference restates"
        leaves, nodes, broot, bcount = blas_trees[int(records["blas"][k])]
        rows, gates, bt, lv = rf.walk_gated(nodes, leaves, broot, bcount, obj)
        box_tests += bt
        leaf_visits += lv
        lens = [len(x) for x in rows]
        got_ray.append(np.repeat(sel, lens))
        got_item.append(items(k, np.concatenate(rows) if rows else np.zeros(0, rh.HIT)))
        got_gate.append(np.fmax(np.repeat(tgate[which], lens), np.concatenate(gates) if gates else np.zeros(0, F)).astype(F))
    out, out_g = [np.zeros(0, ITEM)] * n, [np.zeros(0, F)] * n
    if got_ray:
        gr, it, gt = np.concatenate(got_ray), np.concatenate(got_item), np.concatenate(got_gate)
        order = np.argsort(gr, kind="stable")
        gr, it, gt = gr[order], it[order], gt[order]
        cuts = np.searchsorted(gr, np.arange(n + 1))
        out = [it[cuts[i]:cuts[i + 1]] for i in range(n)]
        out_g = [gt[cuts[i]:cuts[i + 1]] for i in range(n)]
    return out, out_g, box_tests, leaf_visits


def key_order(it):
    """indices that sort ITEMs by (t, instance, id): NaN t last, -0 with +0"""
    t = it["t"]
    nan = np.isnan(t)
    return np.lexsort((it["primitive_id"], it["instance"], np.where(nan, F(np.inf), t + F(0)), nan))


def sorted_row(it):
    return it[key_order(it)]


def same_key(a, b):
    with np.errstate(invalid="ignore"):
        same_t = (a["t"] == b["t"]) | (np.isnan(a["t"]) & np.isnan(b["t"]))
    return same_t & (a["instance"] == b["instance"]) & (a["primitive_id"] == b["primitive_id"])


def below_all(a, b):
    """key of a below key of b, element by element (arrays, or one item against an array)"""
    ta, tb = a["t"], b["t"]
    na, nb = np.isnan(ta), np.isnan(tb)
    with np.errstate(invalid="ignore"):
        same_t = (ta == tb) | (na & nb)
        tail = (a["instance"] < b["instance"]) | ((a["instance"] == b["instance"]) & (a["primitive_id"] < b["primitive_id"]))
        return (ta < tb) | (~na & nb) | (same_t & tail)


def below(a, b):
    return bool(below_all(a, b))


def dedup_sorted(row, gate):
    """Ws and its gates: sorted by key, one item per key, its gate the smallest of the duplicates'"""
    if len(row) == 0:
        return row, gate
    order = key_order(row)
    row, gate = row[order], gate[order]
    first = np.ones(len(row), bool)
    first[1:] = ~same_key(row[1:], row[:-1])
    group = np.cumsum(first) - 1
    g = np.full(int(group[-1]) + 1, np.inf, F)
    np.minimum.at(g, group, gate)
    return row[first], g


def dedup_all(rows, gates):
    return [dedup_sorted(row, gate) for row, gate in zip(rows, gates)]


def expected(rows, gates, k, tmax, dedup=None):
    """-> per ray: (E: ITEM array of min(k, |Ws|) items, decided: bool, T1: float32)"""
    out = []
    for (ws, g), tm in zip(dedup if dedup is not None else dedup_all(rows, gates), tmax):
        E = ws[:k]
        t1 = F(ws["t"][k]) if len(ws) > k else F(tm)
        with np.errstate(invalid="ignore"):
            decided = bool((g[:k] <= t1).all())
        out.append((E, decided, t1))
    return out


def envelope_violation(row, W, gates, k, tmax):
    """claims 1 and 3 for one output row of k ITEMs against the ray's instanced all-hit row W with its gates.  -> None, or
    what is wrong"""
    assert len(row) == k
    is_live = row["primitive_id"] != MISS
    m = int(is_live.sum())
    if is_live[m:].any():
        return "a pad before a live item"
    if row[m:].tobytes() != pad_items(k - m).tobytes():
        return "the padding is not {+inf, MISS, 0, 0} with instance MISS"
    got = np.ascontiguousarray(row[:m])
    gw = got.view(np.uint32).reshape(m, 5)
    ww = np.ascontiguousarray(W).view(np.uint32).reshape(len(W), 5)
    member = (gw[:, None, :] == ww[None, :, :]).all(2).any(1)
    if not member.all():
        j = int(np.argmin(member))
        return f"item {j} {got[j]} is not in the instanced all-hit row"
    if m > 1 and not below_all(got[:-1], got[1:]).all():
        return f"the items are not strictly ascending in (t, instance, id): {got}"
    ws, g = dedup_sorted(W, gates)
    if m < k:
        if len(ws) != m or not same_key(ws, got).all():
            return f"a row of {m} < k items is not the whole all-hit row ({len(ws)} distinct items)"
        return None
    last = got[m - 1]
    T = F(tmax) if np.isnan(last["t"]) else last["t"]
    with np.errstate(invalid="ignore"):
        owed = below_all(ws, last) & (g <= T)
        same_t = (ws["t"][:, None] == got["t"][None, :]) | (np.isnan(ws["t"])[:, None] & np.isnan(got["t"])[None, :])
    listed = (same_t & (ws["instance"][:, None] == got["instance"][None, :]) &
              (ws["primitive_id"][:, None] == got["primitive_id"][None, :])).any(1)
    if (owed & ~listed).any():
        j = int(np.argmax(owed & ~listed))
        return f"{ws[j]} (gate {g[j]} <= final bound {T}) is below the last item {last} and not in the row"
    return None


def envelope_ok(row, W, gates, k, tmax):
    return envelope_violation(row, W, gates, k, tmax) is None


def padded(exp, k):
    """the rows the kernel writes where they equal E: [n, k] ITEMs, E then pads"""
    out = pad_items(len(exp) * k).reshape(len(exp), k)
    for i, e in enumerate(exp):
        out[i, :len(e[0])] = e[0]
    return out


def undecided_share(exp, rows):
    """the share of undecided rays among the rays with a non-empty W"""
    nonempty = np.array([len(r) > 0 for r in rows])
    undecided = np.array([not e[1] for e in exp])
    assert not (undecided & ~nonempty).any()
    return float(undecided.sum()) / max(int(nonempty.sum()), 1)
