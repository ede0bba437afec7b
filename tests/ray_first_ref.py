"""The numpy reference of the first-K ray query (rt_ray_first_hits), restated from include/rt_abi.h with no code shared with
the kernel.  The contract is stated on the all-hit row W of a ray and on the GATE of each of its records, so the reference is
the all-hit tree walk of tests/ray_hits_ref.py carrying one more number:

walk_gated(nodes, leaves, root, count, rays): `walk` with the running maximum of the slab `front` carried down the frontier:
    every record of W comes with its gate g(w), the largest front over the slots on the path from the root run to its leaf
    slot, the leaf slot included.  -> (rows, gates, box_tests, leaf_visits)
expected(rows, gates, k, tmax): per ray (E, decided, T1): Ws = W without duplicates by (t, id) (a duplicate keeps the smallest
    gate: the record is found through any of its paths), sorted by (t, id); E its first min(k, |Ws|) records; T1 the t of its
    (k+1)-th record, or the original tmax; decided = every w in E has g(w) <= T1.  On a decided ray the kernel's row is E.
envelope_violation / envelope_ok(row, W, gates, k, tmax): claims 1 and 3, which hold on EVERY ray.
Order of (t, id): t as floats (-0 equals +0), a NaN t above every number and equal to any other NaN, then the id."""
import numpy as np

from ray_hits_ref import HIT, RAY, SEEDS, live, mt_f32, ray_sets  # noqa: F401  (the tests take them from here)

F = np.float32
INDEX_MASK = 0x1FFFFFFF
NONE, BOX, TRI = 0, 1, 2
MISS = 0xFFFFFFFF
MAX_K = 32
CAP = 0.02               # at most this share of the live rays with a non-empty W may be undecided, per (scene, tree, k)


def miss_records(n):
    out = np.zeros(n, HIT)
    out["t"], out["primitive_id"] = np.inf, MISS
    return out


def slab(lo, hi, o, inv):
    """front / back of boxes [lo, hi] for rays (o, inv), float32 [n, 3]: fminf / fmaxf drop a NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        t1 = ((lo - o).astype(F) * inv).astype(F)
        t2 = ((hi - o).astype(F) * inv).astype(F)
    near, far = np.fmin(t1, t2), np.fmax(t1, t2)
    return (np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2]), np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2]))


def records(t, prim, bu, bv, rot):
    """HIT records with (u, v) mapped back to the caller's corners: rot 1 -> (bv, w0), 2 -> (w0, bu), else (bu, bv)"""
    with np.errstate(all="ignore"):
        w0 = (F(1) - bu).astype(F) - bv
    out = np.zeros(len(t), HIT)
    out["t"], out["primitive_id"] = t, prim
    out["u"] = np.where(rot == 1, bv, np.where(rot == 2, w0, bu))
    out["v"] = np.where(rot == 1, w0, np.where(rot == 2, bu, bv))
    return out


def walk_gated(nodes, leaves, root, count, rays):
    """-> (rows: one HIT array per ray, gates: one float32 array per ray (gates[i][j] belongs to rows[i][j]), box tests, leaf
    visits).  The window is the ray's original one, so rows, box tests and leaf visits are the all-hit query's."""
    n = len(rays)
    o, d = rays["origin"].astype(F), rays["dir"].astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1.0) / d).astype(F)
    tmin, tmax = rays["tmin"].astype(F), rays["tmax"].astype(F)
    alive = np.nonzero(live(rays))[0] if count > 0 else np.zeros(0, np.int64)
    fr_ray = alive.astype(np.int64)
    fr_first = np.full(len(alive), root & INDEX_MASK, np.int64)
    fr_cnt = np.full(len(alive), count, np.int64)
    fr_gate = np.full(len(alive), -np.inf, F)
    box_tests = leaf_visits = 0
    got_ray, got_rec, got_gate = [], [], []
    while len(fr_ray):
        nr, nf, nc, ng, lr, li, lg = [], [], [], [], [], [], []
        for s in range(int(fr_cnt.max())):
            sel = fr_cnt > s
            r, slot = fr_ray[sel], fr_first[sel] + s
            nd = nodes[slot]
            typ = nd["w28"] >> 29
            valid = typ != NONE
            box_tests += int(valid.sum())
            front, back = slab(nd["min"], nd["max"], o[r], inv[r])
            with np.errstate(invalid="ignore"):
                inn = valid & (back >= front) & (front <= tmax[r]) & (back >= tmin[r])
            gate = np.fmax(fr_gate[sel], front)
            child = (nd["w28"] & INDEX_MASK).astype(np.int64)
            ccount = (nd["w12"] >> 29).astype(np.int64)
            is_leaf = inn & (typ == TRI)
            is_box = inn & (typ != TRI) & (ccount > 0)
            lr.append(r[is_leaf]); li.append(child[is_leaf]); lg.append(gate[is_leaf])
            nr.append(r[is_box]); nf.append(child[is_box]); nc.append(ccount[is_box]); ng.append(gate[is_box])
        lr, li, lg = np.concatenate(lr), np.concatenate(li), np.concatenate(lg)
        leaf_visits += len(lr)
        if len(lr):
            L = leaves[li]
            rot = L["rotations"]
            ok, t, bu, bv = mt_f32(L["v0"], L["v1"], L["v2"], o[lr], d[lr], tmin[lr], tmax[lr])
            got_ray.append(lr[ok]); got_gate.append(lg[ok])
            got_rec.append(records(t[ok], L["primitive_id_0"][ok], bu[ok], bv[ok], rot[ok, 0]))
            two = (L["v3"].view(np.uint32) != L["v2"].view(np.uint32)).any(1)          # B = (v2, v1, v3) iff v3 != v2 bit for bit
            ok, t, bu, bv = mt_f32(L["v2"], L["v1"], L["v3"], o[lr], d[lr], tmin[lr], tmax[lr])
            ok &= two
            got_ray.append(lr[ok]); got_gate.append(lg[ok])
            got_rec.append(records(t[ok], L["primitive_id_1"][ok], bu[ok], bv[ok], rot[ok, 1]))
        fr_ray, fr_first, fr_cnt, fr_gate = np.concatenate(nr), np.concatenate(nf), np.concatenate(nc), np.concatenate(ng)
    rows, gates = [np.zeros(0, HIT)] * n, [np.zeros(0, F)] * n
    if got_ray:
        gr, rec, gt = np.concatenate(got_ray), np.concatenate(got_rec), np.concatenate(got_gate).astype(F)
        order = np.argsort(gr, kind="stable")
        gr, rec, gt = gr[order], rec[order], gt[order]
        cuts = np.searchsorted(gr, np.arange(n + 1))
        rows = [rec[cuts[i]:cuts[i + 1]] for i in range(n)]
        gates = [gt[cuts[i]:cuts[i + 1]] for i in range(n)]
    return rows, gates, box_tests, leaf_visits


def key_order(rec):
    """indices that sort HIT records by (t, id): NaN t last, -0 with +0"""
    t = rec["t"]
    nan = np.isnan(t)
    return np.lexsort((rec["primitive_id"], np.where(nan, F(np.inf), t + F(0)), nan))


def same_key(a, b):
    """(t, id) of record arrays a and b equal, element by element (NaN equals NaN)"""
    with np.errstate(invalid="ignore"):
        same_t = (a["t"] == b["t"]) | (np.isnan(a["t"]) & np.isnan(b["t"]))
    return same_t & (a["primitive_id"] == b["primitive_id"])


def below(a, b):
    """(t, id) of record a lexicographically below record b (two scalars of HIT)"""
    ta, tb = a["t"], b["t"]
    na, nb = np.isnan(ta), np.isnan(tb)
    if na or nb:
        return (not na and nb) or (na and nb and a["primitive_id"] < b["primitive_id"])
    return ta < tb or (ta == tb and a["primitive_id"] < b["primitive_id"])


def dedup_sorted(row, gate):
    """Ws and its gates: sorted by (t, id), one record per (t, id), its gate the smallest of the duplicates'"""
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
    """-> per ray: (E: HIT array of min(k, |Ws|) records, decided: bool, T1: float32).  dedup: dedup_all(rows, gates), when the
    caller asks for several k"""
    out = []
    for (ws, g), tm in zip(dedup if dedup is not None else dedup_all(rows, gates), tmax):
        E = ws[:k]
        t1 = F(ws["t"][k]) if len(ws) > k else F(tm)
        with np.errstate(invalid="ignore"):
            decided = bool((g[:k] <= t1).all())               # (a NaN T1 decides nothing but an empty E)
        out.append((E, decided, t1))
    return out


def below_all(a, b):
    """`below`, element by element, for record arrays a and b (or one record against an array)"""
    ta, tb = a["t"], b["t"]
    na, nb = np.isnan(ta), np.isnan(tb)
    with np.errstate(invalid="ignore"):
        same_t = (ta == tb) | (na & nb)
        return (ta < tb) | (~na & nb) | (same_t & (a["primitive_id"] < b["primitive_id"]))


def envelope_violation(row, W, gates, k, tmax):
    """claims 1 and 3 for one output row of k HIT records against the ray's all-hit row W with its gates.  -> None, or what is
    wrong"""
    assert len(row) == k
    is_live = row["primitive_id"] != MISS
    m = int(is_live.sum())
    if is_live[m:].any():
        return "a miss record before a live one"
    if row[m:].tobytes() != miss_records(k - m).tobytes():
        return "the padding is not {+inf, MISS, 0, 0}"
    got = np.ascontiguousarray(row[:m])
    # 1: every live record is a record of W, bit for bit; strictly ascending in (t, id)
    gw = got.view(np.uint32).reshape(m, 4)
    ww = np.ascontiguousarray(W).view(np.uint32).reshape(len(W), 4)
    member = (gw[:, None, :] == ww[None, :, :]).all(2).any(1)
    if not member.all():
        j = int(np.argmin(member))
        return f"record {j} {got[j]} is not in the all-hit row"
    if m > 1 and not below_all(got[:-1], got[1:]).all():
        return f"the records are not strictly ascending in (t, id): {got}"
    # 3: what a full row may lack lies behind a box front beyond the final bound; a row that never filled lacks nothing
    ws, g = dedup_sorted(W, gates)
    if m < k:
        if len(ws) != m or not same_key(ws, got).all():
            return f"a row of {m} < k records is not the whole all-hit row ({len(ws)} distinct records)"
        return None
    last = got[m - 1]
    T = F(tmax) if np.isnan(last["t"]) else last["t"]
    with np.errstate(invalid="ignore"):
        owed = below_all(ws, last) & (g <= T)
    with np.errstate(invalid="ignore"):
        same_t = (ws["t"][:, None] == got["t"][None, :]) | (np.isnan(ws["t"])[:, None] & np.isnan(got["t"])[None, :])
    listed = (same_t & (ws["primitive_id"][:, None] == got["primitive_id"][None, :])).any(1)
    if (owed & ~listed).any():
        j = int(np.argmax(owed & ~listed))
        return f"{ws[j]} (gate {g[j]} <= final bound {T}) is below the last record {last} and not in the row"
    return None


def padded(exp, k):
    """the rows the kernel writes where they equal E: [n, k] HIT records, E then miss records"""
    out = miss_records(len(exp) * k).reshape(len(exp), k)
    for i, e in enumerate(exp):
        out[i, :len(e[0])] = e[0]
    return out


def envelope_ok(row, W, gates, k, tmax):
    return envelope_violation(row, W, gates, k, tmax) is None


def undecided_share(exp, rows):
    """the share of undecided rays among the rays with a non-empty W (a dead ray's W is empty)"""
    nonempty = np.array([len(r) > 0 for r in rows])
    undecided = np.array([not e[1] for e in exp])
    assert not (undecided & ~nonempty).any()
    return float(undecided.sum()) / max(int(nonempty.sum()), 1)
