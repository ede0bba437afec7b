"""The numpy reference of the filtered ray queries (rt_intersect_rays_filtered, rt_ray_hits_count_filtered /
rt_ray_hits_collect_filtered, rt_ray_first_hits_filtered), restated from include/rt_abi.h (hit-filter block) with no code
shared with the kernels.  The contracts are the all-hit and first-K contracts on W_f, the KEPT records of the all-hit row W, so
the reference is the gated all-hit walk of tests/ray_first_ref.py carrying one more number per record:

walk_gated_det(nodes, leaves, root, count, rays): ray_first_ref.walk_gated, and with every record of W the float32 determinant
    `a` of Moller-Trumbore on the STORED corners of the triangle it came from.  -> (rows, gates, dets, box tests, leaf visits)
Filter: the host image of rt_hit_filter -- flags, ray_mask, prim_masks (uint32 array or None), per_ray (RAY_FILTER array or None).
keep(records, a, ray_index, filter): the header's acceptance rule for the records of ONE ray -> bool array.
filtered(rows, gates, dets, filter) -> (W_f rows, their gates): what the first-K reference (ray_first_ref.expected,
    envelope_violation, undecided_share) and the all-hit comparison (ray_hits_ref.canon) are then run on."""
import numpy as np

from ray_first_ref import CAP, HIT, INDEX_MASK, MISS, NONE, RAY, TRI, live, records, slab  # noqa: F401
from ray_hits_ref import EPS

F = np.float32
RAY_FILTER = np.dtype([("mask", "<u4"), ("skip_id", "<u4")])
CULL_BACK, CULL_FRONT = 1, 2
ALL = 0xFFFFFFFF


class Filter:
    def __init__(self, flags=0, ray_mask=ALL, prim_masks=None, per_ray=None):
        self.flags, self.ray_mask = int(flags), int(ray_mask)
        self.prim_masks = None if prim_masks is None else np.ascontiguousarray(prim_masks, np.uint32)
        self.per_ray = None if per_ray is None else np.ascontiguousarray(per_ray, RAY_FILTER)

    def sliced(self, sel):
        """the filter of the sub-batch rays[sel]: per_ray is indexed by the ray's index in its batch"""
        return Filter(self.flags, self.ray_mask, self.prim_masks, None if self.per_ray is None else self.per_ray[sel])


def mt_det_f32(c0, c1, c2, o, d, tmin, tmax):
    """Moller-Trumbore in float32 in the header's operation order -> (accepted, t, bu, bv, a) on the given corners; `a` is the
    determinant e1 . (dir x e2) the facing rule reads"""
    c0, c1, c2, o, d = (np.asarray(x, F) for x in (c0, c1, c2, o, d))
    with np.errstate(all="ignore"):
        e1, e2 = (c1 - c0).astype(F), (c2 - c0).astype(F)
        hx = d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1]
        hy = d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2]
        hz = d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]
        a = e1[:, 0] * hx + e1[:, 1] * hy + e1[:, 2] * hz
        ok = ~((a > -EPS) & (a < EPS))
        f = F(1.0) / a
        s = (o - c0).astype(F)
        u = f * (s[:, 0] * hx + s[:, 1] * hy + s[:, 2] * hz)
        ok &= ~((u < 0) | (u > 1))
        qx = s[:, 1] * e1[:, 2] - s[:, 2] * e1[:, 1]
        qy = s[:, 2] * e1[:, 0] - s[:, 0] * e1[:, 2]
        qz = s[:, 0] * e1[:, 1] - s[:, 1] * e1[:, 0]
        v = f * (d[:, 0] * qx + d[:, 1] * qy + d[:, 2] * qz)
        ok &= ~((v < 0) | ((u + v) > 1))
        t = f * (e2[:, 0] * qx + e2[:, 1] * qy + e2[:, 2] * qz)
        ok &= ~((t < tmin) | (t > tmax))
    return ok, t.astype(F), u.astype(F), v.astype(F), a.astype(F)


def walk_gated_det(nodes, leaves, root, count, rays):
    """-> (rows: one HIT array per ray, gates, dets: one float32 array per ray each (gates[i][j], dets[i][j] belong to
    rows[i][j]), box tests, leaf visits).  The window is the ray's original one: rows, gates and the counts are the all-hit
    query's."""
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
    got_ray, got_rec, got_gate, got_det = [], [], [], []
    while len(fr_ray):
        nxt, leaf = [], []
        for s in range(int(fr_cnt.max())):
            sel = fr_cnt > s
            r, nd = fr_ray[sel], nodes[fr_first[sel] + s]
            typ = nd["w28"] >> 29
            valid = typ != NONE
            box_tests += int(valid.sum())
            front, back = slab(nd["min"], nd["max"], o[r], inv[r])
            with np.errstate(invalid="ignore"):
                inn = valid & (back >= front) & (front <= tmax[r]) & (back >= tmin[r])
            gate = np.fmax(fr_gate[sel], front)
            child, ccount = (nd["w28"] & INDEX_MASK).astype(np.int64), (nd["w12"] >> 29).astype(np.int64)
            is_leaf = inn & (typ == TRI)
            is_box = inn & (typ != TRI) & (ccount > 0)
            leaf.append((r[is_leaf], child[is_leaf], gate[is_leaf]))
            nxt.append((r[is_box], child[is_box], ccount[is_box], gate[is_box]))
        lr, li, lg = (np.concatenate(x) for x in zip(*leaf))
        leaf_visits += len(lr)
        if len(lr):
            L = leaves[li]
            two = (L["v3"].view(np.uint32) != L["v2"].view(np.uint32)).any(1)          # B = (v2, v1, v3) iff v3 != v2 bit for bit
            for corners, pid, which, wanted in ((("v0", "v1", "v2"), "primitive_id_0", 0, None),
                                                (("v2", "v1", "v3"), "primitive_id_1", 1, two)):
                ok, t, bu, bv, a = mt_det_f32(L[corners[0]], L[corners[1]], L[corners[2]], o[lr], d[lr], tmin[lr], tmax[lr])
                if wanted is not None:
                    ok &= wanted
                got_ray.append(lr[ok]); got_gate.append(lg[ok]); got_det.append(a[ok])
                got_rec.append(records(t[ok], L[pid][ok], bu[ok], bv[ok], L["rotations"][ok, which]))
        fr_ray, fr_first, fr_cnt, fr_gate = (np.concatenate(x) for x in zip(*nxt))
    rows, gates, dets = [np.zeros(0, HIT)] * n, [np.zeros(0, F)] * n, [np.zeros(0, F)] * n
    if got_ray:
        gr, rec = np.concatenate(got_ray), np.concatenate(got_rec)
        gt, dt = np.concatenate(got_gate).astype(F), np.concatenate(got_det).astype(F)
        order = np.argsort(gr, kind="stable")
        gr, rec, gt, dt = gr[order], rec[order], gt[order], dt[order]
        cuts = np.searchsorted(gr, np.arange(n + 1))
        rows = [rec[cuts[i]:cuts[i + 1]] for i in range(n)]
        gates = [gt[cuts[i]:cuts[i + 1]] for i in range(n)]
        dets = [dt[cuts[i]:cuts[i + 1]] for i in range(n)]
    return rows, gates, dets, box_tests, leaf_visits


def keep(recs, a, ray_index, flt):
    """the acceptance rule for the records `recs` (HIT array) of ray `ray_index`, `a` their determinants -> bool array"""
    ids = recs["primitive_id"].astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = ~(bool(flt.flags & CULL_BACK) & (a < 0))                  # a NaN a is neither front nor back
        ok &= ~(bool(flt.flags & CULL_FRONT) & (a > 0))
    rm = flt.ray_mask
    if flt.per_ray is not None:
        rm, skip = int(flt.per_ray["mask"][ray_index]), int(flt.per_ray["skip_id"][ray_index])
        if skip != MISS:
            ok &= ids != skip
    pm = np.full(len(recs), ALL, np.int64)
    if flt.prim_masks is not None:
        inside = ids < len(flt.prim_masks)
        pm[inside] = flt.prim_masks[ids[inside]]
    return ok & ((pm & rm) != 0)


def filtered(rows, gates, dets, flt):
    """-> (W_f rows, their gates): the kept records of every ray's W"""
    out_rows, out_gates = [], []
    for i, (row, gate, det) in enumerate(zip(rows, gates, dets)):
        k = keep(row, det, i, flt)
        out_rows.append(row[k])
        out_gates.append(gate[k])
    return out_rows, out_gates


# ------------------------------------------------------------------ the filters and rays the CPU and GPU tests share
FILTERS = ("cull_back", "cull_front", "groups", "skip_nearest", "combined")
KS = (1, 3, 8, 32)
GROUPS = 3
MASK_SEED = 97


def nearest_ids(rows):
    """per ray: the primitive_id of the first record of W in (t, id) order, MISS for an empty row"""
    from ray_first_ref import key_order
    return np.array([row["primitive_id"][key_order(row)[0]] if len(row) else MISS for row in rows], np.uint32)


def group_masks(num_triangles):
    return (np.uint32(1) << (np.arange(num_triangles, dtype=np.uint32) % GROUPS)).astype(np.uint32)


def make_filter(name, rows, num_triangles):
    """the filter `name` of FILTERS for a batch whose unfiltered all-hit rows are `rows` (skip_nearest needs them)"""
    n = len(rows)
    per_ray = np.zeros(n, RAY_FILTER)
    per_ray["mask"], per_ray["skip_id"] = ALL, MISS
    if name == "cull_back":
        return Filter(CULL_BACK)
    if name == "cull_front":
        return Filter(CULL_FRONT)
    if name in ("groups", "combined"):
        per_ray["mask"] = np.random.default_rng(MASK_SEED).integers(1, 1 << GROUPS, n)      # 1 .. 7: never empty
    if name in ("skip_nearest", "combined"):
        per_ray["skip_id"] = nearest_ids(rows)
    if name == "groups":
        return Filter(0, 0, group_masks(num_triangles), per_ray)       # (ray_mask 0: per_ray must win)
    if name == "skip_nearest":
        return Filter(0, 0, None, per_ray)
    if name == "combined":
        return Filter(CULL_BACK, 0, group_masks(num_triangles), per_ray)
    raise KeyError(name)


def bounce_rays(rays, first, seed):
    """the self-hit batch: for every ray with a primary hit `first[i]` (a HIT record, MISS where none) a ray that starts AT the
    hit point o + t d (float32) in a random direction with tmin = 0 -- the rays an epsilon in tmin is usually spent on -- and
    its per-ray filter record (all-ones mask, skip_id = the primary primitive_id).  Rays without a primary hit are dropped.
    -> (RAY array, RAY_FILTER array)"""
    hit = first["primitive_id"] != MISS
    with np.errstate(invalid="ignore"):
        hit &= np.isfinite(first["t"])
    r, h = rays[hit], first[hit]
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(len(r), 3))
    out = np.zeros(len(r), RAY)
    with np.errstate(all="ignore"):
        out["origin"] = r["origin"].astype(F) + (h["t"].astype(F)[:, None] * r["dir"].astype(F)).astype(F)
    out["dir"] = d / np.linalg.norm(d, axis=1)[:, None]
    out["tmin"], out["tmax"] = 0.0, np.inf
    ok = np.isfinite(out["origin"]).all(1)
    per_ray = np.zeros(len(r), RAY_FILTER)
    per_ray["mask"], per_ray["skip_id"] = ALL, h["primitive_id"]
    return out[ok], per_ray[ok]
