"""Two numpy references for the instanced all-hit ray queries (rt_ray_hits_count_instanced / rt_ray_hits_collect_instanced),
restated from include/rt_abi.h with no code shared with the kernel.

(a) walk(tlas_nodes, tlas_leaves, root, count, records, blas_trees, rays): the row of every ray as the header defines it, in
    three steps, each an existing restatement on the DEVICE's own bytes:
      1. entered(): a breadth-first frontier over the TLAS with ray_hits_ref._slab on the world ray (the window is fixed, so
         the frontier visits exactly the slots any other order visits); a triangle slot that passes names instance
         primitive_id_0 of its leaf record, and the instance is entered iff id < len(records), flags == 0, blas <
         len(blas_trees) and the tree's count is in 1..7;
      2. instance_ref.object_rays with the record's own world_to_object bits gives the object rays of the entered pairs;
      3. ray_hits_ref.walk on the BLAS's bytes gives the records, tagged with the instance.
    There is no 64-entry limit.  Returns per-ray ITEM arrays and the two test counts (non-NONE slots examined on both levels,
    BLAS leaf records visited).
(b) brute_f64(world_tris, rays, margin): float64 Moller-Trumbore of every (ray, placed triangle) pair over
    instance_ref.world_triangles, with ray_hits_ref.brute_f64's stability notion -- every acceptance quantity at least `margin`
    away from its limit.

MARGIN = ray_hits_ref.MARGIN (1e-4), the all-hit tests' own.  Here the triangle test runs on the float32 OBJECT ray (o' = W o +
w3, d' = W d, each a rounded three-term sum with a rounded world_to_object) against object-space corners, while the float64
reference places the corners in world space, so the same pair is decided from inputs that differ by a few float32 roundings
on top of the rounding inside Moller-Trumbore that 1e-4 already absorbs.  Whether that needs a wider margin was asked on the
CPU, numpy against numpy, on the scene of tests/test_ray_hits_instanced_ref_cpu.py (12 instances, 2,024 rays, 8.8 million
in-window pairs): at 1e-4 the walk and the brute force agree on every stable pair, none missing and none extra, so the margin
stays 1e-4 and no headroom is added.  0.016 % of the in-window pairs are left out as unstable there (the all-hit tests report
0.03 % on the untransformed sets; the cap is 1 %).  The CPU test asserts the agreement and the share."""
import numpy as np

import instance_ref as ir
import ray_hits_ref as rh

F = np.float32
MARGIN = rh.MARGIN
RECORD = np.dtype([("world_to_object", "<f4", (3, 4)), ("blas", "<u4"), ("flags", "<u4"), ("spare", "<u4", 2)])   # rt_instance_record
ITEM = np.dtype([("instance", "<u4"), ("t", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])   # 20 bytes


def items(instance, hits):
    """ITEM records from an instance id (scalar or array) and HIT records"""
    out = np.zeros(len(hits), ITEM)
    out["instance"] = instance
    for f in ("t", "primitive_id", "u", "v"):
        out[f] = hits[f]
    return out


def entered(tlas_nodes, tlas_leaves, root, count, records, blas_counts, rays):
    """-> (ray index, instance id) arrays of the entered pairs, in no particular order, and the TLAS's box tests"""
    o, d = rays["origin"].astype(F), rays["dir"].astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1.0) / d).astype(F)
    tmin, tmax = rays["tmin"].astype(F), rays["tmax"].astype(F)
    alive = np.nonzero(rh.live(rays))[0] if count > 0 else np.zeros(0, np.int64)
    fr_ray = alive.astype(np.int64)
    fr_first = np.full(len(alive), root & rh.INDEX_MASK, np.int64)
    fr_cnt = np.full(len(alive), count, np.int64)
    box_tests = 0
    got_ray, got_leaf = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    while len(fr_ray):
        nr, nf, nc = [], [], []
        for k in range(int(fr_cnt.max())):
            sel = fr_cnt > k
            r, slot = fr_ray[sel], fr_first[sel] + k
            nd = tlas_nodes[slot]
            typ = nd["w28"] >> 29
            valid = typ != rh.NONE
            box_tests += int(valid.sum())
            front, back = rh._slab(nd["min"], nd["max"], o[r], inv[r])
            with np.errstate(invalid="ignore"):
                inn = valid & (back >= front) & (front <= tmax[r]) & (back >= tmin[r])
            child = (nd["w28"] & rh.INDEX_MASK).astype(np.int64)
            ccount = (nd["w12"] >> 29).astype(np.int64)
            is_leaf = inn & (typ == rh.TRI)
            is_box = inn & (typ != rh.TRI) & (ccount > 0)
            got_ray.append(r[is_leaf]); got_leaf.append(child[is_leaf])
            nr.append(r[is_box]); nf.append(child[is_box]); nc.append(ccount[is_box])
        fr_ray, fr_first, fr_cnt = np.concatenate(nr), np.concatenate(nf), np.concatenate(nc)
    ray, leaf = np.concatenate(got_ray), np.concatenate(got_leaf)
    inst = tlas_leaves["primitive_id_0"][leaf].astype(np.int64)
    ok = inst < len(records)
    safe = np.where(ok, inst, 0)
    if len(records):
        blas = records["blas"][safe].astype(np.int64)
        ok &= (records["flags"][safe] == 0) & (blas < len(blas_counts))
        cnt = np.asarray(list(blas_counts) + [0], np.int64)[np.where(blas < len(blas_counts), blas, len(blas_counts))]
        ok &= (cnt >= 1) & (cnt <= 7)
    return ray[ok], inst[ok], box_tests


def walk(tlas_nodes, tlas_leaves, root, count, records, blas_trees, rays):
    """blas_trees[b] = (leaves, nodes, root, count) of table entry b, host arrays of the device's bytes.
    -> (rows: list of ITEM arrays, one per ray, in no particular order; box_tests; leaf_visits)"""
    n = len(rays)
    ray, inst, box_tests = entered(tlas_nodes, tlas_leaves, root, count, records, [t[3] for t in blas_trees], rays)
    leaf_visits = 0
    got_ray, got_item = [], []
    for k in np.unique(inst):
        sel = ray[inst == k]
        obj = ir.object_rays(rays[sel], records["world_to_object"][k])
        # (the device does not ask the liveness rule again inside an instance; the walk below does.  Finite rays and a finite
        # world_to_object give finite object rays, which is all this reference is used on)
        assert rh.live(obj).all(), "an object ray has a NaN: outside what this reference restates"
        leaves, nodes, broot, bcount = blas_trees[int(records["blas"][k])]
        rows, bt, lv = rh.walk(nodes, leaves, broot, bcount, obj)
        box_tests += bt
        leaf_visits += lv
        got_ray.append(np.repeat(sel, [len(x) for x in rows]))
        got_item.append(items(k, np.concatenate(rows) if rows else np.zeros(0, rh.HIT)))
    out = [np.zeros(0, ITEM)] * n
    if got_ray:
        gr, it = np.concatenate(got_ray), np.concatenate(got_item)
        order = np.argsort(gr, kind="stable")
        gr, it = gr[order], it[order]
        cuts = np.searchsorted(gr, np.arange(n + 1))
        out = [it[cuts[i]:cuts[i + 1]] for i in range(n)]
    return out, box_tests, leaf_visits


def canon(rows):
    """a row as a sorted array of 20-byte items: equal arrays <=> equal multisets of (instance, record), bit for bit"""
    return [np.sort(np.ascontiguousarray(r, ITEM).view(np.dtype((np.void, 20))).reshape(-1)) for r in rows]


def assert_rows_equal(rows, ref_rows, what):
    assert len(rows) == len(ref_rows)
    for k, (a, b) in enumerate(zip(canon(rows), canon(ref_rows))):
        assert a.shape == b.shape and (a == b).all(), f"{what}: ray {k}: {len(a)} items, the reference has {len(b)}"


def is_subset(row, ref_row):
    """multiset inclusion of ITEM rows"""
    a, b = canon([row])[0].tolist(), canon([ref_row])[0].tolist()
    for x in a:
        if x not in b:
            return False
        b.remove(x)
    return True


def offsets(rows):
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)


def brute_f64(world_tris, rays, margin=MARGIN, chunk=128):
    """ray_hits_ref.brute_f64 over placed triangles (float64 [m, 9]) at a stability margin of the caller's choosing.
    -> dict of [rays, triangles] arrays: accepted (the float64 decision), stable, in_window (t inside [tmin, tmax])"""
    T = np.asarray(world_tris, np.float64).reshape(-1, 3, 3)
    m, n = len(rays), T.shape[0]
    out = {k: np.zeros((m, n), bool) for k in ("accepted", "stable", "in_window")}
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    le = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    alive = rh.live(rays)
    for s in range(0, m, chunk):
        r = rays[s:s + chunk]
        o, d = r["origin"].astype(np.float64)[:, None, :], r["dir"].astype(np.float64)[:, None, :]
        lo, hi = r["tmin"].astype(np.float64)[:, None], r["tmax"].astype(np.float64)[:, None]
        with np.errstate(all="ignore"):
            h = np.cross(d, e2[None])
            a = (e1[None] * h).sum(2)
            f = 1.0 / a
            sv = o - T[None, :, 0]
            u = f * (sv * h).sum(2)
            q = np.cross(sv, e1[None])
            v = f * (d * q).sum(2)
            t = f * (e2[None] * q).sum(2)
            scale = np.maximum(1.0, np.abs(t))
            marg = np.stack([u, 1 - u, v, 1 - u - v, (t - lo) / scale, (hi - t) / scale])   # >= 0: the condition holds
            marg = np.where(np.isnan(marg), np.inf, marg)             # inf - inf on an open window: no limit there
            grazing = np.abs(a) < margin * le[None] * np.linalg.norm(d, axis=2)
            acc = (np.abs(a) >= float(rh.EPS)) & (marg >= 0).all(0)
            stab = (np.abs(marg) >= margin).all(0) & ~grazing & np.isfinite(t)
            inw = np.isfinite(t) & (t >= lo) & (t <= hi)
        ok = alive[s:s + chunk, None]
        out["accepted"][s:s + chunk] = acc & ok
        out["stable"][s:s + chunk] = stab | ~ok                       # a dead ray's empty row is certain
        out["in_window"][s:s + chunk] = inw & ok
    return out


def got_matrix(rows, inst_of, prim_of, num_rays):
    """bool [rays, placed triangles]: pair (i, j) is in row i; also whether any pair occurs twice"""
    where = {(int(a), int(b)): j for j, (a, b) in enumerate(zip(inst_of, prim_of))}
    got = np.zeros((num_rays, len(inst_of)), bool)
    twice = False
    for i, row in enumerate(rows):
        for it in row:
            j = where[int(it["instance"]), int(it["primitive_id"])]
            twice |= bool(got[i, j])
            got[i, j] = True
    return got, twice
