"""The numpy references of the filtered instanced all-hit and first-K ray queries (rt_ray_hits_count_instanced_filtered,
rt_ray_hits_collect_instanced_filtered, rt_ray_first_hits_instanced_filtered), restated from include/rt_abi.h (instanced
set-filter block) with no code shared with the kernels.  Everything is put together from existing restatements:

walk_gated(): the filtered all-hit row W of every ray with the gate of each item.  ray_first_instanced_ref.entered_gated's
    TLAS frontier gives the (ray, instance) pairs the unfiltered query enters (ray_hits_instanced_ref.entered's pairs, with the
    TLAS gate); rule 1 drops the pairs whose masks share no bit; for each remaining instance instance_ref.object_rays on the
    record's bytes and ray_filter_ref.walk_gated_det on the BLAS give records, gates and determinants, and
    instance_filter_ref.effective + ray_filter_ref.keep apply rule 2.  A masked pair costs its proxy's slab test in the TLAS
    and nothing else.
walk(): the rows and the two counts of walk_gated: the filtered all-hit query's answer.
The filtered first-K head is ray_first_instanced_ref's definition (dedup_sorted / expected / envelope_violation / padded) on
    that W.
model(): a filtered variant of the sequential ray_first_instanced_model.model -- one ray, a bound, one stack, a sorted list --
    with rule 1 asked at the TLAS leaf before the record is read and rule 2 at the leaf test's acceptance point, taking
    reverse / recull / limit as the model it restates does.
Brute: a float64 brute force over the KEPT world triangles: ray_hits_instanced_ref.brute_f64 (acceptance, stability at
    MARGIN = 1e-4) on instance_ref.world_triangles, with instance_filter_ref.candidates / kept_masks deciding what is kept in
    world space (facing from the float64 world corners, undecided within FACE_MARGIN = 1e-3 of edge-on).

Measured on the CPU (tests/test_instance_set_filter_ref_cpu.py: oracle-built trees, the 12 instances of
tests/ray_hits_instanced_scene.py, about 2,000 rays, numpy against numpy): the walk and the brute force agree on every stable
pair of every arm, none missing and none extra; the unstable share of the in-window pairs of admitted instances is 0.0161 % for
keep-all, the four cull arms and the mask arm (8.76 million in-window pairs, 5.10 million under the masks; the facing margin
adds nothing visible in the fourth digit) and 0.0356 % on the bounce batch of the skip arm (2.67 million pairs); the cap is the
project's 1 %.  The CPU test asserts the agreement and the cap and prints the shares."""
import numpy as np

import instance_filter_ref as ifr
import instance_ref as ir
import ray_filter_ref as rx
import ray_first_instanced_ref as rfi
import ray_hits_instanced_ref as rhi
import ray_hits_ref as rh
from ray_hits_instanced_ref import ITEM, RECORD, items  # noqa: F401  (the tests take them from here)

F = np.float32
MISS = 0xFFFFFFFF
MARGIN = rhi.MARGIN                  # 1e-4
FACE_MARGIN = ifr.FACE_MARGIN        # 1e-3
CAP = 0.01                           # the unstable share the all-hit tests allow


def keep_all(n=None, num_instances=None):
    """the two keep-all filters of contract (a): null arrays, or arrays of all-ones masks with zero flags and no skip"""
    if n is None:
        return ifr.InstanceFilter(0, ifr.ALL)
    per_ray = np.zeros(n, ifr.INSTANCE_RAY_FILTER)
    per_ray["mask"], per_ray["skip_instance"], per_ray["skip_id"] = ifr.ALL, MISS, MISS
    return ifr.InstanceFilter(0, 0, ifr.instance_filters(num_instances), per_ray)


def rule1(flt, ray, inst, n):
    """the instance rule on (ray, instance) pairs -> bool array"""
    if len(inst) == 0:
        return np.zeros(0, bool)
    im = np.array([flt.instance(k)[0] for k in range(int(inst.max()) + 1)], np.uint32)
    return (im[inst] & flt.ray_masks(n)[ray]) != 0


def walk_gated(tlas_nodes, tlas_leaves, root, count, records, blas_trees, rays, flt, first_k=True):
    """blas_trees[b] = (leaves, nodes, root, count) of table entry b.  -> (rows: one ITEM array per ray, gates: one float32
    array per ray, box tests of both levels, BLAS leaf visits).  first_k: a scene without records counts nothing (the first-K
    rule); the all-hit query still counts its TLAS slots"""
    n = len(rays)
    counts = [t[3] for t in blas_trees]
    ray, inst, tgate, box_tests = rfi.entered_gated(tlas_nodes, tlas_leaves, root, count, records, counts, rays)
    if not first_k and len(records) == 0:
        _, _, box_tests = rhi.entered(tlas_nodes, tlas_leaves, root, count, records, counts, rays)
    ok = rule1(flt, ray, inst, n)
    ray, inst, tgate = ray[ok], inst[ok], tgate[ok]
    leaf_visits = 0
    got_ray, got_item, got_gate = [], [], []
    for k in np.unique(inst):
        which = inst == k
        sel = ray[which]
        W = records["world_to_object"][k]
        obj = ir.object_rays(rays[sel], W)
        assert rh.live(obj).all(), "an object ray has a NaN: outside what this reference restates"
        leaves, nodes, broot, bcount = blas_trees[int(records["blas"][k])]
        rows, gates, dets, bt, lv = rx.walk_gated_det(nodes, leaves, broot, bcount, obj)
        box_tests += bt
        leaf_visits += lv
        eff, _ = ifr.effective(flt, int(k), W, n)
        for j, i in enumerate(sel):
            if len(rows[j]) == 0:
                continue
            kept = rx.keep(rows[j], dets[j], int(i), eff)
            if not kept.any():
                continue
            got_ray.append(np.full(int(kept.sum()), i, np.int64))
            got_item.append(items(k, rows[j][kept]))
            got_gate.append(np.fmax(tgate[which][j], gates[j][kept]).astype(F))
    out, out_g = [np.zeros(0, ITEM)] * n, [np.zeros(0, F)] * n
    if got_ray:
        gr, it, gt = np.concatenate(got_ray), np.concatenate(got_item), np.concatenate(got_gate)
        order = np.argsort(gr, kind="stable")
        gr, it, gt = gr[order], it[order], gt[order]
        cuts = np.searchsorted(gr, np.arange(n + 1))
        out = [it[cuts[i]:cuts[i + 1]] for i in range(n)]
        out_g = [gt[cuts[i]:cuts[i + 1]] for i in range(n)]
    return out, out_g, box_tests, leaf_visits


def walk(tlas_nodes, tlas_leaves, root, count, records, blas_trees, rays, flt):
    """the filtered all-hit rows -> (rows, box tests, leaf visits), the shape of ray_hits_instanced_ref.walk"""
    rows, _, box_tests, leaf_visits = walk_gated(tlas_nodes, tlas_leaves, root, count, records, blas_trees, rays, flt, first_k=False)
    return rows, box_tests, leaf_visits


# ------------------------------------------------------------------ the sequential model, filtered
class Run:
    def __init__(self, k):
        self.row = rfi.pad_items(k)
        self.max_depth = 0
        self.enter_depths = []
        self.overflow = False
        self.box_tests = self.leaf_visits = 0
        self.bounds = []          # every value the bound took after the original tmax, in order


def model(tlas, records, trees, ray, ray_index, flt, k, *, reverse=False, recull=False, limit=None):
    """ray_first_instanced_model.model's definition with the two rules.  ray_index: the ray's index in the batch `flt` was made
    for (per_ray).  -> Run"""
    import ray_first_ref as rf
    run = Run(k)
    tl_leaves, tl_nodes, tl_root, tl_count = tlas
    world = np.array([ray], rf.RAY)
    if tl_count == 0 or len(records) == 0 or not rf.live(world)[0]:
        return run
    rm = flt.ray_mask if flt.per_ray is None else int(flt.per_ray["mask"][ray_index])
    skip_instance = MISS if flt.per_ray is None else int(flt.per_ray["skip_instance"][ray_index])
    skip_id = MISS if flt.per_ray is None else int(flt.per_ray["skip_id"][ray_index])
    tmin, tmax = F(ray["tmin"]), F(ray["tmax"])
    bound = tmax
    lst, stack = [], []

    def set_ray(rr):
        o, d = rr["origin"].astype(F), rr["dir"].astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            return o, d, (F(1.0) / d).astype(F)

    o, d, inv = set_ray(world)
    nodes, leaves = tl_nodes, tl_leaves
    inst, base = None, 0
    cull, skip = 0, MISS
    cur = (False, tl_root & rf.INDEX_MASK, tl_count, F(-np.inf))

    def offer(rec):
        nonlocal bound
        it = rfi.items(inst, np.array([rec], rf.HIT))[0]
        if len(lst) == k and not rfi.below(it, lst[-1]):
            return
        if any(rfi.same_key(np.array([e], ITEM), np.array([it], ITEM))[0] for e in lst):
            return
        pos = sum(1 for e in lst if rfi.below(e, it))
        lst.insert(pos, it)
        del lst[k:]
        if len(lst) == k:
            bound = tmax if np.isnan(lst[-1]["t"]) else F(lst[-1]["t"])
            run.bounds.append(bound)

    def push(e):
        if limit is not None and len(stack) >= limit:
            run.overflow = True
            return
        stack.append(e)
        run.max_depth = max(run.max_depth, len(stack))

    def pop():
        while len(stack) > base:
            e = stack.pop()
            if recull and e[3] > bound:
                continue
            return e
        return None

    while True:
        if cur is None:
            if inst is None:
                break
            o, d, inv = set_ray(world)
            nodes, leaves, inst, base = tl_nodes, tl_leaves, None, 0
            cur = pop()
            continue
        is_leaf, index, cnt, _ = cur
        if is_leaf and inst is None:
            iid = int(tl_leaves["primitive_id_0"][index])
            ok = iid < len(records)
            iflags = 0
            if ok:                                             # rule 1, before the record is read
                im, iflags = flt.instance(iid)
                ok = (im & rm) != 0
            ok = ok and records["flags"][iid] == 0 and int(records["blas"][iid]) < len(trees)
            if ok:
                b_leaves, b_nodes, b_root, b_count = trees[int(records["blas"][iid])]
                ok = 1 <= b_count <= 7
            if not ok:
                cur = pop()
                continue
            W = records["world_to_object"][iid]
            o, d, inv = set_ray(ir.object_rays(world, W))
            nodes, leaves, inst, base = b_nodes, b_leaves, iid, len(stack)
            run.enter_depths.append(base)
            cull = flt.flags & 3
            if cull:
                flip = bool(ifr.det_f32(W) < 0) != bool(iflags & ifr.FLIP_FACING)
                if flip:
                    cull = (2 if cull & 1 else 0) | (1 if cull & 2 else 0)
                if iflags & ifr.CULL_DISABLE:
                    cull = 0
            skip = skip_id if iid == skip_instance else MISS
            cur = (False, b_root & rf.INDEX_MASK, b_count, F(-np.inf))
            continue
        if is_leaf:
            run.leaf_visits += 1
            L = leaves[index:index + 1]
            tests = [(("v0", "v1", "v2"), "primitive_id_0", 0, True),
                     (("v2", "v1", "v3"), "primitive_id_1", 1, bool((L["v3"].view(np.uint32) != L["v2"].view(np.uint32)).any()))]
            for corners, pid, which, wanted in (tests[::-1] if reverse else tests):
                if not wanted:
                    continue
                ok, t, bu, bv, a = rx.mt_det_f32(L[corners[0]], L[corners[1]], L[corners[2]], o, d, tmin, bound)
                if not ok[0]:
                    continue
                if (cull & 1 and a[0] < 0) or (cull & 2 and a[0] > 0):          # rule 2 (a NaN a: both comparisons false)
                    continue
                if skip != MISS and int(L[pid][0]) == skip:
                    continue
                offer(rf.records(t, L[pid], bu, bv, L["rotations"][:, which])[0])
            cur = pop()
            continue
        near = None
        slots = range(index, index + cnt)
        for s in (reversed(slots) if reverse else slots):
            nd = nodes[s:s + 1]
            typ = int(nd["w28"][0] >> 29)
            if typ == rf.NONE:
                continue
            run.box_tests += 1
            front, back = rf.slab(nd["min"], nd["max"], o, inv)
            front, back = front[0], back[0]
            with np.errstate(invalid="ignore"):
                if not (back >= front and front <= bound and back >= tmin):
                    continue
            child, ccount = int(nd["w28"][0] & rf.INDEX_MASK), int(nd["w12"][0] >> 29)
            if typ != rf.TRI and ccount == 0:
                continue
            e = (typ == rf.TRI, child, ccount, front)
            if near is None:
                near = e
            elif (front > near[3]) if reverse else (front < near[3]):
                push(near)
                near = e
            else:
                push(e)
        cur = near if near is not None else pop()
    run.row[:len(lst)] = lst
    return run


# ------------------------------------------------------------------ float64 brute force over the kept world triangles
class Brute:
    """the filter-independent part, computed once per (scene, ray set): ray_hits_instanced_ref.brute_f64's dense decisions and
    instance_filter_ref.candidates' sparse list with the world-space facing"""

    def __init__(self, world_tris, inst_of, prim_of, rays, margin=MARGIN):
        self.n, self.m = len(rays), len(inst_of)
        self.inst_of, self.prim_of = np.asarray(inst_of, np.int64), np.asarray(prim_of, np.int64)
        self.b = rhi.brute_f64(world_tris, rays, margin)
        self.cand = ifr.candidates(rays, world_tris)

    def under(self, flt):
        """-> dict of bool [rays, placed triangles]: expected (accepted in float64 AND kept); stable (certain either way: the
        instance masked, the candidate turned down by the mask or the skip pair whatever its geometry, or the acceptance at
        least MARGIN from its limits with the facing not within FACE_MARGIN of edge-on); in_window (t inside the window and the
        instance let in by rule 1: the pairs the unstable share is taken over)"""
        n, m, b, cand = self.n, self.m, self.b, self.cand
        kept, maybe = ifr.kept_masks(cand, self.inst_of, self.prim_of, flt, n)
        C, K, M = (np.zeros((n, m), bool) for _ in range(3))
        C[cand["ray"], cand["tri"]] = True
        K[cand["ray"], cand["tri"]] = kept
        M[cand["ray"], cand["tri"]] = maybe
        let_in = rule1(flt, np.repeat(np.arange(n), m), np.tile(self.inst_of, n), n).reshape(n, m)
        # (a pair outside the candidates is more than BARY_MARGIN outside its triangle: not accepted, whatever the filter)
        stable = ~let_in | (C & ~M) | (b["stable"] & ((K == M) | ~b["accepted"]))
        return dict(expected=b["accepted"] & K, stable=stable, in_window=b["in_window"] & let_in)
