"""A sequential pure-Python model of the instanced first-K definition (include/rt_abi.h, instanced first-K block): one ray, one
step at a time -- a bound, one stack for both levels, a sorted list of ITEMs.  tests/test_ray_first_instanced_ref_cpu.py holds it
to the numpy reference in four orders; tests/test_gpu_ray_first_instanced_edges.py derives the stack depths of the comb scenes
from its shipped order.  Not a test file; numpy and the reference modules only.

Order (an implementation matter the claims do not depend on):
  reverse=False  the kernel's: the slots of a run in ascending order, the surviving slot with the smallest front goes next (ties
                 to the lower slot), a displaced nearest and every other survivor are pushed as they are met, triangle A before
                 B -- on both levels; an instance is walked to the end before the next TLAS entry is popped;
  reverse=True   the opposite: the slots in descending order, the farthest goes next (ties to the higher slot), B before A.
recull: a popped entry (a TLAS instance entry included: its proxy's front) is dropped iff front > b.
limit: the stack's size; a push onto a full stack is dropped (None: unbounded)."""
import numpy as np

import instance_ref as ir
import ray_first_instanced_ref as rfi
import ray_first_ref as rf

F = np.float32


class Run:
    """what one model run leaves behind"""

    def __init__(self, k):
        self.row = rfi.pad_items(k)
        self.max_depth = 0        # the deepest the stack got (entries pending at once, the current one not counted)
        self.enter_depths = []    # the stack depth at which each instance was entered
        self.overflow = False
        self.box_tests = self.leaf_visits = 0


def model(tlas, records, trees, ray, k, *, reverse=False, recull=False, limit=None):
    """tlas = (leaves, nodes, root, count); records: RECORD array; trees[b] = (leaves, nodes, root, count).  -> Run"""
    run = Run(k)
    tl_leaves, tl_nodes, tl_root, tl_count = tlas
    world = np.array([ray], rf.RAY)
    if tl_count == 0 or len(records) == 0 or not rf.live(world)[0]:
        return run
    tmin, tmax = F(ray["tmin"]), F(ray["tmax"])
    bound = tmax
    lst = []                                                   # ITEM scalars, ascending by key
    stack = []                                                 # (is_leaf, index, slot count, front)

    def set_ray(rr):
        o, d = rr["origin"].astype(F), rr["dir"].astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            return o, d, (F(1.0) / d).astype(F)

    o, d, inv = set_ray(world)
    nodes, leaves = tl_nodes, tl_leaves
    inst, base = None, 0
    cur = (False, tl_root & rf.INDEX_MASK, tl_count, F(-np.inf))

    def offer(rec):
        nonlocal bound
        it = rfi.items(inst, np.array([rec], rf.HIT))[0]
        if len(lst) == k and not rfi.below(it, lst[-1]):
            return
        if any(rfi.same_key(np.array([e], rfi.ITEM), np.array([it], rfi.ITEM))[0] for e in lst):
            return
        pos = sum(1 for e in lst if rfi.below(e, it))
        lst.insert(pos, it)
        del lst[k:]
        if len(lst) == k:
            bound = tmax if np.isnan(lst[-1]["t"]) else F(lst[-1]["t"])

    def push(e):
        if limit is not None and len(stack) >= limit:
            run.overflow = True
            return
        stack.append(e)
        run.max_depth = max(run.max_depth, len(stack))

    def pop():
        """-> the next entry of the lane's current tree, or None when its part of the stack is used up"""
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
            o, d, inv = set_ray(world)                         # leaving: the world ray's original bits, the TLAS
            nodes, leaves, inst, base = tl_nodes, tl_leaves, None, 0
            cur = pop()
            continue
        is_leaf, index, cnt, _ = cur
        if is_leaf and inst is None:                           # a TLAS leaf: enter its instance, or go on in the TLAS
            iid = int(tl_leaves["primitive_id_0"][index])
            ok = iid < len(records) and records["flags"][iid] == 0 and int(records["blas"][iid]) < len(trees)
            if ok:
                b_leaves, b_nodes, b_root, b_count = trees[int(records["blas"][iid])]
                ok = 1 <= b_count <= 7
            if not ok:
                cur = pop()
                continue
            o, d, inv = set_ray(ir.object_rays(world, records["world_to_object"][iid]))
            nodes, leaves, inst, base = b_nodes, b_leaves, iid, len(stack)
            run.enter_depths.append(base)
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
                ok, t, bu, bv = rf.mt_f32(L[corners[0]], L[corners[1]], L[corners[2]], o, d, tmin, bound)
                if ok[0]:
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
