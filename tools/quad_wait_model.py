#!/usr/bin/env python3
"""CPU model of the tracer's quad coherence: how many vector-memory requests do the four rays of a 2 x 2 pixel quad need for
their node pairs (three readings of how requests merge: quad_requests), stepping in lock-step or under the hold-at-pop rule of csrc/rt_traverse.hpp (quad_hold)?

The address path of a CU charges per lane request, and only the lanes of a quad that carry the same address share one
(profiles/r02_ta_microbench.txt).  The model walks each ray through an oracle-built tree (oracle/oracle_py.py, read at run
time) in the reference's TraceRay order, exactly as the kernel's Trav does -- slots in order, nearest Box child first (ties:
larger index), the others pushed in encounter order, a push onto a full stack dropped -- and counts, per round of a quad, the
lane requests of the lanes that step.

  lock-step     every unfinished ray steps once per round (leaf tests are taken inline: no parking)
  hold-at-pop   a ray that has just popped entry E from level s < 16 of its stack sits the round out while a quad-mate that is
                still traversing holds E at level s of its own stack with a deeper stack pointer

--wave adds the kernel's real schedule: 16 quads = one 8 x 8 tile per wave, lanes in Morton order, leaf parking by
kParkNum / kParkDen, two box steps per vote (the rule is evaluated before the first; "hold, 2nd too": before both).  It predicts the wave's box-phase and
leaf-phase iteration counts (counters 2 and 3 of rt_trace) and the requests per wave load instruction.

run_wave(pair=1|2) adds the two forms of a box step (RT_TRACE_PAIR_STEP, csrc/rt_traverse.hpp): a NARROW vote -- no lane that
counts sits on more than a pair or carries a near -- runs both of its steps as Ray.pair_step, which asserts what the form
relies on (no carried near; no node of more than two slots in the first step); any other vote runs Ray.box_step.  pair=1
counts every unfinished lane (the rule of RT_TRACE_PAIR_STEP = 1); pair=2 leaves the parked lanes out (the arm that was measured
beside it).  pair=3 is the EXACT vote (RT_TRACE_PAIR_STEP = 2, exact_cur): no unfinished lane carries a near and every unfinished
lane sits on a pair below index 2^27 - 1; both steps run as Ray.pair_step without a tail, and a lane whose cur is not exact
after the first step sits the second out.

--first entry|sp / --second none|entry|sp (run_wave(first=, second=)) choose the rule in front of each of a vote's two steps:
"entry" is quad_hold, "sp" is quad_hold_sp (RT_TRACE_HOLD_FIRST / RT_TRACE_HOLD_SECOND, csrc/rt_traverse.hpp) -- a freshly popped
lane sits out while an unfinished mate's stack is deeper than the popped level, no entry compared.  Given either, one line is
printed for that combination (profiles/hold_second_model.txt); without them the three lines of quad_wait_model.txt.

The arithmetic is float64 on the float32 inputs: a model of the schedule, not a second oracle.

  python3 tools/quad_wait_model.py --grid 708 --camera a --tree lbvh --samples 40
  python3 tools/quad_wait_model.py --grid 708 --camera a --tree lbvh --samples 6 --wave"""
import argparse
import importlib
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

INDEX_MASK = 0x1FFFFFFF
NO_NEAR = 0xFFFFFFFF
STACK_LDS, STACK_MAX = 16, 64            # kStackLds, kStackMax
PARK_NUM, PARK_DEN = 8, 1                # kParkNum, kParkDen
STEP, LEAF0, LEAF1, DONE = 0, 1, 2, 3
EXACT_INDICES = 0x07FFFFFF               # kExactIndices: a pair (count 2) whose index is below this is exact
CHILD_NONE, CHILD_BOX, CHILD_TRI = 0, 1, 2
INF = float("inf")


def exact_cur(cur):
    """rt_traverse.hpp exact_cur, on the packed word as the kernel does it (32-bit wrap-around)"""
    return ((cur - (2 << 29)) & 0xFFFFFFFF) < EXACT_INDICES


class Tree:
    """an oracle tree as plain Python lists (fast scalar access)"""
    def __init__(self, nodes, leaves, root, count):
        self.lo = nodes["min"].astype(np.float64).tolist()
        self.hi = nodes["max"].astype(np.float64).tolist()
        self.w12 = nodes["w12"].tolist()
        self.w28 = nodes["w28"].tolist()
        self.v = [leaves[k].astype(np.float64).tolist() for k in ("v0", "v1", "v2", "v3")]
        self.root, self.count = root, count


def load_tree(ora, tris, kind):
    if kind == "lbvh":
        b = ora.build_bvh(tris)
        return Tree(b["nodes"], b["leaves"], 0, 2)
    s = ora.build_sah(tris)
    return Tree(s["nodes"], s["leaves"], 0, 1)


def camera_ray(cam, w, h, x, y):
    """the primary ray of TraceRays through the centre of pixel (x, y): (origin, direction, tmin, tmax)"""
    c = cam[0] if getattr(cam, "shape", ()) else cam
    u, v, ww, pos = (np.asarray(c[k], np.float64) for k in ("u", "v", "w", "position"))
    nx, ny = 2 * ((x + 0.5) / w) - 1, 2 * ((y + 0.5) / h) - 1
    d = nx * u + ny * v + ww
    d = d / math.sqrt(float(d @ d))
    return pos.tolist(), d.tolist(), 0.00001, float(c["max_depth"])


def _inv(a):
    return 1.0 / a if a != 0.0 else math.copysign(INF, a)


class Ray:
    """One lane of the kernel: Trav (rt_traverse.hpp) plus its ray.  `visits` records the ray's own sequence of tests:
    ("b", pair) per box step, ("t", leaf) per leaf test; `pushes` every entry handed to push(), dropped ones included."""
    def __init__(self, tree, org, d, tmin, tmax, active=True):
        self.t = tree
        self.o, self.d, self.tmin, self.tmax = org, d, tmin, tmax
        self.i = [_inv(a) for a in d]
        self.stack = [0] * STACK_MAX
        self.sp = 0
        self.cur = (tree.root & INDEX_MASK) | (tree.count << 29)
        self.near_e, self.near_d = NO_NEAR, INF
        self.phase = STEP if active and tree.count > 0 else DONE
        self.popped = False                   # PH_STEP_POP: cur was popped from level sp
        self.leaf = 0
        self.f1 = self.k1 = 0.0
        self.e1 = self.t1 = 0
        self.box_tests = self.tri_tests = 0
        self.visits = []
        self.pushes = []
        self.hit = False

    # ---- Trav
    def push(self, e):
        self.pushes.append((len(self.visits), e))
        if self.sp < STACK_MAX:
            self.stack[self.sp] = e
        self.sp = min(self.sp + 1, STACK_MAX)

    def inner_hit(self, inside, e, front):
        closer = front < self.near_d or (front == self.near_d and (e & INDEX_MASK) > (self.near_e & INDEX_MASK))
        if inside and self.near_e != NO_NEAR:
            self.push(self.near_e if closer else e)
        if inside and closer:
            self.near_e, self.near_d = e, front

    def advance(self):
        cnt = self.cur >> 29
        if cnt > 2:
            self.cur = ((self.cur & INDEX_MASK) + 2) | ((cnt - 2) << 29)
            return
        if self.near_e != NO_NEAR and self.sp < STACK_MAX:
            self.cur = self.near_e
        elif self.sp == 0:
            self.phase = DONE
        else:
            self.sp -= 1
            self.cur = self.stack[self.sp]
            self.popped = True
        self.near_e, self.near_d = NO_NEAR, INF

    def slab(self, n):
        lo, hi, o, i = self.t.lo[n], self.t.hi[n], self.o, self.i
        front, back = -INF, INF
        for a in range(3):
            t1, t2 = (lo[a] - o[a]) * i[a], (hi[a] - o[a]) * i[a]
            if t1 != t1 or t2 != t2:          # fminf / fmaxf drop a NaN operand; both NaN: the axis says nothing
                t1 = t2 if t1 != t1 else t1
                t2 = t1 if t2 != t2 else t2
                if t1 != t1:
                    continue
            front, back = max(front, min(t1, t2)), min(back, max(t1, t2))
        return front, back

    def second_slot(self):
        valid = self.t1 != CHILD_NONE
        hit = valid and self.k1 >= self.f1 and self.f1 <= self.tmax and self.k1 >= self.tmin
        self.box_tests += 1 if valid else 0
        is_leaf = hit and self.t1 == CHILD_TRI
        self.inner_hit(hit and not is_leaf, self.e1, self.f1)
        if is_leaf:
            self.leaf, self.phase = self.e1, LEAF1

    def box_step(self):
        assert self.phase == STEP
        self.popped = False
        n = self.cur & INDEX_MASK
        two = (self.cur >> 29) > 1
        self.visits.append(("b", n))
        n1 = n + 1 if two else n
        f0, k0 = self.slab(n)
        self.f1, self.k1 = self.slab(n1)
        w12, w28 = self.t.w12, self.t.w28
        self.e1 = (w28[n1] & INDEX_MASK) | (w12[n1] & ~INDEX_MASK & 0xFFFFFFFF)
        self.t1 = (w28[n1] >> 29) if two else CHILD_NONE
        type0 = w28[n] >> 29
        e0 = (w28[n] & INDEX_MASK) | (w12[n] & ~INDEX_MASK & 0xFFFFFFFF)
        valid0 = type0 != CHILD_NONE
        hit0 = valid0 and k0 >= f0 and f0 <= self.tmax and k0 >= self.tmin
        self.box_tests += 1 if valid0 else 0
        leaf0 = hit0 and type0 == CHILD_TRI
        self.inner_hit(hit0 and not leaf0, e0, f0)
        if leaf0:
            self.leaf, self.phase = e0, LEAF0
        else:
            self.second_slot()
            if self.phase == STEP:
                self.advance()

    def pair_step(self, tail, exact=False):
        """pair_step_on: the box step of a pair entered without a carried near, decided from values of the step alone.
        Returns what the step wrote of near_e: None, "leaf1" (parked with the near kept for the leaf phase) or "tail" (the
        first pair of a node of more than two slots: near kept, cur on the node's next pair).  exact: a step of an exact
        vote, whose loads take cur << 5 as the pair's byte offset."""
        assert self.phase == STEP
        assert self.near_e == NO_NEAR and self.near_d == INF, "a pair-local step starts without a carried near"
        cnt = self.cur >> 29
        assert tail or cnt <= 2, "the first step of a narrow vote never sits on a node of more than two slots"
        assert not exact or (not tail and exact_cur(self.cur) and ((self.cur << 5) & 0xFFFFFFFF) == (self.cur & INDEX_MASK) * 32), \
            "a step of an exact vote sits on a pair whose byte offset is cur << 5 in 32 bits"
        self.popped = False
        n = self.cur & INDEX_MASK
        two = cnt > 1
        self.visits.append(("b", n))
        n1 = n + 1 if two else n
        f0, k0 = self.slab(n)
        f1, k1 = self.slab(n1)
        w12, w28 = self.t.w12, self.t.w28
        e0 = (w28[n] & INDEX_MASK) | (w12[n] & ~INDEX_MASK & 0xFFFFFFFF)
        e1 = (w28[n1] & INDEX_MASK) | (w12[n1] & ~INDEX_MASK & 0xFFFFFFFF)
        type0, type1 = w28[n] >> 29, (w28[n1] >> 29) if two else CHILD_NONE
        hit0 = type0 != CHILD_NONE and k0 >= f0 and f0 <= self.tmax and k0 >= self.tmin
        self.box_tests += 1 if type0 != CHILD_NONE else 0
        self.f1, self.k1, self.e1, self.t1 = f1, k1, e1, type1
        if hit0 and type0 == CHILD_TRI:
            self.leaf, self.phase = e0, LEAF0
            return None
        hit1 = type1 != CHILD_NONE and k1 >= f1 and f1 <= self.tmax and k1 >= self.tmin
        self.box_tests += 1 if type1 != CHILD_NONE else 0
        leaf1 = hit1 and type1 == CHILD_TRI
        box1 = hit1 and not leaf1
        closer = f1 < f0 or (f1 == f0 and (e1 & INDEX_MASK) > (e0 & INDEX_MASK))
        if hit0 and box1:
            self.push(e0 if closer else e1)
        second = box1 and (closer or not hit0)
        near, nd = (e1, f1) if second else ((e0, f0) if hit0 else (NO_NEAR, INF))
        if leaf1:
            self.near_e, self.near_d = near, nd
            self.leaf, self.phase = e1, LEAF1
            return "leaf1"
        if tail and cnt > 2:
            self.near_e, self.near_d = near, nd
            self.cur = ((self.cur & INDEX_MASK) + 2) | ((cnt - 2) << 29)
            return "tail"
        if near != NO_NEAR and self.sp < STACK_MAX:
            self.cur = near
        elif self.sp == 0:
            self.phase = DONE
        else:
            self.sp -= 1
            self.cur = self.stack[self.sp]
            self.popped = True
        return None

    def _tri(self, a, b, c):
        eps = 0.000000001
        e1 = [b[k] - a[k] for k in range(3)]
        e2 = [c[k] - a[k] for k in range(3)]
        d = self.d
        h = [d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]]
        det = e1[0] * h[0] + e1[1] * h[1] + e1[2] * h[2]
        if -eps < det < eps:
            return False
        f = 1.0 / det
        s = [self.o[k] - a[k] for k in range(3)]
        u = f * (s[0] * h[0] + s[1] * h[1] + s[2] * h[2])
        if u < 0.0 or u > 1.0:
            return False
        q = [s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]]
        v = f * (d[0] * q[0] + d[1] * q[1] + d[2] * q[2])
        if v < 0.0 or u + v > 1.0:
            return False
        t = f * (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2])
        if t < self.tmin or t > self.tmax:
            return False
        self.tmax = t
        return True

    def leaf_step(self):
        assert self.phase in (LEAF0, LEAF1)
        self.tri_tests += 1
        li = self.leaf & INDEX_MASK
        self.visits.append(("t", li))
        v0, v1, v2, v3 = (self.t.v[k][li] for k in range(4))
        self.hit |= self._tri(v0, v1, v2)
        if (self.leaf >> 29) > 0 and v3 != v2:
            self.hit |= self._tri(v2, v1, v3)
        was_first = self.phase == LEAF0
        self.phase = STEP
        if was_first:
            self.second_slot()
        if self.phase == STEP:
            self.advance()


def quad_requests(curs):
    """Lane requests of one quad for one load, `curs` = the pair addresses of its lanes that step, under three readings of
    the address path: (any) lanes that agree share a request whatever the others do; (on) the quad pays one request if all
    its switched-on lanes agree, else one per lane -- a switched-off lane does not spoil its mates' merge; (full) one request
    only if all four lanes are on and agree.  ta_microbench section 2 says which one the hardware is."""
    n, d = len(curs), len(set(curs))
    return (d, (1 if d == 1 else n) if n else 0, 1 if (d == 1 and n == 4) else n)


def holds(rays, k):
    """quad_hold for lane k of the quad `rays`"""
    r = rays[k]
    if not (r.phase == STEP and r.popped and r.sp < STACK_LDS):
        return False
    return any(m.phase != DONE and m.sp > r.sp and m.stack[r.sp] == r.cur for m in rays if m is not r)


def holds_sp(rays, k):
    """quad_hold_sp for lane k of the quad `rays`: the stack depths alone, no entry is compared"""
    r = rays[k]
    if not (r.phase == STEP and r.popped and r.sp < STACK_LDS):
        return False
    return any(m.phase != DONE and m.sp > r.sp for m in rays if m is not r)


HOLD_RULES = {"entry": holds, "sp": holds_sp}


def run_quad(rays, hold):
    """Rounds of one quad without parking.  Returns dict(rounds, lane_steps, requests, longest); raises if a round of an
    unfinished quad steps no lane."""
    rounds = lane_steps = 0
    requests = [0, 0, 0]
    while any(r.phase != DONE for r in rays):
        go = [r for k, r in enumerate(rays) if r.phase == STEP and not (hold and holds(rays, k))]
        if not go:
            raise AssertionError("a round of an unfinished quad steps no lane")
        for j, q in enumerate(quad_requests([r.cur & INDEX_MASK for r in go])):
            requests[j] += q
        lane_steps += len(go)
        rounds += 1
        for r in go:
            r.box_step()
            while r.phase in (LEAF0, LEAF1):
                r.leaf_step()
    return dict(rounds=rounds, lane_steps=lane_steps, req_any=requests[0], req_on=requests[1], req_full=requests[2],
                longest=max(sum(1 for v in r.visits if v[0] == "b") for r in rays))


def run_wave(rays, hold, second=False, pair=0, first="entry"):
    """The kernel's loop (trace_ray) over the 64 lanes of a tile, lanes 4q .. 4q+3 = quad q.  Returns dict(nbox, nleaf,
    box_instr, lane_steps, requests): nbox / nleaf are the wave's counters 2 / 3, box_instr the box steps that ran with at
    least one lane, req_* the lane requests (quad_requests) summed over those steps.  second: the second box step under a
    vote evaluates the rule again; the shipped kernel steps every lane in PH_STEP there.  (The kernel arm of it,
    RT_TRACE_QUAD_WAIT_SECOND = 1, was retired: TA busy -19 %, but -2.4 % in time where the shipped form is +5 %)
    pair: 0 every vote runs the general step; 1 / 2 a narrow vote (1, RT_TRACE_PAIR_STEP = 1: no unfinished lane; 2, the arm
    measured beside it: no lane in PH_STEP -- sits on more than a pair or carries a near) runs both steps in the pair-local form.  narrow / general count the
    votes of each form, tails / carried the pair-local steps that left a near behind for a wider node / across a leaf phase
    (of those, wide_carried on the first pair of a node of more than two slots).  pair = 3: the exact vote (RT_TRACE_PAIR_STEP = 2);
    exact counts its votes, sat_out the lanes in PH_STEP that sat out a second step because their new cur was not exact, by what
    it was: sat_wide (more than two slots), sat_lone (a lone slot), sat_far (a pair from index 2^27 - 1 up).  Raises if a pass of
    the loop neither steps a lane nor runs a leaf phase.
    first / second name the rule in front of each step of a vote (RT_TRACE_HOLD_FIRST / RT_TRACE_HOLD_SECOND): first "entry"
    (quad_hold: the mate holds the popped entry at that level) or "sp" (quad_hold_sp: the mate's stack is deeper, nothing is
    compared); second "none" (= False: every lane in PH_STEP steps), "entry" (= True, the retired arm) or "sp" (the
    RT_TRACE_HOLD_SECOND = 1 arm).  held2 counts the lanes in PH_STEP that the second rule kept out of a second step, empty2 the
    second steps that were left with no lane."""
    second = {False: "none", True: "entry"}.get(second, second)
    assert first in HOLD_RULES and second in ("none", "entry", "sp")
    quads = [rays[q:q + 4] for q in range(0, len(rays), 4)]
    nbox = nleaf = box_instr = lane_steps = 0
    requests = [0, 0, 0]
    forms = dict(narrow=0, general=0, tails=0, carried=0, wide_carried=0, exact=0, sat_out=0, sat_wide=0, sat_lone=0, sat_far=0,
                 held2=0, empty2=0)

    def going(rule=first):
        return [r for qd in quads for k, r in enumerate(qd) if r.phase == STEP and not (hold and HOLD_RULES[rule](qd, k))]

    def going2():
        """the lanes of a vote's second step, before the exact vote's own mask"""
        every = [r for r in rays if r.phase == STEP]
        if second == "none" or not hold:
            return every
        nxt = going(second)
        forms["held2"] += len(every) - len(nxt)
        return nxt

    def step(go, narrow=False, tail=False, exact=False):
        nonlocal box_instr, lane_steps
        if not go:
            return
        box_instr += 1
        lane_steps += len(go)
        ids = {id(r) for r in go}
        for qd in quads:
            for j, q in enumerate(quad_requests([r.cur & INDEX_MASK for r in qd if id(r) in ids])):
                requests[j] += q
        for r in go:
            if narrow:
                wide = (r.cur >> 29) > 2
                left = r.pair_step(tail, exact)
                forms["tails"] += left == "tail"
                forms["carried"] += left == "leaf1" and r.near_e != NO_NEAR
                forms["wide_carried"] += left == "leaf1" and r.near_e != NO_NEAR and wide
            else:
                r.box_step()

    while True:
        while True:
            go = going()
            parked = sum(1 for r in rays if r.phase in (LEAF0, LEAF1))
            if not go or len(go) * PARK_DEN < parked * PARK_NUM:
                break
            nbox += 2
            if pair == 3:
                if any(r.phase != DONE and (not exact_cur(r.cur) or r.near_e != NO_NEAR) for r in rays):
                    forms["general"] += 1
                    step(go)
                    nxt = going2()
                    forms["empty2"] += not nxt
                    step(nxt)
                else:
                    forms["exact"] += 1
                    step(go, True, False, True)        # (never empty: the vote is taken with a lane that steps)
                    nxt = going2()
                    for r in nxt:
                        if not exact_cur(r.cur):
                            cnt = r.cur >> 29
                            forms["sat_out"] += 1
                            forms["sat_wide" if cnt > 2 else "sat_lone" if cnt < 2 else "sat_far"] += 1
                    nxt = [r for r in nxt if exact_cur(r.cur)]
                    forms["empty2"] += not nxt
                    step(nxt, True, False, True)
                continue
            counts = [r for r in rays if (r.phase != DONE if pair == 1 else r.phase == STEP)]
            narrow = pair != 0 and not any((r.cur >> 29) > 2 or r.near_e != NO_NEAR for r in counts)
            forms["narrow" if narrow else "general"] += 1
            step(go, narrow, False)
            nxt = going2()
            forms["empty2"] += not nxt
            step(nxt, narrow, True)
        if not go and parked == 0:
            if any(r.phase != DONE for r in rays):
                raise AssertionError("the wave ends with an unfinished lane")
            break
        if parked == 0:
            raise AssertionError("a pass of the loop steps no lane and has no parked lane to free")
        nleaf += 1
        for r in rays:
            if r.phase in (LEAF0, LEAF1):
                r.leaf_step()
    return dict(nbox=nbox, nleaf=nleaf, box_instr=box_instr, lane_steps=lane_steps, req_any=requests[0], req_on=requests[1],
                req_full=requests[2], **forms)


def quad_rays(tree, cam, w, h, qx, qy):
    """the four rays of the 2 x 2 pixel quad (qx, qy) in lane order (x fastest); pixels outside the frame are finished lanes"""
    out = []
    for k in range(4):
        x, y = 2 * qx + (k & 1), 2 * qy + (k >> 1)
        inside = x < w and y < h
        out.append(Ray(tree, *camera_ray(cam, w, h, min(x, w - 1), min(y, h - 1)), active=inside))
    return out


def tile_rays(tree, cam, w, h, tx, ty):
    """the 64 rays of the 8 x 8 tile (tx, ty) in the kernel's Morton lane order"""
    out = []
    for lane in range(64):
        lx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4)
        ly = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4)
        x, y = tx * 8 + lx, ty * 8 + ly
        out.append(Ray(tree, *camera_ray(cam, w, h, min(x, w - 1), min(y, h - 1)), active=x < w and y < h))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grid", type=int, default=708, help="G of grid_mesh")
    ap.add_argument("--camera", choices=["a", "b"], default="a")
    ap.add_argument("--tree", choices=["lbvh", "sah"], default="lbvh")
    ap.add_argument("--samples", type=int, default=40, help="random quads (or tiles with --wave)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--wave", action="store_true", help="the kernel's schedule over whole 8 x 8 tiles")
    ap.add_argument("--pair", type=int, choices=[0, 1, 2, 3], default=0, help="with --wave: narrow votes run the pair-local step (1: every unfinished lane counts, 2: parked lanes left out); 3: the exact vote of RT_TRACE_PAIR_STEP = 2")
    ap.add_argument("--first", choices=["entry", "sp"], default=None, help="with --wave: the rule before a vote's first step (default: the three lines of lock-step, entry / none and entry / entry)")
    ap.add_argument("--second", choices=["none", "entry", "sp"], default=None, help="with --wave: the rule before a vote's second step; giving --first or --second prints that one combination")
    a = ap.parse_args()
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    from oracle import oracle_py as ora
    ora.lib()
    tree = load_tree(ora, scenes.grid_mesh(a.grid, 1), a.tree)
    cam = scenes.camera_a(a.grid) if a.camera == "a" else scenes.camera_b(a.grid)
    rng = random.Random(a.seed)
    w, h = a.width, a.height
    print(f"grid_mesh({a.grid}) {a.tree} camera {a.camera} {w}x{h}, {a.samples} random {'tiles' if a.wave else 'quads'}, seed {a.seed}")
    arms = (("lock-step", False, False), ("hold-at-pop", True, False)) + ((("hold, 2nd too", True, True),) if a.wave else ())
    first = a.first or "entry"
    if a.wave and (a.first or a.second):
        arms = ((f"{first} / {a.second or 'none'}", True, a.second or "none"),)
    for name, hold, second in arms:
        rng.seed(a.seed)
        tot = {}
        seqs = []
        for _ in range(a.samples):
            if a.wave:
                rays = tile_rays(tree, cam, w, h, rng.randrange((w + 7) // 8), rng.randrange((h + 7) // 8))
                res = run_wave(rays, hold, second, a.pair, first)
            else:
                rays = quad_rays(tree, cam, w, h, rng.randrange((w + 1) // 2), rng.randrange((h + 1) // 2))
                res = run_quad(rays, hold)
            for k, v in res.items():
                tot[k] = max(tot.get(k, 0), v) if k == "longest" else tot.get(k, 0) + v
        n = a.samples
        req = " / ".join(f"{tot[k] / max(tot['lane_steps'], 1):.3f}" for k in ("req_any", "req_on", "req_full"))
        if a.wave:
            line = (f"{name:13s} counters 2/3 per wave: box-phase {tot['nbox'] / n:.1f}  leaf-phase {tot['nleaf'] / n:.1f}   "
                    f"box instructions {tot['box_instr'] / n:.1f}  lanes per instruction {tot['lane_steps'] / max(tot['box_instr'], 1):.1f}  "
                    f"requests per lane step any/on/full {req}  "
                    f"requests per box instruction any/on/full " + " / ".join(f"{tot[k] / max(tot['box_instr'], 1):.1f}" for k in ("req_any", "req_on", "req_full")))
            if a.pair == 3:
                line += f"  exact votes {100.0 * tot['exact'] / max(tot['exact'] + tot['general'], 1):.1f} %  lanes that sat out a second step {tot['sat_out']}"
                if a.first or a.second:
                    line += f"  held before a second step {tot['held2']}  second steps left empty {tot['empty2']}"
            elif a.pair:
                line += f"  narrow votes {100.0 * tot['narrow'] / max(tot['narrow'] + tot['general'], 1):.1f} %"
        else:
            line = (f"{name:12s} requests per lane step any/on/full {req}   rounds per quad {tot['rounds'] / n:.1f}   "
                    f"lane steps per quad {tot['lane_steps'] / n:.1f}   longest ray {tot['longest']}")
        print(line)


if __name__ == "__main__":
    main()
