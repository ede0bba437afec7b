"""Trees with runs of one to seven slots, and the inputs tests/test_wide_trees_ref_cpu.py, tests/test_gpu_wide_trees.py and
tests/test_gpu_wide_trees_sets.py share.

include/rt_abi.h lets every query walk "any tree rt_trace takes": runs of 1..7 contiguous slots, any of which may be a NONE
slot.  No builder emits a run of more than two, so the trees here are re-packed from built ones on the host:

  repack(nodes, root, count, ..)   edge_scenes.collapse_wide's pulling-up with a target width per Box child, taken in turn
      from WIDTHS -- a cycle that holds every width 1..7 and a pair after every second wide node, so that plain pairs and wide
      nodes alternate along every path; every second wide run that holds both kinds begins with the pair (Box, leaf).  Width 1 makes a LONE run: the Box child's run is one Box slot (the child's own box
      again) over the run the next width gives.  Some runs with room take a NONE slot -- type 0, min = +1e30, max = -1e30, and
      zero index and count bits -- first, in the middle or last, in turn; so does the root run.  Every other
      slot keeps its box, its leaf record index and its leaf count: the source tree's leaf records serve the wide tree, and
      the wide tree never has more slots than the source had (a pulled-up child frees the slot its parent held; NONE slots and
      lone runs are only made while freed slots are left), so it fits the nodes_out of the BuildInput it came from.
  hist(nodes, root, count)         {run length: runs of that length reached from the root}
  none_places(nodes, root, count)  {"first" / "middle" / "last": runs with a NONE slot there}
  leaf_records(nodes, root, count) the leaf record indices reached, sorted, with multiplicity
  single_run(nodes, root, count)   a tree of up to 7 leaves as ONE root run of leaf slots and no Box child at all

Scenes: scenes.grid_mesh(12, 3) (288 triangles), scenes.soup(300, 7), `layers` (three copies of the grid offset along its
normal: rays cross two or more triangles) and the 3-, 5- and 7-triangle soups.  Rays: ray_hits_ref.ray_sets(per_kind=64) plus
small_scenes.aimed_rays -- at most 384, less three, so that a batch ends inside a wave.  Everything is a pure function of its
arguments: fixed seeds, no shared state."""
import collections

import numpy as np

import ray_hits_ref as rh
import small_scenes as ss
import stack_scenes as sc

F = np.float32
MASK = 0x1FFFFFFF
NONE, BOX, TRI = 0, 1, 2
NODE = sc.NODE
WIDTHS = (2, 3, 1, 4, 5, 7, 6, 2)
NONE_EVERY, LONE_EVERY, ROOT_WIDTH = 3, 1, 7
NONE_MIN, NONE_MAX = F(1e30), F(-1e30)
NONE_CHILD = 0           # a NONE slot's index bits: in bounds, so that a kernel that followed it would answer wrongly, not read wildly
SCENES = ("grid", "soup")
TINY = (3, 5, 7)
KINDS = ("bottom_up", "hybrid", "sah", "sah_pairs", "sah_splits")      # test_gpu_ray_queries._gpu_tree's names
RAY_SEED = {"grid": 1201, "soup": 1213, "layers": 1217, "tiny3": 1223, "tiny5": 1229, "tiny7": 1231}
AIM_NAME = {"grid": "n5", "soup": "twins", "layers": "n4", "tiny3": "n3", "tiny5": "n2", "tiny7": "n1"}   # small_scenes' seeds

Pose = collections.namedtuple("Pose", "triangles_out nodes_out")


# ------------------------------------------------------------------ the re-packer
def _typ(s):
    return int(s["w28"]) >> 29


def _child(s):
    return int(s["w28"]) & MASK, int(s["w12"]) >> 29


def _none_slot(dtype):
    rec = np.zeros((), dtype)
    rec["min"], rec["max"] = NONE_MIN, NONE_MAX
    rec["w28"] = NONE_CHILD
    return rec


def repack(nodes, root, count, widths=WIDTHS, none_every=NONE_EVERY, lone_every=LONE_EVERY, root_width=ROOT_WIDTH):
    """-> (nodes, root, count).  widths: the cycle of target widths, one per Box child in the order the children are emitted
    (depth first); none_every: every none_every-th run with room takes a NONE slot (0: none, the root run's included);
    lone_every: every lone_every-th width of 1 makes a lone run (0: none; a width of 1 that makes none counts as 2);
    root_width: the width the root run is widened to, less one where it takes a NONE slot."""
    dtype = nodes.dtype
    out = []
    state = dict(box=0, runs=0, nones=0, lones=0, spare=0, wide=0)

    def slots_of(index, cnt):
        return [nodes[index + i] for i in range(cnt)]

    def widen(sl, width):
        while True:                          # pull children up, level by level, while they fit
            res, budget = [], width - len(sl)
            for s in sl:
                if _typ(s) == BOX and 0 < _child(s)[1] and _child(s)[1] - 1 <= budget:
                    res.extend(slots_of(*_child(s)))
                    budget -= _child(s)[1] - 1
                    state["spare"] += 1          # the slot that held this child is gone
                else:
                    res.append(s)
            if len(res) == len(sl):
                return res
            sl = res

    def box_leaf_first(sl):
        """every second run of more than two slots that has both kinds begins with the pair (Box, leaf): a near carried across
        a leaf phase to the run's next pair"""
        if len(sl) <= 2:
            return sl
        b = next((s for s in sl if _typ(s) == BOX), None)
        l = next((s for s in sl if _typ(s) == TRI), None)
        if b is None or l is None:
            return sl
        state["wide"] += 1
        if state["wide"] % 2:
            return sl
        return [b, l] + [s for s in sl if s is not b and s is not l]

    def with_none(sl):
        """the run, with a NONE slot where it has room, it is this run's turn and a freed slot is left"""
        if not none_every or len(sl) >= 7:
            return sl
        state["runs"] += 1
        if state["runs"] % none_every or state["spare"] < 1:
            return sl
        state["spare"] -= 1
        place = (0, (len(sl) + 1) // 2, len(sl))[state["nones"] % 3]
        if len(sl) == 1 and place == 1:
            place = 0
        state["nones"] += 1
        return sl[:place] + [None] + sl[place:]

    def next_width():
        w = widths[state["box"] % len(widths)]
        state["box"] += 1
        if w == 1:
            state["lones"] += 1
            if not lone_every or state["lones"] % lone_every or state["spare"] < 1:
                return 2
        return w

    def run_under(s):
        """the run a Box slot's child becomes: (slots, lone) -- lone: one Box slot over the run made at the next width"""
        child, ccount = _child(s)
        src = slots_of(child, ccount)
        w = next_width()
        if w == 1:
            state["spare"] -= 1
            return [s], True
        return box_leaf_first(widen(src, w)), False

    def emit(sl, parent):
        base = len(out)
        out.extend([None] * len(sl))
        for i, s in enumerate(sl):
            if s is None:
                rec = _none_slot(dtype)
                rec["w12"] = parent & MASK
                out[base + i] = rec
                continue
            rec = np.zeros((), dtype)
            rec["min"], rec["max"] = s["min"], s["max"]
            if _typ(s) == BOX and _child(s)[1] > 0:
                kids, lone = run_under(s)
                if lone:
                    cbase = emit_lone(s, base + i)
                    n = 1
                else:
                    kids = with_none(kids)
                    cbase, n = emit(kids, base + i), len(kids)
                rec["w28"] = (BOX << 29) | cbase
                rec["w12"] = (n << 29) | (parent & MASK)
            else:
                rec["w28"] = s["w28"]
                rec["w12"] = (_child(s)[1] << 29) | (parent & MASK)
            out[base + i] = rec
        return base

    def emit_lone(s, parent):
        """a one-slot run: a Box slot with s's box, over s's child run at the width that is next in turn (never 1 again)"""
        base = len(out)
        out.append(None)
        rec = np.zeros((), dtype)
        rec["min"], rec["max"] = s["min"], s["max"]
        w = next_width()
        kids = with_none(box_leaf_first(widen(slots_of(*_child(s)), max(w, 2))))
        cbase = emit(kids, base)
        rec["w28"] = (BOX << 29) | cbase
        rec["w12"] = (len(kids) << 29) | (parent & MASK)
        out[base] = rec
        return base

    # the slots the pulling-up has freed so far pay for the NONE slots and lone runs (state["spare"]).  emit() recurses once per
    # level of the wide tree (twice through a lone run): a few dozen frames on the trees of some hundred leaves used here
    if count == 0:
        return nodes[:0].copy(), 0, 0
    source = sum(hist(nodes, root, count, lengths=True))
    top = widen(slots_of(root, count), root_width - 1 if none_every else root_width)
    if none_every and len(top) < 7:            # (on credit where the root run pulled nothing up: the runs below repay it)
        state["spare"] -= 1
        place = len(top) // 2
        top = top[:place] + [None] + top[place:]
    emit(top, 0)
    arr = np.array(out, dtype=dtype)
    assert len(arr) <= source, (len(arr), source)
    return arr, 0, len(top)


def single_run(nodes, root, count):
    """a tree of at most 7 leaf slots as one root run of leaf slots: no Box child, no NONE slot"""
    arr, r, c = repack(nodes, root, count, widths=(7,), none_every=0, lone_every=0, root_width=7)
    assert c == len(arr) and ((arr["w28"] >> 29) == TRI).all(), "more than seven leaf slots"
    return arr, r, c


# ------------------------------------------------------------------ what a tree looks like
def runs(nodes, root, count):
    """the runs reached from the root, top-down: [(first slot, length)]"""
    todo, i = [(int(root), int(count))], 0
    while i < len(todo):
        f, k = todo[i]
        for s in range(f, f + k):
            if int(nodes["w28"][s]) >> 29 == BOX and int(nodes["w12"][s]) >> 29 > 0:
                todo.append((int(nodes["w28"][s]) & MASK, int(nodes["w12"][s]) >> 29))
        i += 1
    return todo if count else []


def hist(nodes, root, count, lengths=False):
    """{run length: runs of that length reached from the root}, ascending (lengths: the plain list of lengths)"""
    ls = [k for _, k in runs(nodes, root, count)]
    return ls if lengths else dict(sorted(collections.Counter(ls).items()))


def none_places(nodes, root, count):
    """{"first", "middle", "last": runs with a NONE slot at that place}, {"root": NONE slots of the root run}"""
    out = collections.Counter()
    for n, (f, k) in enumerate(runs(nodes, root, count)):
        for s in range(f, f + k):
            if int(nodes["w28"][s]) >> 29 == NONE:
                out["first" if s == f else "last" if s == f + k - 1 else "middle"] += 1
                out["root"] += n == 0
    return dict(out)


def leaf_records(nodes, root, count):
    """the leaf slots reached, as sorted (record index, leaf count) rows with multiplicity"""
    rows = [(int(nodes["w28"][s]) & MASK, int(nodes["w12"][s]) >> 29) for f, k in runs(nodes, root, count)
            for s in range(f, f + k) if int(nodes["w28"][s]) >> 29 == TRI]
    return np.array(sorted(rows), np.int64).reshape(-1, 2)


def reached_slots(nodes, root, count):
    return np.array([s for f, k in runs(nodes, root, count) for s in range(f, f + k)], np.int64)


def leaf_then_continue(leaves, nodes, root, count, hits):
    """how many closest-hit records name a primitive whose leaf slot -- every one of them, where a split tree holds it in
    several -- is slot 0 of a pair that is not the last pair of its run: after that leaf phase the lane tests slot 1 with the
    new tmax and carries the nearest child on to the node's next pair.  From the walker's records and the nodes alone."""
    where = collections.defaultdict(list)
    for f, k in runs(nodes, root, count):
        for s in range(f, f + k):
            if int(nodes["w28"][s]) >> 29 == TRI:
                j, rec = s - f, leaves[int(nodes["w28"][s]) & MASK]
                ids = [int(rec["primitive_id_0"])] + ([int(rec["primitive_id_1"])] if int(rec["primitive_id_1"]) else [])
                for p in ids:
                    where[p].append(j % 2 == 0 and j + 2 < k)
    return sum(1 for p in hits["primitive_id"] if int(p) in where and all(where[int(p)]))


# ------------------------------------------------------------------ scenes and rays
def tris(name, scenes):
    if name == "grid":
        return scenes.grid_mesh(12, 3)
    if name == "soup":
        return scenes.soup(300, 7)
    if name == "layers":
        g = scenes.grid_mesh(12, 3).reshape(-1, 3, 3)
        out = []
        for k in range(3):
            t = g.copy()
            t[:, :, 1] += F(0.75 * k)          # the grid's normal is +y
            out.append(t)
        return np.ascontiguousarray(np.concatenate(out).reshape(-1, 9), F)
    if name.startswith("tiny"):
        return scenes.soup(int(name[4:]), 40 + int(name[4:]), size=0.5)
    raise KeyError(name)


def rays(name, t):
    """ray_sets(per_kind=64) and 125 aimed rays: 381 rays, so that the batch ends inside the sixth wave"""
    return np.concatenate([rh.ray_sets(t, RAY_SEED[name], per_kind=64), ss.aimed_rays(AIM_NAME[name], t, n=125)])


def moved(t, seed=3):
    """pose 1 / the refitted pose: every vertex displaced by up to 0.4 of the mean length of the triangles' first edges, by a
    smooth field of its position (shared vertices stay shared, so paired leaves stay pairs)"""
    v = np.asarray(t, F).reshape(-1, 3).astype(np.float64)
    ext = float(np.ptp(v, axis=0).max())
    T = v.reshape(-1, 3, 3)
    amp = 0.4 * float(np.linalg.norm(T[:, 1] - T[:, 0], axis=1).mean())
    ph = np.random.default_rng(seed).uniform(0, 6.28, (3, 3))
    d = np.stack([np.sin(v @ (np.array(w) * 5.0 / ext) + p[0]) for w, p in zip(((1, .3, .2), (.2, 1, .4), (.5, .1, 1)), ph)], 1)
    return np.ascontiguousarray((v + amp * d).astype(F).reshape(-1, 9))


def at_time(t0, t1, tau):
    """the triangles a ray of time tau sees between two poses: fl(fl(w0 * a) + fl(tau * b)), w0 = 1 - tau, as the motion query"""
    tau = F(tau)
    w0 = F(1) - tau
    return ((w0 * np.asarray(t0, F)).astype(F) + (tau * np.asarray(t1, F)).astype(F)).astype(F)


def ora_tree(ora, t, kind):
    """the oracle's tree of a kind of KINDS (bit-equal to the device builder's): (leaves, nodes, root, count)"""
    if kind == "bottom_up":
        o = ora.build_bvh(t)
        return o["leaves"], o["nodes"], 0, 2
    if kind == "hybrid":
        o = ora.build_hybrid(t)
        return o["leaves"], o["nodes"], o["root"], 2
    o = ora.build_sah(t, pairs="pairs" in kind, splits="splits" in kind)
    return o["leaves"], o["nodes"], 0, 1


class Tree:
    """a wide tree on the host, and on the device once `rt` is given: what every query's wrapper and walker takes"""

    def __init__(self, leaves, nodes, root, count, rt=None):
        self.leaves, self.nodes, self.root, self.count = leaves, np.ascontiguousarray(nodes), int(root), int(count)
        self.pose = Pose(rt.to_device(np.ascontiguousarray(leaves)), rt.to_device(self.nodes)) if rt is not None else None

    @property
    def host(self):
        return self.leaves, self.nodes, self.root, self.count

    @property
    def g(self):
        """(inp-like, root, count): test_gpu_ray_queries._query's tree"""
        return self.pose, self.root, self.count


# ------------------------------------------------------------------ spheres, capsules and sphere casts over the same scenes
N_RAYS = 381


def cast_cap():
    """the unstable-share cap of a sphere cast over a scene that has no name in sphere_cast_ref.CAP: the least of its caps"""
    import sphere_cast_ref as scr
    return min(scr.CAP.values())


def capsule_cap():
    """likewise for capsules: the least of capsule_ref.CAP (what tests/test_gpu_capsules.py allows a scene without a name)"""
    import capsule_ref as cr
    return min(cr.CAP.values())


def sphere_scene(name, scenes):
    """(spheres float32 [n, 4], rays): a sphere at every triangle's centroid, a quarter of its first edge as radius (as
    stack_scenes.fractal_spheres "full"); sphere 5 has a negative radius.  Rays: sphere_ref.make_rays"""
    import sphere_ref as sr
    spheres = sc.fractal_spheres(tris(name, scenes), "full")
    spheres[5, 3] = -1.0
    return spheres, sr.make_rays(spheres, RAY_SEED[name] + 1, N_RAYS)


def capsule_scene(name, scenes):
    """(capsules float32 [n, 8], rays): a capsule along every triangle's first edge, a sixth of its length as radius; capsule
    5 has a negative radius.  Rays: capsule_ref.make_rays"""
    import capsule_ref as cr
    t = tris(name, scenes).reshape(-1, 3, 3).astype(np.float64)
    caps = cr.pack(t[:, 0], np.linalg.norm(t[:, 1] - t[:, 0], axis=1) / 6.0, t[:, 1])
    caps[5, 3] = -1.0
    return caps, cr.make_rays(caps, RAY_SEED[name] + 2, N_RAYS)


def cast_rays(name, t):
    """(rays, radii): sphere_cast_ref.make_rays -- every eighth radius is 0"""
    import sphere_cast_ref as scr
    return scr.make_rays(t, RAY_SEED[name] + 3, N_RAYS)
