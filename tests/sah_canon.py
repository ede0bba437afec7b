"""Feeding the reference's SharedTaskBuild (oracle/_ref/libref_sah.so) from a built tree, and comparing two binned-SAH
trees in canonical form.  Shared by tests/test_ref_sah_cpu.py (the oracle's trees) and tests/test_gpu_ref_sah.py (the
GPU's): both hand in a Node array, nothing else of the builder under test.

FEEDING.  The front end (pairing, splits, the 4 x 4 x 4 cell assignment) is not under test, so the inputs of each launch
are read back from the tree being checked: the items of cell b are the Tri slots reachable from its sub-root (box,
leaf record, count), fed in ascending leaf-record order; the cell's c_aabb / p_aabb are the float32 min / max of the
items' (min + max) * 0.5f and of their boxes.  The top-of-tree launch takes the cells as items (BuildWrapper.cu:246-250),
the hybrid launch the sub-roots and c_aabb of the reference's own ExtractDepth (BuildWrapper.cu:350-360).

COMPARING.  Slot numbers come from atomic arrival in the reference and from BIAS + 2 * mid in ours, so a tree is walked
from its root into (box, item keys beneath, left, right).  Left and right are ORDERED: child_index holds the bins
<= plane, child_index + 1 the rest, in both.  The two members of a 2-item leaf group compare as a set (their order is
partition arrival order).  Boxes must be equal as float32 values; bit differences (-0 / +0: our unions run on the
ordered-int encoding, the reference's small-task path on fminf from FLT_MAX) are collected, not failed.
MEDIAN REGIONS.  A task with more than 2 items whose centroid box has sa(...) <= 0 is split at count >> 1 by buffer
order, which legitimately differs (per_instance_PartitionIds reverses the right side, ours is stable).  Such a sub-tree
compares as (outer box, item set, shape of the sizes: left = count >> 1, recursively); inside it each tree's boxes must
be the unions of its own items.  Whether a task is a median region is decided here from the item boxes with the
reference's sa() in float32, from neither tree.
COVERAGE.  compare() counts what it walked (block-parallel tasks, deferred ones, leaf groups, median regions) and, on
request, records every binned task with its centroid box and sides, so that a test can assert that a tie occurred and
how it was resolved; select_axis / plane_scores restate the two rules for those assertions only.  The scene builders at
the end place items on dyadic coordinates, where extents, scores and bin edges are exact.
"""
import numpy as np

from oracle import oracle_py as ora

F32 = np.float32
CHILD_MASK = np.uint32(0x1FFFFFFF)
SMALL = 32                    # SMALL_TASK_THRESHOLD: a child task below it is deferred to the per-thread loop
FMAX = np.finfo(np.float32).max


class Mismatch(AssertionError):
    pass


def ntype(nodes, s):
    return int(nodes["w28"][s] >> np.uint32(29))


def nchild(nodes, s):
    return int(nodes["w28"][s] & CHILD_MASK)


def ncount(nodes, s):
    return int(nodes["w12"][s] >> np.uint32(29))


def nbox(nodes, s):
    return np.concatenate([nodes["min"][s], nodes["max"][s]]).astype(F32)


# ---------------------------------------------------------------- the reference's float32 arithmetic on item boxes
def centroids(boxes):
    b = np.asarray(boxes, F32).reshape(-1, 6)
    return ((b[:, :3] + b[:, 3:]) * F32(0.5)).astype(F32)


def bounds_of_points(pts):
    return np.concatenate([pts.min(axis=0), pts.max(axis=0)]).astype(F32)


def union_of_boxes(boxes):
    b = np.asarray(boxes, F32).reshape(-1, 6)
    return np.concatenate([b[:, :3].min(axis=0), b[:, 3:].max(axis=0)]).astype(F32)


def sa32(box):
    """sa() of Common.cuh:293-297, float32, no contraction"""
    l = (box[3:] - box[:3]).astype(F32)
    return F32(2.0) * F32(F32(F32(l[0] * l[1]) + F32(l[0] * l[2])) + F32(l[1] * l[2]))


def select_axis(c):
    """SelectAxis (SharedTaskBuilder.cu:197-204) and which of its comparisons met equal operands"""
    l = (c[3:] - c[:3]).astype(F32)
    axis = 2 * int(l[2] > l[0] and l[2] > l[1]) + 1 * int(l[1] > l[0] and l[1] >= l[2])
    longest = max(l)
    tied = tuple(k for k in range(3) if l[k] == longest)
    return axis, tied


def plane_scores(boxes, c, axis):
    """BinCentroids + SelectPlane (SharedTaskBuilder.cu:206-350) restated for the coverage assertions only: the score of
    every plane 0..6 with both sides non-empty, and the left count it gives.  float32 throughout."""
    b = np.asarray(boxes, F32).reshape(-1, 6)
    ctr = centroids(b)
    eps = F32(1.1920929e-7)
    k1 = F32(F32(F32(8) * F32(F32(1) - eps)) / F32(c[3 + axis] - c[axis]))
    bins = (k1 * (ctr[:, axis] - c[axis]).astype(F32)).astype(F32).astype(np.int32)
    out = {}
    for plane in range(7):
        left, right = b[bins <= plane], b[bins > plane]
        if len(left) and len(right):
            score = F32(F32(sa32(union_of_boxes(left)) * F32(len(left))) + F32(sa32(union_of_boxes(right)) * F32(len(right))))
            out[plane] = (score, len(left))
    return out


# ---------------------------------------------------------------- canonical form
class Canon:
    __slots__ = ("box", "keys", "kids", "key", "slot")

    def __init__(self, box, keys, kids, key, slot):
        self.box, self.keys, self.kids, self.key, self.slot = box, keys, kids, key, slot

    @property
    def is_item(self):
        return self.kids is None


def canon(nodes, slot, item_of):
    """Walk from `slot`.  item_of(slot) -> the item's key, or None for an inner slot.  An inner slot must be a Box with
    count 2: (child, child + 1) = (left, right)."""
    key = item_of(slot)
    if key is not None:
        return Canon(nbox(nodes, slot), frozenset([key]), None, key, slot)
    if ntype(nodes, slot) != ora.CHILD_BOX or ncount(nodes, slot) != 2:
        raise Mismatch(f"slot {slot}: inner slot of type {ntype(nodes, slot)} count {ncount(nodes, slot)}")
    c = nchild(nodes, slot)
    kids = [canon(nodes, c, item_of), canon(nodes, c + 1, item_of)]
    if kids[0].keys & kids[1].keys:
        raise Mismatch(f"slot {slot}: an item on both sides")
    return Canon(nbox(nodes, slot), kids[0].keys | kids[1].keys, kids, None, slot)


def new_stats():
    return dict(big=0, root_small=0, small=0, leaf_groups=0, singles=0, median_big=0, median_small=0, median_roots=[],
                bit_diffs=[], tasks=[])


def _name(key):
    return key[0] if isinstance(key, tuple) else key


def _box_check(a, b, path, stats):
    if not np.array_equal(a.box, b.box):
        raise Mismatch(f"{path}: box {a.box.tolist()} != reference {b.box.tolist()} (slots {a.slot} / {b.slot})")
    ab, bb = a.box.view(np.uint32), b.box.view(np.uint32)
    for k in np.nonzero(ab != bb)[0]:
        stats["bit_diffs"].append((path, int(k), hex(int(ab[k])), hex(int(bb[k]))))


def _median_shape(t, item_boxes, path, which):
    """inside a median region: sizes follow count >> 1, every box is the union of its own items"""
    n = len(t.keys)
    want = union_of_boxes([item_boxes[k] for k in t.keys])
    if not np.array_equal(t.box, want):
        raise Mismatch(f"{path} ({which}): box is not the union of its items")
    if t.is_item:
        return
    if n == 2:
        if not (t.kids[0].is_item and t.kids[1].is_item):
            raise Mismatch(f"{path} ({which}): a 2-item task must be a leaf group")
    elif len(t.kids[0].keys) != n >> 1:
        raise Mismatch(f"{path} ({which}): median split of {n} items has {len(t.kids[0].keys)} on the left, not {n >> 1}")
    for side, kid in zip("LR", t.kids):
        _median_shape(kid, item_boxes, path + side, which)


def compare(a, b, item_boxes, stats, root_c=None, path="", record_tasks=False):
    """a: ours, b: the reference's.  item_boxes: key -> the item's box as fed.  root_c: the root task's centroid box
    where the launch is given one that is not the bounds of its items' centroids."""
    if a.keys != b.keys:
        only_a, only_b = [_name(k) for k in sorted(a.keys - b.keys)[:5]], [_name(k) for k in sorted(b.keys - a.keys)[:5]]
        raise Mismatch(f"{path or 'root'}: item sets differ: only ours {only_a}, only the reference {only_b}")
    _box_check(a, b, path or "root", stats)
    if a.is_item or b.is_item:
        if not (a.is_item and b.is_item):
            raise Mismatch(f"{path or 'root'}: an item on one side, a Box on the other")
        stats["singles"] += 1
        return
    n = len(a.keys)
    if n == 2:
        for which, t in (("ours", a), ("reference", b)):
            if not (t.kids[0].is_item and t.kids[1].is_item):
                raise Mismatch(f"{path or 'root'} ({which}): a 2-item task must be a leaf group")
            for kid in t.kids:
                if not np.array_equal(kid.box, item_boxes[kid.key]):
                    raise Mismatch(f"{path or 'root'} ({which}): leaf box of item {_name(kid.key)}")
        for ka in a.kids:     # as a set: match by key, then the boxes bit-report
            kb = b.kids[0] if b.kids[0].key == ka.key else b.kids[1]
            _box_check(ka, kb, (path or "root") + "{}", stats)
        stats["leaf_groups"] += 1
        return
    keys = list(a.keys)
    boxes = [item_boxes[k] for k in keys]
    c = bounds_of_points(centroids(boxes)) if root_c is None else np.asarray(root_c, F32)
    if sa32(c) <= 0:          # median region
        stats["median_big" if n > SMALL else "median_small"] += 1
        stats["median_roots"].append((path or "root", n))
        _median_shape(a, item_boxes, path or "root", "ours")
        _median_shape(b, item_boxes, path or "root", "reference")
        return
    # RunTask (block-parallel) takes the root task of a launch and every child task of at least SMALL items; a smaller
    # child task is deferred to PerInstanceRunTask
    stats["big" if n >= SMALL else "root_small" if path == "" else "small"] += 1
    if record_tasks:
        stats["tasks"].append(dict(path=path or "root", n=n, c=c, boxes=np.asarray(boxes, F32),
                                   left=len(a.kids[0].keys),
                                   on_left=np.array([k in a.kids[0].keys for k in keys])))
    for side in (0, 1):
        compare(a.kids[side], b.kids[side], item_boxes, stats, None, path + "LR"[side], record_tasks)


# ---------------------------------------------------------------- feeding: RunSahBuild
def tri_items(nodes, slot):
    """the Tri slots reachable from `slot`: [(leaf record, count, box)]"""
    out, stack = [], [slot]
    while stack:
        s = stack.pop()
        t = ntype(nodes, s)
        if t == ora.CHILD_TRI:
            out.append((nchild(nodes, s), ncount(nodes, s), nbox(nodes, s)))
        elif t == ora.CHILD_BOX:
            c = nchild(nodes, s)
            stack.extend(range(c, c + ncount(nodes, s)))
        else:
            raise Mismatch(f"slot {s}: type {t} inside a cell tree")
    return out


def sah_feed(nodes, cell_counts, tris, splits):
    """the inputs of RunSahBuild's two SharedTaskBuild launches, read back from a finished tree"""
    counts = np.asarray(cell_counts, np.int64).astype(np.int32)
    scan = (np.cumsum(counts) - counts).astype(np.int32)
    L = int(counts.sum())
    aabbs, prims = np.zeros((max(L, 1), 6), F32), np.zeros((max(L, 1), 2), np.uint32)
    empty = np.array([FMAX] * 3 + [-FMAX] * 3, F32)
    c, p = np.tile(empty, (64, 1)), np.tile(empty, (64, 1))
    for b in range(64):
        if not counts[b]:
            continue
        # (with splits one leaf record can have several references in a cell: the pieces differ in their boxes)
        items = sorted(tri_items(nodes, 128 + 2 * int(scan[b])), key=lambda it: (it[0], it[2].tolist()))
        assert len(items) == counts[b], f"cell {b}: {len(items)} Tri slots under the sub-root, {counts[b]} counted"
        assert len({(it[0], it[2].tobytes()) for it in items}) == len(items), f"cell {b}: the same reference twice"
        for i, (child, count, box) in enumerate(items):
            aabbs[scan[b] + i] = box
            prims[scan[b] + i] = (child, count)
        mine = aabbs[scan[b]:scan[b] + counts[b]]
        c[b] = bounds_of_points(centroids(mine))
        p[b] = union_of_boxes(mine)
    # scene bounds (Multiblock.cu Setup: the centroids of every triangle's own box, also of the two halves of a pair;
    # with splits the centroids of the items)
    if L:
        t = np.ascontiguousarray(tris, F32).reshape(-1, 3, 3)
        tri_boxes = np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1)
        scene_c = bounds_of_points(centroids(aabbs[:L] if splits else tri_boxes))
        scene_p = union_of_boxes(aabbs[:L])
    else:
        scene_c = scene_p = empty
    return dict(L=L, counts=counts, scan=scan, aabbs=aabbs, prims=prims, c=c, p=p, scene_c=scene_c, scene_p=scene_p)


def ref_sah_nodes(feed, width=64, top_width=64, cells=True, top=True, cell_nodes=None):
    """the reference's kernel on the fed inputs: (Node array, error flags of the cell launch, of the top launch)"""
    L = feed["L"]
    nodes = np.zeros(128 + 2 * L + 2, ora.NODE) if cell_nodes is None else cell_nodes.copy()
    err_cells = np.zeros(64, np.int32)
    if cells:
        err_cells = ora.ref_shared_task_build(64, width, feed["c"], feed["p"], nodes, feed["aabbs"], feed["prims"],
                                              np.arange(max(L, 1)), feed["counts"], feed["scan"], L, False,
                                              ora.CHILD_TRI, 128)
    err_top = np.zeros(1, np.int32)
    if top:
        live = np.nonzero(feed["counts"])[0].astype(np.int32)
        K = live.shape[0]
        err_top = ora.ref_shared_task_build(1, top_width, feed["scene_c"], feed["scene_p"], nodes, feed["p"],
                                            np.zeros((64, 2), np.uint32), live if K else np.zeros(1, np.int32),
                                            np.array([K], np.int32), feed["scan"], K, True, ora.CHILD_BOX, 0)
    return nodes, err_cells, err_top


def cell_item_of(nodes):
    """a cell tree's item: (leaf record, box bytes)"""
    return lambda s: (nchild(nodes, s), nbox(nodes, s).tobytes()) if ntype(nodes, s) == ora.CHILD_TRI else None


def cell_descriptors(nodes, feed):
    """(child, count, box bytes) of each non-empty cell's sub-root -> cell: how a top-tree leaf names its cell"""
    d = {}
    for b in np.nonzero(feed["counts"])[0]:
        s = 128 + 2 * int(feed["scan"][b])
        d[(nchild(nodes, s), ncount(nodes, s), nbox(nodes, s).tobytes())] = int(b)
    assert len(d) == int((feed["counts"] > 0).sum()), "two cells with the same sub-root descriptor"
    return d


def top_item_of(nodes, feed):
    d = cell_descriptors(nodes, feed)
    return lambda s: d.get((nchild(nodes, s), ncount(nodes, s), nbox(nodes, s).tobytes()))


def compare_sah(nodes, ref_nodes, feed, stats=None, record_tasks=False, cells=None, top=True):
    """ours against the reference's, cell by cell and then the top tree.  Returns the stats."""
    stats = new_stats() if stats is None else stats
    item_boxes_all = feed["aabbs"]
    for b in (np.nonzero(feed["counts"])[0] if cells is None else cells):
        lo, n = int(feed["scan"][b]), int(feed["counts"][b])
        item_boxes = {(int(feed["prims"][lo + i, 0]), item_boxes_all[lo + i].tobytes()): item_boxes_all[lo + i]
                      for i in range(n)}
        root = 128 + 2 * lo
        a = canon(nodes, root, cell_item_of(nodes))
        r = canon(ref_nodes, root, cell_item_of(ref_nodes))
        try:
            compare(a, r, item_boxes, stats, feed["c"][b], "", record_tasks)
        except Mismatch as e:
            raise Mismatch(f"cell {int(b)}: {e}") from None
    if top and feed["L"]:
        cell_boxes = {int(b): feed["p"][b] for b in np.nonzero(feed["counts"])[0]}
        a = canon(nodes, 0, top_item_of(nodes, feed))
        r = canon(ref_nodes, 0, top_item_of(ref_nodes, feed))
        try:
            compare(a, r, cell_boxes, stats, feed["scene_c"], "", record_tasks)
        except Mismatch as e:
            raise Mismatch(f"top tree: {e}") from None
    return stats


def check_sah(nodes, cell_counts, tris, splits=False, width=64, top_width=64, record_tasks=False):
    """feed, run the reference (error flags must be clear), compare.  Returns (stats, feed, the reference's nodes)."""
    feed = sah_feed(nodes, cell_counts, tris, splits)
    ref_nodes, e1, e2 = ref_sah_nodes(feed, width, top_width)
    assert not e1.any() and not e2.any(), f"the reference kernel raised its error flag: cells {np.nonzero(e1)[0]}, top {e2}"
    stats = compare_sah(nodes, ref_nodes, feed, record_tasks=record_tasks)
    return stats, feed, ref_nodes


# ---------------------------------------------------------------- feeding: the hybrid top tree
def hybrid_item_of(nodes, base):
    return lambda s: nchild(nodes, s) if (ntype(nodes, s) == ora.CHILD_BOX and nchild(nodes, s) < base) else None


def check_hybrid(nodes, L, aabb_ordered, width=64, record_tasks=False):
    """nodes: LBVH in [0, 2(L-1)), our top tree from slot 2L.  The reference's ExtractDepth gives the sub-roots and
    c_aabb; its SharedTaskBuild<<<1, width>>> the top tree (BuildWrapper.cu:350-360).  Returns (stats, sub-roots, c)."""
    base = 2 * L
    lbvh = np.ascontiguousarray(nodes[:base]).copy()
    sub, boxes, c, p = ora.ref_extract_depth(lbvh, aabb_ordered, L)
    K = sub.shape[0]
    ref_nodes = np.zeros(base + 2 * K + 2, ora.NODE)
    ref_nodes[:lbvh.shape[0]] = lbvh
    prims = np.stack([sub, np.full(K, 2, np.uint32)], axis=1)
    err = ora.ref_shared_task_build(1, width, c, p, ref_nodes, boxes, prims, np.arange(K), np.array([K], np.int32),
                                    np.zeros(1, np.int32), K, False, ora.CHILD_BOX, base)
    assert not err.any(), "the reference kernel raised its error flag"
    a = canon(nodes, base, hybrid_item_of(nodes, base))
    r = canon(ref_nodes, base, hybrid_item_of(ref_nodes, base))
    assert a.keys == frozenset(int(s) for s in sub), "our top tree's leaves are not ExtractDepth's sub-roots"
    stats = new_stats()
    compare(a, r, {int(s): boxes[i] for i, s in enumerate(sub)}, stats, c, "", record_tasks)
    return stats, sub, c, ref_nodes


# ---------------------------------------------------------------- scenes with exact (dyadic) coordinates
def small_tris(points, e=0.25):
    """one small triangle per point: box extents (e, e, 0)"""
    p = np.asarray(points, F32).reshape(-1, 1, 3)
    return (p + np.array([[0, 0, 0], [e, 0, 0], [0, e, 0]], F32)).reshape(-1, 9)


def lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return small_tris(g)


def columns(k):
    """k columns one unit apart on x, each of two triangles at y = 0 and 0.5, and one triangle far away on y so that the
    columns share one row of grid cells: every x cell holds k / 4 evenly spaced columns"""
    pts = [(x, y, 0) for x in range(k) for y in (0.0, 0.5)] + [(0, 100, 0)]
    return small_tris(pts)


def bin_edge_scene(shifted, clusters):
    """`clusters` rows (8 apart on y) of 17 columns half a unit apart on x, alternating between y and y + 0.5; with
    `shifted` the columns 4 .. 7.5 lie 2^-21 higher.  Two far triangles keep the rows inside one grid cell.  Returns
    (triangles, the columns' x).  A row's centroid extent on x is exactly 8, so k1 = 1 - 2^-23: the column in the middle
    sits on the edge between bins 3 and 4 (tests/test_ref_sah_cpu.py::test_bin_constant_last_place)."""
    u = F32(2.0) ** F32(-21)
    k1 = F32(1 - 2.0 ** -23)
    xs = [F32(i / 2) + (u if shifted and 8 <= i < 16 else F32(0)) for i in range(17)]
    assert xs[8] == F32(4) + (u if shifted else 0) and int(F32(k1 * xs[8])) == (4 if shifted else 3)
    pts = [(x, y0 + 0.5 * (i & 1), 0) for y0 in (0.0, 8.0)[:clusters] for i, x in enumerate(xs)]
    return small_tris(pts + [(-1000, 0, 0), (0, 1000, 0)]), xs
