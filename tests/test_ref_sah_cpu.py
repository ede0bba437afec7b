"""The oracle's binned-SAH trees (ora.build_sah, ora.build_hybrid) against the reference's own SharedTaskBuild, run on the
CPU (oracle/_ref/libref_sah.so: SharedTaskBuilder.cu compiled from the reference tree, one host thread per CUDA thread,
run in turn between barriers by oracle/ref_sah_driver.cpp).  Each launch is fed from the tree being checked and the two
trees are compared in canonical form (tests/sah_canon.py): ordered children, item sets, boxes as float32 values; median
regions by outer box, item set and the shape of their sizes.  Every launch must leave the kernel's error flag clear.
The scenes are chosen so that every branch of RunTask and PerInstanceRunTask runs, and each test asserts that it ran.
The last tests show that the comparison fails on an item moved across a split, exchanged children, a box one ulp off
and a changed median region."""
import numpy as np
import pytest

import edge_scenes
import sah_canon as sc
from oracle import oracle_py

pytestmark = pytest.mark.skipif(not oracle_py.ref_sah_available(),
                                reason="oracle/_ref/libref_sah.so not built (the reference tree is not on this machine)")

F32 = np.float32


def check(ora, tris, pairs=False, splits=False, **kw):
    o = ora.build_sah(tris, pairs, splits)
    stats, feed, ref_nodes = sc.check_sah(o["nodes"], o["cell_counts"], tris, splits, **kw)
    assert feed["L"] == o["L"]
    return o, stats, feed, ref_nodes


small_tris, lattice, columns = sc.small_tris, sc.lattice, sc.columns


# ---------------------------------------------------------------- whole scenes
@pytest.fixture(scope="module")
def grid60(ora, scenes):
    return check(ora, scenes.grid_mesh(60, 2))


def test_grid60_big_and_deferred_small_tasks(grid60):
    """about 110 items per cell: tasks of >= 32 items run BinCentroids / SelectPlane / PartitionIds across the block,
    their small children are deferred to the per-thread loop"""
    _, st, feed, _ = grid60
    assert feed["L"] == 7200 and (feed["counts"] > 64).sum() >= 32
    assert st["big"] > 64 and st["small"] > 1000 and st["leaf_groups"] > 1000 and st["singles"] > 100
    assert st["bit_diffs"] == []


@pytest.mark.parametrize("name", ["soup3000", "fractal4000", "flat12"])
def test_uneven_and_flat_scenes(name, ora, scenes):
    tris = {"soup3000": lambda: scenes.soup(3000, 5, size=0.02), "fractal4000": lambda: scenes.fractal_corner(4000, 3),
            "flat12": lambda: scenes.flat_mesh(12, 3)}[name]()
    _, st, feed, _ = check(ora, tris)
    # (flat12 has 18 items per cell: its block-parallel tasks are the cells' roots)
    assert (st["big"] > 0 or name == "flat12") and st["big"] + st["root_small"] > 0 and st["small"] > 0
    if name == "fractal4000":      # one dominant cell
        assert feed["counts"].max() > feed["L"] // 4 and (feed["counts"] == 0).sum() > 8
    if name == "flat12":           # a flat axis: 16 cells, coincident centroids inside them
        assert (feed["counts"] > 0).sum() == 16 and st["median_small"] > 0
    assert st["bit_diffs"] == []


def test_pairs_items_with_two_triangles(ora, scenes):
    tris = scenes.grid_mesh(16, 2)
    o, st, feed, _ = check(ora, tris, pairs=True)
    counts = feed["prims"][:feed["L"], 1]
    assert (counts == 2).sum() > 100 and o["L"] < tris.shape[0]
    assert st["big"] > 0 and st["small"] > 0 and st["bit_diffs"] == []


def test_splits_leaf_references_in_several_cells(ora, scenes):
    tris = scenes.soup(3000, 5, size=0.3)
    o, st, feed, _ = check(ora, tris, splits=True)
    records = feed["prims"][:feed["L"], 0]
    assert o["L"] > o["R"] and np.unique(records).shape[0] == o["R"], "one record in several cells"
    assert st["big"] > 0 and st["small"] > 0 and st["bit_diffs"] == []


def test_signed_zero_mesh_values_equal_bits_listed(ora, scenes):
    """Our unions run on the ordered-int encoding (-0 < +0), the reference's small-task path on fminf / fmaxf from
    +-FLT_MAX: values must be equal; a bit difference may only be a zero of the other sign."""
    tris = edge_scenes.signed_zero_mesh(scenes)
    _, st, _, _ = check(ora, tris)
    for path, k, ours, ref in st["bit_diffs"]:
        print(f"signed_zero_mesh bit difference at {path} box[{k}]: ours {ours} reference {ref}")
        assert {ours, ref} == {"0x0", "0x80000000"}
    print(f"signed_zero_mesh: {len(st['bit_diffs'])} bit differences")
    assert st["big"] > 0 and st["small"] > 0


# ---------------------------------------------------------------- ties
def test_axis_ties_on_lattices(ora):
    """Centroid boxes with equal extents on two and on three axes.  SelectAxis: z only if strictly longest; y if longer
    than x and at least z; else x.  So x = y = z -> x, y = z > x -> y, x = y > z -> x, x = z > y -> x.  Each tie must
    occur in a block-parallel task and in a deferred one, and split on the axis the rule names into equal halves."""
    seen = set()
    for dims in ((16, 16, 16), (8, 8, 4), (8, 4, 8)):
        _, st, _, _ = check(ora, lattice(*dims), record_tasks=True)
        assert st["bit_diffs"] == []
        for t in st["tasks"]:
            axis, tied = sc.select_axis(t["c"])
            if len(tied) < 2:
                continue
            assert axis == {(0, 1, 2): 0, (1, 2): 1, (0, 1): 0, (0, 2): 0}[tied]
            ctr = sc.centroids(t["boxes"])
            left = t["on_left"]
            assert ctr[left][:, axis].max() < ctr[~left][:, axis].min(), "split on the axis SelectAxis names"
            for other in tied:
                if other != axis:
                    assert ctr[left][:, other].min() == ctr[~left][:, other].min()
                    assert ctr[left][:, other].max() == ctr[~left][:, other].max()
            assert t["left"] * 2 == t["n"], "the lattice halves"
            seen.add((tied, "parallel" if (t["n"] >= sc.SMALL or t["path"] == "root") else "deferred"))
    assert {((0, 1, 2), "parallel"), ((0, 1, 2), "deferred"), ((1, 2), "parallel"), ((1, 2), "deferred"),
            ((0, 1), "parallel"), ((0, 2), "parallel")} <= seen, seen


@pytest.mark.parametrize("k, where", [(28, "parallel"), (56, "deferred")])
def test_equal_score_planes_highest_wins(k, where, ora):
    """Seven evenly spaced columns fall into bins 0 1 2 3 5 6 7: planes 3 and 4 both give 4 | 3 columns, plane 2 gives
    3 | 4 with the mirrored, exactly equal score.  The sweep runs 6 -> 0 with strict <, so plane 4 stands: 8 items on
    the left, 6 on the right.  With 28 columns that task is a cell's root (RunTask), with 56 a deferred child."""
    _, st, _, _ = check(ora, columns(k), record_tasks=True)
    hits = 0
    for t in st["tasks"]:
        if t["n"] != 14:
            continue
        axis, _ = sc.select_axis(t["c"])
        scores = sc.plane_scores(t["boxes"], t["c"], axis)
        best = min(s for s, _ in scores.values())
        winners = sorted(p for p, (s, _) in scores.items() if s == best)
        assert axis == 0 and winners == [2, 3, 4], (winners, scores)
        assert {scores[p][1] for p in winners} == {6, 8}
        assert t["left"] == 8 == scores[max(winners)][1], "the highest of the equal-score planes wins"
        assert (t["path"] == "root") == (where == "parallel")
        hits += 1
    assert hits == (4 if k == 28 else 8)


@pytest.mark.parametrize("clusters, where", [(1, "parallel"), (2, "deferred")])
@pytest.mark.parametrize("shifted", [False, True])
def test_bin_constant_last_place(shifted, clusters, where, ora):
    """17 columns half a unit apart under a centroid extent of exactly 8, so k1 = 8 (1 - 2^-23) / 8 = 1 - 2^-23 and a
    column at x falls into bin int(fl(x (1 - 2^-23))).  The balanced split lies at the column in the middle:
    - plain: x = 4 gives 4 - 2^-21 -> bin 3, with x = 3.5: the planes offer 9 | 8 (x <= 4 on the left) but not 8 | 9.  A
      constant of 1 puts x = 4 into bin 4 and the builder takes 8 | 9.
    - shifted: the columns 4 .. 7.5 lie 2^-21 higher; 4 + 2^-21 gives 4 - 2^-44, which rounds to 4.0 -> bin 4: 8 | 9 is
      offered and 9 | 8 is not.  A constant of 1 - 2^-22 gives 4 - 2^-21 -> bin 3 and 9 | 8.
    Far triangles keep a cluster inside one grid cell; a second cluster lies 8 higher on y, so the cell's root splits on
    y and each cluster is a deferred task."""
    tris, xs = sc.bin_edge_scene(shifted, clusters)
    _, st, _, _ = check(ora, tris, record_tasks=True)
    hits = 0
    for t in st["tasks"]:
        if t["n"] != 17:
            continue
        assert t["c"][3] - t["c"][0] == 8 and sc.select_axis(t["c"])[0] == 0
        x = sc.centroids(t["boxes"])[:, 0] - t["c"][0]
        assert sorted(x[t["on_left"]].tolist()) == [float(v) for v in xs[:8 if shifted else 9]]
        assert (t["path"] == "root") == (where == "parallel")
        hits += 1
    assert hits == clusters


# ---------------------------------------------------------------- median regions
def test_median_regions_big_and_small(ora, scenes):
    """Coincident centroids (6 triangles x 100) and centroids collinear on one axis: centroid boxes without area, split at
    count >> 1 by buffer order -- compared by outer box, item set and the shape of the sizes."""
    big = small = 0
    for tris in (np.repeat(scenes.soup(6, 3, dup_fraction=0), 100, axis=0),
                 small_tris([(x, 0, 0) for x in range(500)]), small_tris([(0, 0, z) for z in range(40)])):
        _, st, _, _ = check(ora, tris)
        big += sum(1 for _, n in st["median_roots"] if n > 32)
        small += sum(1 for _, n in st["median_roots"] if n <= 32)
        assert st["median_big"] + st["median_small"] == len(st["median_roots"])
    assert big >= 1 and small >= 1, (big, small)


# ---------------------------------------------------------------- tiny scenes
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_tiny_scenes(n, ora, scenes):
    """sub-roots that are leaves, empty cells, a top tree of 1..n cells"""
    tris = scenes.soup(8, 2, dup_fraction=0.0, size=0.3)[:n]
    _, st, feed, _ = check(ora, tris)
    assert feed["L"] == n and (feed["counts"] == 0).sum() >= 64 - n


def test_single_leaf_cell_is_the_documented_difference(ora, scenes):
    """A cell with ONE leaf has a Tri sub-root; the reference's top tree copies child and count and stamps the copy as
    Box (SharedTaskBuilder.cu:432-446, and :797-805 in the deferred path), so its tracer would read a leaf record as a
    node pair.  Ours copies the type.  Everything else of the two slots is equal."""
    tris = scenes.soup(8, 2, dup_fraction=0.0, size=0.3)[:3]
    o, _, feed, ref_nodes = check(ora, tris)
    singles = [int(b) for b in np.nonzero(feed["counts"] == 1)[0]]
    assert singles
    ours_of, ref_of = sc.top_item_of(o["nodes"], feed), sc.top_item_of(ref_nodes, feed)
    for b in singles:
        sub = 128 + 2 * int(feed["scan"][b])
        assert sc.ntype(o["nodes"], sub) == sc.ntype(ref_nodes, sub) == ora.CHILD_TRI
        mine = [s for s in range(128) if ours_of(s) == b and sc.ntype(o["nodes"], s) != 0]
        theirs = [s for s in range(128) if ref_of(s) == b and sc.ntype(ref_nodes, s) != 0]
        assert len(mine) == 1 and len(theirs) == 1
        assert sc.ntype(o["nodes"], mine[0]) == ora.CHILD_TRI
        assert sc.ntype(ref_nodes, theirs[0]) == ora.CHILD_BOX, "the reference's defect"
        assert sc.nchild(o["nodes"], mine[0]) == sc.nchild(ref_nodes, theirs[0])
        assert sc.ncount(o["nodes"], mine[0]) == sc.ncount(ref_nodes, theirs[0])


# ---------------------------------------------------------------- the hybrid top tree
@pytest.mark.parametrize("name", ["grid24", "soup5000", "flat10", "grid2"])
def test_hybrid_top_tree(name, ora, scenes):
    tris = {"grid24": lambda: scenes.grid_mesh(24, 1), "soup5000": lambda: scenes.soup(5000, 3),
            "flat10": lambda: scenes.flat_mesh(10, 1), "grid2": lambda: scenes.grid_mesh(2, 1)}[name]()
    o = ora.build_hybrid(tris)
    st, sub, c, _ = sc.check_hybrid(o["nodes"], o["n"], o["aabb"])
    assert sorted(int(s) for s in sub) == sorted(int(s) for s in o["subroots"]), "the sub-root set is ExtractDepth's"
    K = sub.shape[0]
    boxes = np.array([np.concatenate([np.minimum(o["nodes"]["min"][s], o["nodes"]["min"][s + 1]),
                                      np.maximum(o["nodes"]["max"][s], o["nodes"]["max"][s + 1])]) for s in o["subroots"]])
    assert np.array_equal(c, sc.union_of_boxes(boxes)), "c_aabb = the union of the sub-root BOXES (BottomUpBuilder.cu:341-346)"
    if name == "soup5000":
        assert K == 256 and st["big"] > 0 and st["small"] > 0
    if name == "grid2":
        assert K == 2 and st["leaf_groups"] == 1
    assert st["bit_diffs"] == []


# ---------------------------------------------------------------- the block width does not matter
def test_width_invariance(grid60, ora, scenes):
    """One cell at the reference's own 512, and a whole scene's top tree at its 1024: the same canonical trees as at
    width 64.  (The turn goes round every thread at every barrier, and an empty cell costs two rounds: 64 cell blocks at
    512 take 10 s for 300 triangles, so the whole scene's cells stay at 64.)"""
    o, _, feed, ref64 = grid60
    b = int(np.argmax(feed["counts"]))
    one = dict(feed, counts=np.where(np.arange(64) == b, feed["counts"], 0).astype(np.int32))
    ref512, e1, _ = sc.ref_sah_nodes(one, width=512, top=False)
    assert not e1.any()
    st = sc.compare_sah(ref64, ref512, feed, cells=[b], top=False)
    assert st["big"] > 0 and st["small"] > 0
    sc.compare_sah(o["nodes"], ref512, feed, cells=[b], top=False)

    wide, _, e2 = sc.ref_sah_nodes(feed, top_width=1024, cells=False, cell_nodes=ref64)
    assert not e2.any()
    st = sc.compare_sah(ref64, wide, feed, cells=[])
    assert st["big"] >= 1 and st["small"] > 0, "64 cells: block-parallel tasks and deferred ones in the top tree too"
    sc.compare_sah(o["nodes"], wide, feed, cells=[])


# ---------------------------------------------------------------- teeth
def refit(nodes, slot):
    """recompute the boxes of the Box slots beneath `slot` from their children"""
    if sc.ntype(nodes, slot) != oracle_py.CHILD_BOX:
        return
    c = sc.nchild(nodes, slot)
    refit(nodes, c)
    refit(nodes, c + 1)
    nodes["min"][slot] = np.minimum(nodes["min"][c], nodes["min"][c + 1])
    nodes["max"][slot] = np.maximum(nodes["max"][c], nodes["max"][c + 1])


def walk(t):
    yield t
    if not t.is_item:
        for k in t.kids:
            yield from walk(k)


def is_median(t, item_boxes):
    return len(t.keys) > 2 and sc.sa32(sc.bounds_of_points(sc.centroids([item_boxes[k] for k in t.keys]))) <= 0


def first_item(t):
    while not t.is_item:
        t = t.kids[0]
    return t


@pytest.fixture(scope="module")
def grid_case(ora, scenes):
    tris = scenes.grid_mesh(24, 2)
    o, _, feed, ref_nodes = check(ora, tris)
    b = int(np.argmax(feed["counts"]))
    lo, n = int(feed["scan"][b]), int(feed["counts"][b])
    boxes = {(int(feed["prims"][lo + i, 0]), feed["aabbs"][lo + i].tobytes()): feed["aabbs"][lo + i] for i in range(n)}
    return o["nodes"], feed, ref_nodes, b, boxes


def test_teeth_item_moved_across_a_split(grid_case, ora):
    """a split with a leaf group on the left and a single item on the right: exchange one group member with the single
    and refit -- still a valid tree over the same leaves with the same outer boxes"""
    nodes, feed, ref_nodes, b, boxes = grid_case
    root = sc.canon(nodes, 128 + 2 * int(feed["scan"][b]), sc.cell_item_of(nodes))
    for t in walk(root):
        if (not t.is_item and len(t.keys) == 3 and not is_median(t, boxes) and t.kids[1].is_item
                and not np.array_equal(t.kids[0].kids[1].box, t.kids[1].box)):
            break
    else:
        pytest.fail("no 2 | 1 split in the cell")
    bad = nodes.copy()
    s0, s1 = t.kids[0].kids[1].slot, t.kids[1].slot
    bad[[s0, s1]] = bad[[s1, s0]]
    refit(bad, t.slot)
    assert np.array_equal(sc.nbox(bad, t.slot), t.box) and ora.verify_hierarchy(bad, 0, 1) == 0
    with pytest.raises(sc.Mismatch, match="item sets differ"):
        sc.compare_sah(bad, ref_nodes, feed, cells=[b], top=False)
    sc.compare_sah(nodes, ref_nodes, feed, cells=[b], top=False)


def test_teeth_children_exchanged(grid_case, ora):
    nodes, feed, ref_nodes, b, boxes = grid_case
    root = sc.canon(nodes, 128 + 2 * int(feed["scan"][b]), sc.cell_item_of(nodes))
    t = next(t for t in walk(root) if len(t.keys) > 4 and not is_median(t, boxes))
    bad = nodes.copy()
    c = sc.nchild(nodes, t.slot)
    bad[[c, c + 1]] = bad[[c + 1, c]]
    assert ora.verify_hierarchy(bad, 0, 1) == 0
    with pytest.raises(sc.Mismatch, match="item sets differ"):
        sc.compare_sah(bad, ref_nodes, feed, cells=[b], top=False)


def test_teeth_box_one_ulp_off(grid_case):
    nodes, feed, ref_nodes, b, boxes = grid_case
    root = sc.canon(nodes, 128 + 2 * int(feed["scan"][b]), sc.cell_item_of(nodes))
    t = [t for t in walk(root) if not t.is_item][-1]
    bad = nodes.copy()
    bad["min"][t.slot][0] = np.nextafter(bad["min"][t.slot][0], F32(-np.inf))
    with pytest.raises(sc.Mismatch, match="box"):
        sc.compare_sah(bad, ref_nodes, feed, cells=[b], top=False)
    # and in the top tree
    bad = nodes.copy()
    bad["max"][0][1] = np.nextafter(bad["max"][0][1], F32(np.inf))
    with pytest.raises(sc.Mismatch, match="top tree: root: box"):
        sc.compare_sah(bad, ref_nodes, feed, cells=[], top=True)


def test_teeth_median_region_outer_set_changed(ora, scenes):
    """a median region under a split: exchange one of its items with one from the other side and refit; the region's
    shape stays.  (12 triangles x 50: one cell holds two of them, a split over two median regions of 50.)"""
    tris = np.repeat(scenes.soup(12, 3, dup_fraction=0), 50, axis=0)
    o, st, feed, ref_nodes = check(ora, tris)
    assert st["median_big"] >= 1
    nodes = o["nodes"]
    for b in np.nonzero(feed["counts"])[0]:
        lo, n = int(feed["scan"][b]), int(feed["counts"][b])
        boxes = {(int(feed["prims"][lo + i, 0]), feed["aabbs"][lo + i].tobytes()): feed["aabbs"][lo + i] for i in range(n)}
        root = sc.canon(nodes, 128 + 2 * lo, sc.cell_item_of(nodes))
        hit = [t for t in walk(root) if not t.is_item and not is_median(t, boxes) and len(t.keys) > 2
               and any(is_median(k, boxes) and len(k.keys) > 32 for k in t.kids)]
        if hit:
            break
    else:
        pytest.fail("no split over a median region")
    t = hit[0]
    bad = nodes.copy()
    s0, s1 = first_item(t.kids[0]).slot, first_item(t.kids[1]).slot
    bad[[s0, s1]] = bad[[s1, s0]]
    refit(bad, t.slot)
    assert ora.verify_hierarchy(bad, 0, 1) == 0
    with pytest.raises(sc.Mismatch, match="item sets differ"):
        sc.compare_sah(bad, ref_nodes, feed, cells=[int(b)], top=False)
    sc.compare_sah(nodes, ref_nodes, feed, cells=[int(b)], top=False)
