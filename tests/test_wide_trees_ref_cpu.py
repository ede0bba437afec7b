"""The conditions tests/test_gpu_wide_trees.py and tests/test_gpu_wide_trees_sets.py rest on, checked without a GPU on the
oracle's trees (bit-equal to the device builders') re-packed by tests/wide_trees.py:

  * tree shape: every run length 1..7 occurs at least twice; some run has its NONE slot first, one in the middle, one last; the
    root run has at least 3 slots and holds a NONE slot; the leaf slots reached -- record index and leaf count, with
    multiplicity -- are the source tree's; the wide tree has no more slots than the source.  Trees of 3, 5 and 7 triangles
    become one root run of that many leaf slots, and carry the set-valued cases: rows of two or more hits, filters that keep
    some records and drop some, first-K rows within the undecided cap, hits on the refitted run;
  * the references agree with themselves across the re-packing: the ordered walker's t on the wide tree is the brute force's
    over the leaf records (no push is dropped on any of these trees -- asserted: dropped pushes are the business of
    tests/test_stack_walk_ref_cpu.py), and ray_hits_ref.walk's rows on the wide tree equal the binary tree's as multisets;
  * hit share: the walker alone finds a hit on at least 0.3 of the rays of every scene used for closest hits, and two or more
    hits on at least 10 % of the rays of `layers`;
  * the leaf-then-continue path: some ray's hit leaf sits in slot 0 of a pair that is not the last pair of its run;
  * refit: refit_ref on the wide tree with every vertex moved gives every reached non-NONE slot a box that holds the vertices
    under it, leaves the NONE slots' bytes alone and reports no broken pair;
  * the float64 arms the GPU tests reuse (spheres, capsules, sphere cast) keep their owners' unstable-share caps on these inputs.

The run-length histograms and hit shares are printed (pytest -s)."""
import numpy as np
import pytest

import capsule_ref as cr
import ray_filter_ref as rx
import ray_first_ref as rf
import ray_hits_ref as rh
import refit_ref
import sphere_cast_ref as scr
import sphere_ref as sr
import stack_scenes as sc
import wide_trees as wt

F = np.float32
MISS = 0xFFFFFFFF
ALL_SCENES = wt.SCENES + ("layers",)


@pytest.fixture(scope="module")
def trees(ora, scenes):
    """name, kind -> (triangles, rays, binary (leaves, nodes, root, count), wide (nodes, root, count))"""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            t = wt.tris(name, scenes)
            lv, nd, r, c = wt.ora_tree(ora, t, kind)
            cache[name, kind] = (t, wt.rays(name, t), (lv, nd, r, c), wt.repack(nd, r, c))
        return cache[name, kind]
    return get


@pytest.mark.parametrize("kind", wt.KINDS)
@pytest.mark.parametrize("name", ALL_SCENES)
def test_tree_shape(trees, name, kind):
    t, rays, (lv, nd, r, c), (w, wr, wc) = trees(name, kind)
    h, places = wt.hist(w, wr, wc), wt.none_places(w, wr, wc)
    print(f"{name} {kind}: run lengths {h}, NONE slots {places}, root run {wc}, {len(w)} slots for {len(wt.reached_slots(nd, r, c))}")
    assert set(h) == set(range(1, 8)) and min(h.values()) >= 2, h
    assert all(places.get(k, 0) >= 1 for k in ("first", "middle", "last")), places
    assert wc >= 3 and places.get("root", 0) >= 1
    assert (wt.leaf_records(w, wr, wc) == wt.leaf_records(nd, r, c)).all()
    assert len(w) == len(wt.reached_slots(w, wr, wc)) <= len(wt.reached_slots(nd, r, c)) <= len(nd)
    none = (w["w28"] >> 29) == wt.NONE
    assert (w["min"][none] == wt.NONE_MIN).all() and (w["max"][none] == wt.NONE_MAX).all() and (w["w28"][none] == 0).all()
    # plain pairs and wide runs alternate: some Box child of a pair opens a wide run, and some Box child of a wide run a pair
    kinds = {(k, int(w["w12"][s]) >> 29) for f, k in wt.runs(w, wr, wc) for s in range(f, f + k) if int(w["w28"][s]) >> 29 == wt.BOX}
    assert any(a == 2 and b > 2 for a, b in kinds) and any(a > 2 and b == 2 for a, b in kinds)
    # some wide run begins with the pair (Box, leaf)
    assert any(k > 2 and int(w["w28"][f]) >> 29 == wt.BOX and int(w["w28"][f + 1]) >> 29 == wt.TRI for f, k in wt.runs(w, wr, wc))


def test_repack_is_a_pure_function(trees):
    _, _, (lv, nd, r, c), (w, wr, wc) = trees("grid", "bottom_up")
    again = wt.repack(nd.copy(), r, c)
    assert again[0].tobytes() == w.tobytes() and again[1:] == (wr, wc)
    plain, pr, pc = wt.repack(nd, r, c, none_every=0, lone_every=0)
    assert not ((plain["w28"] >> 29) == wt.NONE).any() and (wt.leaf_records(plain, pr, pc) == wt.leaf_records(nd, r, c)).all()
    for width in (3, 4, 7):
        one, o_r, o_c = wt.repack(nd, r, c, widths=(width,), none_every=0, lone_every=0, root_width=width)
        assert max(wt.hist(one, o_r, o_c)) == width == o_c


@pytest.mark.parametrize("n", wt.TINY)
def test_tiny_trees_are_one_root_run(ora, scenes, n):
    t = wt.tris(f"tiny{n}", scenes)
    for kind in ("bottom_up", "sah"):
        lv, nd, r, c = wt.ora_tree(ora, t, kind)
        w, wr, wc = wt.single_run(nd, r, c)
        assert wt.hist(w, wr, wc) == {n: 1} and wc == n == len(w)
        rays = wt.rays(f"tiny{n}", t)
        hits, st = ora.walk_rays(lv, w, wr, wc, rays)
        share = (hits["primitive_id"] != MISS).mean()
        print(f"tiny{n} {kind}: hit share {share:.3f}")
        assert share >= 0.3 and st[:, 3].sum() == 0
        assert (hits["t"] == sc.brute_leaves_t(lv, rays)).all()
        hit_ids = set(hits["primitive_id"][hits["primitive_id"] != MISS].tolist())
        assert {0, n - 1} <= hit_ids and len(hit_ids) >= n - 1, "the leaves of the first and the last slot, and nearly all, are hit"


@pytest.mark.parametrize("n", wt.TINY)
def test_tiny_trees_carry_the_set_valued_cases(ora, scenes, n):
    """what tests/test_gpu_wide_trees_sets.py asks of its inputs on the single runs, from the references alone: rows of two or
    more hits, every filter keeps some records and drops some, no first-K row is undecided beyond the cap, and the rays aimed at
    the moved triangles hit the refitted run"""
    name = f"tiny{n}"
    t = wt.tris(name, scenes)
    rays = wt.rays(name, t)
    lv, nd, r, c = wt.ora_tree(ora, t, "bottom_up")
    w, wr, wc = wt.single_run(nd, r, c)
    rows, gates, dets, box, leaf = rx.walk_gated_det(w, lv, wr, wc, rays)
    plain, pbox, pleaf = rh.walk(w, lv, wr, wc, rays)
    assert (box, leaf) == (pbox, pleaf) and all(a.tobytes() == b.tobytes() for a, b in zip(rh.canon(rows), rh.canon(plain)))
    many, total = np.mean([len(x) >= 2 for x in rows]), sum(len(x) for x in rows)
    assert sum(len(x) > 0 for x in rows) >= len(rays) // 8 and many >= 0.05
    kept = {}
    for fname in ("cull_back", "combined"):
        frows, fgates = rx.filtered(rows, gates, dets, rx.make_filter(fname, rows, n))
        kept[fname] = sum(len(x) for x in frows)
        assert 0 < kept[fname] < total
        dedup = rf.dedup_all(frows, fgates)
        assert all(rf.undecided_share(rf.expected(frows, fgates, k, rays["tmax"], dedup=dedup), frows) <= rf.CAP for k in (1, 3, 8))
    dedup = rf.dedup_all(rows, gates)
    assert all(rf.undecided_share(rf.expected(rows, gates, k, rays["tmax"], dedup=dedup), rows) <= rf.CAP for k in (1, 3, 8))
    new = wt.moved(t, 4)
    lv1, w1, broken = refit_ref.refit_ref(lv, w, wr, wc, new)
    hits, _ = ora.walk_rays(lv1, w1, wr, wc, wt.rays(name, new))
    share = (hits["primitive_id"] != MISS).mean()
    print(f"{name}: {total} all-hit records, {100 * many:.1f} % of the rays with two or more, the filters keep {kept}; "
          f"hit share on the refitted run {share:.3f}")
    assert not broken and share >= 0.3


@pytest.mark.parametrize("kind", wt.KINDS)
@pytest.mark.parametrize("name", ALL_SCENES)
def test_walkers_on_the_wide_tree(ora, trees, name, kind):
    t, rays, (lv, nd, r, c), (w, wr, wc) = trees(name, kind)
    assert len(rays) <= 384 and len(rays) % 64 != 0, "a batch ends inside a wave"
    hits, st = ora.walk_rays(lv, w, wr, wc, rays)
    binary, _ = ora.walk_rays(lv, nd, r, c, rays)
    share = (hits["primitive_id"] != MISS).mean()
    same = (hits.view(np.dtype((np.void, 16))) == binary.view(np.dtype((np.void, 16)))).mean()
    ltc = wt.leaf_then_continue(lv, w, wr, wc, hits)
    print(f"{name} {kind}: hit share {share:.3f}, records equal to the binary tree's on {100 * same:.1f} % of the rays, "
          f"{ltc} hits in slot 0 of a pair before the run's last pair, greatest depth {int(st[:, 2].max())}")
    assert share >= 0.3
    assert st[:, 3].sum() == 0, "no push is dropped on these trees"
    assert (hits["t"] == sc.brute_leaves_t(lv, rays)).all(), "the walker's t on the wide tree is the brute force's"
    assert (hits["t"] == binary["t"]).all()
    assert ltc >= 5, "the leaf-then-continue path is taken"
    a, ast = ora.walk_rays(lv, w, wr, wc, rays, any_hit=True)
    assert ((a["primitive_id"] != MISS) == (hits["primitive_id"] != MISS)).all() and ast[:, 3].sum() == 0


@pytest.mark.parametrize("kind", ("bottom_up", "sah_pairs", "sah_splits"))
@pytest.mark.parametrize("name", ALL_SCENES)
def test_all_hit_rows_are_the_binary_trees(trees, name, kind):
    t, rays, (lv, nd, r, c), (w, wr, wc) = trees(name, kind)
    rows, box, leaf = rh.walk(w, lv, wr, wc, rays)
    brows, _, _ = rh.walk(nd, lv, r, c, rays)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rh.canon(rows), rh.canon(brows)))
    many = np.mean([len(x) >= 2 for x in rows])
    print(f"{name} {kind}: {100 * many:.1f} % of the rays have two or more hits; {box} box tests, {leaf} leaf visits")
    if name == "layers":
        assert many >= 0.10


@pytest.mark.parametrize("kind", ("bottom_up", "sah_pairs", "sah_splits"))
@pytest.mark.parametrize("name", wt.SCENES)
def test_refit_ref_on_the_wide_tree(trees, name, kind):
    t, rays, (lv, nd, r, c), (w, wr, wc) = trees(name, kind)
    new = wt.moved(t)
    assert (new != t).mean() > 0.9
    lv1, w1, broken = refit_ref.refit_ref(lv, w, wr, wc, new)
    assert not broken
    none = (w["w28"] >> 29) == wt.NONE
    assert none.sum() >= 3 and w1[none].tobytes() == w[none].tobytes(), "the NONE slots' bytes are left alone"
    assert (w1["w12"] == w["w12"]).all() and (w1["w28"] == w["w28"]).all()
    assert (w1["min"][~none] != w["min"][~none]).any()
    T = new.reshape(-1, 3, 3)

    def under(s):
        """(lo, hi) of the vertices under slot s"""
        typ, idx, cnt = int(w1["w28"][s]) >> 29, int(w1["w28"][s]) & wt.MASK, int(w1["w12"][s]) >> 29
        if typ == wt.TRI:
            ids = [int(lv["primitive_id_0"][idx])] + ([int(lv["primitive_id_1"][idx])] if int(lv["primitive_id_1"][idx]) else [])
            v = T[ids].reshape(-1, 3)
            lo, hi = v.min(0), v.max(0)
        else:
            boxes = [under(k) for k in range(idx, idx + cnt) if int(w1["w28"][k]) >> 29 != wt.NONE]
            lo, hi = np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)
        assert (w1["min"][s] <= lo).all() and (w1["max"][s] >= hi).all(), f"slot {s} does not hold its subtree"
        assert (w1["min"][s] == lo).all() and (w1["max"][s] == hi).all(), f"slot {s}'s box is not tight"
        return lo, hi

    for s in range(wr, wr + wc):
        if int(w1["w28"][s]) >> 29 != wt.NONE:
            under(s)


# ------------------------------------------------------------------ the float64 arms the GPU tests reuse
def test_sphere_arm_keeps_its_cap(scenes):
    spheres, rays = wt.sphere_scene("grid", scenes)
    ref = sr.Reference(spheres, rays)
    print(f"spheres over grid: unstable {100 * ref.unstable_share:.3f} %, hits {int(ref.f64['hit'].sum())} of {len(rays)}")
    assert ref.unstable_share <= sr.CAP
    assert ref.f64["hit"].mean() >= 0.3


def test_capsule_arm_keeps_its_cap(scenes):
    caps, rays = wt.capsule_scene("grid", scenes)
    ref = cr.Reference(caps, rays)
    print(f"capsules over grid: unstable {100 * ref.unstable_share:.3f} %, hits {int(ref.f64['hit'].sum())} of {len(rays)}")
    assert ref.unstable_share <= wt.capsule_cap()
    assert ref.f64["hit"].mean() >= 0.3


def test_sphere_cast_arm_keeps_its_cap(scenes):
    t = wt.tris("grid", scenes)
    rays, radii = wt.cast_rays("grid", t)
    ref = scr.Reference(t, rays, radii)
    print(f"sphere cast over grid: unstable {100 * ref.unstable_share:.3f} %, hits {int(ref.f64['hit'].sum())}, "
          f"overlaps {int(ref.f64['over'].sum())} of {len(rays)}")
    assert ref.unstable_share <= wt.cast_cap()
    assert ref.f64["hit"].mean() >= 0.3 and ref.f64["over"].sum() >= 10
