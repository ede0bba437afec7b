"""The exact vote of the hold-at-pop traversal (csrc/rt_traverse.hpp RT_TRACE_PAIR_STEP = 2, exact_cur): a vote under which
no unfinished lane carries a near and every unfinished lane sits on a PAIR whose index is at most 2^27 - 2 runs both of its box
steps in the pair-local form with the pair's address as scalar base + (cur << 5) as a 32-bit lane offset; a lane whose cur is
not such a pair after the first step sits the second one out, and any other vote runs the general step.  Only the interleaving
across lanes may change: every comparison is exact -- frame bytes and sum(box tests) / sum(triangle tests) against the oracle.
(The cases hold for every value of the knob.)

The cases are the smallest shapes on which the guard or the sit-out can go wrong:

* MIXED trees (pairs beside 3-, 4- and 7-slot nodes): a lane reaches a wider node in the second step of an exact vote and must
  sit out -- the schedule model (tools/quad_wait_model.py --pair 3) says that it happens in the frame;
* LONE slots (count 1) under Box children, the last of them the last slot of a node array allocated with no slack: a lone
  slot fetched as a pair would read past the array's end, and would test a slot that is not there;
* the 4 GiB edge: a node array of (2^27 + 64) slots, of which only a grid_mesh(8) LBVH's few hundred are written, its pairs
  re-indexed to sit below the edge, at 2^27 - 4, at 2^27 - 2 (the last exact pair), at 2^27 - 1 (a pair that straddles the
  edge, at an odd index) and from 2^27 up, the root once low and once high: waves change form on the index alone;
* ties, a near carried across a leaf phase, a full 64-entry stack: the pair-step file's scenes;
* 4 spp, a row band that cuts a tile, the node array at an odd 32-byte offset (a pair is not 64-byte aligned).

The CPU test executes the rule on the schedule model: every ray's sequence of box tests, pushes and leaf tests is the general
form's, every step of an exact vote sits on an exact cur (Ray.pair_step asserts it), and every pass of the loop steps a lane
or runs a leaf phase.  A wrong flag is a hang, not a wrong pixel: that test runs without a GPU."""
import numpy as np
import pytest

import edge_scenes
from test_gpu_trace_lean_step import _shifted
from test_gpu_trace_pair_step import _mixed, _mixed_arrays, _widths
from test_gpu_trace_quad_wait import _Tree, _check, _coincident, _model, _tree

gpu = pytest.mark.gpu
SIZES = ((33, 25), (64, 48))
MASK = 0x1FFFFFFF
EDGE = 1 << 27                      # slots: index 2^27 is byte 2^32 of the node array
FORM_KEYS = ("exact", "general", "sat_out", "sat_wide", "sat_lone", "sat_far")


def _lone_nodes(nodes, node_dtype):
    """Every third Box child that points to a pair is led through a LONE slot: the child points to a new node of one slot
    (appended to the array) that repeats the child's box and points to the pair.  A ray tests that box twice, in the oracle
    as in the kernel.  The last slot of the array is a lone one."""
    n = len(nodes)
    out = np.array(nodes, dtype=node_dtype)
    extra = []
    for i in range(n):
        typ, child, ccount = int(nodes[i]["w28"]) >> 29, int(nodes[i]["w28"]) & MASK, int(nodes[i]["w12"]) >> 29
        if typ == 1 and ccount == 2 and (child // 2) % 3 == 0:
            at = n + len(extra)
            lone = nodes[i].copy()
            lone["w12"] = (2 << 29) | (i & MASK)
            extra.append(lone)
            out[i]["w28"] = (1 << 29) | at
            out[i]["w12"] = (1 << 29) | (int(out[i]["w12"]) & MASK)
            for k in range(2):                                            # (the pair's parent; its own count bits stay as they are now)
                out[child + k]["w12"] = (int(out[child + k]["w12"]) & ~MASK & 0xFFFFFFFF) | at
    assert extra, "the tree has lone slots"
    out = np.concatenate([out, np.array(extra, dtype=node_dtype)])
    seen, todo = set(), [(0, 2)]                                          # still a tree: every slot is reached exactly once
    while todo:
        index, cnt = todo.pop()
        for s in range(index, index + cnt):
            assert s not in seen and s < len(out), f"slot {s} is reached twice or lies outside the array"
            seen.add(s)
            if int(out[s]["w28"]) >> 29 == 1:
                todo.append((int(out[s]["w28"]) & MASK, int(out[s]["w12"]) >> 29))
    assert len(seen) == len(out)
    assert int(out[-1]["w12"]) >> 29 == 2 and int(out[int(out[-1]["w12"]) & MASK]["w12"]) >> 29 == 1, "the last slot is a lone one"
    return out


def _lone(rt, ora, tris):
    b = ora.build_bvh(tris)
    nodes = _lone_nodes(b["nodes"], rt.NODE)
    assert _widths(nodes).get(1, 0) > 0 and _widths(nodes).get(2, 0) > 0
    return b["leaves"], nodes, 0, 2, dict(inp=_Tree(rt, nodes, b["leaves"]))


def _forms(m, tree, cam, w, h):
    """the model's counters of the exact vote summed over every tile of a w x h frame"""
    mtree = m.Tree(tree[1], tree[0], tree[2], tree[3])
    tot = dict.fromkeys(FORM_KEYS, 0)
    for ty in range((h + 7) // 8):
        for tx in range((w + 7) // 8):
            res = m.run_wave(m.tile_rays(mtree, cam, w, h, tx, ty), hold=True, pair=3)
            for k in FORM_KEYS:
                tot[k] += res[k]
    return tot


@gpu
@pytest.mark.parametrize("G", [8, 24])
def test_a_wider_node_reached_in_the_second_step_sits_out(rt, scenes, ora, G):
    tree = _mixed(rt, ora, scenes.grid_mesh(G, 1))
    assert {3, 4, 7} & set(_widths(tree[1]))
    forms = _forms(_model(), tree, scenes.camera_a(G), 33, 25)
    assert forms["exact"] > 0 and forms["general"] > 0 and forms["sat_wide"] > 0, forms
    for name, cam in (("top", scenes.camera_a(G)), ("oblique", scenes.camera_b(G))):
        for (w, h) in SIZES:
            for render_type in (0, 1, 2):
                _, oc = _check(ora, tree, cam, w, h, f"mixed grid {G} {name}", render_type)
            assert oc[1] > 0, "the frame hits the mesh"


@gpu
@pytest.mark.parametrize("G", [8, 24])
def test_a_lone_slot_is_never_fetched_as_a_pair(rt, scenes, ora, G):
    """The node array is a tensor of exactly its own size and ends in a lone slot: the pair fetch of that slot would read 32
    bytes past the tensor's end and test them as a second slot."""
    tree = _lone(rt, ora, scenes.grid_mesh(G, 1))
    assert tree[4]["inp"].nodes_out.numel() * tree[4]["inp"].nodes_out.element_size() == tree[1].nbytes, "no slack behind the last slot"
    forms = _forms(_model(), tree, scenes.camera_a(G), 33, 25)
    assert forms["exact"] > 0 and forms["sat_lone"] > 0, forms
    for name, cam in (("top", scenes.camera_a(G)), ("oblique", scenes.camera_b(G))):
        for (w, h) in SIZES:
            for render_type in (0, 1, 2):
                _, oc = _check(ora, tree, cam, w, h, f"lone slots grid {G} {name}", render_type)
            assert oc[1] > 0


def _edge_tree(rt, ora, tris, straddle, root_high):
    """A grid LBVH in a node array of EDGE + 64 slots (host: zero pages never touched; device: uninitialised).  Pairs in
    depth-first order from the root: every other two go high -- the first of them to EDGE - 2 (the last exact pair) or, with
    `straddle`, to EDGE - 1 (slots on both sides of 4 GiB, an odd index), the next ones upwards from there in steps of two
    -- the first pair under the root goes to EDGE - 4 and the rest stay low.  root_high: the root pair takes the topmost place."""
    import torch
    b = ora.build_bvh(tris)
    src = b["nodes"]
    order, todo = [], [0]
    while todo:
        p = todo.pop()
        order.append(p)
        for k in (1, 0):
            assert int(src[p + k]["w12"]) >> 29 == 2 or int(src[p + k]["w28"]) >> 29 != 1, "an LBVH is a tree of pairs"
            if int(src[p + k]["w28"]) >> 29 == 1:
                todo.append(int(src[p + k]["w28"]) & MASK)
    assert 2 * len(order) == len(src)
    first = EDGE - 1 if straddle else EDGE - 2
    high = [first] + list(range(first + 2, EDGE + 63, 2))
    new = {}
    if root_high:
        new[0] = high.pop()
    else:
        new[0] = 0
    low = 2
    for rank, p in enumerate(order[1:], 1):
        if rank == 1:
            new[p] = EDGE - 4
        elif rank % 4 >= 2 and high:
            new[p] = high.pop(0)
        else:
            new[p] = low
            low += 2
    assert first in new.values() and first + 2 in new.values() and len(set(new.values())) == len(order)
    try:
        nodes = np.zeros(EDGE + 64, rt.NODE)
        dev = torch.empty((EDGE + 64) * 32, dtype=torch.uint8, device="cuda")
    except (MemoryError, RuntimeError) as e:
        pytest.skip(f"no room for a node array of 2^27 + 64 slots (4 GiB): {type(e).__name__}")
    slot = {p + k: q + k for p, q in new.items() for k in range(2)}
    for p, q in new.items():
        for k in range(2):
            rec = src[p + k].copy()
            if int(rec["w28"]) >> 29 == 1:
                rec["w28"] = (1 << 29) | new[int(rec["w28"]) & MASK]
            rec["w12"] = (int(rec["w12"]) & ~MASK & 0xFFFFFFFF) | slot.get(int(rec["w12"]) & MASK, 0)
            nodes[q + k] = rec
    for lo, hi in ((0, low), (EDGE - 8, EDGE + 64)):                       # only the slots of the tree are written
        dev[lo * 32:hi * 32] = torch.from_numpy(nodes[lo:hi].view(np.uint8).reshape(-1).copy()).to("cuda")

    class Edge:
        nodes_out = dev
        triangles_out = rt.to_device(np.ascontiguousarray(b["leaves"]))
    return b["leaves"], nodes, new[0], 2, dict(inp=Edge)


@gpu
@pytest.mark.parametrize("root_high", [False, True], ids=["root-low", "root-high"])
@pytest.mark.parametrize("straddle", [False, True], ids=["last-exact", "straddling"])
def test_pairs_on_both_sides_of_4_gib(rt, scenes, ora, straddle, root_high):
    G = 8
    tree = _edge_tree(rt, ora, scenes.grid_mesh(G, 1), straddle, root_high)
    assert (tree[2] > EDGE) == root_high
    for (w, h) in SIZES:
        for render_type in (0, 1, 2):
            _, oc = _check(ora, tree, scenes.camera_a(G), w, h, f"4 GiB edge, straddle {straddle}, root {tree[2]}", render_type)
        assert oc[1] > 0


@gpu
@pytest.mark.parametrize("kind", ["lbvh", "mixed", "lone"])
@pytest.mark.parametrize("scene", ["coincident", "signed-zero"])
def test_equal_fronts_the_larger_index_wins(rt, scenes, ora, scene, kind):
    if scene == "signed-zero":
        tris, cam = edge_scenes.signed_zero_mesh(scenes), scenes.make_camera((0.0, 6.0, 0.0), 0.3, 1.2, 60.0)
    else:
        tris, cam = _coincident(37), scenes.make_camera((0.0, 10.0, 0.0), 0.0, 1.5, 40.0)
    tree = _tree(rt, ora, tris, "lbvh") if kind == "lbvh" else _mixed(rt, ora, tris) if kind == "mixed" else _lone(rt, ora, tris)
    for (w, h) in SIZES:
        for render_type in (0, 1, 2):
            _, oc = _check(ora, tree, cam, w, h, f"{scene} {kind}", render_type)
        assert oc[1] > 0


@gpu
def test_a_near_carried_across_a_leaf_phase(rt, scenes, ora):
    """(Box, leaf) first pairs of wide nodes: reached in a second step the lane sits out, and the general step that takes the
    node carries the near across the leaf phase."""
    tree = _mixed(rt, ora, scenes.grid_mesh(8, 1), box_tri=True)
    for render_type in (0, 1, 2):
        _check(ora, tree, scenes.camera_a(8), 33, 25, "(Box, leaf) first pairs", render_type)


@gpu
def test_full_stack_through_a_mixed_tree(rt, scenes, ora):
    tree = _mixed(rt, ora, scenes.fractal_corner(8000, 3, octaves=140, top_exp=42), base="sah")
    cam = scenes.diagonal_camera(2.0 ** -10, 2.0 ** 45)
    for render_type in (0, 1, 2):
        _, oc = _check(ora, tree, cam, 33, 25, "140 octaves, mixed", render_type)
        assert oc[2] == 64 and oc[3] > 0, oc


@gpu
@pytest.mark.parametrize("kind", ["mixed", "lone"])
@pytest.mark.parametrize("variant", ["spp4", "rows", "shifted"])
def test_variants(rt, scenes, ora, variant, kind):
    G, (w, h) = 24, (64, 48)
    tree = _mixed(rt, ora, scenes.grid_mesh(G, 1)) if kind == "mixed" else _lone(rt, ora, scenes.grid_mesh(G, 1))
    cam = scenes.camera_b(G)
    if variant == "spp4":
        _check(ora, tree, cam, w, h, f"{kind} 4 spp", 1, spp=4)
    elif variant == "rows":
        for rows in ((3, 29), (h - 5, h)):                                # bands that cut a tile: lanes outside the band
            _check(ora, tree, cam, w, h, f"{kind} rows {rows}", 1, rows=rows)
    else:
        for render_type in (0, 1, 2):
            _check(ora, _shifted(rt, tree), cam, w, h, f"{kind}, nodes at an odd 32-byte offset", render_type)


# ---------------------------------------------------------------- CPU: the exact vote and the sit-out on the schedule model
def test_exact_cur_is_a_pair_below_the_edge():
    m = _model()
    for index in (0, 1, 2, EDGE - 3, EDGE - 2):
        assert m.exact_cur((2 << 29) | index), index
        assert ((((2 << 29) | index) << 5) & 0xFFFFFFFF) == index * 32 and index * 32 + 64 <= 1 << 32
    for index in (EDGE - 1, EDGE, EDGE + 1, (1 << 28), (1 << 29) - 1):
        assert not m.exact_cur((2 << 29) | index), index
    for count in (0, 1, 3, 4, 5, 6, 7):
        for index in (0, 2, EDGE - 2, (1 << 29) - 1):
            assert not m.exact_cur((count << 29) | index), (count, index)
    assert not m.exact_cur(m.NO_NEAR)


def test_the_kernels_bound_is_the_models():
    """The GPU cases cannot tell index 2^27 - 2 from 2^27 - 1 as the bound (the straddling pair is still fetched right through a
    64-bit add of the zero-extended offset), so the kernel's constant and its test are pinned in the source text."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-raytracing_amd", "csrc",
                            "rt_traverse.hpp")).read()
    k = re.search(r"constexpr uint32_t kExactIndices = (0x[0-9A-Fa-f]+)u;", src)
    assert k and int(k.group(1), 16) == _model().EXACT_INDICES == EDGE - 1
    assert "return (cur - (2u << 29)) < kExactIndices;" in src, "exact_cur: count 2 and index below kExactIndices, one compare"


@pytest.mark.parametrize("scene", ["lbvh", "mixed", "lone", "coincident", "box-tri", "sah7"])
def test_model_the_exact_vote_gives_every_ray_the_general_sequence(rt, scenes, ora, scene):
    """Whole tiles of a 31 x 25 frame (partial tiles included) through the kernel's schedule with the hold rule: the general
    form against the exact vote.  Ray.pair_step asserts that every step of an exact vote starts without a carried near, on
    an exact cur; run_wave raises on a pass that neither steps a lane nor runs a leaf phase and on a wave that ends with an
    unfinished lane.  On a tree of pairs no lane ever sits out, so the wave's vote count is the narrow rule's."""
    m = _model()
    if scene == "lbvh":
        b = ora.build_bvh(scenes.grid_mesh(16, 1))
        leaves, nodes, root, count, cam = b["leaves"], b["nodes"], 0, 2, scenes.camera_b(16)
    elif scene == "mixed":
        (leaves, nodes, root, count), cam = _mixed_arrays(rt, ora, scenes.grid_mesh(16, 1)), scenes.camera_b(16)
    elif scene == "lone":
        b = ora.build_bvh(scenes.grid_mesh(16, 1))
        leaves, nodes, root, count, cam = b["leaves"], _lone_nodes(b["nodes"], rt.NODE), 0, 2, scenes.camera_b(16)
    elif scene == "coincident":
        (leaves, nodes, root, count), cam = _mixed_arrays(rt, ora, _coincident(37)), scenes.make_camera((0.0, 10.0, 0.0), 0.0, 1.5, 40.0)
    elif scene == "box-tri":
        (leaves, nodes, root, count), cam = _mixed_arrays(rt, ora, scenes.grid_mesh(8, 1), box_tri=True), scenes.camera_a(8)
    else:
        s = ora.build_sah(scenes.grid_mesh(16, 1))
        leaves, cam = s["leaves"], scenes.camera_a(16)
        nodes, root, count = edge_scenes.collapse_wide(s["nodes"], 0, 1, 7, rt.NODE)
    mtree = m.Tree(nodes, leaves, root, count)
    w, h = 31, 25
    tot = dict.fromkeys(FORM_KEYS, 0)
    for ty in range((h + 7) // 8):
        for tx in range((w + 7) // 8):
            base = m.tile_rays(mtree, cam, w, h, tx, ty)
            m.run_wave(base, hold=True)
            rays = m.tile_rays(mtree, cam, w, h, tx, ty)
            res = m.run_wave(rays, hold=True, pair=3)
            for a, b in zip(base, rays):
                assert a.visits == b.visits and a.pushes == b.pushes, f"{scene} tile {tx},{ty}: a ray's sequence differs"
                assert a.tmax == b.tmax and a.box_tests == b.box_tests and a.tri_tests == b.tri_tests and a.hit == b.hit
            for k in FORM_KEYS:
                tot[k] += res[k]
            if scene == "lbvh":
                narrow = m.run_wave(m.tile_rays(mtree, cam, w, h, tx, ty), hold=True, pair=1)
                assert (res["nbox"], res["nleaf"], res["lane_steps"]) == (narrow["nbox"], narrow["nleaf"], narrow["lane_steps"])
    assert tot["exact"] > 0, f"{scene}: no exact vote, the form never ran: {tot}"
    assert tot["sat_out"] == tot["sat_wide"] + tot["sat_lone"] + tot["sat_far"] and tot["sat_far"] == 0, tot
    if scene == "lbvh":
        assert tot["sat_out"] == 0, f"a tree of pairs: no lane sits out: {tot}"
    else:
        assert tot["general"] > 0, f"{scene}: no general vote, the switch never happened: {tot}"
    if scene in ("mixed", "box-tri", "sah7"):
        assert tot["sat_wide"] > 0, f"{scene}: no lane reached a wider node in the second step of an exact vote: {tot}"
    if scene == "lone":
        assert tot["sat_lone"] > 0, f"{scene}: no lane reached a lone slot in the second step of an exact vote: {tot}"
