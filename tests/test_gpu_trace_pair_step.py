"""The pair-local box step of the hold-at-pop traversal (csrc/rt_traverse.hpp RT_TRACE_PAIR_STEP, pair_step_on): a vote under
which no lane that counts sits on a node of more than two slots or carries a nearest child from an earlier pair is NARROW and
runs both of its box steps in a form that decides slot 0, slot 1, the one possible push and the advance from values of the
step alone; any other vote runs the general step.  A wave may change form at every vote and both forms work on one traversal
state, so nothing a ray computes may change: every comparison here is exact -- frame bytes and sum(box tests) / sum(triangle
tests) against the oracle.  (The cases hold with the knob off as well.)

The cases are the smallest shapes on which the two forms, or the switch between them, can go wrong:

* MIXED trees -- an LBVH of grid_mesh(8) / grid_mesh(24) in which only some subtrees are re-packed to nodes of 3, 4 and 7
  slots (_mixed below; the root stays a pair): waves change form between votes, and a lane enters a wide node in the second
  step of a narrow vote, where the form's tail leaves the near behind for the node's next pair;
* roots wider than a pair (the SAH tree re-packed to 3, 4, 7 slots: the first vote is general) and the plain LBVH (every vote
  narrow);
* ties -- coincident boxes and the signed-zero mesh: equal fronts, the larger index wins, in slot 1 against slot 0;
* a leaf in slot 1 of a wide node's first pair: the near and its front are carried across a leaf phase (found on the CPU by
  the schedule model, asserted to occur);
* a full 64-entry stack through a mixed tree: the near is dropped by the keep rule, the farther child by the ladder;
* 4 spp, a row band that cuts a tile (inactive lanes), the node array at an odd 32-byte offset.

The CPU test executes both forms and the narrow-vote rule on the schedule model (tools/quad_wait_model.py): every ray's
sequence of box tests, pushes and leaf tests is the general form's, and every pass of the loop steps a lane or runs a leaf
phase.  A wrong flag is a hang, not a wrong pixel: that test runs without a GPU."""
import numpy as np
import pytest

import edge_scenes
from test_gpu_trace_lean_step import _shifted
from test_gpu_trace_quad_wait import _Tree, _check, _coincident, _model, _tree

gpu = pytest.mark.gpu
SIZES = ((33, 25), (64, 48))
MASK = 0x1FFFFFFF
WIDTHS = (2, 3, 2, 4, 2, 7, 2, 2)     # the width a Box child's node is re-packed to, by the child's place in the source tree


def _mixed_nodes(nodes, root, count, node_dtype, box_tri=False):
    """Re-pack a binary tree so that only SOME of its nodes grow: the node under a Box child at source index c takes up to
    WIDTHS[(c / 2) % 8] slots (edge_scenes.collapse_wide's pulling-up, with a width per node), so pairs, 3-, 4- and 7-slot
    nodes alternate along every path.  The root run stays a pair (a single root slot is opened into its pair: launch_trace
    takes the instantiation with the hold rule for a root run of two or more).
    box_tri: only those nodes grow (to 3, 4 or 7 slots, the first that does it) whose first pair then is (Box, leaf) -- a
    tree of pairs, stepped in the pair-local form, whose few wide nodes all start with the pair that can carry a near across
    a leaf phase."""
    out = []

    def kids_of(child, ccount):
        if not box_tri:
            return widen(slots_of(child, ccount), WIDTHS[(child // 2) % len(WIDTHS)])
        for width in (3, 4, 7):
            kids = widen(slots_of(child, ccount), width)
            if len(kids) > 2 and int(kids[0]["w28"]) >> 29 == 1 and int(kids[1]["w28"]) >> 29 == 2:
                return kids
        return slots_of(child, ccount)

    def slots_of(index, cnt):
        return [nodes[index + i] for i in range(cnt)]

    def widen(sl, width):
        while True:
            res, budget = [], width - len(sl)
            for s in sl:
                typ, child, ccount = int(s["w28"]) >> 29, int(s["w28"]) & MASK, int(s["w12"]) >> 29
                if typ == 1 and ccount - 1 <= budget:
                    res.extend(slots_of(child, ccount))
                    budget -= ccount - 1
                else:
                    res.append(s)
            if len(res) == len(sl):
                return res
            sl = res

    def emit(sl, parent):
        base = len(out)
        out.extend([None] * len(sl))
        for i, s in enumerate(sl):
            rec = np.zeros((), node_dtype)
            rec["min"], rec["max"] = s["min"], s["max"]
            typ, child, ccount = int(s["w28"]) >> 29, int(s["w28"]) & MASK, int(s["w12"]) >> 29
            if typ == 1:
                kids = kids_of(child, ccount)
                cbase = emit(kids, base + i)
                rec["w28"] = (1 << 29) | cbase
                rec["w12"] = (len(kids) << 29) | (parent & MASK)
            else:
                rec["w28"] = s["w28"]
                rec["w12"] = (ccount << 29) | (parent & MASK)
            out[base + i] = rec
        return base

    import sys
    sys.setrecursionlimit(10000)
    top = slots_of(root, count)
    if len(top) < 2:
        top = widen(top, 2)
    emit(top, 0)
    return np.array(out, dtype=node_dtype), 0, len(top)


def _widths(nodes):
    """{slot count: Box children whose node has that many slots}"""
    box = (nodes["w28"] >> 29) == 1
    w, n = np.unique(nodes["w12"][box] >> 29, return_counts=True)
    return dict(zip(w.tolist(), n.tolist()))


def _mixed_arrays(rt, ora, tris, base="lbvh", box_tri=False):
    if base == "lbvh":
        b = ora.build_bvh(tris)
        leaves, nodes, root, count = b["leaves"], b["nodes"], 0, 2
    else:
        s = ora.build_sah(tris)
        leaves, nodes, root, count = s["leaves"], s["nodes"], 0, 1
    nodes, root, count = _mixed_nodes(nodes, root, count, rt.NODE, box_tri)
    hist = _widths(nodes)
    assert count == 2 and hist.get(2, 0) > 0 and sum(n for w, n in hist.items() if w > 2) > 0, \
        f"a mixed tree has plain pairs and nodes of more than two slots: {hist}"
    return leaves, nodes, root, count


def _mixed(rt, ora, tris, base="lbvh", box_tri=False):
    leaves, nodes, root, count = _mixed_arrays(rt, ora, tris, base, box_tri)
    return leaves, nodes, root, count, dict(inp=_Tree(rt, nodes, leaves))


def _cameras(scenes, G):
    return {"top": scenes.camera_a(G), "oblique": scenes.camera_b(G)}


@gpu
@pytest.mark.parametrize("cam", ["top", "oblique"])
@pytest.mark.parametrize("G", [8, 24])
def test_mixed_trees_change_form_between_votes(rt, scenes, ora, G, cam):
    tree = _mixed(rt, ora, scenes.grid_mesh(G, 1))
    hist = _widths(tree[1])
    assert {3, 4, 7} & set(hist), hist
    for (w, h) in SIZES:
        for render_type in (0, 1, 2):
            _, oc = _check(ora, tree, _cameras(scenes, G)[cam], w, h, f"mixed grid {G} {cam}", render_type)
        assert oc[1] > 0, "the frame hits the mesh"


@gpu
@pytest.mark.parametrize("kind", ["lbvh", "sah3", "sah4", "sah7"])
def test_root_runs_wider_than_a_pair_and_the_plain_pair_tree(rt, scenes, ora, kind):
    """sah3 / sah4 / sah7: the first vote of every wave is general (cur is the root run); lbvh: every vote is narrow."""
    G = 24
    tree = _tree(rt, ora, scenes.grid_mesh(G, 1), kind)
    assert tree[3] == (2 if kind == "lbvh" else int(kind[3:])), "the root run"
    for name, cam in _cameras(scenes, G).items():
        for (w, h) in SIZES:
            for render_type in (0, 1, 2):
                _, oc = _check(ora, tree, cam, w, h, f"grid {G} {kind} {name}", render_type)
            assert oc[1] > 0


@gpu
@pytest.mark.parametrize("kind", ["lbvh", "mixed"])
@pytest.mark.parametrize("scene", ["coincident", "signed-zero"])
def test_equal_fronts_the_larger_index_wins(rt, scenes, ora, scene, kind):
    if scene == "signed-zero":
        tris, cam = edge_scenes.signed_zero_mesh(scenes), scenes.make_camera((0.0, 6.0, 0.0), 0.3, 1.2, 60.0)
    else:
        tris, cam = _coincident(37), scenes.make_camera((0.0, 10.0, 0.0), 0.0, 1.5, 40.0)
    tree = _tree(rt, ora, tris, "lbvh") if kind == "lbvh" else _mixed(rt, ora, tris)
    for (w, h) in SIZES:
        for render_type in (0, 1, 2):
            _, oc = _check(ora, tree, cam, w, h, f"{scene} {kind}", render_type)
        assert oc[1] > 0


def _wave_forms(m, mtree, cam, w, h, pair):
    """the model's form counters summed over every tile of a w x h frame"""
    tot = {}
    for ty in range((h + 7) // 8):
        for tx in range((w + 7) // 8):
            res = m.run_wave(m.tile_rays(mtree, cam, w, h, tx, ty), hold=True, pair=pair)
            for k in ("narrow", "general", "tails", "carried", "wide_carried"):
                tot[k] = tot.get(k, 0) + res[k]
    return tot


@gpu
@pytest.mark.parametrize("G", [8, 24])
def test_leaf_in_slot_1_of_a_wide_nodes_first_pair(rt, scenes, ora, G):
    """The near and its front are written to near_e / near_d by the pair-local step and read by the leaf phase's general
    advance(), which moves on to the node's next pair with them.  The tree is built for it (_mixed_nodes, box_tri) and the
    schedule model says that it happens in this frame."""
    w, h = 33, 25
    tree = _mixed(rt, ora, scenes.grid_mesh(G, 1), box_tri=True)
    cam = scenes.camera_a(G)
    m = _model()
    forms = _wave_forms(m, m.Tree(tree[1], tree[0], tree[2], tree[3]), cam, w, h, pair=2)
    assert forms["wide_carried"] > 0 and forms["carried"] > forms["wide_carried"] and forms["tails"] > 0, forms
    for render_type in (0, 1, 2):
        _check(ora, tree, cam, w, h, f"grid {G}, (Box, leaf) first pairs", render_type)


@gpu
def test_full_stack_through_a_mixed_tree(rt, scenes, ora):
    """64 entries and dropped pushes: the pair-local advance drops the near by the keep rule (sp = kStackMax), the push
    ladder drops the farther child."""
    tree = _mixed(rt, ora, scenes.fractal_corner(8000, 3, octaves=140, top_exp=42), base="sah")
    cam = scenes.diagonal_camera(2.0 ** -10, 2.0 ** 45)
    for render_type in (0, 1, 2):
        _, oc = _check(ora, tree, cam, 33, 25, "140 octaves, mixed", render_type)
        assert oc[2] == 64 and oc[3] > 0, oc


@gpu
@pytest.mark.parametrize("variant", ["spp4", "rows", "shifted"])
def test_variants_on_a_mixed_tree(rt, scenes, ora, variant):
    G, (w, h) = 24, (64, 48)
    tree = _mixed(rt, ora, scenes.grid_mesh(G, 1))
    cam = scenes.camera_b(G)
    if variant == "spp4":
        _check(ora, tree, cam, w, h, "mixed 4 spp", 1, spp=4)
    elif variant == "rows":
        for rows in ((3, 29), (h - 5, h)):                                # bands that cut a tile: lanes outside the band
            _check(ora, tree, cam, w, h, f"mixed rows {rows}", 1, rows=rows)
    else:
        for render_type in (0, 1, 2):
            _check(ora, _shifted(rt, tree), cam, w, h, "mixed, nodes at an odd 32-byte offset", render_type)


# ---------------------------------------------------------------- CPU: both forms and the narrow-vote rule on the schedule model
def _model_scene(rt, scenes, ora, m, scene):
    if scene == "mixed":
        leaves, nodes, root, count = _mixed_arrays(rt, ora, scenes.grid_mesh(16, 1))
        cam = scenes.camera_b(16)
    elif scene == "sah7":
        s = ora.build_sah(scenes.grid_mesh(16, 1))
        leaves = s["leaves"]
        nodes, root, count = edge_scenes.collapse_wide(s["nodes"], 0, 1, 7, rt.NODE)
        cam = scenes.camera_a(16)
    elif scene == "box-tri":
        leaves, nodes, root, count = _mixed_arrays(rt, ora, scenes.grid_mesh(8, 1), box_tri=True)
        cam = scenes.camera_a(8)
    else:
        leaves, nodes, root, count = _mixed_arrays(rt, ora, _coincident(37))
        cam = scenes.make_camera((0.0, 10.0, 0.0), 0.0, 1.5, 40.0)
    return m.Tree(nodes, leaves, root, count), cam


@pytest.mark.parametrize("scene", ["mixed", "sah7", "coincident", "box-tri"])
def test_model_both_forms_give_every_ray_the_general_sequence(rt, scenes, ora, scene):
    """Whole tiles of a 31 x 25 frame (partial tiles included) through the kernel's schedule with the hold rule, general
    form against the kernel's narrow-vote rule (every unfinished lane counts) and the one that leaves parked lanes out.  Ray.pair_step asserts that it starts without a carried near and, in the first
    step of a vote, on no node of more than two slots; run_wave raises on a pass that neither steps a lane nor runs a leaf
    phase, and on a wave that ends with an unfinished lane."""
    m = _model()
    mtree, cam = _model_scene(rt, scenes, ora, m, scene)
    w, h = 31, 25
    tot = {1: {}, 2: {}}
    for ty in range((h + 7) // 8):
        for tx in range((w + 7) // 8):
            base = m.tile_rays(mtree, cam, w, h, tx, ty)
            m.run_wave(base, hold=True)
            for pair in (1, 2):
                rays = m.tile_rays(mtree, cam, w, h, tx, ty)
                res = m.run_wave(rays, hold=True, pair=pair)
                for a, b in zip(base, rays):
                    assert a.visits == b.visits and a.pushes == b.pushes, f"{scene} tile {tx},{ty} rule {pair}: a ray's sequence differs"
                    assert a.tmax == b.tmax and a.box_tests == b.box_tests and a.tri_tests == b.tri_tests and a.hit == b.hit
                for k in ("narrow", "general", "tails", "carried", "wide_carried"):
                    tot[pair][k] = tot[pair].get(k, 0) + res[k]
    for pair in (1, 2):
        t = tot[pair]
        assert t["narrow"] > 0, f"{scene} rule {pair}: no narrow vote, the pair-local form never ran: {t}"
        assert t["general"] > 0, f"{scene} rule {pair}: no general vote, the switch never happened: {t}"
        if scene != "coincident":
            assert t["tails"] > 0, f"{scene} rule {pair}: no lane entered a wide node in the second step of a narrow vote: {t}"
        if scene == "box-tri":
            assert t["wide_carried"] > 0, f"{scene} rule {pair}: no near carried across a leaf phase in a wide node: {t}"
    assert tot[2]["narrow"] >= tot[1]["narrow"], "rule 2 counts fewer lanes: at least as many narrow votes"
