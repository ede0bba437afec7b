"""The lean vote of the hold-at-pop traversal (csrc/rt_traverse.hpp kLeanMargin; trace_kernel's instantiations with the rule):
a vote under which no unfinished lane has more than kStackLds - kLeanMargin = 12 entries on its stack runs its box steps, and
the leaf phase that follows it, with pushes and pops that go straight to the LDS column; under any other vote the same sites
take the full ladders (LDS / private / dropped).  A wave may change arm at every vote and both arms work on one stack, so
nothing a ray computes may change: every comparison here is exact -- frame bytes and sum(box tests) / sum(triangle tests)
against the oracle.  (The cases hold for every value of RT_TRACE_LEAN_STEP: 2, as shipped, and 0, every vote on the full ladders.)

The oracle's counters say which path a case takes: oc[2] is the deepest stack of any ray of the frame, counted as the
reference counts it (the nearest child's push included, which the kernel keeps in a register: the kernel's deepest sp is
oc[2] - 1), oc[3] the pushes dropped on a full 64-entry stack.  Every case asserts the property it relies on.

launch_trace takes these instantiations for trees entered through a root pair or a wider root run: the LBVH and the SAH tree
re-packed by edge_scenes.collapse_wide (nodes of 3, 4 and 7 slots take two pushes per step).

* a scene far deeper than the LDS column in which most rays stay shallow (waves cross between the arms both ways);
* a scene for every deepest stack from 2 to kStackLds + 2 = 18, found by a sweep of fractal_corner on the CPU (DEPTH_SCENES):
  the switch sits at a kernel sp of 12, oracle depth 13, and every depth on either side of it and of the LDS column's end is
  a frame of its own, through each tree;
* a full stack (dropped pushes) through re-packed trees;
* one- and two-triangle trees and coincident triangles: the lean arm alone;
* all of it once more with the node array at an odd 32-byte offset inside a larger allocation."""
import numpy as np
import pytest

from test_gpu_trace_quad_wait import _check, _coincident, _tree

gpu = pytest.mark.gpu
K_STACK_LDS, K_LEAN_MARGIN = 16, 4          # csrc/rt_traverse.hpp
KINDS = ("lbvh", "sah3", "sah4", "sah7")
DEPTHS = tuple(range(K_LEAN_MARGIN - 2, K_STACK_LDS + 3))

# fractal_corner(n, seed, octaves=...) under diagonal_camera(2**-10, 2**45) at 33 x 25: oracle max stack = the key, no drops
DEPTH_SCENES = {
    "lbvh": {2: (5, 3, 1), 3: (8, 3, 8), 4: (12, 3, 2), 5: (12, 3, 6), 6: (20, 3, 3), 7: (20, 5, 20), 8: (20, 5, 16),
             9: (30, 3, 5), 10: (30, 5, 17), 11: (60, 3, 9), 12: (60, 3, 10), 13: (60, 3, 19), 14: (60, 7, 7),
             15: (100, 3, 15), 16: (60, 7, 13), 17: (100, 3, 27), 18: (100, 3, 22)},
    "sah3": {2: (5, 3, 4), 3: (8, 3, 2), 4: (12, 3, 10), 5: (12, 3, 4), 6: (20, 3, 8), 7: (20, 3, 5), 8: (20, 7, 27),
             9: (30, 3, 18), 10: (30, 3, 20), 11: (30, 5, 28), 12: (60, 3, 11), 13: (60, 3, 18), 14: (60, 3, 21),
             15: (60, 5, 19), 16: (100, 3, 19), 17: (100, 3, 22), 18: (100, 3, 18)},
    "sah4": {2: (8, 3, 1), 3: (8, 3, 2), 4: (12, 3, 1), 5: (20, 3, 2), 6: (20, 3, 13), 7: (30, 3, 5), 8: (30, 3, 7),
             9: (30, 3, 20), 10: (60, 3, 4), 11: (60, 3, 6), 12: (60, 3, 11), 13: (60, 3, 19), 14: (60, 3, 18),
             15: (60, 7, 28), 16: (60, 7, 21), 17: (100, 3, 5), 18: (100, 3, 19)},
    "sah7": {2: (12, 3, 6), 3: (12, 3, 1), 4: (12, 3, 12), 5: (20, 3, 2), 6: (20, 3, 18), 7: (30, 3, 5), 8: (30, 3, 6),
             9: (60, 3, 4), 10: (60, 3, 13), 11: (60, 3, 6), 12: (60, 3, 11), 13: (60, 3, 14), 14: (60, 5, 18),
             15: (100, 3, 7), 16: (100, 3, 13), 17: (100, 3, 15), 18: (100, 3, 22)},
}


def _diagonal(scenes):
    return scenes.diagonal_camera(2.0 ** -10, 2.0 ** 45)


def _shifted(rt, tree, offset=96):
    """the same tree with its node array `offset` bytes (a multiple of the 32-byte slot, not of a 64-byte pair) into a larger
    device allocation"""
    import torch
    leaves, nodes, root, count, g = tree
    raw = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    big = torch.zeros(offset + raw.size + 4096, dtype=torch.uint8, device="cuda")
    big[offset:offset + raw.size] = torch.from_numpy(raw.copy()).to("cuda")

    class Shifted:
        nodes_out = big[offset:]
        triangles_out = g["inp"].triangles_out
    assert Shifted.nodes_out.data_ptr() % 64 == 32
    return leaves, nodes, root, count, dict(inp=Shifted)


@gpu
@pytest.mark.parametrize("shift", [False, True])
def test_crossing_the_margin_both_ways(rt, scenes, ora, shift):
    tree = _tree(rt, ora, scenes.fractal_corner(4000, 3), "lbvh")
    if shift:
        tree = _shifted(rt, tree)
    cam = _diagonal(scenes)
    for (w, h) in ((33, 25), (96, 64)):
        for render_type in (0, 1, 2):
            _, oc = _check(ora, tree, cam, w, h, "fractal lbvh", render_type)
            assert oc[2] >= 24 and oc[3] == 0, f"oracle max stack {oc[2]}: the scene must pass the margin and the LDS column"
            _check(ora, tree, cam, w, h, "fractal lbvh 4 spp", render_type, spp=4)
        for rows in ((3, 21), (0, 9), (h - 5, h)):                       # bands that split a tile row
            _check(ora, tree, cam, w, h, f"fractal lbvh rows {rows}", 1, rows=rows)
        _check(ora, tree, cam, w, h, "fractal lbvh 4 spp rows", 2, spp=4, rows=(3, 21))


@gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_stack_depth_around_the_switch(rt, scenes, ora, kind, depth):
    n, seed, octaves = DEPTH_SCENES[kind][depth]
    tree = _tree(rt, ora, scenes.fractal_corner(n, seed, octaves=octaves), kind)
    assert tree[3] >= 2, "entered through a root pair or run: the instantiation with the rule"
    cam = _diagonal(scenes)
    for t in (tree, _shifted(rt, tree)):
        for render_type in (0, 1, 2):
            _, oc = _check(ora, t, cam, 33, 25, f"depth {depth} {kind}", render_type)
            assert oc[2] == depth and oc[3] == 0, f"oracle max stack {oc[2]}, dropped {oc[3]}: the scene must peak at {depth}"
    _check(ora, tree, cam, 33, 25, f"depth {depth} {kind} 4 spp rows", 1, spp=4, rows=(3, 21))


@gpu
@pytest.mark.parametrize("width", [2, 3, 4, 7])
def test_full_stack_on_the_hold_arm(rt, scenes, ora, width):
    """The 140-octave scene fills the 64 entries and drops pushes; re-packed, the tree is entered through a root run."""
    tree = _tree(rt, ora, scenes.fractal_corner(8000, 3, octaves=140, top_exp=42), f"sah{width}")
    assert tree[3] >= 2
    cam = _diagonal(scenes)
    for t in (tree, _shifted(rt, tree)):
        for render_type in (0, 1, 2):
            _, oc = _check(ora, t, cam, 33, 25, f"140 octaves, {width} slots", render_type)
            assert oc[2] == 64 and oc[3] > 0, oc


@gpu
@pytest.mark.parametrize("scene", ["one", "two", "coincident"])
def test_tiny_trees_take_the_lean_arm_alone(rt, scenes, ora, scene):
    cam = scenes.make_camera((0.0, 10.0, 0.0), 0.0, 1.5, 40.0)
    tris = _coincident(37) if scene == "coincident" else (_coincident(2)[:1] if scene == "one" else _coincident(2))
    tree = _tree(rt, ora, tris, "lbvh")
    for t in (tree, _shifted(rt, tree)):
        for (w, h) in ((64, 64), (67, 45)):
            for render_type in (0, 1, 2):
                _, oc = _check(ora, t, cam, w, h, f"{scene} lbvh", render_type)
                # (the kernel's deepest sp is oc[2] - 1: never past the lean threshold)
                assert oc[1] > 0 and int(oc[2]) - 1 <= (0 if scene != "coincident" else K_STACK_LDS - K_LEAN_MARGIN), oc
            _check(ora, t, cam, w, h, f"{scene} lbvh 4 spp rows", 1, spp=4, rows=(3, 29))
