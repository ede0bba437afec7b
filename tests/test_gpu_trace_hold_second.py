"""Hold by stack depth alone (csrc/rt_traverse.hpp quad_hold_sp; RT_TRACE_HOLD_SECOND / RT_TRACE_HOLD_FIRST): a lane that has
just popped an entry from level s < 16 of its stack sits a box step out while an unfinished quad-mate's stack is deeper than
s -- before the second step of a vote, before the first, or both, as the library was built.  No stack entry is compared, so
the rule also holds lanes whose mate is somewhere else entirely; what it may change is the interleaving across lanes and
nothing else.  Every comparison is exact: frame bytes and sum(box tests) / sum(triangle tests) against the oracle.  The cases
hold for every value of the two knobs; they run against the shipped library.

* grid_mesh(G), G = 8 / 24 / 48, top-down camera, 64 x 64 and 67 x 45 (partial tiles: quads with finished lanes, whose key is
  0 and for whom nobody holds), through the LBVH, the SAH tree re-packed to 3, 4 and 7 slots (they take the rule, and their
  votes are general ones) and the SAH tree as built (the other arm of launch_trace's dispatch); render types 0 - 2, 4 spp, a
  row band that splits a tile row, interleaved strips;
* the deep-stack scenes of stack_scenes.py: more than 16 levels (a lane popped from a private level is never held, though
  its mates' sp are greater all the time) and a full 64-entry stack with dropped pushes (pops stay LIFO: a hold ends);
* one- and two-triangle trees, coincident and zero-area triangles: every mate has the same sp, nobody may hold, nothing hangs;
* seven frames with counters on seven streams.

A wrong rule is a hang, not a wrong pixel, so the progress argument is executed without a GPU: the schedule model
(tools/quad_wait_model.py) runs every --first / --second combination over tiles of G = 24 and G = 48; run_wave raises on a pass
of the loop that steps no lane and frees none, and each ray's sequence of tests must be the lock-step one."""
import numpy as np
import pytest

import stack_scenes as sc
from test_gpu_trace_pair_step import _mixed
from test_gpu_trace_quad_wait import _check, _coincident, _model, _tree
import edge_scenes

gpu = pytest.mark.gpu
SIZES = ((64, 64), (67, 45))
FIRST, SECOND = ("entry", "sp"), ("none", "entry", "sp")


@gpu
@pytest.mark.parametrize("kind", ["lbvh", "sah3", "sah4", "sah7", "sah"])
@pytest.mark.parametrize("G", [8, 24, 48])
def test_grid_under_the_top_down_camera(rt, scenes, ora, G, kind):
    import torch
    tree = _tree(rt, ora, scenes.grid_mesh(G, 1), kind)
    leaves, nodes, root, count, g = tree
    cam = scenes.camera_a(G)
    what = f"grid {G} {kind}"
    for (w, h) in SIZES:
        for render_type in (0, 1, 2):
            full, oc = _check(ora, tree, cam, w, h, what, render_type)
        assert oc[1] > 0, "the frame hits the mesh"
        _check(ora, tree, cam, w, h, f"{what} rows 3..29", 1, rows=(3, 29))     # a band that splits a tile row
        _check(ora, tree, cam, w, h, f"{what} 4 spp", 0, spp=4)
    # interleaved strips, stored compactly (67 x 45: the last strip is partial)
    w, h = SIZES[1]
    full, _ = ora.trace(leaves, nodes, root, count, cam, w, h, render_type=0)
    strip_rows, first, stride = 8, 1, 2
    strips = range(first, (h + strip_rows - 1) // strip_rows, stride)
    compact = torch.zeros(len(strips) * strip_rows * w * 4, dtype=torch.uint8, device="cuda")
    rt.Trace(g["inp"].triangles_out, g["inp"].nodes_out, compact, (w, h), rt.to_device(cam), root, count,
             strips=(strip_rows, first, stride))
    torch.cuda.synchronize()
    got = compact.cpu().numpy().reshape(len(strips) * strip_rows, w, 4)
    for j, st in enumerate(strips):
        n = min(strip_rows, h - st * strip_rows)
        assert (got[j * strip_rows: j * strip_rows + n] == full[st * strip_rows: st * strip_rows + n]).all(), f"{what} strip {st}"


@gpu
@pytest.mark.parametrize("kind,min_depth", [("lbvh", 24), ("sah3", 40), ("sah", 40)])
def test_a_lane_popped_from_a_private_level_is_never_held(rt, scenes, ora, kind, min_depth):
    """Stacks of more than 16 levels: the mates of a lane that pops at level 16 or above are deeper most of the time."""
    tris, cam = sc.fractal("deep", scenes)
    tree = _tree(rt, ora, tris, kind)
    for render_type in (0, 1, 2):
        _, oc = _check(ora, tree, cam, *sc.FRAME, f"deep fractal {kind}", render_type)
        assert oc[2] >= min_depth > sc.LDS_LEVELS and oc[3] == 0, f"oracle max_stack {oc[2]}, dropped {oc[3]}"


@gpu
@pytest.mark.parametrize("kind", ["mixed", "sah"])
def test_full_stack_with_dropped_pushes(rt, scenes, ora, kind):
    tris, cam = sc.fractal("full", scenes)
    tree = _mixed(rt, ora, tris, base="sah") if kind == "mixed" else _tree(rt, ora, tris, "sah")
    for render_type in (0, 1, 2):
        _, oc = _check(ora, tree, cam, *sc.FRAME, f"full stack {kind}", render_type)
        assert oc[2] == sc.STACK and oc[3] > 0, oc


@gpu
@pytest.mark.parametrize("kind", ["lbvh", "sah4", "sah"])
@pytest.mark.parametrize("scene", ["one", "two", "coincident", "zero-area"])
def test_equal_depths_nobody_holds(rt, scenes, ora, scene, kind):
    cam = scenes.make_camera((0.0, 10.0, 0.0), 0.0, 1.5, 40.0)
    if scene == "zero-area":
        tris, cam = edge_scenes.signed_zero_mesh(scenes), scenes.make_camera((0.0, 6.0, 0.0), 0.3, 1.2, 60.0)
    elif scene == "coincident":
        tris = _coincident(37)
    else:
        tris = _coincident(2)[:1] if scene == "one" else _coincident(2)
    tree = _tree(rt, ora, tris, kind)
    for (w, h) in SIZES:
        for render_type in (0, 1, 2):
            _, oc = _check(ora, tree, cam, w, h, f"{scene} {kind}", render_type)
        assert oc[1] > 0
    _check(ora, tree, cam, 67, 45, f"{scene} {kind} 4 spp rows", 1, spp=4, rows=(3, 29))


@gpu
def test_counters_of_seven_concurrent_streams(rt, scenes, ora):
    import torch
    G = 48
    tris = scenes.grid_mesh(G, 1)
    trees = [_tree(rt, ora, tris, k) for k in ("lbvh", "sah4", "sah")]
    jobs = []
    for i in range(7):
        tree = trees[i % 3]
        w, h = 64 + 9 * i, 45 + 7 * i
        cam = scenes.camera_a(G) if i % 3 else scenes.camera_b(G)
        jobs.append((tree, w, h, cam, torch.cuda.Stream(), torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda"),
                     torch.zeros(4, dtype=torch.int64, device="cuda"), rt.to_device(cam)))
    torch.cuda.synchronize()
    for _ in range(2):
        for (tree, w, h, cam, st, rgba, ctr, cam_d) in jobs:
            g = tree[4]["inp"]
            with torch.cuda.stream(st):
                rt.Trace(g.triangles_out, g.nodes_out, rgba, (w, h), cam_d, tree[2], tree[3], counters=ctr, stream=st)
    torch.cuda.synchronize()
    for i, (tree, w, h, cam, st, rgba, ctr, cam_d) in enumerate(jobs):
        oi, oc = ora.trace(tree[0], tree[1], tree[2], tree[3], cam, w, h, render_type=0)
        gc = ctr.cpu().numpy().astype(np.uint64)[:2]
        assert (gc == 2 * oc[:2]).all(), f"stream {i}: counters {gc} vs 2 x {oc[:2]}"
        assert (rgba.cpu().numpy().reshape(h, w, 4) == oi).all(), f"stream {i}: frame differs"


# ---------------------------------------------------------------- CPU: the rule and its progress argument on the schedule model
class _Lane:
    def __init__(self, m, sp, phase=None, popped=False):
        self.sp, self.phase, self.popped = sp, m.STEP if phase is None else phase, popped


def test_model_rule_is_the_stack_depths_alone():
    m = _model()
    quad = [_Lane(m, 3, popped=True), _Lane(m, 3), _Lane(m, 3, m.LEAF0), _Lane(m, 9, m.DONE)]
    assert not any(m.holds_sp(quad, k) for k in range(4)), "equal depths, and a finished mate counts for nothing"
    quad = [_Lane(m, 3, popped=True), _Lane(m, 4, popped=True), _Lane(m, 2, popped=True), _Lane(m, 4, m.LEAF1)]
    assert [m.holds_sp(quad, k) for k in range(4)] == [True, False, True, False], "the deepest never hold; a parked mate counts"
    quad = [_Lane(m, 3), _Lane(m, 5), _Lane(m, 0, m.DONE), _Lane(m, 0, m.DONE)]
    assert not m.holds_sp(quad, 0), "only a freshly popped lane holds"
    quad = [_Lane(m, m.STACK_LDS, popped=True), _Lane(m, m.STACK_LDS - 1, popped=True), _Lane(m, 40), _Lane(m, 40)]
    assert [m.holds_sp(quad, k) for k in range(2)] == [False, True], "a lane popped from a private level is never held"


@pytest.mark.parametrize("second", SECOND)
@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("G", [24, 48])
def test_model_every_pass_steps_a_lane_and_each_ray_keeps_its_sequence(scenes, ora, G, first, second):
    """Four tiles of the 67 x 45 frame, two of them partial, under the kernel's schedule with the exact vote.  run_wave raises on
    a pass that neither steps a lane nor runs a leaf phase and on a wave that ends with an unfinished lane."""
    m = _model()
    tree = m.load_tree(ora, scenes.grid_mesh(G, 1), "lbvh")
    cam = scenes.camera_a(G)
    w, h = SIZES[1]
    held = 0
    for (tx, ty) in ((0, 0), (4, 2), (8, 0), (8, 5)):
        base = m.tile_rays(tree, cam, w, h, tx, ty)
        m.run_wave(base, hold=False)
        rays = m.tile_rays(tree, cam, w, h, tx, ty)
        res = m.run_wave(rays, hold=True, second=second, pair=3, first=first)
        for a, b in zip(base, rays):
            assert a.visits == b.visits and a.pushes == b.pushes, f"tile {tx},{ty}: a ray's sequence differs from the lock-step one"
            assert a.tmax == b.tmax and a.box_tests == b.box_tests and a.tri_tests == b.tri_tests and a.hit == b.hit
        assert res["nbox"] > 0 and res["box_instr"] <= res["nbox"]
        held += res["held2"]
    assert (held > 0) == (second != "none"), f"lanes held before a second step: {held}"
