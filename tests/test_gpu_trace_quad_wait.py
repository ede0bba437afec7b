"""Hold at pop (csrc/rt_traverse.hpp quad_hold; on in trace_kernel's instantiations named in trace_kernel.hip): a lane that has
just popped entry E from level s of its stack sits box steps out while a quad-mate still holds E at level s of its own, so
that the two step on E together.  Only the interleaving across lanes may change: every comparison here is exact -- frame
bytes and sum(box tests) / sum(triangle tests) against the oracle.

* grid_mesh(G), G = 8 / 24 / 48, under the top-down camera -- the smallest scenes on which quad-mates part (one enters a box
  its neighbour misses) and meet again at a pop -- through the LBVH, the SAH tree and the SAH tree re-packed to nodes of 3, 4
  and 7 slots; 64 x 64 and 67 x 45 (partial tiles: quads with lanes outside the frame); render types 0 - 2; whole frames, row
  bands that split a tile row, 4 spp, interleaved strips;
* stacks deeper than the 16 LDS levels (the rule never looks at a private level) and a full stack (a dropped push leaves
  nobody holding for an entry that is never popped);
* kDiffuse, kTextureLit and kTextureLitShadows on the textured scene.  The shipped library builds the shaded instantiations
  WITHOUT the rule (RT_TRACE_QUAD_WAIT = 1: render types 0 - 2 only), so against it this test runs unchanged kernels; it is
  here for a library built with -DRT_TRACE_QUAD_WAIT=2, where the shadow traversal starts with part of each quad finished;
* seven frames with counters on seven streams;
* one- and two-triangle trees, zero-area triangles and coincident triangles: every mate holds the same entry at the same level.

launch_trace takes the instantiation with the rule for trees entered through a root pair or a wider root run (here: the
LBVH and the re-packed SAH trees) and the plain one for a single root slot (the SAH tree as built): the sah cases are the
same scenes through the other arm of that dispatch.

The CPU test at the end executes the progress argument on the committed model (tools/quad_wait_model.py)."""
import importlib.util
import os

import numpy as np
import pytest

import edge_scenes
import texture_scene

gpu = pytest.mark.gpu
SIZES = ((64, 64), (67, 45))


class _Tree:
    """device buffers of a tree in the reference layout, as helpers.gpu_trace takes them"""
    def __init__(self, rt, nodes, leaves):
        self.nodes_out = rt.to_device(np.ascontiguousarray(nodes))
        self.triangles_out = rt.to_device(np.ascontiguousarray(leaves))


def _tree(rt, ora, tris, kind):
    """(oracle leaves, nodes, root, count, device tree); kind: lbvh | sah | sah3 | sah4 | sah7 (SAH re-packed to that width)"""
    if kind == "lbvh":
        b = ora.build_bvh(tris)
        leaves, nodes, root, count = b["leaves"], b["nodes"], 0, 2
    else:
        s = ora.build_sah(tris)
        leaves, nodes, root, count = s["leaves"], s["nodes"], 0, 1
        if kind != "sah":
            nodes, root, count = edge_scenes.collapse_wide(nodes, 0, 1, int(kind[3:]), rt.NODE)
    return leaves, nodes, root, count, dict(inp=_Tree(rt, nodes, leaves))


def _check(ora, tree, cam, w, h, what, render_type=0, **kw):
    from helpers import gpu_trace
    leaves, nodes, root, count, g = tree
    oi, oc = ora.trace(leaves, nodes, root, count, cam, w, h, render_type=render_type, **kw)
    gi, gc = gpu_trace(g, cam, w, h, render_type, root=root, count=count, **kw)
    r0, r1 = kw.get("rows") or (0, h)
    assert (gc == oc[:2]).all(), f"{what} {w}x{h} render {render_type}: counters {gc} vs {oc[:2]}"
    bad = (gi[r0:r1] != oi[r0:r1]).any(axis=2).sum()
    assert bad == 0, f"{what} {w}x{h} render {render_type}: {bad} pixels differ"
    return oi, oc


@gpu
@pytest.mark.parametrize("kind", ["lbvh", "sah", "sah3", "sah4", "sah7"])
@pytest.mark.parametrize("G", [8, 24, 48])
def test_grid_under_the_top_down_camera(rt, scenes, ora, G, kind):
    import torch
    tree = _tree(rt, ora, scenes.grid_mesh(G, 1), kind)
    cam = scenes.camera_a(G)
    what = f"grid {G} {kind}"
    for (w, h) in SIZES:
        for render_type in (0, 1, 2):
            oi, oc = _check(ora, tree, cam, w, h, what, render_type)
        assert oc[1] > 0, "the frame hits the mesh"
        for rows in ((3, 29), (0, 9), (h - 5, h)):                       # bands that split a tile row
            _check(ora, tree, cam, w, h, f"{what} rows {rows}", 1, rows=rows)
        _check(ora, tree, cam, w, h, f"{what} 4 spp", 0, spp=4)
        _check(ora, tree, cam, w, h, f"{what} 4 spp", 2, spp=4, rows=(3, 29))
        # interleaved strips, stored compactly
        leaves, nodes, root, count, g = tree
        full, _ = ora.trace(leaves, nodes, root, count, cam, w, h, render_type=0)
        for (strip_rows, first, stride) in ((8, 1, 2), (16, 0, 3)):
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
@pytest.mark.parametrize("kind,min_depth", [("lbvh", 24), ("sah", 40)])
def test_stack_deeper_than_the_lds_levels(rt, scenes, ora, kind, min_depth):
    """Entries from level 16 up live in private memory: never looked at, never held for."""
    tree = _tree(rt, ora, scenes.fractal_corner(4000, 3), kind)
    cam = scenes.diagonal_camera(2.0 ** -10, 2.0 ** 45)
    for (w, h) in ((33, 25), (96, 64)):
        for render_type in (0, 1, 2):
            _, oc = _check(ora, tree, cam, w, h, f"fractal {kind}", render_type)
            assert oc[2] >= min_depth and oc[3] == 0, f"oracle max_stack {oc[2]}: the scene must overflow the 16 LDS entries"


@gpu
def test_full_stack_drops_pushes(rt, scenes, ora):
    tree = _tree(rt, ora, scenes.fractal_corner(8000, 3, octaves=140, top_exp=42), "sah")
    cam = scenes.diagonal_camera(2.0 ** -10, 2.0 ** 45)
    for render_type in (0, 1, 2):
        _, oc = _check(ora, tree, cam, 33, 25, "140 octaves", render_type)
        assert oc[2] == 64 and oc[3] > 0, oc


@gpu
@pytest.mark.parametrize("cam", ["top", "oblique"])
def test_shaded_and_shadowed_frames(rt, scenes, ora, cam):
    """kDiffuse, kTextureLit, kTextureLitShadows.  With -DRT_TRACE_QUAD_WAIT=2 the second traversal holds with the lanes that
    missed already finished; the shipped library (level 1) compiles these render types without the rule."""
    sc = texture_scene.make(scenes, ora)
    tree = _tree(rt, ora, sc["tris"], "lbvh")
    kw = dict(attributes=sc["attributes"], materials=sc["materials"], light=sc["light"])
    _check(ora, tree, sc["cameras"][cam], 160, 100, "kDiffuse", 5, **kw)
    lit, _ = _check(ora, tree, sc["cameras"][cam], 160, 100, "kTextureLit", 7, textures=sc["textures"], **kw)
    sh, _ = _check(ora, tree, sc["cameras"][cam], 160, 100, "kTextureLitShadows", 8, textures=sc["textures"], **kw)
    assert (sh != lit).any(axis=-1).mean() > 0.01, "some pixels are shadowed"


@gpu
def test_counters_of_seven_concurrent_streams(rt, scenes, ora):
    import torch
    G = 48
    tris = scenes.grid_mesh(G, 1)
    trees = [_tree(rt, ora, tris, k) for k in ("lbvh", "sah")]
    jobs = []
    for i in range(7):
        tree = trees[i % 2]
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


def _coincident(n):
    """n copies of one triangle (coincident boxes at every level of any tree) beside one that differs"""
    t = np.tile(np.array([[-4.0, 0.0, -4.0, 4.0, 0.0, -4.0, 0.0, 0.5, 4.0]], np.float32), (n, 1))
    t[-1] = (-4.0, 0.2, -4.0, 4.0, 0.2, -4.0, 0.0, 0.3, 5.0)
    return t


@gpu
@pytest.mark.parametrize("kind", ["lbvh", "sah"])
@pytest.mark.parametrize("scene", ["one", "two", "coincident", "signed-zero"])
def test_tiny_and_degenerate_trees(rt, scenes, ora, scene, kind):
    """Identical entries: every ray of a quad holds the same entry at the same level, nobody is deeper, nobody holds."""
    cam = scenes.make_camera((0.0, 10.0, 0.0), 0.0, 1.5, 40.0)
    if scene == "signed-zero":
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
        _check(ora, tree, cam, w, h, f"{scene} {kind} 4 spp rows", 1, spp=4, rows=(3, 29))


# ---------------------------------------------------------------- CPU: the progress argument, executed on the model
def _model():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "quad_wait_model.py")
    spec = importlib.util.spec_from_file_location("quad_wait_model", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("scene", ["grid16", "signed-zero-20", "signed-zero-9"])
@pytest.mark.parametrize("kind", ["lbvh", "sah"])
def test_model_hold_rule_always_steps_a_lane_and_keeps_each_rays_sequence(scenes, ora, scene, kind):
    """About 200 quads per scene (partial quads at the frame's edge included): under the hold rule every round of an
    unfinished quad, and every pass of an unfinished wave's loop, steps a lane or frees a parked one (run_quad / run_wave
    raise otherwise), and each ray's own sequence of tests is its lock-step sequence."""
    m = _model()
    if scene == "grid16":
        tris, cam = scenes.grid_mesh(16, 1), scenes.camera_a(16)
    else:
        tris = edge_scenes.signed_zero_mesh(scenes, G=int(scene.split("-")[-1]), seed=6 if scene.endswith("20") else 11)
        cam = scenes.make_camera((0.0, 6.0, 0.0), 0.3, 1.2, 60.0)
    tree = m.load_tree(ora, tris, kind)
    w, h = 31, 25                                       # odd: the last column and row of quads are partial
    quads = [(qx, qy) for qy in range((h + 1) // 2) for qx in range((w + 1) // 2)]
    assert 190 <= len(quads) <= 220
    held_rounds = steps = 0
    for (qx, qy) in quads:
        base = m.quad_rays(tree, cam, w, h, qx, qy)
        m.run_quad(base, hold=False)
        rays = m.quad_rays(tree, cam, w, h, qx, qy)
        res = m.run_quad(rays, hold=True)               # raises if a round steps nobody
        for a, b in zip(base, rays):
            assert a.visits == b.visits and a.tmax == b.tmax and a.box_tests == b.box_tests and a.tri_tests == b.tri_tests
            steps += len(a.visits)
        held_rounds += res["rounds"]
    assert steps > 0 and held_rounds > 0
    # the kernel's schedule (parking, two steps per vote) over whole tiles
    for (tx, ty) in ((0, 0), (1, 1), (3, 3), (3, 0)):
        base = m.tile_rays(tree, cam, w, h, tx, ty)
        m.run_wave(base, hold=False)
        for second in (False, True):                    # the rule before the first step of a vote / before both
            rays = m.tile_rays(tree, cam, w, h, tx, ty)
            m.run_wave(rays, hold=True, second=second)
            for a, b in zip(base, rays):
                assert a.visits == b.visits and a.tmax == b.tmax
