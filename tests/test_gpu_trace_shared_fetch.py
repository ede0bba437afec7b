"""GPU parity on the two fetch paths of the tracer's hot loop (csrc/rt_traverse.hpp), on the frames that stress them:

* the box phase reads a node pair as four 16-byte requests per lane, a lone slot twice;
* the leaf phase reads a leaf as four 16-byte requests issued together (all sixteen dwords, the unused ones included).

(The cases were written when the loop also carried an arm that read a pair shared by a whole wave once, through the scalar
path; that arm is retired, DESIGN section 5, and the cases remain as parity cases of the plain and leaf fetch paths.)

Neither may change a ray's own sequence of tests, so every comparison here is exact: frame bytes and sum(box tests) /
sum(triangle tests) against the oracle, through the public rt.Trace / rt.IntersectRays.

* frames whose rays all share one path: one large triangle, 1- and 2-triangle trees, root count 1 (SAH) and 2 (LBVH);
* a SAH tree re-packed into nodes of more than two slots (steps through advance()'s count > 2 branch and the lone slot);
* a top-down frame (shared upper tree, then divergence) as a whole, in row bands, at 4 spp and in interleaved strips;
* any-hit queries (a lane leaves the traversal at its first hit while its neighbours go on);
* the counters of 7 frames traced concurrently on 7 streams."""
import numpy as np
import pytest

import edge_scenes

pytestmark = pytest.mark.gpu


class _Tree:
    """device buffers of a tree in the reference layout, as helpers.gpu_trace takes them"""
    def __init__(self, rt, nodes, leaves):
        self.nodes_out = rt.to_device(np.ascontiguousarray(nodes))
        self.triangles_out = rt.to_device(np.ascontiguousarray(leaves))


def _trees(rt, ora, tris):
    """{name: (oracle leaves, oracle nodes, root, count, device tree)}: the LBVH (root count 2) and the SAH tree (root count 1)"""
    b, s = ora.build_bvh(tris), ora.build_sah(tris)
    return {"lbvh": (b["leaves"], b["nodes"], 0, 2, dict(inp=_Tree(rt, b["nodes"], b["leaves"]))),
            "sah": (s["leaves"], s["nodes"], 0, 1, dict(inp=_Tree(rt, s["nodes"], s["leaves"])))}


def _check_frames(ora, tree, cam, sizes, what, render_types=(0, 1, 2), **kw):
    from helpers import gpu_trace
    leaves, nodes, root, count, g = tree
    for (w, h) in sizes:
        for render_type in render_types:
            oi, oc = ora.trace(leaves, nodes, root, count, cam, w, h, render_type=render_type, **kw)
            gi, gc = gpu_trace(g, cam, w, h, render_type, root=root, count=count, **kw)
            rows = kw.get("rows") or (0, h)
            assert (gc == oc[:2]).all(), f"{what} {w}x{h} render {render_type}: counters {gc} vs {oc[:2]}"
            bad = (gi[rows[0]:rows[1]] != oi[rows[0]:rows[1]]).any(axis=2).sum()
            assert bad == 0, f"{what} {w}x{h} render {render_type}: {bad} pixels differ"
    return oi, oc


def _big_triangles(n):
    """n = 1: one triangle that covers the whole view of _above(); n = 2: a quad of two"""
    a, b, c, d = (-50.0, 0.0, -50.0), (50.0, 0.0, -50.0), (-50.0, 0.5, 50.0), (50.0, 0.25, 50.0)
    t = [(-200.0, 0.0, -100.0) + (200.0, 0.0, -100.0) + (0.0, 1.0, 300.0)] if n == 1 else [a + b + c, b + d + c]
    return np.array(t, np.float32)


def _above(scenes, x, z, height, depth):
    return scenes.make_camera((x, height, z), 0.0, 1.5, depth)   # looking (almost) straight down, as the bench's camera A


@pytest.mark.parametrize("tree", ["lbvh", "sah"])
@pytest.mark.parametrize("ntris", [1, 2])
def test_every_ray_shares_one_path(rt, scenes, ora, tree, ntris):
    """Every vote of every wave is a shared one: all 64 lanes step root -> leaf together (and park together)."""
    tris = _big_triangles(ntris)
    cam = _above(scenes, 0.0, 0.0, 10.0, 40.0)
    oi, oc = _check_frames(ora, _trees(rt, ora, tris)[tree], cam, ((64, 64), (67, 45)), f"{ntris} triangle(s) {tree}")
    assert oc[1] >= 67 * 45, "every ray reaches a leaf"
    oi, _ = ora.trace(*_trees(rt, ora, tris)[tree][:4], cam, 67, 45, render_type=0)
    assert (oi[..., 0] > 0).all(), "the triangles cover the frame"


@pytest.mark.parametrize("width", [3, 4, 7])
def test_sah_tree_with_nodes_wider_than_a_pair(rt, scenes, ora, width):
    """A SAH tree re-packed into nodes of up to `width` slots under a top-down camera: the steps at the top of the
    tree, which all rays of a tile share, walk such nodes two slots at a time (cur advances inside the node, identically in
    every lane) and end in a lone slot for odd counts."""
    G = 24
    tris = scenes.grid_mesh(G, 3)
    s = ora.build_sah(tris)
    nodes, root, count = edge_scenes.collapse_wide(s["nodes"], 0, 1, width, rt.NODE)
    assert ((nodes["w12"] >> 29) > 2).any(), "the re-packed tree has nodes of more than two slots"
    tree = (s["leaves"], nodes, root, count, dict(inp=_Tree(rt, nodes, s["leaves"])))
    for cam in (_above(scenes, G / 2, G / 2, 0.45 * G, 1.5 * G), scenes.camera_b(G)):
        _check_frames(ora, tree, cam, ((160, 100),), f"SAH width {width}")


@pytest.fixture(scope="module")
def grid(rt, scenes, ora):
    G = 64
    tris = scenes.grid_mesh(G, 1)
    return dict(G=G, tris=tris, trees=_trees(rt, ora, tris), cam=scenes.camera_a(G))


@pytest.mark.parametrize("tree", ["lbvh", "sah"])
def test_shared_then_divergent_frame_bands_and_spp(grid, ora, tree):
    """The bench's view in small: the rays of a tile share the upper tree and part below it.  Whole frame, row bands that cut
    tiles (inactive lanes vote too) and 4 spp (one traversal per sample, each starting shared again)."""
    t = grid["trees"][tree]
    _check_frames(ora, t, grid["cam"], ((200, 120), (131, 77)), tree)
    for rows in ((13, 50), (0, 9), (70, 77)):
        _check_frames(ora, t, grid["cam"], ((131, 77),), f"{tree} rows {rows}", render_types=(0, 1), rows=rows)
    _check_frames(ora, t, grid["cam"], ((131, 77),), f"{tree} 4 spp", render_types=(0,), spp=4)
    _check_frames(ora, t, grid["cam"], ((131, 77),), f"{tree} 4 spp rows", render_types=(0,), spp=4, rows=(13, 50))


@pytest.mark.parametrize("strip_rows,first,stride", [(8, 0, 3), (8, 2, 3), (16, 1, 2)])
def test_shared_then_divergent_frame_in_strips(rt, grid, ora, strip_rows, first, stride):
    """Interleaved strips (the multi-GPU partition's compact output) of the same view."""
    import torch
    leaves, nodes, root, count, g = grid["trees"]["lbvh"]
    w, h = 130, 101
    full, _ = ora.trace(leaves, nodes, root, count, grid["cam"], w, h, render_type=0)
    strips = range(first, (h + strip_rows - 1) // strip_rows, stride)
    compact = torch.zeros(len(strips) * strip_rows * w * 4, dtype=torch.uint8, device="cuda")
    rt.Trace(g["inp"].triangles_out, g["inp"].nodes_out, compact, (w, h), rt.to_device(grid["cam"]), root, count,
             strips=(strip_rows, first, stride))
    torch.cuda.synchronize()
    got = compact.cpu().numpy().reshape(len(strips) * strip_rows, w, 4)
    for j, st in enumerate(strips):
        rows_in = min(strip_rows, h - st * strip_rows)
        assert (got[j * strip_rows: j * strip_rows + rows_in] == full[st * strip_rows: st * strip_rows + rows_in]).all(), f"strip {st}"


def _camera_queries(rt, g, root, count, cam, w, h, any_hit):
    """the frame's primary rays (8x8-tiled: wave = tile, as in Trace) through IntersectRays -> (HIT records, counters[:2])"""
    import torch
    n = rt.CameraRayCount(w, h, 1, True)
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(rt.to_device(cam), w, h, rays, spp=1, tiled=True)
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    rt.IntersectRays(g["inp"].triangles_out, g["inp"].nodes_out, root, count, rays, hits, any_hit=any_hit, counters=ctr)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(rt.HIT).reshape(-1), ctr.cpu().numpy().astype(np.uint64)[:2]


@pytest.mark.parametrize("tree", ["lbvh", "sah"])
def test_any_hit_queries(rt, scenes, grid, ora, tree):
    """Any-hit rays walk the closest-hit sequence up to their first hit.  So: (a) closest-hit camera rays do exactly the
    oracle's tests; (b) any-hit hits exactly the rays the oracle's frame hits, with no more tests; (c) where no ray hits
    anything, and on a one-triangle tree (one test per ray either way), any-hit's counters ARE the oracle's."""
    leaves, nodes, root, count, g = grid["trees"][tree]
    w, h = 128, 72                                   # whole tiles: no off-frame lanes in the tiled ray buffer
    oi, oc = ora.trace(leaves, nodes, root, count, grid["cam"], w, h, render_type=0)
    c, cc = _camera_queries(rt, g, root, count, grid["cam"], w, h, False)
    a, ac = _camera_queries(rt, g, root, count, grid["cam"], w, h, True)
    assert (cc == oc[:2]).all(), f"closest-hit counters {cc} vs oracle {oc[:2]}"
    assert ((c["primitive_id"] != rt.MISS) == (a["primitive_id"] != rt.MISS)).all()
    k = np.arange(w * h)                              # ray k = tile * 64 + lane, lane = Morton position inside the 8x8 tile
    lane, tile = k & 63, k >> 6
    x = (tile % (w // 8)) * 8 + ((lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4))
    y = (tile // (w // 8)) * 8 + (((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4))
    hit = a["primitive_id"] != rt.MISS
    assert (hit == (oi[y, x, 0] > 0)).all(), "any-hit hits exactly the pixels the oracle's depth frame hits"
    assert hit.sum() > 0.9 * w * h
    assert ac[0] <= cc[0] and ac[1] <= cc[1] and ac[1] >= hit.sum()
    assert (a["t"] >= c["t"]).all()
    # (c) no hits: a camera under the height field looking down
    away = scenes.make_camera((grid["G"] / 2, -5.0, grid["G"] / 2), 0.0, 1.5, 100.0)
    oi, oc = ora.trace(leaves, nodes, root, count, away, w, h, render_type=0)
    assert not oi[..., :3].any()
    a, ac = _camera_queries(rt, g, root, count, away, w, h, True)
    assert (a["primitive_id"] == rt.MISS).all() and (ac == oc[:2]).all(), f"any-hit, all misses: {ac} vs oracle {oc[:2]}"
    one = _trees(rt, ora, _big_triangles(1))[tree]
    cam = _above(scenes, 0.0, 0.0, 10.0, 40.0)
    oi, oc = ora.trace(*one[:4], cam, w, h, render_type=0)
    a, ac = _camera_queries(rt, one[4], one[2], one[3], cam, w, h, True)
    assert (a["primitive_id"] == 0).all() and (ac == oc[:2]).all(), f"any-hit, one triangle: {ac} vs oracle {oc[:2]}"


def test_counters_of_seven_concurrent_streams(rt, scenes, grid, ora):
    """Seven frames of different sizes and trees in flight on seven streams, each with its own counters and frame buffer."""
    import torch
    jobs = []
    for i in range(7):
        tree = grid["trees"]["lbvh" if i % 2 == 0 else "sah"]
        w, h = 96 + 16 * i, 64 + 7 * i
        cam = grid["cam"] if i % 3 else scenes.camera_b(grid["G"])
        jobs.append((tree, w, h, cam, torch.cuda.Stream(), torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda"),
                     torch.zeros(4, dtype=torch.int64, device="cuda"), rt.to_device(cam)))
    torch.cuda.synchronize()
    for _ in range(3):                                # three rounds: the counters accumulate
        for (tree, w, h, cam, st, rgba, ctr, cam_d) in jobs:
            g = tree[4]["inp"]
            with torch.cuda.stream(st):
                rt.Trace(g.triangles_out, g.nodes_out, rgba, (w, h), cam_d, tree[2], tree[3], counters=ctr, stream=st)
    torch.cuda.synchronize()
    for i, (tree, w, h, cam, st, rgba, ctr, cam_d) in enumerate(jobs):
        oi, oc = ora.trace(tree[0], tree[1], tree[2], tree[3], cam, w, h, render_type=0)
        gc = ctr.cpu().numpy().astype(np.uint64)[:2]
        assert (gc == 3 * oc[:2]).all(), f"stream {i}: counters {gc} vs 3 x {oc[:2]}"
        assert (rgba.cpu().numpy().reshape(h, w, 4) == oi).all(), f"stream {i}: frame differs"
