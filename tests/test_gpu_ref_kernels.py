"""The GPU against the reference's own kernels run on the CPU (oracle/_ref/libref_kernels.so, see
tests/test_ref_kernels_cpu.py), without the oracle in between: RunBottomUpBuild (plain and pairs) against
Morton -> stable sort -> GenerateHierarchy -> GenerateTriangles -> GenerateAABBs, and rt_trace on every GPU-built tree
against TraceRays -- frames byte for byte, sum of box tests and of triangle tests exact.  rt_intersect_rays on the
camera rays of rt_generate_camera_rays gives, per pixel, the t of TraceRays' kDepth byte."""
import numpy as np
import pytest

import ref_compare as rc
import texture_scene
from helpers import gpu_build, gpu_trace
from oracle import oracle_py

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not oracle_py.ref_kernels_available(),
                                 reason="oracle/_ref/libref_kernels.so not built (build() on a machine with the reference tree)")]

TREES = ("bottom_up", "pairs", "hybrid", "sah", "sah_pairs", "sah_splits")


def gpu_pairs_build(rt, tris):
    import torch
    n = tris.shape[0]
    inp = rt.BuildInput.allocate(tris)
    inp.nodes_out.fill_(0xCD)
    inp.triangles_out.fill_(0xCD)
    rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kBottomUp, enable_pairs=True))
    torch.cuda.synchronize()
    lay = rt.scratch_layout(n)
    assert int(rt.to_host(inp.scratch, np.uint32, 8, lay.status)[0]) == 0
    L = int(rt.to_host(inp.scratch, np.uint32, 1, lay.num_leaves)[0])
    return dict(inp=inp, L=L, nodes=rt.to_host(inp.nodes_out, rt.NODE, 2 * max(L - 1, 1)),
                leaves=rt.to_host(inp.triangles_out, rt.TRIANGLE_PAIR, L),
                codes=rt.to_host(inp.scratch, np.uint32, L, lay.morton),
                indices=rt.to_host(inp.scratch, np.uint32, L, lay.sorted_indices))


def gpu_tree(rt, tris, tree):
    """GPU build -> (build dict for helpers.gpu_trace, nodes, leaves, root, count); nodes / leaves: the whole buffers"""
    import torch
    n = tris.shape[0]
    if tree.startswith("sah"):
        inp = rt.BuildInput.allocate(tris, sah=True)
        inp.nodes_out.fill_(0xCD)
        inp.triangles_out.fill_(0xCD)
        rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH, enable_pairs="pairs" in tree, enable_splits="splits" in tree))
        torch.cuda.synchronize()
        assert int(rt.to_host(inp.scratch, np.uint32, 8, rt.sah_scratch_layout(n).status)[0]) == 0, tree
        root, count = 0, 1
    else:
        hybrid, pairs = tree == "hybrid", tree == "pairs"
        inp = rt.BuildInput.allocate(tris)
        inp.nodes_out.fill_(0)
        inp.triangles_out.fill_(0xCD)
        rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kHybrid if hybrid else rt.kBottomUp, enable_pairs=pairs),
                            hybrid=hybrid)
        torch.cuda.synchronize()
        lay = rt.scratch_layout(n)
        assert int(rt.to_host(inp.scratch, np.uint32, 8, lay.status)[0]) == 0, tree
        L = int(rt.to_host(inp.scratch, np.uint32, 1, lay.num_leaves)[0]) if pairs else n
        root, count = (2 * max(L, 1) + 1 if hybrid else 0), 2
    nodes = rt.to_host(inp.nodes_out, rt.NODE, inp.nodes_out.numel() // rt.NODE.itemsize)
    leaves = rt.to_host(inp.triangles_out, rt.TRIANGLE_PAIR, inp.triangles_out.numel() // rt.TRIANGLE_PAIR.itemsize)
    return dict(inp=inp), nodes, leaves, root, count


def parity_scenes(scenes, ora):
    out = {}
    for name, tris in (("grid24", scenes.grid_mesh(24, 1)), ("soup2048", scenes.soup(2048, 7)),
                       ("flat12", scenes.flat_mesh(12, 3))):
        b = ora.scene_aabb(tris)
        lo, hi = ora.ordered_to_float(b[:3]), ora.ordered_to_float(b[3:])
        at = scenes.flat_attributes(tris, np.arange(tris.shape[0], dtype=np.int32) % 3)
        out[name] = (tris, scenes.camera_for_box(lo, hi), dict(attributes=at, materials=scenes.default_materials(3),
                                                                light=tuple(float(x) for x in hi + (hi - lo) * 0.5)))
    return out


@pytest.mark.parametrize("n", [0, 511, 512, 513, 32769, 65537, 2097153])
def test_gpu_lbvh_matches_the_reference_kernels(n, rt, scenes, ora):
    """n = 0: the parity scenes (plain and pairs); otherwise soups around the builder's block and sort-tile boundaries"""
    if n == 0:
        cases = [(name, s[0]) for name, s in parity_scenes(scenes, ora).items()]
    else:
        cases = [(f"soup{n}", scenes.soup(n, 21, dup_fraction=0.3 if n < 100000 else 0.05))]
    for name, tris in cases:
        r = ora.ref_build_lbvh(tris)
        rc.assert_build_equal(gpu_build(tris), r, name)
        if n <= 65537:
            rp = ora.ref_build_lbvh(tris, pairs=True)
            g = gpu_pairs_build(rt, tris)
            assert g["L"] == rp["L"], name
            rc.assert_pair_leaves_multiset_equal(g, rp, name + " pairs")


def test_gpu_lbvh_bench_mesh_matches_the_reference_kernels(rt, scenes, ora):
    """The 1M-triangle bench mesh (grid_mesh(708, 1)), plain LBVH, build only."""
    tris = scenes.grid_mesh(708, 1)
    rc.assert_build_equal(gpu_build(tris), ora.ref_build_lbvh(tris), "grid708")


@pytest.mark.parametrize("tree", TREES)
def test_gpu_trace_matches_the_reference_kernel(tree, rt, scenes, ora):
    """Render types 0-4 at 256 x 256 and 97 x 53 on the parity scenes, and kDiffuse."""
    for name, (tris, cam, kw) in parity_scenes(scenes, ora).items():
        g, nodes, leaves, root, count = gpu_tree(rt, tris, tree)
        for (w, h) in ((256, 256), (97, 53)):
            for m in (0, 1, 2, 3, 4, 5):
                img, c = gpu_trace(g, cam, w, h, render_type=m, root=root, count=count, attributes=kw["attributes"],
                                   materials=kw["materials"], light=kw["light"])
                rimg, rcnt = ora.ref_trace(leaves, nodes, root, count, cam, w, h, render_type=m, **kw)
                rc.assert_frames_equal(img, c, rimg, rcnt, f"{name} {tree} {w}x{h} mode {m}")


@pytest.mark.parametrize("tree", TREES)
def test_gpu_textured_modes_match_the_reference_kernel(tree, rt, scenes, ora):
    """Modes 4-8 on the texture scene: the reference's libm log2f / powf / pow against csrc/rt_math.h on the GPU; exact,
    as on the CPU (tests/test_ref_kernels_cpu.py says why)."""
    s = texture_scene.make_smooth(scenes, ora)
    g, nodes, leaves, root, count = gpu_tree(rt, s["tris"], tree)
    kw = dict(attributes=s["attributes"], materials=s["materials"], light=s["light"])
    for cname, cam in s["cameras"].items():
        for m in (4, 5, 6, 7, 8):
            img, c = gpu_trace(g, cam, 97, 53, render_type=m, root=root, count=count, textures=s["textures"], **kw)
            rimg, rcnt = ora.ref_trace(leaves, nodes, root, count, cam, 97, 53, render_type=m, textures=s["textures"], **kw)
            rc.assert_frames_equal(img, c, rimg, rcnt, f"{cname} {tree} mode {m}")


def test_gpu_trace_bench_mesh_matches_the_reference_kernel(rt, scenes, ora):
    """One 480 x 270 kDepth frame of the 1M mesh with camera A, and its box / triangle test sums."""
    G = 708
    tris = scenes.grid_mesh(G, 1)
    g = gpu_build(tris)
    cam = scenes.camera_a(G)
    img, c = gpu_trace(g, cam, 480, 270)
    zeros = np.zeros(tris.shape[0], rt.ATTRIBUTES)
    rimg, rcnt = ora.ref_trace(g["leaves"], g["nodes"], 0, 2, cam, 480, 270, attributes=zeros)
    rc.assert_frames_equal(img, c, rimg, rcnt, "grid708 camera A")
    assert (img[..., 0] > 0).mean() > 0.2


@pytest.mark.parametrize("tree", ("bottom_up", "pairs", "sah_splits"))
def test_gpu_camera_ray_queries_reproduce_the_reference_depth(tree, rt, scenes, ora):
    """rt_generate_camera_rays (row-major) through rt_intersect_rays: each hit's t, run through kDepth's
    min(1, t / max_depth) * 255, is TraceRays' byte for that pixel (a miss is 0)."""
    import torch
    for name, (tris, cam, kw) in parity_scenes(scenes, ora).items():
        g, nodes, leaves, root, count = gpu_tree(rt, tris, tree)
        inp = g["inp"]
        for (w, h) in ((256, 256), (97, 53)):
            n = rt.CameraRayCount(w, h, 1, False)
            rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(rt.to_device(cam), w, h, rays)
            hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            rt.IntersectRays(inp.triangles_out, inp.nodes_out, root, count, rays, hits)
            torch.cuda.synchronize()
            rec = hits.cpu().numpy().view(rt.HIT).reshape(-1)
            md = np.float32(cam["max_depth"][0])
            t = np.where(rec["primitive_id"] != 0xFFFFFFFF, rec["t"], np.float32(0)).astype(np.float32)
            dep = (np.minimum(np.float32(1), (t / md).astype(np.float32)) * np.float32(255)).astype(np.float32)
            rimg, _ = ora.ref_trace(leaves, nodes, root, count, cam, w, h, **kw)
            bad = dep.astype(np.uint8).reshape(h, w) != rimg[..., 0]
            assert not bad.any(), f"{name} {tree} {w}x{h}: {int(bad.sum())} depth bytes differ from TraceRays"
            assert (rec["primitive_id"] != 0xFFFFFFFF).sum() > 10, f"{name}: too few hits to be a test"
