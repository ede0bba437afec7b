"""GPU parity of the surface render types (modes 3-8) on every tree the builders make, on a scene whose attributes show
every corner: smooth, distinct per-corner normals and jittered per-corner uv (texture_scene.make_smooth), with diffuse
textures, a bump map and a normal map on different materials.  Frames byte-equal to the oracle, Σbox / Σtri equal.

The textured modes were exercised before on plain LBVH trees only, and pair trees only with one normal per triangle
and uv = 0, so the attribute rotation of pairs (Tracer.cu:57-82 with the (v2, v1, v3) triangle of :293-306) and
primitive_id on split references never reached a frame.  Here they do -- the scene's corners are rolled so that the
pairs carry every rotation of both triangles (asserted) -- on:
* bottom-up, pairs, hybrid, hybrid + pairs (rooted at 2L+1: frames equal to the pairs tree's), SAH, SAH + pairs,
  SAH + splits, SAH + pairs + splits;
* the pair-prefetch instantiation (scene-size hint >= kPrefetchMinPrims) in modes 4, 6, 7;
* a row band, interleaved strips (rt_trace_strips) and spp = 4 in the lit modes -- kTextureLitShadows runs its shadow
  traversal over the lanes that hit, so ragged tiles and inactive lanes matter there.
One tree per builder is also held against the float64 evaluation of tests/shade_ref.py, which does not depend on the
oracle."""
import numpy as np
import pytest

import shade_ref
import texture_scene

pytestmark = pytest.mark.gpu

W, H = 160, 100
MODES = (3, 4, 5, 6, 7, 8)
BIG = 10_000_000    # scene-size hint that selects the pair-prefetch instantiation (as in test_gpu_traversal_edges.py)
TREES = ("bottom_up", "pairs", "hybrid", "sah", "sah_pairs", "sah_splits", "sah_pairs_splits")


def _gpu_tree(rt, tris, tree):
    """GPU build -> (build dict for helpers.gpu_trace, root, count)"""
    import torch
    n = tris.shape[0]
    if tree.startswith("sah"):
        inp = rt.BuildInput.allocate(tris, sah=True)
        inp.nodes_out.fill_(0xCD)
        inp.triangles_out.fill_(0xCD)
        rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH, enable_pairs="pairs" in tree, enable_splits="splits" in tree))
        torch.cuda.synchronize()
        status = rt.to_host(inp.scratch, np.uint32, 8, rt.sah_scratch_layout(n).status)
        assert status[0] == 0, f"{tree}: build error flags {status[0]:#x}"
        return dict(inp=inp), 0, 1
    hybrid, pairs = "hybrid" in tree, "pairs" in tree
    inp = rt.BuildInput.allocate(tris)
    inp.nodes_out.fill_(0)
    inp.triangles_out.fill_(0xCD)
    rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kHybrid if hybrid else rt.kBottomUp, enable_pairs=pairs), hybrid=hybrid)
    torch.cuda.synchronize()
    lay = rt.scratch_layout(n)
    status = rt.to_host(inp.scratch, np.uint32, 8, lay.status)
    assert status[0] == 0, f"{tree}: build error flags {status[0]:#x}"
    L = int(rt.to_host(inp.scratch, np.uint32, 1, lay.num_leaves)[0]) if pairs else n
    return dict(inp=inp), (2 * max(L, 1) + 1 if hybrid else 0), 2


def _ora_tree(ora, tris, tree):
    if tree == "bottom_up":
        o = ora.build_bvh(tris)
        return o["leaves"], o["nodes"], 0, 2
    if tree in ("pairs", "hybrid_pairs"):      # hybrid + pairs: same leaves, its frames equal the pairs tree's
        o = ora.build_pairs(tris)
        return o["leaves"], o["nodes"], 0, 2
    if tree == "hybrid":
        o = ora.build_hybrid(tris)
        return o["leaves"], o["nodes"], o["root"], 2
    o = ora.build_sah(tris, pairs="pairs" in tree, splits="splits" in tree)
    return o["leaves"], o["nodes"], 0, 1


@pytest.fixture(scope="module")
def world(rt, scenes, ora):
    sc = texture_scene.make_smooth(scenes, ora)
    sc["cam"] = sc["cameras"]["oblique"]
    sc["kw"] = dict(attributes=sc["attributes"], materials=sc["materials"], light=sc["light"], textures=sc["textures"])
    sc["gpu"], sc["ora"] = {}, {}
    for tree in TREES + ("hybrid_pairs",):
        sc["gpu"][tree] = _gpu_tree(rt, sc["tris"], tree)
        sc["ora"][tree] = _ora_tree(ora, sc["tris"], tree)
    return sc


@pytest.mark.parametrize("tree", ["pairs", "sah_pairs", "sah_pairs_splits"])
def test_gpu_pair_leaves_hold_every_rotation(world, rt, tree):
    """the GPU's pair leaves equal the oracle's and store every rotation of both triangles (so the frames below run
    every case of RotateAttributes)"""
    leaves = world["ora"][tree][0]
    got = rt.to_host(world["gpu"][tree][0]["inp"].triangles_out, rt.TRIANGLE_PAIR, leaves.shape[0])
    assert got.tobytes() == leaves.tobytes()
    rot = texture_scene.pair_rotations(leaves)
    for side in (0, 1):
        assert (np.bincount(rot[:, side], minlength=3) > 0).all(), f"rotations[{side}]"


def _ora_frame(ora, sc, tree, mode, w=W, h=H, **extra):
    leaves, nodes, root, count = sc["ora"][tree]
    return ora.trace(leaves, nodes, root, count, sc["cam"], w, h, render_type=mode, **sc["kw"], **extra)


def _gpu_frame(sc, tree, mode, w=W, h=H, **extra):
    from helpers import gpu_trace
    g, root, count = sc["gpu"][tree]
    return gpu_trace(g, sc["cam"], w, h, mode, root=root, count=count, **sc["kw"], **extra)


def _assert_same(got, exp, what):
    if not (got == exp).all():
        d = np.abs(got.astype(np.int32) - exp.astype(np.int32))
        ys, xs = np.nonzero(d.max(axis=-1))
        raise AssertionError(f"{what}: {ys.size} pixels differ (max {d.max()}), first (x={xs[0]}, y={ys[0]}): "
                             f"gpu {got[ys[0], xs[0]].tolist()} oracle {exp[ys[0], xs[0]].tolist()}")


@pytest.mark.parametrize("tree", TREES)
def test_surface_modes_every_tree(world, ora, tree):
    for mode in MODES:
        exp, oc = _ora_frame(ora, world, tree, mode)
        got, gc = _gpu_frame(world, tree, mode)
        _assert_same(got, exp, f"{tree} mode {mode}")
        assert (gc == oc[:2]).all(), f"{tree} mode {mode}: counters {gc} vs {oc[:2]}"


def test_surface_modes_hybrid_pairs(world, ora):
    """hybrid + pairs rooted at 2L+1: the same leaves as the pairs tree, so the same frames (counters come from a
    different tree and are not compared)"""
    for mode in MODES:
        exp, _ = _ora_frame(ora, world, "hybrid_pairs", mode)
        got, _ = _gpu_frame(world, "hybrid_pairs", mode)
        _assert_same(got, exp, f"hybrid + pairs mode {mode}")


@pytest.fixture(scope="module")
def f64(world):
    return shade_ref.Reference(world["tris"], world["attributes"], world["materials"], world["textures"], world["light"],
                               world["cam"], W, H)


@pytest.mark.parametrize("tree", ["bottom_up", "pairs", "hybrid", "sah_pairs_splits"])
def test_gpu_frames_match_float64(world, f64, tree):
    """one tree per builder (LBVH, LBVH + pairs, hybrid top tree, SAH with pairs and splits) against the float64
    evaluation, independently of the oracle"""
    for mode in MODES:
        got, _ = _gpu_frame(world, tree, mode)
        r = shade_ref.compare(got, f64, mode)
        print(f"{tree} mode {mode}: masked {100 * r['masked_fraction']:.2f} %, max |diff| {r['max_diff']}, {r['n_bad']} bad")
        assert r["masked_fraction"] <= shade_ref.MASK_BOUND[mode]
        assert r["n_bad"] == 0, f"{tree} mode {mode}: {r['n_bad']} stable pixels out of tolerance (max {r['max_diff']})"


@pytest.mark.parametrize("tree", ["bottom_up", "sah_pairs"])
def test_prefetch_instantiation_textured_modes(world, ora, tree):
    for mode in (4, 6, 7):
        exp, oc = _ora_frame(ora, world, tree, mode)
        got, gc = _gpu_frame(world, tree, mode, num_primitives=BIG)
        _assert_same(got, exp, f"prefetch {tree} mode {mode}")
        assert (gc == oc[:2]).all()


@pytest.mark.parametrize("tree", ["pairs", "sah_pairs_splits"])
def test_lit_modes_row_band_strips_and_spp(world, rt, ora, tree):
    import torch
    g, root, count = world["gpu"][tree]
    w, h = 130, 101
    for mode in (7, 8):
        rows = (13, 71)
        exp, oc = _ora_frame(ora, world, tree, mode, w, h, rows=rows)
        got, gc = _gpu_frame(world, tree, mode, w, h, rows=rows)
        _assert_same(got[rows[0]:rows[1]], exp[rows[0]:rows[1]], f"{tree} mode {mode} rows {rows}")
        assert (gc == oc[:2]).all()
        full, _ = _ora_frame(ora, world, tree, mode, w, h)
        at, mt = rt.to_device(world["attributes"]), rt.to_device(world["materials"])
        tex = rt.DeviceTextures(world["textures"])
        for first, stride in ((0, 3), (2, 3)):
            nstr = len(range(first, (h + 7) // 8, stride))
            compact = torch.zeros(nstr * 8 * w * 4, dtype=torch.uint8, device="cuda")
            rt.Trace(g["inp"].triangles_out, g["inp"].nodes_out, compact, (w, h), rt.to_device(world["cam"]), root, count,
                     render_type=mode, attributes=at, materials=mt, num_materials=world["materials"].shape[0],
                     light=world["light"], textures=tex, strips=(8, first, stride))
            torch.cuda.synchronize()
            got = compact.cpu().numpy().reshape(nstr * 8, w, 4)
            for j, st in enumerate(range(first, (h + 7) // 8, stride)):
                rows_in = min(8, h - st * 8)
                _assert_same(got[j * 8: j * 8 + rows_in], full[st * 8: st * 8 + rows_in], f"{tree} mode {mode} strip {st}")
    exp, oc = _ora_frame(ora, world, tree, 8, w, h, spp=4)
    got, gc = _gpu_frame(world, tree, 8, w, h, spp=4)
    _assert_same(got, exp, f"{tree} mode 8 spp 4")
    assert (gc == oc[:2]).all()
