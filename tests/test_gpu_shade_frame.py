"""GPU tests of deferred shading (rt_generate_shadow_rays, rt_shade_frame) on texture_scene.make_smooth, the scene of
tests/test_gpu_shading_trees.py: generate -> intersect -> (shadow rays -> any hit) -> ShadeFrame against rt_trace.

* shadow rays bit-equal to the numpy restatement (tests/shade_pipeline_ref.py), from LBVH and SAH-pairs records;
* non-pair trees (bottom_up, hybrid, sah, sah_splits): the pipeline's frame == rt_trace's frame, byte for byte, in modes
  0, 3-8, both layouts, 160x100 and the ragged 130x101, spp 1 and 4 (16 once);
* pair trees: mode 0 against the numpy byte of the GPU's own records, modes 3-8 against the float64 evaluation of
  tests/shade_ref.py with its existing bounds;
* the frame depends on the records only (sorted-index query, sah_splits vs bottom_up records);
* the miss rule (garbage in miss records, ids >= num_triangles) and the bytes after rgba8;
* the five-call chain recorded in a HIP graph."""
import numpy as np
import pytest

import shade_pipeline_ref as ref
import shade_ref
import texture_scene
from test_gpu_shading_trees import _gpu_tree

pytestmark = pytest.mark.gpu

MODES = (0, 3, 4, 5, 6, 7, 8)
EXACT_TREES = ("bottom_up", "hybrid", "sah", "sah_splits")
PAIR_TREES = ("pairs", "sah_pairs", "sah_pairs_splits")
SIZES = ((160, 100), (130, 101))


@pytest.fixture(scope="module")
def world(rt, scenes, ora):
    sc = texture_scene.make_smooth(scenes, ora)
    sc["cam"] = sc["cameras"]["oblique"]
    sc["kw"] = dict(attributes=sc["attributes"], materials=sc["materials"], light=sc["light"], textures=sc["textures"])
    sc["n"] = sc["tris"].shape[0]
    sc["gpu"] = {tree: _gpu_tree(rt, sc["tris"], tree) for tree in EXACT_TREES + PAIR_TREES}
    sc["dev"] = dict(cam=rt.to_device(sc["cam"]), attributes=rt.to_device(sc["attributes"]),
                     materials=rt.to_device(sc["materials"]), textures=rt.DeviceTextures(sc["textures"]))
    return sc


def _records(rt, sc, tree, w, h, spp=1, tiled=False, shadows=True, stream=None, bufs=None):
    """generate -> intersect -> shadow rays -> any hit; returns the four device buffers"""
    import torch
    g, root, count = sc["gpu"][tree]
    inp = g["inp"]
    n = rt.CameraRayCount(w, h, spp, tiled)
    if bufs is None:
        bufs = dict(rays=torch.zeros((n, 8), dtype=torch.float32, device="cuda"),
                    hits=torch.zeros((n, 4), dtype=torch.float32, device="cuda"),
                    srays=torch.zeros((n, 8), dtype=torch.float32, device="cuda"),
                    shits=torch.zeros((n, 4), dtype=torch.float32, device="cuda"))
    rt.GenerateCameraRays(sc["dev"]["cam"], w, h, bufs["rays"], spp=spp, tiled=tiled, stream=stream)
    rt.IntersectRays(inp.triangles_out, inp.nodes_out, root, count, bufs["rays"], bufs["hits"], stream=stream)
    if shadows:
        rt.GenerateShadowRays(bufs["rays"], bufs["hits"], sc["n"], sc["light"], bufs["srays"], stream=stream)
        rt.IntersectRays(inp.triangles_out, inp.nodes_out, root, count, bufs["srays"], bufs["shits"], any_hit=True,
                         stream=stream)
    return bufs


def _shade(rt, sc, tree, rec, w, h, mode, spp=1, tiled=False, rgba=None, stream=None, hits=None):
    import torch
    inp = sc["gpu"][tree][0]["inp"]
    own = rgba is None
    if own:
        rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    d = sc["dev"]
    rt.ShadeFrame(inp.triangles_in, sc["n"], rec["rays"], rec["hits"] if hits is None else hits, rgba, (w, h),
                  render_type=mode, spp=spp, tiled=tiled, shadow_hits=rec["shits"] if mode == 8 else None,
                  attributes=d["attributes"], materials=d["materials"], num_materials=sc["materials"].shape[0],
                  light=sc["light"], textures=d["textures"], stream=stream)
    if not own:
        return None
    torch.cuda.synchronize()
    return rgba.cpu().numpy().reshape(h, w, 4)


def _trace(sc, tree, mode, w, h, spp=1):
    from helpers import gpu_trace
    g, root, count = sc["gpu"][tree]
    return gpu_trace(g, sc["cam"], w, h, mode, root=root, count=count, spp=spp, **sc["kw"])[0]


def _assert_same(got, exp, what):
    if not (got == exp).all():
        d = np.abs(got.astype(np.int32) - exp.astype(np.int32))
        ys, xs = np.nonzero(d.max(axis=-1))
        raise AssertionError(f"{what}: {ys.size} pixels differ (max {d.max()}), first (x={xs[0]}, y={ys[0]}): "
                             f"pipeline {got[ys[0], xs[0]].tolist()} rt_trace {exp[ys[0], xs[0]].tolist()}")


def _host(rt, t, dtype):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(-1).view(dtype).copy()


# ------------------------------------------------------------------ 1. shadow rays
@pytest.mark.parametrize("tree", ["bottom_up", "sah_pairs"])
@pytest.mark.parametrize("tiled", [False, True])
def test_shadow_rays_equal_the_restatement(world, rt, tree, tiled):
    w, h = 130, 101
    rec = _records(rt, world, tree, w, h, spp=4, tiled=tiled)
    rays, hits = _host(rt, rec["rays"], ref.RAY), _host(rt, rec["hits"], ref.HIT)
    got = _host(rt, rec["srays"], ref.RAY)
    exp = ref.shadow_rays(rays, hits, world["n"], world["light"])
    n_hit = int((hits["primitive_id"] < world["n"]).sum())
    assert n_hit > 10_000 and n_hit < rays.shape[0], "the frame has hits and misses"
    assert got.tobytes() == exp.tobytes()
    alive = got["tmax"] != -1
    assert int(alive.sum()) == n_hit
    # the documented divergence (hit point at the light) is not in play on this scene
    assert (got["tmax"][alive] > 0.001).all()
    assert not np.isnan(got["origin"]).any() and not np.isnan(got["dir"]).any() and not np.isnan(got["tmax"]).any()
    shadowed = _host(rt, rec["shits"], ref.HIT)["primitive_id"] < world["n"]
    assert not shadowed[~alive].any() and 0 < int(shadowed.sum()) < n_hit, "some hits are in shadow, some are lit"


# ------------------------------------------------------------------ 2. byte-exact against rt_trace
@pytest.mark.parametrize("tree", EXACT_TREES)
def test_pipeline_frame_equals_rt_trace(world, rt, tree):
    for (w, h) in SIZES:
        for spp in (1, 4):
            exp = {mode: _trace(world, tree, mode, w, h, spp) for mode in MODES}
            for tiled in (False, True):
                rec = _records(rt, world, tree, w, h, spp=spp, tiled=tiled)
                for mode in MODES:
                    got = _shade(rt, world, tree, rec, w, h, mode, spp=spp, tiled=tiled)
                    _assert_same(got, exp[mode], f"{tree} {w}x{h} spp {spp} {'tiled' if tiled else 'row-major'} mode {mode}")


def test_pipeline_frame_equals_rt_trace_spp16(world, rt):
    w, h = 130, 101
    for tiled in (False, True):
        rec = _records(rt, world, "sah", w, h, spp=16, tiled=tiled)
        for mode in (0, 4, 8):
            _assert_same(_shade(rt, world, "sah", rec, w, h, mode, spp=16, tiled=tiled), _trace(world, "sah", mode, w, h, 16),
                         f"sah spp 16 {'tiled' if tiled else 'row-major'} mode {mode}")


# ------------------------------------------------------------------ 3. pair trees
@pytest.fixture(scope="module")
def f64(world):
    return shade_ref.Reference(world["tris"], world["attributes"], world["materials"], world["textures"], world["light"],
                               world["cam"], 160, 100)


@pytest.mark.parametrize("tree", PAIR_TREES)
def test_pair_trees(world, rt, f64, tree):
    w, h = 160, 100
    for tiled in (False, True):
        rec = _records(rt, world, tree, w, h, tiled=tiled)
        if not tiled:
            hits = _host(rt, rec["hits"], ref.HIT)
            b = ref.depth_byte(hits, _host(rt, rec["rays"], ref.RAY)["tmax"], world["n"]).reshape(h, w)
            exp = np.stack([b, b, b, np.full_like(b, 255)], axis=-1)
            _assert_same(_shade(rt, world, tree, rec, w, h, 0), exp, f"{tree} mode 0 from its own records")
        for mode in (3, 4, 5, 6, 7, 8):
            got = _shade(rt, world, tree, rec, w, h, mode, tiled=tiled)
            r = shade_ref.compare(got, f64, mode)
            print(f"{tree} {'tiled' if tiled else 'row-major'} mode {mode}: masked {100 * r['masked_fraction']:.2f} %, "
                  f"max |diff| {r['max_diff']}, {r['n_bad']} bad")
            assert r["n_bad"] == 0, f"{tree} mode {mode}: {r['n_bad']} stable pixels out of tolerance (max {r['max_diff']})"
            assert r["masked_fraction"] <= shade_ref.MASK_BOUND[mode]


# ------------------------------------------------------------------ 4. records, not trees, decide the frame
def test_indexed_query_records_give_the_same_frame(world, rt):
    import torch
    w, h, tree = 130, 101, "sah"
    g, root, count = world["gpu"][tree]
    inp = g["inp"]
    rec = _records(rt, world, tree, w, h, spp=4)
    n = rec["rays"].shape[0]
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    scratch = rt.device_bytes(rt.RaySortScratchBytes(n))
    rt.SortRays(inp.nodes_out, root, count, rec["rays"], order, scratch)
    hits2 = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    rt.IntersectRaysIndexed(inp.triangles_out, inp.nodes_out, root, count, rec["rays"], order, hits2)
    torch.cuda.synchronize()
    assert hits2.cpu().numpy().tobytes() == rec["hits"].cpu().numpy().tobytes()
    for mode in MODES:
        _assert_same(_shade(rt, world, tree, rec, w, h, mode, spp=4, hits=hits2), _shade(rt, world, tree, rec, w, h, mode, spp=4),
                     f"indexed records, mode {mode}")


def test_records_from_two_trees_give_identical_frames(world, rt):
    w, h = 160, 100
    a = _records(rt, world, "sah_splits", w, h, tiled=True)
    b = _records(rt, world, "bottom_up", w, h, tiled=True)
    import torch
    torch.cuda.synchronize()
    for k in ("rays", "hits", "srays"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), f"{k} differ between the two trees"
    # (an any-hit record may name another occluder from another tree: only hit / miss is compared)
    sa, sb = _host(rt, a["shits"], ref.HIT)["primitive_id"], _host(rt, b["shits"], ref.HIT)["primitive_id"]
    assert ((sa < world["n"]) == (sb < world["n"])).all()
    for mode in MODES:
        fa = _shade(rt, world, "sah_splits", a, w, h, mode, tiled=True)
        fb = _shade(rt, world, "bottom_up", b, w, h, mode, tiled=True)
        assert fa.tobytes() == fb.tobytes(), f"mode {mode}"


# ------------------------------------------------------------------ 5. the miss rule, and nothing written past the frame
@pytest.mark.parametrize("tiled", [False, True])
def test_miss_records_and_guard_bytes(world, rt, tiled):
    import torch
    w, h, tree, spp = 130, 101, "bottom_up", 4
    rec = _records(rt, world, tree, w, h, spp=spp, tiled=tiled)
    clean = {mode: _shade(rt, world, tree, rec, w, h, mode, spp=spp, tiled=tiled) for mode in MODES}
    hits = rec["hits"].cpu().numpy().copy()
    ids = hits.view(np.uint32)[:, 1]
    miss = np.nonzero(ids >= world["n"])[0]
    assert miss.size > 1000
    rng = np.random.default_rng(3)
    junk = rng.choice(np.float32([np.nan, -1.0, 0.0, 1e30, 5.0, -np.inf]), (miss.size, 3))
    hits[miss, 0], hits[miss, 2], hits[miss, 3] = junk[:, 0], junk[:, 1], junk[:, 2]
    ids[miss[::2]] = world["n"] + rng.integers(0, 1 << 20, miss[::2].size).astype(np.uint32)
    ids[miss[0]] = world["n"]                                    # the first id that is no triangle
    dirty = rt.to_device(hits)
    shits = rec["shits"].cpu().numpy().copy()                    # shadow records: only primitive_id is read
    shits[:, 0], shits[:, 2], shits[:, 3] = np.nan, -7.0, np.inf
    rec2 = dict(rec, shits=rt.to_device(shits))
    guard = 64
    for mode in MODES:
        buf = torch.full((w * h * 4 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        _shade(rt, world, tree, rec2, w, h, mode, spp=spp, tiled=tiled, rgba=buf, hits=dirty)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[w * h * 4:] == 0xA5).all(), f"mode {mode}: bytes after rgba8 were written"
        _assert_same(out[:w * h * 4].reshape(h, w, 4), clean[mode], f"mode {mode}: dirty miss records")


# ------------------------------------------------------------------ 6. the whole chain in a HIP graph
def test_five_call_chain_in_a_hip_graph(world, rt):
    import torch
    w, h, tree, spp, mode = 160, 100, "sah", 4, 8
    eager_rec = _records(rt, world, tree, w, h, spp=spp, tiled=True)
    eager = _shade(rt, world, tree, eager_rec, w, h, mode, spp=spp, tiled=True)
    _assert_same(eager, _trace(world, tree, mode, w, h, spp), "eager pipeline")

    bufs = {k: torch.zeros_like(v) for k, v in eager_rec.items()}
    frame = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")

    def chain():   # five calls, one stream, no branches
        _records(rt, world, tree, w, h, spp=spp, tiled=True, bufs=bufs)
        _shade(rt, world, tree, bufs, w, h, mode, spp=spp, tiled=True, rgba=frame)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        chain()                           # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            chain()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in list(bufs.values()) + [frame]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(frame.cpu().numpy().reshape(h, w, 4), eager, "graph replay")
