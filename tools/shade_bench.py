"""Deferred shading against rt_trace on the bench scene: parity first, then time.  Prints ONE JSON line and (--out) writes it.

Scene: grid_mesh(708) = 1,002,528 triangles with per-corner normals and uv (scenes.smooth_uv_attributes), the two textures of
tests/golden/tiles (tiles_kd 16x12, tiles_bump 8x8, mip chains by Texture::GenerateLODs) and four materials in the arrangement
of tests/texture_scene.py (texture / texture + bump / texture + normal map in `disp` / untextured; runs of 5 cells share a
material), texture_scene's light scaled to the grid, camera A, 1920 x 1080, spp 1, built as LBVH and as SAH.  Per tree and mode (5, 6, 7, 8):
  parity   the pipeline's frame == rt_trace's frame, byte for byte (asserted before anything is timed)
  trace    rt_trace in that mode, the yardstick
  camera   rt_generate_camera_rays, tiled
  closest  rt_intersect_rays, closest hit
  shadow   rt_generate_shadow_rays + rt_intersect_rays any hit (mode 8 only)
  shade    rt_shade_frame
  total    the sum of the parts the mode needs; ratio = total / trace
Each launch (or launch pair) is timed alone between two device events: warm-up first, then --iters launches, median.
The pipeline moves 48 bytes per ray through memory that rt_trace never touches (32 B ray + 16 B hit; mode 8: as much again
for the shadow ray and its record); record_bytes says how much per frame.
Usage: python tools/shade_bench.py [--iters 30] [--warmup 5] [--grid 708] [--out profiles/shade_bench.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILES = os.path.join(ROOT, "tests", "golden", "tiles")
MODES = (5, 6, 7, 8)


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def read_ppm(path):
    """binary P6, maxval 255 -> [sy, sx] uint32 texels r | g<<8 | b<<16 | 255<<24"""
    data = open(path, "rb").read()
    tok, pos = [], 0
    while len(tok) < 4:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        tok.append(data[pos:end])
        pos = end
    assert tok[0] == b"P6" and tok[3] == b"255", path
    sx, sy = int(tok[1]), int(tok[2])
    px = np.frombuffer(data, np.uint8, sx * sy * 3, pos + 1).reshape(sy, sx, 3).astype(np.uint32)
    return px[..., 0] | (px[..., 1] << 8) | (px[..., 2] << 16) | np.uint32(255 << 24)


def make_scene(rt, scenes, ora, grid):
    tris = scenes.grid_mesh(grid, 1)
    n = tris.shape[0]
    mat_ids = ((np.arange(n, dtype=np.int32) // 2 // 5) % 4).astype(np.int32)
    at = scenes.smooth_uv_attributes(tris, mat_ids, seed=1, uv_scale=0.21)
    chains = [ora.generate_lods(read_ppm(os.path.join(TILES, "tiles_kd.ppm"))),
              ora.generate_lods(read_ppm(os.path.join(TILES, "tiles_bump.ppm")))]
    mats = scenes.default_materials(4)
    mats["texture"] = [0, 0, 0, -1]
    mats["bump"] = [-1, 1, -1, -1]
    mats["disp"] = [-1, -1, 1, -1]
    light = (0.5 * grid, 0.075 * grid, -0.25 * grid)   # texture_scene's (20, 3, -10) over its 40-cell grid, scaled to this one
    return tris, at, mats, chains, light


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    from oracle import oracle_py as ora
    tris, at, mats, chains, light = make_scene(rt, scenes, ora, a.grid)
    n = tris.shape[0]
    w, h = a.w, a.h
    cam = rt.to_device(scenes.camera_a(a.grid))
    at_d, mt_d, tex = rt.to_device(at), rt.to_device(mats), rt.DeviceTextures(chains)
    kw = dict(attributes=at_d, materials=mt_d, num_materials=int(mats.shape[0]), light=light, textures=tex)
    k = rt.CameraRayCount(w, h, 1, True)
    rays = torch.empty((k, 8), dtype=torch.float32, device="cuda")
    hits = torch.empty((k, 4), dtype=torch.float32, device="cuda")
    srays, shits = torch.empty_like(rays), torch.empty_like(hits)
    f_trace = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    f_pipe = torch.zeros_like(f_trace)
    res = {}
    for tree in ("lbvh", "sah"):
        inp = rt.BuildInput.allocate(tris, sah=tree == "sah")
        if tree == "sah":
            rt.RunSahBuild(inp)
            root, count = 0, 1
        else:
            rt.RunBottomUpBuild(inp)
            root, count = 0, 2
        T, N = inp.triangles_out, inp.nodes_out

        def trace(mode):
            rt.Trace(T, N, f_trace, (w, h), cam, root, count, render_type=mode, num_primitives=n, **kw)

        def camera():
            rt.GenerateCameraRays(cam, w, h, rays, tiled=True)

        def closest():
            rt.IntersectRays(T, N, root, count, rays, hits, num_primitives=n)

        def shadow():
            rt.GenerateShadowRays(rays, hits, n, light, srays)
            rt.IntersectRays(T, N, root, count, srays, shits, any_hit=True, num_primitives=n)

        def shade(mode):
            rt.ShadeFrame(inp.triangles_in, n, rays, hits, f_pipe, (w, h), render_type=mode, tiled=True,
                          shadow_hits=shits if mode == 8 else None, **kw)

        camera(); closest(); shadow()
        for mode in MODES:                       # parity first
            f_trace.zero_(); f_pipe.zero_()
            trace(mode); shade(mode)
            torch.cuda.synchronize()
            diff = int((f_trace != f_pipe).view(-1, 4).any(dim=1).sum())
            assert diff == 0, f"{tree} mode {mode}: {diff} pixels differ between the pipeline and rt_trace"
        t_cam, t_closest, t_shadow = (timed(f, a.iters, a.warmup) for f in (camera, closest, shadow))
        res[tree] = {}
        for mode in MODES:
            t_trace = timed(lambda: trace(mode), a.iters, a.warmup)
            t_shade = timed(lambda: shade(mode), a.iters, a.warmup)
            total = t_cam + t_closest + t_shade + (t_shadow if mode == 8 else 0.0)
            res[tree][str(mode)] = dict(parity="byte-equal", trace_ms=round(t_trace, 4), camera_ms=round(t_cam, 4),
                                        closest_ms=round(t_closest, 4), shadow_ms=round(t_shadow, 4) if mode == 8 else None,
                                        shade_ms=round(t_shade, 4), total_ms=round(total, 4), ratio=round(total / t_trace, 3))
        del inp
    out = dict(tool="shade_bench", triangles=n, w=w, h=h, camera="A", spp=1, layout="tiled", iters=a.iters, warmup=a.warmup,
               rays=k, record_bytes=dict(modes_5_6_7=48 * k, mode_8=96 * k), results=res,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
