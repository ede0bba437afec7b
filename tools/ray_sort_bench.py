"""Ray sorting on the bench scene: prints ONE JSON line.

Scene and timing as tools/ray_query_bench.py: grid_mesh(708) = 1,002,528 triangles, camera A, 1920 x 1080, counters off, each
launch (or launch sequence) timed alone between two device events, warm-up first, median of --iters.  Trees: the LBVH and the
SAH tree.  Batches:
  camera_tiled   camera rays in 8x8-tile order (already coherent: what the sort costs where it cannot help)
  bounce1        one diffuse bounce from the primary hits (raygen.bounce_rays; dead rays where the pixel missed)
  bounce1_shuffled  bounce1 in a seeded random order (rays from scattered points: no coherence in the caller's order)
  bounce2        a second bounce from bounce1's hits
  occlusion      4 short rays per primary hit, tmax = 3 % of the scene extent (raygen.occlusion_rays)
Per (tree, batch, closest / any hit):
  yardstick_ms   rt_intersect_rays on the caller's order
  sort_ms        rt_sort_rays (box + keys + radix sort)
  indexed_ms     rt_intersect_rays_indexed through the sorted order, all num_rays positions
  live_ms        ... through the live prefix only (num_indices = num_live)
  total_ratio    (sort_ms + indexed_ms) / yardstick_ms -- the figure that matters; below 1 the sort pays for itself in ONE query
  steps_*        wave steps (counters[2] + counters[3]) per live ray, caller's order and sorted order

--layouts 0,1,2: compare key layouts (bounce and occlusion batches, LBVH, closest hit).  Needs the experiment build
(make -C gpu-raytracing_amd/csrc librt_amd_exp.so EXPFLAGS=-DRT_EXP_RAY_KEYS) loaded through RT_LIB=<path>: it reads the layout
per launch from the RT_RAY_KEY environment variable (0 = the shipped layout; see ray_sort.hip for the others).
--sort-only: nothing but --iters sorts of bounce1 and of occlusion (for a rocprofv3 --kernel-trace --stats run).
Usage: python tools/ray_sort_bench.py [--iters 30] [--warmup 5] [--grid 708]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUT_NAMES = {0: "o7.d2 (shipped)", 1: "octant | o7 | d1", 2: "o6.d3", 3: "o9", 4: "d2 | o7", 5: "o8.d1"}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--layouts", default="")
    ap.add_argument("--sort-only", action="store_true")
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if os.environ.get("RT_LIB"):
        rt.LIB_PATH = os.path.abspath(os.environ["RT_LIB"])
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    raygen = importlib.import_module("gpu-raytracing_amd.raygen")
    tris = scenes.grid_mesh(a.grid, 1)
    n = tris.shape[0]
    w, h = a.w, a.h
    cam = rt.to_device(scenes.camera_a(a.grid))
    lbvh = rt.BuildInput.allocate(tris)
    rt.RunBottomUpBuild(lbvh)
    sah = rt.BuildInput.allocate(tris, sah=True)
    rt.RunSahBuild(sah)
    torch.cuda.synchronize()
    trees = dict(lbvh=(lbvh.triangles_out, lbvh.nodes_out, 0, 2), sah=(sah.triangles_out, sah.nodes_out, 0, 1))

    def dev(rays):
        return rt.to_device(rays).view(torch.float32).view(-1, 8)

    def trace_host(tree, rays_dev):
        T, N, root, count = trees[tree]
        hits = torch.empty((rays_dev.shape[0], 4), dtype=torch.float32, device="cuda")
        rt.IntersectRays(T, N, root, count, rays_dev, hits, num_primitives=n)
        torch.cuda.synchronize()
        return hits.cpu().numpy().view(rt.HIT).reshape(-1)

    # the batches (host-generated from the LBVH's hits; every tree gets the same rays)
    prim = torch.empty((w * h, 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, w, h, prim)
    tiled = torch.empty((rt.CameraRayCount(w, h, 1, True), 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, w, h, tiled, tiled=True)
    prim_h = prim.cpu().numpy().view(rt.RAY).reshape(-1)
    hits0 = trace_host("lbvh", prim)
    extent = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    b1, live1 = raygen.bounce_rays(prim_h, hits0, tris, seed=1)
    b1d = dev(b1)
    b2, live2 = raygen.bounce_rays(b1, trace_host("lbvh", b1d), tris, seed=2)
    ao, live_ao = raygen.occlusion_rays(prim_h, hits0, tris, per_hit=4, length=0.03 * extent, seed=3)
    batches = dict(camera_tiled=tiled, bounce1=b1d, bounce1_shuffled=dev(b1[np.random.default_rng(7).permutation(b1.size)]),
                   bounce2=dev(b2), occlusion=dev(ao))
    del b1, b2, ao

    nmax = max(b.shape[0] for b in batches.values())
    hits = torch.empty((nmax, 4), dtype=torch.float32, device="cuda")
    order = torch.empty(nmax, dtype=torch.int32, device="cuda")
    scratch = rt.device_bytes(rt.RaySortScratchBytes(nmax))
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")

    def steps(fn):
        ctr.zero_()
        fn(ctr)
        torch.cuda.synchronize()
        c = ctr.cpu().numpy()
        return int(c[2] + c[3])

    def row(tree, rays, any_hit, full=True):
        T, N, root, count = trees[tree]
        k = rays.shape[0]
        o, hv = order[:k], hits[:k]
        sort = lambda: rt.SortRays(N, root, count, rays, o, scratch)
        sort()
        live = rt.ray_sort_live(scratch, k)
        direct = lambda c=None: rt.IntersectRays(T, N, root, count, rays, hv, any_hit=any_hit, num_primitives=n, counters=c)
        indexed = lambda c=None: rt.IntersectRaysIndexed(T, N, root, count, rays, o, hv, any_hit=any_hit, num_primitives=n, counters=c)
        prefix = lambda: rt.IntersectRaysIndexed(T, N, root, count, rays, o, hv, num_indices=live, any_hit=any_hit, num_primitives=n)
        r = dict(rays=k, live=live, steps_caller_order=round(steps(direct) / max(live, 1), 3),
                 steps_sorted=round(steps(indexed) / max(live, 1), 3))
        r["indexed_ms"] = round(timed(indexed, a.iters, a.warmup), 4)
        if full:
            r["yardstick_ms"] = round(timed(direct, a.iters, a.warmup), 4)
            r["sort_ms"] = round(timed(sort, a.iters, a.warmup), 4)
            r["live_ms"] = round(timed(prefix, a.iters, a.warmup), 4)
            r["total_ratio"] = round((r["sort_ms"] + r["indexed_ms"]) / r["yardstick_ms"], 3)
            r["query_ratio"] = round(r["indexed_ms"] / r["yardstick_ms"], 3)
        return r

    if a.sort_only:
        for name in ("bounce1", "occlusion"):
            rays = batches[name]
            for _ in range(a.iters):
                rt.SortRays(lbvh.nodes_out, 0, 2, rays, order[:rays.shape[0]], scratch)
        torch.cuda.synchronize()
        print(json.dumps(dict(tool="ray_sort_bench", sort_only=True, iters=a.iters, rays=[batches["bounce1"].shape[0],
                                                                                          batches["occlusion"].shape[0]])))
        return

    out = dict(tool="ray_sort_bench", triangles=n, w=w, h=h, camera="A", iters=a.iters, warmup=a.warmup,
               live=dict(bounce1=live1, bounce2=live2, occlusion=live_ao), device=torch.cuda.get_device_name(0),
               library=os.path.basename(rt.LIB_PATH))
    if a.layouts:
        res = {}
        for lay in [int(x) for x in a.layouts.split(",")]:
            os.environ["RT_RAY_KEY"] = str(lay)
            res[str(lay)] = dict(name=LAYOUT_NAMES.get(lay, "?"),
                                 **{b: row("lbvh", batches[b], False, full=(lay == 0)) for b in ("bounce1", "bounce2", "occlusion")})
        out["layouts"] = res
    else:
        res = {}
        for tree in trees:
            for mode, any_hit in (("closest", False), ("any", True)):
                for b, rays in batches.items():
                    res[f"{tree}_{b}_{mode}"] = row(tree, rays, any_hit)
        out["results"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
