"""Indexed instanced ray queries on an instanced scene: does sorting a secondary batch pay, and what does the index list cost?
Prints ONE JSON line.

Scene: tools/instance_bench.py's -- grid_mesh(177) (62,658 triangles) as one BLAS, 16 instances on a 4 x 4 layout with small
distinct rotations (1,002,528 instanced triangles), per builder (LBVH, SAH) the BLAS and the TLAS built by it.  Batches, made
from the closest hits of the 1920 x 1080 row-major camera-A rays (the LBVH scene's; every builder gets the same rays):
  bounce   one diffuse bounce (raygen.bounce_rays on the flattened world triangles; dead rays where the pixel missed), traced
           closest hit and then any hit -- one sort serves both queries
  shadow   rt_generate_shadow_rays towards a light above the layout, traced any hit
Arms, each timed alone between two device events, warm-up first, median of --iters, counters off:
  a_direct_ms     rt_intersect_rays_instanced on the caller's order (the unsorted direct call)
  b_sort_ms       rt_sort_rays over the TLAS
  b_indexed_ms    rt_intersect_rays_instanced_indexed through the sorted order
  c_gather_ms     today's advice without the indexed call, in ONE timed sequence: rt_sort_rays, the order widened to int64
                  (torch scatters take no int32 index), the rays gathered by it, the direct call on the gathered rays, hits
                  and instance_ids scattered back; every buffer of it is allocated once, outside the timing
  d_identity_ms   rt_intersect_rays_instanced_indexed through the identity list: the price of the indirection alone
Ratios: b_over_a = (sort + indexed) / direct for ONE query; for the bounce batch b2_over_a2 = (sort + closest + any indexed) /
(closest + any direct), one sort serving both; b_over_c = (sort + indexed) / gather sequence; d_over_a = identity / direct.
steps_own / steps_sorted: wave steps (counters[2] + counters[3]) per live ray in the caller's order and the sorted one.
Usage: python tools/instance_indexed_bench.py [--iters 20] [--warmup 3] [--grid 177]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from instance_bench import layout, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=177)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    raygen = importlib.import_module("gpu-raytracing_amd.raygen")
    G = a.grid
    blas_tris = scenes.grid_mesh(G, 1)
    nb = blas_tris.shape[0]
    inst = layout(rt, 4, G, seed=1)
    M = inst["object_to_world"].astype(np.float64)
    T = blas_tris.reshape(-1, 3, 3).astype(np.float64)
    flat = np.concatenate([(T @ m[:, :3].T + m[:, 3]).reshape(-1, 9) for m in M]).astype(np.float32)
    n = flat.shape[0]
    span = 4.3 * G
    cam = rt.to_device(scenes.camera_a(int(round(span))))
    prim = torch.empty((a.w * a.h, 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, a.w, a.h, prim)
    nr = prim.shape[0]

    def build(inp, sah):
        if sah:
            rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH))
        else:
            rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kBottomUp))

    hits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(nr, dtype=torch.int32, device="cuda")
    g_rays, g_hits, g_ids = torch.empty_like(prim), torch.empty_like(hits), torch.empty_like(ids)
    order = torch.empty(nr, dtype=torch.int32, device="cuda")
    order64 = torch.empty(nr, dtype=torch.int64, device="cuda")    # arm (c)'s widened order: allocated once, outside the timing
    identity = torch.arange(nr, dtype=torch.int32, device="cuda")
    scratch = rt.device_bytes(rt.RaySortScratchBytes(nr))
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    batches, live, res = {}, {}, {}
    for name, sah in (("lbvh", False), ("sah", True)):
        root, count = (0, 1) if sah else (0, 2)
        blas = rt.BuildInput.allocate(blas_tris, sah=sah)
        build(blas, sah)
        table = rt.accel_table([(blas.triangles_out, blas.nodes_out, root, count)])
        tlas = rt.BuildInput.allocate(np.zeros((16, 9), np.float32), sah=sah)
        rec, status = rt.device_bytes(64 * 16), rt.device_bytes(4)
        rt.PrepareInstances(rt.to_device(inst), 16, table, 1, tlas.triangles_in, rec, status)
        build(tlas, sah)
        torch.cuda.synchronize()
        assert rt.instance_status(status) == 0
        scene = (tlas.triangles_out, tlas.nodes_out, root, count, rec, 16, table, 1)

        def direct(rays, h, i, any_hit, c=None):
            rt.IntersectRaysInstanced(*scene, rays, h, i, any_hit=any_hit, num_primitives=n, counters=c)

        def indexed(rays, o, any_hit, c=None):
            rt.IntersectRaysInstancedIndexed(*scene, rays, o, hits, ids, any_hit=any_hit, num_primitives=n, counters=c)

        if not batches:     # the two batches, from this (the first) scene's primary hits
            direct(prim, hits, ids, False)
            torch.cuda.synchronize()
            shadow = torch.empty_like(prim)
            rt.GenerateShadowRays(prim, hits, nb, (0.5 * span, 2.0 * span, 0.5 * span), shadow)
            h0 = hits.cpu().numpy().view(rt.HIT).reshape(-1).copy()
            i0 = ids.cpu().numpy().view(np.uint32)
            ok = i0 != rt.MISS
            h0["primitive_id"][ok] = (i0[ok].astype(np.uint64) * nb + h0["primitive_id"][ok]).astype(np.uint32)
            b, live["bounce"] = raygen.bounce_rays(prim.cpu().numpy().view(rt.RAY).reshape(-1), h0, flat, seed=1)
            batches["bounce"] = rt.to_device(b.astype(rt.RAY)).view(torch.float32).view(-1, 8)
            batches["shadow"] = shadow
            live["shadow"] = int(ok.sum())
            del b, h0, i0

        def steps(fn):
            ctr.zero_()
            fn(ctr)
            torch.cuda.synchronize()
            c = ctr.cpu().numpy()
            return int(c[2] + c[3])

        def row(rays, any_hit):
            sort = lambda: rt.SortRays(tlas.nodes_out, root, count, rays, order, scratch)

            def gather():
                sort()
                order64.copy_(order)
                torch.index_select(rays, 0, order64, out=g_rays)
                direct(g_rays, g_hits, g_ids, any_hit)
                hits.index_copy_(0, order64, g_hits)
                ids.index_copy_(0, order64, g_ids)
            sort()
            r = dict(a_direct_ms=timed(lambda: direct(rays, hits, ids, any_hit), a.iters, a.warmup),
                     b_sort_ms=timed(sort, a.iters, a.warmup),
                     b_indexed_ms=timed(lambda: indexed(rays, order, any_hit), a.iters, a.warmup),
                     c_gather_ms=timed(gather, a.iters, a.warmup),
                     d_identity_ms=timed(lambda: indexed(rays, identity, any_hit), a.iters, a.warmup))
            lv = max(rt.ray_sort_live(scratch, nr), 1)
            r["steps_own"] = round(steps(lambda c: direct(rays, hits, ids, any_hit, c)) / lv, 3)
            r["steps_sorted"] = round(steps(lambda c: indexed(rays, order, any_hit, c)) / lv, 3)
            r["b_over_a"] = round((r["b_sort_ms"] + r["b_indexed_ms"]) / r["a_direct_ms"], 3)
            r["b_over_c"] = round((r["b_sort_ms"] + r["b_indexed_ms"]) / r["c_gather_ms"], 3)
            r["d_over_a"] = round(r["d_identity_ms"] / r["a_direct_ms"], 3)
            return {k: round(v, 4) if k.endswith("_ms") else v for k, v in r.items()}

        r = dict(bounce_closest=row(batches["bounce"], False), bounce_any=row(batches["bounce"], True),
                 shadow_any=row(batches["shadow"], True))
        c, y = r["bounce_closest"], r["bounce_any"]
        r["bounce_b2_over_a2"] = round((c["b_sort_ms"] + c["b_indexed_ms"] + y["b_indexed_ms"]) / (c["a_direct_ms"] + y["a_direct_ms"]), 3)
        res[name] = r
        del blas, tlas
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool="instance_indexed_bench", blas_triangles=nb, instances=16, instanced_triangles=n, rays=nr,
                          live=live, camera="A %dx%d row-major" % (a.w, a.h), iters=a.iters, warmup=a.warmup, results=res,
                          device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
