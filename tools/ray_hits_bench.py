"""All-hit ray-query throughput on the bench scene: prints ONE JSON line (and writes it to --out when given).

Scene: grid_mesh(708) = 1,002,528 triangles, on the LBVH and SAH trees.  Rays: the camera-A frame (1920 x 1080, 8 x 8-tiled,
tmax = the camera's max depth) and one diffuse bounce from its primary hits (tools/ray_query_bench.py's batch, tmax = +inf).
Per (tree, ray set), each launch sequence timed alone between two device events (warm-up first, then --iters, median):
  count_ms    rt_ray_hits_count (traversal + workgroup scan, the scan of the workgroup sums, the add)
  collect_ms  rt_ray_hits_collect into exactly offsets[n] records, with counts
  fixed_ms    rt_ray_hits_collect with offsets[i] = i * K (--k, default 4), with counts: the one-pass pattern
  closest_ms  the yardstick: rt_intersect_rays closest hit on the same rays in the same run
and, from one counted launch of each, the box tests and leaf visits per ray of the all-hit traversal and of closest hit.
The figure to read: count_ms / closest_ms beside box_per_ray / closest_box_per_ray -- a fixed window visits more of the tree;
what time grows beyond that is the kernel's.
Usage: python tools/ray_hits_bench.py [--iters 30] [--warmup 5] [--grid 708] [--w 1920] [--h 1080] [--k 4]
                                      [--out profiles/ray_hits_bench.json]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from point_query_bench import build, timed  # noqa: E402
from ray_query_bench import bounce_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    tris = scenes.grid_mesh(a.grid, 1)
    n = tris.shape[0]
    cam = rt.to_device(scenes.camera_a(a.grid))
    w, h, K = a.w, a.h, a.k
    res = {}
    sets = {}
    for kind in ("lbvh", "sah"):
        inp, root, count = build(rt, tris, kind)
        T, N = inp.triangles_out, inp.nodes_out
        if not sets:                               # the rays do not depend on the tree
            tiled = torch.empty((rt.CameraRayCount(w, h, 1, True), 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(cam, w, h, tiled, tiled=True)
            row_major = torch.empty((w * h, 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(cam, w, h, row_major)
            prim = torch.empty((w * h, 4), dtype=torch.float32, device="cuda")
            rt.IntersectRays(T, N, root, count, row_major, prim, num_primitives=n)
            torch.cuda.synchronize()
            sets = {"camera_a_tiled": tiled, "bounce": bounce_rays(rt, row_major, prim, tris)[0]}
            del row_major, prim
        row = {}
        for name, rays in sets.items():
            nr = rays.shape[0]
            offsets = torch.empty(nr + 1, dtype=torch.int64, device="cuda")
            fixed = torch.arange(nr + 1, dtype=torch.int64, device="cuda") * K
            scratch = rt.device_bytes(rt.RayHitsScratchBytes(nr))
            counts = torch.empty(nr, dtype=torch.int32, device="cuda")
            closest = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
            ctr = torch.zeros(8, dtype=torch.int64, device="cuda")
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            closest_ms = timed(lambda: rt.IntersectRays(T, N, root, count, rays, closest, num_primitives=n), a.iters, a.warmup)
            count_ms = timed(lambda: rt.RayHitsCount(T, N, root, count, rays, offsets, scratch=scratch), a.iters, a.warmup)
            rt.RayHitsCount(T, N, root, count, rays, offsets, scratch=scratch, counters=ctr[:4], status=st)
            rt.IntersectRays(T, N, root, count, rays, closest, num_primitives=n, counters=ctr[4:])
            total = int(offsets[nr].item())
            c = ctr.cpu().numpy()
            hits = torch.empty((max(total, 1), 4), dtype=torch.float32, device="cuda")
            collect_ms = timed(lambda: rt.RayHitsCollect(T, N, root, count, rays, offsets, hits, counts=counts, status=st),
                               a.iters, a.warmup)
            longest, status = int(counts.max().item()), rt.ray_hits_status(st)
            del hits
            hits = torch.empty((nr * K, 4), dtype=torch.float32, device="cuda")
            fixed_ms = timed(lambda: rt.RayHitsCollect(T, N, root, count, rays, fixed, hits, counts=counts, status=st),
                             a.iters, a.warmup)
            row[name] = {
                "rays": nr, "records": total, "mean_row": round(total / nr, 3), "longest_row": longest,
                "closest_ms": round(closest_ms, 4), "count_ms": round(count_ms, 4), "collect_ms": round(collect_ms, 4),
                "fixed_k": K, "fixed_ms": round(fixed_ms, 4),
                "count_over_closest": round(count_ms / closest_ms, 3), "collect_over_closest": round(collect_ms / closest_ms, 3),
                "fixed_over_closest": round(fixed_ms / closest_ms, 3),
                "mrays_s_count": round(nr / count_ms / 1e3, 1), "mrays_s_closest": round(nr / closest_ms / 1e3, 1),
                "box_per_ray": round(c[0] / nr, 2), "leaf_per_ray": round(c[1] / nr, 2),
                "closest_box_per_ray": round(c[4] / nr, 2), "closest_leaf_per_ray": round(c[5] / nr, 2),
                "box_ratio": round(c[0] / max(c[4], 1), 3), "status": status}
            del hits, offsets, fixed, counts, closest
        res[kind] = row
        del inp
    out = {"tool": "ray_hits_bench", "triangles": int(n), "w": w, "h": h, "camera": "A", "iters": a.iters, "warmup": a.warmup,
           "results": res, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
