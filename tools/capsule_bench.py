"""Ray queries over capsules beside ray queries over spheres of the same count and layout: prints ONE JSON line and writes it to
--out (default profiles/capsule_bench.json).

Scene: tools/sphere_bench.py's -- grid_mesh(G) (2 G^2 triangles; G = 708: 1,002,528) -- with one capsule per triangle: the first
edge as the axis, radius 0.1 of the mean edge; beside it sphere_bench's sphere scene (one sphere per triangle at the centroid,
radius 0.4 of the mean edge) through IntersectRaysSpheres.  Per builder (LBVH = RunBottomUpBuild, SAH = RunSahBuild):
  camera   1920 x 1080 tiled camera-A rays (top-down, coherent);
  bounce   one ray per camera hit, from the hit point into a random direction of the hemisphere around the surface normal (for a
           capsule: from the axis point at the record's v to the hit point), unsorted;
  mrays_closest / mrays_any   the median of --iters launches after --warmup, each timed alone between two device events,
                              counters off;
  box_per_ray / leaf_per_ray  closest-hit box tests and capsule (sphere) tests per camera ray, from one extra launch with counters.
The two scenes do not cover the same area (thin capsules along edges against fat spheres at centroids), so the rates are set
beside each other, not divided: what they price is the leaf.  Single-session medians.
RT_LIB=<path>: time another build of the library instead (e.g. `make librt_amd_exp.so EXPFLAGS=-DRT_CAPSULE_WAVES=6`).
Usage: python tools/capsule_bench.py [--grid 708] [--iters 20] [--warmup 3] [--out profiles/capsule_bench.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sphere_bench import bounce_rays, spheres_of, timed  # noqa: E402


def capsules_of(tris):
    t = tris.reshape(-1, 3, 3).astype(np.float64)
    e = (np.linalg.norm(t[:, 1] - t[:, 0], axis=1) + np.linalg.norm(t[:, 2] - t[:, 1], axis=1) +
         np.linalg.norm(t[:, 0] - t[:, 2], axis=1)) / 3
    c = np.zeros((t.shape[0], 8), np.float32)
    c[:, 0:3], c[:, 3], c[:, 4:7] = t[:, 0], 0.1 * e, t[:, 1]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capsule_bench.json"))
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if os.environ.get("RT_LIB"):
        rt.LIB_PATH = os.path.abspath(os.environ["RT_LIB"])
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    G = a.grid
    tris = scenes.grid_mesh(G, 1)
    n = tris.shape[0]
    cap_dev = rt.to_device(capsules_of(tris)).view(torch.float32).view(-1, 8)
    sph_dev = rt.to_device(spheres_of(tris)).view(torch.float32).view(-1, 4)
    cam = rt.to_device(scenes.camera_a(G))
    rays = torch.empty((rt.CameraRayCount(a.w, a.h, 1, True), 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, a.w, a.h, rays, tiled=True)
    nr = rays.shape[0]
    mr = lambda ms, k: round(k / (ms * 1e-3) / 1e6, 1)

    res = {}
    for name, sah in (("lbvh", False), ("sah", True)):
        root, count = (0, 1) if sah else (0, 2)
        r = {}
        for kind in ("capsules", "spheres"):
            tree = rt.BuildInput.allocate(np.zeros((n, 9), np.float32), sah=sah)
            status = rt.device_bytes(4)
            if kind == "capsules":
                rt.PrepareCapsules(cap_dev, n, tree.triangles_in, status)
            else:
                rt.PrepareSpheres(sph_dev, n, tree.triangles_in, status)
            if sah:
                rt.RunSahBuild(tree, rt.Arguments(build_type=rt.kSAH))
            else:
                rt.RunBottomUpBuild(tree, rt.Arguments(build_type=rt.kBottomUp))
            torch.cuda.synchronize()
            assert rt.capsule_status(status) == 0

            def q(rr, hh, any_hit=False, counters=None):
                if kind == "capsules":
                    rt.IntersectRaysCapsules(tree.triangles_out, tree.nodes_out, root, count, cap_dev, n, rr, hh, any_hit=any_hit,
                                             counters=counters)
                else:
                    rt.IntersectRaysSpheres(tree.triangles_out, tree.nodes_out, root, count, sph_dev, n, rr, hh, any_hit=any_hit,
                                            counters=counters)

            hits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
            ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
            q(rays, hits, counters=ctr)
            torch.cuda.synchronize()
            d = dict(camera=dict(rays=nr, hit_fraction=round(float((hits[:, 1].view(torch.int32) != -1).float().mean()), 4),
                                 box_per_ray=round(int(ctr[0]) / nr, 2), leaf_per_ray=round(int(ctr[1]) / nr, 2),
                                 mrays_closest=mr(timed(lambda: q(rays, hits), a.iters, a.warmup), nr),
                                 mrays_any=mr(timed(lambda: q(rays, hits, any_hit=True), a.iters, a.warmup), nr)))
            q(rays, hits)
            ids = hits[:, 1].view(torch.int32).long().clamp(min=0)
            p = rays[:, 0:3] + hits[:, 0:1] * rays[:, 4:7]
            if kind == "capsules":
                axis = cap_dev[ids, 0:3] + hits[:, 3:4] * (cap_dev[ids, 4:7] - cap_dev[ids, 0:3])
                normals = (p - axis) / cap_dev[ids, 3:4]
                hit = hits[:, 1].view(torch.int32) != -1      # body_of_hits: the share of the hits with 0 < v < 1
                d["camera"]["body_of_hits"] = round(float(((hits[hit, 3] > 0) & (hits[hit, 3] < 1)).float().mean()), 4)
            else:
                normals = (p - sph_dev[ids, 0:3]) / sph_dev[ids, 3:4]
            b = bounce_rays(rays, hits, normals, seed=3)
            nb = b.shape[0]
            bh = torch.empty((nb, 4), dtype=torch.float32, device="cuda")
            ctr.zero_()
            q(b, bh, counters=ctr)
            torch.cuda.synchronize()
            d["bounce"] = dict(rays=nb, hit_fraction=round(float((bh[:, 1].view(torch.int32) != -1).float().mean()), 4),
                               box_per_ray=round(int(ctr[0]) / nb, 2), leaf_per_ray=round(int(ctr[1]) / nb, 2),
                               mrays_closest=mr(timed(lambda: q(b, bh), a.iters, a.warmup), nb),
                               mrays_any=mr(timed(lambda: q(b, bh, any_hit=True), a.iters, a.warmup), nb))
            r[kind] = d
            del tree
            torch.cuda.empty_cache()
        res[name] = r
    line = json.dumps(dict(tool="capsule_bench", library=os.path.basename(rt.LIB_PATH), primitives=n,
                           rays="camera A %dx%d tiled + one bounce" % (a.w, a.h), iters=a.iters, warmup=a.warmup,
                           note="single-session medians", results=res, device=torch.cuda.get_device_name(0)))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
