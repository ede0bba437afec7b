"""Sphere casts beside ray queries on the same tree and the same rays: prints ONE JSON line and writes it to --out (default
profiles/sphere_cast_bench.json).

Scene: tools/sphere_bench.py's -- grid_mesh(G) (2 G^2 triangles; G = 708: 1,002,528).  Per builder (LBVH = RunBottomUpBuild,
SAH = RunSahBuild):
  camera   1920 x 1080 tiled camera-A rays (top-down, coherent);
  bounce   one ray per camera hit of the ray query, from the hit point into a random direction of the hemisphere around the
           triangle's normal, unsorted.  With a radius these rays begin 1e-3 above the surface, so nearly all of them begin in
           contact: the row prices the overlap exit, not a sweep (overlap_fraction says how many);
  rows     "rays" = IntersectRays; "r=0", "r=0.1", "r=1", "r=10" = SphereCast with that uniform radius in mean edge lengths;
  mrays_closest / mrays_any   the median of --iters launches after --warmup, each timed alone between two device events,
                              counters off;
  box_per_ray / leaf_per_ray  closest-hit box tests and leaf visits per ray, from one extra launch with counters.
The rows are set beside each other and not divided: growing the boxes legitimately costs box tests.  Single-session medians.
RT_LIB=<path>: time another build of the library instead (e.g. `make librt_amd_exp.so EXPFLAGS=-DRT_SPHERE_CAST_WAVES=6`).
Usage: python tools/sphere_cast_bench.py [--grid 708] [--iters 20] [--warmup 3] [--out profiles/sphere_cast_bench.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sphere_bench import bounce_rays, timed  # noqa: E402

RADII = (0.0, 0.1, 1.0, 10.0)      # in mean edge lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sphere_cast_bench.json"))
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if os.environ.get("RT_LIB"):
        rt.LIB_PATH = os.path.abspath(os.environ["RT_LIB"])
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    G = a.grid
    tris = scenes.grid_mesh(G, 1)
    n = tris.shape[0]
    t64 = tris.reshape(-1, 3, 3).astype(np.float64)
    edge = float((np.linalg.norm(t64[:, 1] - t64[:, 0], axis=1) + np.linalg.norm(t64[:, 2] - t64[:, 1], axis=1) +
                  np.linalg.norm(t64[:, 0] - t64[:, 2], axis=1)).mean() / 3)
    nrm = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    normals_dev = rt.to_device(np.ascontiguousarray(nrm, np.float32)).view(torch.float32).view(-1, 3)
    cam = rt.to_device(scenes.camera_a(G))
    rays = torch.empty((rt.CameraRayCount(a.w, a.h, 1, True), 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, a.w, a.h, rays, tiled=True)
    mr = lambda ms, k: round(k / (ms * 1e-3) / 1e6, 1)

    res = {}
    for name, sah in (("lbvh", False), ("sah", True)):
        root, count = (0, 1) if sah else (0, 2)
        tree = rt.BuildInput.allocate(tris, sah=sah)
        if sah:
            rt.RunSahBuild(tree, rt.Arguments(build_type=rt.kSAH))
        else:
            rt.RunBottomUpBuild(tree, rt.Arguments(build_type=rt.kBottomUp))
        torch.cuda.synchronize()

        def q(radius, rr, hh, any_hit=False, counters=None, features=None):
            if radius is None:
                rt.IntersectRays(tree.triangles_out, tree.nodes_out, root, count, rr, hh, any_hit=any_hit, num_primitives=n,
                                 counters=counters)
            else:
                rt.SphereCast(tree.triangles_out, tree.nodes_out, root, count, rr, hh, radius=radius * edge, features=features,
                              any_hit=any_hit, counters=counters)

        def rows(rr):
            k = rr.shape[0]
            hh = torch.empty((k, 4), dtype=torch.float32, device="cuda")
            feats = torch.zeros(k, dtype=torch.int32, device="cuda")
            ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
            out = {}
            for label, radius in [("rays", None)] + [("r=%g" % r, r) for r in RADII]:
                ctr.zero_()
                q(radius, rr, hh, counters=ctr, features=feats)
                torch.cuda.synchronize()
                d = dict(hit_fraction=round(float((hh[:, 1].view(torch.int32) != -1).float().mean()), 4),
                         box_per_ray=round(int(ctr[0]) / k, 2), leaf_per_ray=round(int(ctr[1]) / k, 2),
                         mrays_closest=mr(timed(lambda: q(radius, rr, hh), a.iters, a.warmup), k),
                         mrays_any=mr(timed(lambda: q(radius, rr, hh, any_hit=True), a.iters, a.warmup), k))
                if radius is not None:
                    d["overlap_fraction"] = round(float((feats == rt.RT_SWEEP_OVERLAP).float().mean()), 4)
                out[label] = d
            return out

        r = dict(camera=dict(num_rays=rays.shape[0], **rows(rays)))
        hits = torch.empty((rays.shape[0], 4), dtype=torch.float32, device="cuda")
        q(None, rays, hits)
        ids = hits[:, 1].view(torch.int32).long().clamp(min=0)
        b = bounce_rays(rays, hits, normals_dev[ids], seed=3)
        r["bounce"] = dict(num_rays=b.shape[0], **rows(b))
        res[name] = r
        del tree
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="sphere_cast_bench", library=os.path.basename(rt.LIB_PATH), primitives=n,
                           mean_edge=round(edge, 4), rays="camera A %dx%d tiled + one bounce" % (a.w, a.h), iters=a.iters,
                           warmup=a.warmup, note="single-session medians; rows beside each other, not divided", results=res,
                           device=torch.cuda.get_device_name(0)))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
