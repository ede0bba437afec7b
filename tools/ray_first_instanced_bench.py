"""Instanced first-K ray queries beside the three calls a caller could use instead, on the same geometry and rays: prints ONE
JSON line (and writes it to --out).

Scene: tools/instance_bench.py's -- grid_mesh(177) (62,658 triangles) as one BLAS, 16 instances on a 4 x 4 layout with small
distinct rotations, the same world-space triangles flattened into one tree.  Two ray sets: the 1920 x 1080 tiled camera-A frame
(top-down over the whole layout) and one diffuse bounce from its primary hits (tools/ray_query_bench.py's batch off the
flattened tree, tmax = +inf).  Per builder (LBVH = RunBottomUpBuild, SAH = RunSahBuild; the BLAS, the TLAS and the flattened tree
each built by it) and ray set, for k in {1, 4, 32}, each figure the median of --iters launches timed alone between two device
events after --warmup launches:
  instanced   RayFirstHitsInstanced: ms, Mrays/s, slot tests and BLAS leaf visits per ray (one further launch with counters)
  flattened   RayFirstHits on the flattened tree: the yardstick instancing is meant to avoid; ratio = instanced rate /
              flattened rate (DESIGN sections 9 and 29 measured 0.50 to 0.60 for closest hit and all hits)
  closest     IntersectRaysInstanced, closest hit (per ray set): what the two-level walk costs without a list
  sorted      RayHitsInstanced(sort=True): count, read-back, allocation, collect and three torch sorts -- the composition this
              call replaces, host synchronisation included (host clocks, --sorted-iters runs; the cut of its rows to k is NOT
              included, so the figure is a lower bound of the composition)
--lib measures another build of the library, e.g. another launch bound of the kernel:
  make -C gpu-raytracing_amd/csrc librt_amd_exp.so EXPFLAGS=-DRT_RAY_FIRST_INSTANCED_WAVES=6 EXPNAME=librt_amd_rfi6.so
Usage: python tools/ray_first_instanced_bench.py [--iters 30] [--warmup 5] [--lib LIBRARY]
                                                 [--out profiles/ray_first_instanced_bench.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from instance_bench import layout, timed   # noqa: E402
from ray_query_bench import bounce_rays    # noqa: E402

KS = (1, 4, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sorted-iters", type=int, default=3)
    ap.add_argument("--grid", type=int, default=177)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--out", default="")
    ap.add_argument("--lib", default="", help="another build of the library (csrc/Makefile's librt_amd_exp.so)")
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if a.lib:
        rt.LIB_PATH = os.path.abspath(a.lib)
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    G = a.grid
    blas_tris = scenes.grid_mesh(G, 1)
    nb = blas_tris.shape[0]
    inst = layout(rt, 4, G, seed=1)
    M = inst["object_to_world"].astype(np.float64)
    T = blas_tris.reshape(-1, 3, 3).astype(np.float64)
    flat = np.concatenate([(T @ m[:, :3].T + m[:, 3]).reshape(-1, 9) for m in M]).astype(np.float32)
    n = flat.shape[0]
    cam = rt.to_device(scenes.camera_a(int(round(4.3 * G))))
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def build(inp, sah):
        if sah:
            rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH))
        else:
            rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kBottomUp))

    def counted(fn):
        """one launch with counters -> (slot tests, leaf visits, status)"""
        ctr.zero_()
        st.zero_()
        fn(counters=ctr, status=st)
        torch.cuda.synchronize()
        c = ctr.cpu().numpy()
        return int(c[0]), int(c[1]), int(st.item())

    res, sets = {}, {}
    for name, sah in (("lbvh", False), ("sah", True)):
        root, count = (0, 1) if sah else (0, 2)
        blas = rt.BuildInput.allocate(blas_tris, sah=sah)
        build(blas, sah)
        table = rt.accel_table([(blas.triangles_out, blas.nodes_out, root, count)])
        tlas = rt.BuildInput.allocate(np.zeros((16, 9), np.float32), sah=sah)
        rec, status = rt.device_bytes(64 * 16), rt.device_bytes(4)
        rt.PrepareInstances(rt.to_device(inst), 16, table, 1, tlas.triangles_in, rec, status)
        build(tlas, sah)
        fl = rt.BuildInput.allocate(flat, sah=sah)
        build(fl, sah)
        torch.cuda.synchronize()
        assert rt.instance_status(status) == 0
        two = (tlas.triangles_out, tlas.nodes_out, root, count, rec, 16, table, 1)
        one = (fl.triangles_out, fl.nodes_out, root, count)
        if not sets:                               # the rays do not depend on the builder
            tiled = torch.empty((rt.CameraRayCount(a.w, a.h, 1, True), 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(cam, a.w, a.h, tiled, tiled=True)
            row_major = torch.empty((a.w * a.h, 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(cam, a.w, a.h, row_major)
            prim = torch.empty((a.w * a.h, 4), dtype=torch.float32, device="cuda")
            rt.IntersectRays(*one, row_major, prim, num_primitives=n)
            torch.cuda.synchronize()
            sets = {"camera_a_tiled": tiled, "bounce": bounce_rays(rt, row_major, prim, flat)[0]}
            del row_major, prim
        row = {}
        for sname, rays in sets.items():
            nr = rays.shape[0]
            rate = lambda ms: round(nr / ms / 1e3, 1)
            chits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
            cids = torch.empty(nr, dtype=torch.int32, device="cuda")
            closest_ms = timed(lambda: rt.IntersectRaysInstanced(*two, rays, chits, cids, num_primitives=n), a.iters, a.warmup)
            ctr.zero_()
            rt.IntersectRaysInstanced(*two, rays, chits, cids, num_primitives=n, counters=ctr)
            torch.cuda.synchronize()
            c = ctr.cpu().numpy()
            cell = {"rays": nr, "closest": {"ms": round(closest_ms, 4), "mrays_s": rate(closest_ms),
                                            "box_per_ray": round(int(c[0]) / nr, 2), "leaf_per_ray": round(int(c[1]) / nr, 2),
                                            "hit_fraction": round(float((cids != -1).float().mean()), 4)}}
            rt.RayHitsInstanced(*two, rays, sort=True)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.sorted_iters):
                t0 = time.perf_counter()
                off, hits, ids = rt.RayHitsInstanced(*two, rays, sort=True)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            lens = off[1:] - off[:-1]
            cell["sorted"] = {"ms": round(float(np.median(ts)), 4), "records": int(hits.shape[0]),
                              "mean_row": round(hits.shape[0] / nr, 3), "longest_row": int(lens.max().item())}
            del off, hits, ids, lens
            out = torch.empty((nr, max(KS), 4), dtype=torch.float32, device="cuda")
            oid = torch.empty((nr, max(KS)), dtype=torch.int32, device="cuda")
            for k in KS:
                o = out.view(-1)[:nr * k * 4].view(nr, k, 4)
                oi = oid.view(-1)[:nr * k].view(nr, k)
                ms = timed(lambda: rt.RayFirstHitsInstanced(*two, rays, k, o, oi), a.iters, a.warmup)
                box, leaf, s1 = counted(lambda **kw: rt.RayFirstHitsInstanced(*two, rays, k, o, oi, **kw))
                live = int((oi != -1).sum().item())
                flat_ms = timed(lambda: rt.RayFirstHits(*one, rays, k, o), a.iters, a.warmup)
                fbox, fleaf, s2 = counted(lambda **kw: rt.RayFirstHits(*one, rays, k, o, **kw))
                cell[f"k{k}"] = {"instanced": {"ms": round(ms, 4), "mrays_s": rate(ms), "box_per_ray": round(box / nr, 2),
                                               "leaf_per_ray": round(leaf / nr, 2), "status": s1,
                                               "live_records_per_ray": round(live / nr, 3)},
                                 "flattened": {"ms": round(flat_ms, 4), "mrays_s": rate(flat_ms), "box_per_ray": round(fbox / nr, 2),
                                               "leaf_per_ray": round(fleaf / nr, 2), "status": s2},
                                 "ratio_instanced_over_flattened": round(flat_ms / ms, 3),
                                 "rate_over_closest": round(closest_ms / ms, 3),
                                 "time_over_sorted": round(ms / cell["sorted"]["ms"], 4)}
            del out, oid, chits, cids
            row[sname] = cell
        res[name] = row
        del blas, fl, tlas
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="ray_first_instanced_bench", library=os.path.basename(a.lib or "librt_amd.so"), blas_triangles=nb, instances=16, instanced_triangles=16 * nb,
                           rays="camera A %dx%d tiled + one diffuse bounce" % (a.w, a.h), ks=list(KS), iters=a.iters,
                           warmup=a.warmup, sorted_iters=a.sorted_iters, runs=1, results=res,
                           device=torch.cuda.get_device_name(0)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
