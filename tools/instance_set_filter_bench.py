"""The filtered instanced all-hit and first-K ray queries beside their unfiltered siblings of the same library, on the same
geometry and rays: prints ONE JSON line (and writes it to --out).

Scene and rays: tools/ray_hits_instanced_bench.py's and tools/ray_first_instanced_bench.py's -- grid_mesh(177) (62,658
triangles) as one BLAS, 16 instances on a 4 x 4 layout with small distinct rotations; the 1920 x 1080 tiled camera-A frame and
one diffuse bounce from the primary hits of its row-major twin.  Per builder (LBVH, SAH) and ray set, for count, collect into
the counted offsets, fixed K = 4 and first-K at k in {1, 4, 32}, each figure the median of --iters launches timed alone between
two device events after --warmup launches, with the slot tests and BLAS leaf visits per ray of one further launch beside it:
  unfiltered  the sibling entry points: the code of the parent commit (profiles/instance_set_filter_asm_diff.txt)
  keep_all    a filter that keeps everything (flags 0, null arrays): the price of the FILTERED arm itself
  cull_back   RT_FILTER_CULL_BACK
  half        every odd instance masked out (per_instance masks): its counters must drop against unfiltered (asserted); its
              time is only reported
  skip        (bounce rays only) every ray leaves out the (instance, primitive) it starts on, from the instanced closest hit
              of its parent
--lib measures another build of the library, e.g. other launch bounds of the FILTERED arms:
  make -C gpu-raytracing_amd/csrc librt_amd_exp.so EXPNAME=librt_amd_isf5.so EXPFLAGS="-DRT_RAY_HITS_INSTANCED_COUNT_FILTERED_WAVES=5
      -DRT_RAY_HITS_INSTANCED_COLLECT_FILTERED_WAVES=4 -DRT_RAY_FIRST_INSTANCED_FILTERED_WAVES=5"
Usage: python tools/instance_set_filter_bench.py [--iters 30] [--warmup 5] [--lib LIBRARY]
                                                 [--out profiles/instance_set_filter_bench.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from instance_bench import layout, timed   # noqa: E402
from ray_query_bench import bounce_rays    # noqa: E402

KS = (1, 4, 32)
FIXED_K = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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

    half = torch.from_numpy(np.stack([np.where(np.arange(16) % 2 == 0, 1, 2), np.zeros(16)], axis=1).astype(np.int32)).cuda()
    res, sets, skips = {}, {}, {}
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
        two = (tlas.triangles_out, tlas.nodes_out, root, count, rec, 16, table, 1)
        if not sets:                               # the rays do not depend on the builder
            tiled = torch.empty((rt.CameraRayCount(a.w, a.h, 1, True), 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(cam, a.w, a.h, tiled, tiled=True)
            row_major = torch.empty((a.w * a.h, 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(cam, a.w, a.h, row_major)
            prim = torch.empty((a.w * a.h, 4), dtype=torch.float32, device="cuda")
            pids = torch.empty(a.w * a.h, dtype=torch.int32, device="cuda")
            rt.IntersectRaysInstanced(*two, row_major, prim, pids, num_primitives=n)
            torch.cuda.synchronize()
            # the bounce batch needs the hit triangle's corners: the flattened id of (instance, primitive) is instance * nb + id
            flat_hits = prim.clone()
            fid = pids.to(torch.int64) * nb + (prim.view(torch.int32)[:, 1].to(torch.int64) & 0xFFFFFFFF)
            flat_hits.view(torch.int32)[:, 1] = torch.where(pids >= 0, fid, torch.full_like(fid, -1)).to(torch.int32)
            sets = {"camera_a_tiled": tiled, "bounce": bounce_rays(rt, row_major, flat_hits, flat)[0]}
            per_ray = torch.zeros((a.w * a.h, 4), dtype=torch.int32, device="cuda")
            per_ray[:, 0] = -1                         # all-ones mask
            per_ray[:, 1] = pids                       # the parent's instance (RT_MISS where it missed: the ray is dead anyway)
            per_ray[:, 2] = prim.view(torch.int32)[:, 1]
            skips = {"bounce": per_ray}
            del row_major, prim, pids, flat_hits, fid
        row = {}
        for sname, rays in sets.items():
            nr = rays.shape[0]
            rate = lambda ms: round(nr / ms / 1e3, 1)
            arms = {"unfiltered": "unfiltered", "keep_all": rt.InstanceHitFilter(), "cull_back": rt.InstanceHitFilter(flags=1),
                    "half": rt.InstanceHitFilter(ray_mask=1, per_instance=half)}
            if sname in skips:
                arms["skip"] = rt.InstanceHitFilter(ray_mask=0, per_ray=skips[sname])
            offsets = torch.empty(nr + 1, dtype=torch.int64, device="cuda")
            fixed = torch.arange(nr + 1, dtype=torch.int64, device="cuda") * FIXED_K
            scratch = rt.device_bytes(rt.RayHitsScratchBytes(nr))
            counts = torch.empty(nr, dtype=torch.int32, device="cuda")
            hits_k = torch.empty((nr * FIXED_K, 4), dtype=torch.float32, device="cuda")
            ids_k = torch.empty(nr * FIXED_K, dtype=torch.int32, device="cuda")
            out = torch.empty((nr, max(KS), 4), dtype=torch.float32, device="cuda")
            oid = torch.empty((nr, max(KS)), dtype=torch.int32, device="cuda")
            cell = {"rays": nr}
            for aname, flt in arms.items():
                if flt == "unfiltered":
                    cnt = lambda off, **kw: rt.RayHitsCountInstanced(*two, rays, off, **kw)
                    col = lambda off, *o, **kw: rt.RayHitsCollectInstanced(*two, rays, off, *o, **kw)
                    fst = lambda k, o, oi, **kw: rt.RayFirstHitsInstanced(*two, rays, k, o, oi, **kw)
                else:
                    cnt = lambda off, flt=flt, **kw: rt.RayHitsCountInstancedFiltered(*two, rays, flt, off, **kw)
                    col = lambda off, *o, flt=flt, **kw: rt.RayHitsCollectInstancedFiltered(*two, rays, flt, off, *o, **kw)
                    fst = lambda k, o, oi, flt=flt, **kw: rt.RayFirstHitsInstancedFiltered(*two, rays, k, flt, o, oi, **kw)
                box, leaf, s0 = counted(lambda **kw: cnt(offsets, scratch=scratch, **kw))
                total = int(offsets[nr].item())
                hits = torch.empty((max(total, 1), 4), dtype=torch.float32, device="cuda")
                ids = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
                d = {"records": total, "mean_row": round(total / nr, 4), "box_per_ray": round(box / nr, 3),
                     "leaf_per_ray": round(leaf / nr, 3), "status": s0,
                     "count_ms": round(timed(lambda: cnt(offsets, scratch=scratch), a.iters, a.warmup), 4),
                     "collect_ms": round(timed(lambda: col(offsets, hits, ids), a.iters, a.warmup), 4),
                     "fixed_k_ms": round(timed(lambda: col(fixed, hits_k, ids_k, counts=counts), a.iters, a.warmup), 4)}
                del hits, ids
                for k in KS:
                    o = out.view(-1)[:nr * k * 4].view(nr, k, 4)
                    oi = oid.view(-1)[:nr * k].view(nr, k)
                    ms = timed(lambda: fst(k, o, oi), a.iters, a.warmup)
                    fbox, fleaf, s1 = counted(lambda **kw: fst(k, o, oi, **kw))
                    d[f"first_k{k}"] = {"ms": round(ms, 4), "mrays_s": rate(ms), "box_per_ray": round(fbox / nr, 3),
                                        "leaf_per_ray": round(fleaf / nr, 3), "status": s1}
                cell[aname] = d
            base = cell["unfiltered"]
            for aname in arms:
                if aname == "unfiltered":
                    continue
                d = cell[aname]
                d["time_over_unfiltered"] = {key: round(d[key] / base[key], 3) for key in ("count_ms", "collect_ms", "fixed_k_ms")}
                for k in KS:
                    d["time_over_unfiltered"][f"first_k{k}"] = round(d[f"first_k{k}"]["ms"] / base[f"first_k{k}"]["ms"], 3)
            # the condition: a half-masked scene examines fewer slots and visits fewer leaves, in every call
            h = cell["half"]
            assert h["box_per_ray"] < base["box_per_ray"] and h["leaf_per_ray"] < base["leaf_per_ray"], (sname, h, base)
            for k in KS:
                assert h[f"first_k{k}"]["box_per_ray"] < base[f"first_k{k}"]["box_per_ray"], (sname, k)
                assert h[f"first_k{k}"]["leaf_per_ray"] < base[f"first_k{k}"]["leaf_per_ray"], (sname, k)
            # keep-all examines exactly what the sibling examines
            ka = cell["keep_all"]
            assert (ka["records"], ka["box_per_ray"], ka["leaf_per_ray"]) == (base["records"], base["box_per_ray"], base["leaf_per_ray"])
            del offsets, fixed, scratch, counts, hits_k, ids_k, out, oid
            row[sname] = cell
        res[name] = row
        del blas, tlas
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="instance_set_filter_bench", library=os.path.basename(a.lib or "librt_amd.so"), blas_triangles=nb,
                           instances=16, instanced_triangles=16 * nb,
                           rays="camera A %dx%d tiled + one diffuse bounce" % (a.w, a.h), fixed_k=FIXED_K, ks=list(KS),
                           iters=a.iters, warmup=a.warmup, runs=1, results=res, device=torch.cuda.get_device_name(0)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
