"""The price of the instance filter: the filtered instanced ray query against the unfiltered one, on the same rays, in one run.

Scene and rays: tools/instance_bench.py's -- grid_mesh(177) as one BLAS, 16 instances on a 4 x 4 layout (1,002,528 instanced
triangles), 1920 x 1080 tiled camera-A rays; plus a bounce batch: one ray from every primary hit point in a random direction,
tmin = 0.  Per builder (LBVH, SAH; BLAS and TLAS built by it), closest hit, the median of --iters launches timed alone between
two device events, the arms taken in turn inside every iteration (so a drift of the machine hits all of them alike):
  camera rays   unfiltered (rt_intersect_rays_instanced: the yardstick) | keep-all (flags 0, null arrays) | cull back |
                half masked (instance k has mask 1 << (k & 1), every ray mask 1: eight of the sixteen instances are never entered)
  bounce rays   unfiltered | keep-all | skip own hit (per-ray records: all-ones mask, skip = the primary (instance, primitive))
with the spread of the timed launches (min, quartiles, max), and beside each time the box tests (both levels) and triangle
tests per ray of one counted launch, and the share of rays that hit.  No ratio is fixed in advance; the one expectation is that the half-masked arm does fewer box tests than the unfiltered
arm and is not slower.  Writes the JSON to --out (default profiles/instance_filter_bench.json) and prints it as one line, then
the table of DESIGN section 21.
Usage: python tools/instance_filter_bench.py [--iters 30] [--warmup 5] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from instance_bench import layout  # noqa: E402


def timed_in_turn(fns, iters, warmup):
    """{name: (median, min, first quartile, third quartile, max) in ms}: every iteration runs each arm once, each timed alone
    between two device events"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: tuple(float(x) for x in (np.median(v), np.min(v), np.percentile(v, 25), np.percentile(v, 75), np.max(v)))
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=177)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_filter_bench.json"))
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    G = a.grid
    blas_tris = scenes.grid_mesh(G, 1)
    nb = blas_tris.shape[0]
    inst = layout(rt, 4, G, seed=1)
    num = inst.size
    n_prims = num * nb
    cam = rt.to_device(scenes.camera_a(int(round(4.3 * G))))
    rays = torch.empty((rt.CameraRayCount(a.w, a.h, 1, True), 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, a.w, a.h, rays, tiled=True)
    nr = rays.shape[0]
    hits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(nr, dtype=torch.int32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")

    half = np.zeros(num, rt.INSTANCE_FILTER)
    half["mask"] = 1 << (np.arange(num) & 1)
    half_dev = rt.to_device(half).view(torch.int32).view(-1, 2)

    res = {}
    for name, sah in (("lbvh", False), ("sah", True)):
        root, count = (0, 1) if sah else (0, 2)

        def build(inp):
            if sah:
                rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH))
            else:
                rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kBottomUp))
        blas = rt.BuildInput.allocate(blas_tris, sah=sah)
        build(blas)
        table = rt.accel_table([(blas.triangles_out, blas.nodes_out, root, count)])
        tlas = rt.BuildInput.allocate(np.zeros((num, 9), np.float32), sah=sah)
        rec, status = rt.device_bytes(64 * num), rt.device_bytes(4)
        rt.PrepareInstances(rt.to_device(inst), num, table, 1, tlas.triangles_in, rec, status)
        build(tlas)
        torch.cuda.synchronize()
        assert rt.instance_status(status) == 0

        def query(r, flt, counters=None):
            if flt is None:
                rt.IntersectRaysInstanced(tlas.triangles_out, tlas.nodes_out, root, count, rec, num, table, 1, r, hits, ids,
                                          num_primitives=n_prims, counters=counters)
            else:
                rt.IntersectRaysInstancedFiltered(tlas.triangles_out, tlas.nodes_out, root, count, rec, num, table, 1, r, hits,
                                                  ids, flt, num_primitives=n_prims, counters=counters)

        # the bounce batch off the unfiltered primary hits (rays that miss keep their camera ray: every batch has nr rays)
        query(rays, None)
        torch.cuda.synchronize()
        h, hid, r0 = hits.cpu().numpy(), ids.cpu().numpy().view(np.uint32), rays.cpu().numpy()
        hit = hid != rt.MISS
        rng = np.random.default_rng(7)
        d = rng.normal(size=(nr, 3)).astype(np.float32)
        b = r0.copy()
        b[hit, 0:3] = r0[hit, 0:3] + h[hit, 0:1] * r0[hit, 4:7]
        b[hit, 4:7] = d[hit] / np.linalg.norm(d[hit], axis=1, keepdims=True)
        b[hit, 3], b[hit, 7] = 0.0, np.inf
        bounce = rt.to_device(b).view(torch.float32).view(-1, 8)
        own = np.zeros(nr, rt.INSTANCE_RAY_FILTER)
        own["mask"], own["skip_instance"] = 0xFFFFFFFF, hid
        own["skip_id"] = np.where(hit, h[:, 1].view(np.uint32), rt.MISS)
        own_dev = rt.to_device(own).view(torch.int32).view(-1, 4)

        arms = {"camera": (rays, {"unfiltered": None, "keep_all": rt.InstanceHitFilter(),
                                  "cull_back": rt.InstanceHitFilter(rt.RT_FILTER_CULL_BACK),
                                  "half_masked": rt.InstanceHitFilter(0, 1, half_dev)}),
                "bounce": (bounce, {"unfiltered": None, "keep_all": rt.InstanceHitFilter(),
                                    "skip_own_hit": rt.InstanceHitFilter(0, 0, None, own_dev)})}
        r = {}
        for batch, (rr, filters) in arms.items():
            ms = timed_in_turn({k: (lambda rr=rr, f=f: query(rr, f)) for k, f in filters.items()}, a.iters, a.warmup)
            r[batch] = {}
            for k, f in filters.items():
                ctr.zero_()
                query(rr, f, counters=ctr)
                torch.cuda.synchronize()
                c = ctr.cpu().numpy()
                r[batch][k] = dict(ms=round(ms[k][0], 4), ratio=round(ms[k][0] / ms["unfiltered"][0], 3),
                                   ms_min=round(ms[k][1], 4), ms_q1=round(ms[k][2], 4), ms_q3=round(ms[k][3], 4),
                                   ms_max=round(ms[k][4], 4),
                                   box_per_ray=round(int(c[0]) / nr, 2), tri_per_ray=round(int(c[1]) / nr, 2),
                                   hit_fraction=round(float((ids != -1).float().mean()), 4))
        r["half_masked_fewer_box_tests"] = bool(r["camera"]["half_masked"]["box_per_ray"] < r["camera"]["unfiltered"]["box_per_ray"])
        r["half_masked_not_slower"] = bool(r["camera"]["half_masked"]["ms"] <= r["camera"]["unfiltered"]["ms"])
        res[name] = r
        del blas, tlas
        torch.cuda.empty_cache()

    out = dict(tool="instance_filter_bench", blas_triangles=nb, instances=num, instanced_triangles=n_prims,
               rays="camera A %dx%d tiled, %d rays per batch" % (a.w, a.h, nr), iters=a.iters, warmup=a.warmup, results=res,
               device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    print("\n| builder, rays | arm | ms (ratio to unfiltered) | min .. max (quartiles) | box tests / ray | triangle tests / ray | rays that hit |")
    print("|---|---|---|---|---|---|---|")
    for name, r in res.items():
        for batch in ("camera", "bounce"):
            for k, v in r[batch].items():
                print(f"| {name}, {batch} | {k} | {v['ms']:.3f} ({v['ratio']:.3f}) | {v['ms_min']:.3f} .. {v['ms_max']:.3f} "
                      f"({v['ms_q1']:.3f}, {v['ms_q3']:.3f}) | {v['box_per_ray']} | {v['tri_per_ray']} | "
                      f"{100 * v['hit_fraction']:.1f} % |")


if __name__ == "__main__":
    main()
