"""The price of instance motion: IntersectRaysInstancedMotion on a scene of moving instances against IntersectRaysInstanced on
its pose-0 scene, the same rays.  Prints ONE JSON line.

Scene: tools/instance_bench.py's -- grid_mesh(177) (62,658 triangles) as one BLAS, 16 instances on a 4 x 4 layout with small
distinct rotations; pose 1 turns every instance by up to 0.15 rad about its own centre and shifts it by up to 0.1 of its
extent.  1920 x 1080 tiled camera-A rays, top-down over the whole layout.  Per builder (LBVH / SAH: BLAS and TLAS built by it;
TLAS pose 1 = a byte copy refitted with proxies1):
  static              IntersectRaysInstanced over PrepareInstances(pose 0)
  time0 / shared / random   IntersectRaysInstancedMotion with every time 0, every time 0.5, one uniform random time per ray
each closest-hit and any-hit, ms = the median of --iters launches timed alone between two device events, Mrays/s from it, the
ratio to `static`, and the box / triangle tests per ray of the closest-hit call from the counters.
RT_LIB=<path>: time another build of the library instead (`make librt_amd_exp.so EXPFLAGS=-DRT_INSTANCE_MOTION_WAVES=5`).
Usage: python tools/instance_motion_bench.py [--iters 30] [--warmup 5]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from instance_bench import layout, rotation, timed  # noqa: E402


def moved(inst0, G, seed):
    """pose 1 of instance_bench.layout's instances: a further small rotation about each instance's centre and a shift"""
    rng = np.random.default_rng(seed)
    c = np.array([G / 2, 1.0, G / 2])
    out = inst0["object_to_world"].astype(np.float64).copy()
    for k in range(out.shape[0]):
        M = out[k]
        wc = M[:, :3] @ c + M[:, 3]
        R = rotation(*rng.uniform(-0.15, 0.15, 3) / np.sqrt(3))
        out[k] = np.hstack([R @ M[:, :3], (wc + R @ (M[:, 3] - wc) + rng.uniform(-0.1, 0.1, 3) * G)[:, None]])
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=177)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if os.environ.get("RT_LIB"):
        rt.LIB_PATH = os.path.abspath(os.environ["RT_LIB"])
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    G = a.grid
    blas_tris = scenes.grid_mesh(G, 1)
    nb = blas_tris.shape[0]
    inst0 = layout(rt, 4, G, seed=1)
    k = inst0.size
    minst = np.zeros(k, rt.MOTION_INSTANCE)
    minst["object_to_world0"], minst["object_to_world1"] = inst0["object_to_world"], moved(inst0, G, seed=3)
    cam = rt.to_device(scenes.camera_a(int(round(4.3 * G))))
    rays = torch.empty((rt.CameraRayCount(a.w, a.h, 1, True), 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, a.w, a.h, rays, tiled=True)
    nr = rays.shape[0]
    hits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(nr, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(7)
    times = dict(time0=torch.zeros(nr, device="cuda"), shared=torch.full((nr,), 0.5, device="cuda"),
                 random=torch.rand(nr, device="cuda", generator=gen))

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
        status = rt.device_bytes(4)
        # the static scene: pose 0
        tlas_s = rt.BuildInput.allocate(np.zeros((k, 9), np.float32), sah=sah)
        rec_s = rt.device_bytes(64 * k)
        rt.PrepareInstances(rt.to_device(inst0), k, table, 1, tlas_s.triangles_in, rec_s, status)
        build(tlas_s)
        assert rt.instance_status(status) == 0
        # the moving scene: TLAS over proxies0, its copy refitted with proxies1
        tlas0 = rt.BuildInput.allocate(np.zeros((k, 9), np.float32), sah=sah)
        prox1 = torch.zeros_like(tlas0.triangles_in)
        rec_m = rt.device_bytes(128 * k)
        rt.PrepareMotionInstances(rt.to_device(minst), k, table, 1, tlas0.triangles_in, prox1, rec_m, status)
        build(tlas0)
        tlas1, plan = rt.MotionPose(tlas0, root, count, prox1)
        torch.cuda.synchronize()
        assert rt.instance_status(status) == 0 and rt.refit_status(plan, k) == 0

        def q_static(any_hit, counters=None):
            rt.IntersectRaysInstanced(tlas_s.triangles_out, tlas_s.nodes_out, root, count, rec_s, k, table, 1, rays, hits, ids,
                                      any_hit=any_hit, counters=counters)

        def q_motion(tm, any_hit, counters=None):
            rt.IntersectRaysInstancedMotion(tlas0, tlas1, root, count, rec_m, k, table, 1, rays, tm, hits, ids, any_hit=any_hit,
                                            counters=counters)

        def measure(fn):
            out = {}
            for mode, any_hit in (("closest", False), ("any", True)):
                ms = timed(lambda: fn(any_hit), a.iters, a.warmup)
                out[mode] = dict(ms=round(ms, 4), mrays=round(nr / (ms * 1e-3) / 1e6, 1))
            ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
            fn(False, ctr)
            torch.cuda.synchronize()
            out.update(box_per_ray=round(int(ctr[0]) / nr, 2), tri_per_ray=round(int(ctr[1]) / nr, 2),
                       hit_fraction=round(float((ids != -1).float().mean()), 4))
            return out

        r = dict(static=measure(q_static))
        for arm, tm in times.items():
            r[arm] = measure(lambda any_hit, counters=None, tm=tm: q_motion(tm, any_hit, counters))
            for mode in ("closest", "any"):
                r[arm][mode]["ratio_to_static"] = round(r[arm][mode]["ms"] / r["static"][mode]["ms"], 3)
        res[name] = r
        del blas, tlas_s, tlas0, tlas1
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool="instance_motion_bench", lib=os.path.basename(rt.LIB_PATH), blas_triangles=nb, instances=k,
                          instanced_triangles=k * nb, rays="camera A %dx%d tiled" % (a.w, a.h), iters=a.iters, warmup=a.warmup, results=res,
                          device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
