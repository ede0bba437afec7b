"""Motion-query throughput against the static ray query of the same build: prints a table and ONE JSON line.

Scene: grid_mesh(708) = 1,002,528 triangles (the bench mesh), camera A, 1920 x 1080 camera rays in 8x8-tile order, counters
off.  Pose 1 is a smooth displacement of the mesh (p + 0.05 E sin(3 q.yzx), q = (p - lo) / E: a function of position), made
by MotionPose.  Trees: LBVH and SAH; closest-hit and any-hit.  Four arms per tree and mode:
  static       rt_intersect_rays on pose 0 (the yardstick)
  motion_t0    rt_intersect_rays_motion, every time 0 (the same records: what the second pose's fetches and the interpolation cost)
  motion_half  every time 0.5 (one shared time: the rays of a wave see one geometry)
  motion_rand  one uniform random time per ray (seeded)
Each launch is timed alone between two device events.  The arms are run in --rounds rounds, alternating, each round the median of
--iters launches after --warmup; the table gives the median over the rounds and their spread, and the ratio to `static`.
RT_LIB=<path>: time another build of the library instead (tools/point_query_bench.py's override; the occupancy arm of DESIGN
section 22 is `make librt_amd_exp.so EXPFLAGS=-DRT_MOTION_WAVES=6`).
Usage: python tools/motion_bench.py [--iters 20] [--warmup 3] [--rounds 3] [--grid 708] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def smooth(tris, amp=0.05):
    P = tris.reshape(-1, 3).astype(np.float64)
    lo, E = P.min(axis=0), float(np.ptp(P, axis=0).max()) or 1.0
    q = (P - lo) / E
    return (P + amp * E * np.sin(3.0 * q[:, [1, 2, 0]])).astype(np.float32).reshape(-1, 9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if os.environ.get("RT_LIB"):
        rt.LIB_PATH = os.path.abspath(os.environ["RT_LIB"])
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    tris = scenes.grid_mesh(a.grid, 1)
    n = tris.shape[0]
    moved = smooth(tris)
    cam = rt.to_device(scenes.camera_a(a.grid))
    w, h = a.w, a.h
    nr = rt.CameraRayCount(w, h, 1, True)
    rays = torch.empty((nr, 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, w, h, rays, tiled=True)
    hits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    check = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    times = {"motion_t0": torch.zeros(nr, dtype=torch.float32, device="cuda"),
             "motion_half": torch.full((nr,), 0.5, dtype=torch.float32, device="cuda"),
             "motion_rand": torch.from_numpy(np.random.default_rng(1).random(nr, dtype=np.float32)).cuda()}
    res, lines = {}, []
    for tree in ("lbvh", "sah"):
        if tree == "lbvh":
            inp = rt.BuildInput.allocate(tris)
            rt.RunBottomUpBuild(inp)
            root, count = 0, 2
        else:
            inp = rt.BuildInput.allocate(tris, sah=True)
            rt.RunSahBuild(inp)
            root, count = 0, 1
        pose1, plan = rt.MotionPose(inp, root, count, moved)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        rt.MotionValidate(inp, pose1, root, count, n, status)
        assert rt.refit_status(plan, n) == 0 and rt.motion_status(status) == 0
        T, N = inp.triangles_out, inp.nodes_out
        for anyh in (False, True):
            arms = {"static": lambda: rt.IntersectRays(T, N, root, count, rays, hits, any_hit=anyh, num_primitives=n)}
            for name, t in times.items():
                arms[name] = lambda t=t: rt.IntersectRaysMotion(inp, pose1, root, count, rays, t, hits, any_hit=anyh)
            # the same records at time 0 (numbers: a zero's sign may differ)
            rt.IntersectRays(T, N, root, count, rays, check, any_hit=anyh, num_primitives=n)
            arms["motion_t0"]()
            torch.cuda.synchronize()
            assert torch.equal(hits.view(torch.int32)[:, 1], check.view(torch.int32)[:, 1]), "primitive ids at time 0"
            assert bool((hits[:, [0, 2, 3]] == check[:, [0, 2, 3]]).all()), "t, u, v at time 0"
            ms = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    ms[k].append(timed(fn, a.iters, a.warmup))
            mode = "any" if anyh else "closest"
            base = float(np.median(ms["static"]))
            for k in arms:
                med = float(np.median(ms[k]))
                res[f"{tree}_{mode}_{k}"] = dict(ms=round(med, 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4),
                                                 mrays_s=round(nr / (med * 1e-3) / 1e6, 1), ratio_to_static=round(med / base, 3))
                lines.append(f"{tree:5s} {mode:8s} {k:12s} {med:8.4f} ms  [{min(ms[k]):.4f} .. {max(ms[k]):.4f}]  "
                             f"{nr / (med * 1e-3) / 1e6:8.1f} Mrays/s  x{med / base:.3f}")
    head = (f"motion_bench: {n} triangles, {w} x {h} camera A, {nr} tiled rays, {a.rounds} rounds x median of {a.iters} "
            f"launches, {os.path.basename(rt.LIB_PATH)}, {torch.cuda.get_device_name(0)}\n"
            "tree  mode     arm          median        [rounds' min .. max]        rate      vs static")
    text = head + "\n" + "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps(dict(tool="motion_bench", triangles=n, w=w, h=h, camera="A", rays=nr, iters=a.iters, warmup=a.warmup,
                          rounds=a.rounds, results=res, device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
