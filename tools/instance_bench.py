"""Instanced vs flattened ray queries on the same geometry, and the per-frame price of rigid motion: prints ONE JSON line.

Scene: grid_mesh(177) (62,658 triangles) as one BLAS, 16 instances on a 4 x 4 layout with small distinct rotations
(1,002,528 instanced triangles), against the same world-space triangles flattened into one mesh built as one tree.  Per builder
(LBVH = RunBottomUpBuild, SAH = RunSahBuild; the BLAS, the TLAS and the flattened tree each built by it):
  mrays_closest / mrays_any   1920 x 1080 tiled camera-A rays (top-down over the whole layout) through
                              IntersectRaysInstanced (instanced) or IntersectRays (flattened), each the median of --iters
                              launches timed alone between two device events
  box_per_ray / tri_per_ray   closest-hit box tests (both levels) and triangle tests per ray, from the counters
  tree_bytes                  the buffers the trees need: 64 B per leaf record + rt_nodes_bytes per tree (+ 64 B instance
                              records and 24 B table entries for the instanced scene)
  ratio                       instanced / flattened closest-hit rate (the goal: >= 0.75)
Rigid motion: PrepareInstances + the TLAS rebuild, for 16 and 65,536 instances (a 256 x 256 layout of the same BLAS), median
of --iters frames.
Usage: python tools/instance_bench.py [--iters 30] [--warmup 5]"""
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


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def layout(rt, side, G, seed):
    """side x side instances of a G-cell grid, spaced 1.1 G apart, each turned by a small distinct rotation about its centre"""
    rng = np.random.default_rng(seed)
    inst = np.zeros(side * side, rt.INSTANCE)
    c = np.array([G / 2, 1.0, G / 2])
    for k in range(side * side):
        R = rotation(*rng.uniform(-0.08, 0.08, 3))
        t = np.array([(k % side) * 1.1 * G, 0.0, (k // side) * 1.1 * G]) + c - R @ c
        inst["object_to_world"][k] = np.hstack([R, t[:, None]]).astype(np.float32)
    return inst


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
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    G = a.grid
    blas_tris = scenes.grid_mesh(G, 1)
    nb = blas_tris.shape[0]
    inst = layout(rt, 4, G, seed=1)
    M = inst["object_to_world"].astype(np.float64)
    T = blas_tris.reshape(-1, 3, 3).astype(np.float64)
    flat = np.concatenate([(T @ m[:, :3].T + m[:, 3]).reshape(-1, 9) for m in M]).astype(np.float32)
    n = flat.shape[0]
    cam = rt.to_device(scenes.camera_a(int(round(4.3 * G))))   # the top-down camera over the 4.3 G x 4.3 G layout
    rays = torch.empty((rt.CameraRayCount(a.w, a.h, 1, True), 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, a.w, a.h, rays, tiled=True)
    nr = rays.shape[0]
    hits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(nr, dtype=torch.int32, device="cuda")
    mr = lambda ms: round(nr / (ms * 1e-3) / 1e6, 1)

    def build(inp, sah, stream=None):
        if sah:
            rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH), stream=stream)
        else:
            rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kBottomUp), stream=stream)

    def tree_bytes(k):
        return 64 * k + rt.NodesBytes(k)

    res = {}
    for name, sah in (("lbvh", False), ("sah", True)):
        root, count = (0, 1) if sah else (0, 2)
        blas = rt.BuildInput.allocate(blas_tris, sah=sah)
        build(blas, sah)
        table = rt.accel_table([(blas.triangles_out, blas.nodes_out, root, count)])

        def scene(instances):
            k = instances.size
            tlas = rt.BuildInput.allocate(np.zeros((k, 9), np.float32), sah=sah)
            d = dict(tlas=tlas, inst=rt.to_device(instances), rec=rt.device_bytes(64 * k), status=rt.device_bytes(4), k=k)

            def frame():
                rt.PrepareInstances(d["inst"], k, table, 1, tlas.triangles_in, d["rec"], d["status"])
                build(tlas, sah)
            d["frame"] = frame
            return d

        s16 = scene(inst)
        s16["frame"]()
        torch.cuda.synchronize()
        assert rt.instance_status(s16["status"]) == 0

        def q_inst(any_hit):
            t = s16["tlas"]
            rt.IntersectRaysInstanced(t.triangles_out, t.nodes_out, root, count, s16["rec"], 16, table, 1, rays, hits, ids,
                                      any_hit=any_hit, num_primitives=n)
        fl = rt.BuildInput.allocate(flat, sah=sah)
        build(fl, sah)

        def q_flat(any_hit):
            rt.IntersectRays(fl.triangles_out, fl.nodes_out, root, count, rays, hits, any_hit=any_hit, num_primitives=n)
        r = dict(instanced=dict(mrays_closest=mr(timed(lambda: q_inst(False), a.iters, a.warmup)),
                                mrays_any=mr(timed(lambda: q_inst(True), a.iters, a.warmup)),
                                tree_bytes=tree_bytes(nb) + tree_bytes(16) + 64 * 16 + 24),
                 flattened=dict(mrays_closest=mr(timed(lambda: q_flat(False), a.iters, a.warmup)),
                                mrays_any=mr(timed(lambda: q_flat(True), a.iters, a.warmup)),
                                tree_bytes=tree_bytes(n)))
        # work per ray (one counted launch each): box tests of both levels, triangle tests
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        t = s16["tlas"]
        rt.IntersectRaysInstanced(t.triangles_out, t.nodes_out, root, count, s16["rec"], 16, table, 1, rays, hits, ids,
                                  num_primitives=n, counters=ctr)
        torch.cuda.synchronize()
        r["hit_fraction"] = round(float((ids != -1).float().mean()), 4)
        r["instanced"].update(box_per_ray=round(int(ctr[0]) / nr, 2), tri_per_ray=round(int(ctr[1]) / nr, 2))
        ctr.zero_()
        rt.IntersectRays(fl.triangles_out, fl.nodes_out, root, count, rays, hits, num_primitives=n, counters=ctr)
        torch.cuda.synchronize()
        r["flattened"].update(box_per_ray=round(int(ctr[0]) / nr, 2), tri_per_ray=round(int(ctr[1]) / nr, 2))
        r["ratio_closest"] = round(r["instanced"]["mrays_closest"] / r["flattened"]["mrays_closest"], 3)
        r["ratio_any"] = round(r["instanced"]["mrays_any"] / r["flattened"]["mrays_any"], 3)
        motion = {}
        for side in (4, 256):
            s = s16 if side == 4 else scene(layout(rt, side, G, seed=2))
            motion[str(side * side)] = round(timed(s["frame"], a.iters, a.warmup), 4)
        r["rigid_motion_ms"] = motion
        res[name] = r
        del blas, fl, s16
        torch.cuda.empty_cache()
    print(json.dumps(dict(tool="instance_bench", blas_triangles=nb, instances=16, instanced_triangles=16 * nb,
                          rays="camera A %dx%d tiled" % (a.w, a.h), iters=a.iters, warmup=a.warmup, results=res,
                          device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
