"""Closest-point query throughput on the bench scene: prints ONE JSON line (and writes it to --out when given).

Scene: grid_mesh(708) = 1,002,528 triangles, on LBVH, pairs, SAH and SAH-pairs trees.  Four seeded query sets of 2^20 points:
  a_near_coherent  points on random triangles offset along the normal by up to +-1 % of the extent, in the Morton order of
                   their xz cell (1024 x 1024 cells over the scene box)
  b_near_shuffled  the same points, shuffled
  c_uniform        uniform in the scene box grown by 1.5x
  d_near_radius    set (a) with dist2_max = (1 % of the extent)^2
Each launch is timed alone between two device events (warm-up first, then --iters launches, median); box / triangle tests per
query come from one further launch with counters.  For comparison the tiled closest-hit camera rays (camera A, 1920 x 1080)
through rt_intersect_rays on the same LBVH tree, timed the same way.
Usage: python tools/point_query_bench.py [--iters 30] [--warmup 5] [--grid 708] [--out profiles/point_query_bench.json]
RT_LIB=<path>: time another build of the library instead (an experiment build made with `make librt_amd_exp.so EXPFLAGS=...`,
or another commit's library: DESIGN, "What the point queries share").  Kernel times per tree and set from a rocprofv3
run of this tool: tools/point_query_kstats.py."""
import argparse
import hashlib
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


def morton2(x, z):
    def spread(v):
        v = v.astype(np.uint64) & 0x3FF
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v
    return spread(x) | (spread(z) << 1)


def query_sets(tris, n, seed=1):
    rng = np.random.default_rng(seed)
    T = tris.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
    ext = float((hi - lo).max())
    k = rng.integers(0, len(T), n)
    b = rng.dirichlet((1, 1, 1), n)
    on = (b[:, :, None] * T[k]).sum(1)
    nrm = np.cross(T[k, 1] - T[k, 0], T[k, 2] - T[k, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    near = (on + nrm * rng.uniform(-0.01, 0.01, (n, 1)) * ext).astype(np.float32)
    cell = np.clip(((near[:, [0, 2]] - lo[[0, 2]]) / np.maximum(hi - lo, 1e-30)[[0, 2]] * 1024).astype(np.int64), 0, 1023)
    near = near[np.argsort(morton2(cell[:, 0], cell[:, 1]), kind="stable")]
    shuffled = near[rng.permutation(n)]
    c, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    uniform = (c + rng.uniform(-1, 1, (n, 3)) * half).astype(np.float32)
    r2 = np.float32((0.01 * ext) ** 2)

    def q(p, r):
        out = np.zeros((n, 4), np.float32)
        out[:, :3], out[:, 3] = p, r
        return out
    return {"a_near_coherent": q(near, np.inf), "b_near_shuffled": q(shuffled, np.inf), "c_uniform": q(uniform, np.inf),
            "d_near_radius": q(near, r2)}, ext


def build(rt, tris, kind):
    import torch
    n = tris.shape[0]
    if kind.startswith("sah"):
        inp = rt.BuildInput.allocate(tris, sah=True)
        rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH, enable_pairs=kind == "sah_pairs"))
        torch.cuda.synchronize()
        assert rt.to_host(inp.scratch, np.uint32, 1, rt.sah_scratch_layout(n).status)[0] == 0
        return inp, 0, 1
    inp = rt.BuildInput.allocate(tris)
    rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kBottomUp, enable_pairs=kind == "pairs"))
    torch.cuda.synchronize()
    return inp, 0, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if os.environ.get("RT_LIB"):
        rt.LIB_PATH = os.path.abspath(os.environ["RT_LIB"])
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    tris = scenes.grid_mesh(a.grid, 1)
    nq = 1 << a.log2n
    sets, ext = query_sets(tris, nq)
    dev = {k: torch.from_numpy(v).cuda() for k, v in sets.items()}
    hits = torch.empty((nq, 4), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = {}
    for kind in ("lbvh", "pairs", "sah", "sah_pairs"):
        inp, root, count = build(rt, tris, kind)
        T, N = inp.triangles_out, inp.nodes_out
        row = {}
        for name, q in dev.items():
            ms = timed(lambda: rt.ClosestPoints(T, N, root, count, q, hits), a.iters, a.warmup)
            ctr.zero_()
            st.zero_()
            rt.ClosestPoints(T, N, root, count, q, hits, counters=ctr, status=st)
            torch.cuda.synchronize()
            c = ctr.cpu().numpy()
            h = hits.cpu().numpy().view(np.uint32)
            row[name] = {"ms": round(ms, 4), "mqueries_s": round(nq / ms / 1e3, 1), "box_per_query": round(c[0] / nq, 2),
                         "tri_per_query": round(c[1] / nq, 2), "hit_fraction": round(float((h[:, 1] != 0xFFFFFFFF).mean()), 4),
                         "status": rt.point_status(st), "records_sha1": hashlib.sha1(h.tobytes()).hexdigest()[:16]}
        if kind == "lbvh":
            w, hh = 1920, 1080
            nr = rt.CameraRayCount(w, hh, 1, True)
            rays = torch.empty((nr, 8), dtype=torch.float32, device="cuda")
            rh = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(rt.to_device(scenes.camera_a(a.grid)), w, hh, rays, tiled=True)
            ms = timed(lambda: rt.IntersectRays(T, N, 0, 2, rays, rh), a.iters, a.warmup)
            ctr.zero_()
            rt.IntersectRays(T, N, 0, 2, rays, rh, counters=ctr)
            torch.cuda.synchronize()
            c = ctr.cpu().numpy()
            row["camera_closest_tiled_rays"] = {"ms": round(ms, 4), "mrays_s": round(w * hh / ms / 1e3, 1),
                                                "box_per_ray": round(c[0] / (w * hh), 2)}
        res[kind] = row
        del inp
    goal = res["lbvh"]["a_near_coherent"]["mqueries_s"]
    out = {"tool": "point_query_bench", "library": os.path.basename(rt.LIB_PATH), "triangles": int(tris.shape[0]),
           "queries": nq, "extent": ext, "iters": a.iters, "warmup": a.warmup, "results": res, "goal_mqueries_s": 890.0, "goal_met": bool(goal >= 890.0),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
