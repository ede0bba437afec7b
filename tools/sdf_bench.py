"""Signed-distance / occupancy throughput against the composition they replace: prints ONE JSON line (and writes it to --out).

Scene: scenes.noisy_sphere(289) = 1,002,252 triangles, closed, on the LBVH and SAH trees.  Query sets:
  lattice_bricks     a 128^3 lattice over 1.2 x the scene box, rt_generate_grid_points' brick layout (one wave = one 4x4x4 brick)
  lattice_row_major  the same lattice, row-major
  near_surface       2M random points within 2 % of the extent of the surface (points on random triangles, offset along the
                     normal), in random order
Per (tree, set), each launch sequence timed alone between two device events (warm-up first, then --iters, median):
  sdf1_ms / sdf3_ms  SignedDistance with votes 1 / 3          occ1_ms / occ3_ms  Occupancy with votes 1 / 3
  comp1_ms / comp3_ms  the yardstick, the composition through the older entry points on the same points in the same run:
                     ClosestPoints + per direction (ray-batch construction in torch + RayHitsCount) + the parity arithmetic, the
                     vote, the square root and the sign in torch.  Every direction is cast for every point: the composition has no
                     early-out short of a compaction pass.
  occ_comp1_ms / occ_comp3_ms  the same without ClosestPoints and the square root.
and the ratios fused / composition, Mpoints/s, and from one further, checked run (fused bits == composition bits) two shares of
the live points -- the only evidence of how often a non-watertight edge crossing spoils a single ray:
  third_cast_share     the first two votes disagree (the fused kernel casts the third for exactly these)
  not_unanimous_share  the three parities are not all equal
Usage: python tools/sdf_bench.py [--iters 30] [--warmup 5] [--cells 289] [--lattice 128] [--near 2000000]
                                 [--out profiles/sdf_bench.json]
RT_LIB=<path>: time another build of the library instead (tools/point_query_bench.py's override)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from point_query_bench import build, timed  # noqa: E402


def near_surface(tris, n, seed=1, rel=0.02):
    rng = np.random.default_rng(seed)
    T = tris.reshape(-1, 3, 3).astype(np.float64)
    V = T.reshape(-1, 3)
    ext = float((V.max(0) - V.min(0)).max())
    k = rng.integers(0, len(T), n)
    b = rng.dirichlet((1, 1, 1), n)
    on = (b[:, :, None] * T[k]).sum(1)
    nrm = np.cross(T[k, 1] - T[k, 0], T[k, 2] - T[k, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    q = np.zeros((n, 4), np.float32)
    q[:, :3] = on + nrm * rng.uniform(-rel, rel, (n, 1)) * ext
    q[:, 3] = np.inf
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cells", type=int, default=289)
    ap.add_argument("--lattice", type=int, default=128)
    ap.add_argument("--near", type=int, default=2_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if os.environ.get("RT_LIB"):
        rt.LIB_PATH = os.path.abspath(os.environ["RT_LIB"])
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    tris = scenes.noisy_sphere(a.cells, 1)
    V = tris.reshape(-1, 3)
    c, half = (V.min(0) + V.max(0)) / 2, (V.max(0) - V.min(0)) / 2 * 1.2
    G = a.lattice
    dims, origin, spacing = (G, G, G), c - half, 2 * half / (G - 1)
    sets = {}
    for name, bricks in (("lattice_bricks", True), ("lattice_row_major", False)):
        q = torch.empty((rt.GridPointCount(dims, bricks), 4), dtype=torch.float32, device="cuda")
        rt.GenerateGridPoints(origin, spacing, dims, q, bricks=bricks)
        sets[name] = q
    sets["near_surface"] = rt.to_device(near_surface(tris, a.near)).view(torch.float32).view(-1, 4)
    D = torch.from_numpy(rt.SDF_DEFAULT_DIRS.copy()).cuda()
    res = {}
    for kind in ("lbvh", "sah"):
        inp, root, count = build(rt, tris, kind)
        T, N = inp.triangles_out, inp.nodes_out
        row = {}
        for name, q in sets.items():
            n = q.shape[0]
            out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
            ins = torch.empty(n, dtype=torch.uint8, device="cuda")
            hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            offs = [torch.empty(n + 1, dtype=torch.int64, device="cuda") for _ in range(3)]
            scratch = rt.device_bytes(rt.RayHitsScratchBytes(n))
            live = torch.isfinite(q[:, :3]).all(1) & (q[:, 3] >= 0)
            keep = {}

            def composition(votes, distance):
                if distance:
                    rt.ClosestPoints(T, N, root, count, q, hits)
                odd = torch.zeros(n, dtype=torch.int64, device="cuda")
                for j in range(votes):
                    # the ray batch: (p, 0, D[j], +inf); a query that is not traced gets tmin > tmax
                    rays[:, :3] = q[:, :3]
                    rays[:, 3] = torch.where(live, 0.0, 1.0)
                    rays[:, 4:7] = D[j]
                    rays[:, 7] = torch.where(live, float("inf"), -1.0)
                    rt.RayHitsCount(T, N, root, count, rays, offs[j], scratch=scratch)
                    odd += (offs[j][1:] - offs[j][:-1]) & 1
                inside = odd * 2 > votes
                keep["inside"] = inside
                if distance:
                    sd = torch.sqrt(hits[:, 0])
                    keep["sdist"] = torch.where(inside & (sd != 0), -sd, sd)

            t = {}
            for votes in (1, 3):
                t[f"sdf{votes}_ms"] = timed(lambda: rt.SignedDistance(T, N, root, count, q, out, votes=votes), a.iters, a.warmup)
                t[f"occ{votes}_ms"] = timed(lambda: rt.Occupancy(T, N, root, count, q, ins, votes=votes), a.iters, a.warmup)
                t[f"comp{votes}_ms"] = timed(lambda: composition(votes, True), a.iters, a.warmup)
                t[f"occ_comp{votes}_ms"] = timed(lambda: composition(votes, False), a.iters, a.warmup)
            # one checked run: the fused results equal the composition's, and the vote statistics
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
            rt.SignedDistance(T, N, root, count, q, out, votes=3, counters=ctr, status=st)
            rt.Occupancy(T, N, root, count, q, ins, votes=3)
            composition(3, True)
            torch.cuda.synchronize()
            same = bool((out[:, 0].view(torch.int32) == keep["sdist"].view(torch.int32)).all()) and \
                bool((ins.bool() == keep["inside"]).all())
            par = torch.stack([(o[1:] - o[:-1]) & 1 for o in offs])
            nl = max(int(live.sum().item()), 1)
            third = int(((par[0] != par[1]) & live).sum().item())
            mixed = int((((par[0] != par[1]) | (par[1] != par[2])) & live).sum().item())
            cc = ctr.cpu().numpy()
            r = {"points": n, "live": nl, "inside_share": round(float(ins.sum().item()) / nl, 4),
                 "equals_composition": same, "status": rt.sdf_status(st),
                 "third_cast_share": round(third / nl, 6), "not_unanimous_share": round(mixed / nl, 6),
                 "box_per_point_sdf3": round(float(cc[0]) / nl, 2), "leaf_per_point_sdf3": round(float(cc[1]) / nl, 2)}
            for k, v in t.items():
                r[k] = round(v, 4)
            for votes in (1, 3):
                r[f"mpoints_s_sdf{votes}"] = round(n / t[f"sdf{votes}_ms"] / 1e3, 1)
                r[f"mpoints_s_occ{votes}"] = round(n / t[f"occ{votes}_ms"] / 1e3, 1)
                r[f"sdf{votes}_over_comp"] = round(t[f"sdf{votes}_ms"] / t[f"comp{votes}_ms"], 3)
                r[f"occ{votes}_over_comp"] = round(t[f"occ{votes}_ms"] / t[f"occ_comp{votes}_ms"], 3)
            row[name] = r
            del out, ins, hits, rays, offs, scratch
        res[kind] = row
        del inp
    o = {"tool": "sdf_bench", "triangles": int(tris.shape[0]), "lattice": G, "iters": a.iters, "warmup": a.warmup,
         "results": res, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(o)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
