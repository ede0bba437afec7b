"""First-K ray-query throughput on the bench scene, per pending-entry arm: prints ONE JSON line (and writes it to --out).

Scene: grid_mesh(708) = 1,002,528 triangles, on LBVH, pairs, SAH and SAH-pairs trees.  Three ray sets: the camera-A frame
(1920 x 1080, 8 x 8-tiled, tmax = the camera's max depth), one diffuse bounce from its primary hits (tools/ray_query_bench.py's
batch, tmax = +inf), and 2^18 seeded rays from inside the scene box in random directions with tmax = +inf -- the rays that
cross the whole mesh on their line.  For k in {1, 4, 32} each launch of rt_ray_first_hits is timed alone between two device
events (warm-up first, then --iters launches, median); box tests and leaf visits per ray come from one further launch with
counters.  Three yardsticks are timed in the same run on the same rays:
  closest_ms      rt_intersect_rays closest hit: the same bound as k = 1, another order and no list
  fixed_ms[k]     rt_ray_hits_collect with offsets[i] = i * k: the same output size, no order, a window that never shrinks
  sorted_ms       RayHits(..., sort=True): count, read-back, allocation, collect and two torch sorts -- the composition this
                  call replaces, host synchronisation included (timed between host clocks, --sorted-iters runs)
An arm is one build of the library (RT_RAY_FIRST_PENDING of csrc/ray_first_query.hip): the shipped one (4-byte entries, no
re-test on pop), and the experiment build (8-byte (entry, front) entries, re-culled on pop) made with
  make -C gpu-raytracing_amd/csrc librt_amd_exp.so EXPFLAGS=-DRT_RAY_FIRST_PENDING=8 EXPNAME=librt_amd_rayfirst8.so
Each arm runs in a child process of its own (a process binds one library), one after the other:
  python tools/ray_first_bench.py --arms pending4=gpu-raytracing_amd/csrc/librt_amd.so \
      pending8=gpu-raytracing_amd/csrc/librt_amd_rayfirst8.so [--iters 30] [--warmup 5] [--out profiles/ray_first_bench.json]
Rows: every child leaves one 32-bit checksum per row; the parent counts, per (tree, set, k), the rows on which the arms differ
and reports rows_sha1 per arm.  The arms promise equal rows on DECIDED rays only (include/rt_abi.h, claim 2): a differing row
is an undecided ray, whose share tests/test_gpu_ray_first.py caps at 2 % on its scenes; the parent fails above that share.
The parent adds per arm the ratios the design discussion needs: k = 1 time / closest-hit time, and time and box tests relative
to k = 1."""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TREES = ("lbvh", "pairs", "sah", "sah_pairs")
SETS = ("camera_a_tiled", "bounce", "inside_inf")
KS = (1, 4, 32)
MAX_DIFFER = 0.02


def inside_rays(tris, n, seed=1):
    """n rays from inside the scene box, random directions, tmin = 1e-3, tmax = +inf"""
    rng = np.random.default_rng(seed)
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    out = np.zeros((n, 8), np.float32)
    out[:, :3] = lo + rng.random((n, 3)) * (hi - lo)
    d = rng.normal(size=(n, 3))
    out[:, 4:7] = d / np.linalg.norm(d, axis=1)[:, None]
    out[:, 3], out[:, 7] = 1e-3, np.inf
    return out


def row_checksums(torch, o):
    """one 32-bit word per row of a float32 [n, k, 4] tensor (a weighted sum of the row's words, wrapping)"""
    w = o.view(torch.int32).reshape(o.shape[0], -1).to(torch.int64)
    mult = (torch.arange(w.shape[1], device=w.device, dtype=torch.int64) * 2654435761 + 40503) | 1
    return ((w * mult).sum(1) & 0xFFFFFFFF).to(torch.int64).cpu().numpy().astype(np.uint32)


def run_arm(a):
    """one library: every (tree, set): the yardsticks, then rt_ray_first_hits for each k"""
    import torch
    from point_query_bench import build, timed
    from ray_query_bench import bounce_rays
    rt = importlib.import_module("gpu-raytracing_amd")
    rt.LIB_PATH = os.path.abspath(a.lib)
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    tris = scenes.grid_mesh(a.grid, 1)
    n = tris.shape[0]
    cam = rt.to_device(scenes.camera_a(a.grid))
    w, h = a.w, a.h
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    res, sets = {}, {}
    for kind in TREES:
        inp, root, count = build(rt, tris, kind)
        T, N = inp.triangles_out, inp.nodes_out
        if not sets:                               # the rays do not depend on the tree
            tiled = torch.empty((rt.CameraRayCount(w, h, 1, True), 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(cam, w, h, tiled, tiled=True)
            row_major = torch.empty((w * h, 8), dtype=torch.float32, device="cuda")
            rt.GenerateCameraRays(cam, w, h, row_major)
            prim = torch.empty((w * h, 4), dtype=torch.float32, device="cuda")
            rt.IntersectRays(T, N, root, count, row_major, prim, num_primitives=n)
            torch.cuda.synchronize()
            sets = {"camera_a_tiled": tiled, "bounce": bounce_rays(rt, row_major, prim, tris)[0],
                    "inside_inf": torch.from_numpy(inside_rays(tris, 1 << a.log2n)).cuda()}
            del row_major, prim
        row = {}
        for name, rays in sets.items():
            nr = rays.shape[0]
            closest = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
            closest_ms = timed(lambda: rt.IntersectRays(T, N, root, count, rays, closest, num_primitives=n), a.iters, a.warmup)
            ctr.zero_()
            rt.IntersectRays(T, N, root, count, rays, closest, num_primitives=n, counters=ctr)
            torch.cuda.synchronize()
            c = ctr.cpu().numpy()
            ch = closest.cpu().numpy().view(np.uint32)
            cell = {"rays": nr, "closest": {"ms": round(closest_ms, 4), "mrays_s": round(nr / closest_ms / 1e3, 1),
                                            "box_per_ray": round(c[0] / nr, 2), "leaf_per_ray": round(c[1] / nr, 2)}}
            # the composition: count, read-back, allocation, collect, two sorts -- host clocks around the whole call
            rt.RayHits(T, N, root, count, rays, sort=True)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.sorted_iters):
                t0 = time.perf_counter()
                off, hits = rt.RayHits(T, N, root, count, rays, sort=True)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            cell["sorted"] = {"ms": round(float(np.median(ts)), 4), "records": int(hits.shape[0]),
                              "mean_row": round(hits.shape[0] / nr, 3)}
            del off, hits
            out = torch.empty((nr, max(KS), 4), dtype=torch.float32, device="cuda")
            counts = torch.empty(nr, dtype=torch.int32, device="cuda")
            for k in KS:
                o = out.view(-1)[:nr * k * 4].view(nr, k, 4)
                fixed = torch.arange(nr + 1, dtype=torch.int64, device="cuda") * k
                fixed_ms = timed(lambda: rt.RayHitsCollect(T, N, root, count, rays, fixed, o, counts=counts), a.iters, a.warmup)
                ms = timed(lambda: rt.RayFirstHits(T, N, root, count, rays, k, o), a.iters, a.warmup)
                ctr.zero_()
                st.zero_()
                o.fill_(0)
                rt.RayFirstHits(T, N, root, count, rays, k, o, counters=ctr, status=st)
                torch.cuda.synchronize()
                c = ctr.cpu().numpy()
                sums = row_checksums(torch, o)
                np.save(os.path.join(a.rows_dir, f"{kind}.{name}.k{k}.npy"), sums)
                cell[f"k{k}"] = {"ms": round(ms, 4), "mrays_s": round(nr / ms / 1e3, 1), "box_per_ray": round(c[0] / nr, 2),
                                 "leaf_per_ray": round(c[1] / nr, 2), "status": rt.ray_first_status(st),
                                 "fixed_collect_ms": round(fixed_ms, 4), "over_fixed_collect": round(ms / fixed_ms, 3),
                                 "over_sorted": round(ms / cell["sorted"]["ms"], 4),
                                 "rows_sha1": hashlib.sha1(o.cpu().numpy().tobytes()).hexdigest()[:16]}
                if k == 1:          # same t as closest hit wherever both report a hit (ids may differ among coincident triangles)
                    r = o.cpu().numpy().view(np.uint32).reshape(nr, 4)
                    cell["k1"]["t_equals_closest"] = round(float((r[:, 0] == ch[:, 0]).mean()), 6)
                del fixed
            del out, counts, closest
            row[name] = cell
        res[kind] = row
        del inp
        print(f"{os.path.basename(rt.LIB_PATH)}: {kind} done", file=sys.stderr, flush=True)
    print(json.dumps({"library": os.path.basename(rt.LIB_PATH), "triangles": int(n), "w": w, "h": h,
                      "device": torch.cuda.get_device_name(0), "results": res}))


def ratios(res):
    """per (tree, set): k = 1 against closest hit, and the growth of time and tests from k = 1 to 4 to 32"""
    out = {}
    for tree, row in res.items():
        out[tree] = {}
        for name, cell in row.items():
            k1 = cell["k1"]
            out[tree][name] = {"k1_over_closest": {"time": round(k1["ms"] / cell["closest"]["ms"], 3),
                                                   "box_tests": round(k1["box_per_ray"] / max(cell["closest"]["box_per_ray"], 1e-9), 3)},
                               **{f"k{k}_over_k1": {"time": round(cell[f"k{k}"]["ms"] / k1["ms"], 2),
                                                    "box_tests": round(cell[f"k{k}"]["box_per_ray"] / max(k1["box_per_ray"], 1e-9), 2),
                                                    "leaf_visits": round(cell[f"k{k}"]["leaf_per_ray"] / max(k1["leaf_per_ray"], 1e-9), 2)}
                                  for k in KS[1:]}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", nargs="+", default=[], metavar="NAME=LIBRARY")
    ap.add_argument("--lib", default="", help="(child) the one library to measure")
    ap.add_argument("--rows-dir", default="", help="(child) where the row checksums go")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sorted-iters", type=int, default=3)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--log2n", type=int, default=18)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.lib:
        run_arm(a)
        return
    arms = dict(s.split("=", 1) for s in a.arms) or {"shipped": os.path.join(ROOT, "gpu-raytracing_amd", "csrc", "librt_amd.so")}
    got, differ = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, lib in arms.items():      # one child at a time: each opens the GPU, measures, and exits
            os.mkdir(os.path.join(tmp, name))
            cmd = [sys.executable, os.path.abspath(__file__), "--lib", lib, "--rows-dir", os.path.join(tmp, name),
                   "--iters", str(a.iters), "--warmup", str(a.warmup), "--sorted-iters", str(a.sorted_iters),
                   "--grid", str(a.grid), "--w", str(a.w), "--h", str(a.h), "--log2n", str(a.log2n)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
            if p.returncode != 0:
                sys.exit(f"arm {name} ({lib}) failed with exit code {p.returncode}")
            got[name] = json.loads(p.stdout.strip().splitlines()[-1])
            print(f"arm {name}: done", file=sys.stderr, flush=True)
        first = next(iter(arms))
        worst = 0.0
        for tree in TREES:
            for s in SETS:
                for k in KS:
                    f = f"{tree}.{s}.k{k}.npy"
                    ref = np.load(os.path.join(tmp, first, f))
                    d = {name: int((np.load(os.path.join(tmp, name, f)) != ref).sum()) for name in arms if name != first}
                    differ[f"{tree}.{s}.k{k}"] = {"rays": int(len(ref)), "rows_differ_from_" + first: d}
                    worst = max([worst] + [v / len(ref) for v in d.values()])
    r0 = got[first]
    out = {"tool": "ray_first_bench", "triangles": r0["triangles"], "w": r0["w"], "h": r0["h"], "camera": "A",
           "device": r0["device"], "iters": a.iters, "warmup": a.warmup, "sorted_iters": a.sorted_iters,
           "worst_share_of_rows_differing_across_arms": round(worst, 6), "rows_across_arms": differ,
           "arms": {name: {"library": r["library"], "results": r["results"], "ratios": ratios(r["results"])}
                    for name, r in got.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if worst > MAX_DIFFER:
        sys.exit(f"the arms differ on {100 * worst:.2f} % of the rows of one cell: more than undecided rays can explain")


if __name__ == "__main__":
    main()
