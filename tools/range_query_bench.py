"""Range-query throughput on the bench scene: prints ONE JSON line (and writes it to --out when given).

Scene: grid_mesh(708) = 1,002,528 triangles, on the LBVH and SAH trees.  Queries: the 2^20 near-surface points of
tools/point_query_bench.py (set a: Morton order of their xz cell), as spheres (p, dist2_max) and as cubes centred on p.  Per
shape three sizes, calibrated by bisection with rt_range_count itself on the first 2^16 queries so that the mean result size
is about 1, 16 and 256 triangles.  Per (tree, shape, size), each launch sequence timed alone between two device events
(warm-up first, then --iters, median):
  count_ms    rt_range_count (traversal + workgroup scan, the scan of the workgroup sums, the add)
  collect_ms  rt_range_collect into exactly offsets[n] ids, with counts
  scan_ms     rt_range_count on an EMPTY tree (count = 0): no traversal, so the three launches and the scan traffic alone
  closest_ms  the yardstick: rt_closest_points on the same points with the same dist2_max (sphere rows; a box row repeats the
              sphere row of its size, for the ratio only)
and the box / triangle tests per query of one count launch.
Usage: python tools/range_query_bench.py [--iters 30] [--warmup 5] [--grid 708] [--log2n 20] [--out profiles/range_query_bench.json]
Kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/range_query_bench.py --iters 3 --warmup 1`
(a run of its own: the event timings above are taken without the profiler)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from point_query_bench import build, query_sets, timed  # noqa: E402

TARGETS = (1, 16, 256)


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
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    tris = scenes.grid_mesh(a.grid, 1)
    nq = 1 << a.log2n
    sets, ext = query_sets(tris, nq)
    pts = sets["a_near_coherent"][:, :3].copy()
    P = torch.from_numpy(pts).cuda()

    def sphere(r):
        q = torch.empty((nq, 4), dtype=torch.float32, device="cuda")
        q[:, :3], q[:, 3] = P, float(np.float32(r) * np.float32(r))
        return q

    def cube(h):
        q = torch.zeros((nq, 8), dtype=torch.float32, device="cuda")
        q[:, 0:3], q[:, 4:7] = P - float(h), P + float(h)
        return q

    make = {"sphere": (sphere, rt.kRangeSphere), "box": (cube, rt.kRangeBox)}
    offsets = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
    scratch = rt.device_bytes(rt.RangeScratchBytes(nq))
    counts = torch.empty(nq, dtype=torch.int32, device="cuda")
    hits = torch.empty((nq, 4), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    ns = min(nq, 1 << 16)                      # the calibration sample

    def mean_size(T, N, root, count, q, shape):
        rec = q.shape[1]
        rt.RangeCount(T, N, root, count, q[:ns].contiguous().view(-1, rec), offsets[:ns + 1], shape=shape, scratch=scratch)
        return int(offsets[ns].item()) / ns

    def calibrate(T, N, root, count, shape_name, target):
        mk, shape = make[shape_name]
        lo, hi = 0.0, 0.05 * ext
        while mean_size(T, N, root, count, mk(hi), shape) < target:
            hi *= 2
        for _ in range(18):
            mid = 0.5 * (lo + hi)
            if mean_size(T, N, root, count, mk(mid), shape) < target:
                lo = mid
            else:
                hi = mid
        return hi

    res, sizes = {}, {}
    for kind in ("lbvh", "sah"):
        inp, root, count = build(rt, tris, kind)
        T, N = inp.triangles_out, inp.nodes_out
        if not sizes:                          # the result sets do not depend on the tree: calibrate once
            sizes = {(s, t): calibrate(T, N, root, count, s, t) for s in make for t in TARGETS}
        row = {}
        for t in TARGETS:
            closest = None
            for shape_name, (mk, shape) in make.items():
                size = sizes[shape_name, t]
                q = mk(size)
                count_ms = timed(lambda: rt.RangeCount(T, N, root, count, q, offsets, shape=shape, scratch=scratch),
                                 a.iters, a.warmup)
                scan_ms = timed(lambda: rt.RangeCount(T, N, 0, 0, q, offsets, shape=shape, scratch=scratch), a.iters, a.warmup)
                ctr.zero_()
                st.zero_()
                rt.RangeCount(T, N, root, count, q, offsets, shape=shape, scratch=scratch, counters=ctr, status=st)
                total = int(offsets[nq].item())
                c = ctr.cpu().numpy()
                ids = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
                collect_ms = timed(lambda: rt.RangeCollect(T, N, root, count, q, offsets, ids, shape=shape, counts=counts,
                                                           status=st), a.iters, a.warmup)
                if shape_name == "sphere":
                    closest = timed(lambda: rt.ClosestPoints(T, N, root, count, q, hits), a.iters, a.warmup)
                row[f"{shape_name}_{t}"] = {
                    "size": float(size), "mean_ids": round(total / nq, 3), "max_ids": int(counts.max().item()),
                    "count_ms": round(count_ms, 4), "collect_ms": round(collect_ms, 4), "scan_ms": round(scan_ms, 4),
                    "closest_ms": round(closest, 4), "count_over_closest": round(count_ms / closest, 3),
                    "collect_over_closest": round(collect_ms / closest, 3),
                    "mqueries_s_count": round(nq / count_ms / 1e3, 1), "mids_s_collect": round(total / collect_ms / 1e3, 1),
                    "box_per_query": round(c[0] / nq, 2), "tri_per_query": round(c[1] / nq, 2), "status": rt.range_status(st)}
                del ids
        res[kind] = row
        del inp
    out = {"tool": "range_query_bench", "triangles": int(tris.shape[0]), "queries": nq, "extent": ext, "iters": a.iters,
           "warmup": a.warmup, "targets": list(TARGETS), "results": res, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
