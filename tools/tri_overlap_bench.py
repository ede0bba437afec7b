"""Triangle-overlap query throughput on the bench scene: prints ONE JSON line (and writes it to --out when given).

Scene: grid_mesh(708) = 1,002,528 triangles, on the LBVH and SAH trees.  Workloads:
  self        RT_TRI_SELF over all triangles of the scene (the height field does not cut itself: the rows are empty, the cost is
              the traversal, the box tests and the id / corner exclusions)
  moved_<d>   2^20 scene triangles (in scene order: coherent) with every corner displaced by up to d cells in a random direction,
              d = 0.25 and 1.0
Per (tree, workload), each launch sequence timed alone between two device events (warm-up first, then --iters, median):
  count_ms    rt_tri_overlaps_count (traversal + workgroup scan, the scan of the workgroup sums, the add)
  collect_ms  rt_tri_overlaps_collect into exactly offsets[n] ids, with counts
  fixed_ms    rt_tri_overlaps_collect with offsets[i] = i * K, K = 8
and the same three for the yardstick: rt_range_count / rt_range_collect with RT_RANGE_BOX on the same queries' vertex boxes, in
the same run.  Also the mean / longest row of both, their ratio, and the box / leaf tests per query of one count launch (the two
traversals examine the same slots and leaves).
Usage: python tools/tri_overlap_bench.py [--iters 30] [--warmup 5] [--grid 708] [--log2n 20] [--out profiles/tri_overlap_bench.json]"""
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

K = 8
STEPS = (0.25, 1.0)


def moved_set(tris, n, step, seed=1):
    rng = np.random.default_rng(seed)
    T = tris.reshape(-1, 3, 3)
    k = np.sort(rng.integers(0, len(T), n))
    d = rng.normal(size=(n, 3, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return (T[k] + d * rng.uniform(0.0, step, (n, 3, 1)).astype(np.float32)).astype(np.float32).reshape(n, 9)


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
    tris = np.ascontiguousarray(scenes.grid_mesh(a.grid, 1), np.float32).reshape(-1, 9)
    nq = 1 << a.log2n
    work = [("self", tris, True)] + [(f"moved_{s}", moved_set(tris, nq, s), False) for s in STEPS]

    def run(T, N, root, count, name, q, self_pairs):
        n = len(q)
        qd = torch.from_numpy(q).cuda()
        c = q.reshape(n, 3, 3)
        box = np.zeros((n, 8), np.float32)
        box[:, 0:3], box[:, 4:7] = c.min(1), c.max(1)
        bd = torch.from_numpy(box).cuda()
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        fixed = (torch.arange(n + 1, dtype=torch.int64) * K).cuda()
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        scratch = rt.device_bytes(rt.TriOverlapsScratchBytes(n))
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        row = {"queries": n}
        for label in ("tri", "box"):
            if label == "tri":
                cnt = lambda off, **kw: rt.TriOverlapsCount(T, N, root, count, qd, off, self_pairs=self_pairs, scratch=scratch, **kw)
                col = lambda off, ids, **kw: rt.TriOverlapsCollect(T, N, root, count, qd, off, ids, self_pairs=self_pairs, **kw)
            else:
                cnt = lambda off, **kw: rt.RangeCount(T, N, root, count, bd, off, shape=rt.kRangeBox, scratch=scratch, **kw)
                col = lambda off, ids, **kw: rt.RangeCollect(T, N, root, count, bd, off, ids, shape=rt.kRangeBox, **kw)
            count_ms = timed(lambda: cnt(offsets), a.iters, a.warmup)
            ctr.zero_()
            st.zero_()
            cnt(offsets, counters=ctr, status=st)
            total = int(offsets[n].item())
            tests = ctr.cpu().numpy()
            ids = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
            collect_ms = timed(lambda: col(offsets, ids, counts=counts), a.iters, a.warmup)
            longest = int(counts.max().item())
            kids = torch.empty(n * K, dtype=torch.int32, device="cuda")
            fixed_ms = timed(lambda: col(fixed, kids, counts=counts), a.iters, a.warmup)
            row[label] = {"count_ms": round(count_ms, 4), "collect_ms": round(collect_ms, 4), "fixed_k_ms": round(fixed_ms, 4),
                          "mean_row": round(total / n, 4), "longest_row": longest, "box_per_query": round(tests[0] / n, 2),
                          "leaf_per_query": round(tests[1] / n, 2), "status": int(st.item())}
            del ids, kids
        t, b = row["tri"], row["box"]
        row["row_ratio"] = round(t["mean_row"] / b["mean_row"], 4) if b["mean_row"] else None
        for key in ("count_ms", "collect_ms", "fixed_k_ms"):
            row[key.replace("_ms", "") + "_time_ratio"] = round(t[key] / b[key], 3)
        return row

    res = {}
    for kind in ("lbvh", "sah"):
        inp, root, count = build(rt, tris, kind)
        res[kind] = {name: run(inp.triangles_out, inp.nodes_out, root, count, name, q, sp) for name, q, sp in work}
        del inp
    out = {"tool": "tri_overlap_bench", "triangles": int(tris.shape[0]), "queries": nq, "fixed_k": K, "iters": a.iters,
           "warmup": a.warmup, "steps": list(STEPS), "results": res, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
