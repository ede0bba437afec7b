"""k-nearest query throughput on the bench scene, per list-storage arm: prints ONE JSON line (and writes it to --out when given).

Scene: grid_mesh(708) = 1,002,528 triangles, on LBVH, pairs, SAH and SAH-pairs trees.  Three seeded query sets of 2^20 points
(tools/point_query_bench.py's): a_near_coherent, b_near_shuffled, c_uniform, all with an infinite radius.  For k in {1, 8, 32}
each launch of rt_k_nearest is timed alone between two device events (warm-up first, then --iters launches, median); box /
triangle tests per query come from one further launch with counters, and rows_sha1 is the hash of the whole output.  In the same
run rt_closest_points is timed on the same sets the same way: the yardstick -- its traversal is the k = 1 traversal.

An arm is one build of the library (RT_KNN_LIST of csrc/knn_query.hip): the shipped one, and experiment builds made with
  make -C gpu-raytracing_amd/csrc librt_amd_exp.so EXPFLAGS=-DRT_KNN_LIST=0 EXPNAME=librt_amd_knn_row.so
Each arm runs in a child process of its own (a process binds one library), one after the other:
  python tools/knn_bench.py --arms private=gpu-raytracing_amd/csrc/librt_amd.so row=gpu-raytracing_amd/csrc/librt_amd_knn_row.so \
      [--iters 30] [--warmup 5] [--out profiles/knn_bench.json]
Without --arms the one arm is the shipped library, or the build that RT_LIB=<path> names.
The parent merges the children's results, requires rows_sha1 to agree across arms for every (tree, set, k), and adds per arm
the ratios the design discussion needs: k = 1 time / rt_closest_points time, and time and box tests relative to k = 1."""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TREES = ("lbvh", "pairs", "sah", "sah_pairs")
SETS = ("a_near_coherent", "b_near_shuffled", "c_uniform")
KS = (1, 8, 32)


def run_arm(a):
    """one library: every (tree, set): rt_closest_points, then rt_k_nearest for each k"""
    import torch
    from point_query_bench import build, query_sets, timed
    rt = importlib.import_module("gpu-raytracing_amd")
    rt.LIB_PATH = os.path.abspath(a.lib)
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    tris = scenes.grid_mesh(a.grid, 1)
    nq = 1 << a.log2n
    sets, ext = query_sets(tris, nq)
    dev = {k: torch.from_numpy(sets[k]).cuda() for k in SETS}
    hits = torch.empty((nq, 4), dtype=torch.float32, device="cuda")
    out = torch.empty((nq, max(KS), 2), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = {}
    for kind in TREES:
        inp, root, count = build(rt, tris, kind)
        T, N = inp.triangles_out, inp.nodes_out
        row = {}
        for name, q in dev.items():
            ms = timed(lambda: rt.ClosestPoints(T, N, root, count, q, hits), a.iters, a.warmup)
            ctr.zero_()
            rt.ClosestPoints(T, N, root, count, q, hits, counters=ctr)
            torch.cuda.synchronize()
            c = ctr.cpu().numpy()
            h = hits.cpu().numpy().view(np.uint32)
            cell = {"closest_points": {"ms": round(ms, 4), "mqueries_s": round(nq / ms / 1e3, 1),
                                       "box_per_query": round(c[0] / nq, 2), "tri_per_query": round(c[1] / nq, 2)}}
            for k in KS:
                o = out.view(-1)[:nq * k * 2].view(nq, k, 2)
                ms = timed(lambda: rt.KNearest(T, N, root, count, q, k, o), a.iters, a.warmup)
                ctr.zero_()
                st.zero_()
                o.fill_(0)
                rt.KNearest(T, N, root, count, q, k, o, counters=ctr, status=st)
                torch.cuda.synchronize()
                c = ctr.cpu().numpy()
                r = o.cpu().numpy().view(np.uint32)
                cell[f"k{k}"] = {"ms": round(ms, 4), "mqueries_s": round(nq / ms / 1e3, 1), "box_per_query": round(c[0] / nq, 2),
                                 "tri_per_query": round(c[1] / nq, 2), "status": rt.knn_status(st),
                                 "rows_sha1": hashlib.sha1(r.tobytes()).hexdigest()[:16]}
                if k == 1:          # the yardstick's record and the k = 1 row are the same (dist2, id)
                    cell["k1"]["equals_closest_points"] = bool((r.reshape(nq, 2) == h[:, :2]).all())
            row[name] = cell
        res[kind] = row
        del inp
    print(json.dumps({"library": os.path.basename(rt.LIB_PATH), "triangles": int(tris.shape[0]), "queries": nq, "extent": ext,
                      "device": torch.cuda.get_device_name(0), "results": res}))


def ratios(res):
    """per (tree, set): k = 1 against rt_closest_points, and the growth of time and box tests from k = 1 to 8 to 32"""
    out = {}
    for tree, row in res.items():
        out[tree] = {}
        for name, cell in row.items():
            k1 = cell["k1"]
            out[tree][name] = {"k1_over_closest_points": round(k1["ms"] / cell["closest_points"]["ms"], 3),
                               **{f"k{k}_over_k1": {"time": round(cell[f"k{k}"]["ms"] / k1["ms"], 2),
                                                    "box_tests": round(cell[f"k{k}"]["box_per_query"] / k1["box_per_query"], 2),
                                                    "tri_tests": round(cell[f"k{k}"]["tri_per_query"] / k1["tri_per_query"], 2)}
                                  for k in KS[1:]}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", nargs="+", default=[], metavar="NAME=LIBRARY")
    ap.add_argument("--lib", default="", help="(child) the one library to measure")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grid", type=int, default=708)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.lib:
        run_arm(a)
        return
    # without --arms: the shipped library, or the build RT_LIB names (tools/point_query_bench.py's override)
    shipped = os.environ.get("RT_LIB") or os.path.join(ROOT, "gpu-raytracing_amd", "csrc", "librt_amd.so")
    arms = dict(s.split("=", 1) for s in a.arms) or {"shipped": shipped}
    got = {}
    for name, lib in arms.items():      # one child at a time: each opens the GPU, measures, and exits
        cmd = [sys.executable, os.path.abspath(__file__), "--lib", lib, "--iters", str(a.iters), "--warmup", str(a.warmup),
               "--grid", str(a.grid), "--log2n", str(a.log2n)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit(f"arm {name} ({lib}) failed with exit code {p.returncode}")
        got[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(f"arm {name}: done", file=sys.stderr, flush=True)
    first = next(iter(got.values()))
    agree = True
    for name, r in got.items():
        for tree in TREES:
            for s in SETS:
                for k in KS:
                    agree &= r["results"][tree][s][f"k{k}"]["rows_sha1"] == first["results"][tree][s][f"k{k}"]["rows_sha1"]
    out = {"tool": "knn_bench", "triangles": first["triangles"], "queries": first["queries"], "device": first["device"],
           "iters": a.iters, "warmup": a.warmup, "rows_sha1_equal_across_arms": bool(agree),
           "arms": {name: {"library": r["library"], "results": r["results"], "ratios": ratios(r["results"])}
                    for name, r in got.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not agree:
        sys.exit("rows_sha1 differs between arms")


if __name__ == "__main__":
    main()
