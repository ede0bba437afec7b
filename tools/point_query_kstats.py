#!/usr/bin/env python3
"""Kernel times of point_query_kernel per tree and query set, from the kernel trace of a rocprofv3 run of
tools/point_query_bench.py:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/point_query_bench.py --iters I --warmup W
  python3 tools/point_query_kstats.py OUT/run_kernel_trace.csv --iters I --warmup W

The bench launches the kernel in a fixed order -- for each tree (lbvh, pairs, sah, sah_pairs) and each set (a..d): W warm-up
launches, I timed launches, one launch with counters -- so the dispatches are split by position.  Prints the median of the I
timed launches per (tree, set) in microseconds and Mqueries/s for 2^20 queries."""
import argparse
import csv

import numpy as np

TREES = ("lbvh", "pairs", "sah", "sah_pairs")
SETS = ("a_near_coherent", "b_near_shuffled", "c_uniform", "d_near_radius")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--iters", type=int, required=True)
    ap.add_argument("--warmup", type=int, required=True)
    ap.add_argument("--queries", type=int, default=1 << 20)
    a = ap.parse_args()
    rows = [r for r in csv.DictReader(open(a.trace)) if "point_query_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    per = a.warmup + a.iters + 1
    assert len(rows) == per * len(TREES) * len(SETS), f"{len(rows)} dispatches, expected {per * 16}"
    print(f"# point_query_kernel, median of {a.iters} timed launches per (tree, set), {a.queries} queries")
    print(f"{'tree':10s} {'set':16s} {'us':>9s} {'Mq/s':>8s}")
    for t, tree in enumerate(TREES):
        for s, name in enumerate(SETS):
            g = rows[(t * len(SETS) + s) * per:][:per][a.warmup:a.warmup + a.iters]
            us = float(np.median([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in g]))
            print(f"{tree:10s} {name:16s} {us:9.1f} {a.queries / us:8.1f}")


if __name__ == "__main__":
    main()
