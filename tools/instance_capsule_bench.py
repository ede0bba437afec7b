"""The mixed instanced ray query with capsule BLASes (IntersectRaysInstancedMixedCapsules) beside the calls a caller has without
it: prints ONE JSON line (and writes it to --out).

Geometry: grid_mesh(G) (2 G^2 triangles; G = 177: 62,658) as the mesh BLAS, one sphere per triangle of it (tools/sphere_bench.py's
construction) as the sphere BLAS and one capsule per triangle of it (tools/capsule_bench.py's: along the first edge, radius 0.1
of the mean edge) as the capsule BLAS: the same primitive count and the same spatial layout for the three kinds.  16 instances
on tools/instance_bench.py's 4 x 4 layout with small distinct rotations.  Rays: 1920 x 1080 tiled camera-A rays, top-down over
the whole layout.  Per builder (LBVH = RunBottomUpBuild, SAH = RunSahBuild; every BLAS, TLAS and flat tree built by it), ONE
scene of all three kinds -- instance k holds kind k mod 3 -- and three comparisons on it:
  no_capsules   the scene's mesh and sphere instances alone (a table without a capsule entry) through the new call beside
                IntersectRaysInstancedMixed on the same buffers: what the extra arm and the new kernels' register bound cost a
                caller who does not need them, i.e. when to stay with the old call;
  three_kinds   the whole scene through the new call beside the route a caller has today: IntersectRaysInstancedMixed over the
                mesh and sphere instances, then IntersectRaysCapsules over the capsule sets flattened into one world-space
                tree (the rotations are rigid, so they stay capsules), the two timed together as one frame; the merge of the
                two hit buffers, which that route also needs, is not timed;
  identity      the flattened capsule tree under ONE identity instance through the new call beside IntersectRaysCapsules on
                that tree: the price of the second level.
Each pair is timed ALTERNATING, --rounds times: per side `mrays_closest` / `mrays_any` are the median over all timed launches
of rays per second (millions), `spread_*` the least and the greatest of the per-round medians; each launch is timed alone
between two device events after --warmup launches, counters off.  box_per_ray / leaf_per_ray: closest-hit tests per ray from
one counted launch.  One process, one session: the spread is the run-to-run spread inside it and says nothing about another day.
RT_LIB=<path>: time another build of the library instead (e.g. one with -DRT_INSTANCE_MIXED_CAPSULE_WAVES=5).
Usage: python tools/instance_capsule_bench.py [--grid 177] [--iters 20] [--warmup 3] [--rounds 3] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from capsule_bench import capsules_of        # noqa: E402
from instance_bench import layout             # noqa: E402
from sphere_bench import spheres_of           # noqa: E402


def launch_ms(fn, iters, warmup):
    """the time of each of `iters` launches of fn, alone between two device events, after `warmup` launches"""
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
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid", type=int, default=177)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("gpu-raytracing_amd")
    if os.environ.get("RT_LIB"):
        rt.LIB_PATH = os.path.abspath(os.environ["RT_LIB"])
    scenes = importlib.import_module("gpu-raytracing_amd.scenes")
    G = a.grid
    mesh = scenes.grid_mesh(G, 1)
    balls, caps = spheres_of(mesh), capsules_of(mesh)
    nb = mesh.shape[0]
    inst = layout(rt, 4, G, seed=1)
    inst["blas"] = np.arange(16) % 3                    # 0 mesh, 1 spheres, 2 capsules
    M = inst["object_to_world"].astype(np.float64)
    with_caps = [k for k in range(16) if k % 3 == 2]
    without = [k for k in range(16) if k % 3 != 2]

    def flat_capsules(which):
        p0, p1 = caps[:, 0:3].astype(np.float64), caps[:, 4:7].astype(np.float64)
        out = []
        for k in which:
            c = caps.copy()
            c[:, 0:3], c[:, 4:7] = p0 @ M[k][:, :3].T + M[k][:, 3], p1 @ M[k][:, :3].T + M[k][:, 3]
            out.append(c)
        return np.ascontiguousarray(np.concatenate(out), np.float32)

    cam = rt.to_device(scenes.camera_a(int(round(4.3 * G))))
    rays = torch.empty((rt.CameraRayCount(a.w, a.h, 1, True), 8), dtype=torch.float32, device="cuda")
    rt.GenerateCameraRays(cam, a.w, a.h, rays, tiled=True)
    nr = rays.shape[0]
    hits = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    hits2 = torch.empty((nr, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty(nr, dtype=torch.int32, device="cuda")
    mr = lambda ms: round(nr / (ms * 1e-3) / 1e6, 1)

    def build(inp, sah):
        if sah:
            rt.RunSahBuild(inp, rt.Arguments(build_type=rt.kSAH))
        else:
            rt.RunBottomUpBuild(inp, rt.Arguments(build_type=rt.kBottomUp))

    def pair(new, other, other_name):
        """both sides alternating: {new_call: {...}, other_name: {...}, ratio_closest, ratio_any}"""
        out = {"new_call": {}, other_name: {}}
        for mode, any_hit in (("closest", False), ("any", True)):
            per = {"new_call": [], other_name: []}
            for _ in range(a.rounds):
                for name, fn in (("new_call", new), (other_name, other)):
                    per[name].append(launch_ms(lambda: fn(any_hit), a.iters, a.warmup))
            for name, rounds in per.items():
                out[name]["mrays_" + mode] = mr(float(np.median(np.concatenate(rounds))))
                meds = [mr(float(np.median(r))) for r in rounds]
                out[name]["spread_" + mode] = [min(meds), max(meds)]
            out["ratio_" + mode] = round(out["new_call"]["mrays_" + mode] / out[other_name]["mrays_" + mode], 3)
        return out

    def counted(fn):
        ctr = torch.zeros(4, dtype=torch.int64, device="cuda")
        fn(False, ctr)
        torch.cuda.synchronize()
        return dict(box_per_ray=round(int(ctr[0]) / nr, 2), leaf_per_ray=round(int(ctr[1]) / nr, 2))

    res = {}
    for name, sah in (("lbvh", False), ("sah", True)):
        root, count = (0, 1) if sah else (0, 2)

        def proxy_tree(data, width, prepare, status_of):
            dev = rt.to_device(data).view(torch.float32).view(-1, width)
            tree = rt.BuildInput.allocate(np.zeros((data.shape[0], 9), np.float32), sah=sah)
            status = rt.device_bytes(4)
            prepare(dev, data.shape[0], tree.triangles_in, status)
            build(tree, sah)
            torch.cuda.synchronize()
            assert status_of(status) == 0
            return dev, tree

        def tlas_over(instances, table, num_blas):
            k = instances.size
            tlas = rt.BuildInput.allocate(np.zeros((k, 9), np.float32), sah=sah)
            rec, status = rt.device_bytes(64 * k), rt.device_bytes(4)
            rt.PrepareInstances(rt.to_device(instances), k, table, num_blas, tlas.triangles_in, rec, status)
            build(tlas, sah)
            torch.cuda.synchronize()
            assert rt.instance_status(status) == 0
            return tlas, rec, k

        blas = rt.BuildInput.allocate(mesh, sah=sah)
        build(blas, sah)
        ball_dev, ball_tree = proxy_tree(balls, 4, rt.PrepareSpheres, rt.sphere_status)
        cap_dev, cap_tree = proxy_tree(caps, 8, rt.PrepareCapsules, rt.capsule_status)
        table = rt.accel_table([(t.triangles_out, t.nodes_out, root, count) for t in (blas, ball_tree, cap_tree)])
        geom = rt.geometry_table([None, (ball_dev, nb), (cap_dev, nb, rt.RT_GEOM_CAPSULES)])
        r = {}

        def q_new(any_hit, ctr, tlas, rec, k, table=table, geom=geom, num_blas=3):
            rt.IntersectRaysInstancedMixedCapsules(tlas.triangles_out, tlas.nodes_out, root, count, rec, k, table, geom, num_blas,
                                                   rays, hits, ids, any_hit=any_hit, counters=ctr)

        def q_old(any_hit, ctr, tlas, rec, k):
            rt.IntersectRaysInstancedMixed(tlas.triangles_out, tlas.nodes_out, root, count, rec, k, table, geom, 3, rays, hits,
                                           ids, any_hit=any_hit, counters=ctr)

        def q_caps(any_hit, ctr, dev, tree, n, out):
            rt.IntersectRaysCapsules(tree.triangles_out, tree.nodes_out, root, count, dev, n, rays, out, any_hit=any_hit,
                                     counters=ctr)

        # ---- no capsules: the new call beside the old mixed call over the mesh and sphere instances
        ptlas, prec, pk = tlas_over(inst[without], table, 3)
        new = lambda any_hit, ctr=None: q_new(any_hit, ctr, ptlas, prec, pk)
        old = lambda any_hit, ctr=None: q_old(any_hit, ctr, ptlas, prec, pk)
        d = pair(new, old, "mixed_call")
        d["new_call"].update(counted(new))
        d["hit_fraction"] = round(float((ids != -1).float().mean()), 4)
        d["mixed_call"].update(counted(old))
        r["no_capsules"] = d

        # ---- three kinds: the new call beside the old mixed call plus the capsule query over the flattened capsule sets
        tlas, rec, k = tlas_over(inst, table, 3)
        some = flat_capsules(with_caps)
        some_dev, some_tree = proxy_tree(some, 8, rt.PrepareCapsules, rt.capsule_status)
        new = lambda any_hit, ctr=None: q_new(any_hit, ctr, tlas, rec, k)

        def two(any_hit, ctr=None):
            q_old(any_hit, ctr, ptlas, prec, pk)
            q_caps(any_hit, ctr, some_dev, some_tree, some.shape[0], hits2)
        d = pair(new, two, "two_calls")
        d["new_call"].update(counted(new))
        d["hit_fraction"] = round(float((ids != -1).float().mean()), 4)
        d["two_calls"].update(counted(two))
        r["three_kinds"] = d
        del some_dev, some_tree

        # ---- identity: one identity instance over the flat capsule tree beside the capsule query
        flat = flat_capsules(range(16))
        flat_dev, flat_tree = proxy_tree(flat, 8, rt.PrepareCapsules, rt.capsule_status)
        ftable = rt.accel_table([(flat_tree.triangles_out, flat_tree.nodes_out, root, count)])
        fgeom = rt.geometry_table([(flat_dev, flat.shape[0], rt.RT_GEOM_CAPSULES)])
        ident = np.zeros(1, rt.INSTANCE)
        ident["object_to_world"][0] = np.eye(3, 4, dtype=np.float32)
        ftlas, frec, _ = tlas_over(ident, ftable, 1)
        new = lambda any_hit, ctr=None: q_new(any_hit, ctr, ftlas, frec, 1, table=ftable, geom=fgeom, num_blas=1)
        alone = lambda any_hit, ctr=None: q_caps(any_hit, ctr, flat_dev, flat_tree, flat.shape[0], hits)
        d = pair(new, alone, "capsules")
        d["new_call"].update(counted(new))
        d["capsules"].update(counted(alone))
        d["hit_fraction"] = round(float((hits[:, 1].view(torch.int32) != -1).float().mean()), 4)
        r["identity"] = d
        res[name] = r
        del blas, ball_tree, cap_tree, flat_dev, flat_tree, ftlas, tlas, ptlas
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="instance_capsule_bench", lib=os.environ.get("RT_LIB", "default"), blas_primitives=nb, instances=16,
                           primitives=16 * nb, rays="camera A %dx%d tiled" % (a.w, a.h), iters=a.iters, warmup=a.warmup,
                           rounds=a.rounds, results=res, device=torch.cuda.get_device_name(0)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
