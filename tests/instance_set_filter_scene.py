"""The filters and the bounce batch that tests/test_instance_set_filter_ref_cpu.py (oracle-built trees, host records) and the
GPU tests of the filtered instanced all-hit / first-K queries (device-built trees, the device's records) share, on the
12-instance scene of tests/ray_hits_instanced_scene.py.  Not a test file and not part of the reference."""
import numpy as np

import instance_filter_ref as ifr
import ray_first_instanced_ref as rfi
import ray_hits_ref as rh

F = np.float32
MISS = 0xFFFFFFFF
MIRROR = 4                    # the mirrored instance of ray_hits_instanced_scene.scene_instances
TWINS = (5, 6)                # the same BLAS in the same place
NEVER = (9, 10, 11)           # singular, bad BLAS, the empty tree: never entered
ARMS = ifr.ARMS               # instance_filter_ref.make_arm's: cull_back, cull_front, cull_disable, flip_facing, masks
BOUNCE_SEED = 23


def arm(name, num_instances, n):
    """instance_filter_ref.make_arm's filter (its CULL_DISABLE instances are 2 and the mirror, 4; its FLIP_FACING instance 2)"""
    return ifr.make_arm(name, num_instances, n)


def nearest_items(rows):
    """per ray the first item of the row in (t, instance, primitive_id) order, None for an empty row"""
    return [rfi.sorted_row(r)[0] if len(r) else None for r in rows]


def bounce(rays, rows, seed=BOUNCE_SEED):
    """the self-hit batch: for every ray with a non-empty row a ray that starts AT its nearest crossing o + t d (float32) in a
    random direction with tmin = 0, and its per-ray record (all-ones mask, skip = that crossing's (instance, primitive)).
    -> (RAY array, INSTANCE_RAY_FILTER array)"""
    near = nearest_items(rows)
    pick = [i for i, it in enumerate(near) if it is not None and np.isfinite(it["t"])]
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(len(pick), 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    out = np.zeros(len(pick), rh.RAY)
    per_ray = np.zeros(len(pick), ifr.INSTANCE_RAY_FILTER)
    per_ray["mask"] = ifr.ALL
    for j, i in enumerate(pick):
        it = near[i]
        with np.errstate(all="ignore"):
            out["origin"][j] = rays["origin"][i].astype(F) + (F(it["t"]) * rays["dir"][i].astype(F)).astype(F)
        per_ray["skip_instance"][j], per_ray["skip_id"][j] = it["instance"], it["primitive_id"]
    out["dir"] = d
    out["tmin"], out["tmax"] = 0.0, np.inf
    ok = np.isfinite(out["origin"]).all(1)
    return out[ok], per_ray[ok]


def skip_filter(per_ray):
    return ifr.InstanceFilter(0, 0, None, per_ray)           # (ray_mask 0: per_ray must win)


def skip_nearest(rows, only=None):
    """per-ray records that skip each ray's nearest crossing (of instance `only`, where given), all-ones masks"""
    per_ray = np.zeros(len(rows), ifr.INSTANCE_RAY_FILTER)
    per_ray["mask"], per_ray["skip_instance"], per_ray["skip_id"] = ifr.ALL, MISS, MISS
    for i, r in enumerate(rows):
        r = r if only is None else r[r["instance"] == only]
        if len(r):
            it = rfi.sorted_row(r)[0]
            per_ray["skip_instance"][i], per_ray["skip_id"][i] = it["instance"], it["primitive_id"]
    return per_ray


def half_masked(num_instances):
    """every odd instance masked out for every ray"""
    im = np.where(np.arange(num_instances) % 2 == 0, 1, 2).astype(np.uint32)
    return ifr.InstanceFilter(0, 1, ifr.instance_filters(num_instances, masks=im))


def none_admitted(num_instances):
    """masks that admit no instance: every instance mask 2, every ray mask 1"""
    return ifr.InstanceFilter(0, 1, ifr.instance_filters(num_instances, masks=np.full(num_instances, 2, np.uint32)))
