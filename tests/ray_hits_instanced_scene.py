"""The scene and the rays that tests/test_ray_hits_instanced_ref_cpu.py (oracle-built trees, host records) and
tests/test_gpu_ray_hits_instanced.py (device-built trees, the device's records) share.  Not a test file and not part of the
reference: tests/ray_hits_instanced_ref.py stays numpy and instance_ref / ray_hits_ref only; this module may borrow the ray
generator of tests/test_gpu_instances.py."""
import numpy as np

import instance_ref as ir
import ray_hits_ref as rh
from ray_hits_instanced_ref import RECORD
from test_gpu_instances import _world_rays

F = np.float32
BLAS_SCENES = ("grid", "soup", "cornell")
EMPTY_BLAS = 3                # table entry 3: an empty tree (count 0)
NUM_BLAS = 4


def scene_instances(blas_tris):
    """12 instances of the three BLASes (+ the empty table entry 3): rotations, a non-uniform scale, a mirror, two instances of
    one BLAS in the same place, one nested inside another's box, a singular one, a bad-BLAS one, one of the empty tree.
    Instances 9, 10, 11 are never entered."""
    ext = [float(np.ptp(np.asarray(t).reshape(-1, 3), axis=0).max()) for t in blas_tris]
    cen = [np.asarray(t, np.float64).reshape(-1, 3).mean(axis=0) for t in blas_tris]
    s = max(ext)

    def place(b, A, at):
        """object_to_world = A about the BLAS's centroid, moved to `at` (in units of the largest extent)"""
        A = np.asarray(A, np.float64) * (s / ext[b])
        return np.hstack([A, (np.asarray(at, np.float64) * s - A @ cen[b]).reshape(3, 1)])

    R1, R2, R3 = ir.rotation(0.3, -0.5, 0.9), ir.rotation(-0.7, 0.2, 0.4), ir.rotation(1.1, 0.6, -0.3)
    mats = [
        place(0, R1, (0, 0, 0)),                                    # 0 rotation
        place(1, R2, (1.1, 0, 0)),                                  # 1 rotation, another BLAS
        place(2, R3, (0, 1.1, 0)),                                  # 2 rotation, the third BLAS
        place(0, np.diag([1.5, 0.6, 2.0]), (0, 0, 1.1)),            # 3 non-uniform scale
        place(1, np.diag([-1.0, 1.0, 1.0]), (-1.1, 0, 0)),          # 4 mirror (negative determinant)
        place(2, R1, (1.1, 1.1, 0)),                                # 5 ...
        place(2, R1, (1.1, 1.1, 0)),                                # 6 ... the same BLAS in the same place
        place(1, R3 * 0.3, (0, 1.1, 0)),                            # 7 nested inside instance 2's box
        place(0, R2 @ np.diag([1.0, 1.3, 0.7]), (0, -1.1, 0.3)),    # 8 rotation and scale
        np.zeros((3, 4)),                                           # 9 singular
        place(0, R1, (0.2, 0.1, 0)),                                # 10 bad BLAS (index 7 >= NUM_BLAS)
        place(0, R2, (0.3, 0.3, 0.3)),                              # 11 the empty tree
    ]
    return ir.instance_array(mats, [0, 1, 2, 0, 1, 2, 2, 1, 0, 0, 7, EMPTY_BLAS])


def host_scene(instances, blas_host_trees):
    """the CPU test's stand-in for rt_prepare_instances (the GPU tests read the device's own bytes): instance_ref.prepare's
    proxies, and records with the float64 inverse rounded to float32 (zeros and the flags for a flagged instance).
    blas_host_trees[b] = (leaves, nodes, root, count).  -> (proxies float32 [n, 9], RECORD array)"""
    boxes = [ir.root_box(t[1], t[2], t[3]) if 1 <= t[3] <= 7 else None for t in blas_host_trees]
    prox, inv, flags = ir.prepare(instances, boxes)
    rec = np.zeros(instances.size, RECORD)
    rec["world_to_object"] = np.where((flags == 0)[:, None, None], inv, 0.0).astype(F)
    rec["blas"], rec["flags"] = instances["blas"], flags
    return prox, rec


def scene_rays(world_tris, n_world=500, per_kind=256, seed=97):
    """test_gpu_instances._world_rays (rays from outside at interior points, then the same with random windows: 2 * n_world
    rays) plus ray_hits_ref.ray_sets on the world triangles (4 * per_kind rays): about 2,000 in all"""
    return np.concatenate([_world_rays(np.asarray(world_tris, np.float64), n_world, seed).astype(rh.RAY),
                           rh.ray_sets(np.asarray(world_tris, F), seed + 1, per_kind=per_kind).astype(rh.RAY)])
