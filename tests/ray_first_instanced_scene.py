"""The two scenes and the rays that tests/test_ray_first_instanced_ref_cpu.py (oracle-built trees, host records) and
tests/test_gpu_ray_first_instanced.py (device-built trees, the device's records) share.  Not a test file and not part of the
reference.

The instanced all-hit scene (ray_hits_instanced_scene.scene_instances) places the Cornell BLAS twice in one place, instances 5
and 6, so every crossing of a wall ties exactly with its twin; a flat leaf box's front and the wall's t are one quantity
computed twice, so such rays are undecided whenever the front rounds above t (7 % of the rays at k = 1).  Hence two scenes:

main_instances(): scene_instances with the twins 5 and 6 re-pointed to the grid BLAS (table entry 0) under the same rotation at
    the same place; everything else stays -- the rotations, the non-uniform scale, the mirror, the nested instance, the
    singular, bad-BLAS and empty-tree instances.  Its undecided share stays within ray_first_ref.CAP.
twins_instances(): the existing scene, kept as the undecided case: claims 1 and 3 on every ray, claim 2 on its decided rays."""
import numpy as np

import instance_ref as ir
import ray_hits_instanced_scene as rsc
from ray_hits_instanced_scene import BLAS_SCENES, EMPTY_BLAS, NUM_BLAS, host_scene, scene_rays  # noqa: F401

TWINS = (5, 6)


def twins_instances(blas_tris):
    return rsc.scene_instances(blas_tris)


def main_instances(blas_tris):
    inst = rsc.scene_instances(blas_tris).copy()
    # scene_instances's own placement arithmetic for BLAS 0: R1 about the BLAS's centroid, scaled to the largest extent, at
    # (1.1, 1.1, 0) in units of that extent
    ext = [float(np.ptp(np.asarray(t).reshape(-1, 3), axis=0).max()) for t in blas_tris]
    cen = np.asarray(blas_tris[0], np.float64).reshape(-1, 3).mean(axis=0)
    s = max(ext)
    A = ir.rotation(0.3, -0.5, 0.9) * (s / ext[0])
    M = np.hstack([A, (np.asarray((1.1, 1.1, 0.0)) * s - A @ cen).reshape(3, 1)])
    for k in TWINS:
        inst["object_to_world"][k] = M.astype(np.float32)
        inst["blas"][k] = 0
    return inst
