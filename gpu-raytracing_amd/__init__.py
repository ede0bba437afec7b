"""gpu-raytracing_amd -- MI355X-native LBVH builder + primary-ray tracer (hot path of gregc-91/GPU-Raytracing).

Python is only the harness language here (tests, bench): the product is ``csrc/librt_amd.so`` -- hand-written
HIP kernels for gfx950 behind the C ABI of ``include/rt_abi.h`` -- and the C++ host mirror in ``host/``.
This module binds that C ABI with ctypes and mirrors the reference's entry points by name
(``BuildInput``, ``BuMemoryRequirements``, ``RunBottomUpBuild``, ``RadixSort``, ``Trace``; reference
``src/BuildWrapper.cuh:6-20``, ``src/RadixSort.cuh:6-7``, ``src/main.cu:125-127``), plus ray queries over any built
tree (``GenerateCameraRays``, ``IntersectRays``: rays tensor in, hits tensor out) and refit of a built tree after its
vertices moved (``BuildRefitPlan`` once per build, ``Refit`` per frame), instancing (``accel_table``,
``PrepareInstances``, ``IntersectRaysInstanced``: ray queries over placed copies of built trees), sphere primitives
(``PrepareSpheres``, ``IntersectRaysSpheres``: ray queries over a tree built on spheres), capsule primitives
(``PrepareCapsules``, ``IntersectRaysCapsules``: ray queries over a tree built on round linear segments), mixed instancing
(``geometry_table``, ``IntersectRaysInstancedMixed``: triangle and sphere BLASes under one TLAS), and closest-point queries
(``ClosestPoints``: the nearest triangle to each point, through any built tree), range queries (``RangeCount``,
``RangeCollect``, ``RangeQuery``: every triangle within a radius or overlapping a box, as CSR), k-nearest queries
(``KNearest``: the k nearest triangles to each point, in order), all-hit ray queries (``RayHitsCount``, ``RayHitsCollect``,
``RayHits``: every triangle a ray crosses inside its window, as CSR; ``RayHitsCountInstanced``, ``RayHitsCollectInstanced``,
``RayHitsInstanced``: the same over placed copies, each record with its instance; ``RayFirstHitsInstanced``: the k nearest
crossings over placed copies, in order, in one launch), triangle-overlap queries (``TriOverlapsCount``,
``TriOverlapsCollect``, ``TriOverlaps``: every triangle a query triangle cuts, as CSR; ``self_pairs`` for the
self-intersections of the mesh the tree was built over), signed distance and occupancy (``SignedDistance``, ``Occupancy``:
how far the nearest triangle is and whether a point is inside a closed mesh, in one launch; ``GenerateGridPoints`` for the
lattice such queries usually run on), hit filters for the ray queries (``HitFilter`` with ``IntersectRaysFiltered``,
``RayHitsCountFiltered``, ``RayHitsCollectFiltered``, ``RayFirstHitsFiltered``: face culling, a skip id per ray, primitive
masks against ray masks, applied inside the traversal), and ray sorting (``SortRays``: a coherence
order of a ray batch; ``IntersectRaysIndexed``: a query through that order or any list of ray indices).  torch is used for device
memory and streams only.  There is NO CPU fallback: if the HIP library is missing, import of the
native symbols fails loudly.

The directory name contains a hyphen, so import it with
``importlib.import_module("gpu-raytracing_amd")``.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librt_amd.so")

# ---------------------------------------------------------------- POD layouts (include/rt_abi.h)
TRIANGLE = np.dtype([("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3)])                        # 36 B
NODE = np.dtype([("min", "<f4", 3), ("w12", "<u4"), ("max", "<f4", 3), ("w28", "<u4")])              # 32 B
TRIANGLE_PAIR = np.dtype([("v0", "<f4", 3), ("primitive_id_0", "<u4"), ("v1", "<f4", 3), ("primitive_id_1", "<u4"),
                          ("v2", "<f4", 3), ("rotations", "<u2", 2), ("v3", "<f4", 3), ("pad3", "<f4")])  # 64 B
CAMERA = np.dtype([("position", "<f4", 3), ("pitch", "<f4"), ("w", "<f4", 3), ("yaw", "<f4"),
                   ("u", "<f4", 3), ("scale", "<f4"), ("v", "<f4", 3), ("max_depth", "<f4")])          # 64 B
ATTRIBUTES = np.dtype([("normal", "<f4", (3, 3)), ("pad0", "<u4"), ("uv", "<f4", (3, 2)),
                       ("material_id", "<i4"), ("pad1", "<u4")])                                     # 72 B
MATERIAL = np.dtype([("ambient", "<f4", 3), ("diffuse", "<f4", 3), ("specular", "<f4", 3),
                     ("specular_exp", "<f4"), ("texture", "<i4"), ("bump", "<i4"), ("disp", "<i4")])  # 52 B
assert TRIANGLE.itemsize == 36 and NODE.itemsize == 32 and TRIANGLE_PAIR.itemsize == 64
assert CAMERA.itemsize == 64 and ATTRIBUTES.itemsize == 72 and MATERIAL.itemsize == 52
# ray queries (rt_intersect_rays / rt_generate_camera_rays)
RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])                 # 32 B
HIT = np.dtype([("t", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])                          # 16 B
assert RAY.itemsize == 32 and HIT.itemsize == 16
MISS = 0xFFFFFFFF
kClosestHit, kAnyHit = 0, 1
kRaysRowMajor, kRaysTiled = 0, 1
# refit status flags (rt_refit_plan_layout.status)
RT_REFIT_BAD_TREE, RT_REFIT_PLAN_MISMATCH, RT_REFIT_PAIR_BROKEN = 1, 2, 4
RT_MOTION_TOPOLOGY_MISMATCH = 1    # rt_motion_validate's status flag
# instancing (rt_prepare_instances / rt_intersect_rays_instanced)
INSTANCE = np.dtype([("object_to_world", "<f4", (3, 4)), ("blas", "<u4"), ("pad", "<u4", 3)])                # 64 B
INSTANCE_RECORD = np.dtype([("world_to_object", "<f4", (3, 4)), ("blas", "<u4"), ("flags", "<u4"), ("spare", "<u4", 2)])
MOTION_INSTANCE = np.dtype([("object_to_world0", "<f4", (3, 4)), ("object_to_world1", "<f4", (3, 4)), ("blas", "<u4"),
                            ("pad", "<u4", 7)])                                                                 # 128 B
MOTION_INSTANCE_RECORD = np.dtype([("object_to_world0", "<f4", (3, 4)), ("object_to_world1", "<f4", (3, 4)), ("blas", "<u4"),
                                   ("flags", "<u4"), ("spare", "<u4", 6)])                                      # 128 B
ACCEL = np.dtype([("triangles", "<u8"), ("nodes", "<u8"), ("root", "<u4"), ("count", "<u4")])                # 24 B
assert INSTANCE.itemsize == 64 and INSTANCE_RECORD.itemsize == 64 and ACCEL.itemsize == 24
RT_INSTANCE_BAD_BLAS, RT_INSTANCE_SINGULAR = 1, 2
# sphere primitives (rt_prepare_spheres / rt_intersect_rays_spheres)
SPHERE = np.dtype([("center", "<f4", 3), ("radius", "<f4")])                                                 # 16 B
assert SPHERE.itemsize == 16
RT_SPHERE_BAD = 1
# capsule primitives (rt_prepare_capsules / rt_intersect_rays_capsules)
CAPSULE = np.dtype([("p0", "<f4", 3), ("radius", "<f4"), ("p1", "<f4", 3), ("pad", "<u4")])                  # 32 B
assert CAPSULE.itemsize == 32
RT_CAPSULE_BAD = 1
# sphere cast (rt_sphere_cast): which part of the triangle the ball touched
RT_SWEEP_NONE, RT_SWEEP_FACE, RT_SWEEP_EDGE, RT_SWEEP_CORNER, RT_SWEEP_OVERLAP = 0, 1, 2, 3, 4
# mixed instancing (rt_intersect_rays_instanced_mixed): what the leaves of each BLAS hold, parallel to the ACCEL table
GEOMETRY = np.dtype([("data", "<u8"), ("count", "<u4"), ("kind", "<u4")])                                    # 16 B
RT_GEOM_TRIANGLES = 0
RT_GEOM_SPHERES = 1
RT_GEOM_CAPSULES = 2      # entered by rt_intersect_rays_instanced_mixed_capsules only
# instanced deferred shading (rt_shade_frame_instanced): what a hit in BLAS b is shaded from, parallel to the BLAS table
SHADE_GEOMETRY = np.dtype([("triangles", "<u8"), ("attributes", "<u8"), ("num_triangles", "<u4"), ("material_base", "<i4"),
                           ("pad", "<u4", 2)])                                                                # 32 B
assert SHADE_GEOMETRY.itemsize == 32
RT_SHADE_RENORMALIZE = 1
# ray sorting (rt_sort_rays): a dead ray's key; every live key is below it
RAY_KEY_BITS, RAY_KEY_DEAD = 30, 1 << 29
# closest-point queries (rt_closest_points)
POINT_QUERY = np.dtype([("p", "<f4", 3), ("dist2_max", "<f4")])                                            # 16 B
POINT_HIT = np.dtype([("dist2", "<f4"), ("primitive_id", "<u4"), ("u", "<f4"), ("v", "<f4")])              # 16 B
assert POINT_QUERY.itemsize == 16 and POINT_HIT.itemsize == 16
RT_POINT_STACK_OVERFLOW = 1
# range queries (rt_range_count / rt_range_collect): sphere queries are POINT_QUERY records, box queries RANGE_BOX records
RANGE_BOX = np.dtype([("lo", "<f4", 3), ("pad0", "<u4"), ("hi", "<f4", 3), ("pad1", "<u4")])                # 32 B
assert RANGE_BOX.itemsize == 32
kRangeSphere, kRangeBox = 0, 1
RT_RANGE_STACK_OVERFLOW, RT_RANGE_TRUNCATED = 1, 2
# k-nearest queries (rt_k_nearest): POINT_QUERY records in, rows of k KNN_HIT records out
KNN_HIT = np.dtype([("dist2", "<f4"), ("primitive_id", "<u4")])                                              # 8 B
assert KNN_HIT.itemsize == 8
RT_KNN_MAX_K = 32
RT_KNN_STACK_OVERFLOW = 1
# all-hit ray queries (rt_ray_hits_count / rt_ray_hits_collect): RAY records in, CSR rows of HIT records out
RT_RAY_HITS_STACK_OVERFLOW, RT_RAY_HITS_TRUNCATED = 1, 2
# first-K ray queries (rt_ray_first_hits): RAY records in, rows of k HIT records out
RT_RAY_FIRST_MAX_K = 32
# rt_ray_filter: a ray's own mask and the primitive_id it skips (MISS: none); RT_FILTER_*: HitFilter.flags
RAY_FILTER = np.dtype([("mask", "<u4"), ("skip_id", "<u4")])                                                    # 8 B
RT_FILTER_CULL_BACK, RT_FILTER_CULL_FRONT = 1, 2
# rt_instance_filter / rt_instance_ray_filter (rt_intersect_rays_instanced_filtered): an instance's mask and
# RT_INSTANCE_FILTER_* flags; a ray's own mask and the (instance, primitive_id) pair it skips (skip_instance MISS: none)
INSTANCE_FILTER = np.dtype([("mask", "<u4"), ("flags", "<u4")])                                                 # 8 B
INSTANCE_RAY_FILTER = np.dtype([("mask", "<u4"), ("skip_instance", "<u4"), ("skip_id", "<u4"), ("pad", "<u4")])  # 16 B
assert INSTANCE_FILTER.itemsize == 8 and INSTANCE_RAY_FILTER.itemsize == 16
RT_INSTANCE_FILTER_CULL_DISABLE, RT_INSTANCE_FILTER_FLIP_FACING = 1, 2
RT_RAY_FIRST_STACK_OVERFLOW = 1
# triangle-overlap queries (rt_tri_overlaps_count / rt_tri_overlaps_collect): TRIANGLE records in, CSR rows of ids out
kTriSelf = 1
RT_TRI_STACK_OVERFLOW, RT_TRI_TRUNCATED = 1, 2
# signed distance and occupancy (rt_signed_distance / rt_occupancy): POINT_QUERY records in, SDF_HIT records or bytes out
SDF_HIT = np.dtype([("sdist", "<f4"), ("primitive_id", "<u4")])                                              # 8 B
assert SDF_HIT.itemsize == 8
RT_SDF_MAX_VOTES = 3
RT_SDF_STACK_OVERFLOW = 1
SDF_DEFAULT_DIRS = np.array([[0.577, 0.211, 0.789], [-0.683, 0.619, 0.387], [0.259, -0.857, 0.446]], np.float32)
SDF_DEFAULT_DIRS.setflags(write=False)
kGridRowMajor, kGridBricks = 0, 1

INDEX_MASK = 0x1FFFFFFF
CHILD_NONE, CHILD_BOX, CHILD_TRI = 0, 1, 2
# Arguments.h:8-26
kSAH, kBottomUp, kHybrid, kNone = 0, 1, 2, 3
kDepth, kBoxtests, kTriangleTests, kMaterialId, kLODs, kDiffuse, kTexture, kTextureLit, kTextureLitShadows = range(9)


class RtError(RuntimeError):
    pass


# ---------------------------------------------------------------- ctypes structs
class _BuildInput(ctypes.Structure):
    _fields_ = [("triangles_in", ctypes.c_void_p), ("triangles_out", ctypes.c_void_p),
                ("num_triangles", ctypes.c_uint32), ("nodes_out", ctypes.c_void_p), ("scratch", ctypes.c_void_p)]


class _Arguments(ctypes.Structure):
    _fields_ = [("build_type", ctypes.c_int32), ("enable_splits", ctypes.c_int32),
                ("enable_pairs", ctypes.c_int32), ("render_type", ctypes.c_int32)]


class _Accel(ctypes.Structure):
    _fields_ = [("triangles", ctypes.c_void_p), ("nodes", ctypes.c_void_p),
                ("root", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class _Scene(ctypes.Structure):
    _fields_ = [("attributes", ctypes.c_void_p), ("materials", ctypes.c_void_p), ("textures", ctypes.c_void_p),
                ("camera", ctypes.c_void_p), ("light", ctypes.c_float * 3),
                ("num_attributes", ctypes.c_uint32), ("num_materials", ctypes.c_uint32),
                ("num_textures", ctypes.c_uint32)]


NUM_LODS = 13  # Common.cuh:17


class _Texture(ctypes.Structure):  # rt_texture
    _fields_ = [("mips", ctypes.c_void_p * NUM_LODS), ("size_x", ctypes.c_int32 * NUM_LODS),
                ("size_y", ctypes.c_int32 * NUM_LODS), ("max_lod", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


assert ctypes.sizeof(_Texture) == 216


class _ScratchLayout(ctypes.Structure):
    _fields_ = [("p_aabb", ctypes.c_size_t), ("status", ctypes.c_size_t), ("num_leaves", ctypes.c_size_t),
                ("morton", ctypes.c_size_t),
                ("sorted_indices", ctypes.c_size_t), ("total", ctypes.c_size_t)]


class _SahScratchLayout(ctypes.Structure):
    _fields_ = [("p_aabb", ctypes.c_size_t), ("c_aabb", ctypes.c_size_t), ("status", ctypes.c_size_t),
                ("num_leaves", ctypes.c_size_t), ("cell_counts", ctypes.c_size_t), ("total", ctypes.c_size_t)]


class _RaySortLayout(ctypes.Structure):
    _fields_ = [("box", ctypes.c_size_t), ("num_live", ctypes.c_size_t), ("keys", ctypes.c_size_t),
                ("tmp_keys", ctypes.c_size_t), ("tmp_values", ctypes.c_size_t), ("sort", ctypes.c_size_t),
                ("total", ctypes.c_size_t)]


class _HitFilter(ctypes.Structure):  # rt_hit_filter
    _fields_ = [("flags", ctypes.c_uint32), ("ray_mask", ctypes.c_uint32), ("num_primitives", ctypes.c_uint32),
                ("pad", ctypes.c_uint32), ("prim_masks", ctypes.c_void_p), ("per_ray", ctypes.c_void_p)]


class _InstanceHitFilter(ctypes.Structure):  # rt_instance_hit_filter
    _fields_ = [("flags", ctypes.c_uint32), ("ray_mask", ctypes.c_uint32), ("num_instance_filters", ctypes.c_uint32),
                ("pad", ctypes.c_uint32), ("per_instance", ctypes.c_void_p), ("per_ray", ctypes.c_void_p)]


class _MotionAccel(ctypes.Structure):  # rt_motion_accel
    _fields_ = [("triangles0", ctypes.c_void_p), ("nodes0", ctypes.c_void_p), ("triangles1", ctypes.c_void_p),
                ("nodes1", ctypes.c_void_p), ("root", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class _MotionInstance(ctypes.Structure):  # rt_motion_instance (MOTION_INSTANCE's mirror)
    _fields_ = [("object_to_world0", ctypes.c_float * 12), ("object_to_world1", ctypes.c_float * 12),
                ("blas", ctypes.c_uint32), ("pad", ctypes.c_uint32 * 7)]


class _MotionInstanceRecord(ctypes.Structure):  # rt_motion_instance_record (MOTION_INSTANCE_RECORD's mirror)
    _fields_ = [("object_to_world0", ctypes.c_float * 12), ("object_to_world1", ctypes.c_float * 12),
                ("blas", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("spare", ctypes.c_uint32 * 6)]


class _RefitPlanLayout(ctypes.Structure):
    _fields_ = [("status", ctypes.c_size_t), ("parents", ctypes.c_size_t), ("arrivals", ctypes.c_size_t),
                ("leaves", ctypes.c_size_t), ("total", ctypes.c_size_t)]


EXPORTS = ["rt_bu_memory_requirements", "rt_nodes_bytes", "rt_run_bottom_up_build", "rt_bu_scratch_layout_get",
           "rt_sah_memory_requirements", "rt_run_sah_build", "rt_sah_scratch_layout_get",
           "rt_calculate_scene_aabb", "rt_generate_morton_codes", "rt_radix_sort_scratch_bytes",
           "rt_radix_sort_u32_pairs", "rt_radix_sort_u32_pairs_bits", "rt_radix_sort_input_in_tmp", "rt_trace", "rt_trace_strips",
           "rt_intersect_rays", "rt_generate_camera_rays", "rt_refit_plan_bytes", "rt_refit_plan_layout_get",
           "rt_build_refit_plan", "rt_refit", "rt_motion_validate", "rt_intersect_rays_motion",
           "rt_prepare_instances", "rt_intersect_rays_instanced", "rt_prepare_motion_instances",
           "rt_intersect_rays_instanced_motion", "rt_prepare_spheres", "rt_intersect_rays_spheres",
           "rt_prepare_capsules", "rt_intersect_rays_capsules", "rt_sphere_cast",
           "rt_intersect_rays_instanced_mixed", "rt_closest_points",
           "rt_range_scratch_bytes", "rt_range_count", "rt_range_collect", "rt_k_nearest",
           "rt_ray_sort_scratch_bytes", "rt_ray_sort_layout_get", "rt_sort_rays", "rt_intersect_rays_indexed",
           "rt_ray_hits_scratch_bytes", "rt_ray_hits_count", "rt_ray_hits_collect",
           "rt_ray_first_hits",
           "rt_intersect_rays_filtered", "rt_ray_hits_count_filtered", "rt_ray_hits_collect_filtered",
           "rt_ray_first_hits_filtered", "rt_intersect_rays_instanced_filtered",
           "rt_tri_overlaps_scratch_bytes", "rt_tri_overlaps_count", "rt_tri_overlaps_collect",
           "rt_signed_distance", "rt_occupancy", "rt_generate_grid_points",
           "rt_generate_shadow_rays", "rt_shade_frame", "rt_shade_frame_instanced",
           "rt_ray_hits_count_instanced", "rt_ray_hits_collect_instanced", "rt_ray_first_hits_instanced",
           "rt_ray_hits_count_instanced_filtered", "rt_ray_hits_collect_instanced_filtered",
           "rt_ray_first_hits_instanced_filtered",
           "rt_intersect_rays_instanced_indexed", "rt_intersect_rays_instanced_motion_indexed",
           "rt_intersect_rays_instanced_mixed_indexed", "rt_intersect_rays_motion_indexed",
           "rt_intersect_rays_instanced_mixed_capsules",
           "rt_error_string", "rt_version_string"]

_lib = None


def lib() -> ctypes.CDLL:
    """Load csrc/librt_amd.so.  Fails loudly when it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # torch ships its own HIP runtime: it must be the one in the process before librt_amd.so resolves its HIP symbols
    # (loaded the other way round, the two runtimes disagree about the device: hipErrorNoDevice at the first launch)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.rt_bu_memory_requirements.restype = ctypes.c_size_t
    L.rt_bu_memory_requirements.argtypes = [u32]
    L.rt_nodes_bytes.restype = ctypes.c_size_t
    L.rt_nodes_bytes.argtypes = [u32]
    L.rt_run_bottom_up_build.restype = i32
    L.rt_run_bottom_up_build.argtypes = [ctypes.POINTER(_BuildInput), ctypes.POINTER(_Arguments), i32, vp]
    L.rt_bu_scratch_layout_get.restype = i32
    L.rt_bu_scratch_layout_get.argtypes = [u32, ctypes.POINTER(_ScratchLayout)]
    L.rt_sah_memory_requirements.restype = ctypes.c_size_t
    L.rt_sah_memory_requirements.argtypes = [u32]
    L.rt_run_sah_build.restype = i32
    L.rt_run_sah_build.argtypes = [ctypes.POINTER(_BuildInput), ctypes.POINTER(_Arguments), vp]
    L.rt_sah_scratch_layout_get.restype = i32
    L.rt_sah_scratch_layout_get.argtypes = [u32, ctypes.POINTER(_SahScratchLayout)]
    L.rt_calculate_scene_aabb.restype = i32
    L.rt_calculate_scene_aabb.argtypes = [vp, u32, vp, vp]
    L.rt_generate_morton_codes.restype = i32
    L.rt_generate_morton_codes.argtypes = [vp, vp, vp, vp, u32, vp]
    L.rt_radix_sort_scratch_bytes.restype = ctypes.c_size_t
    L.rt_radix_sort_scratch_bytes.argtypes = [u32]
    L.rt_radix_sort_u32_pairs.restype = i32
    L.rt_radix_sort_u32_pairs.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    L.rt_radix_sort_u32_pairs_bits.restype = i32
    L.rt_radix_sort_u32_pairs_bits.argtypes = [vp, vp, vp, vp, u32, u32, i32, vp, vp]
    L.rt_radix_sort_input_in_tmp.restype = i32
    L.rt_radix_sort_input_in_tmp.argtypes = [u32, u32]
    L.rt_trace.restype = i32
    L.rt_trace.argtypes = [ctypes.POINTER(_Accel), ctypes.POINTER(_Scene), vp, i32, vp, u32, u32, u32, u32, u32, vp]
    L.rt_trace_strips.restype = i32
    L.rt_trace_strips.argtypes = [ctypes.POINTER(_Accel), ctypes.POINTER(_Scene), vp, i32, vp, u32, u32, u32, u32, u32, u32, vp]
    L.rt_intersect_rays.restype = i32
    L.rt_intersect_rays.argtypes = [ctypes.POINTER(_Accel), vp, vp, u32, i32, u32, vp, vp]
    L.rt_generate_camera_rays.restype = i32
    L.rt_generate_camera_rays.argtypes = [vp, u32, u32, u32, i32, vp, vp]
    L.rt_refit_plan_bytes.restype = ctypes.c_size_t
    L.rt_refit_plan_bytes.argtypes = [u32]
    L.rt_refit_plan_layout_get.restype = i32
    L.rt_refit_plan_layout_get.argtypes = [u32, ctypes.POINTER(_RefitPlanLayout)]
    L.rt_build_refit_plan.restype = i32
    L.rt_build_refit_plan.argtypes = [ctypes.POINTER(_BuildInput), u32, u32, vp, vp]
    L.rt_refit.restype = i32
    L.rt_refit.argtypes = [ctypes.POINTER(_BuildInput), u32, u32, vp, vp]
    L.rt_motion_validate.restype = i32
    L.rt_motion_validate.argtypes = [ctypes.POINTER(_MotionAccel), u32, vp, vp]
    L.rt_intersect_rays_motion.restype = i32
    L.rt_intersect_rays_motion.argtypes = [ctypes.POINTER(_MotionAccel), vp, vp, vp, u32, i32, vp, vp]
    L.rt_prepare_instances.restype = i32
    L.rt_prepare_instances.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp]
    L.rt_intersect_rays_instanced.restype = i32
    L.rt_intersect_rays_instanced.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, vp, vp, u32, i32, u32, vp, vp]
    L.rt_prepare_motion_instances.restype = i32
    L.rt_prepare_motion_instances.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp]
    L.rt_intersect_rays_instanced_motion.restype = i32
    L.rt_intersect_rays_instanced_motion.argtypes = [ctypes.POINTER(_MotionAccel), vp, u32, vp, u32, vp, vp, vp, vp, u32, i32, vp,
                                                     vp]
    L.rt_prepare_spheres.restype = i32
    L.rt_prepare_spheres.argtypes = [vp, u32, vp, vp, vp]
    L.rt_intersect_rays_spheres.restype = i32
    L.rt_intersect_rays_spheres.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, vp, i32, vp, vp]
    L.rt_prepare_capsules.restype = i32
    L.rt_prepare_capsules.argtypes = [vp, u32, vp, vp, vp]
    L.rt_intersect_rays_capsules.restype = i32
    L.rt_intersect_rays_capsules.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, vp, i32, vp, vp]
    L.rt_sphere_cast.restype = i32
    L.rt_sphere_cast.argtypes = [ctypes.POINTER(_Accel), vp, vp, ctypes.c_float, u32, vp, u32, vp, vp, i32, vp, vp]
    L.rt_intersect_rays_instanced_mixed.restype = i32
    L.rt_intersect_rays_instanced_mixed.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, vp, u32, vp, vp, vp, u32, i32, vp, vp]
    L.rt_closest_points.restype = i32
    L.rt_closest_points.argtypes = [ctypes.POINTER(_Accel), vp, vp, u32, vp, vp, vp]
    L.rt_range_scratch_bytes.restype = ctypes.c_size_t
    L.rt_range_scratch_bytes.argtypes = [u32]
    L.rt_range_count.restype = i32
    L.rt_range_count.argtypes = [ctypes.POINTER(_Accel), vp, u32, i32, vp, vp, vp, vp, vp]
    L.rt_range_collect.restype = i32
    L.rt_range_collect.argtypes = [ctypes.POINTER(_Accel), vp, u32, i32, vp, vp, vp, vp, vp, vp]
    L.rt_k_nearest.restype = i32
    L.rt_k_nearest.argtypes = [ctypes.POINTER(_Accel), vp, u32, u32, vp, vp, vp, vp]
    L.rt_ray_sort_scratch_bytes.restype = ctypes.c_size_t
    L.rt_ray_sort_scratch_bytes.argtypes = [u32]
    L.rt_ray_sort_layout_get.restype = i32
    L.rt_ray_sort_layout_get.argtypes = [u32, ctypes.POINTER(_RaySortLayout)]
    L.rt_sort_rays.restype = i32
    L.rt_sort_rays.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, vp, vp]
    L.rt_intersect_rays_indexed.restype = i32
    L.rt_intersect_rays_indexed.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, i32, u32, vp, vp]
    L.rt_ray_hits_scratch_bytes.restype = ctypes.c_size_t
    L.rt_ray_hits_scratch_bytes.argtypes = [u32]
    L.rt_ray_hits_count.restype = i32
    L.rt_ray_hits_count.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, vp, vp, vp, vp]
    L.rt_ray_hits_collect.restype = i32
    L.rt_ray_hits_collect.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, vp, vp, vp, vp, vp]
    L.rt_ray_first_hits.restype = i32
    L.rt_ray_first_hits.argtypes = [ctypes.POINTER(_Accel), vp, u32, u32, vp, vp, vp, vp]
    fl = ctypes.POINTER(_HitFilter)
    L.rt_intersect_rays_filtered.restype = i32
    L.rt_intersect_rays_filtered.argtypes = [ctypes.POINTER(_Accel), vp, vp, u32, i32, u32, fl, vp, vp]
    L.rt_ray_hits_count_filtered.restype = i32
    L.rt_ray_hits_count_filtered.argtypes = [ctypes.POINTER(_Accel), vp, u32, fl, vp, vp, vp, vp, vp]
    L.rt_ray_hits_collect_filtered.restype = i32
    L.rt_ray_hits_collect_filtered.argtypes = [ctypes.POINTER(_Accel), vp, u32, fl, vp, vp, vp, vp, vp, vp]
    L.rt_ray_first_hits_filtered.restype = i32
    L.rt_ray_first_hits_filtered.argtypes = [ctypes.POINTER(_Accel), vp, u32, u32, fl, vp, vp, vp, vp]
    L.rt_intersect_rays_instanced_filtered.restype = i32
    L.rt_intersect_rays_instanced_filtered.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, vp, vp, u32, i32, u32,
                                                       ctypes.POINTER(_InstanceHitFilter), vp, vp]
    L.rt_ray_hits_count_instanced.restype = i32
    L.rt_ray_hits_count_instanced.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, vp, vp, vp, vp, vp]
    L.rt_ray_hits_collect_instanced.restype = i32
    L.rt_ray_hits_collect_instanced.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.rt_ray_first_hits_instanced.restype = i32
    L.rt_ray_first_hits_instanced.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, u32, vp, vp, vp, vp, vp]
    ifl = ctypes.POINTER(_InstanceHitFilter)
    L.rt_ray_hits_count_instanced_filtered.restype = i32
    L.rt_ray_hits_count_instanced_filtered.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, ifl, vp, vp, vp, vp, vp]
    L.rt_ray_hits_collect_instanced_filtered.restype = i32
    L.rt_ray_hits_collect_instanced_filtered.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, ifl, vp, vp, vp, vp,
                                                         vp, vp, vp]
    L.rt_ray_first_hits_instanced_filtered.restype = i32
    L.rt_ray_first_hits_instanced_filtered.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, u32, ifl, vp, vp, vp, vp,
                                                       vp]
    L.rt_intersect_rays_instanced_indexed.restype = i32
    L.rt_intersect_rays_instanced_indexed.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, u32, vp, u32, vp, u32, vp, vp, i32, u32,
                                                      ifl, vp, vp]
    L.rt_intersect_rays_instanced_motion_indexed.restype = i32
    L.rt_intersect_rays_instanced_motion_indexed.argtypes = [ctypes.POINTER(_MotionAccel), vp, u32, vp, u32, vp, vp, u32, vp, u32,
                                                             vp, vp, i32, vp, vp]
    L.rt_intersect_rays_instanced_mixed_indexed.restype = i32
    L.rt_intersect_rays_instanced_mixed_indexed.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, vp,
                                                            i32, vp, vp]
    L.rt_intersect_rays_instanced_mixed_capsules.restype = i32
    L.rt_intersect_rays_instanced_mixed_capsules.argtypes = [ctypes.POINTER(_Accel), vp, u32, vp, vp, u32, vp, u32, vp, u32, vp,
                                                             vp, i32, vp, vp]
    L.rt_intersect_rays_motion_indexed.restype = i32
    L.rt_intersect_rays_motion_indexed.argtypes = [ctypes.POINTER(_MotionAccel), vp, vp, u32, vp, u32, vp, i32, vp, vp]
    L.rt_tri_overlaps_scratch_bytes.restype = ctypes.c_size_t
    L.rt_tri_overlaps_scratch_bytes.argtypes = [u32]
    L.rt_tri_overlaps_count.restype = i32
    L.rt_tri_overlaps_count.argtypes = [ctypes.POINTER(_Accel), vp, u32, u32, vp, vp, vp, vp, vp]
    L.rt_tri_overlaps_collect.restype = i32
    L.rt_tri_overlaps_collect.argtypes = [ctypes.POINTER(_Accel), vp, u32, u32, vp, vp, vp, vp, vp, vp]
    fp = ctypes.POINTER(ctypes.c_float)
    L.rt_signed_distance.restype = i32
    L.rt_signed_distance.argtypes = [ctypes.POINTER(_Accel), vp, u32, u32, fp, vp, vp, vp, vp]
    L.rt_occupancy.restype = i32
    L.rt_occupancy.argtypes = [ctypes.POINTER(_Accel), vp, u32, u32, fp, vp, vp, vp, vp]
    L.rt_generate_grid_points.restype = i32
    L.rt_generate_grid_points.argtypes = [fp, fp, ctypes.POINTER(u32), ctypes.c_float, i32, vp, vp]
    L.rt_generate_shadow_rays.restype = i32
    L.rt_generate_shadow_rays.argtypes = [vp, vp, u32, u32, ctypes.POINTER(ctypes.c_float), vp, vp]
    L.rt_shade_frame.restype = i32
    L.rt_shade_frame.argtypes = [ctypes.POINTER(_Scene), vp, u32, vp, vp, vp, u32, u32, u32, i32, i32, vp, vp]
    L.rt_shade_frame_instanced.restype = i32
    L.rt_shade_frame_instanced.argtypes = [ctypes.POINTER(_Scene), vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, u32, u32, u32, i32, i32,
                                           u32, vp, vp]
    L.rt_error_string.restype = ctypes.c_char_p
    L.rt_error_string.argtypes = [i32]
    L.rt_version_string.restype = ctypes.c_char_p
    _lib = L
    return L


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RtError(f"{what} failed: {rc} ({lib().rt_error_string(rc).decode()})")


def _torch():
    import torch
    return torch


def _stream_ptr(stream) -> int:
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def device_bytes(nbytes: int, device="cuda"):
    """Uninitialised device buffer (256-byte aligned by the caching allocator)."""
    torch = _torch()
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def to_device(arr: np.ndarray, device="cuda"):
    torch = _torch()
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(device)


def to_host(t, dtype: np.dtype, count: Optional[int] = None, offset: int = 0) -> np.ndarray:
    """Copy (part of) a device byte buffer back as a numpy array of `dtype`."""
    dtype = np.dtype(dtype)
    nbytes = t.numel() - offset if count is None else count * dtype.itemsize
    return t[offset:offset + nbytes].cpu().numpy().view(dtype).copy()


# ---------------------------------------------------------------- reference-named entry points
def BuMemoryRequirements(num_triangles: int) -> int:
    """BuildWrapper.cu:132-136"""
    return int(lib().rt_bu_memory_requirements(num_triangles))


def NodesBytes(num_triangles: int) -> int:
    """main.cu:235-237"""
    return int(lib().rt_nodes_bytes(num_triangles))


@dataclass
class Arguments:
    """Arguments.h:28-33 (defaults as in the reference)"""
    build_type: int = kSAH
    enable_splits: bool = False
    enable_pairs: bool = False
    render_type: int = kDepth


@dataclass
class BuildInput:
    """BuildWrapper.cuh:6-12; fields are torch uint8 device buffers owned by the caller."""
    triangles_in: object
    triangles_out: object
    num_triangles: int
    nodes_out: object
    scratch: object

    @staticmethod
    def allocate(triangles: np.ndarray, device="cuda", sah: bool = False) -> "BuildInput":
        """What Display() does at frame 0 (main.cu:226-240): allocate the four buffers, upload triangles.
        sah: size the scratch with SahMemoryRequirements instead of BuMemoryRequirements (main.cu:227-234)."""
        tri = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
        n = tri.shape[0]
        return BuildInput(triangles_in=to_device(tri, device) if n else device_bytes(64, device),
                          triangles_out=device_bytes(64 * max(n, 1) + 64, device), num_triangles=n,
                          nodes_out=device_bytes(NodesBytes(n), device),
                          scratch=device_bytes(SahMemoryRequirements(n) if sah else BuMemoryRequirements(n), device))


def RunBottomUpBuild(inp: BuildInput, args: Optional[Arguments] = None, hybrid: bool = False, stream=None) -> None:
    """BuildWrapper.cu:253-362.  Asynchronous on `stream` (torch current stream by default)."""
    args = args or Arguments(build_type=kHybrid if hybrid else kBottomUp)
    ci = _BuildInput(_ptr(inp.triangles_in), _ptr(inp.triangles_out), inp.num_triangles, _ptr(inp.nodes_out),
                     _ptr(inp.scratch))
    ca = _Arguments(args.build_type, int(args.enable_splits), int(args.enable_pairs), args.render_type)
    _check(lib().rt_run_bottom_up_build(ctypes.byref(ci), ctypes.byref(ca), int(hybrid), _stream_ptr(stream)),
           "rt_run_bottom_up_build")


def SahMemoryRequirements(num_triangles: int) -> int:
    """BuildWrapper.cu:126-130"""
    return int(lib().rt_sah_memory_requirements(num_triangles))


def RunSahBuild(inp: BuildInput, args: Optional[Arguments] = None, stream=None) -> None:
    """BuildWrapper.cu:140-251.  Trace root = (0, 1).  Asynchronous on `stream` (no copy, no synchronisation: graph-capturable);
    error flags in the scratch status word (sah_scratch_layout(n).status)."""
    args = args or Arguments(build_type=kSAH)
    ci = _BuildInput(_ptr(inp.triangles_in), _ptr(inp.triangles_out), inp.num_triangles, _ptr(inp.nodes_out),
                     _ptr(inp.scratch))
    ca = _Arguments(args.build_type, int(args.enable_splits), int(args.enable_pairs), args.render_type)
    _check(lib().rt_run_sah_build(ctypes.byref(ci), ctypes.byref(ca), _stream_ptr(stream)), "rt_run_sah_build")


def sah_scratch_layout(num_triangles: int) -> _SahScratchLayout:
    out = _SahScratchLayout()
    _check(lib().rt_sah_scratch_layout_get(num_triangles, ctypes.byref(out)), "rt_sah_scratch_layout_get")
    return out


def scratch_layout(num_triangles: int) -> _ScratchLayout:
    out = _ScratchLayout()
    _check(lib().rt_bu_scratch_layout_get(num_triangles, ctypes.byref(out)), "rt_bu_scratch_layout_get")
    return out


def CalculateSceneAabb(triangles_dev, n: int, aabb_dev, stream=None) -> None:
    """Multiblock.cu:104-114 (aabb_dev: 6 x int32, ordered-int encoded)"""
    _check(lib().rt_calculate_scene_aabb(_ptr(triangles_dev), n, _ptr(aabb_dev), _stream_ptr(stream)),
           "rt_calculate_scene_aabb")


def GenerateMortonCodes(codes_dev, values_dev, triangles_dev, aabb_dev, n: int, stream=None) -> None:
    """BottomUpBuilder.cu:98-115"""
    _check(lib().rt_generate_morton_codes(_ptr(codes_dev), _ptr(values_dev), _ptr(triangles_dev), _ptr(aabb_dev), n,
                                          _stream_ptr(stream)), "rt_generate_morton_codes")


def RadixSort(keys, values, temp1, temp2, count: int, sort_scratch=None, stream=None) -> None:
    """RadixSort.cuh:6-7.  The reference mallocs its tables per call (RadixSort.cu:187-190); here the caller may
    pass `sort_scratch` (>= RadixSortScratchBytes(count)), else one is taken from torch's caching allocator."""
    if sort_scratch is None:
        sort_scratch = device_bytes(int(lib().rt_radix_sort_scratch_bytes(count)), keys.device)
    _check(lib().rt_radix_sort_u32_pairs(_ptr(keys), _ptr(values), _ptr(temp1), _ptr(temp2), count,
                                         _ptr(sort_scratch), _stream_ptr(stream)), "rt_radix_sort_u32_pairs")


def RadixSortBits(keys, values, temp1, temp2, count: int, key_bits: int, input_in_tmp: bool = False, sort_scratch=None,
                  stream=None) -> None:
    """rt_radix_sort_u32_pairs_bits: the sort for keys of `key_bits` significant bits (the builder's Morton codes: 30)."""
    if sort_scratch is None:
        sort_scratch = device_bytes(int(lib().rt_radix_sort_scratch_bytes(count)), keys.device)
    _check(lib().rt_radix_sort_u32_pairs_bits(_ptr(keys), _ptr(values), _ptr(temp1), _ptr(temp2), count, key_bits,
                                              int(input_in_tmp), _ptr(sort_scratch), _stream_ptr(stream)),
           "rt_radix_sort_u32_pairs_bits")


def RadixSortScratchBytes(count: int) -> int:
    return int(lib().rt_radix_sort_scratch_bytes(count))


class DeviceTextures:
    """The device-side Texture table of DeviceScene (Common.cuh:342-351, uploaded by main.cu:100-113): one
    rt_texture per texture, mips in device memory.  `chains` is a list of mip chains, each a list of [sy, sx]
    uint32 arrays (r | g<<8 | b<<16 | a<<24), level 0 first."""

    def __init__(self, chains, device="cuda"):
        table = (_Texture * max(1, len(chains)))()
        self._mips = []
        for t, chain in enumerate(chains):
            if not 1 <= len(chain) <= NUM_LODS:
                raise ValueError("a texture has 1..13 mip levels")
            for l, m in enumerate(chain):
                m = np.ascontiguousarray(m, np.uint32)
                d = to_device(m, device)
                self._mips.append(d)
                table[t].mips[l] = _ptr(d)
                table[t].size_x[l], table[t].size_y[l] = m.shape[1], m.shape[0]
            table[t].max_lod = len(chain) - 1
        self.count = len(chains)
        self.table = to_device(np.frombuffer(bytes(table), np.uint8).copy(), device)


def Trace(triangles, nodes, rgba8, dims, camera, root: int, count: int, *, render_type: int = kDepth,
          attributes=None, materials=None, num_materials: int = 0, light=(0.0, 0.0, 0.0), counters=None,
          rows=None, spp: int = 1, stream=None, textures: Optional[DeviceTextures] = None, strips=None,
          num_primitives: int = 0) -> None:
    """main.cu:125-192 Trace(): `camera` is a 64-byte DEVICE buffer, `rgba8` a w*h*4-byte device buffer
    (the reference writes a GL surface; row 0 first).  rows=(y0, y1) restricts to a row band (multi-GPU tiling);
    strips=(strip_rows, first, stride) renders interleaved strips into a COMPACT buffer (rt_trace_strips).
    num_primitives: DeviceScene::num_attributes (main.cu:166 sets it to the triangle count; 0 = unknown) -- the library
    reads it as the scene size when it picks the tracer instantiation (pair prefetch from 8M primitives on)."""
    w, h = int(dims[0]), int(dims[1])
    y0, y1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    if strips is not None:
        a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
        s = _Scene(_ptr(attributes), _ptr(materials), _ptr(textures.table) if textures is not None else 0, _ptr(camera),
                   (ctypes.c_float * 3)(*[float(x) for x in light]),
                   int(num_primitives), num_materials, textures.count if textures is not None else 0)
        _check(lib().rt_trace_strips(ctypes.byref(a), ctypes.byref(s), _ptr(counters), render_type, _ptr(rgba8), w, h,
                                     int(strips[0]), int(strips[1]), int(strips[2]), spp, _stream_ptr(stream)),
               "rt_trace_strips")
        return
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    s = _Scene(_ptr(attributes), _ptr(materials), _ptr(textures.table) if textures is not None else 0, _ptr(camera),
               (ctypes.c_float * 3)(*[float(x) for x in light]),
               int(num_primitives), num_materials, textures.count if textures is not None else 0)
    _check(lib().rt_trace(ctypes.byref(a), ctypes.byref(s), _ptr(counters), render_type, _ptr(rgba8), w, h, y0, y1,
                          spp, _stream_ptr(stream)), "rt_trace")


def _nbytes(t) -> int:
    return int(t.numel()) * int(t.element_size())


def CameraRayCount(w: int, h: int, spp: int = 1, tiled: bool = False) -> int:
    """Number of rays GenerateCameraRays writes: w*h*spp row-major, ceil(w/8)*ceil(h/8)*spp*64 tiled."""
    return ((w + 7) // 8) * ((h + 7) // 8) * spp * 64 if tiled else w * h * spp


def GenerateCameraRays(camera, w: int, h: int, rays, *, spp: int = 1, tiled: bool = False, stream=None) -> int:
    """rt_generate_camera_rays: the primary rays Trace() traces, as RAY records (`rays`: a contiguous device tensor of at
    least CameraRayCount(w, h, spp, tiled) * 32 bytes, e.g. float32 [N, 8]; `camera`: a 64-byte device buffer as for Trace).
    Row-major: ray (y*w + x)*spp + s.  Tiled: ray (tile*spp + s)*64 + lane, 8x8 tiles row by row, lane = Morton position in
    the tile; off-frame lanes get tmax < tmin.  Returns the number of rays written."""
    n = CameraRayCount(int(w), int(h), int(spp), tiled)
    if not rays.is_contiguous() or _nbytes(rays) < 32 * n:
        raise ValueError(f"rays must be a contiguous device buffer of >= {32 * n} bytes")
    _check(lib().rt_generate_camera_rays(_ptr(camera), int(w), int(h), int(spp), kRaysTiled if tiled else kRaysRowMajor,
                                         _ptr(rays), _stream_ptr(stream)), "rt_generate_camera_rays")
    return n


def IntersectRays(triangles, nodes, root: int, count: int, rays, hits, *, any_hit: bool = False, num_primitives: int = 0,
                  counters=None, stream=None) -> None:
    """rt_intersect_rays: one HIT record per RAY record of `rays` (a contiguous device tensor of 32-byte records, e.g.
    float32 [N, 8]) into `hits` (>= 16 N bytes, e.g. float32 [N, 4]; view it as int32 for primitive_id).  Any tree Trace()
    takes (`triangles` / `nodes` as for Trace, root / count of its root node).  Closest hit by default; any_hit=True
    ends each ray at its first accepted triangle.  A miss is {+inf, MISS, 0, 0}.  counters: optional int64[4] device
    tensor, added to as by Trace.  num_primitives: scene-size hint as for Trace.  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits a contiguous device buffer")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n:
        raise ValueError(f"hits must hold {n} 16-byte records")
    if n == 0:
        return
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_intersect_rays(ctypes.byref(a), _ptr(rays), _ptr(hits), n, kAnyHit if any_hit else kClosestHit,
                                   int(num_primitives), _ptr(counters), _stream_ptr(stream)), "rt_intersect_rays")


def RefitPlanBytes(num_triangles: int) -> int:
    """rt_refit_plan_bytes: device bytes of a refit plan for n triangles (36 per triangle + about 18 KB)."""
    return int(lib().rt_refit_plan_bytes(num_triangles))


def refit_plan_layout(num_triangles: int) -> _RefitPlanLayout:
    out = _RefitPlanLayout()
    _check(lib().rt_refit_plan_layout_get(num_triangles, ctypes.byref(out)), "rt_refit_plan_layout_get")
    return out


def _build_input(inp: BuildInput) -> _BuildInput:
    return _BuildInput(_ptr(inp.triangles_in), _ptr(inp.triangles_out), inp.num_triangles, _ptr(inp.nodes_out),
                       _ptr(inp.scratch))


def BuildRefitPlan(inp: BuildInput, root: int, count: int, plan, stream=None) -> None:
    """rt_build_refit_plan: walk the tree built into `inp` from its root (root, count as for Trace) and fill `plan` (a device
    buffer of >= RefitPlanBytes(n) bytes, 256-byte aligned, e.g. device_bytes(RefitPlanBytes(n))).  Once per build.
    Asynchronous on `stream`; errors land in the plan's status word (refit_status)."""
    ci = _build_input(inp)
    _check(lib().rt_build_refit_plan(ctypes.byref(ci), int(root), int(count), _ptr(plan), _stream_ptr(stream)),
           "rt_build_refit_plan")


def Refit(inp: BuildInput, root: int, count: int, plan, stream=None) -> None:
    """rt_refit: inp.triangles_in holds the NEW positions (same triangles, same order as at build time); rewrites the leaf
    records in inp.triangles_out and the boxes of the reachable slots in inp.nodes_out.  `plan` from BuildRefitPlan on the
    same tree.  Asynchronous on `stream`, one launch; status flags in the plan (refit_status)."""
    ci = _build_input(inp)
    _check(lib().rt_refit(ctypes.byref(ci), int(root), int(count), _ptr(plan), _stream_ptr(stream)), "rt_refit")


def refit_status(plan, num_triangles: int) -> int:
    """The plan's RT_REFIT_* flags (copies the status word back: waits for the work queued before it on the current stream).
    Sticky: BuildRefitPlan clears them, every Refit only adds to them."""
    return int(to_host(plan, np.uint32, 1, refit_plan_layout(num_triangles).status)[0])


def MotionPose(inp: BuildInput, root: int, count: int, moved_triangles):
    """The second key pose of a motion query: clones inp.triangles_out / inp.nodes_out (the built tree, pose 0), builds a refit
    plan on the clone (a plan fingerprints its nodes_out) and refits it with `moved_triangles` (the same triangles in the same
    order, moved: a numpy [n, 9] array or a device buffer of TRIANGLE records).  Returns (pose 1 as a BuildInput whose
    triangles_in holds the moved triangles, its plan): Refit(pose1, root, count, plan) moves it again.  The plan's status
    (refit_status) must be 0.  On a split tree refit pose 0 with its own triangles first (rt_abi.h, motion block).
    Asynchronous on the current stream; composes BuildRefitPlan and Refit."""
    moved = moved_triangles if hasattr(moved_triangles, "data_ptr") else \
        to_device(np.ascontiguousarray(moved_triangles, np.float32).reshape(-1, 9), inp.nodes_out.device)
    pose1 = BuildInput(triangles_in=moved, triangles_out=inp.triangles_out.clone(), num_triangles=inp.num_triangles,
                       nodes_out=inp.nodes_out.clone(), scratch=inp.scratch)
    plan = device_bytes(RefitPlanBytes(inp.num_triangles), inp.nodes_out.device)
    BuildRefitPlan(pose1, root, count, plan)
    Refit(pose1, root, count, plan)
    return pose1, plan


def _pose(pose):
    """(triangles, nodes) of a key pose given as such a pair or as a BuildInput"""
    return (pose.triangles_out, pose.nodes_out) if isinstance(pose, BuildInput) else pose


def _motion_accel(pose0, pose1, root: int, count: int) -> _MotionAccel:
    (t0, n0), (t1, n1) = _pose(pose0), _pose(pose1)
    return _MotionAccel(_ptr(t0), _ptr(n0), _ptr(t1), _ptr(n1), int(root), int(count))


def MotionValidate(pose0, pose1, root: int, count: int, num_triangles: int, status, stream=None) -> None:
    """rt_motion_validate: sets RT_MOTION_TOPOLOGY_MISMATCH in `status` (a device uint32) when the two poses ((triangles, nodes)
    pairs or BuildInputs) are not one tree -- a w12 / w28 word, an id or a rotation differs -- and clears it otherwise.  Once per
    pair of poses.  Asynchronous on `stream`; read the word with motion_status."""
    a = _motion_accel(pose0, pose1, root, count)
    _check(lib().rt_motion_validate(ctypes.byref(a), int(num_triangles), _ptr(status), _stream_ptr(stream)), "rt_motion_validate")


def motion_status(status) -> int:
    """The RT_MOTION_* flags of the last MotionValidate (copies the word back: waits for the work queued before it)."""
    return _status_word(status)


def IntersectRaysMotion(pose0, pose1, root: int, count: int, rays, times, hits, *, any_hit: bool = False, counters=None,
                        stream=None) -> None:
    """rt_intersect_rays_motion: IntersectRays with a time per ray over two key poses of one tree.  pose0 / pose1: (triangles,
    nodes) pairs or BuildInputs -- pose 0 the built tree, pose 1 from MotionPose.  `times`: a contiguous device float32 tensor,
    one value in [0, 1] per ray; ray i sees the tree interpolated at times[i] (w0 * pose0 + t * pose1, w0 = 1 - t).  A ray with a
    NaN time or one outside [0, 1] is a miss.  rays / hits / any_hit / counters as for IntersectRays.  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or not times.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, times / hits contiguous device buffers")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n or _nbytes(times) < 4 * n:
        raise ValueError(f"hits must hold {n} 16-byte records and times {n} floats")
    if n == 0:
        return
    a = _motion_accel(pose0, pose1, root, count)
    _check(lib().rt_intersect_rays_motion(ctypes.byref(a), _ptr(rays), _ptr(times), _ptr(hits), n,
                                          kAnyHit if any_hit else kClosestHit, _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_motion")


def accel_table(trees, device="cuda"):
    """The device BLAS table of instancing: one rt_accel per (triangles, nodes, root, count) of `trees` (e.g. a BuildInput's
    triangles_out / nodes_out and its trace root), as an ACCEL-array device buffer.  The caller keeps the trees alive."""
    tab = np.zeros(len(trees), ACCEL)
    for k, (tris, nodes, root, count) in enumerate(trees):
        tab[k] = (_ptr(tris), _ptr(nodes), int(root), int(count))
    return to_device(tab, device)


def PrepareInstances(instances, num_instances: int, blas_table, num_blas: int, proxies, records, status, stream=None) -> None:
    """rt_prepare_instances: `instances` (INSTANCE records, device), the BLAS table (accel_table) -> `proxies` (num_instances
    TRIANGLE records: the TLAS build input, e.g. a BuildInput's triangles_in), `records` (INSTANCE_RECORD, the query's input)
    and `status` (a device uint32 the call clears; RT_INSTANCE_* flags, see instance_status).  Asynchronous on `stream`."""
    _check(lib().rt_prepare_instances(_ptr(instances), int(num_instances), _ptr(blas_table), int(num_blas), _ptr(proxies),
                                      _ptr(records), _ptr(status), _stream_ptr(stream)), "rt_prepare_instances")


def _status_word(status) -> int:
    return int(to_host(status, np.uint32, 1)[0])


def instance_status(status) -> int:
    """The RT_INSTANCE_* flags of the last PrepareInstances (copies the word back: waits for the work queued before it)."""
    return _status_word(status)


def IntersectRaysInstanced(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                           num_blas: int, rays, hits, instance_ids, *, any_hit: bool = False, num_primitives: int = 0,
                           counters=None, stream=None) -> None:
    """rt_intersect_rays_instanced: IntersectRays through a TLAS (built over PrepareInstances's proxies; root / count of its
    root) and the instances' BLASes.  `instance_ids` (>= 4 N bytes, e.g. int32 [N]) gets the instance of each hit or MISS;
    hits[i] carries the BLAS's own primitive_id and (u, v) and the world-space t.  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or not instance_ids.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits / instance_ids contiguous buffers")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n or _nbytes(instance_ids) < 4 * n:
        raise ValueError(f"hits must hold {n} 16-byte records and instance_ids {n} words")
    if n == 0:
        return
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_intersect_rays_instanced(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                             int(num_blas), _ptr(rays), _ptr(hits), _ptr(instance_ids), n,
                                             kAnyHit if any_hit else kClosestHit, int(num_primitives), _ptr(counters),
                                             _stream_ptr(stream)), "rt_intersect_rays_instanced")


def PrepareMotionInstances(instances, num_instances: int, blas_table, num_blas: int, proxies0, proxies1, records, status,
                           stream=None) -> None:
    """rt_prepare_motion_instances: `instances` (MOTION_INSTANCE records, device: two key matrices per instance), the BLAS table
    (accel_table) -> `proxies0` / `proxies1` (num_instances TRIANGLE records each: the TLAS build input of pose 0 and the refit
    input of pose 1, e.g. MotionPose's moved_triangles), `records` (MOTION_INSTANCE_RECORD, the query's input) and `status` (a
    device uint32 the call clears; RT_INSTANCE_* flags, see instance_status).  Asynchronous on `stream`."""
    n = int(num_instances)
    for name, buf, size in (("instances", instances, 128), ("proxies0", proxies0, 36), ("proxies1", proxies1, 36),
                            ("records", records, 128)):
        if n and (not buf.is_contiguous() or _nbytes(buf) < size * n):
            raise ValueError(f"{name} must be a contiguous device buffer of {n} {size}-byte records")
    _check(lib().rt_prepare_motion_instances(_ptr(instances), n, _ptr(blas_table), int(num_blas), _ptr(proxies0), _ptr(proxies1),
                                             _ptr(records), _ptr(status), _stream_ptr(stream)), "rt_prepare_motion_instances")


def IntersectRaysInstancedMotion(tlas_pose0, tlas_pose1, root: int, count: int, records, num_instances: int, blas_table,
                                 num_blas: int, rays, times, hits, instance_ids, *, any_hit: bool = False, counters=None,
                                 stream=None) -> None:
    """rt_intersect_rays_instanced_motion: IntersectRaysInstanced with a time per ray over two key transforms of every instance.
    tlas_pose0 / tlas_pose1: (triangles, nodes) pairs or BuildInputs -- pose 0 the TLAS built over PrepareMotionInstances's
    proxies0, pose 1 from MotionPose(tlas, root, count, proxies1).  `records`: PrepareMotionInstances's.  `times`: a contiguous
    device float32 tensor, one value in [0, 1] per ray (NaN or outside: a miss).  hits / instance_ids / any_hit / counters as for
    IntersectRaysInstanced.  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or not instance_ids.is_contiguous() or not times.is_contiguous() \
            or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, times / hits / instance_ids contiguous "
                         "device buffers")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n or _nbytes(instance_ids) < 4 * n or _nbytes(times) < 4 * n:
        raise ValueError(f"hits must hold {n} 16-byte records, instance_ids {n} words and times {n} floats")
    if num_instances and (not records.is_contiguous() or _nbytes(records) < 128 * int(num_instances)):
        raise ValueError(f"records must be a contiguous device buffer of {int(num_instances)} 128-byte records")
    if n == 0:
        return
    a = _motion_accel(tlas_pose0, tlas_pose1, root, count)
    _check(lib().rt_intersect_rays_instanced_motion(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                    int(num_blas), _ptr(rays), _ptr(times), _ptr(hits), _ptr(instance_ids), n,
                                                    kAnyHit if any_hit else kClosestHit, _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_instanced_motion")


def PrepareSpheres(spheres, num_spheres: int, proxies, status, stream=None) -> None:
    """rt_prepare_spheres: `spheres` (SPHERE records, device, e.g. float32 [N, 4]: centre, radius) -> `proxies` (num_spheres
    TRIANGLE records: the build input of any builder with pairs and splits off, e.g. a BuildInput's triangles_in; prepare into
    them again and Refit for moving spheres) and `status` (a device uint32 the call clears; RT_SPHERE_BAD when a sphere is not
    valid, see sphere_status).  Asynchronous on `stream`."""
    n = int(num_spheres)
    for name, buf, size in (("spheres", spheres, 16), ("proxies", proxies, 36)):
        if n and (not buf.is_contiguous() or _nbytes(buf) < size * n):
            raise ValueError(f"{name} must be a contiguous device buffer of {n} {size}-byte records")
    _check(lib().rt_prepare_spheres(_ptr(spheres), n, _ptr(proxies), _ptr(status), _stream_ptr(stream)), "rt_prepare_spheres")


def sphere_status(status) -> int:
    """The RT_SPHERE_* flags of the last PrepareSpheres (copies the word back: waits for the work queued before it)."""
    return _status_word(status)


def IntersectRaysSpheres(triangles, nodes, root: int, count: int, spheres, num_spheres: int, rays, hits, *,
                         any_hit: bool = False, order=None, num_indices: Optional[int] = None, counters=None,
                         stream=None) -> None:
    """rt_intersect_rays_spheres: IntersectRays over a tree built on PrepareSpheres's proxies (`triangles` / `nodes`: its
    triangles_out / nodes_out, root / count of its root) and the `spheres` it was prepared from.  A HIT record carries t, the
    sphere index as primitive_id, u = 1 when the ray began inside the sphere (its far root was taken) else 0, v = 0; a miss is
    {+inf, MISS, 0, 0}.  `order` (optional): a contiguous device tensor of uint32 / int32 words -- SortRays's output on this
    tree, or any list of ray indices -- used as by IntersectRaysIndexed; num_indices: how many of its words (default: all).
    counters: optional int64[4] device tensor (box tests, sphere tests, wave steps).  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits a contiguous device buffer")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n:
        raise ValueError(f"hits must hold {n} 16-byte records")
    ns = int(num_spheres)
    if ns and (not spheres.is_contiguous() or _nbytes(spheres) < 16 * ns):
        raise ValueError(f"spheres must be a contiguous device buffer of {ns} 16-byte records")
    k = 0
    if order is not None:
        if not order.is_contiguous():
            raise ValueError("order must be a contiguous device buffer")
        k = _nbytes(order) // 4 if num_indices is None else int(num_indices)
        if _nbytes(order) < 4 * k:
            raise ValueError(f"order must hold {k} words")
        if k == 0:
            return
    if n == 0:
        return
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_intersect_rays_spheres(ctypes.byref(a), _ptr(spheres), ns, _ptr(rays), n, _ptr(order), k, _ptr(hits),
                                           kAnyHit if any_hit else kClosestHit, _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_spheres")


def PrepareCapsules(capsules, num_capsules: int, proxies, status, stream=None) -> None:
    """rt_prepare_capsules: `capsules` (CAPSULE records, device, e.g. float32 [N, 8]: p0, radius, p1, pad) -> `proxies`
    (num_capsules TRIANGLE records: the build input of any builder with pairs and splits off; prepare into them again and Refit
    for moving capsules) and `status` (a device uint32 the call clears; RT_CAPSULE_BAD when a capsule is not valid, see
    capsule_status).  Asynchronous on `stream`."""
    n = int(num_capsules)
    for name, buf, size in (("capsules", capsules, 32), ("proxies", proxies, 36)):
        if n and (not buf.is_contiguous() or _nbytes(buf) < size * n):
            raise ValueError(f"{name} must be a contiguous device buffer of {n} {size}-byte records")
    _check(lib().rt_prepare_capsules(_ptr(capsules), n, _ptr(proxies), _ptr(status), _stream_ptr(stream)),
           "rt_prepare_capsules")


def capsule_status(status) -> int:
    """The RT_CAPSULE_* flags of the last PrepareCapsules (copies the word back: waits for the work queued before it)."""
    return _status_word(status)


def IntersectRaysCapsules(triangles, nodes, root: int, count: int, capsules, num_capsules: int, rays, hits, *,
                          any_hit: bool = False, order=None, num_indices: Optional[int] = None, counters=None,
                          stream=None) -> None:
    """rt_intersect_rays_capsules: IntersectRaysSpheres over a tree built on PrepareCapsules's proxies and the `capsules` it was
    prepared from.  A HIT record carries t, the capsule index as primitive_id, u = 1 when the ray began inside the capsule (its
    far crossing was taken) else 0, and v = where along the axis the ray crossed: 0 on p0's cap, 1 on p1's cap, between them on
    the body; a miss is {+inf, MISS, 0, 0}.  `order`, num_indices, counters (box tests, capsule tests, wave steps) as for
    IntersectRaysSpheres.  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits a contiguous device buffer")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n:
        raise ValueError(f"hits must hold {n} 16-byte records")
    nc = int(num_capsules)
    if nc and (not capsules.is_contiguous() or _nbytes(capsules) < 32 * nc):
        raise ValueError(f"capsules must be a contiguous device buffer of {nc} 32-byte records")
    k = 0
    if order is not None:
        if not order.is_contiguous():
            raise ValueError("order must be a contiguous device buffer")
        k = _nbytes(order) // 4 if num_indices is None else int(num_indices)
        if _nbytes(order) < 4 * k:
            raise ValueError(f"order must hold {k} words")
        if k == 0:
            return
    if n == 0:
        return
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_intersect_rays_capsules(ctypes.byref(a), _ptr(capsules), nc, _ptr(rays), n, _ptr(order), k, _ptr(hits),
                                            kAnyHit if any_hit else kClosestHit, _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_capsules")


def SphereCast(triangles, nodes, root: int, count: int, rays, hits, radii=None, radius: float = 0.0, features=None, order=None,
               any_hit: bool = False, counters=None, *, num_indices: Optional[int] = None, stream=None) -> None:
    """rt_sphere_cast: a ball swept along each ray over any triangle tree IntersectRays takes (`triangles` / `nodes`: the
    builder's triangles_out / nodes_out, root / count of its root).  `radii` (optional): a contiguous device float32 buffer, one
    world-space radius per ray; without it every ray takes `radius` (finite, not negative).  A HIT record carries t = the
    centre's parameter at first contact, primitive_id, and (u, v) = the weights of the contact point on the triangle for the
    caller's corners v1 and v2: the contact normal is (o + t*d - contact) / radius.  A miss is {+inf, MISS, 0, 0}.  `features`
    (optional): a contiguous device uint32 / int32 buffer, one RT_SWEEP_* word per ray -- which part of the triangle was
    touched, RT_SWEEP_OVERLAP when the ball touches at tmin already, RT_SWEEP_NONE on a miss.  A ray with a negative, NaN or
    infinite radius is not traced.  Radius 0 gives IntersectRays's records.  `order`, num_indices and counters (box tests,
    leaves visited, wave steps) as for IntersectRaysSpheres.  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits a contiguous device buffer")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n:
        raise ValueError(f"hits must hold {n} 16-byte records")
    if radii is not None:
        if not radii.is_contiguous() or radii.element_size() != 4 or not radii.dtype.is_floating_point or _nbytes(radii) < 4 * n:
            raise ValueError(f"radii must be a contiguous device buffer of {n} float32 values")
    else:
        radius = float(radius)
        if not (0.0 <= radius < float("inf")):
            raise ValueError("radius must be finite and not negative")
    if features is not None and (not features.is_contiguous() or features.element_size() != 4 or _nbytes(features) < 4 * n):
        raise ValueError(f"features must be a contiguous device buffer of {n} 32-bit words")
    k = 0
    if order is not None:
        if not order.is_contiguous():
            raise ValueError("order must be a contiguous device buffer")
        k = _nbytes(order) // 4 if num_indices is None else int(num_indices)
        if _nbytes(order) < 4 * k:
            raise ValueError(f"order must hold {k} words")
        if k == 0:
            return
    if n == 0:
        return
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_sphere_cast(ctypes.byref(a), _ptr(rays), _ptr(radii), float(radius), n, _ptr(order), k, _ptr(hits),
                                _ptr(features), kAnyHit if any_hit else kClosestHit, _ptr(counters), _stream_ptr(stream)),
           "rt_sphere_cast")


def geometry_table(entries, device="cuda"):
    """The device geometry table of mixed instancing, parallel to accel_table's: one rt_geometry per BLAS.  An entry is None
    for a triangle BLAS, (spheres, num_spheres) for a sphere BLAS -- the device SPHERE buffer its tree was prepared from --, or
    (buffer, n, kind) with kind RT_GEOM_SPHERES or RT_GEOM_CAPSULES: for capsules the device CAPSULE buffer (32-byte records)
    the tree was prepared from, which only IntersectRaysInstancedMixedCapsules enters.  The caller keeps the buffers alive."""
    tab = np.zeros(len(entries), GEOMETRY)
    for k, e in enumerate(entries):
        if e is None:
            tab[k] = (0, 0, RT_GEOM_TRIANGLES)
            continue
        if len(e) == 3:
            buf, ns, kind = e
            if kind not in (RT_GEOM_SPHERES, RT_GEOM_CAPSULES):
                raise ValueError(f"entry {k}: kind must be RT_GEOM_SPHERES or RT_GEOM_CAPSULES")
            if kind == RT_GEOM_CAPSULES:
                if int(ns) and (not buf.is_contiguous() or _nbytes(buf) < 32 * int(ns)):
                    raise ValueError(f"entry {k}: capsules must be a contiguous device buffer of {int(ns)} 32-byte records")
                tab[k] = (_ptr(buf), int(ns), RT_GEOM_CAPSULES)
                continue
            e = (buf, ns)
        spheres, ns = e
        if int(ns) and (not spheres.is_contiguous() or _nbytes(spheres) < 16 * int(ns)):
            raise ValueError(f"entry {k}: spheres must be a contiguous device buffer of {int(ns)} 16-byte records")
        tab[k] = (_ptr(spheres), int(ns), RT_GEOM_SPHERES)
    return to_device(tab, device)


def IntersectRaysInstancedMixed(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                                geom_table, num_blas: int, rays, hits, instance_ids, *, any_hit: bool = False, counters=None,
                                stream=None) -> None:
    """rt_intersect_rays_instanced_mixed: IntersectRaysInstanced over a BLAS table whose trees hold triangles or spheres;
    `geom_table` (geometry_table, parallel to `blas_table`) says which.  A hit in a triangle BLAS is IntersectRaysInstanced's
    record, a hit in a sphere BLAS is IntersectRaysSpheres's (t, the sphere index, u = 1 for the far root, v = 0); tell them
    apart by instance_ids[i] -> records[].blas -> the table's kind.  geom_table=None: every BLAS holds triangles
    (IntersectRaysInstanced with num_primitives = 0).  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or not instance_ids.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits / instance_ids contiguous buffers")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n or _nbytes(instance_ids) < 4 * n:
        raise ValueError(f"hits must hold {n} 16-byte records and instance_ids {n} words")
    if geom_table is not None and (not geom_table.is_contiguous() or _nbytes(geom_table) < 16 * int(num_blas)):
        raise ValueError(f"geom_table must be a contiguous device buffer of {int(num_blas)} 16-byte records")
    if n == 0:
        return
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_intersect_rays_instanced_mixed(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                   _ptr(geom_table), int(num_blas), _ptr(rays), _ptr(hits), _ptr(instance_ids),
                                                   n, kAnyHit if any_hit else kClosestHit, _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_instanced_mixed")


def ClosestPoints(triangles, nodes, root: int, count: int, queries, hits, *, counters=None, status=None, stream=None) -> None:
    """rt_closest_points: one POINT_HIT record per POINT_QUERY record of `queries` (a contiguous device tensor of 16-byte
    records (p, dist2_max), e.g. float32 [N, 4]) into `hits` (>= 16 N bytes, e.g. float32 [N, 4]; view it as int32 for
    primitive_id).  Any tree Trace() takes (`triangles` / `nodes` as for Trace, root / count of its root node).  The record is
    the lexicographic minimum of (dist2, primitive_id) over the triangles within dist2_max; a miss is {+inf, MISS, 0, 0}.
    counters: optional int64[4] device tensor ([0] box tests, [1] triangle tests).  status: optional device uint32 the call
    ORs RT_POINT_STACK_OVERFLOW into (the caller clears it; see point_status).  Asynchronous on `stream`."""
    if not queries.is_contiguous() or not hits.is_contiguous() or _nbytes(queries) % 16:
        raise ValueError("queries must be a contiguous device buffer of 16-byte records, hits a contiguous device buffer")
    n = _nbytes(queries) // 16
    if _nbytes(hits) < 16 * n:
        raise ValueError(f"hits must hold {n} 16-byte records")
    if n == 0:
        return
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_closest_points(ctypes.byref(a), _ptr(queries), _ptr(hits), n, _ptr(counters), _ptr(status),
                                   _stream_ptr(stream)), "rt_closest_points")


def point_status(status) -> int:
    """The RT_POINT_* flags ClosestPoints ORed into `status` (copies the word back: waits for the work queued before it)."""
    return _status_word(status)


def _csr_count(entry, scratch_bytes, tree, queries, n: int, extra, offsets, *, scratch, counters, status, stream) -> int:
    """The count call of a CSR query family: the offsets / scratch checks, then the call.  entry: the library's rt_*_count;
    scratch_bytes: the family's public *ScratchBytes; tree: (triangles, nodes, root, count); extra: the family's own arguments
    between the batch size and the offsets."""
    if not offsets.is_contiguous() or _nbytes(offsets) < 8 * (n + 1):
        raise ValueError(f"offsets must be a contiguous device buffer of {n + 1} 64-bit words")
    if scratch is None:
        scratch = device_bytes(scratch_bytes(n), queries.device)
    elif _nbytes(scratch) < scratch_bytes(n):
        raise ValueError(f"scratch must hold {scratch_bytes.__name__}({n}) bytes")
    triangles, nodes, root, count = tree
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    # (an empty torch tensor has no storage; the call still wants a pointer and, with n = 0, reads nothing through it)
    _check(entry(ctypes.byref(a), _ptr(queries) or _ptr(scratch), n, *extra, _ptr(offsets), _ptr(scratch), _ptr(counters),
                 _ptr(status), _stream_ptr(stream)), entry.__name__)
    return n


def _csr_collect(entry, tree, queries, n: int, extra, offsets, rows, rows_name: str, *, counts, counters, status, stream) -> int:
    """The collect call of a CSR query family: the offsets / rows / counts checks, then the call.  entry: the library's
    rt_*_collect; tree, extra: as for _csr_count; rows: the output (`rows_name` in the error message)."""
    if not offsets.is_contiguous() or not rows.is_contiguous() or _nbytes(offsets) < 8 * (n + 1):
        raise ValueError(f"offsets must be a contiguous device buffer of {n + 1} 64-bit words, {rows_name} a contiguous device buffer")
    if counts is not None and (not counts.is_contiguous() or _nbytes(counts) < 4 * n):
        raise ValueError(f"counts must hold {n} words")
    if n == 0:
        return 0
    triangles, nodes, root, count = tree
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(entry(ctypes.byref(a), _ptr(queries), n, *extra, _ptr(offsets), _ptr(rows), _ptr(counts), _ptr(counters), _ptr(status),
                 _stream_ptr(stream)), entry.__name__)
    return n


def _on_stream(stream):
    """The context in which torch's own work (an .item() read-back, an allocation, a sort) goes to `stream`."""
    return _torch().cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def RangeScratchBytes(num_queries: int) -> int:
    """rt_range_scratch_bytes: device bytes of RangeCount's scratch (8 bytes per 256 queries, 256-byte aligned)."""
    return int(lib().rt_range_scratch_bytes(int(num_queries)))


def _range_batch(queries, shape: int) -> int:
    rec = {kRangeSphere: 16, kRangeBox: 32}.get(int(shape))
    if rec is None:
        raise ValueError("shape must be kRangeSphere or kRangeBox")
    if not queries.is_contiguous() or _nbytes(queries) % rec:
        raise ValueError(f"queries must be a contiguous device buffer of {rec}-byte records")
    return _nbytes(queries) // rec


def RangeCount(triangles, nodes, root: int, count: int, queries, offsets, *, shape: int = kRangeSphere, scratch=None,
               counters=None, status=None, stream=None) -> int:
    """rt_range_count: offsets[0 .. N] (a contiguous device int64 tensor of >= N + 1 words) = the exclusive prefix sum of the
    number of triangles each query matches; offsets[N] is the total.  `queries`: kRangeSphere -- 16-byte POINT_QUERY records
    (p, dist2_max), e.g. float32 [N, 4]; kRangeBox -- 32-byte RANGE_BOX records (lo, -, hi, -), e.g. float32 [N, 8].  Any tree
    Trace() takes.  scratch: >= RangeScratchBytes(N) bytes, 256-byte aligned (device_bytes; taken from torch's allocator when
    None).  counters: optional int64[4] ([0] box tests, [1] triangle tests).  status: optional device uint32 the call ORs
    RT_RANGE_* flags into (see range_status).  Asynchronous on `stream`, nothing is read back.  Returns N."""
    n = _range_batch(queries, shape)
    return _csr_count(lib().rt_range_count, RangeScratchBytes, (triangles, nodes, root, count), queries, n, (int(shape),), offsets,
                      scratch=scratch, counters=counters, status=status, stream=stream)


def RangeCollect(triangles, nodes, root: int, count: int, queries, offsets, ids, *, shape: int = kRangeSphere, counts=None,
                 counters=None, status=None, stream=None) -> int:
    """rt_range_collect: query i writes the ids of its first offsets[i+1] - offsets[i] matches at ids[offsets[i]:] (`ids`: a
    contiguous device int32 / uint32 tensor the offsets stay inside -- the caller's contract; `offsets`: int64 [N + 1] from
    RangeCount, or i * K for a fixed K per query).  counts: optional device int32 [N], each query's true match count.
    A query with more matches than room sets RT_RANGE_TRUNCATED in `status`.  Ids come in traversal order (unspecified but
    deterministic); on non-split trees each matching triangle appears exactly once.  Asynchronous on `stream`.  Returns N."""
    n = _range_batch(queries, shape)
    return _csr_collect(lib().rt_range_collect, (triangles, nodes, root, count), queries, n, (int(shape),), offsets, ids, "ids",
                        counts=counts, counters=counters, status=status, stream=stream)


def range_status(status) -> int:
    """The RT_RANGE_* flags RangeCount / RangeCollect ORed into `status` (copies the word back: waits for the work queued before it)."""
    return _status_word(status)


def RangeQuery(triangles, nodes, root: int, count: int, queries, *, shape: int = kRangeSphere, counters=None, status=None,
               stream=None):
    """Everything each query matches, as CSR: RangeCount, then the total offsets[N] is READ BACK TO THE HOST -- one
    synchronisation of `stream` per call, the only one -- to allocate the id array, then RangeCollect.  Returns (offsets, ids):
    torch int64 [N + 1] and int32 [total] device tensors; query i owns ids[offsets[i]:offsets[i+1]].  A caller who cannot
    afford the synchronisation (a captured graph, a fixed budget per query) uses RangeCount / RangeCollect directly.  With
    `counters`, the tests of both passes are added (twice one traversal)."""
    torch = _torch()
    n = _range_batch(queries, shape)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=queries.device)
    RangeCount(triangles, nodes, root, count, queries, offsets, shape=shape, counters=counters, status=status, stream=stream)
    with _on_stream(stream):
        total = int(offsets[n].item())
    ids = torch.empty(max(total, 1), dtype=torch.int32, device=queries.device)[:total]
    RangeCollect(triangles, nodes, root, count, queries, offsets, ids, shape=shape, counters=counters, status=status,
                 stream=stream)
    return offsets, ids


def RayHitsScratchBytes(num_rays: int) -> int:
    """rt_ray_hits_scratch_bytes: device bytes of RayHitsCount's scratch (8 bytes per 256 rays, 256-byte aligned)."""
    return int(lib().rt_ray_hits_scratch_bytes(int(num_rays)))


def _ray_batch(rays) -> int:
    if not rays.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records")
    return _nbytes(rays) // 32


def RayHitsCount(triangles, nodes, root: int, count: int, rays, offsets, *, scratch=None, counters=None, status=None,
                 stream=None) -> int:
    """rt_ray_hits_count: offsets[0 .. N] (a contiguous device int64 tensor of >= N + 1 words) = the exclusive prefix sum of the
    number of triangles each ray of `rays` (32-byte RAY records, e.g. float32 [N, 8]) crosses inside its [tmin, tmax] window;
    offsets[N] is the total.  Any tree Trace() takes.  scratch: >= RayHitsScratchBytes(N) bytes, 256-byte aligned
    (device_bytes; taken from torch's allocator when None).  counters: optional int64[4] ([0] box tests, [1] leaf records
    visited).  status: optional device uint32 the call ORs RT_RAY_HITS_* flags into (see ray_hits_status).  Asynchronous on
    `stream`, nothing is read back.  Returns N."""
    return _csr_count(lib().rt_ray_hits_count, RayHitsScratchBytes, (triangles, nodes, root, count), rays, _ray_batch(rays), (),
                      offsets, scratch=scratch, counters=counters, status=status, stream=stream)


def RayHitsCollect(triangles, nodes, root: int, count: int, rays, offsets, hits, *, counts=None, counters=None, status=None,
                   stream=None) -> int:
    """rt_ray_hits_collect: ray i writes the HIT records of its first offsets[i+1] - offsets[i] crossings at hits[offsets[i]:]
    (`hits`: a contiguous device buffer of 16-byte records, e.g. float32 [total, 4], that the offsets stay inside -- the
    caller's contract; `offsets`: int64 [N + 1] from RayHitsCount, or i * K for a fixed K per ray).  counts: optional device
    int32 [N], each ray's true row length.  A ray with more records than room sets RT_RAY_HITS_TRUNCATED in `status`.
    Records come in traversal order (unspecified but deterministic; RayFirstHits gives the first k in order); on non-split trees each
    crossed triangle appears exactly once.  Asynchronous on `stream`.  Returns N."""
    return _csr_collect(lib().rt_ray_hits_collect, (triangles, nodes, root, count), rays, _ray_batch(rays), (), offsets, hits,
                        "hits", counts=counts, counters=counters, status=status, stream=stream)


def ray_hits_status(status) -> int:
    """The RT_RAY_HITS_* flags RayHitsCount / RayHitsCollect ORed into `status` (copies the word back: waits for the work queued
    before it)."""
    return _status_word(status)


def RayHits(triangles, nodes, root: int, count: int, rays, *, sort: bool = False, counters=None, status=None, stream=None):
    """Every triangle each ray crosses, as CSR: RayHitsCount, then the total offsets[N] is READ BACK TO THE HOST -- one
    synchronisation of `stream` per call, the only one -- to allocate the record array, then RayHitsCollect.  Returns
    (offsets, hits): torch int64 [N + 1] and float32 [total, 4] device tensors (t, primitive_id bits, u, v; view column 1 as
    int32); ray i owns hits[offsets[i]:offsets[i+1]].  sort=True orders every row by ascending (t, primitive_id) on the device
    (two stable torch sorts over the records: plumbing, not a kernel).  A caller who cannot afford the synchronisation (a
    captured graph, a fixed budget per ray) uses RayHitsCount / RayHitsCollect directly.  With `counters`, the tests of both
    passes are added (twice one traversal)."""
    torch = _torch()
    n = _ray_batch(rays)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=rays.device)
    RayHitsCount(triangles, nodes, root, count, rays, offsets, counters=counters, status=status, stream=stream)
    with _on_stream(stream):
        total = int(offsets[n].item())
        hits = torch.empty((max(total, 1), 4), dtype=torch.float32, device=rays.device)[:total]
        RayHitsCollect(triangles, nodes, root, count, rays, offsets, hits, counters=counters, status=status, stream=stream)
        if sort and total > 1:
            # two stable sorts: by primitive_id (unsigned), then by the 64-bit key row << 32 | the monotone integer image of t
            # (-0 counted as +0), which keeps every record inside its row
            row = torch.repeat_interleave(torch.arange(n, device=rays.device), offsets[1:] - offsets[:-1], output_size=total)
            bits = hits.view(torch.int32).to(torch.int64)
            order = torch.argsort(bits[:, 1] & 0xFFFFFFFF, stable=True)
            tb = (hits[:, 0] + 0.0).contiguous().view(torch.int32).to(torch.int64)
            key = (row << 32) | (torch.where(tb >= 0, tb, tb ^ 0x7FFFFFFF) + (1 << 31))
            order = order[torch.argsort(key[order], stable=True)]
            hits = hits[order].contiguous()
    return offsets, hits


def RayHitsCountInstanced(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                          num_blas: int, rays, offsets, *, scratch=None, counters=None, status=None, stream=None) -> int:
    """rt_ray_hits_count_instanced: RayHitsCount through a TLAS (built over PrepareInstances's proxies without pairs or splits;
    root / count of its root) and the instances' BLASes: offsets[0 .. N] = the exclusive prefix sum of the number of crossings of
    each ray over all entered instances.  scratch: >= RayHitsScratchBytes(N) bytes, 256-byte aligned (taken from torch's
    allocator when None).  counters: optional int64[4] ([0] box tests of both levels, [1] BLAS leaf records visited).  status:
    optional device uint32 the call ORs RT_RAY_HITS_* flags into (see ray_hits_status).  N = 0: nothing runs.  Asynchronous on
    `stream`, nothing is read back.  Returns N."""
    n = _ray_batch(rays)
    if not offsets.is_contiguous() or _nbytes(offsets) < 8 * (n + 1):
        raise ValueError(f"offsets must be a contiguous device buffer of {n + 1} 64-bit words")
    if n == 0:
        return 0
    if scratch is None:
        scratch = device_bytes(RayHitsScratchBytes(n), rays.device)
    elif _nbytes(scratch) < RayHitsScratchBytes(n):
        raise ValueError(f"scratch must hold RayHitsScratchBytes({n}) bytes")
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_ray_hits_count_instanced(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table), int(num_blas),
                                             _ptr(rays), n, _ptr(offsets), _ptr(scratch), _ptr(counters), _ptr(status),
                                             _stream_ptr(stream)), "rt_ray_hits_count_instanced")
    return n


def RayHitsCollectInstanced(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                            num_blas: int, rays, offsets, hits, instance_ids, *, counts=None, counters=None, status=None,
                            stream=None) -> int:
    """rt_ray_hits_collect_instanced: ray i writes the HIT records of its first offsets[i+1] - offsets[i] crossings at
    hits[offsets[i]:] and the instance of each at instance_ids[offsets[i]:] (`hits`: 16-byte records, `instance_ids`: 4-byte
    words, both contiguous device buffers the offsets stay inside -- the caller's contract; `offsets`: int64 [N + 1] from
    RayHitsCountInstanced, or i * K for a fixed K per ray).  A record carries the BLAS's own primitive_id and (u, v) and the
    world-space t.  counts: optional device int32 [N], each ray's true row length.  A ray with more records than room sets
    RT_RAY_HITS_TRUNCATED in `status`.  Order within a row: unspecified but deterministic.  Asynchronous on `stream`.
    Returns N."""
    n = _ray_batch(rays)
    if not offsets.is_contiguous() or not hits.is_contiguous() or not instance_ids.is_contiguous() or \
            _nbytes(offsets) < 8 * (n + 1):
        raise ValueError(f"offsets must be a contiguous device buffer of {n + 1} 64-bit words, hits / instance_ids contiguous "
                         "device buffers")
    if counts is not None and (not counts.is_contiguous() or _nbytes(counts) < 4 * n):
        raise ValueError(f"counts must hold {n} words")
    if n == 0:
        return 0
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_ray_hits_collect_instanced(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                               int(num_blas), _ptr(rays), n, _ptr(offsets), _ptr(hits), _ptr(instance_ids),
                                               _ptr(counts), _ptr(counters), _ptr(status), _stream_ptr(stream)),
           "rt_ray_hits_collect_instanced")
    return n


def RayHitsInstanced(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table, num_blas: int,
                     rays, *, sort: bool = False, counters=None, status=None, stream=None):
    """Every crossing of every placed copy, as CSR: RayHitsCountInstanced, then the total offsets[N] is READ BACK TO THE HOST --
    one synchronisation of `stream` per call, the only one, as in RayHits -- to allocate the rows, then
    RayHitsCollectInstanced.  Returns (offsets, hits, instance_ids): torch int64 [N + 1], float32 [total, 4] (t, primitive_id
    bits, u, v) and int32 [total] device tensors; ray i owns hits[offsets[i]:offsets[i+1]] and the same slice of instance_ids.
    sort=True orders every row by ascending (t, instance, primitive_id) on the device (stable torch sorts: plumbing, not a
    kernel).  With `counters`, the tests of both passes are added (twice one traversal)."""
    torch = _torch()
    n = _ray_batch(rays)
    tree = (tlas_triangles, tlas_nodes, root, count, records, num_instances, blas_table, num_blas)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=rays.device)    # (no fill kernel: nothing of torch's runs off `stream`)
    RayHitsCountInstanced(*tree, rays, offsets, counters=counters, status=status, stream=stream)
    with _on_stream(stream):
        if n == 0:
            offsets.zero_()                                                  # the count call runs nothing for an empty batch
        total = int(offsets[n].item())
        hits = torch.empty((max(total, 1), 4), dtype=torch.float32, device=rays.device)[:total]
        ids = torch.empty(max(total, 1), dtype=torch.int32, device=rays.device)[:total]
        RayHitsCollectInstanced(*tree, rays, offsets, hits, ids, counters=counters, status=status, stream=stream)
        if sort and total > 1:
            hits, ids = _sort_instanced_rows(offsets, hits, ids, n, total)
    return offsets, hits, ids


def _sort_instanced_rows(offsets, hits, ids, n: int, total: int):
    """sort=True of RayHitsInstanced[Filtered]: three stable sorts, by primitive_id (unsigned), by instance (unsigned), then by
    the 64-bit key row << 32 | the monotone integer image of t (-0 counted as +0), which keeps every record inside its row"""
    torch = _torch()
    row = torch.repeat_interleave(torch.arange(n, device=hits.device), offsets[1:] - offsets[:-1], output_size=total)
    bits = hits.view(torch.int32).to(torch.int64)
    order = torch.argsort(bits[:, 1] & 0xFFFFFFFF, stable=True)
    order = order[torch.argsort(ids.to(torch.int64)[order] & 0xFFFFFFFF, stable=True)]
    tb = (hits[:, 0] + 0.0).contiguous().view(torch.int32).to(torch.int64)
    key = (row << 32) | (torch.where(tb >= 0, tb, tb ^ 0x7FFFFFFF) + (1 << 31))
    order = order[torch.argsort(key[order], stable=True)]
    return hits[order].contiguous(), ids[order].contiguous()


def RayFirstHits(triangles, nodes, root: int, count: int, rays, k: int, out, *, counters=None, status=None, stream=None) -> int:
    """rt_ray_first_hits: for each ray of `rays` (32-byte RAY records, e.g. float32 [N, 8]) a row of k HIT records
    (t, primitive_id bits, u, v) in `out` (float32 [N, k, 4] on the device; view column 1 as int32): the k nearest crossings
    inside the ray's [tmin, tmax] window in ascending (t, primitive_id) order, padded with {+inf, MISS, 0, 0}.
    1 <= k <= RT_RAY_FIRST_MAX_K.  One launch: the window shrinks to the k-th hit while the ray is traced.  Any tree Trace()
    takes.  Exactness: include/rt_abi.h, first-K block (decided / undecided rays).  counters: optional int64[4] device tensor
    ([0] box tests, [1] leaf records visited).  status: optional device uint32 the call ORs RT_RAY_FIRST_STACK_OVERFLOW into
    (the caller clears it; see ray_first_status).  Asynchronous on `stream`, nothing is allocated or read back.  Returns N."""
    k = int(k)
    if not 1 <= k <= RT_RAY_FIRST_MAX_K:
        raise ValueError(f"k must be in 1 .. {RT_RAY_FIRST_MAX_K}")
    n = _ray_batch(rays)
    if not out.is_contiguous() or out.dtype != _torch().float32 or tuple(out.shape) != (n, k, 4):
        raise ValueError(f"out must be a contiguous float32 tensor of shape [{n}, {k}, 4]")
    if n == 0:
        return 0
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_ray_first_hits(ctypes.byref(a), _ptr(rays), n, k, _ptr(out), _ptr(counters), _ptr(status),
                                   _stream_ptr(stream)), "rt_ray_first_hits")
    return n


def RayFirstHitsInstanced(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                          num_blas: int, rays, k: int, hits, instance_ids, *, counters=None, status=None, stream=None) -> int:
    """rt_ray_first_hits_instanced: RayFirstHits through a TLAS (built over PrepareInstances's proxies without pairs or splits;
    root / count of its root) and the instances' BLASes: for each ray a row of k HIT records in `hits` (float32 [N, k, 4] on the
    device) and the instance of each in `instance_ids` (int32 [N, k]): the k nearest crossings over all placed copies in
    ascending (t, instance, primitive_id) order, padded with {+inf, MISS, 0, 0} / MISS.  A record carries the BLAS's own
    primitive_id and (u, v) and the world-space t.  1 <= k <= RT_RAY_FIRST_MAX_K.  One launch: the window shrinks to the k-th
    hit on both levels while the ray is traced.  Exactness: include/rt_abi.h, instanced first-K block (decided / undecided
    rays).  counters: optional int64[4] ([0] box tests of both levels, [1] BLAS leaf records visited).  status: optional device
    uint32 the call ORs RT_RAY_FIRST_STACK_OVERFLOW into (the caller clears it; see ray_first_status).  Asynchronous on
    `stream`, nothing is allocated or read back.  Returns N."""
    torch = _torch()
    k = int(k)
    if not 1 <= k <= RT_RAY_FIRST_MAX_K:
        raise ValueError(f"k must be in 1 .. {RT_RAY_FIRST_MAX_K}")
    n = _ray_batch(rays)
    if not hits.is_contiguous() or hits.dtype != torch.float32 or tuple(hits.shape) != (n, k, 4):
        raise ValueError(f"hits must be a contiguous float32 tensor of shape [{n}, {k}, 4]")
    if not instance_ids.is_contiguous() or instance_ids.dtype != torch.int32 or tuple(instance_ids.shape) != (n, k):
        raise ValueError(f"instance_ids must be a contiguous int32 tensor of shape [{n}, {k}]")
    if n == 0:
        return 0
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_ray_first_hits_instanced(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table), int(num_blas),
                                             _ptr(rays), n, k, _ptr(hits), _ptr(instance_ids), _ptr(counters), _ptr(status),
                                             _stream_ptr(stream)), "rt_ray_first_hits_instanced")
    return n


def ray_first_status(status) -> int:
    """The RT_RAY_FIRST_* flags RayFirstHits ORed into `status` (copies the word back: waits for the work queued before it)."""
    return _status_word(status)


class HitFilter:
    """rt_hit_filter: which of the triangles a ray crosses count (include/rt_abi.h, hit-filter block).  flags:
    RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT (front: the side the counter-clockwise normal points to).  prim_masks: optional
    contiguous device int32 / uint32 tensor [num_primitives], one mask per primitive_id (ids beyond it: all ones).  per_ray:
    optional contiguous device buffer of 8-byte RAY_FILTER records (mask, skip_id), e.g. int32 [N, 2], one per ray of the batch
    it is used with; without it every ray has `ray_mask` and skips nothing.  A candidate is kept iff it is not culled, its
    primitive_id is not the ray's skip_id (MISS: none) and prim mask & ray mask != 0.  The object keeps its tensors alive."""

    def __init__(self, flags: int = 0, ray_mask: int = 0xFFFFFFFF, prim_masks=None, per_ray=None):
        for name, t, rec in (("prim_masks", prim_masks, 4), ("per_ray", per_ray, 8)):
            if t is not None and (not t.is_contiguous() or _nbytes(t) % rec):
                raise ValueError(f"{name} must be a contiguous device buffer of {rec}-byte records")
        self.flags, self.ray_mask, self.prim_masks, self.per_ray = int(flags), int(ray_mask) & 0xFFFFFFFF, prim_masks, per_ray

    def _struct(self, num_rays: int) -> _HitFilter:
        if self.per_ray is not None and _nbytes(self.per_ray) < 8 * num_rays:
            raise ValueError(f"per_ray must hold {num_rays} 8-byte records")
        num_prims = 0 if self.prim_masks is None else _nbytes(self.prim_masks) // 4
        return _HitFilter(self.flags, self.ray_mask, num_prims, 0, _ptr(self.prim_masks) or None, _ptr(self.per_ray) or None)


def _filter_ref(filter, num_rays: int):
    """the `filter` argument of a filtered entry point: NULL for None (the call forwards to the unfiltered entry point)"""
    return None if filter is None else ctypes.byref(filter._struct(num_rays))


def IntersectRaysFiltered(triangles, nodes, root: int, count: int, rays, hits, filter, *, any_hit: bool = False,
                          num_primitives: int = 0, counters=None, stream=None) -> None:
    """rt_intersect_rays_filtered: IntersectRays over the candidates `filter` (a HitFilter, or None for all) keeps.  The filter
    acts inside the traversal: a rejected triangle neither shrinks the ray's window nor ends an any-hit ray."""
    if not rays.is_contiguous() or not hits.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits a contiguous device buffer")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n:
        raise ValueError(f"hits must hold {n} 16-byte records")
    if n == 0:
        return
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_intersect_rays_filtered(ctypes.byref(a), _ptr(rays), _ptr(hits), n, kAnyHit if any_hit else kClosestHit,
                                            int(num_primitives), _filter_ref(filter, n), _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_filtered")


def RayHitsCountFiltered(triangles, nodes, root: int, count: int, rays, filter, offsets, *, scratch=None, counters=None,
                         status=None, stream=None) -> int:
    """rt_ray_hits_count_filtered: RayHitsCount over the candidates `filter` (a HitFilter, or None for all) keeps.  The counters
    are the unfiltered call's: the filter acts after the leaf test."""
    n = _ray_batch(rays)
    return _csr_count(lib().rt_ray_hits_count_filtered, RayHitsScratchBytes, (triangles, nodes, root, count), rays, n,
                      (_filter_ref(filter, n),), offsets, scratch=scratch, counters=counters, status=status, stream=stream)


def RayHitsCollectFiltered(triangles, nodes, root: int, count: int, rays, filter, offsets, hits, *, counts=None, counters=None,
                           status=None, stream=None) -> int:
    """rt_ray_hits_collect_filtered: RayHitsCollect over the candidates `filter` keeps (the same filter as the count call)."""
    n = _ray_batch(rays)
    return _csr_collect(lib().rt_ray_hits_collect_filtered, (triangles, nodes, root, count), rays, n, (_filter_ref(filter, n),),
                        offsets, hits, "hits", counts=counts, counters=counters, status=status, stream=stream)


def RayFirstHitsFiltered(triangles, nodes, root: int, count: int, rays, k: int, filter, out, *, counters=None, status=None,
                         stream=None) -> int:
    """rt_ray_first_hits_filtered: RayFirstHits over the candidates `filter` (a HitFilter, or None for all) keeps: the k nearest
    KEPT crossings, in order; the bound only falls to the t of a kept record."""
    k = int(k)
    if not 1 <= k <= RT_RAY_FIRST_MAX_K:
        raise ValueError(f"k must be in 1 .. {RT_RAY_FIRST_MAX_K}")
    n = _ray_batch(rays)
    if not out.is_contiguous() or out.dtype != _torch().float32 or tuple(out.shape) != (n, k, 4):
        raise ValueError(f"out must be a contiguous float32 tensor of shape [{n}, {k}, 4]")
    if n == 0:
        return 0
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_ray_first_hits_filtered(ctypes.byref(a), _ptr(rays), n, k, _filter_ref(filter, n), _ptr(out), _ptr(counters),
                                            _ptr(status), _stream_ptr(stream)), "rt_ray_first_hits_filtered")
    return n


class InstanceHitFilter:
    """rt_instance_hit_filter: the filter of the instanced ray query (include/rt_abi.h, instance-filter block).  flags:
    RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT, decided on the WORLD-space facing (a mirrored instance swaps them).
    per_instance: optional contiguous device buffer of 8-byte INSTANCE_FILTER records (mask, flags), e.g. int32 [K, 2], indexed
    by the instance index; instances beyond it have an all-ones mask and no flags.  per_ray: optional contiguous device buffer
    of 16-byte INSTANCE_RAY_FILTER records (mask, skip_instance, skip_id, pad), e.g. int32 [N, 4], one per ray of the batch it
    is used with; without it every ray has `ray_mask` and skips nothing.  An instance is entered only if its mask & the ray's
    mask != 0; a candidate is kept iff it is not culled and is not primitive skip_id of instance skip_instance.  The object
    keeps its tensors alive."""

    def __init__(self, flags: int = 0, ray_mask: int = 0xFFFFFFFF, per_instance=None, per_ray=None):
        for name, t, rec in (("per_instance", per_instance, 8), ("per_ray", per_ray, 16)):
            if t is not None and (not t.is_contiguous() or _nbytes(t) % rec):
                raise ValueError(f"{name} must be a contiguous device buffer of {rec}-byte records")
        self.flags, self.ray_mask = int(flags), int(ray_mask) & 0xFFFFFFFF
        self.per_instance, self.per_ray = per_instance, per_ray

    def _struct(self, num_rays: int) -> _InstanceHitFilter:
        if self.per_ray is not None and _nbytes(self.per_ray) < 16 * num_rays:
            raise ValueError(f"per_ray must hold {num_rays} 16-byte records")
        num = 0 if self.per_instance is None else _nbytes(self.per_instance) // 8
        return _InstanceHitFilter(self.flags, self.ray_mask, num, 0, _ptr(self.per_instance) or None, _ptr(self.per_ray) or None)


def IntersectRaysInstancedFiltered(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                                   num_blas: int, rays, hits, instance_ids, filter, *, any_hit: bool = False,
                                   num_primitives: int = 0, counters=None, stream=None) -> None:
    """rt_intersect_rays_instanced_filtered: IntersectRaysInstanced over the instances and candidates `filter` (an
    InstanceHitFilter, or None for all) keeps.  A masked-out instance is never entered (no BLAS descent); a rejected triangle
    neither shrinks the ray's window nor ends an any-hit ray."""
    if not rays.is_contiguous() or not hits.is_contiguous() or not instance_ids.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits / instance_ids contiguous buffers")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n or _nbytes(instance_ids) < 4 * n:
        raise ValueError(f"hits must hold {n} 16-byte records and instance_ids {n} words")
    if filter is not None and not isinstance(filter, InstanceHitFilter):
        raise ValueError("filter must be an InstanceHitFilter or None")
    flt = _filter_ref(filter, n)
    if n == 0:
        return
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_intersect_rays_instanced_filtered(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                      int(num_blas), _ptr(rays), _ptr(hits), _ptr(instance_ids), n,
                                                      kAnyHit if any_hit else kClosestHit, int(num_primitives), flt,
                                                      _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_instanced_filtered")


def _instance_filter_ref(filter, num_rays: int):
    if filter is not None and not isinstance(filter, InstanceHitFilter):
        raise ValueError("filter must be an InstanceHitFilter or None")
    return _filter_ref(filter, num_rays)


def RayHitsCountInstancedFiltered(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                                  num_blas: int, rays, filter, offsets, *, scratch=None, counters=None, status=None,
                                  stream=None) -> int:
    """rt_ray_hits_count_instanced_filtered: RayHitsCountInstanced over the instances and candidates `filter` (an
    InstanceHitFilter, or None for all) keeps (include/rt_abi.h, instanced set-filter block).  A masked-out instance is never
    entered (no record load, no BLAS descent); a rejected triangle is not a crossing.  Everything else is the sibling's."""
    n = _ray_batch(rays)
    if not offsets.is_contiguous() or _nbytes(offsets) < 8 * (n + 1):
        raise ValueError(f"offsets must be a contiguous device buffer of {n + 1} 64-bit words")
    flt = _instance_filter_ref(filter, n)
    if n == 0:
        return 0
    if scratch is None:
        scratch = device_bytes(RayHitsScratchBytes(n), rays.device)
    elif _nbytes(scratch) < RayHitsScratchBytes(n):
        raise ValueError(f"scratch must hold RayHitsScratchBytes({n}) bytes")
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_ray_hits_count_instanced_filtered(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                      int(num_blas), _ptr(rays), n, flt, _ptr(offsets), _ptr(scratch),
                                                      _ptr(counters), _ptr(status), _stream_ptr(stream)),
           "rt_ray_hits_count_instanced_filtered")
    return n


def RayHitsCollectInstancedFiltered(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                                    num_blas: int, rays, filter, offsets, hits, instance_ids, *, counts=None, counters=None,
                                    status=None, stream=None) -> int:
    """rt_ray_hits_collect_instanced_filtered: RayHitsCollectInstanced over the instances and candidates `filter` (an
    InstanceHitFilter, or None for all) keeps: the rows RayHitsCountInstancedFiltered counted under the same filter."""
    n = _ray_batch(rays)
    if not offsets.is_contiguous() or not hits.is_contiguous() or not instance_ids.is_contiguous() or \
            _nbytes(offsets) < 8 * (n + 1):
        raise ValueError(f"offsets must be a contiguous device buffer of {n + 1} 64-bit words, hits / instance_ids contiguous "
                         "device buffers")
    if counts is not None and (not counts.is_contiguous() or _nbytes(counts) < 4 * n):
        raise ValueError(f"counts must hold {n} words")
    flt = _instance_filter_ref(filter, n)
    if n == 0:
        return 0
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_ray_hits_collect_instanced_filtered(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                        int(num_blas), _ptr(rays), n, flt, _ptr(offsets), _ptr(hits),
                                                        _ptr(instance_ids), _ptr(counts), _ptr(counters), _ptr(status),
                                                        _stream_ptr(stream)), "rt_ray_hits_collect_instanced_filtered")
    return n


def RayHitsInstancedFiltered(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                             num_blas: int, rays, filter, *, sort: bool = False, counters=None, status=None, stream=None):
    """RayHitsInstanced over the instances and candidates `filter` (an InstanceHitFilter, or None for all) keeps:
    RayHitsCountInstancedFiltered, the total READ BACK TO THE HOST (one synchronisation of `stream`), then
    RayHitsCollectInstancedFiltered.  Returns (offsets, hits, instance_ids) as RayHitsInstanced does; sort=True orders every
    row by ascending (t, instance, primitive_id)."""
    torch = _torch()
    n = _ray_batch(rays)
    tree = (tlas_triangles, tlas_nodes, root, count, records, num_instances, blas_table, num_blas)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=rays.device)
    RayHitsCountInstancedFiltered(*tree, rays, filter, offsets, counters=counters, status=status, stream=stream)
    with _on_stream(stream):
        if n == 0:
            offsets.zero_()
        total = int(offsets[n].item())
        hits = torch.empty((max(total, 1), 4), dtype=torch.float32, device=rays.device)[:total]
        ids = torch.empty(max(total, 1), dtype=torch.int32, device=rays.device)[:total]
        RayHitsCollectInstancedFiltered(*tree, rays, filter, offsets, hits, ids, counters=counters, status=status, stream=stream)
        if sort and total > 1:
            hits, ids = _sort_instanced_rows(offsets, hits, ids, n, total)
    return offsets, hits, ids


def RayFirstHitsInstancedFiltered(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                                  num_blas: int, rays, k: int, filter, hits, instance_ids, *, counters=None, status=None,
                                  stream=None) -> int:
    """rt_ray_first_hits_instanced_filtered: RayFirstHitsInstanced over the instances and candidates `filter` (an
    InstanceHitFilter, or None for all) keeps: the k nearest KEPT crossings.  A rejected crossing never enters the list and
    never shrinks the bound (include/rt_abi.h, instanced set-filter block)."""
    torch = _torch()
    k = int(k)
    if not 1 <= k <= RT_RAY_FIRST_MAX_K:
        raise ValueError(f"k must be in 1 .. {RT_RAY_FIRST_MAX_K}")
    n = _ray_batch(rays)
    if not hits.is_contiguous() or hits.dtype != torch.float32 or tuple(hits.shape) != (n, k, 4):
        raise ValueError(f"hits must be a contiguous float32 tensor of shape [{n}, {k}, 4]")
    if not instance_ids.is_contiguous() or instance_ids.dtype != torch.int32 or tuple(instance_ids.shape) != (n, k):
        raise ValueError(f"instance_ids must be a contiguous int32 tensor of shape [{n}, {k}]")
    flt = _instance_filter_ref(filter, n)
    if n == 0:
        return 0
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_ray_first_hits_instanced_filtered(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                      int(num_blas), _ptr(rays), n, k, flt, _ptr(hits), _ptr(instance_ids),
                                                      _ptr(counters), _ptr(status), _stream_ptr(stream)),
           "rt_ray_first_hits_instanced_filtered")
    return n


def TriOverlapsScratchBytes(num_queries: int) -> int:
    """rt_tri_overlaps_scratch_bytes: device bytes of TriOverlapsCount's scratch (8 bytes per 256 queries, 256-byte aligned)."""
    return int(lib().rt_tri_overlaps_scratch_bytes(int(num_queries)))


def _tri_batch(queries) -> int:
    if not queries.is_contiguous() or _nbytes(queries) % 36:
        raise ValueError("queries must be a contiguous device buffer of 36-byte TRIANGLE records")
    return _nbytes(queries) // 36


def TriOverlapsCount(triangles, nodes, root: int, count: int, queries, offsets, *, self_pairs: bool = False, scratch=None,
                     counters=None, status=None, stream=None) -> int:
    """rt_tri_overlaps_count: offsets[0 .. N] (a contiguous device int64 tensor of >= N + 1 words) = the exclusive prefix sum of
    the number of triangles each query triangle of `queries` (36-byte TRIANGLE records, e.g. float32 [N, 9]) cuts; offsets[N]
    is the total.  Any tree Trace() takes.  self_pairs (kTriSelf): `queries` are the triangles the tree was built over, query i
    is triangle i, and row i holds only j > i without a corner shared with i -- every intersecting pair once.  scratch:
    >= TriOverlapsScratchBytes(N) bytes, 256-byte aligned (device_bytes; taken from torch's allocator when None).  counters:
    optional int64[4] ([0] box tests, [1] leaf records visited).  status: optional device uint32 the call ORs RT_TRI_* flags
    into (see tri_overlap_status).  Asynchronous on `stream`, nothing is read back.  Returns N."""
    return _csr_count(lib().rt_tri_overlaps_count, TriOverlapsScratchBytes, (triangles, nodes, root, count), queries,
                      _tri_batch(queries), (kTriSelf if self_pairs else 0,), offsets, scratch=scratch, counters=counters,
                      status=status, stream=stream)


def TriOverlapsCollect(triangles, nodes, root: int, count: int, queries, offsets, ids, *, self_pairs: bool = False, counts=None,
                       counters=None, status=None, stream=None) -> int:
    """rt_tri_overlaps_collect: query i writes the ids of its first offsets[i+1] - offsets[i] matches at ids[offsets[i]:]
    (`ids`: a contiguous device int32 / uint32 tensor the offsets stay inside -- the caller's contract; `offsets`: int64
    [N + 1] from TriOverlapsCount, or i * K for a fixed K per query).  counts: optional device int32 [N], each query's true
    match count.  A query with more matches than room sets RT_TRI_TRUNCATED in `status`.  Ids come in traversal order
    (unspecified but deterministic); on non-split trees each matching triangle appears exactly once.  Asynchronous on
    `stream`.  Returns N."""
    return _csr_collect(lib().rt_tri_overlaps_collect, (triangles, nodes, root, count), queries, _tri_batch(queries),
                        (kTriSelf if self_pairs else 0,), offsets, ids, "ids", counts=counts, counters=counters, status=status,
                        stream=stream)


def tri_overlap_status(status) -> int:
    """The RT_TRI_* flags TriOverlapsCount / TriOverlapsCollect ORed into `status` (copies the word back: waits for the work
    queued before it)."""
    return _status_word(status)


def TriOverlaps(triangles, nodes, root: int, count: int, queries, *, self_pairs: bool = False, counters=None, status=None,
                stream=None):
    """Everything each query triangle cuts, as CSR: TriOverlapsCount, then the total offsets[N] is READ BACK TO THE HOST -- one
    synchronisation of `stream` per call, the only one -- to allocate the id array, then TriOverlapsCollect.  Returns
    (offsets, ids): torch int64 [N + 1] and int32 [total] device tensors; query i owns ids[offsets[i]:offsets[i+1]].  A
    caller who cannot afford the synchronisation (a captured graph, a fixed budget per query) uses TriOverlapsCount /
    TriOverlapsCollect directly.  With `counters`, the tests of both passes are added (twice one traversal)."""
    torch = _torch()
    n = _tri_batch(queries)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=queries.device)
    TriOverlapsCount(triangles, nodes, root, count, queries, offsets, self_pairs=self_pairs, counters=counters, status=status,
                     stream=stream)
    with _on_stream(stream):
        total = int(offsets[n].item())
    ids = torch.empty(max(total, 1), dtype=torch.int32, device=queries.device)[:total]
    TriOverlapsCollect(triangles, nodes, root, count, queries, offsets, ids, self_pairs=self_pairs, counters=counters,
                       status=status, stream=stream)
    return offsets, ids


def KNearest(triangles, nodes, root: int, count: int, queries, k: int, out, *, counters=None, status=None, stream=None) -> int:
    """rt_k_nearest: for each POINT_QUERY record of `queries` (a contiguous device tensor of 16-byte records (p, dist2_max),
    e.g. float32 [N, 4]) a row of k KNN_HIT records (dist2, primitive_id) in `out` (>= 8 k N bytes, e.g. float32 [N, k, 2];
    view it as int32 for primitive_id): the k nearest triangles within dist2_max in ascending (dist2, primitive_id) order,
    padded with {+inf, MISS}.  1 <= k <= RT_KNN_MAX_K.  Any tree Trace() takes.  counters: optional int64[4] device tensor
    ([0] box tests, [1] triangle tests).  status: optional device uint32 the call ORs RT_KNN_STACK_OVERFLOW into (the caller
    clears it; see knn_status).  Asynchronous on `stream`, nothing is allocated or read back.  Returns N."""
    k = int(k)
    if not 1 <= k <= RT_KNN_MAX_K:
        raise ValueError(f"k must be in 1 .. {RT_KNN_MAX_K}")
    if not queries.is_contiguous() or not out.is_contiguous() or _nbytes(queries) % 16:
        raise ValueError("queries must be a contiguous device buffer of 16-byte records, out a contiguous device buffer")
    n = _nbytes(queries) // 16
    if _nbytes(out) < 8 * k * n:
        raise ValueError(f"out must hold {n} rows of {k} 8-byte records")
    if n == 0:
        return 0
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_k_nearest(ctypes.byref(a), _ptr(queries), n, k, _ptr(out), _ptr(counters), _ptr(status),
                              _stream_ptr(stream)), "rt_k_nearest")
    return n


def knn_status(status) -> int:
    """The RT_KNN_* flags KNearest ORed into `status` (copies the word back: waits for the work queued before it)."""
    return _status_word(status)


def _sdf_call(entry, triangles, nodes, root: int, count: int, queries, result, record: int, votes, dirs, counters, status,
              stream) -> int:
    votes = int(votes)
    if votes not in (1, RT_SDF_MAX_VOTES):
        raise ValueError(f"votes must be 1 or {RT_SDF_MAX_VOTES}")
    if not queries.is_contiguous() or not result.is_contiguous() or _nbytes(queries) % 16:
        raise ValueError("queries must be a contiguous device buffer of 16-byte records, the output a contiguous device buffer")
    n = _nbytes(queries) // 16
    if _nbytes(result) < record * n:
        raise ValueError(f"the output must hold {n} records of {record} byte(s)")
    d = None
    if dirs is not None:
        host = np.ascontiguousarray(dirs, np.float32).reshape(-1)
        if host.size < 3 * votes:
            raise ValueError(f"dirs must hold {votes} directions of 3 floats")
        d = (ctypes.c_float * (3 * votes))(*host[:3 * votes].tolist())
    if n == 0:
        return 0
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(entry(ctypes.byref(a), _ptr(queries), n, votes, d, _ptr(result), _ptr(counters), _ptr(status), _stream_ptr(stream)),
           entry.__name__)
    return n


def SignedDistance(triangles, nodes, root: int, count: int, queries, out, *, votes: int = 3, dirs=None, counters=None,
                   status=None, stream=None) -> int:
    """rt_signed_distance: for each POINT_QUERY record of `queries` (a contiguous device tensor of 16-byte records
    (p, dist2_max), e.g. float32 [N, 4]) one SDF_HIT record (sdist, primitive_id) in `out` (>= 8 N bytes, e.g. float32 [N, 2];
    view it as int32 for primitive_id).  (sdist**2, primitive_id) is ClosestPoints's nearest triangle within dist2_max
    (|sdist| = sqrt(dist2); {inf, MISS} beyond the radius), negative when the point is inside: `votes` rays (1 or 3; the third
    only where the first two disagree) along `dirs` (host float32 [votes, 3]; None = SDF_DEFAULT_DIRS) are counted as by
    RayHitsCount and the majority of odd counts decides.  The sign means something only for a closed mesh on a tree without
    spatial splits.  counters: optional int64[4] ([0] box tests, [1] leaf records, over every traversal that ran).  status:
    optional device uint32 the call ORs RT_SDF_STACK_OVERFLOW into (see sdf_status).  Asynchronous on `stream`, nothing is
    allocated or read back.  Returns N."""
    return _sdf_call(lib().rt_signed_distance, triangles, nodes, root, count, queries, out, 8, votes, dirs, counters, status,
                     stream)


def Occupancy(triangles, nodes, root: int, count: int, queries, inside, *, votes: int = 3, dirs=None, counters=None,
              status=None, stream=None) -> int:
    """rt_occupancy: the inside / outside bit of SignedDistance alone: inside[i] = 1 or 0 for queries[i] (`inside`: a contiguous
    device buffer of >= N bytes, e.g. uint8 [N]).  dist2_max only decides whether the query is traced (NaN or negative: not
    traced, outside).  Other arguments as for SignedDistance.  Returns N."""
    return _sdf_call(lib().rt_occupancy, triangles, nodes, root, count, queries, inside, 1, votes, dirs, counters, status, stream)


def sdf_status(status) -> int:
    """The RT_SDF_* flags SignedDistance / Occupancy ORed into `status` (copies the word back: waits for the work queued before
    it)."""
    return _status_word(status)


def GridPointCount(dims, bricks: bool = False) -> int:
    """Number of records GenerateGridPoints writes: dims[0]*dims[1]*dims[2] row-major, ceil(dims/4) bricks of 64 per axis
    product in the brick layout (0 when a dimension is 0)."""
    dx, dy, dz = (int(v) for v in dims)
    if min(dx, dy, dz) <= 0:
        return 0
    return ((dx + 3) // 4) * ((dy + 3) // 4) * ((dz + 3) // 4) * 64 if bricks else dx * dy * dz


def GenerateGridPoints(origin, spacing, dims, queries, *, dist2_max: float = float("inf"), bricks: bool = False,
                       stream=None) -> int:
    """rt_generate_grid_points: the POINT_QUERY records of a lattice, point (i, j, k) = origin + (i, j, k) * spacing in float32
    (one multiply, one add), every one with `dist2_max`, into `queries` (a contiguous device tensor of at least
    GridPointCount(dims, bricks) * 16 bytes, e.g. float32 [N, 4]).  Row-major: index (k*dims[1] + j)*dims[0] + i.  Bricks:
    4x4x4 bricks in row-major brick order, 64 records each, lane = 3-D Morton code of the offset in the brick (one wave of
    SignedDistance / Occupancy gets one brick); off-lattice lanes of edge bricks get {0, 0, 0, -1}, a query that is not traced.
    origin, spacing, dims: host triples.  Asynchronous on `stream`.  Returns the number of records written."""
    n = GridPointCount(dims, bricks)
    if not queries.is_contiguous() or _nbytes(queries) < 16 * n:
        raise ValueError(f"queries must be a contiguous device buffer of >= {16 * n} bytes")
    if n == 0:
        return 0
    o = (ctypes.c_float * 3)(*[float(v) for v in origin])
    sp = (ctypes.c_float * 3)(*[float(v) for v in spacing])
    d = (ctypes.c_uint32 * 3)(*[int(v) for v in dims])
    _check(lib().rt_generate_grid_points(o, sp, d, float(dist2_max), kGridBricks if bricks else kGridRowMajor,
                                         _ptr(queries), _stream_ptr(stream)), "rt_generate_grid_points")
    return n


def RaySortScratchBytes(num_rays: int) -> int:
    """rt_ray_sort_scratch_bytes: device bytes of SortRays's scratch (12 bytes per ray + the sort's tables + 256)."""
    return int(lib().rt_ray_sort_scratch_bytes(num_rays))


def ray_sort_layout(num_rays: int) -> _RaySortLayout:
    out = _RaySortLayout()
    _check(lib().rt_ray_sort_layout_get(num_rays, ctypes.byref(out)), "rt_ray_sort_layout_get")
    return out


def SortRays(nodes, root: int, count: int, rays, order, scratch, stream=None) -> int:
    """rt_sort_rays: a coherence order of `rays` (a contiguous device tensor of 32-byte RAY records) into `order` (a device
    tensor of >= N uint32 / int32 words): ray indices by ascending key -- origin cell in the box of the tree's root run
    (`nodes`, root / count as for IntersectRays; a TLAS will do), then direction cell; dead rays (the ones IntersectRays does
    not trace) last.  `scratch`: >= RaySortScratchBytes(N) bytes, 256-byte aligned (device_bytes).  One sort serves any
    number of IntersectRaysIndexed calls on the same rays.  Asynchronous on `stream`.  Returns N."""
    if not rays.is_contiguous() or not order.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, order a contiguous device buffer")
    n = _nbytes(rays) // 32
    if _nbytes(order) < 4 * n or _nbytes(scratch) < RaySortScratchBytes(n):
        raise ValueError(f"order must hold {n} words and scratch RaySortScratchBytes({n}) bytes")
    if n == 0:
        return 0
    a = _Accel(0, _ptr(nodes), root, count)
    _check(lib().rt_sort_rays(ctypes.byref(a), _ptr(rays), n, _ptr(order), _ptr(scratch), _stream_ptr(stream)), "rt_sort_rays")
    return n


def ray_sort_live(scratch, num_rays: int) -> int:
    """The number of live rays of the last SortRays on `scratch`: order[:live] are the rays a query traces (copies the word
    back: waits for the work queued before it on the current stream)."""
    return int(to_host(scratch, np.uint32, 1, ray_sort_layout(num_rays).num_live)[0])


def IntersectRaysIndexed(triangles, nodes, root: int, count: int, rays, order, hits, *, num_indices: Optional[int] = None,
                         any_hit: bool = False, num_primitives: int = 0, counters=None, stream=None) -> None:
    """rt_intersect_rays_indexed: IntersectRays through an index list.  Launch position j (64 consecutive j per wave) traces
    rays[order[j]] and writes hits[order[j]]; an index >= N (0xFFFFFFFF, say) is skipped and unlisted records are not
    written.  `order`: a contiguous device tensor of uint32 / int32 words -- SortRays's output, or any list of the rays still
    alive; num_indices: how many of its words to use (default: all).  Each written record equals IntersectRays's bit for
    bit.  counters[2:4] (wave steps) measure the order's coherence.  Asynchronous on `stream`."""
    if not rays.is_contiguous() or not hits.is_contiguous() or not order.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits / order contiguous device buffers")
    n = _nbytes(rays) // 32
    k = _nbytes(order) // 4 if num_indices is None else int(num_indices)
    if _nbytes(hits) < 16 * n or _nbytes(order) < 4 * k:
        raise ValueError(f"hits must hold {n} 16-byte records and order {k} words")
    if k == 0:
        return
    a = _Accel(_ptr(triangles), _ptr(nodes), root, count)
    _check(lib().rt_intersect_rays_indexed(ctypes.byref(a), _ptr(rays), n, _ptr(order), k, _ptr(hits),
                                           kAnyHit if any_hit else kClosestHit, int(num_primitives), _ptr(counters),
                                           _stream_ptr(stream)), "rt_intersect_rays_indexed")


def _indexed_batch(rays, order, num_indices, hits, instance_ids=None, times=None):
    """(N, K) of an indexed call after the buffer checks its four forms share: N rays, K words of `order` to use"""
    bufs = [rays, order, hits] + [t for t in (instance_ids, times) if t is not None]
    if any(not t.is_contiguous() for t in bufs) or _nbytes(rays) % 32:
        raise ValueError("rays must be a contiguous device buffer of 32-byte records, order / hits / instance_ids / times "
                         "contiguous device buffers")
    n = _nbytes(rays) // 32
    k = _nbytes(order) // 4 if num_indices is None else int(num_indices)
    if _nbytes(hits) < 16 * n or _nbytes(order) < 4 * k:
        raise ValueError(f"hits must hold {n} 16-byte records and order {k} words")
    if instance_ids is not None and _nbytes(instance_ids) < 4 * n:
        raise ValueError(f"instance_ids must hold {n} words")
    if times is not None and _nbytes(times) < 4 * n:
        raise ValueError(f"times must hold {n} floats")
    return n, k


def IntersectRaysInstancedIndexed(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int, blas_table,
                                  num_blas: int, rays, order, hits, instance_ids, *, num_indices: Optional[int] = None,
                                  filter=None, any_hit: bool = False, num_primitives: int = 0, counters=None,
                                  stream=None) -> None:
    """rt_intersect_rays_instanced_indexed: IntersectRaysInstanced (filter=None) or IntersectRaysInstancedFiltered (an
    InstanceHitFilter) through an index list, with IntersectRaysIndexed's contract: launch position j (64 consecutive j per
    wave) traces rays[order[j]] and writes hits[order[j]] and instance_ids[order[j]]; an index >= N is skipped and unlisted
    records are not written.  The filter's per_ray records go by the ray's index too.  `order`: SortRays's output over the
    TLAS (nodes, root, count), or any list of the rays still alive; num_indices: how many of its words to use (default: all).
    Each written record equals the direct call's bit for bit.  Asynchronous on `stream`."""
    n, k = _indexed_batch(rays, order, num_indices, hits, instance_ids)
    flt = _instance_filter_ref(filter, n)
    if n == 0 or k == 0:
        return
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_intersect_rays_instanced_indexed(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                     int(num_blas), _ptr(rays), n, _ptr(order), k, _ptr(hits),
                                                     _ptr(instance_ids), kAnyHit if any_hit else kClosestHit,
                                                     int(num_primitives), flt, _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_instanced_indexed")


def IntersectRaysInstancedMotionIndexed(tlas_pose0, tlas_pose1, root: int, count: int, records, num_instances: int, blas_table,
                                        num_blas: int, rays, times, order, hits, instance_ids, *,
                                        num_indices: Optional[int] = None, any_hit: bool = False, counters=None,
                                        stream=None) -> None:
    """rt_intersect_rays_instanced_motion_indexed: IntersectRaysInstancedMotion through an index list (order / num_indices as
    for IntersectRaysInstancedIndexed); `times` goes by the ray's index like rays, hits and instance_ids."""
    n, k = _indexed_batch(rays, order, num_indices, hits, instance_ids, times)
    if num_instances and (not records.is_contiguous() or _nbytes(records) < 128 * int(num_instances)):
        raise ValueError(f"records must be a contiguous device buffer of {int(num_instances)} 128-byte records")
    if n == 0 or k == 0:
        return
    a = _motion_accel(tlas_pose0, tlas_pose1, root, count)
    _check(lib().rt_intersect_rays_instanced_motion_indexed(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                            int(num_blas), _ptr(rays), _ptr(times), n, _ptr(order), k,
                                                            _ptr(hits), _ptr(instance_ids),
                                                            kAnyHit if any_hit else kClosestHit, _ptr(counters),
                                                            _stream_ptr(stream)),
           "rt_intersect_rays_instanced_motion_indexed")


def IntersectRaysInstancedMixedIndexed(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int,
                                       blas_table, geom_table, num_blas: int, rays, order, hits, instance_ids, *,
                                       num_indices: Optional[int] = None, any_hit: bool = False, counters=None,
                                       stream=None) -> None:
    """rt_intersect_rays_instanced_mixed_indexed: IntersectRaysInstancedMixed through an index list (order / num_indices as for
    IntersectRaysInstancedIndexed).  geom_table=None: IntersectRaysInstancedIndexed with num_primitives = 0 and no filter."""
    n, k = _indexed_batch(rays, order, num_indices, hits, instance_ids)
    if geom_table is not None and (not geom_table.is_contiguous() or _nbytes(geom_table) < 16 * int(num_blas)):
        raise ValueError(f"geom_table must be a contiguous device buffer of {int(num_blas)} 16-byte records")
    if n == 0 or k == 0:
        return
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_intersect_rays_instanced_mixed_indexed(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                           _ptr(geom_table), int(num_blas), _ptr(rays), n, _ptr(order), k,
                                                           _ptr(hits), _ptr(instance_ids),
                                                           kAnyHit if any_hit else kClosestHit, _ptr(counters),
                                                           _stream_ptr(stream)),
           "rt_intersect_rays_instanced_mixed_indexed")


def IntersectRaysInstancedMixedCapsules(tlas_triangles, tlas_nodes, root: int, count: int, records, num_instances: int,
                                        blas_table, geom_table, num_blas: int, rays, hits, instance_ids, order=None, *,
                                        num_indices: Optional[int] = None, any_hit: bool = False, counters=None,
                                        stream=None) -> None:
    """rt_intersect_rays_instanced_mixed_capsules: IntersectRaysInstancedMixed over a table that may also hold capsule BLASes
    (geometry_table's (capsules, n, RT_GEOM_CAPSULES) entries).  A hit in a capsule BLAS is IntersectRaysCapsules's record: t,
    the capsule index, u = 1 for the far root, v = the axial parameter.  order=None is the direct form; with `order` the call
    is IntersectRaysInstancedMixedIndexed's.  `geom_table` is required: the all-triangle shortcut stays with the two older
    calls, whose kernels these are not.  Asynchronous on `stream`."""
    if geom_table is None:
        raise ValueError("geom_table is required (IntersectRaysInstancedMixed takes None for an all-triangle table)")
    if order is not None:
        n, k = _indexed_batch(rays, order, num_indices, hits, instance_ids)
    else:
        if not rays.is_contiguous() or not hits.is_contiguous() or not instance_ids.is_contiguous() or _nbytes(rays) % 32:
            raise ValueError("rays must be a contiguous device buffer of 32-byte records, hits / instance_ids contiguous buffers")
        n, k = _nbytes(rays) // 32, 0
        if _nbytes(hits) < 16 * n or _nbytes(instance_ids) < 4 * n:
            raise ValueError(f"hits must hold {n} 16-byte records and instance_ids {n} words")
    if not geom_table.is_contiguous() or _nbytes(geom_table) < 16 * int(num_blas):
        raise ValueError(f"geom_table must be a contiguous device buffer of {int(num_blas)} 16-byte records")
    if n == 0 or (order is not None and k == 0):
        return
    a = _Accel(_ptr(tlas_triangles), _ptr(tlas_nodes), root, count)
    _check(lib().rt_intersect_rays_instanced_mixed_capsules(ctypes.byref(a), _ptr(records), int(num_instances), _ptr(blas_table),
                                                            _ptr(geom_table), int(num_blas), _ptr(rays), n, _ptr(order), k,
                                                            _ptr(hits), _ptr(instance_ids),
                                                            kAnyHit if any_hit else kClosestHit, _ptr(counters),
                                                            _stream_ptr(stream)),
           "rt_intersect_rays_instanced_mixed_capsules")


def IntersectRaysMotionIndexed(pose0, pose1, root: int, count: int, rays, times, order, hits, *,
                               num_indices: Optional[int] = None, any_hit: bool = False, counters=None, stream=None) -> None:
    """rt_intersect_rays_motion_indexed: IntersectRaysMotion through an index list (order / num_indices as for
    IntersectRaysIndexed); `times` goes by the ray's index like rays and hits."""
    n, k = _indexed_batch(rays, order, num_indices, hits, None, times)
    if n == 0 or k == 0:
        return
    a = _motion_accel(pose0, pose1, root, count)
    _check(lib().rt_intersect_rays_motion_indexed(ctypes.byref(a), _ptr(rays), _ptr(times), n, _ptr(order), k, _ptr(hits),
                                                  kAnyHit if any_hit else kClosestHit, _ptr(counters), _stream_ptr(stream)),
           "rt_intersect_rays_motion_indexed")


def GenerateShadowRays(rays, hits, num_triangles: int, light, shadow_rays, stream=None) -> int:
    """rt_generate_shadow_rays: for every RAY record of `rays` whose HIT record names a triangle (primitive_id <
    num_triangles), the ray from the hit point to `light` (tmin 0.001, tmax = the light's distance) at the same index of
    `shadow_rays`; a dead ray (tmax -1) for a miss.  IntersectRays(..., any_hit=True) on the result gives the shadow records
    ShadeFrame takes for kTextureLitShadows.  Returns the number of rays."""
    if not rays.is_contiguous() or not hits.is_contiguous() or not shadow_rays.is_contiguous() or _nbytes(rays) % 32:
        raise ValueError("rays / shadow_rays must be contiguous device buffers of 32-byte records, hits a contiguous device buffer")
    n = _nbytes(rays) // 32
    if _nbytes(hits) < 16 * n or _nbytes(shadow_rays) < 32 * n:
        raise ValueError(f"hits must hold {n} 16-byte records, shadow_rays {n} 32-byte records")
    _check(lib().rt_generate_shadow_rays(_ptr(rays), _ptr(hits), n, int(num_triangles),
                                         (ctypes.c_float * 3)(*[float(x) for x in light]), _ptr(shadow_rays),
                                         _stream_ptr(stream)), "rt_generate_shadow_rays")
    return n


def ShadeFrame(triangles_in, num_triangles: int, rays, hits, rgba8, dims, *, render_type: int = kDepth, spp: int = 1,
               tiled: bool = False, shadow_hits=None, attributes=None, materials=None, num_materials: int = 0,
               light=(0.0, 0.0, 0.0), textures: Optional[DeviceTextures] = None, stream=None) -> None:
    """rt_shade_frame: the frame Trace() renders, from stored records -- `rays` as GenerateCameraRays wrote them (same dims,
    spp and layout), `hits` from IntersectRays / IntersectRaysIndexed on them, `shadow_hits` (kTextureLitShadows only) from
    an any-hit query on GenerateShadowRays's rays.  `triangles_in`: the caller's 36-byte triangles on the device
    (BuildInput.triangles_in); no tree is needed.  kBoxtests / kTriangleTests are not available from records (RtError, -2).
    Byte-equal to Trace() on non-pair trees; asynchronous on `stream`."""
    w, h = int(dims[0]), int(dims[1])
    n = CameraRayCount(w, h, int(spp), tiled)
    if _nbytes(rays) < 32 * n or _nbytes(hits) < 16 * n or _nbytes(rgba8) < 4 * w * h:
        raise ValueError(f"rays / hits must hold {n} records, rgba8 {4 * w * h} bytes")
    if shadow_hits is not None and _nbytes(shadow_hits) < 16 * n:
        raise ValueError(f"shadow_hits must hold {n} 16-byte records")
    s = _Scene(_ptr(attributes), _ptr(materials), _ptr(textures.table) if textures is not None else 0, 0,
               (ctypes.c_float * 3)(*[float(x) for x in light]),
               int(num_triangles), num_materials, textures.count if textures is not None else 0)
    _check(lib().rt_shade_frame(ctypes.byref(s), _ptr(triangles_in), int(num_triangles), _ptr(rays), _ptr(hits),
                                _ptr(shadow_hits), w, h, int(spp), kRaysTiled if tiled else kRaysRowMajor, int(render_type),
                                _ptr(rgba8), _stream_ptr(stream)), "rt_shade_frame")


def shade_geometry_table(entries, device="cuda"):
    """The device table of instanced shading, parallel to accel_table's: one rt_shade_geometry per BLAS.  An entry is
    (triangles_in, attributes, num_triangles) or (triangles_in, attributes, num_triangles, material_base) -- the device
    buffers of the BLAS's caller triangles (36-byte records, BuildInput.triangles_in) and of its 72-byte ATTRIBUTES -- or
    None for a BLAS that is not shaded (a sphere BLAS of the mixed query): its hits shade as misses.  The caller keeps the
    buffers alive."""
    tab = np.zeros(len(entries), SHADE_GEOMETRY)
    for k, e in enumerate(entries):
        if e is None:
            continue
        tris, attrs, nt = e[0], e[1], int(e[2])
        base = int(e[3]) if len(e) > 3 else 0
        if not tris.is_contiguous() or not attrs.is_contiguous() or _nbytes(tris) < 36 * nt or _nbytes(attrs) < 72 * nt:
            raise ValueError(f"entry {k}: triangles / attributes must be contiguous device buffers of {nt} 36- / 72-byte records")
        tab[k] = (_ptr(tris), _ptr(attrs), nt, base, (0, 0))
    return to_device(tab, device)


def ShadeFrameInstanced(geometry, num_blas: int, instances, records, num_instances: int, rays, hits, instance_ids, rgba8, dims,
                        *, render_type: int = kDepth, spp: int = 1, tiled: bool = False, renormalize: bool = True,
                        instance_materials=None, shadow_instance_ids=None, materials=None, num_materials: int = 0,
                        light=(0.0, 0.0, 0.0), textures: Optional[DeviceTextures] = None, stream=None) -> None:
    """rt_shade_frame_instanced: ShadeFrame for the records of IntersectRaysInstanced (and its filtered / motion siblings) --
    `hits` and `instance_ids` as the query wrote them for `rays` (GenerateCameraRays, same dims, spp and layout), `instances`
    (INSTANCE) and `records` (PrepareInstances) of the pose to shade, `geometry` (shade_geometry_table, parallel to the BLAS
    table).  `shadow_instance_ids` (kTextureLitShadows only): the instance ids of an any-hit instanced query on
    GenerateShadowRays(rays, hits, MISS, ...)'s rays.  renormalize: re-unit the placed normals (RT_SHADE_RENORMALIZE; off, an
    identity instance gives ShadeFrame's bytes).  instance_materials: an optional device int32 per instance, >= 0 replaces the
    material id of every hit in that instance.  The frame is ShadeFrame's on the flattened scene, byte for byte.
    Asynchronous on `stream`."""
    w, h = int(dims[0]), int(dims[1])
    n = CameraRayCount(w, h, int(spp), tiled)
    ni, nb = int(num_instances), int(num_blas)
    if _nbytes(rays) < 32 * n or _nbytes(hits) < 16 * n or _nbytes(instance_ids) < 4 * n or _nbytes(rgba8) < 4 * w * h:
        raise ValueError(f"rays / hits / instance_ids must hold {n} records, rgba8 {4 * w * h} bytes")
    if shadow_instance_ids is not None and _nbytes(shadow_instance_ids) < 4 * n:
        raise ValueError(f"shadow_instance_ids must hold {n} words")
    if ni and (_nbytes(instances) < 64 * ni or _nbytes(records) < 64 * ni or _nbytes(geometry) < 32 * nb):
        raise ValueError(f"instances / records must hold {ni} 64-byte records, geometry {nb} 32-byte records")
    if instance_materials is not None and (instance_materials.element_size() != 4 or _nbytes(instance_materials) < 4 * ni):
        raise ValueError(f"instance_materials must hold {ni} int32 words")
    for name, t in (("rays", rays), ("hits", hits), ("instance_ids", instance_ids), ("rgba8", rgba8), ("geometry", geometry),
                    ("instances", instances), ("records", records), ("shadow_instance_ids", shadow_instance_ids),
                    ("instance_materials", instance_materials)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous device buffer")
    s = _Scene(0, _ptr(materials), _ptr(textures.table) if textures is not None else 0, 0,
               (ctypes.c_float * 3)(*[float(x) for x in light]), 0, num_materials, textures.count if textures is not None else 0)
    _check(lib().rt_shade_frame_instanced(ctypes.byref(s), _ptr(geometry), nb, _ptr(instances), _ptr(records), ni,
                                          _ptr(instance_materials), _ptr(rays), _ptr(hits), _ptr(instance_ids),
                                          _ptr(shadow_instance_ids), w, h, int(spp), kRaysTiled if tiled else kRaysRowMajor,
                                          int(render_type), RT_SHADE_RENORMALIZE if renormalize else 0, _ptr(rgba8),
                                          _stream_ptr(stream)), "rt_shade_frame_instanced")


def version() -> str:
    return lib().rt_version_string().decode()
