// rt_instance_filter.hpp -- the filter of rt_intersect_rays_instanced_filtered (rt_abi.h, instance-filter block; DESIGN
// section 21): the kernel-side image of rt_instance_hit_filter and the per-lane policy InstanceRayFilter that trace_instanced
// (rt_instance_traverse.hpp) asks at the TLAS leaf (enter), tells which instance it entered (set_instance) and hands, as `tri`,
// to intersect_tri (rt_traverse.hpp) at its one acceptance point.  Included by instances.hip, whose query kernel has a
// FILTERED arm.
// Device code, force-inlined; the one host function is instance_filter_params, the launch's conversion.
#pragma once

#include "rt_device.hpp"

namespace rt {

// rt_instance_hit_filter after the entry point's checks: num_filters = 0 when per_instance is null (an absent array is an
// empty one)
struct InstanceFilterParams {
    uint32_t flags, ray_mask, num_filters;
    const uint2* per_instance;    // rt_instance_filter = one uint2: (mask, flags)
    const uint4* per_ray;         // rt_instance_ray_filter = one uint4: (mask, skip_instance, skip_id, pad)
};

inline InstanceFilterParams instance_filter_params(const rt_instance_hit_filter& f)   // (host)
{
    InstanceFilterParams fp;
    fp.flags = f.flags;
    fp.ray_mask = f.ray_mask;
    fp.num_filters = f.per_instance ? f.num_instance_filters : 0u;   // an absent array: nothing is read, every instance mask is all ones
    fp.per_instance = reinterpret_cast<const uint2*>(f.per_instance);
    fp.per_ray = reinterpret_cast<const uint4*>(f.per_ray);
    return fp;
}

// The per-instance part of a lane's filter, the policy of intersect_tri inside the entered instance: the cull bits that act on
// the OBJECT-space determinant (the call's bits, swapped when the instance shows the world its other side, 0 under
// RT_INSTANCE_FILTER_CULL_DISABLE) and the primitive skipped in this instance (RT_MISS: none).
struct InstanceTriFilter {
    static constexpr bool active = true;
    uint32_t cull, skip;

    __device__ __forceinline__ bool keep(float a, uint32_t prim) const
    {
        // a NaN determinant is neither front nor back: both comparisons are false
        if ((cull & RT_FILTER_CULL_BACK) && a < 0.0f) return false;
        if ((cull & RT_FILTER_CULL_FRONT) && a > 0.0f) return false;
        return !(prim == skip && skip != (uint32_t)RT_MISS);
    }
};

// One lane's filter.  flags, num_filters and per_instance are wave-uniform (kernel arguments: SGPRs); mask, skip_instance and
// skip_id are the ray's own and live across the whole traversal; inst_flags and tri belong to the instance the lane is in.
struct InstanceRayFilter {
    static constexpr bool active = true;
    uint32_t flags, num_filters;
    const uint2* per_instance;
    uint32_t mask, skip_instance, skip_id;
    uint32_t inst_flags;
    InstanceTriFilter tri;

    // the instance rule: one 8-byte load when the instance has a record, none otherwise
    __device__ __forceinline__ bool enter(uint32_t id)
    {
        uint32_t im = 0xFFFFFFFFu;
        inst_flags = 0u;
        if (id < num_filters) {
            const uint2 q = per_instance[id];
            im = q.x;
            inst_flags = q.y;
        }
        return (im & mask) != 0u;
    }

    // instance `id` is entered; w0 .. w2: the rows of its world_to_object, already loaded.  det only when a cull bit is set
    // (flags is wave-uniform: the branch is the whole wave's).
    __device__ __forceinline__ void set_instance(uint32_t id, const float4& w0, const float4& w1, const float4& w2)
    {
        uint32_t cull = 0u;
        if (flags & (uint32_t)(RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT)) {
            // the header's order: cofactors along the first row, each a difference of two products, ((c0 - c1) + c2)
            const float det = (w0.x * (w1.y * w2.z - w1.z * w2.y) - w0.y * (w1.x * w2.z - w1.z * w2.x)) +
                              w0.z * (w1.x * w2.y - w1.y * w2.x);
            const bool flip = (det < 0.0f) != ((inst_flags & RT_INSTANCE_FILTER_FLIP_FACING) != 0u);   // a NaN det: not mirrored
            const uint32_t swapped = ((flags & RT_FILTER_CULL_BACK) ? (uint32_t)RT_FILTER_CULL_FRONT : 0u) |
                                     ((flags & RT_FILTER_CULL_FRONT) ? (uint32_t)RT_FILTER_CULL_BACK : 0u);
            cull = flip ? swapped : (flags & (uint32_t)(RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT));
            if (inst_flags & RT_INSTANCE_FILTER_CULL_DISABLE) cull = 0u;
        }
        tri.cull = cull;
        tri.skip = id == skip_instance ? skip_id : (uint32_t)RT_MISS;
    }
};

// ray i's filter: one 16-byte load at ray setup when the caller gave per-ray records (lanes past the batch read nothing)
__device__ __forceinline__ InstanceRayFilter instance_ray_filter(const InstanceFilterParams& fp, uint64_t i, bool in_range)
{
    InstanceRayFilter f;
    f.flags = fp.flags;
    f.num_filters = fp.num_filters;
    f.per_instance = fp.per_instance;
    f.mask = fp.ray_mask;
    f.skip_instance = (uint32_t)RT_MISS;
    f.skip_id = (uint32_t)RT_MISS;
    f.inst_flags = 0u;
    f.tri.cull = 0u;
    f.tri.skip = (uint32_t)RT_MISS;
    if (fp.per_ray && in_range) {
        const uint4 q = fp.per_ray[i];
        f.mask = q.x;
        f.skip_instance = q.y;
        f.skip_id = q.z;
    }
    return f;
}

}  // namespace rt
