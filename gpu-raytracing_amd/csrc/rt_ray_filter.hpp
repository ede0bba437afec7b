// rt_ray_filter.hpp -- the hit filter of the filtered ray queries (rt_abi.h, hit-filter block): the
// kernel-side image of rt_hit_filter and the per-lane policy RayFilter that intersect_tri / trace_ray (rt_traverse.hpp), the
// all-hit loop (ray_hits_query.hip) and the first-K loop (ray_first_query.hip) ask at their one acceptance point.  Included by
// ray_query.hip, ray_hits_query.hip and ray_first_query.hip, whose kernels have a FILTERED arm.
// Device code, force-inlined; the one host function is filter_params, the launches' conversion.
#pragma once

#include "rt_device.hpp"

namespace rt {

// rt_hit_filter after the entry point's checks: num_prims = 0 when prim_masks is null (an absent array is an empty one)
struct FilterParams {
    uint32_t flags, ray_mask, num_prims;
    const uint32_t* prim_masks;
    const uint2* per_ray;         // rt_ray_filter = one uint2: (mask, skip_id)
};

inline FilterParams filter_params(const rt_hit_filter& f)   // (host)
{
    FilterParams fp;
    fp.flags = f.flags;
    fp.ray_mask = f.ray_mask;
    fp.num_prims = f.prim_masks ? f.num_primitives : 0u;   // an absent array: nothing is read, every primitive mask is all ones
    fp.prim_masks = f.prim_masks;
    fp.per_ray = reinterpret_cast<const uint2*>(f.per_ray);
    return fp;
}

// One lane's filter.  keep() orders its tests by cost: facing (a is in registers), the skip compare, then the one 4-byte
// prim_masks load -- only for a candidate that survived everything else.
struct RayFilter {
    static constexpr bool active = true;
    uint32_t flags, mask, skip, num_prims;
    const uint32_t* prim_masks;

    __device__ __forceinline__ bool keep(float a, uint32_t prim) const
    {
        // a NaN determinant is neither front nor back: both comparisons are false
        if ((flags & RT_FILTER_CULL_BACK) && a < 0.0f) return false;
        if ((flags & RT_FILTER_CULL_FRONT) && a > 0.0f) return false;
        if (prim == skip && skip != (uint32_t)RT_MISS) return false;
        const uint32_t pm = prim < num_prims ? prim_masks[prim] : 0xFFFFFFFFu;
        return (pm & mask) != 0;
    }
};

// ray i's filter: one 8-byte load at ray setup when the caller gave per-ray records (lanes past the batch read nothing)
__device__ __forceinline__ RayFilter ray_filter(const FilterParams& fp, uint64_t i, bool in_range)
{
    RayFilter f;
    f.flags = fp.flags;
    f.mask = fp.ray_mask;
    f.skip = (uint32_t)RT_MISS;
    f.num_prims = fp.num_prims;
    f.prim_masks = fp.prim_masks;
    if (fp.per_ray && in_range) {
        const uint2 q = fp.per_ray[i];
        f.mask = q.x;
        f.skip = q.y;
    }
    return f;
}

}  // namespace rt
