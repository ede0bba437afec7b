// rt_ray_first.hpp -- what the first-K ray kernels share: ray_first_query.hip (rt_ray_first_hits) and ray_filter_query.hip
// (its filtered sibling) declare their own __global__ kernel around ONE body, rt_ray_first_body.inc, included as text inside
// the kernel's braces -- for the reason and with the two macros rt_ray_hits.hpp gives (RT_BODY_FILTER,
// RT_BODY_MAKE_FILTER(i, in_range)); the kernel names its parameters `RayFirstParams p`.  The filter is asked inside
// intersect_tri, before `offer`: a candidate that is turned down never moves the bound.
// What the traversal is: ray_first_query.hip's header.
#pragma once

#include "rt_device.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 16, "rt_ray: two 16-byte halves; rt_hit: one 16-byte record");

#ifndef RT_RAY_FIRST_PENDING
#define RT_RAY_FIRST_PENDING 4
#endif
static_assert(RT_RAY_FIRST_PENDING == 8 || RT_RAY_FIRST_PENDING == 4, "RT_RAY_FIRST_PENDING: 4 (entry) or 8 (entry, front)");

namespace rt {

namespace {   // (as in the kernels' own files: every translation unit has its own copy, and its own kernel symbols)

constexpr int kRfStackLds = 16;   // LDS-resident entries per lane: 16 x 4 B (or 8 B) x 256 lanes = 16 KB (32 KB) per workgroup

struct RayFirstParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* rays;           // rt_ray = two float4: (origin, tmin), (dir, tmax)
    float4* out;                  // rt_hit = one float4: (t, primitive_id bits, u, v); row i at out + i * k
    uint32_t num_rays, k;
    unsigned long long* counters;
    uint32_t* status;
};

#if RT_RAY_FIRST_PENDING == 8
typedef uint64_t RfEntry;         // entry (low word) | front bits (high word)
constexpr int kRfMinWaves = 5;    // 32 KB of LDS per workgroup of 4 waves: 5 workgroups per CU, 5 waves per SIMD
#else
typedef uint32_t RfEntry;
constexpr int kRfMinWaves = 6;    // 16 KB of LDS would allow 8, but 64 VGPRs spill eleven and 72 spill six: 6 waves, no spills
#endif
typedef RfEntry RfSpill[kStackMax - kRfStackLds];
typedef __attribute__((address_space(3))) RfEntry lds_rf_entry;

// (t, id) order with NaN above every number and equal to itself
__device__ __forceinline__ bool rf_same_t(float a, float b) { return a == b || (__builtin_isnan(a) && __builtin_isnan(b)); }
__device__ __forceinline__ bool rf_below(float t, uint32_t id, float et, uint32_t eid)
{
    return t < et || (!__builtin_isnan(t) && __builtin_isnan(et)) || (rf_same_t(t, et) && id < eid);
}

}  // namespace

}  // namespace rt
