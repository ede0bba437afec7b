// rt_ray_hits.hpp -- what the all-hit ray kernels share: ray_hits_query.hip (rt_ray_hits_count / rt_ray_hits_collect) and
// ray_filter_query.hip (their filtered siblings) declare their own __global__ kernels around ONE body, rt_ray_hits_body.inc,
// included as text inside the kernel's braces.  Text, not a function template: the unfiltered kernels must stay the code they
// were, instruction for instruction, and a body reached through a call -- force-inlined or not -- is
// optimised in another order and comes out a few instructions different.  The including kernel names its parameters
// `RayHitsParams p` (and has a template parameter or constant COLLECT) and defines two macros around the #include:
//   RT_BODY_FILTER                     the lane's hit-filter type (rt_traverse.hpp: NoFilter; rt_ray_filter.hpp: RayFilter)
//   RT_BODY_MAKE_FILTER(i, in_range)   an expression that makes it for ray i
// What the traversal is and where its parts come from: ray_hits_query.hip's header.
#pragma once

#include "rt_csr.hpp"
#include "rt_device.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 16, "rt_ray: two 16-byte halves; rt_hit: one 16-byte record");

namespace rt {

namespace {   // (as in the kernels' own files: every translation unit has its own copy, and its own kernel symbols)

struct RayHitsParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* rays;           // rt_ray = two float4: (origin, tmin), (dir, tmax)
    uint32_t num_rays;
    uint64_t* offsets;            // count: out, workgroup-local prefixes; collect: in
    uint64_t* block_sums;         // count: out, one total per workgroup
    float4* hits;                 // collect: rt_hit = one float4: (t, primitive_id bits, u, v)
    uint32_t* counts;             // collect, optional
    unsigned long long* counters;
    uint32_t* status;
};

typedef uint32_t RhSpill[kStackMax - kCsrStackLds];

}  // namespace

}  // namespace rt
