// instance_filter_query.hip -- rt_intersect_rays_instanced_filtered: the instanced ray query with an instance visibility mask,
// world-space face culling and a per-ray (instance, primitive) skip (semantics: rt_abi.h, instance-filter block; DESIGN
// section 21).
//
// instance_query_filtered_kernel<PF, ANY> is instance_query_kernel's body (rt_instance_query_body.inc, one text for both)
// around the same two-level loop, trace_instanced (rt_instance_traverse.hpp), with one more policy, the lane's
// InstanceRayFilter (rt_instance_filter.hpp):
//   * ray setup: one 16-byte load of the ray's {mask, skip_instance, skip_id} when the caller gave per-ray records;
//   * PH_ENTER: the instance rule comes first -- one 8-byte load of the instance's {mask, flags} (none when the instance has no
//     record), and an instance whose mask misses the ray's is left like a flagged one: no record load, no rt_accel load, the
//     lane advances in the TLAS.  An entered instance sets the lane's per-instance part from the w0 .. w2 rows the kernel has
//     already loaded: the effective cull bits (the 3x3 determinant's sign only when a cull bit is set -- the flags are
//     wave-uniform) and the effective skip id;
//   * leaf test: that per-instance part goes by value to intersect_tri, which asks it after the t window test and before
//     r.tmax = t -- a rejected candidate shrinks no window and ends no any-hit ray.
// Launch bounds, LDS stack, XCD remap and per-workgroup counters are the sibling's.  instances.hip's kernels are untouched by
// this file: NoInstanceFilter instantiations keep their code (the assembly comparison).
// Compiled with -ffp-contract=off and IEEE division like every ray query: a kept record is the unfiltered record, bit for bit.
#include "rt_launch.hpp"
#include "rt_instance_filter.hpp"
#include "rt_instance_traverse.hpp"

namespace rt {

namespace {

// instance_query_kernel's body with the lane's InstanceRayFilter handed to trace_instanced
template <bool PF, bool ANY>
__global__ __launch_bounds__(kTraceWaves * 64, RT_INSTANCE_QUERY_WAVES)
void instance_query_filtered_kernel(InstParams p, InstanceFilterParams fp)
{
#define RT_BODY_MAKE_FILTER(i, in_range) instance_ray_filter(fp, i, in_range)
#include "rt_instance_query_body.inc"
#undef RT_BODY_MAKE_FILTER
}

}  // namespace

hipError_t launch_instance_query_filtered(const InstanceQuery& q, const rt_instance_hit_filter& filter, hipStream_t st)
{
    InstParams p;
    p.tlas_nodes = q.tlas.nodes;
    p.tlas_leaves = q.tlas.triangles;
    p.root = q.tlas.root;
    p.count = q.tlas.count;
    p.records = q.records;
    p.num_instances = q.num_instances;
    p.num_blas = q.num_blas;
    p.blas_table = q.blas_table;
    p.rays = reinterpret_cast<const float4*>(q.rays);
    p.hits = reinterpret_cast<float4*>(q.hits);
    p.instance_ids = q.instance_ids;
    p.num_rays = q.num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(q.counters);
    InstanceFilterParams fp;
    fp.flags = filter.flags;
    fp.ray_mask = filter.ray_mask;
    fp.num_filters = filter.per_instance ? filter.num_instance_filters : 0u;   // an absent array: nothing is read, every instance mask is all ones
    fp.per_instance = reinterpret_cast<const uint2*>(filter.per_instance);
    fp.per_ray = reinterpret_cast<const uint4*>(filter.per_ray);
    const uint32_t rays_per_block = kTraceWaves * 64;
    const dim3 grid((uint32_t)(((uint64_t)q.num_rays + rays_per_block - 1) / rays_per_block)), block(rays_per_block);
    const bool pf = q.num_primitives >= kPrefetchMinPrims;   // as launch_instance_query
    if (pf) {
        if (q.any_hit) instance_query_filtered_kernel<true, true><<<grid, block, 0, st>>>(p, fp);
        else instance_query_filtered_kernel<true, false><<<grid, block, 0, st>>>(p, fp);
    } else {
        if (q.any_hit) instance_query_filtered_kernel<false, true><<<grid, block, 0, st>>>(p, fp);
        else instance_query_filtered_kernel<false, false><<<grid, block, 0, st>>>(p, fp);
    }
    return hipGetLastError();
}

}  // namespace rt
