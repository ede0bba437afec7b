// ray_hits_query.hip -- rt_ray_hits_count / rt_ray_hits_collect: EVERY triangle a ray crosses inside its [tmin, tmax] window,
// through any tree rt_intersect_rays takes (semantics: rt_abi.h, all-hit block).  The set-valued ray query:
// the result is CSR -- offsets[0..n] by a 64-bit device scan of the per-ray counts, then 16-byte hit records written per ray
// segment.
//
// A ray whose window never shrinks is one more region shape, so ray_hits_kernel<COLLECT> is range_query_kernel's frame with
// the slab test in the place of `keep` and Moller-Trumbore in the place of `match`: one lane per ray, 64 consecutive rays per
// wave, kTraceWaves waves (256 rays) per workgroup, xcd_chunk_block, the ray in two 16-byte loads, a leaf in four 16-byte
// requests, rt_traverse.hpp's wave-level two phases (box steps while enough lanes hold a box run, then one leaf step), exact
// per-workgroup counters.  What it takes from where:
//   * slab() and intersect_tri() are rt_traverse.hpp's, unchanged: a slot is entered iff back >= front && front <= tmax &&
//     back >= tmin with the ray's ORIGINAL tmin / tmax; intersect_tri writes r.tmax on acceptance and the kernel puts the
//     original value back after every test, so no test sees a shrunk window;
//   * nothing is ordered and nothing re-culled: a stack entry is the 4-byte entry alone (a box run child : 29 | count : 3, or
//     a leaf index : 29 | 0), 16 entries in an LDS column per lane (16 KB per workgroup) + 48 private; the first surviving
//     slot of a run is visited next, the others are pushed in slot order.  Both instantiations run this one traversal, so the
//     count and the collect call visit the same leaves in the same order and cannot disagree;
//   * a leaf entry does not carry the slot's count, so triangle B = (v2, v1, v3) is tested iff v3 != v2 bit for bit: a
//     single-triangle record has v3 == v2 (rt_abi.h, refit block) and every builder gives a leaf slot a count >= 1, which makes
//     this trace_ray's rule (count > 0 && v3 != v2) on every record the library writes;
//   * a push onto a full stack of 64 is dropped and flagged (RT_RAY_HITS_STACK_OVERFLOW): the row is then a subset;
//   * COLLECT = false: the lane's count goes through a workgroup scan (rt_csr.hpp: two 21-bit limbs); offsets[i] gets the
//     workgroup-local exclusive prefix and the workgroup's total goes to the scratch; launch_csr_offsets (csr_scan.hip) does
//     the rest, as for the range queries.  Three launches, nothing read back.
//   * COLLECT = true: the lane stores record j < offsets[i+1] - offsets[i] at hits[offsets[i] + j] -- its own segment, in its
//     own traversal order, one 16-byte vector store, no atomics on the output -- and keeps counting beyond the room
//     (counts[i], RT_RAY_HITS_TRUNCATED).  (u, v) go back to the caller's corners as in ray_query_kernel.
// Compiled with -ffp-contract=off and IEEE division: every accepted record is bit for bit the one rt_intersect_rays would
// report for that triangle.
// The kernel's body is rt_ray_hits_body.inc, shared as text with the filtered kernels of ray_filter_query.hip.
#include "rt_launch.hpp"
#include "rt_ray_hits.hpp"

namespace rt {

namespace {

template <bool COLLECT>
__global__ __launch_bounds__(kTraceWaves * 64, RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA) void ray_hits_kernel(RayHitsParams p)
{
#define RT_BODY_FILTER NoFilter
#define RT_BODY_MAKE_FILTER(i, in_range) NoFilter()
#include "rt_ray_hits_body.inc"
#undef RT_BODY_FILTER
#undef RT_BODY_MAKE_FILTER
}

RayHitsParams hits_params(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, uint64_t* counters, uint32_t* status)
{
    RayHitsParams p = {};
    p.nodes = as.nodes;
    p.leaves = as.triangles;
    p.root = as.root;
    p.count = as.count;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    return p;
}

}  // namespace

size_t ray_hits_scratch_bytes(uint32_t num_rays) { return csr_scratch_bytes(num_rays); }

hipError_t launch_ray_hits_count(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, uint64_t* offsets, void* scratch,
                                 uint64_t* counters, uint32_t* status, hipStream_t st)
{
    RayHitsParams p = hits_params(as, rays, num_rays, counters, status);
    p.offsets = offsets;
    p.block_sums = static_cast<uint64_t*>(scratch);
    const uint32_t blocks = csr_blocks(num_rays);
    if (blocks) ray_hits_kernel<false><<<blocks, kCsrBlock, 0, st>>>(p);
    return launch_csr_offsets(offsets, p.block_sums, num_rays, st);
}

hipError_t launch_ray_hits_collect(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const uint64_t* offsets,
                                   rt_hit* hits, uint32_t* counts, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    RayHitsParams p = hits_params(as, rays, num_rays, counters, status);
    p.offsets = const_cast<uint64_t*>(offsets);   // (the collect instantiation only reads them)
    p.hits = reinterpret_cast<float4*>(hits);
    p.counts = counts;
    ray_hits_kernel<true><<<csr_blocks(num_rays), kCsrBlock, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
