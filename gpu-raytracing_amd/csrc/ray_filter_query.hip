// ray_filter_query.hip -- the filtered ray queries: rt_intersect_rays_filtered, rt_ray_hits_count_filtered,
// rt_ray_hits_collect_filtered, rt_ray_first_hits_filtered (semantics: rt_abi.h, hit-filter block).
//
// Each kernel here is its unfiltered sibling's traversal with one more policy at the one place where a candidate is accepted:
//   * closest / any: ray_query_filtered_kernel is ray_query_kernel's frame around trace_ray<PF, ANY> (rt_traverse.hpp) with a
//     RayFilter handed down to intersect_tri, which asks it after the t window test and before r.tmax = t -- a rejected
//     candidate shrinks no window and ends no any-hit ray;
//   * all-hit: rt_ray_hits_body.inc (rt_ray_hits.hpp) with RayFilter -- asked before the record is counted or stored;
//   * first-K: rt_ray_first_body.inc (rt_ray_first.hpp) with RayFilter -- asked before `offer`, so the bound only ever falls
//     to the t of a kept record.
// There is no post-pass: box tests, leaf visits, liveness, stack and status rules are the siblings', instruction for
// instruction.  The filter (rt_ray_filter.hpp) costs one 8-byte load per ray at ray setup when the caller gave per-ray
// records, and per candidate that passed Moller-Trumbore and the window: two compares of the determinant that is already in
// registers, one compare against skip_id, and -- only for a candidate that survived those -- one 4-byte prim_masks load.
// The existing kernels are untouched by this file: NoFilter instantiations keep their code (the assembly
// comparison).
// Compiled with -ffp-contract=off and IEEE division like every ray query: a kept record is the unfiltered record, bit for bit.
#include "rt_launch.hpp"
#include "rt_ray_filter.hpp"
#include "rt_ray_first.hpp"
#include "rt_ray_hits.hpp"

namespace rt {

namespace {

FilterParams filter_params(const rt_hit_filter& f)
{
    FilterParams fp;
    fp.flags = f.flags;
    fp.ray_mask = f.ray_mask;
    fp.num_prims = f.prim_masks ? f.num_primitives : 0u;   // an absent array: nothing is read, every primitive mask is all ones
    fp.prim_masks = f.prim_masks;
    fp.per_ray = reinterpret_cast<const uint2*>(f.per_ray);
    return fp;
}

// ---- closest / any
struct FilteredQueryParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* rays;   // rt_ray = two float4: (origin, tmin), (dir, tmax)
    float4* hits;         // rt_hit = one float4: (t, primitive_id bits, u, v)
    uint32_t num_rays;
    unsigned long long* counters;
    FilterParams filter;
    static constexpr int park_num = kParkNum, park_den = kParkDen;   // (trace_ray reads them as members)
};

// ray_query_kernel (ray_query.hip) with the lane's RayFilter handed to trace_ray; everything else is that kernel's
template <bool PF, bool ANY>
__global__ __launch_bounds__(kTraceWaves * 64, PF ? RT_TRACE_PF_WAVES : RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA)
void ray_query_filtered_kernel(FilteredQueryParams p)
{
    __shared__ uint32_t stack_lds[kTraceWaves][kStackLds][64];
    __shared__ unsigned long long csum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p.counters) {                         // (kernel argument: the same for every thread)
        if (threadIdx.x < 4) csum[threadIdx.x] = 0ull;
        __syncthreads();
    }
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_rays;

    float4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, -1.f};
    if (in_range) { a = p.rays[2 * i]; b = p.rays[2 * i + 1]; }
    Ray r;
    r.ox = a.x; r.oy = a.y; r.oz = a.z; r.tmin = a.w;
    r.dx = b.x; r.dy = b.y; r.dz = b.z; r.tmax = b.w;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray;
    const RayFilter flt = ray_filter(p.filter, i, in_range);

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    Hit h = {0u, 0u, 0.f, 0.f};
    const bool hit = trace_ray<PF, ANY>(p, r, h, t, active, steps, flt);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            // RotateAttributes, as ray_query_kernel
            const uint32_t rot = p.leaves[h.tri_id >> 1].rotations[h.tri_id & 1];
            const float w0 = 1 - h.bu - h.bv;
            o.x = r.tmax;
            o.y = __uint_as_float(h.primitive_id);
            o.z = rot == 1 ? h.bv : (rot == 2 ? w0 : h.bu);
            o.w = rot == 1 ? w0 : (rot == 2 ? h.bu : h.bv);
        }
        p.hits[i] = o;
    }
    if (p.counters) {
        const uint32_t bsum = wave_sum_u32(t.box_tests), tsum = wave_sum_u32(t.tri_tests);
        if (lane == 0) {
            atomicAdd(&csum[0], (unsigned long long)bsum);
            atomicAdd(&csum[1], (unsigned long long)tsum);
            atomicAdd(&csum[2], (unsigned long long)steps[0]);
            atomicAdd(&csum[3], (unsigned long long)steps[1]);
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const unsigned long long v = csum[threadIdx.x];
            if (v) atomicAdd(&p.counters[threadIdx.x], v);
        }
    }
}

// ---- all-hit
template <bool COLLECT>
__global__ __launch_bounds__(kTraceWaves * 64, RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA)
void ray_hits_filtered_kernel(RayHitsParams p, FilterParams fp)
{
#define RT_BODY_FILTER RayFilter
#define RT_BODY_MAKE_FILTER(i, in_range) ray_filter(fp, i, in_range)
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

// ---- first-K
__global__ __launch_bounds__(kTraceWaves * 64, kRfMinWaves) void ray_first_filtered_kernel(RayFirstParams p, FilterParams fp)
{
#define RT_BODY_FILTER RayFilter
#define RT_BODY_MAKE_FILTER(i, in_range) ray_filter(fp, i, in_range)
#include "rt_ray_first_body.inc"
#undef RT_BODY_FILTER
#undef RT_BODY_MAKE_FILTER
}

}  // namespace

hipError_t launch_ray_query_filtered(const rt_accel& as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, bool any_hit,
                                     uint32_t num_primitives, const rt_hit_filter& filter, uint64_t* counters, hipStream_t st)
{
    FilteredQueryParams p;
    p.nodes = as.nodes;
    p.leaves = as.triangles;
    p.root = as.root;
    p.count = as.count;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.hits = reinterpret_cast<float4*>(hits);
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.filter = filter_params(filter);
    const uint32_t rays_per_block = kTraceWaves * 64;
    const dim3 grid((uint32_t)(((uint64_t)num_rays + rays_per_block - 1) / rays_per_block)), block(rays_per_block);
    const bool pf = num_primitives >= kPrefetchMinPrims;   // as launch_ray_query
    if (pf) {
        if (any_hit) ray_query_filtered_kernel<true, true><<<grid, block, 0, st>>>(p);
        else ray_query_filtered_kernel<true, false><<<grid, block, 0, st>>>(p);
    } else {
        if (any_hit) ray_query_filtered_kernel<false, true><<<grid, block, 0, st>>>(p);
        else ray_query_filtered_kernel<false, false><<<grid, block, 0, st>>>(p);
    }
    return hipGetLastError();
}

hipError_t launch_ray_hits_count_filtered(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter& filter,
                                          uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    RayHitsParams p = hits_params(as, rays, num_rays, counters, status);
    p.offsets = offsets;
    p.block_sums = static_cast<uint64_t*>(scratch);
    const uint32_t blocks = csr_blocks(num_rays);
    if (blocks) ray_hits_filtered_kernel<false><<<blocks, kCsrBlock, 0, st>>>(p, filter_params(filter));
    return launch_csr_offsets(offsets, p.block_sums, num_rays, st);
}

hipError_t launch_ray_hits_collect_filtered(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter& filter,
                                            const uint64_t* offsets, rt_hit* hits, uint32_t* counts, uint64_t* counters,
                                            uint32_t* status, hipStream_t st)
{
    RayHitsParams p = hits_params(as, rays, num_rays, counters, status);
    p.offsets = const_cast<uint64_t*>(offsets);   // (the collect instantiation only reads them)
    p.hits = reinterpret_cast<float4*>(hits);
    p.counts = counts;
    ray_hits_filtered_kernel<true><<<csr_blocks(num_rays), kCsrBlock, 0, st>>>(p, filter_params(filter));
    return hipGetLastError();
}

hipError_t launch_ray_first_hits_filtered(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, uint32_t k,
                                          const rt_hit_filter& filter, rt_hit* out, uint64_t* counters, uint32_t* status,
                                          hipStream_t st)
{
    RayFirstParams p;
    p.nodes = as.nodes;
    p.leaves = as.triangles;
    p.root = as.root;
    p.count = as.count;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.out = reinterpret_cast<float4*>(out);
    p.num_rays = num_rays;
    p.k = k;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    const uint32_t per_block = kTraceWaves * 64;
    const dim3 grid((uint32_t)(((uint64_t)num_rays + per_block - 1) / per_block)), block(per_block);
    ray_first_filtered_kernel<<<grid, block, 0, st>>>(p, filter_params(filter));
    return hipGetLastError();
}

}  // namespace rt
