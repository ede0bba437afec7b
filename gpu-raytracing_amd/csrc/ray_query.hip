// ray_query.hip -- caller rays -> hit records (rt_intersect_rays) and the camera-ray generator (rt_generate_camera_rays).
//
// ray_query_kernel runs the traversal of trace_kernel (rt_traverse.hpp: the wave-level two-phase loop, the lane-interleaved
// LDS stack with its private spill, the pair prefetch of the PF instantiation) on rays it loads instead of rays it makes:
//   * one lane per ray, 64 consecutive rays per wave, kTraceWaves waves (256 rays) per workgroup, workgroups remapped to
//     XCDs in chunks of 8 as in trace_kernel -- rays laid out in RT_RAYS_TILED order give a wave one 8 x 8 tile of one
//     sample, trace_kernel's coherence;
//   * a ray is two 16-byte loads, 1/dir is computed once (IEEE division: bit-identical to trace_kernel's), the record one
//     16-byte store; ray and hit addresses are 64-bit;
//   * lanes past num_rays, rays with an empty or NaN [tmin, tmax] and rays with a NaN component trace nothing (a miss, no
//     tests counted) but still take part in the ballots;
//   * ANY: a lane is done at its first accepted triangle (trace_ray<PF, true>);
//   * the record's (u, v) are mapped from the leaf triangle's corners to the caller's through TrianglePair::rotations with
//     the corner map of RotateAttributes (trace_kernel.hip shade_sample; Tracer.cu:57-82);
//   * counters (optional): the four sums are wave-reduced, added in LDS, and published with 4 device atomics per workgroup
//     (exact; no shared slots).  At 8,100 workgroups per 1080p frame those same-address atomics queue at ~18 ns each, about
//     0.15 ms behind the last workgroup -- a cost of counting, not of the query (counters off: none).
//   * FILTERED (rt_intersect_rays_filtered; rt_abi.h, hit-filter block): the lane's RayFilter
//     (rt_ray_filter.hpp) goes down to intersect_tri, which asks it after the t window test and before r.tmax = t -- a
//     rejected candidate shrinks no window and ends no any-hit ray.  No post-pass: box tests, leaf visits and stack are the
//     unfiltered arm's.  Cost: one 8-byte load per ray at ray setup when the caller gave per-ray records, and per candidate
//     that passed Moller-Trumbore and the window two compares of the determinant already in registers, one compare against
//     skip_id and -- only for a survivor -- one 4-byte prim_masks load.  A kept record is the unfiltered record, bit for bit.
// No shading: the launch bounds are those of trace_kernel's lean (kDepth) instantiation.
// Compiled with -ffp-contract=off: results are bit-identical to trace_kernel's and the C oracle's.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_ray_filter.hpp"
#include "rt_traverse.hpp"

#include <type_traits>

namespace rt {

struct QueryParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* rays;   // rt_ray = two float4: (origin, tmin), (dir, tmax)
    float4* hits;         // rt_hit = one float4: (t, primitive_id bits, u, v)
    uint32_t num_rays;
    unsigned long long* counters;
    static constexpr int park_num = kParkNum, park_den = kParkDen;   // (trace_ray reads them as members)
};

// rt_intersect_rays_indexed: the same query through an index list.  Launch position j takes ray order[j]; everything after
// the choice of the ray index is the same code.
struct IndexedQueryParams : QueryParams {
    const uint32_t* order;
    uint32_t num_indices;
};

// rt_intersect_rays_filtered: the same query with a hit filter (never indexed: there is no such entry point)
struct FilteredQueryParams : QueryParams {
    FilterParams filter;
};

// launch position j -> ray index (0xFFFFFFFF: no ray -- num_rays is a uint32, so it is never in range)
template <bool INDEXED, class Params>
__device__ __forceinline__ uint64_t ray_index(const Params& p, uint64_t j)
{
    if constexpr (INDEXED) return j < p.num_indices ? p.order[j] : 0xFFFFFFFFull;
    else return j;
}

// One kernel body for the three entry points.  INDEXED only changes how the lane's ray index i is obtained: the launch
// position itself, or order[position] (positions past num_indices and indices >= num_rays: no ray, nothing written).
// FILTERED only changes the policy handed to trace_ray.  The lane's filter is made HERE, under `if constexpr`: made by a
// helper function it changes the unfiltered arms' code.
template <bool PF, bool ANY, bool INDEXED, bool FILTERED>
__global__ __launch_bounds__(kTraceWaves * 64, PF ? RT_TRACE_PF_WAVES : RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA)
void ray_query_kernel(std::conditional_t<FILTERED, FilteredQueryParams,
                                         std::conditional_t<INDEXED, IndexedQueryParams, QueryParams>> p)
{
    static_assert(!(INDEXED && FILTERED), "there is no filtered indexed query");
    __shared__ uint32_t stack_lds[kTraceWaves][kStackLds][64];
    __shared__ unsigned long long csum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p.counters) {                         // (kernel argument: the same for every thread)
        if (threadIdx.x < 4) csum[threadIdx.x] = 0ull;
        __syncthreads();
    }
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ray_index<INDEXED>(p, ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane);
    const bool in_range = i < p.num_rays;

    float4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, -1.f};
    if (in_range) { a = p.rays[2 * i]; b = p.rays[2 * i + 1]; }
    Ray r;
    r.ox = a.x; r.oy = a.y; r.oz = a.z; r.tmin = a.w;
    r.dx = b.x; r.dy = b.y; r.dz = b.z; r.tmax = b.w;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    // not traced (a miss, no tests): lanes past the batch, an empty or NaN [tmin, tmax], a NaN origin or direction (the slab
    // test's fminf / fmaxf drop a NaN axis and Moller-Trumbore's range tests pass NaN: such a ray could "hit" at t = NaN)
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray;
    std::conditional_t<FILTERED, RayFilter, NoFilter> flt;
    if constexpr (FILTERED) flt = ray_filter(p.filter, i, in_range);

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
            const uint32_t rot = p.leaves[h.tri_id >> 1].rotations[h.tri_id & 1];
            o = hit_record(r.tmax, h.primitive_id, h.bu, h.bv, rot);
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

// rt_generate_camera_rays: one thread per ray (see rt_abi.h for the two layouts)
__global__ __launch_bounds__(256) void camera_rays_kernel(const rt_camera* camera, uint32_t w, uint32_t h, uint32_t spp,
                                                          uint32_t tiles_x, int tiled, uint64_t num_rays, float4* rays)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= num_rays) return;
    uint32_t x, y, s;
    if (tiled) {
        // lane -> pixel inside the 8x8 tile, Morton order (as trace_kernel)
        const uint32_t lane = (uint32_t)(i & 63u);
        const uint64_t q = i >> 6;
        s = (uint32_t)(q % spp);
        const uint64_t tile = q / spp;
        const uint32_t lx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4);
        const uint32_t ly = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4);
        x = (uint32_t)(tile % tiles_x) * 8 + lx;
        y = (uint32_t)(tile / tiles_x) * 8 + ly;
    } else {
        s = (uint32_t)(i % spp);
        const uint64_t pix = i / spp;
        x = (uint32_t)(pix % w);
        y = (uint32_t)(pix / w);
    }
    float ox = 0.5f, oy = 0.5f;
    if (spp > 1) subpixel_offset(s, spp, ox, oy);
    const rt_camera cam = *camera;
    Ray r;
    camera_ray(cam, w, h, x, y, ox, oy, r);
    if (x >= w || y >= h) { r.dx = r.dy = r.dz = 0.0f; r.tmax = -1.0f; }   // off-frame lane of an edge tile: tmax < tmin
    rays[2 * i] = float4{r.ox, r.oy, r.oz, r.tmin};
    rays[2 * i + 1] = float4{r.dx, r.dy, r.dz, r.tmax};
}

static_assert(kQueryBlock == kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

// the fields both launches fill (P: FilteredQueryParams or IndexedQueryParams)
template <class P>
static P query_params(const rt_accel& as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, uint64_t* counters)
{
    P p;
    set_tree(p, as);
    p.rays = reinterpret_cast<const float4*>(rays);
    p.hits = reinterpret_cast<float4*>(hits);
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    return p;
}

hipError_t launch_ray_query(const rt_accel& as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, bool any_hit,
                            uint32_t num_primitives, const rt_hit_filter* filter, uint64_t* counters, hipStream_t st)
{
    FilteredQueryParams p = query_params<FilteredQueryParams>(as, rays, hits, num_rays, counters);
    if (filter) p.filter = filter_params(*filter);
    const dim3 grid(query_blocks(num_rays)), block(kQueryBlock);
    // pf as launch_trace: trees that do not fit the caches
    dispatch_pf_any(num_primitives >= kPrefetchMinPrims, any_hit, [&](auto pf, auto any) {
        if (filter) ray_query_kernel<pf(), any(), false, true><<<grid, block, 0, st>>>(p);
        else ray_query_kernel<pf(), any(), false, false><<<grid, block, 0, st>>>(p);   // (its QueryParams part)
    });
    return hipGetLastError();
}

hipError_t launch_ray_query_indexed(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const uint32_t* order,
                                    uint32_t num_indices, rt_hit* hits, bool any_hit, uint32_t num_primitives,
                                    uint64_t* counters, hipStream_t st)
{
    IndexedQueryParams p = query_params<IndexedQueryParams>(as, rays, hits, num_rays, counters);
    p.order = order;
    p.num_indices = num_indices;
    const dim3 grid(query_blocks(num_indices)), block(kQueryBlock);
    dispatch_pf_any(num_primitives >= kPrefetchMinPrims, any_hit, [&](auto pf, auto any) {
        ray_query_kernel<pf(), any(), true, false><<<grid, block, 0, st>>>(p);
    });
    return hipGetLastError();
}

hipError_t launch_camera_rays(const rt_camera* camera, uint32_t w, uint32_t h, uint32_t spp, bool tiled, rt_ray* rays,
                              hipStream_t st)
{
    const uint32_t tiles_x = (w + 7) / 8, tiles_y = (h + 7) / 8;
    const uint64_t n = tiled ? (uint64_t)tiles_x * tiles_y * spp * 64u : (uint64_t)w * h * spp;
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
    camera_rays_kernel<<<dim3((uint32_t)blocks), dim3(256), 0, st>>>(camera, w, h, spp, tiles_x, tiled ? 1 : 0, n,
                                                                      reinterpret_cast<float4*>(rays));
    return hipGetLastError();
}

}  // namespace rt
