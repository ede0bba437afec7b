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
// No shading: the launch bounds are those of trace_kernel's lean (kDepth) instantiation.
// Compiled with -ffp-contract=off: results are bit-identical to trace_kernel's and the C oracle's.
#include "rt_device.hpp"
#include "rt_launch.hpp"
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

// launch position j -> ray index (0xFFFFFFFF: no ray -- num_rays is a uint32, so it is never in range)
template <bool INDEXED, class Params>
__device__ __forceinline__ uint64_t ray_index(const Params& p, uint64_t j)
{
    if constexpr (INDEXED) return j < p.num_indices ? p.order[j] : 0xFFFFFFFFull;
    else return j;
}

// One kernel body for both entry points.  INDEXED only changes how the lane's ray index i is obtained: the launch position
// itself, or order[position] (positions past num_indices and indices >= num_rays: no ray, nothing written).
template <bool PF, bool ANY, bool INDEXED>
__global__ __launch_bounds__(kTraceWaves * 64, PF ? RT_TRACE_PF_WAVES : RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA)
void ray_query_kernel(std::conditional_t<INDEXED, IndexedQueryParams, QueryParams> p)
{
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

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    Hit h = {0u, 0u, 0.f, 0.f};
    const bool hit = trace_ray<PF, ANY>(p, r, h, t, active, steps);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            // RotateAttributes: leaf corner k is the caller's corner i_k, so the caller's weights are W[i0] = 1-bu-bv,
            // W[i1] = bu, W[i2] = bv, and (u, v) = (W[1], W[2])
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

hipError_t launch_ray_query(const rt_accel& as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, bool any_hit,
                            uint32_t num_primitives, uint64_t* counters, hipStream_t st)
{
    QueryParams p;
    p.nodes = as.nodes;
    p.leaves = as.triangles;
    p.root = as.root;
    p.count = as.count;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.hits = reinterpret_cast<float4*>(hits);
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    const uint32_t rays_per_block = kTraceWaves * 64;
    const dim3 grid((uint32_t)(((uint64_t)num_rays + rays_per_block - 1) / rays_per_block)), block(rays_per_block);
    const bool pf = num_primitives >= kPrefetchMinPrims;   // as launch_trace: trees that do not fit the caches
    if (pf) {
        if (any_hit) ray_query_kernel<true, true, false><<<grid, block, 0, st>>>(p);
        else ray_query_kernel<true, false, false><<<grid, block, 0, st>>>(p);
    } else {
        if (any_hit) ray_query_kernel<false, true, false><<<grid, block, 0, st>>>(p);
        else ray_query_kernel<false, false, false><<<grid, block, 0, st>>>(p);
    }
    return hipGetLastError();
}

hipError_t launch_ray_query_indexed(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const uint32_t* order,
                                    uint32_t num_indices, rt_hit* hits, bool any_hit, uint32_t num_primitives,
                                    uint64_t* counters, hipStream_t st)
{
    IndexedQueryParams p;
    p.nodes = as.nodes;
    p.leaves = as.triangles;
    p.root = as.root;
    p.count = as.count;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.hits = reinterpret_cast<float4*>(hits);
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.order = order;
    p.num_indices = num_indices;
    const uint32_t rays_per_block = kTraceWaves * 64;
    const dim3 grid((uint32_t)(((uint64_t)num_indices + rays_per_block - 1) / rays_per_block)), block(rays_per_block);
    const bool pf = num_primitives >= kPrefetchMinPrims;   // as launch_ray_query
    if (pf) {
        if (any_hit) ray_query_kernel<true, true, true><<<grid, block, 0, st>>>(p);
        else ray_query_kernel<true, false, true><<<grid, block, 0, st>>>(p);
    } else {
        if (any_hit) ray_query_kernel<false, true, true><<<grid, block, 0, st>>>(p);
        else ray_query_kernel<false, false, true><<<grid, block, 0, st>>>(p);
    }
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
