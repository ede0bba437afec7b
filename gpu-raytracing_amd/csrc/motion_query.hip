// motion_query.hip -- the motion-blur ray query (rt_intersect_rays_motion) and the topology check of its two poses
// (rt_motion_validate).  rt_abi.h, motion block; DESIGN section 22.
//
// motion_query_kernel is ray_query_kernel (ray_query.hip) with a time per ray and two poses of one tree:
//   * the same launch shape: one lane per ray, 64 consecutive rays per wave, kTraceWaves waves per workgroup, workgroups
//     remapped to XCDs by xcd_chunk_block, the same LDS stack column and private spill, the same counters;
//   * a ray is two 16-byte loads and one 4-byte load (its time); w0 = 1 - time is computed once;
//   * the traversal is trace_ray_motion (rt_motion_traverse.hpp): every box step fetches the pair from both poses (eight
//     16-byte requests instead of four) and every leaf test both records, interpolates at the lane's time and runs
//     rt_traverse.hpp's tests.  The address path bounds the static tracer, and this kernel issues twice
//     its requests per step;
//   * lanes past num_rays, rays rt_intersect_rays would not trace, and rays whose time is NaN or outside [0, 1] trace nothing
//     (a miss, no tests counted) but still take part in the ballots;
//   * ids, rotations and the slots' w12 / w28 words are pose 0's (rt_motion_validate checks that pose 1's are the same).
// The registers of the doubled fetch cost occupancy: RT_MOTION_WAVES (rt_motion_traverse.hpp) is chosen so that nothing but
// the stack's own spill array lives in scratch.
// Compiled with -ffp-contract=off: the interpolation is two rounded products and one rounded sum, as rt_abi.h defines it.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_motion_traverse.hpp"

#include <type_traits>

namespace rt {

// rt_intersect_rays_motion_indexed: the same query through an index list (ray_query.hip's IndexedQueryParams: the plain
// part's kernarg offsets do not move)
namespace {   // (beside its base: rt_motion_traverse.hpp keeps MotionParams in the anonymous namespace)
struct IndexedMotionParams : MotionParams {
    const uint32_t* order;
    uint32_t num_indices;
};
}  // namespace

// INDEXED only changes how the lane's ray index i is obtained: the launch position itself, or order[position] (positions
// past num_indices and indices >= num_rays: no ray, nothing written).  rays, times and hits are indexed by i.  The choice
// stands HERE, under `if constexpr`, not in a helper function (DESIGN sections 20 and 32).
template <bool ANY, bool INDEXED>
__global__ __launch_bounds__(kTraceWaves * 64, RT_MOTION_WAVES)
void motion_query_kernel(std::conditional_t<INDEXED, IndexedMotionParams, MotionParams> p)
{
    __shared__ uint32_t stack_lds[kTraceWaves][kStackLds][64];
    __shared__ unsigned long long csum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p.counters) {                         // (kernel argument: the same for every thread)
        if (threadIdx.x < 4) csum[threadIdx.x] = 0ull;
        __syncthreads();
    }
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    if constexpr (INDEXED) i = i < p.num_indices ? p.order[i] : 0xFFFFFFFFull;   // (num_rays is a uint32: never in range)
    const bool in_range = i < p.num_rays;

    float4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, -1.f};
    float tau = 0.0f;
    if (in_range) { a = p.rays[2 * i]; b = p.rays[2 * i + 1]; tau = p.times[i]; }
    Ray r;
    r.ox = a.x; r.oy = a.y; r.oz = a.z; r.tmin = a.w;
    r.dx = b.x; r.dy = b.y; r.dz = b.z; r.tmax = b.w;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    // not traced (a miss, no tests): ray_query_kernel's cases, and a time that is NaN or outside [0, 1] (both compares are
    // false for a NaN)
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray && tau >= 0.0f && tau <= 1.0f;

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    Hit h = {0u, 0u, 0.f, 0.f};
    const bool hit = trace_ray_motion<ANY>(p, r, tau, h, t, active, steps);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            const uint32_t rot = p.leaves0[h.tri_id >> 1].rotations[h.tri_id & 1];
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

// rt_motion_validate: thread i compares slot i's w12 / w28 words (i < slots) and record i's id / rotations words (i < n)
// between the poses.  *status was cleared by the launch; every thread that finds a difference stores the same flag word (a
// plain store: one flag, so there is nothing to combine).
__global__ __launch_bounds__(256) void motion_validate_kernel(const uint4* nodes0, const uint4* nodes1, const uint4* leaves0,
                                                              const uint4* leaves1, uint32_t slots, uint32_t n, uint32_t* status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool differ = false;
    if (i < slots) {
        const uint64_t s = 2 * (uint64_t)i;   // (min, w12), (max, w28)
        differ = nodes0[s].w != nodes1[s].w || nodes0[s + 1].w != nodes1[s + 1].w;
    }
    if (i < n) {
        const uint64_t k = 4 * (uint64_t)i;   // (v0, id 0), (v1, id 1), (v2, rotations), (v3, pad)
        differ |= leaves0[k].w != leaves1[k].w || leaves0[k + 1].w != leaves1[k + 1].w || leaves0[k + 2].w != leaves1[k + 2].w;
    }
    if (differ) *status = RT_MOTION_TOPOLOGY_MISMATCH;
}

static_assert(kQueryBlock == kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

hipError_t launch_motion_query(const rt_motion_accel& as, const rt_ray* rays, const float* times, rt_hit* hits, uint32_t num_rays,
                               const uint32_t* order, uint32_t num_indices, bool any_hit, uint64_t* counters, hipStream_t st)
{
    IndexedMotionParams p;
    p.nodes0 = as.nodes0;
    p.leaves0 = as.triangles0;
    p.nodes1 = as.nodes1;
    p.leaves1 = as.triangles1;
    p.root = as.root;
    p.count = as.count;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.times = times;
    p.hits = reinterpret_cast<float4*>(hits);
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.order = order;
    p.num_indices = num_indices;
    const dim3 grid(query_blocks(order ? num_indices : num_rays)), block(kQueryBlock);
    if (order) {
        if (any_hit) motion_query_kernel<true, true><<<grid, block, 0, st>>>(p);
        else motion_query_kernel<false, true><<<grid, block, 0, st>>>(p);
    } else {
        if (any_hit) motion_query_kernel<true, false><<<grid, block, 0, st>>>(p);   // (its MotionParams part)
        else motion_query_kernel<false, false><<<grid, block, 0, st>>>(p);
    }
    return hipGetLastError();
}

hipError_t launch_motion_validate(const rt_motion_accel& as, uint32_t num_triangles, uint32_t* status, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || as.count == 0) return e;
    const uint32_t slots = (uint32_t)(rt_nodes_bytes(num_triangles) / 32);   // (> num_triangles)
    motion_validate_kernel<<<dim3((slots + 255) / 256), dim3(256), 0, st>>>(
        reinterpret_cast<const uint4*>(as.nodes0), reinterpret_cast<const uint4*>(as.nodes1),
        reinterpret_cast<const uint4*>(as.triangles0), reinterpret_cast<const uint4*>(as.triangles1), slots, num_triangles, status);
    return hipGetLastError();
}

}  // namespace rt
