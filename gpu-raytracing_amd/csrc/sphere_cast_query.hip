// sphere_cast_query.hip -- rt_sphere_cast: how far a ball of radius rad travels along each ray before it touches the mesh, and
// where it touches (semantics: rt_abi.h, sphere-cast block).  A new query over the existing triangle
// trees: no builder, no prepare step.
//
// sphere_cast_kernel<ANY, INDEXED>: sphere_query_kernel's launch shape -- one lane per ray, 64 consecutive rays (or order[]
// entries) per wave, kTraceWaves waves per workgroup, workgroups remapped to XCDs in chunks of 8, the lane-interleaved LDS
// stack with its private spill, counters wave-reduced, added in LDS and published with 4 device atomics per workgroup -- on
// the traversal of rt_sphere_cast_traverse.hpp: the tracer's box phase on boxes grown by the lane's radius, the swept test at
// the leaf.  A ray is two 16-byte loads and (with per-ray radii) one 4-byte load, plus the root run's slots once for the
// pad; a leaf visit four 16-byte loads (load_leaf_wide); the record one 16-byte store and, when asked for, one 4-byte store.
// Lanes past the batch, rays with an empty or NaN [tmin, tmax], rays with a NaN component and rays whose radius is negative,
// NaN or +inf trace nothing.  Lanes with rad == 0 run the ray query's tests on ungrown boxes; they may share a wave with
// lanes of rad > 0.  No pair-prefetch arm, no hold at pop.
// Compiled with -ffp-contract=off: every float operation is the documented one.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_sphere_cast_traverse.hpp"
#include "rt_traverse.hpp"

static_assert(rt::kQueryBlock == rt::kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

namespace rt {

namespace {

template <bool ANY, bool INDEXED>
__global__ __launch_bounds__(kTraceWaves * 64, RT_SPHERE_CAST_WAVES)
void sphere_cast_kernel(CastParams p)
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
    float rad = p.radius;
    if (in_range) {
        a = p.rays[2 * i];
        b = p.rays[2 * i + 1];
        if (p.radii) rad = p.radii[i];
    }
    Ray r;
    r.ox = a.x; r.oy = a.y; r.oz = a.z; r.tmin = a.w;
    r.dx = b.x; r.dy = b.y; r.dz = b.z; r.tmax = b.w;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    // not traced (a miss, no tests): as ray_query_kernel, and a radius that is negative, NaN or +inf
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool bad_rad = !(rad >= 0.0f) || rad == __builtin_inff();
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray && !bad_rad;
    if (!active) rad = 0.0f;

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    CastHit ch = {{0u, 0u, 0.f, 0.f}, (uint32_t)RT_SWEEP_NONE};
    const bool hit = trace_sphere_cast<ANY>(p, r, rad, ch, t, active, steps);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            if (ch.feature == RT_SWEEP_OVERLAP) {
                o = float4{r.tmax, __uint_as_float(ch.h.primitive_id), ch.h.bu + 0.0f, ch.h.bv + 0.0f};   // (+ 0: -0 becomes +0, as rt_closest_points writes them)
            } else {
                const uint32_t rot = p.leaves[ch.h.tri_id >> 1].rotations[ch.h.tri_id & 1];
                o = hit_record(r.tmax, ch.h.primitive_id, ch.h.bu, ch.h.bv, rot);
            }
        }
        p.hits[i] = o;
        if (p.features) p.features[i] = hit ? ch.feature : (uint32_t)RT_SWEEP_NONE;
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

}  // namespace

hipError_t launch_sphere_cast(const rt_accel& as, const rt_ray* rays, const float* radii, float radius, uint32_t num_rays,
                              const uint32_t* order, uint32_t num_indices, rt_hit* hits, uint32_t* features, bool any_hit,
                              uint64_t* counters, hipStream_t st)
{
    CastParams p;
    set_tree(p, as);
    p.rays = reinterpret_cast<const float4*>(rays);
    p.radii = radii;
    p.radius = radius;
    p.hits = reinterpret_cast<float4*>(hits);
    p.features = features;
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.order = order;
    p.num_indices = order ? num_indices : 0u;
    const dim3 grid(query_blocks(order ? num_indices : num_rays)), block(kQueryBlock);
    if (order) {
        if (any_hit) sphere_cast_kernel<true, true><<<grid, block, 0, st>>>(p);
        else sphere_cast_kernel<false, true><<<grid, block, 0, st>>>(p);
    } else {
        if (any_hit) sphere_cast_kernel<true, false><<<grid, block, 0, st>>>(p);
        else sphere_cast_kernel<false, false><<<grid, block, 0, st>>>(p);
    }
    return hipGetLastError();
}

}  // namespace rt
