// instance_motion_query.hip -- rt_prepare_motion_instances and rt_intersect_rays_instanced_motion: ray queries over placed
// copies of built trees whose placement moves during the shutter, a time per ray (semantics: rt_abi.h, instance-motion block;
// DESIGN section 23).
//
// prepare_motion_instances_kernel, one thread per instance: the proxy of the BLAS's object box under each of the two key
// matrices (rt_instance_proxy.hpp: rt_prepare_instances's arithmetic, pose by pose) and the validated copy of the input as
// the record.  No inverse is stored: it depends on the ray's time.
//
// instance_motion_query_kernel<ANY> is instance_query_kernel<false, ANY, false> (instances.hip) with a time per ray:
//   * the same launch shape, LDS stack, XCD remap and counters; a ray is two 16-byte loads and its time;
//   * the traversal is trace_instanced_motion (rt_instance_motion_traverse.hpp): TLAS steps read both TLAS poses and
//     interpolate, entering an instance interpolates its two matrices at the lane's time and inverts the result in float32,
//     BLAS steps and leaf tests are the static ones;
//   * lanes past num_rays, rays rt_intersect_rays would not trace, and rays whose time is NaN or outside [0, 1] trace nothing
//     (a miss, RT_MISS, no tests counted) but still take part in the ballots.
// RT_INSTANCE_MOTION_WAVES (rt_instance_motion_traverse.hpp) is chosen so that nothing but the stack's own spill array lives
// in scratch.
// Compiled with -ffp-contract=off: every float operation is the documented one.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_instance_motion_traverse.hpp"
#include "rt_instance_proxy.hpp"

#include <type_traits>

static_assert(sizeof(rt_motion_instance) == 128 && offsetof(rt_motion_instance, object_to_world1) == 48 &&
              offsetof(rt_motion_instance, blas) == 96, "rt_motion_instance: two 3x4 matrices, blas, 7 pads");
static_assert(sizeof(rt_motion_instance_record) == 128 && offsetof(rt_motion_instance_record, object_to_world1) == 48 &&
              offsetof(rt_motion_instance_record, blas) == 96 && offsetof(rt_motion_instance_record, flags) == 100,
              "rt_motion_instance_record: two 3x4 matrices, blas, flags, 6 spare");
static_assert(rt::kQueryBlock == rt::kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

namespace rt {

namespace {

// a key matrix's part of RT_INSTANCE_SINGULAR: finite entries, and the 3x3 determinant in double as prepare_instances_kernel
__device__ __forceinline__ double key_determinant(const float* m, bool& finite)
{
    for (int k = 0; k < 12; k++) finite &= __builtin_isfinite(m[k]);
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    return a00 * c00 + a01 * c01 + a02 * c02;
}

// ---------------------------------------------------------------- prepare
__global__ __launch_bounds__(256) void prepare_motion_instances_kernel(const rt_motion_instance* instances,
                                                                       uint32_t num_instances, const rt_accel* blas_table,
                                                                       uint32_t num_blas, rt_triangle* proxies0,
                                                                       rt_triangle* proxies1, rt_motion_instance_record* records,
                                                                       uint32_t* status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= num_instances) return;
    const rt_motion_instance in = instances[i];

    int lo_i[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi_i[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    uint32_t flags = 0;
    instance_object_box(blas_table, num_blas, in.blas, lo_i, hi_i, flags);

    // singular: at either key, or in between (determinants of opposite sign: the interpolated matrix passes through one)
    bool finite = true;
    const double det0 = key_determinant(in.object_to_world0, finite), det1 = key_determinant(in.object_to_world1, finite);
    if (!finite || det0 == 0.0 || det1 == 0.0 || (det0 < 0.0) != (det1 < 0.0)) flags |= RT_INSTANCE_SINGULAR;

    rt_motion_instance_record rec;
    for (int k = 0; k < 12; k++) {
        rec.object_to_world0[k] = in.object_to_world0[k];
        rec.object_to_world1[k] = in.object_to_world1[k];
    }
    rec.blas = in.blas;
    rec.flags = flags;
    for (int k = 0; k < 6; k++) rec.spare[k] = 0;
    records[i] = rec;

    rt_triangle px0 = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, px1 = px0;   // flagged: point proxies at the origin
    if (!flags) {
        Affine34 m0, m1;
        for (int k = 0; k < 12; k++) { m0.m[k] = in.object_to_world0[k]; m1.m[k] = in.object_to_world1[k]; }
        px0 = proxy_triangle(instance_proxy(m0, lo_i, hi_i));
        px1 = proxy_triangle(instance_proxy(m1, lo_i, hi_i));
    }
    proxies0[i] = px0;
    proxies1[i] = px1;
    if (flags) atomicOr(status, flags);
}

}  // namespace

// ---------------------------------------------------------------- query (the two-level loop: rt_instance_motion_traverse.hpp)
// rt_intersect_rays_instanced_motion_indexed: the same query through an index list (ray_query.hip's IndexedQueryParams: the
// plain part's kernarg offsets do not move)
namespace {   // (beside its base: rt_instance_motion_traverse.hpp keeps InstMotionParams in the anonymous namespace)
struct IndexedInstMotionParams : InstMotionParams {
    const uint32_t* order;
    uint32_t num_indices;
};
}  // namespace

// INDEXED only changes how the lane's ray index i is obtained: the launch position itself, or order[position] (positions
// past num_indices and indices >= num_rays: no ray, nothing written).  rays, times, hits, instance_ids and the reload of
// the world ray (trace_instanced_motion's ri) are indexed by i.  The choice stands HERE, under `if constexpr`, not in a
// helper function (DESIGN sections 20 and 32).
template <bool ANY, bool INDEXED>
__global__ __launch_bounds__(kTraceWaves * 64, RT_INSTANCE_MOTION_WAVES)
void instance_motion_query_kernel(std::conditional_t<INDEXED, IndexedInstMotionParams, InstMotionParams> p)
{
    __shared__ uint32_t stack_lds[kTraceWaves][kStackLds][64];
    __shared__ unsigned long long csum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p.counters) {
        if (threadIdx.x < 4) csum[threadIdx.x] = 0ull;
        __syncthreads();
    }
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    if constexpr (INDEXED) i = i < p.num_indices ? p.order[i] : 0xFFFFFFFFull;   // (num_rays is a uint32: never in range)
    const bool in_range = i < p.num_rays;

    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    r.tmin = 0.0f;
    r.tmax = -1.0f;
    float tau = 0.0f;
    if (in_range) {
        load_world_ray(p, i, r);
        r.tmin = p.rays[2 * i].w;
        r.tmax = p.rays[2 * i + 1].w;
        tau = p.times[i];
    }
    // not traced (a miss, no tests): instance_query_kernel's cases, and a time that is NaN or outside [0, 1] (both compares
    // are false for a NaN)
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray && tau >= 0.0f && tau <= 1.0f;

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    Hit h = {0u, 0u, 0.f, 0.f};
    uint32_t hit_inst = RT_MISS;
    const bool hit = trace_instanced_motion<ANY>(p, i, r, tau, h, hit_inst, t, active, steps);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            // the hit instance's BLAS leaves; (u, v) back to the caller's corners as ray_query_kernel does
            const uint32_t b = reinterpret_cast<const uint4*>(p.records + hit_inst)[6].x;
            const rt_triangle_pair* lv = reinterpret_cast<const rt_triangle_pair*>(
                *reinterpret_cast<const uint64_t*>(p.blas_table + b));
            const uint32_t rot = lv[h.tri_id >> 1].rotations[h.tri_id & 1];
            o = hit_record(r.tmax, h.primitive_id, h.bu, h.bv, rot);
        }
        p.hits[i] = o;
        p.instance_ids[i] = hit ? hit_inst : RT_MISS;
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

hipError_t launch_prepare_motion_instances(const rt_motion_instance* instances, uint32_t num_instances,
                                           const rt_accel* blas_table, uint32_t num_blas, rt_triangle* proxies0,
                                           rt_triangle* proxies1, rt_motion_instance_record* records, uint32_t* status,
                                           hipStream_t st)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || num_instances == 0) return e;
    prepare_motion_instances_kernel<<<dim3((num_instances + 255) / 256), dim3(256), 0, st>>>(
        instances, num_instances, blas_table, num_blas, proxies0, proxies1, records, status);
    return hipGetLastError();
}

hipError_t launch_instance_motion_query(const rt_motion_accel& tlas, const rt_motion_instance_record* records,
                                        uint32_t num_instances, const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays,
                                        const float* times, rt_hit* hits, uint32_t* instance_ids, uint32_t num_rays,
                                        const uint32_t* order, uint32_t num_indices, bool any_hit, uint64_t* counters,
                                        hipStream_t st)
{
    IndexedInstMotionParams p;
    p.tlas_nodes0 = tlas.nodes0;
    p.tlas_leaves0 = tlas.triangles0;
    p.tlas_nodes1 = tlas.nodes1;
    p.root = tlas.root;
    p.count = tlas.count;
    p.records = records;
    p.num_instances = num_instances;
    p.num_blas = num_blas;
    p.blas_table = blas_table;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.times = times;
    p.hits = reinterpret_cast<float4*>(hits);
    p.instance_ids = instance_ids;
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.order = order;
    p.num_indices = num_indices;
    const dim3 grid(query_blocks(order ? num_indices : num_rays)), block(kQueryBlock);
    if (order) {
        if (any_hit) instance_motion_query_kernel<true, true><<<grid, block, 0, st>>>(p);
        else instance_motion_query_kernel<false, true><<<grid, block, 0, st>>>(p);
    } else {
        if (any_hit) instance_motion_query_kernel<true, false><<<grid, block, 0, st>>>(p);   // (its InstMotionParams part)
        else instance_motion_query_kernel<false, false><<<grid, block, 0, st>>>(p);
    }
    return hipGetLastError();
}

}  // namespace rt
