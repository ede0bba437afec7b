// sphere_query.hip -- rt_prepare_spheres and rt_intersect_rays_spheres: ray queries over a tree built on spheres (semantics:
// rt_abi.h, sphere block).
//
// prepare_spheres_kernel, one thread per sphere: one 16-byte load, the padded box of the sphere as a proxy triangle (the
// build input of any builder; rt_instance_proxy.hpp's proxy_triangle), an invalid sphere flagged and given the point proxy.
//
// sphere_query_kernel<ANY, INDEXED>: ray_query_kernel's launch shape -- one lane per ray, 64 consecutive rays (or order[]
// entries) per wave, kTraceWaves waves per workgroup, workgroups remapped to XCDs in chunks of 8, the lane-interleaved LDS
// stack with its private spill, counters wave-reduced, added in LDS and published with 4 device atomics per workgroup -- on
// the traversal of rt_sphere_traverse.hpp: the tracer's box phase, a sphere test at the leaf.  A ray is two 16-byte loads,
// a leaf visit two dependent 16-byte loads (the leaf's first quarter for the index, then the sphere), the record one 16-byte
// store.  Lanes past the batch, rays with an empty or NaN [tmin, tmax] and rays with a NaN component trace nothing, as in
// ray_query_kernel.  No pair-prefetch arm, no hold at pop.
// Compiled with -ffp-contract=off: every float operation is the documented one.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_instance_proxy.hpp"
#include "rt_sphere_traverse.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_sphere) == 16 && offsetof(rt_sphere, radius) == 12, "rt_sphere: one 16-byte record (centre, radius)");
static_assert(rt::kQueryBlock == rt::kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

namespace rt {

namespace {

constexpr float kSpherePad = 1.0f / 262144.0f;   // 2^-18 of the box's largest |bound| (rt_abi.h)

// ---------------------------------------------------------------- prepare
__global__ __launch_bounds__(256) void prepare_spheres_kernel(const float4* spheres, uint32_t num_spheres, rt_triangle* proxies,
                                                              uint32_t* status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= num_spheres) return;
    const float4 s = spheres[i];
    const bool valid = __builtin_isfinite(s.x) && __builtin_isfinite(s.y) && __builtin_isfinite(s.z) && s.w >= 0.0f &&
                       s.w < __builtin_inff();
    rt_triangle px = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};   // invalid: a point proxy at the origin
    if (valid) {
        const float c[3] = {s.x, s.y, s.z};
        Box3 bx;
        float e = 0.0f;
        for (int k = 0; k < 3; k++) {
            bx.lo[k] = c[k] - s.w;
            bx.hi[k] = c[k] + s.w;
            e = fmaxf(e, fmaxf(fabsf(bx.lo[k]), fabsf(bx.hi[k])));
        }
        const float pad = e * kSpherePad;
        for (int k = 0; k < 3; k++) { bx.lo[k] = bx.lo[k] - pad; bx.hi[k] = bx.hi[k] + pad; }
        px = proxy_triangle(bx);
    }
    proxies[i] = px;
    if (!valid) atomicOr(status, (uint32_t)RT_SPHERE_BAD);
}

// ---------------------------------------------------------------- query
template <bool ANY, bool INDEXED>
__global__ __launch_bounds__(kTraceWaves * 64, RT_SPHERE_WAVES)
void sphere_query_kernel(SphereParams p)
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
    // not traced (a miss, no tests): as ray_query_kernel
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray;

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    SphereHit h = {0u, 0.f};
    const bool hit = trace_ray_spheres<ANY>(p, r, h, t, active, steps);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) o = float4{r.tmax, __uint_as_float(h.id), h.far_root, 0.f};
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

}  // namespace

hipError_t launch_prepare_spheres(const rt_sphere* spheres, uint32_t num_spheres, rt_triangle* proxies, uint32_t* status,
                                  hipStream_t st)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || num_spheres == 0) return e;
    prepare_spheres_kernel<<<dim3((num_spheres + 255) / 256), dim3(256), 0, st>>>(reinterpret_cast<const float4*>(spheres),
                                                                                  num_spheres, proxies, status);
    return hipGetLastError();
}

hipError_t launch_sphere_query(const rt_accel& as, const rt_sphere* spheres, uint32_t num_spheres, const rt_ray* rays,
                               uint32_t num_rays, const uint32_t* order, uint32_t num_indices, rt_hit* hits, bool any_hit,
                               uint64_t* counters, hipStream_t st)
{
    SphereParams p;
    set_tree(p, as);
    p.spheres = reinterpret_cast<const float4*>(spheres);
    p.num_spheres = num_spheres;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.hits = reinterpret_cast<float4*>(hits);
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.order = order;
    p.num_indices = order ? num_indices : 0u;
    const dim3 grid(query_blocks(order ? num_indices : num_rays)), block(kQueryBlock);
    if (order) {
        if (any_hit) sphere_query_kernel<true, true><<<grid, block, 0, st>>>(p);
        else sphere_query_kernel<false, true><<<grid, block, 0, st>>>(p);
    } else {
        if (any_hit) sphere_query_kernel<true, false><<<grid, block, 0, st>>>(p);
        else sphere_query_kernel<false, false><<<grid, block, 0, st>>>(p);
    }
    return hipGetLastError();
}

}  // namespace rt
