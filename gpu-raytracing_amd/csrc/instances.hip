// instances.hip -- rt_prepare_instances and rt_intersect_rays_instanced: ray queries over placed copies of built trees
// (semantics: rt_abi.h, instancing block).
//
// prepare_instances_kernel, one thread per instance: the world box of the BLAS's root run through object_to_world, the
// padded box as a proxy triangle (the TLAS build input), world_to_object in double.
//
// instance_query_kernel<PF, ANY, FILTERED, INDEXED>: rt_traverse.hpp's wave-level two-phase loop with a second level (trace_instanced,
// rt_instance_traverse.hpp).  One lane per ray, the
// launch geometry, LDS stack, XCD remap and counters of ray_query_kernel.  What the second level adds to a lane:
//   * per-lane node / leaf base pointers: the lanes of one wave sit in different BLASes (and in the TLAS);
//   * TLAS leaves are ordered with the box children: a leaf hit in the TLAS becomes an entry of count 0 (child : 29 | 0,
//     never a box run, whose count is 1..7) that takes part in the nearest-child choice or is pushed like a box child, so
//     the second slot of a TLAS pair is always evaluated in world space before any instance is entered, and nothing of the
//     TLAS is pending while a BLAS is traversed except its stack;
//   * when advance() picks such an entry the lane parks in PH_ENTER; the leaf phase loads the TLAS leaf's instance index,
//     the instance record and the BLAS's rt_accel, transforms the ray, switches the base pointers and remembers the stack
//     depth (base).  BLAS traversal is trace_ray's, with its stack starting at base;
//   * a BLAS whose advance() finds no near child and the stack back at base parks in PH_EXIT; the leaf phase reloads the
//     world ray from the ray array (the original bits), switches back to the TLAS and advances there -- which may enter the
//     next instance in the same leaf phase.
// tmax is shared by both spaces (an affine map preserves t): one closest hit across all instances.
// FILTERED (rt_intersect_rays_instanced_filtered; rt_abi.h, instance-filter block) hands trace_instanced one
// more policy, the lane's InstanceRayFilter (rt_instance_filter.hpp); the unfiltered arms keep their code, instruction for
// instruction:
//   * ray setup: one 16-byte load of the ray's {mask, skip_instance, skip_id} when the caller gave per-ray records;
//   * PH_ENTER: the instance rule comes first -- one 8-byte load of the instance's {mask, flags} (none when the instance has no
//     record), and an instance whose mask misses the ray's is left like a flagged one: no record load, no rt_accel load, the
//     lane advances in the TLAS.  An entered instance sets the lane's per-instance part from the w0 .. w2 rows the kernel has
//     already loaded: the effective cull bits (the 3x3 determinant's sign only when a cull bit is set -- the flags are
//     wave-uniform) and the effective skip id;
//   * leaf test: that per-instance part goes by value to intersect_tri, which asks it after the t window test and before
//     r.tmax = t -- a rejected candidate shrinks no window and ends no any-hit ray.
// INDEXED (rt_intersect_rays_instanced_indexed; rt_abi.h, indexed-instanced block) only changes how the
// lane's ray index is obtained -- order[launch position] -- and so the grid; the ray, its filter record, its two output
// records and the reload of the world ray in PH_EXIT all go by that index.  It combines with FILTERED.
// Compiled with -ffp-contract=off: every float operation is the documented one.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_instance_filter.hpp"
#include "rt_instance_proxy.hpp"
#include "rt_instance_traverse.hpp"
#include "rt_traverse.hpp"

#include <type_traits>

static_assert(sizeof(rt_instance) == 64 && offsetof(rt_instance, blas) == 48, "rt_instance: 3x4 matrix, blas, 3 pads");
static_assert(sizeof(rt_instance_record) == 64 && offsetof(rt_instance_record, blas) == 48 &&
              offsetof(rt_instance_record, flags) == 52, "rt_instance_record: 3x4 matrix, blas, flags, 2 spare");
static_assert(sizeof(rt_accel) == 24, "rt_accel: two pointers, root, count");
static_assert(rt::kQueryBlock == rt::kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

namespace rt {

namespace {

// ---------------------------------------------------------------- prepare
__global__ __launch_bounds__(256) void prepare_instances_kernel(const rt_instance* instances, uint32_t num_instances,
                                                                const rt_accel* blas_table, uint32_t num_blas,
                                                                rt_triangle* proxies, rt_instance_record* records,
                                                                uint32_t* status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= num_instances) return;
    const rt_instance in = instances[i];
    const float* m = in.object_to_world;
    uint32_t flags = 0;

    // the object box: ordered min / max over the non-NONE slots of the root run (rt_instance_proxy.hpp)
    int lo_i[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi_i[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    instance_object_box(blas_table, num_blas, in.blas, lo_i, hi_i, flags);

    // world_to_object in double: adjugate / det of the 3x3 part, translation -W3 * t
    bool finite = true;
    for (int k = 0; k < 12; k++) finite &= __builtin_isfinite(m[k]);
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    float w[12];
    if (!finite || det == 0.0) flags |= RT_INSTANCE_SINGULAR;
    else {
        const double r = 1.0 / det;
        const double inv[9] = {c00 * r, (a02 * a21 - a01 * a22) * r, (a01 * a12 - a02 * a11) * r,
                               c01 * r, (a00 * a22 - a02 * a20) * r, (a02 * a10 - a00 * a12) * r,
                               c02 * r, (a01 * a20 - a00 * a21) * r, (a00 * a11 - a01 * a10) * r};
        const double t0 = m[3], t1 = m[7], t2 = m[11];
        bool fits = true;
        for (int k = 0; k < 3; k++) {
            const double* row = inv + 3 * k;
            const double tr = -(row[0] * t0 + row[1] * t1 + row[2] * t2);
            w[4 * k + 0] = (float)row[0]; w[4 * k + 1] = (float)row[1]; w[4 * k + 2] = (float)row[2]; w[4 * k + 3] = (float)tr;
        }
        for (int k = 0; k < 12; k++) fits &= __builtin_isfinite(w[k]);
        if (!fits) flags |= RT_INSTANCE_SINGULAR;
    }

    rt_instance_record rec;
    for (int k = 0; k < 12; k++) rec.world_to_object[k] = flags ? 0.0f : w[k];
    rec.blas = in.blas;
    rec.flags = flags;
    rec.spare[0] = rec.spare[1] = 0;
    records[i] = rec;

    rt_triangle px = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};   // flagged: a point proxy at the origin
    if (!flags) {
        Affine34 mm;
        for (int k = 0; k < 12; k++) mm.m[k] = m[k];
        px = proxy_triangle(instance_proxy(mm, lo_i, hi_i));   // corners through object_to_world, ordered min / max, the pad
    }
    proxies[i] = px;
    if (flags) atomicOr(status, flags);
}

// ---------------------------------------------------------------- query (the two-level loop: rt_instance_traverse.hpp)

struct FilteredInstParams : InstParams {
    InstanceFilterParams filter;
};

// the index list of the INDEXED arms, appended to either struct (ray_query.hip's IndexedQueryParams: the kernarg offsets of
// the part in front do not move)
template <class Base> struct IndexedParams : Base {
    const uint32_t* order;
    uint32_t num_indices;
};

// ray setup, the two-level traversal, the record and instance id of the hit, the per-workgroup counters.
// INDEXED only changes how the lane's ray index i is obtained: the launch position itself, or order[position] (positions
// past num_indices and indices >= num_rays: no ray, nothing written).  The choice stands HERE, under `if constexpr`, not in
// a helper function (DESIGN sections 20 and 32).
template <bool PF, bool ANY, bool FILTERED, bool INDEXED>
__global__ __launch_bounds__(kTraceWaves * 64, RT_INSTANCE_QUERY_WAVES)
void instance_query_kernel(std::conditional_t<INDEXED,
                                              IndexedParams<std::conditional_t<FILTERED, FilteredInstParams, InstParams>>,
                                              std::conditional_t<FILTERED, FilteredInstParams, InstParams>> p)
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
    if (in_range) {
        load_world_ray(p, i, r);
        r.tmin = p.rays[2 * i].w;
        r.tmax = p.rays[2 * i + 1].w;
    }
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray;

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    Hit h = {0u, 0u, 0.f, 0.f};
    uint32_t hit_inst = RT_MISS;
    // the lane's filter, made HERE under `if constexpr`, not by a helper function (DESIGN sections 20 and 21)
    std::conditional_t<FILTERED, InstanceRayFilter, NoInstanceFilter> flt;
    if constexpr (FILTERED) flt = instance_ray_filter(p.filter, i, in_range);
    const bool hit = trace_instanced<PF, ANY>(p, i, r, h, hit_inst, t, active, steps, flt);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            // the hit instance's BLAS leaves; (u, v) back to the caller's corners as ray_query_kernel does
            const uint32_t b = reinterpret_cast<const uint4*>(p.records + hit_inst)[3].x;
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

}  // namespace

hipError_t launch_prepare_instances(const rt_instance* instances, uint32_t num_instances, const rt_accel* blas_table,
                                    uint32_t num_blas, rt_triangle* proxies, rt_instance_record* records, uint32_t* status,
                                    hipStream_t st)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || num_instances == 0) return e;
    prepare_instances_kernel<<<dim3((num_instances + 255) / 256), dim3(256), 0, st>>>(instances, num_instances, blas_table,
                                                                                      num_blas, proxies, records, status);
    return hipGetLastError();
}

hipError_t launch_instance_query(const InstanceQuery& q, const rt_instance_hit_filter* filter, hipStream_t st)
{
    FilteredInstParams p;
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
    if (filter) p.filter = instance_filter_params(*filter);
    const dim3 grid(query_blocks(q.order ? q.num_indices : q.num_rays)), block(kQueryBlock);
    if (q.order) {
        // the index list goes behind the struct the launched arm takes: one copy of that part of p
        auto indexed = [&](const auto& base) {
            IndexedParams<std::decay_t<decltype(base)>> pi;
            static_cast<std::decay_t<decltype(base)>&>(pi) = base;
            pi.order = q.order;
            pi.num_indices = q.num_indices;
            return pi;
        };
        dispatch_pf_any(q.num_primitives >= kPrefetchMinPrims, q.any_hit, [&](auto pf, auto any) {
            if (filter) instance_query_kernel<pf(), any(), true, true><<<grid, block, 0, st>>>(indexed(p));
            else instance_query_kernel<pf(), any(), false, true><<<grid, block, 0, st>>>(indexed(static_cast<const InstParams&>(p)));
        });
        return hipGetLastError();
    }
    dispatch_pf_any(q.num_primitives >= kPrefetchMinPrims, q.any_hit, [&](auto pf, auto any) {
        if (filter) instance_query_kernel<pf(), any(), true, false><<<grid, block, 0, st>>>(p);
        else instance_query_kernel<pf(), any(), false, false><<<grid, block, 0, st>>>(p);   // (its InstParams part)
    });
    return hipGetLastError();
}

}  // namespace rt
