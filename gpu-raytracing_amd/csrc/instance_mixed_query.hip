// instance_mixed_query.hip -- rt_intersect_rays_instanced_mixed: the instanced ray query over a BLAS table whose trees hold
// triangles or spheres, the kind told per BLAS by an rt_geometry table (semantics: rt_abi.h, mixed-instancing block; DESIGN
// section 25).
//
// mixed_instance_query_kernel<ANY> is instance_query_kernel<false, ANY, false> (instances.hip) with a kind per entered BLAS:
//   * the same launch shape, LDS stack, XCD remap and counters; a ray is two 16-byte loads;
//   * the traversal is trace_instanced_mixed (rt_instance_mixed_traverse.hpp): TLAS and BLAS box steps are the static
//     ones, entering an instance reads geom_table[blas] after the rt_accel, a BLAS leaf is tested as a triangle pair or as a
//     sphere by the kind of the BLAS the lane is in;
//   * the record of a hit is rt_intersect_rays_instanced's in a triangle BLAS and rt_intersect_rays_spheres's in a sphere
//     BLAS; the kind is re-read from the hit instance's table entry, as instance_query_kernel re-reads the rotation;
//   * lanes past num_rays and rays rt_intersect_rays would not trace trace nothing (a miss, RT_MISS, no tests counted) but
//     still take part in the ballots.
// mixed_instance_query_kernel<ANY, INDEXED, true> is rt_intersect_rays_instanced_mixed_capsules's: capsule BLASes as a third
// kind, launched by that entry point alone.
// No pair-prefetch arm, no hold at pop.
// Compiled with -ffp-contract=off: every float operation is the documented one.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_instance_mixed_traverse.hpp"

#include <type_traits>

static_assert(sizeof(rt_geometry) == 16 && offsetof(rt_geometry, data) == 0 && offsetof(rt_geometry, count) == 8 &&
              offsetof(rt_geometry, kind) == 12, "rt_geometry: one 16-byte record (data, count, kind)");
static_assert(rt::kQueryBlock == rt::kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

namespace rt {

namespace {

// rt_intersect_rays_instanced_mixed_indexed: the same query through an index list (ray_query.hip's IndexedQueryParams: the
// plain part's kernarg offsets do not move)
struct IndexedMixedInstParams : MixedInstParams {
    const uint32_t* order;
    uint32_t num_indices;
};

// INDEXED only changes how the lane's ray index i is obtained: the launch position itself, or order[position] (positions
// past num_indices and indices >= num_rays: no ray, nothing written).  rays, hits, instance_ids and the reload of the world
// ray (trace_instanced_mixed's ri) are indexed by i.  The choice stands HERE, under `if constexpr`, not in a helper function
// (DESIGN sections 20 and 32).
// CAPS (rt_intersect_rays_instanced_mixed_capsules): trace_instanced_mixed's capsule arm, a register bound
// of its own and the capsule record at the write-out; the four <ANY, INDEXED, false> kernels are the ones from before the arm.
template <bool ANY, bool INDEXED, bool CAPS = false>
__global__ __launch_bounds__(kTraceWaves * 64, CAPS ? RT_INSTANCE_MIXED_CAPSULE_WAVES : RT_INSTANCE_MIXED_WAVES)
void mixed_instance_query_kernel(std::conditional_t<INDEXED, IndexedMixedInstParams, MixedInstParams> p)
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
    const bool hit = trace_instanced_mixed<ANY, CAPS>(p, i, r, h, hit_inst, t, active, steps);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            // the hit instance's BLAS and its kind: a sphere record as sphere_query_kernel writes it, or (u, v) back to the
            // caller's corners through the BLAS's leaves as instance_query_kernel does
            const uint32_t b = reinterpret_cast<const uint4*>(p.records + hit_inst)[3].x;
            const uint32_t kind = reinterpret_cast<const uint4*>(p.geom_table + b)[0].w;
            bool tri_rec = kind != RT_GEOM_SPHERES;
            if constexpr (CAPS) {   // a capsule record as capsule_query_kernel writes it
                tri_rec = kind == RT_GEOM_TRIANGLES;
                if (kind == RT_GEOM_CAPSULES) o = float4{r.tmax, __uint_as_float(h.primitive_id), h.bu, h.bv};
            }
            if (kind == RT_GEOM_SPHERES) {
                o = float4{r.tmax, __uint_as_float(h.primitive_id), h.bu, 0.f};
            } else if (tri_rec) {
                const rt_triangle_pair* lv = reinterpret_cast<const rt_triangle_pair*>(
                    *reinterpret_cast<const uint64_t*>(p.blas_table + b));
                const uint32_t rot = lv[h.tri_id >> 1].rotations[h.tri_id & 1];
                o = hit_record(r.tmax, h.primitive_id, h.bu, h.bv, rot);
            }
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

hipError_t launch_instance_mixed_query(const InstanceQuery& q, const rt_geometry* geom_table, bool capsules, hipStream_t st)
{
    IndexedMixedInstParams p;
    p.tlas_nodes = q.tlas.nodes;
    p.tlas_leaves = q.tlas.triangles;
    p.root = q.tlas.root;
    p.count = q.tlas.count;
    p.records = q.records;
    p.num_instances = q.num_instances;
    p.num_blas = q.num_blas;
    p.blas_table = q.blas_table;
    p.geom_table = geom_table;
    p.rays = reinterpret_cast<const float4*>(q.rays);
    p.hits = reinterpret_cast<float4*>(q.hits);
    p.instance_ids = q.instance_ids;
    p.num_rays = q.num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(q.counters);
    p.order = q.order;
    p.num_indices = q.num_indices;
    const dim3 grid(query_blocks(q.order ? q.num_indices : q.num_rays)), block(kQueryBlock);
    if (capsules) {   // the CAPS kernels: rt_intersect_rays_instanced_mixed_capsules alone
        if (q.order) {
            if (q.any_hit) mixed_instance_query_kernel<true, true, true><<<grid, block, 0, st>>>(p);
            else mixed_instance_query_kernel<false, true, true><<<grid, block, 0, st>>>(p);
        } else {
            if (q.any_hit) mixed_instance_query_kernel<true, false, true><<<grid, block, 0, st>>>(p);
            else mixed_instance_query_kernel<false, false, true><<<grid, block, 0, st>>>(p);
        }
    } else if (q.order) {
        if (q.any_hit) mixed_instance_query_kernel<true, true><<<grid, block, 0, st>>>(p);
        else mixed_instance_query_kernel<false, true><<<grid, block, 0, st>>>(p);
    } else {
        if (q.any_hit) mixed_instance_query_kernel<true, false><<<grid, block, 0, st>>>(p);   // (its MixedInstParams part)
        else mixed_instance_query_kernel<false, false><<<grid, block, 0, st>>>(p);
    }
    return hipGetLastError();
}

}  // namespace rt
