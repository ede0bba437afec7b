// ray_hits_instanced_query.hip -- rt_ray_hits_count_instanced / rt_ray_hits_collect_instanced: EVERY triangle a ray crosses
// inside its [tmin, tmax] window in a scene of placed copies of built trees, each record with the instance it lies in
// (semantics: rt_abi.h, instanced all-hit block).  The set-valued form of rt_intersect_rays_instanced: the
// result is CSR -- offsets[0..n] by the 64-bit device scan of the per-ray counts, then a 16-byte hit record and a 4-byte
// instance id per crossing, both written at the ray's segment.
//
// ray_hits_instanced_kernel<COLLECT> is ray_hits_kernel's frame (ray_hits_query.hip) with trace_instanced's second level
// (rt_instance_traverse.hpp) written into its loop.  From ray_hits_kernel: one lane per ray, 256 rays per workgroup,
// xcd_chunk_block, the 4-byte unordered stack (kCsrStackLds entries in an LDS column per lane, the rest private), "the first
// surviving slot is visited next, the others are pushed in slot order", the wave-level two phases, the workgroup scan of the
// counts and launch_csr_offsets, exact per-workgroup counters, the ballot-ORed status word.  From trace_instanced: per-lane
// node and leaf base pointers, `inst` (kTop in the TLAS), `base` (the stack depth at which the lane entered its BLAS), the
// record load and load_accel, the enter arithmetic, load_world_ray on exit.  What the two make together:
//   * an entry of count 0 means two things: while the lane is in the TLAS it is a TLAS leaf -- an instance to enter --, inside
//     a BLAS it is a leaf record to test.  Either way it parks the lane for the leaf phase, as does a BLAS whose stack is back
//     at `base` (leaving).  The leaf phase runs, in this order, the lane's BLAS leaf, its exit, and its entry: a lane that
//     leaves an instance may enter the next one in the same phase;
//   * the window never moves: every slab test of both levels and every triangle test sees the ray's original tmin / tmax
//     (intersect_tri writes r.tmax on acceptance; the kernel puts it back), so whether a slot or an instance is entered does
//     not depend on what was visited before it.  The row is a function of the bytes and the ray; the count and the collect
//     instantiation run this one traversal and cannot disagree;
//   * one stack of 64 for both levels: a BLAS entered at depth k pushes at k .. 63 and leaves when its pops reach k again.  A
//     push onto a full stack is dropped and flagged (RT_RAY_HITS_STACK_OVERFLOW): the row is then a subset;
//   * COLLECT: record j < room goes to hits[offsets[i] + j] and its instance to instance_ids[offsets[i] + j].
// FILTERED (rt_ray_hits_count_instanced_filtered / rt_ray_hits_collect_instanced_filtered; rt_abi.h, instanced set-filter block;
// DESIGN section 31) is the same traversal with the lane's InstanceRayFilter (rt_instance_filter.hpp): enter(id) is asked at the
// TLAS leaf before the record is read, set_instance once the rows are in registers, and `tri` is intersect_tri's policy at its
// one acceptance point.  The window does not move, so the filtered row is the unfiltered one less what the two rules reject.
// No pair-prefetch arm.  Compiled with -ffp-contract=off and IEEE division: inside an instance every record is
// bit for bit rt_ray_hits_collect's for the object ray, which is rt_intersect_rays_instanced's object ray.
#include "rt_csr.hpp"
#include "rt_device.hpp"
#include "rt_instance_filter.hpp"
#include "rt_instance_traverse.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

#include <type_traits>

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 16, "rt_ray: two 16-byte halves; rt_hit: one 16-byte record");
static_assert(sizeof(rt_instance_record) == 64 && sizeof(rt_accel) == 24, "the record and table entry trace_instanced loads");

// the launch bounds of the FILTERED arms (below), overridable for the bound sweep of tools/instance_set_filter_bench.py.
// Count: 7 (71 VGPRs, 40 spilled) measured 5 to 7 % faster on an MI355X than 6 in every cell, and faster than 5 and 8.
// Collect: 6 (80 VGPRs, 37 spilled) measured faster than 5 in three of four cells and than 4 in all
#ifndef RT_RAY_HITS_INSTANCED_COUNT_FILTERED_WAVES
#define RT_RAY_HITS_INSTANCED_COUNT_FILTERED_WAVES 7
#endif
#ifndef RT_RAY_HITS_INSTANCED_COLLECT_FILTERED_WAVES
#define RT_RAY_HITS_INSTANCED_COLLECT_FILTERED_WAVES 6
#endif

namespace rt {

namespace {

// waves per SIMD the register allocation of each instantiation must fit: the largest at which it keeps every value in
// registers.  Count: 6 (80 VGPRs, no spill; at 7 it spills 18).  Collect: 5 (96 VGPRs, no spill; at 6 it spills 30 inside the
// loop and measured 3 % slower on the SAH trees, no faster on the LBVH ones).  DESIGN section 29 has the table and the runs.
constexpr int kRayHitsInstancedCountWaves = 6, kRayHitsInstancedCollectWaves = 5;
// the FILTERED arms keep six more values live per lane (mask, skip_instance, skip_id, inst_flags, tri.cull, tri.skip) and spill
// at the siblings' bounds: their own, measured ones (above)
constexpr int kRayHitsInstancedCountFilteredWaves = RT_RAY_HITS_INSTANCED_COUNT_FILTERED_WAVES,
              kRayHitsInstancedCollectFilteredWaves = RT_RAY_HITS_INSTANCED_COLLECT_FILTERED_WAVES;
constexpr int ray_hits_instanced_waves(bool collect, bool filtered)
{
    return collect ? (filtered ? kRayHitsInstancedCollectFilteredWaves : kRayHitsInstancedCollectWaves)
                   : (filtered ? kRayHitsInstancedCountFilteredWaves : kRayHitsInstancedCountWaves);
}

// InstParams's fields as trace_instanced reads them (hits: rt_hit as one float4; instance_ids: parallel to hits), and the CSR part
struct RayHitsInstParams : InstParams {
    uint64_t* offsets;            // count: out, workgroup-local prefixes; collect: in
    uint64_t* block_sums;         // count: out, one total per workgroup
    uint32_t* counts;             // collect, optional
    uint32_t* status;
};
struct FilteredRayHitsInstParams : RayHitsInstParams {
    InstanceFilterParams filter;
};

typedef uint32_t RhiSpill[kStackMax - kCsrStackLds];

template <bool COLLECT, bool FILTERED>
__global__ __launch_bounds__(kTraceWaves * 64, ray_hits_instanced_waves(COLLECT, FILTERED))
void ray_hits_instanced_kernel(std::conditional_t<FILTERED, FilteredRayHitsInstParams, RayHitsInstParams> p)
{
    __shared__ uint32_t stack_lds[kTraceWaves][kCsrStackLds][64];
    __shared__ unsigned long long csum[2];
    __shared__ uint32_t ws[kTraceWaves + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_rays;
    if (p.counters && threadIdx.x < 2) csum[threadIdx.x] = 0ull;   // (kernel argument: the same for every thread)

    float4 ra = {0.f, 0.f, 0.f, 0.f}, rb = {0.f, 0.f, 0.f, -1.f};
    if (in_range) { ra = p.rays[2 * i]; rb = p.rays[2 * i + 1]; }
    Ray r;
    r.ox = ra.x; r.oy = ra.y; r.oz = ra.z; r.tmin = ra.w;
    r.dx = rb.x; r.dy = rb.y; r.dz = rb.z; r.tmax = rb.w;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    const float tmax0 = r.tmax;       // the window never shrinks: put back after every triangle test
    // not traced (an empty row, no tests), the all-hit rule: lanes past the batch, an empty or NaN [tmin, tmax], a NaN origin or
    // direction
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    bool live = in_range && r.tmin <= r.tmax && !nan_ray && p.count > 0;

    // collect: the lane's segment [out, out + room) of the records, and of the ids beside them
    float4* out = nullptr;
    uint32_t* out_ids = nullptr;
    uint32_t room = 0;
    if (COLLECT && in_range) {
        out = csr_segment(p.offsets, p.hits, i, room);
        out_ids = p.instance_ids + (out - p.hits);
    }

    lds_u32* const col = (lds_u32*)&stack_lds[wave][0][lane];
    RhiSpill spill;
    int sp = 0;
    bool overflow = false;            // a push was dropped: the row is a subset
    uint32_t found = 0;               // accepted triangles so far (collect: also beyond the room)
    uint32_t box_tests = 0, tri_tests = 0;
    uint32_t cur = (p.root & kIndexMask) | (p.count << 29);
    // the second level: the lane's own node and leaf arrays, its instance (kTop: in the TLAS) and its BLAS's stack bottom
    const rt_node* nodes = p.tlas_nodes;
    const rt_triangle_pair* leaves = p.tlas_leaves;
    uint32_t inst = kTop;
    int base = 0;
    bool leaving = false;             // the BLAS's part of the stack is used up: parked until the leaf phase takes the lane out
    // the lane's filter, made HERE under `if constexpr`, not by a helper function (DESIGN sections 20 and 21)
    std::conditional_t<FILTERED, InstanceRayFilter, NoInstanceFilter> flt;
    if constexpr (FILTERED) flt = instance_ray_filter(p.filter, i, in_range);

    auto next_from_stack = [&]() {
        if (sp == base) {
            if (inst == kTop) live = false;
            else leaving = true;
            return;
        }
        --sp;
        cur = sp < kCsrStackLds ? col[sp * 64] : spill[sp - kCsrStackLds];
    };
    // one triangle (leaf corners c0, c1, c2, rotation rot) against the original window; an accepted one emits its record
    auto test = [&](float c0x, float c0y, float c0z, float c1x, float c1y, float c1z, float c2x, float c2y, float c2z,
                    uint32_t prim, uint32_t rot) {
        Hit h;
        if constexpr (FILTERED) {
            if (!intersect_tri(c0x, c0y, c0z, c1x, c1y, c1z, c2x, c2y, c2z, r, h, 0u, prim, flt.tri)) return;
        } else {
            if (!intersect_tri(c0x, c0y, c0z, c1x, c1y, c1z, c2x, c2y, c2z, r, h, 0u, prim)) return;
        }
        const float t = r.tmax;
        r.tmax = tmax0;
        if (COLLECT) {
            if (found < room) {
                out[found] = hit_record(t, prim, h.bu, h.bv, rot);
                out_ids[found] = inst;
            }
        }
        found++;
    };
    auto leaf_step = [&]() {
        tri_tests++;
        uint4 l0, l1, l2, l3;
        load_leaf_wide(leaves + (cur & kIndexMask), l0, l1, l2, l3);
        test(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
             __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), l0.w, l2.w & 0xFFFFu);
        // triangle B = (v2, v1, v3); for a single triangle v3 == v2 bit for bit and B is skipped (as ray_hits_kernel)
        if (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z)
            test(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                 __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                 __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z), l1.w, l2.w >> 16);
        next_from_stack();
    };
    // a run of the lane's current tree.  In the TLAS a triangle slot that passes is an instance entry (leaf index : 29 | 0)
    auto box_step = [&]() {
        const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
        uint32_t next = kNoNear;
        for (uint32_t k = 0; k < cnt; k++) {
            const uint4* np = reinterpret_cast<const uint4*>(nodes + first + k);
            const uint4 a = np[0], b = np[1];
            const uint32_t type = b.w >> 29;
            if (type == RT_CHILD_NONE) continue;
            box_tests++;
            const uint32_t e = slot_entry(a, b);
            float front, back;
            slab(a, b, r, front, back);
            const bool in = (back >= front) & (front <= tmax0) & (back >= r.tmin);
            if (!in || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // missed by the ray, or an empty run
            if (next == kNoNear) { next = e; continue; }   // the first survivor is visited next, the others wait
            if (sp < kCsrStackLds) col[sp * 64] = e;
            else if (sp < kStackMax) spill[sp - kCsrStackLds] = e;
            else overflow = true;             // dropped: what lies below it is missing from the row
            sp = min(sp + 1, kStackMax);
        }
        if (next != kNoNear) cur = next;
        else next_from_stack();
    };

    while (true) {
        uint64_t stepping, parked;
        while (true) {                        // box phase (both levels): step while enough lanes hold a box run
            const bool box = live && !leaving && (cur >> 29) != 0;
            stepping = __builtin_amdgcn_ballot_w64(box);
            parked = __builtin_amdgcn_ballot_w64(live && !box);
            if (stepping == 0 || __popcll(stepping) * kParkDen < __popcll(parked) * kParkNum) break;
            if (box) box_step();
        }
        if ((stepping | parked) == 0) break;
        // leaf phase: every lane that holds a BLAS leaf, is leaving its BLAS, or holds an instance to enter
        if (live && (leaving || (cur >> 29) == 0)) {
            if (inst != kTop && !leaving) leaf_step();
            if (leaving) {                    // the BLAS is done: back to the world ray (its original bits) and the TLAS
                load_world_ray(p, i, r);
                nodes = p.tlas_nodes;
                leaves = p.tlas_leaves;
                inst = kTop;
                base = 0;
                leaving = false;
                next_from_stack();
            }
            if (live && inst == kTop && (cur >> 29) == 0) {   // a TLAS leaf: enter its instance, or go on in the TLAS
                const uint32_t id = reinterpret_cast<const uint4*>(p.tlas_leaves + (cur & kIndexMask))[0].w;
                bool ok = id < p.num_instances;
                uint32_t nroot = 0, ncount = 0;
                uint64_t ntris = 0, nnodes = 0;
                float4 w0, w1, w2;
                if constexpr (FILTERED) {
                    if (ok) ok = flt.enter(id);   // the instance rule: asked first, a masked-out instance makes no further load
                }
                if (ok) {
                    const float4* rec = reinterpret_cast<const float4*>(p.records + id);
                    w0 = rec[0]; w1 = rec[1]; w2 = rec[2];
                    const uint4 tail = reinterpret_cast<const uint4*>(rec)[3];   // blas, flags, spare
                    ok = (tail.y == 0u) & (tail.x < p.num_blas);
                    if (ok) {
                        load_accel(p.blas_table, tail.x, ntris, nnodes, nroot, ncount);
                        ok = (ncount - 1u) < 7u;
                    }
                }
                if (ok) {
                    const float ox = r.ox, oy = r.oy, oz = r.oz, dx = r.dx, dy = r.dy, dz = r.dz;
                    r.ox = ((w0.x * ox + w0.y * oy) + w0.z * oz) + w0.w;
                    r.oy = ((w1.x * ox + w1.y * oy) + w1.z * oz) + w1.w;
                    r.oz = ((w2.x * ox + w2.y * oy) + w2.z * oz) + w2.w;
                    r.dx = (w0.x * dx + w0.y * dy) + w0.z * dz;
                    r.dy = (w1.x * dx + w1.y * dy) + w1.z * dz;
                    r.dz = (w2.x * dx + w2.y * dy) + w2.z * dz;
                    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
                    nodes = reinterpret_cast<const rt_node*>(nnodes);
                    leaves = reinterpret_cast<const rt_triangle_pair*>(ntris);
                    inst = id;
                    base = sp;
                    cur = (nroot & kIndexMask) | (ncount << 29);
                    if constexpr (FILTERED) flt.set_instance(id, w0, w1, w2);
                } else {
                    next_from_stack();
                }
            }
        }
    }

    uint32_t flags = overflow ? (uint32_t)RT_RAY_HITS_STACK_OVERFLOW : 0u;
    if (COLLECT) {
        if (in_range && p.counts) p.counts[i] = found;
        if (found > room) flags |= (uint32_t)RT_RAY_HITS_TRUNCATED;
    } else {
        // the workgroup's exclusive scan of the counts (a count is below 2^32: two 21-bit limbs); lanes past the batch add 0
        uint64_t total;
        const uint64_t ex = block_excl_scan_u64<kTraceWaves * 64, 2>(found, ws, &total);
        if (in_range) p.offsets[i] = ex;
        if (threadIdx.x == 0) p.block_sums[vb] = total;
    }
    if (p.status) {
        const bool any_over = __builtin_amdgcn_ballot_w64((flags & RT_RAY_HITS_STACK_OVERFLOW) != 0) != 0;
        const bool any_trunc = __builtin_amdgcn_ballot_w64((flags & RT_RAY_HITS_TRUNCATED) != 0) != 0;
        const uint32_t wf = (any_over ? (uint32_t)RT_RAY_HITS_STACK_OVERFLOW : 0u) |
                            (any_trunc ? (uint32_t)RT_RAY_HITS_TRUNCATED : 0u);
        if (wf && lane == 0) atomicOr(p.status, wf);
    }
    if (p.counters) {
        const uint32_t bsum = wave_sum_u32(box_tests), tsum = wave_sum_u32(tri_tests);
        __syncthreads();                      // csum's zeroes
        if (lane == 0) {
            atomicAdd(&csum[0], (unsigned long long)bsum);
            atomicAdd(&csum[1], (unsigned long long)tsum);
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const unsigned long long v = csum[threadIdx.x];
            if (v) atomicAdd(&p.counters[threadIdx.x], v);
        }
    }
}

// the fields both launches fill (filter: null for the unfiltered kernels, which are handed the RayHitsInstParams part)
FilteredRayHitsInstParams hits_instanced_params(const InstanceQuery& q, const rt_instance_hit_filter* filter, uint32_t* status)
{
    FilteredRayHitsInstParams p = {};
    if (filter) p.filter = instance_filter_params(*filter);
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
    p.status = status;
    return p;
}

}  // namespace

hipError_t launch_ray_hits_count_instanced(const InstanceQuery& q, const rt_instance_hit_filter* filter, uint64_t* offsets,
                                           void* scratch, uint32_t* status, hipStream_t st)
{
    FilteredRayHitsInstParams p = hits_instanced_params(q, filter, status);
    p.offsets = offsets;
    p.block_sums = static_cast<uint64_t*>(scratch);
    const uint32_t blocks = csr_blocks(q.num_rays);
    if (blocks) {
        if (filter) ray_hits_instanced_kernel<false, true><<<blocks, kCsrBlock, 0, st>>>(p);
        else ray_hits_instanced_kernel<false, false><<<blocks, kCsrBlock, 0, st>>>(p);   // (its RayHitsInstParams part)
    }
    return launch_csr_offsets(offsets, p.block_sums, q.num_rays, st);
}

hipError_t launch_ray_hits_collect_instanced(const InstanceQuery& q, const rt_instance_hit_filter* filter,
                                             const uint64_t* offsets, uint32_t* counts, uint32_t* status, hipStream_t st)
{
    FilteredRayHitsInstParams p = hits_instanced_params(q, filter, status);
    p.offsets = const_cast<uint64_t*>(offsets);   // (the collect instantiation only reads them)
    p.counts = counts;
    if (filter) ray_hits_instanced_kernel<true, true><<<csr_blocks(q.num_rays), kCsrBlock, 0, st>>>(p);
    else ray_hits_instanced_kernel<true, false><<<csr_blocks(q.num_rays), kCsrBlock, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
