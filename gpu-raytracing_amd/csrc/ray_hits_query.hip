// ray_hits_query.hip -- rt_ray_hits_count / rt_ray_hits_collect: EVERY triangle a ray crosses inside its [tmin, tmax] window,
// through any tree rt_intersect_rays takes (semantics: rt_abi.h, all-hit block).  The set-valued ray query:
// the result is CSR -- offsets[0..n] by a 64-bit device scan of the per-ray counts, then 16-byte hit records written per ray
// segment.
//
// A ray whose window never shrinks is one more region shape, so ray_hits_kernel<COLLECT> is range_query_kernel's frame with
// the slab test in the place of `keep` and Moller-Trumbore in the place of `match`: one lane per ray, 64 consecutive rays per
// wave, kTraceWaves waves (256 rays) per workgroup, xcd_chunk_block, the ray in two 16-byte loads, a leaf in four 16-byte
// requests, rt_traverse.hpp's wave-level two phases (box steps while enough lanes hold a box run, then one leaf step), exact
// per-workgroup counters.  What it takes from where:
//   * slab() and intersect_tri() are rt_traverse.hpp's, unchanged: a slot is entered iff back >= front && front <= tmax &&
//     back >= tmin with the ray's ORIGINAL tmin / tmax; intersect_tri writes r.tmax on acceptance and the kernel puts the
//     original value back after every test, so no test sees a shrunk window;
//   * nothing is ordered and nothing re-culled: a stack entry is the 4-byte entry alone (a box run child : 29 | count : 3, or
//     a leaf index : 29 | 0), 16 entries in an LDS column per lane (16 KB per workgroup) + 48 private; the first surviving
//     slot of a run is visited next, the others are pushed in slot order.  Both instantiations run this one traversal, so the
//     count and the collect call visit the same leaves in the same order and cannot disagree;
//   * a leaf entry does not carry the slot's count, so triangle B = (v2, v1, v3) is tested iff v3 != v2 bit for bit: a
//     single-triangle record has v3 == v2 (rt_abi.h, refit block) and every builder gives a leaf slot a count >= 1, which makes
//     this trace_ray's rule (count > 0 && v3 != v2) on every record the library writes;
//   * a push onto a full stack of 64 is dropped and flagged (RT_RAY_HITS_STACK_OVERFLOW): the row is then a subset;
//   * COLLECT = false: the lane's count goes through a workgroup scan (rt_csr.hpp: two 21-bit limbs); offsets[i] gets the
//     workgroup-local exclusive prefix and the workgroup's total goes to the scratch; launch_csr_offsets (csr_scan.hip) does
//     the rest, as for the range queries.  Three launches, nothing read back.
//   * COLLECT = true: the lane stores record j < offsets[i+1] - offsets[i] at hits[offsets[i] + j] -- its own segment, in its
//     own traversal order, one 16-byte vector store, no atomics on the output -- and keeps counting beyond the room
//     (counts[i], RT_RAY_HITS_TRUNCATED).  (u, v) go back to the caller's corners as in ray_query_kernel.
// Compiled with -ffp-contract=off and IEEE division: every accepted record is bit for bit the one rt_intersect_rays would
// report for that triangle.
// FILTERED (rt_ray_hits_count_filtered / rt_ray_hits_collect_filtered; rt_abi.h, hit-filter block) is the
// same traversal with the lane's RayFilter (rt_ray_filter.hpp) at the one place where a candidate is accepted; the
// unfiltered arms are the code they were before the filter existed, instruction for instruction.
#include "rt_csr.hpp"
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_ray_filter.hpp"
#include "rt_traverse.hpp"

#include <type_traits>

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 16, "rt_ray: two 16-byte halves; rt_hit: one 16-byte record");

namespace rt {

namespace {

struct RayHitsParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* rays;           // rt_ray = two float4: (origin, tmin), (dir, tmax)
    uint32_t num_rays;
    uint64_t* offsets;            // count: out, workgroup-local prefixes; collect: in
    uint64_t* block_sums;         // count: out, one total per workgroup
    float4* hits;                 // collect: rt_hit = one float4: (t, primitive_id bits, u, v)
    uint32_t* counts;             // collect, optional
    unsigned long long* counters;
    uint32_t* status;
};
struct FilteredRayHitsParams : RayHitsParams {
    FilterParams filter;
};

typedef uint32_t RhSpill[kStackMax - kCsrStackLds];

template <bool COLLECT, bool FILTERED>
__global__ __launch_bounds__(kTraceWaves * 64, RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA)
void ray_hits_kernel(std::conditional_t<FILTERED, FilteredRayHitsParams, RayHitsParams> p)
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
    // not traced (an empty row, no tests), rt_intersect_rays's rule: lanes past the batch, an empty or NaN [tmin, tmax], a NaN
    // origin or direction
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    bool live = in_range && r.tmin <= r.tmax && !nan_ray && p.count > 0;
    // the lane's filter goes to intersect_tri, which asks it after its t window test: a candidate it turns down is not counted,
    // not stored and does not exist for the row.  Made HERE, under `if constexpr`: made by a helper function it costs the
    // unfiltered collect kernel two more spilled registers
    std::conditional_t<FILTERED, RayFilter, NoFilter> flt;
    if constexpr (FILTERED) flt = ray_filter(p.filter, i, in_range);

    // collect: the lane's segment [out, out + room)
    float4* out = nullptr;
    uint32_t room = 0;
    if (COLLECT && in_range) out = csr_segment(p.offsets, p.hits, i, room);

    lds_u32* const col = (lds_u32*)&stack_lds[wave][0][lane];
    RhSpill spill;
    int sp = 0;
    bool overflow = false;            // a push was dropped: the row is a subset
    uint32_t found = 0;               // accepted triangles so far (collect: also beyond the room)
    uint32_t box_tests = 0, tri_tests = 0;
    uint32_t cur = (p.root & kIndexMask) | (p.count << 29);

    auto next_from_stack = [&]() {
        if (sp == 0) { live = false; return; }
        --sp;
        cur = sp < kCsrStackLds ? col[sp * 64] : spill[sp - kCsrStackLds];
    };
    // one triangle (leaf corners c0, c1, c2, rotation rot) against the original window; an accepted one emits its record
    auto test = [&](float c0x, float c0y, float c0z, float c1x, float c1y, float c1z, float c2x, float c2y, float c2z,
                    uint32_t prim, uint32_t rot) {
        Hit h;
        if (!intersect_tri(c0x, c0y, c0z, c1x, c1y, c1z, c2x, c2y, c2z, r, h, 0u, prim, flt)) return;
        const float t = r.tmax;
        r.tmax = tmax0;
        if (COLLECT) {
            if (found < room) out[found] = hit_record(t, prim, h.bu, h.bv, rot);
        }
        found++;
    };
    auto leaf_step = [&]() {
        tri_tests++;
        uint4 l0, l1, l2, l3;
        load_leaf_wide(p.leaves + (cur & kIndexMask), l0, l1, l2, l3);
        test(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
             __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), l0.w, l2.w & 0xFFFFu);
        // triangle B = (v2, v1, v3); for a single triangle v3 == v2 bit for bit and B is skipped (as trace_ray)
        if (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z)
            test(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                 __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                 __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z), l1.w, l2.w >> 16);
        next_from_stack();
    };
    auto box_step = [&]() {
        const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
        uint32_t next = kNoNear;
        for (uint32_t k = 0; k < cnt; k++) {
            const uint4* np = reinterpret_cast<const uint4*>(p.nodes + first + k);
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
        while (true) {                        // box phase: step while enough lanes hold a box run
            stepping = __builtin_amdgcn_ballot_w64(live && (cur >> 29) != 0);
            parked = __builtin_amdgcn_ballot_w64(live && (cur >> 29) == 0);
            if (stepping == 0 || __popcll(stepping) * kParkDen < __popcll(parked) * kParkNum) break;
            if (live && (cur >> 29) != 0) box_step();
        }
        if ((stepping | parked) == 0) break;
        if (live && (cur >> 29) == 0) leaf_step();   // leaf phase: every lane that holds a leaf
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

// the fields both launches fill; the filter part only when there is one
FilteredRayHitsParams hits_params(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                                  uint64_t* counters, uint32_t* status)
{
    FilteredRayHitsParams p = {};
    set_tree(p, as);
    p.rays = reinterpret_cast<const float4*>(rays);
    p.num_rays = num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    if (filter) p.filter = filter_params(*filter);
    return p;
}

}  // namespace

size_t ray_hits_scratch_bytes(uint32_t num_rays) { return csr_scratch_bytes(num_rays); }

hipError_t launch_ray_hits_count(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                                 uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    FilteredRayHitsParams p = hits_params(as, rays, num_rays, filter, counters, status);
    p.offsets = offsets;
    p.block_sums = static_cast<uint64_t*>(scratch);
    const uint32_t blocks = csr_blocks(num_rays);
    if (blocks && filter) ray_hits_kernel<false, true><<<blocks, kCsrBlock, 0, st>>>(p);
    else if (blocks) ray_hits_kernel<false, false><<<blocks, kCsrBlock, 0, st>>>(p);   // (its RayHitsParams part)
    return launch_csr_offsets(offsets, p.block_sums, num_rays, st);
}

hipError_t launch_ray_hits_collect(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                                   const uint64_t* offsets, rt_hit* hits, uint32_t* counts, uint64_t* counters,
                                   uint32_t* status, hipStream_t st)
{
    FilteredRayHitsParams p = hits_params(as, rays, num_rays, filter, counters, status);
    p.offsets = const_cast<uint64_t*>(offsets);   // (the collect instantiation only reads them)
    p.hits = reinterpret_cast<float4*>(hits);
    p.counts = counts;
    if (filter) ray_hits_kernel<true, true><<<csr_blocks(num_rays), kCsrBlock, 0, st>>>(p);
    else ray_hits_kernel<true, false><<<csr_blocks(num_rays), kCsrBlock, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
