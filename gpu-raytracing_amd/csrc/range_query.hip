// range_query.hip -- rt_range_count / rt_range_collect: every triangle within a radius of a point (RT_RANGE_SPHERE) or whose
// vertex box overlaps a box (RT_RANGE_BOX), through any tree rt_intersect_rays takes (semantics: rt_abi.h, range-query block;
// DESIGN section 13).  The library's first query with a data-dependent output length: the result is CSR -- offsets[0..n] by a
// 64-bit device scan of the per-query counts, then ids written per query segment.
//
// range_query_kernel<SHAPE, COLLECT> keeps the frame of point_query_kernel: one lane per query, 64 consecutive queries per
// wave, kTraceWaves waves (256 queries) per workgroup, xcd_chunk_block, the query in one (sphere) or two (box) 16-byte
// loads, a leaf in four 16-byte requests, rt_traverse.hpp's wave-level two phases (box steps while enough lanes hold a box
// run, then one leaf step), exact per-workgroup counters.  What differs from the point query:
//   * the region never shrinks, so nothing is ordered and nothing re-culled: a stack entry is the 4-byte entry alone (a box
//     run child : 29 | count : 3, or a leaf index : 29 | 0), 16 entries in an LDS column per lane (16 KB per workgroup) + 48
//     private; the first surviving slot of a run is visited next, the others are pushed in slot order;
//   * a slot is skipped iff its box fails the shape's test (sphere: boxdist2 > dist2_max; box: the closed overlap test), a
//     triangle matches by the exact predicate of the header; both instantiations of a shape run this one traversal, so the
//     count and the collect call visit the same leaves in the same order and cannot disagree;
//   * a push onto a full stack of 64 is dropped and flagged (RT_RANGE_STACK_OVERFLOW): the result is then a subset;
//   * COLLECT = false: the lane's match count goes through a workgroup scan (rt_csr.hpp: two 21-bit limbs); offsets[i] gets
//     the workgroup-local exclusive prefix and the workgroup's total goes to the scratch.  launch_csr_offsets (csr_scan.hip)
//     turns the totals into exclusive prefixes, writes offsets[n] and adds each workgroup's prefix to its 256 offsets.  Three
//     launches, nothing read back;
//   * COLLECT = true: the lane stores match j < offsets[i+1] - offsets[i] at ids[offsets[i] + j] -- its own segment, in its
//     own traversal order, plain 4-byte vector stores, no atomics on the output -- and keeps counting beyond the room
//     (counts[i], RT_RANGE_TRUNCATED).
// d2, the corner un-rotation, boxdist2 and slot_entry live in rt_point_math.hpp (shared with the point queries); the workgroup
// geometry, the limb scan and the segment prologue in rt_csr.hpp (shared with ray_hits_query.hip and tri_overlap_query.hip),
// as does the epilogue csr_finish (shared with tri_overlap_query.hip).
// Compiled with -ffp-contract=off and IEEE division: every float operation is the one rt_abi.h writes down.
#include "rt_csr.hpp"
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_range_box) == 32 && offsetof(rt_range_box, hi) == 16, "rt_range_box: two 16-byte halves (lo | hi)");
static_assert(sizeof(rt_point_query) == 16, "rt_point_query: one 16-byte record");

namespace rt {

namespace {

struct RangeParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* queries;        // sphere: (p, dist2_max); box: (lo, -), (hi, -)
    uint32_t num_queries;
    uint64_t* offsets;            // count: out, workgroup-local prefixes; collect: in
    uint64_t* block_sums;         // count: out, one total per workgroup
    uint32_t* ids;                // collect
    uint32_t* counts;             // collect, optional
    unsigned long long* counters;
    uint32_t* status;
};

// the query region, per shape: keep(slot box) and match(triangle).  SPHERE holds (p, dist2_max), BOX holds (lo, hi).
template <int SHAPE> struct Region;
template <> struct Region<RT_RANGE_SPHERE> {
    float px, py, pz, r;
    __device__ __forceinline__ bool load(const float4* q, uint64_t i)
    {
        const float4 v = q[i];
        px = v.x; py = v.y; pz = v.z; r = v.w;
        // not traced: a non-finite p, a NaN or negative dist2_max  (r >= 0 is false for NaN)
        return __builtin_isfinite(px) & __builtin_isfinite(py) & __builtin_isfinite(pz) & (r >= 0.0f);
    }
    __device__ __forceinline__ bool keep(const uint4& a, const uint4& b) const { return !(box_d2(a, b, px, py, pz) > r); }
    // the caller's corners in the caller's order: (s0, s1, s2) stored with rotation rot
    __device__ __forceinline__ bool match(float s0x, float s0y, float s0z, float s1x, float s1y, float s1z, float s2x, float s2y,
                                          float s2z, uint32_t rot) const
    {
        return range_tri_d2(px, py, pz, unrotate(s0x, s0y, s0z, s1x, s1y, s1z, s2x, s2y, s2z, rot)) <= r;
    }
};
template <> struct Region<RT_RANGE_BOX> {
    float lx, ly, lz, hx, hy, hz;
    __device__ __forceinline__ bool load(const float4* q, uint64_t i)
    {
        const float4 l = q[2 * i], h = q[2 * i + 1];
        lx = l.x; ly = l.y; lz = l.z; hx = h.x; hy = h.y; hz = h.z;
        // not traced: a NaN component, or lo > hi on an axis  (lo <= hi is false for NaN)
        return (lx <= hx) & (ly <= hy) & (lz <= hz);
    }
    // closed overlap on every axis: tlo <= hi && thi >= lo
    __device__ __forceinline__ bool over(float tlx, float tly, float tlz, float thx, float thy, float thz) const
    {
        return (tlx <= hx) & (tly <= hy) & (tlz <= hz) & (thx >= lx) & (thy >= ly) & (thz >= lz);
    }
    __device__ __forceinline__ bool keep(const uint4& a, const uint4& b) const
    {
        return over(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(b.x), __uint_as_float(b.y),
                    __uint_as_float(b.z));
    }
    // fminf / fmaxf of the three corners do not depend on their order (a -0 / +0 pick compares equal): no unrotate
    __device__ __forceinline__ bool match(float s0x, float s0y, float s0z, float s1x, float s1y, float s1z, float s2x, float s2y,
                                          float s2z, uint32_t) const
    {
        return over(fminf(fminf(s0x, s1x), s2x), fminf(fminf(s0y, s1y), s2y), fminf(fminf(s0z, s1z), s2z),
                    fmaxf(fmaxf(s0x, s1x), s2x), fmaxf(fmaxf(s0y, s1y), s2y), fmaxf(fmaxf(s0z, s1z), s2z));
    }
};

typedef uint32_t RgSpill[kStackMax - kCsrStackLds];

template <int SHAPE, bool COLLECT>
__global__ __launch_bounds__(kTraceWaves * 64, RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA) void range_query_kernel(RangeParams p)
{
    __shared__ uint32_t stack_lds[kTraceWaves][kCsrStackLds][64];
    __shared__ unsigned long long csum[2];
    __shared__ uint32_t ws[kTraceWaves + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_queries;
    if (p.counters && threadIdx.x < 2) csum[threadIdx.x] = 0ull;   // (kernel argument: the same for every thread)

    Region<SHAPE> rg = {};
    bool live = false;
    if (in_range) live = rg.load(p.queries, i) && p.count > 0;

    // collect: the lane's segment [out, out + room)
    uint32_t* out = nullptr;
    uint32_t room = 0;
    if (COLLECT && in_range) out = csr_segment(p.offsets, p.ids, i, room);

    lds_u32* const col = (lds_u32*)&stack_lds[wave][0][lane];
    RgSpill spill;
    int sp = 0;
    bool overflow = false;            // a push was dropped: the result is a subset
    uint32_t found = 0;               // matches so far (collect: also beyond the room)
    uint32_t box_tests = 0, tri_tests = 0;
    uint32_t cur = (p.root & kIndexMask) | (p.count << 29);

    auto next_from_stack = [&]() {
        if (sp == 0) { live = false; return; }
        --sp;
        cur = sp < kCsrStackLds ? col[sp * 64] : spill[sp - kCsrStackLds];
    };
    auto emit = [&](uint32_t id) {
        if (COLLECT) {
            if (found < room) out[found] = id;
        }
        found++;
    };
    auto leaf_step = [&]() {
        tri_tests++;
        uint4 l0, l1, l2, l3;
        load_leaf_wide(p.leaves + (cur & kIndexMask), l0, l1, l2, l3);
        if (rg.match(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
                     __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                     __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), l2.w & 0xFFFFu))
            emit(l0.w);
        if (l1.w == l0.w + 1u) {              // a pair record: B = (v2, v1, v3) with rotations[1]
            if (rg.match(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                         __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                         __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z), l2.w >> 16))
                emit(l1.w);
        }
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
            if (!rg.keep(a, b) || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // outside the region, or an empty run
            if (next == kNoNear) { next = e; continue; }   // the first survivor is visited next, the others wait
            if (sp < kCsrStackLds) col[sp * 64] = e;
            else if (sp < kStackMax) spill[sp - kCsrStackLds] = e;
            else overflow = true;             // dropped: what lies below it is missing from the result
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

    csr_finish<COLLECT, RT_RANGE_STACK_OVERFLOW, RT_RANGE_TRUNCATED>(
        in_range, i, vb, lane, overflow, found, room, box_tests, tri_tests, p.offsets, p.block_sums, p.counts, p.status,
        p.counters, ws, csum);
}

RangeParams range_params(const rt_accel& as, const void* queries, uint32_t num_queries, uint64_t* counters, uint32_t* status)
{
    RangeParams p = {};
    set_tree(p, as);
    p.queries = reinterpret_cast<const float4*>(queries);
    p.num_queries = num_queries;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    return p;
}

}  // namespace

size_t range_scratch_bytes(uint32_t num_queries) { return csr_scratch_bytes(num_queries); }

hipError_t launch_range_count(const rt_accel& as, const void* queries, uint32_t num_queries, int shape, uint64_t* offsets,
                              void* scratch, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    RangeParams p = range_params(as, queries, num_queries, counters, status);
    p.offsets = offsets;
    p.block_sums = static_cast<uint64_t*>(scratch);
    const uint32_t blocks = csr_blocks(num_queries);
    if (blocks) {
        if (shape == RT_RANGE_SPHERE) range_query_kernel<RT_RANGE_SPHERE, false><<<blocks, kCsrBlock, 0, st>>>(p);
        else range_query_kernel<RT_RANGE_BOX, false><<<blocks, kCsrBlock, 0, st>>>(p);
    }
    return launch_csr_offsets(offsets, p.block_sums, num_queries, st);
}

hipError_t launch_range_collect(const rt_accel& as, const void* queries, uint32_t num_queries, int shape, const uint64_t* offsets,
                                uint32_t* ids, uint32_t* counts, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    RangeParams p = range_params(as, queries, num_queries, counters, status);
    p.offsets = const_cast<uint64_t*>(offsets);   // (the collect instantiations only read them)
    p.ids = ids;
    p.counts = counts;
    const uint32_t blocks = csr_blocks(num_queries);
    if (shape == RT_RANGE_SPHERE) range_query_kernel<RT_RANGE_SPHERE, true><<<blocks, kCsrBlock, 0, st>>>(p);
    else range_query_kernel<RT_RANGE_BOX, true><<<blocks, kCsrBlock, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
