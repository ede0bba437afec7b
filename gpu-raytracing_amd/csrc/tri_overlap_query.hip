// tri_overlap_query.hip -- rt_tri_overlaps_count / rt_tri_overlaps_collect: every triangle of a built tree that a caller
// triangle cuts (semantics: rt_abi.h, triangle-overlap block), through any tree rt_intersect_rays takes.  The
// result is CSR, as for the range queries: offsets[0..n] by a 64-bit device scan of the per-query counts, then ids written per
// query segment.
//
// tri_overlap_kernel<SELF, COLLECT> keeps the frame of range_query_kernel (range_query.hip): one lane per query, 64 consecutive
// queries per wave, kTraceWaves waves (256 queries) per workgroup, xcd_chunk_block, a 4-byte stack entry (a box run child : 29 |
// count : 3, or a leaf index : 29 | 0), 16 entries in an LDS column per lane (16 KB per workgroup) + 48 private, the first
// surviving slot of a run visited next and the others pushed in slot order, rt_traverse.hpp's wave-level two phases with the
// park ratio, a leaf in four 16-byte requests, exact per-workgroup counters, the status word through ballots, the workgroup
// scan of the counts (COLLECT = false) and plain stores into the lane's own segment (COLLECT = true).  What differs:
//   * the query is a 36-byte rt_triangle (nine 4-byte loads); the lane keeps its vertex box (the slot test and condition 1 of
//     the predicate: Region<RT_RANGE_BOX>'s closed overlap test), P' = (0, p1 - p0, p2 - p0), the edge e1 and the normal nP;
//     everything on the Q side is derived per leaf triangle;
//   * the leaf test is cuts(P, Q): the vertex boxes first, in SELF mode then the id rule (j > i) and the nine corner
//     comparisons, and only then the separating-axis arithmetic, which leaves at the first separating axis.  The seventeen
//     axes run in three rolled loops (the two normals, the nine edge crosses, the six in-plane axes) over one projection
//     routine: the axis operands are picked by selects, so the code stays a fraction of seventeen unrolled copies;
//   * SELF = true: the query index is the triangle's id; the lane also keeps p1 and p2 for the corner comparisons.
// The workgroup geometry, the limb scan, the segment prologue, the epilogue (csr_finish) and the scan over the workgroups'
// totals are rt_csr.hpp's and csr_scan.hip's (launch_csr_offsets); the corner un-rotation and slot_entry live in
// rt_point_math.hpp.
// Compiled with -ffp-contract=off and IEEE division: every float operation is the one rt_abi.h writes down.
#include "rt_csr.hpp"
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_triangle) == 36, "rt_triangle: nine floats");

// waves per SIMD the register allocator must fit: the lean bound of the sibling query kernels (8: 64 VGPRs) spills inside the
// separating-axis loops of the SELF instantiations; one wave less (72 VGPRs) keeps the loops of the plain instantiations free
// of spill code and leaves a handful in the SELF ones (resource table)
#ifndef RT_TRI_MIN_WAVES
#define RT_TRI_MIN_WAVES (RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA - 1)
#endif

namespace rt {

namespace {

struct TriOverlapParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float* queries;         // nine floats per query: p0, p1, p2
    uint32_t num_queries;
    uint64_t* offsets;            // count: out, workgroup-local prefixes; collect: in
    uint64_t* block_sums;         // count: out, one total per workgroup
    uint32_t* ids;                // collect
    uint32_t* counts;             // collect, optional
    unsigned long long* counters;
    uint32_t* status;
};

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 v_sub(const V3& a, const V3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 v_cross(const V3& a, const V3& b)
{
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float v_dot(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// element k of (a, b, c) by selects (k is a loop counter, not a compile-time constant: the loops stay rolled)
__device__ __forceinline__ V3 v_pick(int k, const V3& a, const V3& b, const V3& c)
{
    return {k == 0 ? a.x : k == 1 ? b.x : c.x, k == 0 ? a.y : k == 1 ? b.y : c.y, k == 0 ? a.z : k == 1 ? b.z : c.z};
}
__device__ __forceinline__ V3 v_neg(const V3& a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ bool v_eq(const V3& a, const V3& b) { return (a.x == b.x) & (a.y == b.y) & (a.z == b.z); }

// the query side of cuts(P, Q), per lane
struct QueryTri {
    V3 p0, p1, p2;                 // the corners (p1, p2: read by the SELF corner comparisons only)
    V3 d1, d2;                     // P'_1 = p1 - p0 (= e0), P'_2 = p2 - p0
    V3 e1;                         // p2 - p1.  e2 = p0 - p2 is taken as -P'_2: IEEE subtraction is antisymmetric, so the two
                                   // differ at most in the sign of a zero, which no product, sum, fminf / fmaxf or comparison
                                   // below turns into a different verdict
    V3 n;                          // nP = cross(e0, e1)
    float lx, ly, lz, hx, hy, hz;  // the vertex box
    // closed overlap on every axis: tlo <= hi && thi >= lo  (Region<RT_RANGE_BOX>::over)
    __device__ __forceinline__ bool over(float tlx, float tly, float tlz, float thx, float thy, float thz) const
    {
        return (tlx <= hx) & (tly <= hy) & (tlz <= hz) & (thx >= lx) & (thy >= ly) & (thz >= lz);
    }
    __device__ __forceinline__ bool keep(const uint4& a, const uint4& b) const
    {
        return over(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(b.x), __uint_as_float(b.y),
                    __uint_as_float(b.z));
    }
};

// does axis a separate P' = (0, d1, d2) from Q' = (r0, r1, r2)?  Strict comparisons; a NaN makes both false.
// (the projection of P'_0 = 0 is computed, not assumed: an infinite axis component makes it NaN, which fminf / fmaxf drop)
__device__ __forceinline__ bool axis_separates(const V3& a, const QueryTri& q, const V3& r0, const V3& r1, const V3& r2)
{
    const V3 zero = {0.0f, 0.0f, 0.0f};
    const float p0 = v_dot(a, zero), p1 = v_dot(a, q.d1), p2 = v_dot(a, q.d2);
    const float q0 = v_dot(a, r0), q1 = v_dot(a, r1), q2 = v_dot(a, r2);
    const float minp = fminf(fminf(p0, p1), p2), maxp = fmaxf(fmaxf(p0, p1), p2);
    const float minq = fminf(fminf(q0, q1), q2), maxq = fmaxf(fmaxf(q0, q1), q2);
    return (minp > maxq) | (minq > maxp);
}

// condition 2 of cuts(P, Q): no separating axis among the seventeen of rt_abi.h; t holds the caller's corners of Q in the
// caller's order.  Any evaluation order gives the same answer (a conjunction over the axes); this one leaves at the first
// separating axis.
__device__ __forceinline__ bool no_separating_axis(const QueryTri& q, const Tri& t)
{
    const V3 c0 = {t.ax, t.ay, t.az}, c1 = {t.bx, t.by, t.bz}, c2 = {t.cx, t.cy, t.cz};
    const V3 r0 = v_sub(c0, q.p0), r1 = v_sub(c1, q.p0), r2 = v_sub(c2, q.p0);
    const V3 f0 = v_sub(c1, c0), f1 = v_sub(c2, c1), f2 = v_sub(c0, c2);
    const V3 nq = v_cross(f0, f1);
#pragma unroll 1
    for (int k = 0; k < 2; k++) {                       // the two normals
        const V3 a = {k == 0 ? q.n.x : nq.x, k == 0 ? q.n.y : nq.y, k == 0 ? q.n.z : nq.z};
        if (axis_separates(a, q, r0, r1, r2)) return false;
    }
#pragma unroll 1
    for (int k = 0; k < 9; k++) {                       // cross(e_i, f_j): i outer, j inner
        const int i = k / 3, j = k - 3 * i;
        const V3 e = v_pick(i, q.d1, q.e1, v_neg(q.d2)), f = v_pick(j, f0, f1, f2);
        if (axis_separates(v_cross(e, f), q, r0, r1, r2)) return false;
    }
#pragma unroll 1
    for (int k = 0; k < 6; k++) {                       // in-plane: cross(nP, e_i), then cross(nQ, f_j)
        const int i = k < 3 ? k : k - 3;
        const V3 g = k < 3 ? v_pick(i, q.d1, q.e1, v_neg(q.d2)) : v_pick(i, f0, f1, f2);
        const V3 n = {k < 3 ? q.n.x : nq.x, k < 3 ? q.n.y : nq.y, k < 3 ? q.n.z : nq.z};
        if (axis_separates(v_cross(n, g), q, r0, r1, r2)) return false;
    }
    return true;
}

typedef uint32_t ToSpill[kStackMax - kCsrStackLds];

template <bool SELF, bool COLLECT>
__global__ __launch_bounds__(kTraceWaves * 64, RT_TRI_MIN_WAVES) void tri_overlap_kernel(TriOverlapParams p)
{
    __shared__ uint32_t stack_lds[kTraceWaves][kCsrStackLds][64];
    __shared__ unsigned long long csum[2];
    __shared__ uint32_t ws[kTraceWaves + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_queries;
    if (p.counters && threadIdx.x < 2) csum[threadIdx.x] = 0ull;   // (kernel argument: the same for every thread)

    QueryTri q = {};
    bool live = false;
    if (in_range) {
        const float* c = p.queries + i * 9u;
        q.p0 = {c[0], c[1], c[2]};
        q.p1 = {c[3], c[4], c[5]};
        q.p2 = {c[6], c[7], c[8]};
        // not traced: a non-finite corner component
        const bool finite = __builtin_isfinite(q.p0.x) & __builtin_isfinite(q.p0.y) & __builtin_isfinite(q.p0.z) &
                            __builtin_isfinite(q.p1.x) & __builtin_isfinite(q.p1.y) & __builtin_isfinite(q.p1.z) &
                            __builtin_isfinite(q.p2.x) & __builtin_isfinite(q.p2.y) & __builtin_isfinite(q.p2.z);
        live = finite && p.count > 0;
        q.lx = fminf(fminf(q.p0.x, q.p1.x), q.p2.x); q.hx = fmaxf(fmaxf(q.p0.x, q.p1.x), q.p2.x);
        q.ly = fminf(fminf(q.p0.y, q.p1.y), q.p2.y); q.hy = fmaxf(fmaxf(q.p0.y, q.p1.y), q.p2.y);
        q.lz = fminf(fminf(q.p0.z, q.p1.z), q.p2.z); q.hz = fmaxf(fmaxf(q.p0.z, q.p1.z), q.p2.z);
        q.d1 = v_sub(q.p1, q.p0);
        q.d2 = v_sub(q.p2, q.p0);
        q.e1 = v_sub(q.p2, q.p1);
        q.n = v_cross(q.d1, q.e1);
    }

    // collect: the lane's segment [out, out + room)
    uint32_t* out = nullptr;
    uint32_t room = 0;
    if (COLLECT && in_range) out = csr_segment(p.offsets, p.ids, i, room);

    lds_u32* const col = (lds_u32*)&stack_lds[wave][0][lane];
    ToSpill spill;
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
    // cuts(P, Q) on the stored corners (s0, s1, s2) of triangle `id`, rotation rot: the vertex boxes, in SELF mode the id and
    // corner exclusions, then the separating axes on the caller's corner order
    auto cuts = [&](float s0x, float s0y, float s0z, float s1x, float s1y, float s1z, float s2x, float s2y, float s2z,
                    uint32_t rot, uint32_t id) -> bool {
        // fminf / fmaxf of the three corners do not depend on their order: no unrotate yet
        if (!q.over(fminf(fminf(s0x, s1x), s2x), fminf(fminf(s0y, s1y), s2y), fminf(fminf(s0z, s1z), s2z),
                    fmaxf(fmaxf(s0x, s1x), s2x), fmaxf(fmaxf(s0y, s1y), s2y), fmaxf(fmaxf(s0z, s1z), s2z)))
            return false;
        if (SELF) {
            if (!(id > (uint32_t)i)) return false;
            const V3 s0 = {s0x, s0y, s0z}, s1 = {s1x, s1y, s1z}, s2 = {s2x, s2y, s2z};
            if (v_eq(s0, q.p0) || v_eq(s0, q.p1) || v_eq(s0, q.p2) || v_eq(s1, q.p0) || v_eq(s1, q.p1) || v_eq(s1, q.p2) ||
                v_eq(s2, q.p0) || v_eq(s2, q.p1) || v_eq(s2, q.p2))
                return false;
        }
        return no_separating_axis(q, unrotate(s0x, s0y, s0z, s1x, s1y, s1z, s2x, s2y, s2z, rot));
    };
    auto leaf_step = [&]() {
        tri_tests++;
        uint4 l0, l1, l2, l3;
        load_leaf_wide(p.leaves + (cur & kIndexMask), l0, l1, l2, l3);
        // A = (v0, v1, v2) with rotations[0]; a pair record also holds B = (v2, v1, v3) with rotations[1].  One rolled loop:
        // the predicate's code exists once
        const int ntri = l1.w == l0.w + 1u ? 2 : 1;
#pragma unroll 1
        for (int t = 0; t < ntri; t++) {
            const bool b = t != 0;
            const uint32_t id = b ? l1.w : l0.w;
            if (cuts(__uint_as_float(b ? l2.x : l0.x), __uint_as_float(b ? l2.y : l0.y), __uint_as_float(b ? l2.z : l0.z),
                     __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                     __uint_as_float(b ? l3.x : l2.x), __uint_as_float(b ? l3.y : l2.y), __uint_as_float(b ? l3.z : l2.z),
                     b ? l2.w >> 16 : l2.w & 0xFFFFu, id))
                emit(id);
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
            if (!q.keep(a, b) || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // outside the query's box, or an empty run
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

    csr_finish<COLLECT, RT_TRI_STACK_OVERFLOW, RT_TRI_TRUNCATED>(
        in_range, i, vb, lane, overflow, found, room, box_tests, tri_tests, p.offsets, p.block_sums, p.counts, p.status,
        p.counters, ws, csum);
}

TriOverlapParams tri_params(const rt_accel& as, const rt_triangle* queries, uint32_t num_queries, uint64_t* counters,
                            uint32_t* status)
{
    TriOverlapParams p = {};
    set_tree(p, as);
    p.queries = reinterpret_cast<const float*>(queries);
    p.num_queries = num_queries;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    return p;
}

}  // namespace

size_t tri_overlaps_scratch_bytes(uint32_t num_queries) { return csr_scratch_bytes(num_queries); }

hipError_t launch_tri_overlaps_count(const rt_accel& as, const rt_triangle* queries, uint32_t num_queries, bool self,
                                     uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    TriOverlapParams p = tri_params(as, queries, num_queries, counters, status);
    p.offsets = offsets;
    p.block_sums = static_cast<uint64_t*>(scratch);
    const uint32_t blocks = csr_blocks(num_queries);
    if (blocks) {
        if (self) tri_overlap_kernel<true, false><<<blocks, kCsrBlock, 0, st>>>(p);
        else tri_overlap_kernel<false, false><<<blocks, kCsrBlock, 0, st>>>(p);
    }
    return launch_csr_offsets(offsets, p.block_sums, num_queries, st);
}

hipError_t launch_tri_overlaps_collect(const rt_accel& as, const rt_triangle* queries, uint32_t num_queries, bool self,
                                       const uint64_t* offsets, uint32_t* ids, uint32_t* counts, uint64_t* counters,
                                       uint32_t* status, hipStream_t st)
{
    TriOverlapParams p = tri_params(as, queries, num_queries, counters, status);
    p.offsets = const_cast<uint64_t*>(offsets);   // (the collect instantiations only read them)
    p.ids = ids;
    p.counts = counts;
    const uint32_t blocks = csr_blocks(num_queries);
    if (self) tri_overlap_kernel<true, true><<<blocks, kCsrBlock, 0, st>>>(p);
    else tri_overlap_kernel<false, true><<<blocks, kCsrBlock, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
