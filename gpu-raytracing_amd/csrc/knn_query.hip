// knn_query.hip -- rt_k_nearest: the K nearest triangles to each caller point, in ascending (dist2, primitive_id) order, through
// any tree rt_intersect_rays takes (semantics: rt_abi.h, k-nearest block).
//
// knn_query_kernel keeps the frame of point_query_kernel: one lane per query, 64 consecutive queries per wave, kTraceWaves
// waves (256 queries) per workgroup, xcd_chunk_block, the query in one 16-byte load, the nearest-first box step with 8-byte
// (entry, boxdist2) stack entries (16 in an LDS column per lane, 48 private), pops re-culled against the current bound,
// rt_traverse.hpp's wave-level two phases, a leaf in four 16-byte requests, the restart rule (a pass that dropped a push is
// followed by another from the root, at most kNearRestarts more), exact per-workgroup counters.  What differs: the lane keeps
// the K best instead of one and prunes against the K-th.
//   * bound = dist2_max while the list holds fewer than k entries, the k-th dist2 once it is full; a slot or a popped entry is
//     skipped iff boxdist2 > bound;
//   * the list is a sorted array of m <= k records (dist2, id) at lane-private addresses; m, the k-th record and the bound live
//     in registers.  A leaf's candidate is first tested against the registers alone: beyond the radius, NaN, or not below the
//     k-th of a full list -- most candidates end there, without a memory access;
//   * a survivor finds its position first (a scan down from the top; an equal record means the triangle is already listed --
//     a restart re-visits, a split tree holds several references -- and the candidate is dropped) and shifts afterwards: a
//     shift-while-scanning insertion would have moved records before it meets the equal one;
//   * plain vector loads and stores, no atomics.
// Where the list lives, RT_KNN_LIST (both arms give byte-identical rows: the result is a function of the candidate set):
//   0  the output row itself, out + i * k, finished in place (misses appended at the end): no copy, but a lane's records lie
//      8 k bytes from its neighbours';
//   1  a private array of RT_KNN_MAX_K records written out once at the end: scratch is lane-interleaved, so equal indices of a
//      wave share cache lines.
// Shipped: 1.  tools/knn_bench.py measures both arms in one session (an arm is a library build: csrc/Makefile's
// librt_amd_exp.so with EXPFLAGS=-DRT_KNN_LIST=0); DESIGN section 14 holds the state of that measurement.
// Compiled with -ffp-contract=off and IEEE division: every float operation is the one rt_abi.h writes down.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_point_query) == 16 && offsetof(rt_point_query, dist2_max) == 12, "rt_point_query: p, dist2_max");
static_assert(sizeof(rt_knn_hit) == 8 && offsetof(rt_knn_hit, primitive_id) == 4, "rt_knn_hit: one 8-byte record");

#ifndef RT_KNN_LIST
#define RT_KNN_LIST 1
#endif

namespace rt {

namespace {

static_assert(kQueryBlock == kTraceWaves * 64, "rt_launch.hpp: one lane per query, kTraceWaves waves per workgroup");

struct KnnParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* queries;   // rt_point_query = one float4: (p, dist2_max)
    uint2* out;              // rt_knn_hit = one uint2: (dist2 bits, primitive_id); row i at out + i * k
    uint32_t num_queries, k;
    unsigned long long* counters;
    uint32_t* status;
};

typedef NearEntry KnnSpill[kStackMax - kNearStackLds];
typedef __attribute__((address_space(3))) NearEntry lds_knn_entry;

__global__ __launch_bounds__(kTraceWaves * 64) void knn_query_kernel(KnnParams p)
{
    // the counters' workgroup sums reuse the stack's LDS once every lane is done with it (no extra bytes: 32 KB exactly)
    __shared__ alignas(8) NearEntry stack_lds[kTraceWaves][kNearStackLds][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_queries;
    const uint32_t k = p.k;

    float4 q = {0.f, 0.f, 0.f, -1.f};
    if (in_range) q = p.queries[i];
    const float px = q.x, py = q.y, pz = q.z;
    // not traced (a row of misses, no tests): lanes past the batch, a non-finite p, a NaN or negative dist2_max
    const bool finite_p = __builtin_isfinite(px) & __builtin_isfinite(py) & __builtin_isfinite(pz);
    bool live = in_range && finite_p && q.w >= 0.0f && p.count > 0;   // (q.w >= 0 is false for NaN)

    // the list: m records in ascending (dist2, id) order.  Only a live lane touches it, and a live lane is in range.
#if RT_KNN_LIST == 0
    uint2* const list = p.out + i * k;
#else
    uint2 list[RT_KNN_MAX_K];
#endif
    uint32_t m = 0;
    float kth_d = __builtin_inff();   // the k-th record, valid once m == k
    uint32_t kth_id = RT_MISS;
    float bound = q.w;                // dist2_max while m < k, kth_d after

    lds_knn_entry* const col = (lds_knn_entry*)&stack_lds[wave][0][lane];
    KnnSpill spill;
    int sp = 0;
    bool overflow = false;            // a push of the current pass was dropped
    int restarts = 0;
    uint32_t box_tests = 0, tri_tests = 0;
    uint32_t cur = (p.root & kIndexMask) | (p.count << 29);

    // a candidate (d, id) of a leaf.  d2 is a sum of squares: never -0, so equal floats are equal bit patterns.
    auto offer = [&](float d, uint32_t id) {
        if (!(d <= q.w)) return;                                              // beyond the radius, or NaN
        const bool full = m == k;
        if (full && !(d < kth_d || (d == kth_d && id < kth_id))) return;      // not below the k-th: registers only
        // the position: the records above the candidate are [pos, m); a full list's k-th is above it (the test before)
        const uint32_t top = full ? k - 1 : m;
        uint32_t pos = top;
        while (pos > 0) {
            const uint2 e = list[pos - 1];
            const float ed = __uint_as_float(e.x);
            if (ed == d && e.y == id) return;                                 // already listed
            if (ed < d || (ed == d && e.y < id)) break;
            pos--;
        }
        // the shift, from the top down: [pos, top) -> [pos + 1, top + 1); a full list loses its k-th
        for (uint32_t j = top; j > pos; j--) list[j] = list[j - 1];
        list[pos] = make_uint2(__float_as_uint(d), id);
        m = top + 1;
        if (m == k) {
            if (pos == k - 1) { kth_d = d; kth_id = id; }
            else { const uint2 e = list[k - 1]; kth_d = __uint_as_float(e.x); kth_id = e.y; }
            bound = kth_d;
        }
    };

    // the next entry after a finished run or leaf: a pop, re-culled against the current bound; on an empty stack the lane is
    // done -- unless the pass dropped a push: then the whole traversal runs again from the root with the list so far, whose
    // bound prunes what is farther and whose records are recognised when they are met again
    auto next_from_stack = [&]() {
        while (sp > 0) {
            --sp;
            const NearEntry se = sp < kNearStackLds ? col[sp * 64] : spill[sp - kNearStackLds];
            if (__uint_as_float((uint32_t)(se >> 32)) <= bound) { cur = (uint32_t)se; return; }
        }
        if (!overflow || restarts == kNearRestarts) { live = false; return; }
        restarts++;
        overflow = false;
        cur = (p.root & kIndexMask) | (p.count << 29);
    };
    auto leaf_step = [&]() {
        tri_tests++;
        uint4 l0, l1, l2, l3;
        load_leaf_wide(p.leaves + (cur & kIndexMask), l0, l1, l2, l3);
        offer(range_tri_d2(px, py, pz, leaf_tri_a(l0, l1, l2)), l0.w);
        if (l1.w == l0.w + 1u)                // a pair record: B = (v2, v1, v3) with rotations[1]
            offer(range_tri_d2(px, py, pz, leaf_tri_b(l1, l2, l3)), l1.w);
        next_from_stack();
    };
    auto box_step = [&]() {
        const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
        uint32_t near_e = kNoNear;
        float near_d = __builtin_inff();
        for (uint32_t s = 0; s < cnt; s++) {
            const uint4* np = reinterpret_cast<const uint4*>(p.nodes + first + s);
            const uint4 a = np[0], b = np[1];
            const uint32_t type = b.w >> 29;
            if (type == RT_CHILD_NONE) continue;
            box_tests++;
            const float bd = box_d2(a, b, px, py, pz);
            const uint32_t e = slot_entry(a, b);
            if (bd > bound || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // pruned, or an empty run
            NearEntry pe = (uint64_t)e | ((uint64_t)__float_as_uint(bd) << 32);
            if (bd < near_d) {                // the new nearest; the old one (if any) is pushed
                pe = (uint64_t)near_e | ((uint64_t)__float_as_uint(near_d) << 32);
                near_e = e; near_d = bd;
            }
            if ((uint32_t)pe != kNoNear) {
                if (sp < kNearStackLds) col[sp * 64] = pe;
                else if (sp < kStackMax) spill[sp - kNearStackLds] = pe;
                else overflow = true;         // dropped: this pass may miss one of the nearest
                sp = min(sp + 1, kStackMax);
            }
        }
        if (near_e != kNoNear) cur = near_e;
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

    if (in_range) {
        uint2* const row = p.out + i * k;
        const uint2 miss = make_uint2(__float_as_uint(__builtin_inff()), RT_MISS);
#if RT_KNN_LIST == 0
        for (uint32_t j = m; j < k; j++) row[j] = miss;
#else
        for (uint32_t j = 0; j < k; j++) row[j] = j < m ? list[j] : miss;
#endif
    }
    if (p.status && __builtin_amdgcn_ballot_w64(overflow) != 0 && lane == 0) atomicOr(p.status, (uint32_t)RT_KNN_STACK_OVERFLOW);
    finish_counters(p.counters, reinterpret_cast<unsigned long long*>(&stack_lds[0][0][0]), lane, box_tests, tri_tests);
}

}  // namespace

hipError_t launch_knn_query(const rt_accel& as, const rt_point_query* queries, uint32_t num_queries, uint32_t k, rt_knn_hit* out,
                            uint64_t* counters, uint32_t* status, hipStream_t st)
{
    KnnParams p;
    set_tree(p, as);
    p.queries = reinterpret_cast<const float4*>(queries);
    p.out = reinterpret_cast<uint2*>(out);
    p.num_queries = num_queries;
    p.k = k;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    const dim3 grid(query_blocks(num_queries)), block(kQueryBlock);
    knn_query_kernel<<<grid, block, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
