// point_query.hip -- rt_closest_points: the nearest triangle to each caller point, through any tree rt_intersect_rays takes
// (semantics: rt_abi.h, closest-point block).
//
// point_query_kernel keeps the frame of ray_query_kernel: one lane per query, 64 consecutive queries per wave, kTraceWaves
// waves (256 queries) per workgroup, xcd_chunk_block, one 16-byte load per query and one 16-byte store per record, exact
// per-workgroup counters (LDS sum, then one device atomic per counter).  The visiting order is by distance instead of along a
// ray, per lane:
//   * the lane holds one entry: a box run (child : 29 | count : 3, count 1..7) or a leaf (index : 29 | 0 -- a box run never has
//     count 0, so the two cannot be confused; a box slot whose run is empty is skipped);
//   * a box run: boxdist2 of every non-NONE slot (counted as a box test); a slot with boxdist2 > best is pruned, the nearest
//     survivor (leaf or box child; ties to the lower slot) becomes the next entry and the other survivors are pushed with their
//     boxdist2;
//   * a leaf: the 64-byte record, its corners put back in the caller's order through TrianglePair::rotations, d2 on triangle A
//     and, for a pair record (primitive_id_1 == primitive_id_0 + 1), on B; (dist2, id) replaces the best when it is
//     lexicographically smaller (counted as one triangle test);
//   * a pop re-culls: an entry whose stored boxdist2 is > best is dropped unvisited;
//   * stack: 16 entries of 8 bytes (entry, boxdist2) in an LDS column per lane, 48 more in private memory; a push onto a full
//     stack of 64 is dropped.  A pass that dropped a push is followed, once its stack is empty, by another pass from the root
//     with the best so far (at most kNearRestarts more): a pass that drops nothing makes the record exact.  When the last pass
//     still dropped a push the lane sets RT_POINT_STACK_OVERFLOW (one atomicOr per wave that has such a lane).
// Schedule: rt_traverse.hpp's wave-level two phases -- box steps while enough lanes hold a box run, then one leaf step for the
// lanes that hold a leaf.  It measured 1.02-1.17x faster than a per-lane loop, and 8-byte entries beat 4-byte slot entries
// re-tested on pop on 12 of 16 (tree, set) cells (profiles/point_query_variants.json).
// d2 with the weights, the corner un-rotation, boxdist2, slot_entry and the descent's constants live in rt_point_math.hpp,
// shared with knn_query.hip, range_query.hip and sdf_query.hip.  Phase 1 of sdf_kernel (sdf_query.hip) is this descent with
// the weight-free d2 and promises this kernel's (dist2, primitive_id), dropped pushes included: a change to the descent here
// is a change there (tests/test_gpu_sdf.py::test_overflowed_distance_equals_closest_points).
// Compiled with -ffp-contract=off and IEEE division: every float operation is the one rt_abi.h writes down.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_point_query) == 16 && offsetof(rt_point_query, dist2_max) == 12, "rt_point_query: p, dist2_max");
static_assert(sizeof(rt_point_hit) == 16 && offsetof(rt_point_hit, primitive_id) == 4 && offsetof(rt_point_hit, v) == 12,
              "rt_point_hit: one 16-byte record");

namespace rt {

namespace {

static_assert(kQueryBlock == kTraceWaves * 64, "rt_launch.hpp: one lane per query, kTraceWaves waves per workgroup");

struct PointParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* queries;   // rt_point_query = one float4: (p, dist2_max)
    float4* hits;            // rt_point_hit = one float4: (dist2, primitive_id bits, u, v)
    uint32_t num_queries;
    unsigned long long* counters;
    uint32_t* status;
};

typedef NearEntry PtSpill[kStackMax - kNearStackLds];
typedef __attribute__((address_space(3))) NearEntry lds_entry;

__global__ __launch_bounds__(kTraceWaves * 64) void point_query_kernel(PointParams p)
{
    // the counters' workgroup sums reuse the stack's LDS once every lane is done with it (no extra bytes: 32 KB exactly)
    __shared__ alignas(8) NearEntry stack_lds[kTraceWaves][kNearStackLds][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_queries;

    float4 q = {0.f, 0.f, 0.f, -1.f};
    if (in_range) q = p.queries[i];
    const float px = q.x, py = q.y, pz = q.z;
    // not traced (a miss, no tests): lanes past the batch, a non-finite p, a NaN or negative dist2_max
    const bool finite_p = __builtin_isfinite(px) & __builtin_isfinite(py) & __builtin_isfinite(pz);
    bool live = in_range && finite_p && q.w >= 0.0f && p.count > 0;   // (q.w >= 0 is false for NaN)

    lds_entry* const col = (lds_entry*)&stack_lds[wave][0][lane];
    PtSpill spill;
    int sp = 0;
    bool overflow = false;            // a push of the current pass was dropped
    int restarts = 0;
    float best = q.w;
    uint32_t best_id = RT_MISS;
    float bu = 0.0f, bv = 0.0f;
    uint32_t box_tests = 0, tri_tests = 0;
    uint32_t cur = (p.root & kIndexMask) | (p.count << 29);

    // the next entry after a finished run or leaf: a pop, re-culled against the current best; on an empty stack the lane is
    // done -- unless the pass dropped a push: then the whole traversal runs again from the root with the best so far, which
    // prunes what is farther (the result is exact when a pass drops nothing)
    auto next_from_stack = [&]() {
        while (sp > 0) {
            --sp;
            const NearEntry se = sp < kNearStackLds ? col[sp * 64] : spill[sp - kNearStackLds];
            if (__uint_as_float((uint32_t)(se >> 32)) <= best) { cur = (uint32_t)se; return; }
        }
        if (!overflow || restarts == kNearRestarts) { live = false; return; }
        restarts++;
        overflow = false;
        cur = (p.root & kIndexMask) | (p.count << 29);
    };
    auto leaf_step = [&]() {
        tri_tests++;
        const uint4* tp = reinterpret_cast<const uint4*>(p.leaves + (cur & kIndexMask));
        const uint4 l0 = tp[0], l1 = tp[1], l2 = tp[2], l3 = tp[3];
        {
            const Tri ta = leaf_tri_a(l0, l1, l2);
            float u, v;
            const float d = tri_d2<true>(px, py, pz, ta, u, v);
            if (d < best || (d == best && l0.w < best_id)) { best = d; best_id = l0.w; bu = u; bv = v; }
        }
        if (l1.w == l0.w + 1u) {              // a pair record: B = (v2, v1, v3) with rotations[1]
            const Tri tb = leaf_tri_b(l1, l2, l3);
            float u, v;
            const float d = tri_d2<true>(px, py, pz, tb, u, v);
            if (d < best || (d == best && l1.w < best_id)) { best = d; best_id = l1.w; bu = u; bv = v; }
        }
        next_from_stack();
    };
    auto box_step = [&]() {
        const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
        uint32_t near_e = kNoNear;
        float near_d = __builtin_inff();
        for (uint32_t k = 0; k < cnt; k++) {
            const uint4* np = reinterpret_cast<const uint4*>(p.nodes + first + k);
            const uint4 a = np[0], b = np[1];
            const uint32_t type = b.w >> 29;
            if (type == RT_CHILD_NONE) continue;
            box_tests++;
            const float bd = box_d2(a, b, px, py, pz);
            const uint32_t e = slot_entry(a, b);
            if (bd > best || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // pruned, or an empty run
            NearEntry pe = (uint64_t)e | ((uint64_t)__float_as_uint(bd) << 32);
            if (bd < near_d) {                // the new nearest; the old one (if any) is pushed
                pe = (uint64_t)near_e | ((uint64_t)__float_as_uint(near_d) << 32);
                near_e = e; near_d = bd;
            }
            if ((uint32_t)pe != kNoNear) {
                if (sp < kNearStackLds) col[sp * 64] = pe;
                else if (sp < kStackMax) spill[sp - kNearStackLds] = pe;
                else overflow = true;         // dropped: this pass may miss the nearest triangle
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
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (best_id != RT_MISS) o = {best, __uint_as_float(best_id), bu + 0.0f, bv + 0.0f};   // (+ 0: -0 becomes +0)
        p.hits[i] = o;
    }
    if (p.status && __builtin_amdgcn_ballot_w64(overflow) != 0 && lane == 0) atomicOr(p.status, (uint32_t)RT_POINT_STACK_OVERFLOW);
    finish_counters(p.counters, reinterpret_cast<unsigned long long*>(&stack_lds[0][0][0]), lane, box_tests, tri_tests);
}

}  // namespace

hipError_t launch_point_query(const rt_accel& as, const rt_point_query* queries, rt_point_hit* hits, uint32_t num_queries,
                              uint64_t* counters, uint32_t* status, hipStream_t st)
{
    PointParams p;
    set_tree(p, as);
    p.queries = reinterpret_cast<const float4*>(queries);
    p.hits = reinterpret_cast<float4*>(hits);
    p.num_queries = num_queries;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    const dim3 grid(query_blocks(num_queries)), block(kQueryBlock);
    point_query_kernel<<<grid, block, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
