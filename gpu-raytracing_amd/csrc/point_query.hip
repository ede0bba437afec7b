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
//     with the best so far (at most kPtRestarts more): a pass that drops nothing makes the record exact.  When the last pass
//     still dropped a push the lane sets RT_POINT_STACK_OVERFLOW (one atomicOr per wave that has such a lane).
// Schedule: rt_traverse.hpp's wave-level two phases -- box steps while enough lanes hold a box run, then one leaf step for the
// lanes that hold a leaf.  It measured 1.02-1.17x faster than a per-lane loop, and 8-byte entries beat 4-byte slot entries
// re-tested on pop on 12 of 16 (tree, set) cells (profiles/point_query_variants.json); both other arms
// stay compilable behind RT_POINT_PHASED / RT_POINT_DIST_STACK.
// Compiled with -ffp-contract=off and IEEE division: every float operation is the one rt_abi.h writes down.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_point_query) == 16 && offsetof(rt_point_query, dist2_max) == 12, "rt_point_query: p, dist2_max");
static_assert(sizeof(rt_point_hit) == 16 && offsetof(rt_point_hit, primitive_id) == 4 && offsetof(rt_point_hit, v) == 12,
              "rt_point_hit: one 16-byte record");

namespace rt {

namespace {

constexpr int kPtStackLds = 16;   // LDS-resident entries per lane: 16 x 8 B x 256 lanes = 32 KB per workgroup
constexpr int kPtRestarts = 2;    // passes from the root after a pass that dropped a push (each starts from the best so far)
// (sdf_query.hip restates this traversal -- kSdfStackLds, kSdfRestarts, the 8-byte entries of RT_POINT_DIST_STACK = 1 -- and
// promises rt_closest_points's record bit for bit, dropped pushes included: change the two files together)

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

__device__ __forceinline__ float pt_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return (ax * bx + ay * by) + az * bz;
}
// a denominator that is not > 0 (0, negative, NaN) gives weight 0; else the IEEE quotient
__device__ __forceinline__ float pt_guard(float num, float den) { return den > 0.0f ? num / den : 0.0f; }
// by selects: NaN -> 0, -0 -> +0
__device__ __forceinline__ float pt_clamp01(float t)
{
    t = t > 0.0f ? t : 0.0f;
    return t < 1.0f ? t : 1.0f;
}

struct Tri {
    float ax, ay, az, bx, by, bz, cx, cy, cz;
};

// rt_abi.h's FACE_NOISE: a face sum at or below this share of the magnitudes of its six products is rounding noise
constexpr float kFaceNoise = 0x1p-20f;

// dist2 of p to q after q is clamped into the triangle's vertex box (fmaxf, then fminf)
__device__ __forceinline__ float pt_clamped(float px, float py, float pz, float qx, float qy, float qz, const Tri& t)
{
    const float lox = fminf(fminf(t.ax, t.bx), t.cx), loy = fminf(fminf(t.ay, t.by), t.cy), loz = fminf(fminf(t.az, t.bz), t.cz);
    const float hix = fmaxf(fmaxf(t.ax, t.bx), t.cx), hiy = fmaxf(fmaxf(t.ay, t.by), t.cy), hiz = fmaxf(fmaxf(t.az, t.bz), t.cz);
    const float dx = px - fminf(fmaxf(qx, lox), hix);
    const float dy = py - fminf(fmaxf(qy, loy), hiy);
    const float dz = pz - fminf(fmaxf(qz, loz), hiz);
    return (dx * dx + dy * dy) + dz * dz;
}

// d2(p, a, b, c) of rt_abi.h: Ericson's ClosestPtPointTriangle (RTCD 5.1.5), the clamp into the vertex box, the squared
// distance.  u, v: the weights of b and c.
__device__ __forceinline__ float point_tri_d2(float px, float py, float pz, const Tri& t, float& u, float& v)
{
    const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
    const float acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
    const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
    const float d1 = pt_dot(abx, aby, abz, apx, apy, apz), d2 = pt_dot(acx, acy, acz, apx, apy, apz);
    float qx, qy, qz;
    if (d1 <= 0.0f && d2 <= 0.0f) {                                     // vertex region A
        u = 0.0f; v = 0.0f;
        return pt_clamped(px, py, pz, t.ax, t.ay, t.az, t);
    }
    const float bpx = px - t.bx, bpy = py - t.by, bpz = pz - t.bz;
    const float d3 = pt_dot(abx, aby, abz, bpx, bpy, bpz), d4 = pt_dot(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0f && d4 <= d3) {                                       // vertex region B
        u = 1.0f; v = 0.0f;
        return pt_clamped(px, py, pz, t.bx, t.by, t.bz, t);
    }
    const float vc = d1 * d4 - d3 * d2;
    const float t_ab = pt_clamp01(pt_guard(d1, d1 - d3));
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f && d1 - d3 > 0.0f) {    // edge region AB (of an edge that has a length)
        u = t_ab; v = 0.0f;
        return pt_clamped(px, py, pz, t.ax + t_ab * abx, t.ay + t_ab * aby, t.az + t_ab * abz, t);
    }
    const float cpx = px - t.cx, cpy = py - t.cy, cpz = pz - t.cz;
    const float d5 = pt_dot(abx, aby, abz, cpx, cpy, cpz), d6 = pt_dot(acx, acy, acz, cpx, cpy, cpz);
    if (d6 >= 0.0f && d5 <= d6) {                                       // vertex region C
        u = 0.0f; v = 1.0f;
        return pt_clamped(px, py, pz, t.cx, t.cy, t.cz, t);
    }
    const float vb = d5 * d2 - d1 * d6;
    const float t_ac = pt_clamp01(pt_guard(d2, d2 - d6));
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f && d2 - d6 > 0.0f) {    // edge region AC
        u = 0.0f; v = t_ac;
        return pt_clamped(px, py, pz, t.ax + t_ac * acx, t.ay + t_ac * acy, t.az + t_ac * acz, t);
    }
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const float t_bc = pt_clamp01(pt_guard(e43, e43 + e56));
    const float bcx = t.cx - t.bx, bcy = t.cy - t.by, bcz = t.cz - t.bz;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f && e43 + e56 > 0.0f) {   // edge region BC
        u = 1.0f - t_bc; v = t_bc;
        return pt_clamped(px, py, pz, t.bx + t_bc * bcx, t.by + t_bc * bcy, t.bz + t_bc * bcz, t);
    }
    // no vertex or edge region holds.  s is the squared area (times 4) as a sum of six products: where it stands clear of their
    // rounding noise, the face point as Ericson takes it
    const float s = (va + vb) + vc;
    const float noise = ((fabsf(d1 * d4) + fabsf(d3 * d2)) + (fabsf(d5 * d2) + fabsf(d1 * d6))) + (fabsf(d3 * d6) + fabsf(d5 * d4));
    const float fv = vb / s, fw = vc / s;
    qx = (t.ax + abx * fv) + acx * fw;
    qy = (t.ay + aby * fv) + acy * fw;
    qz = (t.az + abz * fv) + acz * fw;
    if (s > kFaceNoise * noise) {                                       // (false for a NaN)
        u = fv; v = fw;
        return pt_clamped(px, py, pz, qx, qy, qz, t);
    }
    // a face whose area is rounding noise (a collinear triangle: va, vb, vc are residues of any sign): the nearest of the three
    // edge points (ties: AB, then AC), unless the face point is a point of the triangle and no edge point is strictly nearer
    float best = pt_clamped(px, py, pz, t.ax + t_ab * abx, t.ay + t_ab * aby, t.az + t_ab * abz, t);
    u = t_ab; v = 0.0f;
    const float g_ac = pt_clamped(px, py, pz, t.ax + t_ac * acx, t.ay + t_ac * acy, t.az + t_ac * acz, t);
    if (g_ac < best) { best = g_ac; u = 0.0f; v = t_ac; }
    const float g_bc = pt_clamped(px, py, pz, t.bx + t_bc * bcx, t.by + t_bc * bcy, t.bz + t_bc * bcz, t);
    if (g_bc < best) { best = g_bc; u = 1.0f - t_bc; v = t_bc; }
    if (s > 0.0f && fv >= 0.0f && fw >= 0.0f && fv + fw <= 1.0f) {
        const float g_f = pt_clamped(px, py, pz, qx, qy, qz, t);
        if (!(best < g_f)) { best = g_f; u = fv; v = fw; }
    }
    return best;
}

// the caller's corners of a leaf triangle stored as (s0, s1, s2) with rotation r (RotateAttributes' corner map):
// r = 1: (c0, c1, c2) = (s1, s2, s0); r = 2: (s2, s0, s1); else as stored
__device__ __forceinline__ Tri unrotate(float s0x, float s0y, float s0z, float s1x, float s1y, float s1z, float s2x, float s2y,
                                        float s2z, uint32_t r)
{
    Tri t;
    if (r == 1) t = {s1x, s1y, s1z, s2x, s2y, s2z, s0x, s0y, s0z};
    else if (r == 2) t = {s2x, s2y, s2z, s0x, s0y, s0z, s1x, s1y, s1z};
    else t = {s0x, s0y, s0z, s1x, s1y, s1z, s2x, s2y, s2z};
    return t;
}

// boxdist2 of a slot: g = max(lo - p, p - hi, 0) per axis, squared and summed in d2's order
__device__ __forceinline__ float box_d2(const uint4& a, const uint4& b, float px, float py, float pz)
{
    const float gx = fmaxf(fmaxf(__uint_as_float(a.x) - px, px - __uint_as_float(b.x)), 0.0f);
    const float gy = fmaxf(fmaxf(__uint_as_float(a.y) - py, py - __uint_as_float(b.y)), 0.0f);
    const float gz = fmaxf(fmaxf(__uint_as_float(a.z) - pz, pz - __uint_as_float(b.z)), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

// The two design arms the issue left open, both kept compilable and measured (profiles/point_query_bench.json):
//   RT_POINT_PHASED      1: rt_traverse.hpp's wave-level schedule -- box steps while enough lanes hold a box run (kParkNum /
//                        kParkDen), then one leaf step for every lane that holds a leaf; 0: every lane runs its own loop
//   RT_POINT_DIST_STACK  1: a stack entry is 8 bytes, (entry, boxdist2): a pop is re-culled without a memory access;
//                        0: a stack entry is the 4-byte slot index that referenced it, and a pop reloads that slot and
//                        recomputes its boxdist2 (half the LDS: 16 KB per workgroup)
#ifndef RT_POINT_PHASED
#define RT_POINT_PHASED 1
#endif
#ifndef RT_POINT_DIST_STACK
#define RT_POINT_DIST_STACK 1
#endif
#if RT_POINT_DIST_STACK
typedef uint64_t PtEntry;   // entry (low word) | boxdist2 bits (high word)
#else
typedef uint32_t PtEntry;   // the referencing slot's index
#endif
typedef PtEntry PtSpill[kStackMax - kPtStackLds];
typedef __attribute__((address_space(3))) PtEntry lds_entry;

// the entry a slot refers to: a leaf (index : 29 | 0) or a box run (child : 29 | count : 3)
__device__ __forceinline__ uint32_t slot_entry(const uint4& a, const uint4& b)
{
    return (b.w >> 29) == RT_CHILD_TRI ? (b.w & kIndexMask) : ((b.w & kIndexMask) | (a.w & ~kIndexMask));
}

__global__ __launch_bounds__(kTraceWaves * 64) void point_query_kernel(PointParams p)
{
    // the counters' workgroup sums reuse the stack's LDS once every lane is done with it (no extra bytes: 32 KB exactly)
    __shared__ alignas(8) PtEntry stack_lds[kTraceWaves][kPtStackLds][64];
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
            const PtEntry se = sp < kPtStackLds ? col[sp * 64] : spill[sp - kPtStackLds];
#if RT_POINT_DIST_STACK
            if (__uint_as_float((uint32_t)(se >> 32)) <= best) { cur = (uint32_t)se; return; }
#else
            const uint4* np = reinterpret_cast<const uint4*>(p.nodes + se);
            const uint4 a = np[0], b = np[1];
            if (box_d2(a, b, px, py, pz) <= best) { cur = slot_entry(a, b); return; }
#endif
        }
        if (!overflow || restarts == kPtRestarts) { live = false; return; }
        restarts++;
        overflow = false;
        cur = (p.root & kIndexMask) | (p.count << 29);
    };
    auto leaf_step = [&]() {
        tri_tests++;
        const uint4* tp = reinterpret_cast<const uint4*>(p.leaves + (cur & kIndexMask));
        const uint4 l0 = tp[0], l1 = tp[1], l2 = tp[2], l3 = tp[3];
        {
            const Tri ta = unrotate(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
                                    __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                    __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), l2.w & 0xFFFFu);
            float u, v;
            const float d = point_tri_d2(px, py, pz, ta, u, v);
            if (d < best || (d == best && l0.w < best_id)) { best = d; best_id = l0.w; bu = u; bv = v; }
        }
        if (l1.w == l0.w + 1u) {              // a pair record: B = (v2, v1, v3) with rotations[1]
            const Tri tb = unrotate(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                    __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                    __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z), l2.w >> 16);
            float u, v;
            const float d = point_tri_d2(px, py, pz, tb, u, v);
            if (d < best || (d == best && l1.w < best_id)) { best = d; best_id = l1.w; bu = u; bv = v; }
        }
        next_from_stack();
    };
    auto box_step = [&]() {
        const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
        uint32_t near_e = kNoNear;
        float near_d = __builtin_inff();
#if !RT_POINT_DIST_STACK
        uint32_t near_s = 0;                  // the slot that refers to near_e
#endif
        for (uint32_t k = 0; k < cnt; k++) {
            const uint4* np = reinterpret_cast<const uint4*>(p.nodes + first + k);
            const uint4 a = np[0], b = np[1];
            const uint32_t type = b.w >> 29;
            if (type == RT_CHILD_NONE) continue;
            box_tests++;
            const float bd = box_d2(a, b, px, py, pz);
            const uint32_t e = slot_entry(a, b);
            if (bd > best || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // pruned, or an empty run
#if RT_POINT_DIST_STACK
            const PtEntry se_new = (uint64_t)e | ((uint64_t)__float_as_uint(bd) << 32);
            PtEntry pe = se_new;
            if (bd < near_d) {                // the new nearest; the old one (if any) is pushed
                pe = (uint64_t)near_e | ((uint64_t)__float_as_uint(near_d) << 32);
                near_e = e; near_d = bd;
            }
            const bool push = (uint32_t)pe != kNoNear;
#else
            PtEntry pe = first + k;
            bool push = true;
            if (bd < near_d) {
                pe = near_s;
                push = near_e != kNoNear;
                near_e = e; near_d = bd; near_s = first + k;
            }
#endif
            if (push) {
                if (sp < kPtStackLds) col[sp * 64] = pe;
                else if (sp < kStackMax) spill[sp - kPtStackLds] = pe;
                else overflow = true;         // dropped: this pass may miss the nearest triangle
                sp = min(sp + 1, kStackMax);
            }
        }
        if (near_e != kNoNear) cur = near_e;
        else next_from_stack();
    };

#if RT_POINT_PHASED
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
#else
    while (live) {
        if ((cur >> 29) == 0) leaf_step();
        else box_step();
    }
#endif

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (best_id != RT_MISS) o = {best, __uint_as_float(best_id), bu + 0.0f, bv + 0.0f};   // (+ 0: -0 becomes +0)
        p.hits[i] = o;
    }
    if (p.status && __builtin_amdgcn_ballot_w64(overflow) != 0 && lane == 0) atomicOr(p.status, (uint32_t)RT_POINT_STACK_OVERFLOW);
    if (p.counters) {                         // (kernel argument: the same for every thread)
        const uint32_t bsum = wave_sum_u32(box_tests), tsum = wave_sum_u32(tri_tests);
        unsigned long long* const csum = reinterpret_cast<unsigned long long*>(&stack_lds[0][0][0]);
        __syncthreads();                      // every lane is done with its stack column
        if (threadIdx.x < 2) csum[threadIdx.x] = 0ull;
        __syncthreads();
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

}  // namespace

hipError_t launch_point_query(const rt_accel& as, const rt_point_query* queries, rt_point_hit* hits, uint32_t num_queries,
                              uint64_t* counters, uint32_t* status, hipStream_t st)
{
    PointParams p;
    p.nodes = as.nodes;
    p.leaves = as.triangles;
    p.root = as.root;
    p.count = as.count;
    p.queries = reinterpret_cast<const float4*>(queries);
    p.hits = reinterpret_cast<float4*>(hits);
    p.num_queries = num_queries;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    const uint32_t per_block = kTraceWaves * 64;
    const dim3 grid((uint32_t)(((uint64_t)num_queries + per_block - 1) / per_block)), block(per_block);
    point_query_kernel<<<grid, block, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
