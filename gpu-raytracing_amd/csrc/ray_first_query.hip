// ray_first_query.hip -- rt_ray_first_hits: the K nearest crossings of each caller ray inside its [tmin, tmax] window, in
// ascending (t, primitive_id) order, through any tree rt_intersect_rays takes (semantics: rt_abi.h, first-K block; DESIGN
// section 19).  The fixed-length sibling of the all-hit query: row i has exactly k records, one launch, nothing counted,
// scanned or read back.
//
// ray_first_kernel is ray_hits_kernel's frame -- one lane per ray, 64 consecutive rays per wave, kTraceWaves waves (256 rays)
// per workgroup, xcd_chunk_block, the ray in two 16-byte loads, a leaf in four 16-byte requests, rt_traverse.hpp's wave-level
// two phases, exact per-workgroup counters, one status ballot per wave -- with slab() and intersect_tri() of rt_traverse.hpp
// unchanged, and knn_query_kernel's list in the place of the CSR segment.  What is new against the all-hit kernel:
//   * the bound b: the ray's original tmax while the list holds fewer than k records, the k-th record's t once it is full.  A
//     slot is entered iff back >= front && front <= b && back >= tmin; a triangle is tested against [tmin, b] (intersect_tri
//     writes r.tmax on acceptance: the kernel puts b back after every test);
//   * the order: the surviving slot of a run with the smallest front is visited next (ties: the lower slot), the others are
//     pushed -- point_query_kernel's nearest-first step with front in the place of boxdist2 -- so the bound falls as fast as
//     the near hits arrive;
//   * the list: a private array of RT_RAY_FIRST_MAX_K 16-byte records in ascending (t, id) order, written to the row once at
//     the end; m, the k-th (t, id) and b live in registers.  A candidate is first tested against the registers alone: not
//     below the k-th of a full list -- most candidates end there.  A survivor finds its position first (a scan down from the
//     top; an equal (t, id) means the record is already listed -- a split tree holds several references -- and the candidate
//     is dropped) and shifts afterwards.  Plain vector loads and stores at lane-private addresses, no atomics;
//   * a NaN t (an overflowed product that Moller-Trumbore's comparisons let through) orders above every number and NaNs are
//     equal to each other; the bound is never NaN: while the k-th t is NaN it stays the original tmax.
// Pending entries, RT_RAY_FIRST_PENDING (rows on decided rays -- rt_abi.h, claim 2 -- are identical in both arms):
//   4  the entry alone, 16 in an LDS column per lane (16 KB per workgroup: ray_hits_kernel's LDS bound of eight waves per
//      SIMD, of which the list's registers leave six) + 48 private; a pop is not re-culled: the slots of a popped run, and the
//      triangles of a popped leaf, meet the current b anyway;
//   8  (entry, front) in 8 bytes, 16 in an LDS column (32 KB per workgroup: five waves per SIMD) + 48 private; a popped entry
//      is dropped iff front > b with the current b.
// Shipped: 4, by measurement (tools/ray_first_bench.py, profiles/ray_first_bench.json): the re-test saves
// at most 1.5 % of the box tests and the wider entries cost up to 45 % more time.  The other arm is a library build:
// csrc/Makefile's librt_amd_exp.so with EXPFLAGS=-DRT_RAY_FIRST_PENDING=8.
// A push onto a full stack of 64 is dropped and flagged (RT_RAY_FIRST_STACK_OVERFLOW): the row is then a sorted subset of the
// all-hit row.  No restart pass.
// Compiled with -ffp-contract=off and IEEE division: every listed record is bit for bit the one rt_ray_hits_collect emits for
// that triangle.
// FILTERED (rt_ray_first_hits_filtered; rt_abi.h, hit-filter block) is the same traversal with the lane's
// RayFilter (rt_ray_filter.hpp) at the one place where a candidate is accepted, so the bound only ever falls to the t of a
// kept record; the unfiltered arm is the code it was before the filter existed, instruction for instruction.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_ray_filter.hpp"
#include "rt_traverse.hpp"

#include <type_traits>

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 16, "rt_ray: two 16-byte halves; rt_hit: one 16-byte record");
static_assert(rt::kQueryBlock == rt::kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

#ifndef RT_RAY_FIRST_PENDING
#define RT_RAY_FIRST_PENDING 4
#endif
static_assert(RT_RAY_FIRST_PENDING == 8 || RT_RAY_FIRST_PENDING == 4, "RT_RAY_FIRST_PENDING: 4 (entry) or 8 (entry, front)");

namespace rt {

namespace {

constexpr int kRfStackLds = 16;   // LDS-resident entries per lane: 16 x 4 B (or 8 B) x 256 lanes = 16 KB (32 KB) per workgroup

struct RayFirstParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* rays;           // rt_ray = two float4: (origin, tmin), (dir, tmax)
    float4* out;                  // rt_hit = one float4: (t, primitive_id bits, u, v); row i at out + i * k
    uint32_t num_rays, k;
    unsigned long long* counters;
    uint32_t* status;
};
struct FilteredRayFirstParams : RayFirstParams {
    FilterParams filter;
};

#if RT_RAY_FIRST_PENDING == 8
typedef uint64_t RfEntry;         // entry (low word) | front bits (high word)
constexpr int kRfMinWaves = 5;    // 32 KB of LDS per workgroup of 4 waves: 5 workgroups per CU, 5 waves per SIMD
#else
typedef uint32_t RfEntry;
constexpr int kRfMinWaves = 6;    // 16 KB of LDS would allow 8, but 64 VGPRs spill eleven and 72 spill six: 6 waves, no spills
#endif
typedef RfEntry RfSpill[kStackMax - kRfStackLds];
typedef __attribute__((address_space(3))) RfEntry lds_rf_entry;

// (t, id) order with NaN above every number and equal to itself
__device__ __forceinline__ bool rf_same_t(float a, float b) { return a == b || (__builtin_isnan(a) && __builtin_isnan(b)); }
__device__ __forceinline__ bool rf_below(float t, uint32_t id, float et, uint32_t eid)
{
    return t < et || (!__builtin_isnan(t) && __builtin_isnan(et)) || (rf_same_t(t, et) && id < eid);
}

template <bool FILTERED>
__global__ __launch_bounds__(kTraceWaves * 64, kRfMinWaves)
void ray_first_kernel(std::conditional_t<FILTERED, FilteredRayFirstParams, RayFirstParams> p)
{
    // the counters' workgroup sums reuse the stack's LDS once every lane is done with it (no extra bytes)
    __shared__ alignas(8) RfEntry stack_lds[kTraceWaves][kRfStackLds][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_rays;
    const uint32_t k = p.k;

    float4 ra = {0.f, 0.f, 0.f, 0.f}, rb = {0.f, 0.f, 0.f, -1.f};
    if (in_range) { ra = p.rays[2 * i]; rb = p.rays[2 * i + 1]; }
    Ray r;
    r.ox = ra.x; r.oy = ra.y; r.oz = ra.z; r.tmin = ra.w;
    r.dx = rb.x; r.dy = rb.y; r.dz = rb.z; r.tmax = rb.w;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    const float tmax0 = r.tmax;
    // not traced (a row of misses, no tests), rt_intersect_rays's rule: lanes past the batch, an empty or NaN [tmin, tmax], a
    // NaN origin or direction
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    bool live = in_range && r.tmin <= r.tmax && !nan_ray && p.count > 0;
    // the lane's filter is asked inside intersect_tri, before `offer`: a candidate that is turned down never moves the bound.
    // Made HERE, under `if constexpr`, not by a helper function
    std::conditional_t<FILTERED, RayFilter, NoFilter> flt;
    if constexpr (FILTERED) flt = ray_filter(p.filter, i, in_range);

    // the list: m records in ascending (t, id) order.  Only a live lane touches it, and a live lane is in range.
    float4 list[RT_RAY_FIRST_MAX_K];
    uint32_t m = 0;
    float kth_t = __builtin_inff();   // the k-th record, valid once m == k
    uint32_t kth_id = RT_MISS;
    float bound = tmax0;              // tmax while m < k (or while the k-th t is NaN), kth_t after

    lds_rf_entry* const col = (lds_rf_entry*)&stack_lds[wave][0][lane];
    RfSpill spill;
    int sp = 0;
    bool overflow = false;            // a push was dropped: the row is a subset
    uint32_t box_tests = 0, tri_tests = 0;
    uint32_t cur = (p.root & kIndexMask) | (p.count << 29);

    // an accepted triangle (t <= bound, stored weights bu / bv, rotation rot)
    auto offer = [&](float t, uint32_t id, float bu, float bv, uint32_t rot) {
        const bool full = m == k;
        if (full && !rf_below(t, id, kth_t, kth_id)) return;                  // not below the k-th: registers only
        // the position: the records above the candidate are [pos, m); a full list's k-th is above it (the test before)
        const uint32_t top = full ? k - 1 : m;
        uint32_t pos = top;
        while (pos > 0) {
            const float4 e = list[pos - 1];
            const uint32_t eid = __float_as_uint(e.y);
            if (rf_same_t(e.x, t) && eid == id) return;                       // already listed
            if (rf_below(e.x, eid, t, id)) break;
            pos--;
        }
        // the shift, from the top down: [pos, top) -> [pos + 1, top + 1); a full list loses its k-th
        for (uint32_t j = top; j > pos; j--) list[j] = list[j - 1];
        list[pos] = hit_record(t, id, bu, bv, rot);
        m = top + 1;
        if (m == k) {
            if (pos == k - 1) { kth_t = t; kth_id = id; }
            else { const float4 e = list[k - 1]; kth_t = e.x; kth_id = __float_as_uint(e.y); }
            bound = __builtin_isnan(kth_t) ? tmax0 : kth_t;
        }
    };
    // one triangle (leaf corners c0, c1, c2, rotation rot) against [tmin, bound]
    auto test = [&](float c0x, float c0y, float c0z, float c1x, float c1y, float c1z, float c2x, float c2y, float c2z,
                    uint32_t prim, uint32_t rot) {
        Hit h;
        if (intersect_tri(c0x, c0y, c0z, c1x, c1y, c1z, c2x, c2y, c2z, r, h, 0u, prim, flt)) offer(r.tmax, prim, h.bu, h.bv, rot);
        r.tmax = bound;               // intersect_tri shrank it to t: the window's end is the bound, nothing else
    };
    auto next_from_stack = [&]() {
#if RT_RAY_FIRST_PENDING == 8
        while (sp > 0) {              // re-culled against the current bound, never on equality
            --sp;
            const RfEntry se = sp < kRfStackLds ? col[sp * 64] : spill[sp - kRfStackLds];
            if (__uint_as_float((uint32_t)(se >> 32)) <= bound) { cur = (uint32_t)se; return; }
        }
        live = false;
#else
        if (sp == 0) { live = false; return; }
        --sp;
        cur = sp < kRfStackLds ? col[sp * 64] : spill[sp - kRfStackLds];
#endif
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
        uint32_t near_e = kNoNear;
        float near_f = __builtin_inff();
        for (uint32_t s = 0; s < cnt; s++) {
            const uint4* np = reinterpret_cast<const uint4*>(p.nodes + first + s);
            const uint4 a = np[0], b = np[1];
            const uint32_t type = b.w >> 29;
            if (type == RT_CHILD_NONE) continue;
            box_tests++;
            const uint32_t e = slot_entry(a, b);
            float front, back;
            slab(a, b, r, front, back);
            const bool in = (back >= front) & (front <= bound) & (back >= r.tmin);
            if (!in || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // missed or pruned, or an empty run
            uint32_t pe = e;
            float pf = front;
            if (front < near_f) {             // the new nearest; the old one (if any) is pushed
                pe = near_e; pf = near_f;
                near_e = e; near_f = front;
            }
            if (pe != kNoNear) {
#if RT_RAY_FIRST_PENDING == 8
                const RfEntry se = (uint64_t)pe | ((uint64_t)__float_as_uint(pf) << 32);
#else
                const RfEntry se = pe;
                (void)pf;
#endif
                if (sp < kRfStackLds) col[sp * 64] = se;
                else if (sp < kStackMax) spill[sp - kRfStackLds] = se;
                else overflow = true;         // dropped: what lies below it is missing from the row
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
        float4* const row = p.out + i * k;
        const float4 miss = {__builtin_inff(), __uint_as_float((uint32_t)RT_MISS), 0.0f, 0.0f};
        for (uint32_t j = 0; j < k; j++) row[j] = j < m ? list[j] : miss;
    }
    if (p.status && __builtin_amdgcn_ballot_w64(overflow) != 0 && lane == 0)
        atomicOr(p.status, (uint32_t)RT_RAY_FIRST_STACK_OVERFLOW);
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

hipError_t launch_ray_first_hits(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, uint32_t k,
                                 const rt_hit_filter* filter, rt_hit* out, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    FilteredRayFirstParams p;
    set_tree(p, as);
    p.rays = reinterpret_cast<const float4*>(rays);
    p.out = reinterpret_cast<float4*>(out);
    p.num_rays = num_rays;
    p.k = k;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    const dim3 grid(query_blocks(num_rays)), block(kQueryBlock);
    if (filter) {
        p.filter = filter_params(*filter);
        ray_first_kernel<true><<<grid, block, 0, st>>>(p);
    } else ray_first_kernel<false><<<grid, block, 0, st>>>(p);   // (its RayFirstParams part)
    return hipGetLastError();
}

}  // namespace rt
