// ray_first_instanced_query.hip -- rt_ray_first_hits_instanced: the K nearest crossings of each caller ray inside its
// [tmin, tmax] window in a scene of placed copies of built trees, in ascending (t, instance, primitive_id) order, each record
// with the instance it lies in (semantics: rt_abi.h, instanced first-K block).  The fixed-length sibling of
// the instanced all-hit query: row i has exactly k records and k instance ids, one launch, nothing counted, scanned or read back.
//
// ray_first_instanced_kernel is ray_first_kernel's frame (ray_first_query.hip) with ray_hits_instanced_kernel's second level
// (ray_hits_instanced_query.hip) written into its loop.  From ray_first_kernel: one lane per ray, 256 rays per workgroup,
// xcd_chunk_block, the bound b (the original tmax while the list holds fewer than k items, the k-th item's t after; never NaN),
// the nearest-first step (the surviving slot of a run with the smallest front goes next, ties to the lower slot, the others are
// pushed), the shipped 4-byte pending entries (16 in an LDS column per lane + 48 private, a pop is not re-tested), the
// wave-level two phases, the private list written to the row once at the end, the counter and status reductions.  From
// ray_hits_instanced_kernel: per-lane node and leaf base pointers, `inst` (kTop in the TLAS), `base` (the stack depth at which
// the lane entered its BLAS), `leaving`, the record load and load_accel, the enter arithmetic, load_world_ray on exit; an
// entry of count 0 is an instance to enter in the TLAS and a leaf record to test inside a BLAS, and the leaf phase runs the
// lane's BLAS leaf, its exit and its entry in this order.  What the two make together:
//   * ONE bound for both levels: an affine map keeps t, so b prunes TLAS slots against the world ray and BLAS slots against
//     the object ray without conversion (a slot is entered iff back >= front && front <= b && back >= tmin), and a triangle is
//     tested against [tmin, b] (intersect_tri writes r.tmax on acceptance: the kernel puts b back after every test, and the
//     reload of the world ray on exit leaves r.tmax, the bound, alone);
//   * nearest first on both levels, and an instance is walked to the end before the next TLAS entry is popped (its entries lie
//     above `base`), so the bound the near instances leave prunes the far ones in the TLAS;
//   * the list holds 20 bytes an item: the 16-byte hit records as in ray_first_kernel and the instances in a PARALLEL array of
//     4-byte words (the records keep their one 16-byte load / store each, the shift moves the two arrays in one loop; a 32-byte
//     record would double the list's private bytes for 4 useful ones).  m, the k-th (t, instance, id) and b live in registers;
//     a candidate is first tested against the registers alone;
//   * a popped TLAS entry is NOT re-tested against the current b before its instance is entered: the 4-byte entry carries no
//     front, re-computing it means re-loading the TLAS slot the entry came from (its address is not in the entry), and the 8-byte
//     arm that would carry it cost ray_first_kernel up to 45 % for 1.5 % of the box tests.  The entered instance's root run meets
//     the current b at once, so a stale entry costs one record load, one transform and the slab tests of one run.
// A push onto a full stack of 64 (both levels together) is dropped and flagged (RT_RAY_FIRST_STACK_OVERFLOW): the row is then
// a sorted subset of the instanced all-hit row.  No restart pass, no 8-byte pending arm.
// FILTERED (rt_ray_first_hits_instanced_filtered; rt_abi.h, instanced set-filter block) is the same traversal
// with the lane's InstanceRayFilter (rt_instance_filter.hpp): enter(id) is asked at the TLAS leaf before the record is read
// (a popped entry of a masked instance goes on in the TLAS), set_instance once the rows are in registers, and `tri` is
// intersect_tri's policy at its one acceptance point -- BEFORE the offer, so a rejected crossing never enters the list and
// never moves the bound.
// Compiled with -ffp-contract=off and IEEE division: every listed item is bit for bit the one rt_ray_hits_collect_instanced
// emits for that instance and triangle.
#include "rt_device.hpp"
#include "rt_instance_filter.hpp"
#include "rt_instance_traverse.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

#include <type_traits>

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 16, "rt_ray: two 16-byte halves; rt_hit: one 16-byte record");
static_assert(sizeof(rt_instance_record) == 64 && sizeof(rt_accel) == 24, "the record and table entry trace_instanced loads");
static_assert(rt::kQueryBlock == rt::kTraceWaves * 64, "rt_launch.hpp: one lane per ray, kTraceWaves waves per workgroup");

// waves per SIMD the register allocation must fit.  5 is the largest bound that spills nothing (96 VGPRs); 6 (80 VGPRs, 29
// spilled) measured faster on an MI355X in 11 of 12 (builder, ray set, k) cells and ships (DESIGN section 30 has the table of
// bounds 3 to 8 and both sets of numbers)
#ifndef RT_RAY_FIRST_INSTANCED_WAVES
#define RT_RAY_FIRST_INSTANCED_WAVES 6
#endif
// the FILTERED arm keeps six more values live per lane and has its own bound.  6, the sibling's (80 VGPRs, 42 spilled), ships:
// 7 (72 VGPRs, 53 spilled) measured up to 4 % faster on an MI355X at k = 1 and 4 and on incoherent rays, and 3 to 12 % slower
// on coherent rays at k = 32; 5 loses to 6 in ten of twelve cells (DESIGN section 31 has the tables)
#ifndef RT_RAY_FIRST_INSTANCED_FILTERED_WAVES
#define RT_RAY_FIRST_INSTANCED_FILTERED_WAVES 6
#endif

namespace rt {

namespace {

constexpr int kRayFirstInstancedWaves = RT_RAY_FIRST_INSTANCED_WAVES;
constexpr int kRayFirstInstancedFilteredWaves = RT_RAY_FIRST_INSTANCED_FILTERED_WAVES;
constexpr int kRfiStackLds = 16;  // LDS-resident entries per lane: 16 x 4 B x 256 lanes = 16 KB per workgroup

// InstParams's fields as trace_instanced reads them (hits: rt_hit as one float4, row i at hits + i * k; instance_ids: parallel)
struct RayFirstInstParams : InstParams {
    uint32_t k;
    uint32_t* status;
};
struct FilteredRayFirstInstParams : RayFirstInstParams {
    InstanceFilterParams filter;
};

typedef uint32_t RfiSpill[kStackMax - kRfiStackLds];

// (t, instance, id) order with NaN above every number and equal to itself
__device__ __forceinline__ bool rfi_same_t(float a, float b) { return a == b || (__builtin_isnan(a) && __builtin_isnan(b)); }
__device__ __forceinline__ bool rfi_below(float t, uint32_t in, uint32_t id, float et, uint32_t ein, uint32_t eid)
{
    return t < et || (!__builtin_isnan(t) && __builtin_isnan(et)) || (rfi_same_t(t, et) && (in < ein || (in == ein && id < eid)));
}

template <bool FILTERED>
__global__ __launch_bounds__(kTraceWaves * 64, FILTERED ? kRayFirstInstancedFilteredWaves : kRayFirstInstancedWaves)
void ray_first_instanced_kernel(std::conditional_t<FILTERED, FilteredRayFirstInstParams, RayFirstInstParams> p)
{
    // the counters' workgroup sums reuse the stack's LDS once every lane is done with it (no extra bytes)
    __shared__ alignas(8) uint32_t stack_lds[kTraceWaves][kRfiStackLds][64];
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
    // not traced (a row of pads, no tests), the first-K rule: lanes past the batch, an empty or NaN [tmin, tmax], a NaN origin or
    // direction; and every ray of a scene without instances or with an empty TLAS
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    bool live = in_range && r.tmin <= r.tmax && !nan_ray && p.count > 0 && p.num_instances > 0;

    // the list: m items in ascending (t, instance, id) order, records and instances in parallel arrays.  Only a live lane touches
    // it, and a live lane is in range.
    float4 list[RT_RAY_FIRST_MAX_K];
    uint32_t list_inst[RT_RAY_FIRST_MAX_K];
    uint32_t m = 0;
    float kth_t = __builtin_inff();   // the k-th item, valid once m == k
    uint32_t kth_inst = RT_MISS, kth_id = RT_MISS;
    float bound = tmax0;              // tmax while m < k (or while the k-th t is NaN), kth_t after

    lds_u32* const col = (lds_u32*)&stack_lds[wave][0][lane];
    RfiSpill spill;
    int sp = 0;
    bool overflow = false;            // a push was dropped: the row is a subset
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

    // an accepted triangle of the lane's instance (t <= bound, stored weights bu / bv, rotation rot)
    auto offer = [&](float t, uint32_t id, float bu, float bv, uint32_t rot) {
        const bool full = m == k;
        if (full && !rfi_below(t, inst, id, kth_t, kth_inst, kth_id)) return;   // not below the k-th: registers only
        // the position: the items above the candidate are [pos, m); a full list's k-th is above it (the test before)
        const uint32_t top = full ? k - 1 : m;
        uint32_t pos = top;
        while (pos > 0) {
            const float4 e = list[pos - 1];
            const uint32_t ein = list_inst[pos - 1], eid = __float_as_uint(e.y);
            if (rfi_same_t(e.x, t) && ein == inst && eid == id) return;         // already listed (a split BLAS)
            if (rfi_below(e.x, ein, eid, t, inst, id)) break;
            pos--;
        }
        // the shift, from the top down: [pos, top) -> [pos + 1, top + 1); a full list loses its k-th
        for (uint32_t j = top; j > pos; j--) { list[j] = list[j - 1]; list_inst[j] = list_inst[j - 1]; }
        list[pos] = hit_record(t, id, bu, bv, rot);
        list_inst[pos] = inst;
        m = top + 1;
        if (m == k) {
            if (pos == k - 1) { kth_t = t; kth_inst = inst; kth_id = id; }
            else { const float4 e = list[k - 1]; kth_t = e.x; kth_inst = list_inst[k - 1]; kth_id = __float_as_uint(e.y); }
            bound = __builtin_isnan(kth_t) ? tmax0 : kth_t;
        }
    };
    // one triangle (leaf corners c0, c1, c2, rotation rot) against [tmin, bound]
    auto test = [&](float c0x, float c0y, float c0z, float c1x, float c1y, float c1z, float c2x, float c2y, float c2z,
                    uint32_t prim, uint32_t rot) {
        Hit h;
        if constexpr (FILTERED) {
            if (intersect_tri(c0x, c0y, c0z, c1x, c1y, c1z, c2x, c2y, c2z, r, h, 0u, prim, flt.tri))
                offer(r.tmax, prim, h.bu, h.bv, rot);
        } else {
            if (intersect_tri(c0x, c0y, c0z, c1x, c1y, c1z, c2x, c2y, c2z, r, h, 0u, prim)) offer(r.tmax, prim, h.bu, h.bv, rot);
        }
        r.tmax = bound;               // intersect_tri shrank it to t: the window's end is the bound, nothing else
    };
    auto next_from_stack = [&]() {
        if (sp == base) {
            if (inst == kTop) live = false;
            else leaving = true;
            return;
        }
        --sp;
        cur = sp < kRfiStackLds ? col[sp * 64] : spill[sp - kRfiStackLds];
    };
    auto leaf_step = [&]() {
        tri_tests++;
        uint4 l0, l1, l2, l3;
        load_leaf_wide(leaves + (cur & kIndexMask), l0, l1, l2, l3);
        test(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
             __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), l0.w, l2.w & 0xFFFFu);
        // triangle B = (v2, v1, v3); for a single triangle v3 == v2 bit for bit and B is skipped (as ray_first_kernel)
        if (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z)
            test(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                 __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                 __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z), l1.w, l2.w >> 16);
        next_from_stack();
    };
    // a run of the lane's current tree, nearest first.  In the TLAS a triangle slot that passes is an instance entry (leaf
    // index : 29 | 0), ordered by its proxy's front like any other slot
    auto box_step = [&]() {
        const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
        uint32_t near_e = kNoNear;
        float near_f = __builtin_inff();
        for (uint32_t s = 0; s < cnt; s++) {
            const uint4* np = reinterpret_cast<const uint4*>(nodes + first + s);
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
            if (front < near_f) {             // the new nearest; the old one (if any) is pushed
                pe = near_e;
                near_e = e; near_f = front;
            }
            if (pe != kNoNear) {
                if (sp < kRfiStackLds) col[sp * 64] = pe;
                else if (sp < kStackMax) spill[sp - kRfiStackLds] = pe;
                else overflow = true;         // dropped: what lies below it is missing from the row
                sp = min(sp + 1, kStackMax);
            }
        }
        if (near_e != kNoNear) cur = near_e;
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
                load_world_ray(p, i, r);      // (r.tmin and r.tmax, the bound, are not the transform's and stay)
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

    if (in_range) {
        float4* const row = p.hits + i * k;
        uint32_t* const row_ids = p.instance_ids + i * k;
        const float4 miss = {__builtin_inff(), __uint_as_float((uint32_t)RT_MISS), 0.0f, 0.0f};
        for (uint32_t j = 0; j < k; j++) {
            row[j] = j < m ? list[j] : miss;
            row_ids[j] = j < m ? list_inst[j] : (uint32_t)RT_MISS;
        }
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

hipError_t launch_ray_first_hits_instanced(const InstanceQuery& q, uint32_t k, const rt_instance_hit_filter* filter,
                                           uint32_t* status, hipStream_t st)
{
    FilteredRayFirstInstParams p = {};
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
    p.k = k;
    p.status = status;
    const dim3 grid(query_blocks(q.num_rays)), block(kQueryBlock);
    if (filter) {
        p.filter = instance_filter_params(*filter);
        ray_first_instanced_kernel<true><<<grid, block, 0, st>>>(p);
    } else {
        ray_first_instanced_kernel<false><<<grid, block, 0, st>>>(p);   // (its RayFirstInstParams part)
    }
    return hipGetLastError();
}

}  // namespace rt
