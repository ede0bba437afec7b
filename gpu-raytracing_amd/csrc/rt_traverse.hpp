// rt_traverse.hpp -- the per-ray BVH traversal shared by trace_kernel.hip (camera rays + shading) and ray_query.hip (caller
// rays -> hit records): Ray / Hit, Moller-Trumbore, the slab test, the lane state and the wave-level two-phase loop
// trace_ray, plus the primary-ray setup of TraceRays.  Semantics and machine mapping: see trace_kernel.hip's header.
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"
#include "rt_math.h"

namespace rt {

constexpr int kStackLds = 16;    // LDS-resident stack entries per lane (bench scenes peak at 10)
constexpr int kStackMax = 64;    // reference stack size (Tracer.cu:314)
constexpr uint32_t kPrefetchMinPrims = 8u << 20;   // scenes from here on take the pair-prefetch instantiation (see trace_kernel)
#ifndef RT_TRACE_WAVES
#define RT_TRACE_WAVES 4
#endif
constexpr int kTraceWaves = RT_TRACE_WAVES;   // waves (8x8 tiles) per workgroup
#ifndef RT_TRACE_MIN_WAVES
#define RT_TRACE_MIN_WAVES 7   // waves per SIMD the register allocator must fit (72 VGPRs: no spills; 8 -> 64 VGPRs spills)
#endif
// kernels without shading (trace_kernel's kDepth / kBoxtests / kTriangleTests, ray_query_kernel) fit 64 VGPRs: one wave more
// per SIMD.  (RT_TRACE_LEAN_EXTRA = 0 is the compile-time arm of tools/trace_spill_experiment.sh, which priced the spills of
// the 64-VGPR instantiations: see DESIGN section 5)
#ifndef RT_TRACE_LEAN_EXTRA
#define RT_TRACE_LEAN_EXTRA 1
#endif
#ifndef RT_TRACE_PF_WAVES
#define RT_TRACE_PF_WAVES 5    // waves per SIMD of the pair-prefetch (PF) instantiations
#endif
// (The experiment arms this loop once carried -- wave-shared pairs through the scalar path, a narrowed leaf fetch, a second
// hold test per vote and others -- lost their measurements and were retired; numbers, and the commit that still builds
// them: DESIGN section 5.)

// the wave runs a box step while  stepping * park_den >= parked * park_num  (else one leaf phase)
constexpr int kParkNum = 8, kParkDen = 1;   // (round-2 sweep under the chunked XCD order, tools/sweep_park.sh: 4..8 equal on the 1080p LBVH frame; 4 is +5 % on the SAH tree but -4 % on the 4K x 16 spp frame)

// Workgroup order vs XCDs: hardware deals workgroup b to XCD b % 8.  XCD x takes chunks of kXcdChunk consecutive workgroups
// (for trace_kernel 8 x 4 tiles = a 256 x 8 pixel run: neighbouring rays meet in one L2) dealt round-robin over the whole
// frame, so every XCD sees every region of the image.  (Round 1 gave each XCD one contiguous eighth of the frame: fine for a
// uniform view, but a view whose cost is concentrated in part of the frame -- camera B: the foreground rows -- then
// runs on two or three XCDs while the others idle: 1297 vs 3490 Mrays/s serial, 2548 vs 5397 with frames in flight.)
// RT_TRACE_XCD_CHUNK overrides the chunk at compile time (tools/xcd_chunk_experiment.sh).  Returns the virtual block.
#ifndef RT_TRACE_XCD_CHUNK
#define RT_TRACE_XCD_CHUNK 8
#endif
__device__ __forceinline__ uint32_t xcd_chunk_block(uint32_t bid, uint32_t nb)
{
    constexpr uint32_t kXcdChunk = RT_TRACE_XCD_CHUNK;
    const uint32_t full = nb / (8u * kXcdChunk) * (8u * kXcdChunk);   // (the last < 8 * chunk workgroups keep their index)
    const uint32_t xcd = bid & 7u, loc = bid >> 3;
    return bid < full ? (loc / kXcdChunk) * (8u * kXcdChunk) + xcd * kXcdChunk + (loc % kXcdChunk) : bid;
}

typedef __attribute__((address_space(3))) uint32_t lds_u32;

struct Ray {
    float ox, oy, oz, dx, dy, dz, ix, iy, iz, tmin, tmax;
};
struct Hit {
    uint32_t primitive_id, tri_id;
    float bu, bv;
};

// The hit-filter policy of intersect_tri / trace_ray.  NoFilter: every triangle Moller-Trumbore accepts is accepted (all
// existing kernels; `if constexpr` leaves no trace of the policy in them).  A policy with active = true (rt_ray_filter.hpp)
// supplies keep(a, primitive_id), asked after the t window test and before r.tmax is written: a candidate it turns down is a
// candidate the leaf test rejected.  The object travels by value: handed down by reference, even the empty NoFilter changed the
// code of existing kernels.
struct NoFilter {
    static constexpr bool active = false;
};

// Tracer.cu:256-291
template <class Filter = NoFilter>
__device__ __forceinline__ bool intersect_tri(float v0x, float v0y, float v0z, float v1x, float v1y, float v1z,
                                              float v2x, float v2y, float v2z, Ray& r, Hit& h, uint32_t tri_id,
                                              uint32_t prim_id, Filter flt = Filter())
{
    const float epsilon = 0.000000001f;
    const float e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;
    const float e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;
    const float hx = r.dy * e2z - r.dz * e2y, hy = r.dz * e2x - r.dx * e2z, hz = r.dx * e2y - r.dy * e2x;
    const float a = e1x * hx + e1y * hy + e1z * hz;
    if (a > -epsilon && a < epsilon) return false;
    const float f = 1.0f / a;
    const float sx = r.ox - v0x, sy = r.oy - v0y, sz = r.oz - v0z;
    const float u = f * (sx * hx + sy * hy + sz * hz);
    if (u < 0.0f || u > 1.0f) return false;
    const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    const float v = f * (r.dx * qx + r.dy * qy + r.dz * qz);
    if (v < 0.0f || (u + v) > 1.0f) return false;
    const float t = f * (e2x * qx + e2y * qy + e2z * qz);
    if (t < r.tmin || t > r.tmax) return false;
    if constexpr (Filter::active) {
        if (!flt.keep(a, prim_id)) return false;
    }
    r.tmax = t;
    h.primitive_id = prim_id;
    h.tri_id = tri_id;
    h.bu = u;
    h.bv = v;
    return true;
}

// Hold at pop (trace_ray<.., QW = true>; 0 here builds every kernel without it, the parent arm of tools/quad_wait_arms.sh):
// a lane that has just popped entry E from level s of its stack takes no box step while a quad-mate still holds E at level s
// of its own stack -- the mate is deeper in the subtree both took first, and when it pops E the two step on E with one
// address, which the address path charges as one request (quad_hold below).  The rule is evaluated once per
// vote: the second box step under the vote steps every lane in PH_STEP.  (Which kernels take it at 1 and 2: trace_kernel.hip.
// Shipped since: quad_hold_sp, the same rule on the stack depths alone, before BOTH steps -- RT_TRACE_HOLD_FIRST / _SECOND below.)
#ifndef RT_TRACE_QUAD_WAIT
#define RT_TRACE_QUAD_WAIT 1
#endif

// The lean vote (trace_ray<.., QW = true> only).  A vote under which no unfinished lane has more than kStackLds - kLeanMargin
// entries on its stack is LEAN: every push / pop site of its box steps -- and of the leaf phase that follows it, if the vote
// ends the box phase -- takes a scalar branch on the vote's wave-uniform flag (`lean`) straight to the LDS column, with no
// sp < kStackLds ladder, no private array and no kStackMax clamp.  Any other vote runs the full ladders.  One stack, one sp: a
// wave may change arm at every vote, and no ray's sequence of tests depends on the arm.
// The margin: a lean push at sp writes lds[sp * 64], so every push under the vote must find sp <= kStackLds - 1.  A box step
// pushes at most TWO entries (a pair entered with `near` set, inside a node of more than two slots; else one), advance() only
// pops, and a vote runs two box steps: a lane that starts it at sp pushes at levels sp .. sp + 3 at most.  A vote that ends
// the box phase runs no box step; the leaf phase's second_slot pushes at most one entry, at level sp.  Hence kLeanMargin =
// 2 steps x 2 pushes = 4, and a lean vote never sees sp above kStackLds (< kStackMax: its pops always read LDS).
// RT_TRACE_LEAN_STEP: 2 (shipped) as above, -3.1 % issued instructions, +1.6 % on the headline; 0 every vote runs the full
// ladders (`lean` is never set and folds away).  DESIGN section 5, profiles/lean_step_bench.txt.
#ifndef RT_TRACE_LEAN_STEP
#define RT_TRACE_LEAN_STEP 2
#endif
constexpr int kLeanStep = RT_TRACE_LEAN_STEP;
// (1 was the two-copy arm, -1.9 %: retired, its numbers are in profiles/lean_step_bench.txt)
static_assert(kLeanStep == 0 || kLeanStep == 2, "RT_TRACE_LEAN_STEP is 0 (full ladders) or 2 (shipped); arm 1 was retired");
constexpr int kLeanMargin = 4;
static_assert(kLeanMargin <= kStackLds, "the lean vote's threshold is a stack level");

// The pair-local step (trace_ray<.., QW = true> only; pair_step_on below).  near_e / near_d are carried from box step to box
// step, but advance() resets them at the end of every pair unless the node has more than two slots: in an LBVH, a pairs
// tree or a hybrid tree EVERY pair is entered with near_e == kNoNear.  For such a pair slot 0's push site is dead, its
// `closer` test compares against +inf and the nearest child never leaves the step: the pair-local form decides slot 0,
// slot 1, the one possible push and the advance from values of the step alone, and writes near_e / near_d only where
// they outlive it (a leaf in slot 1, the first pair of a node of more than two slots).  A ray's sequence of tests, pushes
// and pops is the general form's.
// A vote is NARROW iff no unfinished lane -- stepping, held or parked -- has (cur >> 29) > 2 or near_e != kNoNear.  A narrow
// vote runs both of its steps in the pair-local form, any other vote today's general step.  Why no lane of a narrow vote
// starts a step with a carried near: at the vote no lane's cur is wider than a pair and none carries a near.  A lane's first
// step ends in advance -- near_e untouched, still kNoNear -- or in a park, and a parked lane takes no second step.  The cur
// it advances to may be a node of more than two slots: the lane steps that node's FIRST pair in the second step at the
// earliest, near_e == kNoNear as the form asks, and the form's tail leaves the near in near_e / near_d and cur on the
// node's next pair.  That carried near makes the next vote a general one, and a general vote steps anything.  A lane freed by
// a leaf phase comes back with whatever second_slot / advance left: counted by the next vote like any other.  (A parked lane
// takes neither step of a vote, so the rule could leave it out -- a lane parked in PH_LEAF1 often carries a near and makes
// the votes it sits out general ones.  Measured as a second arm: 100 % instead of 99.2 % narrow votes on the bench frame
// and no different in time on any workload, profiles/pair_step_bench.txt; the rule counts every unfinished lane.)
// The lean margin is untouched: the pair-local form pushes at most once per step.  Nothing in either form makes a lane wait
// (quad_hold's progress argument holds word for word); one traversal state and one sp, so a wave may change form at every
// vote.  How the two forms are laid out in the loop, and why: at the vote in trace_ray and profiles/pair_step_asm.txt.
//   2 (shipped)  the EXACT vote below replaces the narrow one as the condition of the pair-local form: two forms, no TAIL, no
//                lone slot, the pair fetched at a 32-bit offset: +1.0 % on the headline over 1, +6 % at 16 spp (DESIGN section 5,
//                profiles/exact_pair_bench.txt);
//   1            narrow votes run the pair-local form: -7.8 % issued instructions, +3.6 % on the headline over 0;
//   0            every vote runs the general step: the loop before this knob, instruction for instruction.
#ifndef RT_TRACE_PAIR_STEP
#define RT_TRACE_PAIR_STEP 2
#endif
constexpr int kPairStep = RT_TRACE_PAIR_STEP;
static_assert(kPairStep >= 0 && kPairStep <= 2, "RT_TRACE_PAIR_STEP is 0 (general step), 1 (narrow vote) or 2 (exact vote)");

// The exact vote (kPairStep == 2).  launch_trace gets a node pointer, not a node count, so the kernel cannot know at launch
// that every pair lies within 4 GiB of p.nodes; the vote establishes it from the data.  A cur is EXACT when its count is 2
// and its index is at most 2^27 - 2: then cur << 5 is the pair's byte offset without wrapping 32 bits, the pair's 64 bytes
// end below 4 GiB, and the four loads are scalar base + one 32-bit lane offset + 0 / 16 / 32 / 48 -- no 64-bit arithmetic, no
// `two`, no second address.  One compare on the packed word: count 2 is bit 30 alone, so cur - 2^30 is the index.
// A vote is exact iff no unfinished lane carries a near and every unfinished lane's cur is exact (the lane set the narrow
// rule counts).  An exact vote runs both steps in the pair-local form on the short address; any other vote the general step.
// The vote has only seen the cur a lane brought to it.  After the first step cur is a popped entry or the near child: anything.
// The second step's lane mask is therefore PH_STEP && exact_cur(cur): a lane whose new cur is a lone slot, a node of more
// than two slots or a pair beyond the edge sits the step out, as a held lane sits out the first.  So the form has no TAIL
// and no lone slot, and no lane of an exact vote starts a step with a carried near: the first step ends in advance (near_e
// untouched) or a park, and the second writes near_e only when it parks.  Each ray's sequence of tests, pushes and pops is
// the general form's; only the interleaving across lanes changes.
// Progress (beside quad_hold's argument): a lane that sits out is in PH_STEP / PH_STEP_POP with an inexact cur, so it is
// unfinished and makes the NEXT vote a general one.  A general vote steps every lane in PH_STEP that is not held, and for
// those the hold rule's own argument is unchanged: the unfinished lane of a quad with the greatest sp never holds.  An exact
// vote itself steps every lane of `stepping` in its first step (all exact, and a vote is taken only with stepping != 0), so
// every pass of the loop still steps a lane or runs a leaf phase, and no lane sits out two votes in a row for this rule.
constexpr uint32_t kExactIndices = 0x07FFFFFFu;   // 2^27 - 1: the pair indices whose 64 bytes end at or below 4 GiB
static_assert(((uint64_t)(kExactIndices - 1) << 5) + 64 <= (1ull << 32), "the last exact pair ends at 4 GiB");
__device__ __forceinline__ bool exact_cur(uint32_t cur) { return (cur - (2u << 29)) < kExactIndices; }

// per-lane traversal state.  PH_STEP_POP (QW traversals only): PH_STEP whose cur was popped from the stack, from level sp.
enum : uint32_t { PH_STEP = 0, PH_LEAF0 = 1, PH_LEAF1 = 2, PH_DONE = 3, PH_STEP_POP = 4 };
constexpr uint32_t kNoNear = 0xFFFFFFFFu;  // "no Box child hit yet" (child 2^29-1, count 7: not a real entry)

// The private spill array is NOT a member: a dynamically indexed member would pin the whole struct in scratch.
typedef uint32_t SpillArray[kStackMax - kStackLds];

struct Trav {
    lds_u32* lds;  // this lane's stack column: entry k at lds[k * 64]
    uint32_t* spill;
    int sp;
    uint32_t cur;       // slots still to visit of the current node: first slot : 29 | slot count : 3
    uint32_t near_e;    // nearest Box child so far (packed like cur) or kNoNear.  Outlives a box step only inside a node of more
    float near_d;       // than two slots or across a leaf test; the pair-local step writes the two only then.  near_d: its front distance (+inf while kNoNear)
    uint32_t phase;
    uint32_t leaf;      // pending leaf: index : 29 | count : 3
    // second slot of the current pair, kept while parked in PH_LEAF0
    float f1, k1;       // front / back
    uint32_t e1;        // child : 29 | count : 3
    uint32_t t1;        // type, 0 = none / absent
    uint32_t box_tests, tri_tests;
    // PF instantiations only (scenes whose tree does not fit the caches, see launch_trace): the next pair's four 16-byte
    // loads, issued as soon as advance() has picked it -- before the wave's next vote -- and carried in registers
    uint4 pf0, pf1, pf2, pf3;

    // `lean` (here and below): the vote's wave-uniform flag (kLeanMargin); a site takes its LDS-only form under it, else its ladder
    __device__ __forceinline__ void push(uint32_t e, bool lean = false)
    {
        if (lean) { lds[sp * 64] = e; sp++; }
        else {
            if (sp < kStackLds) lds[sp * 64] = e;
            else if (sp < kStackMax) spill[sp - kStackLds] = e;
            sp = min(sp + 1, kStackMax);  // a push onto a full stack is dropped (the reference overruns its array, Tracer.cu:353-369)
        }
    }
    // the pop ladder: an empty stack ends the ray, else the top entry becomes cur.  QW: a popped cur is marked (PH_STEP_POP).
    template <bool QW>
    __device__ __forceinline__ void pop_or_done(bool lean)
    {
        if (sp == 0) phase = PH_DONE;
        else {
            --sp;
            if (lean) cur = lds[sp * 64];
            else cur = sp < kStackLds ? lds[sp * 64] : spill[sp - kStackLds];
            if constexpr (QW) phase = PH_STEP_POP;
        }
    }
    // A Box child (Tracer.cu:338-363), predicated on `in`: the first hit becomes `near`; a closer one (ties:
    // larger child index) displaces `near` onto the stack; otherwise it is pushed itself.  Bitwise logic on
    // purpose (no short-circuit branches); with no near yet near_d = +inf makes every hit "closer".
    __device__ __forceinline__ void inner_hit(bool in, uint32_t e, float front, bool lean = false)
    {
        const bool closer = (front < near_d) | ((front == near_d) & ((e & kIndexMask) > (near_e & kIndexMask)));
        if (in & (near_e != kNoNear)) push(closer ? near_e : e, lean);
        const bool take = in & closer;
        near_e = take ? e : near_e;
        near_d = take ? front : near_d;
    }
    // the current pair is finished: remaining slots of the same node (count > 2 only, never in an LBVH), else
    // the nearest child (the reference pushes it last and pops it first -- so on a FULL stack that push is dropped
    // like any other and the entry below it is popped instead: same rule as the oracle), else a popped entry, else done
    // (pop_or_done).  The lane is in PH_STEP when it gets here.
    template <bool QW = false>
    __device__ __forceinline__ void advance(bool lean = false)
    {
        const uint32_t cnt = cur >> 29;
        if (cnt > 2) { cur = ((cur & kIndexMask) + 2) | ((cnt - 2) << 29); return; }
        const bool keep = (near_e != kNoNear) & (sp < kStackMax);
        if (keep) cur = near_e;
        else pop_or_done<QW>(lean);
        near_e = kNoNear;
        near_d = __builtin_inff();
    }
    // second slot of the pair, evaluated with the CURRENT tmax (after any leaf hit of the first slot)
    __device__ __forceinline__ void second_slot(float tmin, float tmax, bool lean = false)
    {
        const bool valid = t1 != RT_CHILD_NONE;
        const bool hit = valid & (k1 >= f1) & (f1 <= tmax) & (k1 >= tmin);
        box_tests += valid ? 1u : 0u;
        const bool is_leaf = hit & (t1 == RT_CHILD_TRI);
        inner_hit(hit & !is_leaf, e1, f1, lean);
        if (is_leaf) { leaf = e1; phase = PH_LEAF1; }
    }
};

// IntersectRayAabb without the tmax/tmin comparisons (Tracer.cu:187-197): front/back of one slot
__device__ __forceinline__ void slab(const uint4& a, const uint4& b, const Ray& r, float& front, float& back)
{
    // x and y go through v_pk_add_f32 / v_pk_mul_f32 (two IEEE f32 ops per instruction, same rounding)
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f o2 = {r.ox, r.oy}, i2 = {r.ix, r.iy};
    const v2f lo = {__uint_as_float(a.x), __uint_as_float(a.y)}, hi = {__uint_as_float(b.x), __uint_as_float(b.y)};
    const v2f t1 = (lo - o2) * i2, t2 = (hi - o2) * i2;
    const float t1z = (__uint_as_float(a.z) - r.oz) * r.iz, t2z = (__uint_as_float(b.z) - r.oz) * r.iz;
    front = fmaxf(fmaxf(fminf(t1.x, t2.x), fminf(t1.y, t2.y)), fminf(t1z, t2z));
    back = fminf(fminf(fmaxf(t1.x, t2.x), fmaxf(t1.y, t2.y)), fmaxf(t1z, t2z));
}

template <bool PF, class Params>
__device__ __forceinline__ void prefetch_pair(const Params& p, Trav& t)
{
    if constexpr (PF) {
        if (t.phase == PH_STEP) {
            const uint4* np = reinterpret_cast<const uint4*>(p.nodes + (t.cur & kIndexMask));
            const int o1 = (t.cur >> 29) > 1 ? 2 : 0;
            t.pf0 = np[0]; t.pf1 = np[1]; t.pf2 = np[o1]; t.pf3 = np[o1 + 1];
        }
    }
}

// The tests of one box step on a fetched pair (Tracer.cu:323-352 for one pair): both slabs are computed before the ordered
// tmax compares; a leaf in the first slot parks the lane with the second slot's slab kept.  `two`: the pair has a second slot
// (else a1 / b1 repeat the first).
template <bool PF, bool QW = false, class Params>
__device__ __forceinline__ void box_step_on(const Params& p, const Ray& r, Trav& t, bool two, const uint4& a0, const uint4& b0,
                                            const uint4& a1, const uint4& b1, bool lean = false)
{
    if constexpr (QW) t.phase = PH_STEP;   // (PH_STEP_POP: the popped entry is being stepped on)
    float f0, k0;
    slab(a0, b0, r, f0, k0);
    slab(a1, b1, r, t.f1, t.k1);
    t.e1 = (b1.w & kIndexMask) | (a1.w & ~kIndexMask);
    t.t1 = two ? (b1.w >> 29) : (uint32_t)RT_CHILD_NONE;
    const uint32_t type0 = b0.w >> 29;
    const uint32_t e0 = (b0.w & kIndexMask) | (a0.w & ~kIndexMask);
    const bool valid0 = type0 != RT_CHILD_NONE;
    const bool hit0 = valid0 & (k0 >= f0) & (f0 <= r.tmax) & (k0 >= r.tmin);
    t.box_tests += valid0 ? 1u : 0u;
    const bool leaf0 = hit0 & (type0 == RT_CHILD_TRI);
    t.inner_hit(hit0 & !leaf0, e0, f0, lean);
    if (leaf0) { t.leaf = e0; t.phase = PH_LEAF0; }
    else {
        t.second_slot(r.tmin, r.tmax, lean);
        if (t.phase == PH_STEP) { t.template advance<QW>(lean); prefetch_pair<PF>(p, t); }
    }
}

// The same tests for a pair entered WITHOUT a carried near (t.near_e == kNoNear, t.near_d == +inf: every pair of a narrow
// vote, see RT_TRACE_PAIR_STEP), QW traversals only.  Both slots are decided before anything is pushed: no leaf test lies
// between them unless slot 0 is a leaf hit, and that parks the lane exactly as box_step_on does.  Otherwise the general form
// would make slot 0's Box hit the near (nothing to displace, nothing pushed) and hand slot 1 to inner_hit against it:
// `closer` below is that call's test, the one push its push, `near` / `nd` what it leaves in near_e / near_d.  (A Box hit
// whose front is +inf is "not closer than no near" there and is lost; it takes tmax = +inf and a ray without a direction,
// which no camera ray has, and the `<` against +inf that would keep even that is not spent here.)  Then advance(), inline
// on the local near.  TAIL: the pair may be the first of a node of more than two slots (the second step of a narrow vote;
// never its first): near and its front go to near_e / near_d and cur moves on to the node's next pair.
template <bool TAIL>
__device__ __forceinline__ void pair_step_on(const Ray& r, Trav& t, bool two, const uint4& a0, const uint4& b0, const uint4& a1,
                                             const uint4& b1, bool lean)
{
    t.phase = PH_STEP;   // (PH_STEP_POP: the popped entry is being stepped on)
    float f0, k0, f1, k1;
    slab(a0, b0, r, f0, k0);
    slab(a1, b1, r, f1, k1);
    const uint32_t e0 = (b0.w & kIndexMask) | (a0.w & ~kIndexMask), e1 = (b1.w & kIndexMask) | (a1.w & ~kIndexMask);
    const uint32_t type0 = b0.w >> 29, type1 = two ? (b1.w >> 29) : (uint32_t)RT_CHILD_NONE;
    const bool valid0 = type0 != RT_CHILD_NONE, valid1 = type1 != RT_CHILD_NONE;
    const bool hit0 = valid0 & (k0 >= f0) & (f0 <= r.tmax) & (k0 >= r.tmin);
    t.box_tests += valid0 ? 1u : 0u;
    // (the second slot goes to t.f1 .. t.t1 on every path, as in box_step_on, though only a lane parked in PH_LEAF0 reads it:
    // written under that branch alone, the four registers are copied aside and back on every other path)
    t.f1 = f1; t.k1 = k1; t.e1 = e1; t.t1 = type1;
    if (hit0 & (type0 == RT_CHILD_TRI)) {   // parks as in box_step_on, nothing else touched
        t.leaf = e0; t.phase = PH_LEAF0;
        return;
    }
    const bool hit1 = valid1 & (k1 >= f1) & (f1 <= r.tmax) & (k1 >= r.tmin);
    t.box_tests += valid1 ? 1u : 0u;
    const bool leaf1 = hit1 & (type1 == RT_CHILD_TRI), box1 = hit1 & !leaf1;
    const bool closer = (f1 < f0) | ((f1 == f0) & ((e1 & kIndexMask) > (e0 & kIndexMask)));
    if (hit0 & box1) t.push(closer ? e0 : e1, lean);
    const bool second = box1 & (closer | !hit0);
    const uint32_t near = second ? e1 : (hit0 ? e0 : kNoNear);
    const float nd = second ? f1 : (hit0 ? f0 : __builtin_inff());
    if (leaf1) {   // the leaf phase's advance() reads the near; its front is needed if the node goes on
        t.near_e = near; t.near_d = nd;
        t.leaf = e1; t.phase = PH_LEAF1;
        return;
    }
    if constexpr (TAIL) {
        const uint32_t cnt = t.cur >> 29;
        if (cnt > 2) {
            t.near_e = near; t.near_d = nd;
            t.cur = ((t.cur & kIndexMask) + 2) | ((cnt - 2) << 29);
            return;
        }
    }
    // advance(): the near under the keep rule, else a popped entry, else done; near_e / near_d stay kNoNear / +inf
    const bool keep = (near != kNoNear) & (t.sp < kStackMax);
    if (keep) t.cur = near;
    else t.template pop_or_done<true>(lean);
}

// One box step of a lane: both slots of the current pair are loaded (four 16-byte vector loads issued together), then tested.
// PAIR (QW only): 0 the general tests, 1 / 2 the pair-local ones of a narrow vote (1: its first step, no TAIL; 2: its second).
// 3 (QW only): a step of an exact vote (kPairStep == 2) -- cur is a pair below kExactIndices: one 32-bit offset off p.nodes, four
// loads at 0 / 16 / 32 / 48 from it, slot 1 always there, no TAIL.
template <bool PF, bool QW = false, int PAIR = 0, class Params>
__device__ __forceinline__ void box_step(const Params& p, const Ray& r, Trav& t, bool lean = false)
{
    if constexpr (QW && PAIR == 3) {
        static_assert(!PF, "the exact form loads its pair itself");
        // cur << 5 drops the count (2: bit 30) and index bits 28 / 27 (zero: exact_cur): the pair's byte offset, below 4 GiB
        const uint4* np = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(p.nodes) + (uint64_t)(uint32_t)(t.cur << 5));
        const uint4 a0 = np[0], b0 = np[1], a1 = np[2], b1 = np[3];
        pair_step_on<false>(r, t, true, a0, b0, a1, b1, lean);
        return;
    }
    const uint32_t cnt = t.cur >> 29;
    const uint4* np = reinterpret_cast<const uint4*>(p.nodes + (t.cur & kIndexMask));
    const bool two = cnt > 1;
    const int o1 = two ? 2 : 0;  // all four loads issue together; a lone slot is simply read twice
    uint4 a0, b0, a1, b1;
    if constexpr (PF) { a0 = t.pf0; b0 = t.pf1; a1 = t.pf2; b1 = t.pf3; }
    else { a0 = np[0]; b0 = np[1]; a1 = np[o1]; b1 = np[o1 + 1]; }
    if constexpr (QW && PAIR != 0) pair_step_on<PAIR == 2>(r, t, two, a0, b0, a1, b1, lean);
    else box_step_on<PF, QW>(p, r, t, two, a0, b0, a1, b1, lean);
}

// Hold at pop, evaluated by the WHOLE wave (it reads its quad-mates' registers through DPP, and a switched-off lane's registers
// are not defined data for such a read: never call this under a lane-divergent branch).  True for a lane that sits on a
// freshly popped entry (PH_STEP_POP, popped from level sp < kStackLds) while a quad-mate that is still traversing has
// mate.sp > sp and the same entry at level sp of its own stack.  The quad's four entries of one level lie side by side in
// the stack column layout: one 16-byte LDS read.  Levels from kStackLds up live in private memory: never looked at, never
// held for.  A finished lane (PH_DONE; a lane outside the frame is finished from the start) counts as sp = 0, which no level
// is below.
//
// Why nobody waits for ever: a lane holds only for a mate with strictly greater sp, so the unfinished lane of a quad with the
// greatest sp never holds -- it steps, or it is parked for a leaf test.  A wave with an unfinished lane therefore always has a
// lane that steps or a parked lane, and every pass of trace_ray's loop takes a box step with at least one lane or runs a leaf
// phase that frees the parked ones.  The entry a lane holds for is a live entry of the mate's stack (level sp < mate.sp): the
// mate pops it after finitely many of its own tests -- pops are LIFO also on a full stack, where only pushes are dropped -- or
// finishes first (any-hit), and either ends the hold.  No spin, no flag, nothing outside the wave.
template <bool ANY>
__device__ __forceinline__ bool quad_hold(const Trav& t)
{
    const bool popped = t.phase == PH_STEP_POP && t.sp < kStackLds;
    const int key = ANY && t.phase == PH_DONE ? 0 : t.sp;   // (a closest-hit lane finishes on an empty stack: sp = 0 already)
    // quad_perm broadcasts of the quad's lanes 0..3 (row_mask / bank_mask all, bound_ctrl on)
    const int k0 = __builtin_amdgcn_mov_dpp(key, 0x00, 0xF, 0xF, true), k1 = __builtin_amdgcn_mov_dpp(key, 0x55, 0xF, 0xF, true);
    const int k2 = __builtin_amdgcn_mov_dpp(key, 0xAA, 0xF, 0xF, true), k3 = __builtin_amdgcn_mov_dpp(key, 0xFF, 0xF, 0xF, true);
    bool hold = false;
    if (popped) {
        typedef uint32_t lds_u32x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) lds_u32x4 lds_quad;
        // (the stack array is 16-byte aligned and a quad's four columns share one 16-byte group: rounding the lane's own column down finds it)
        const lds_u32x4 e = *(const lds_quad*)(((uintptr_t)t.lds & ~(uintptr_t)15) + (uintptr_t)t.sp * 256u);
        hold = ((k0 > t.sp) & (e.x == t.cur)) | ((k1 > t.sp) & (e.y == t.cur)) | ((k2 > t.sp) & (e.z == t.cur)) |
               ((k3 > t.sp) & (e.w == t.cur));
    }
    return hold;
}

// Hold by stack depth alone (RT_TRACE_HOLD_SECOND / RT_TRACE_HOLD_FIRST), evaluated by the WHOLE wave like quad_hold and for
// the same reason: never under a lane-divergent branch.  True for a lane that sits on a freshly popped entry (PH_STEP_POP,
// popped from level sp < kStackLds) while a quad-mate that is still traversing has mate.sp > sp.  No stack entry is compared
// and nothing is read from LDS: the key is quad_hold's, broadcast afresh (four quad-perm DPP moves), then four compares,
// three ORs and one AND.  A lane never holds for itself: its own key is its own sp (or 0).  A mate with greater sp is deeper
// in a subtree this lane has left; most often it is the subtree both took first, and the entry this lane popped is the one
// the mate will pop at the same level -- the case quad_hold tests for exactly.  Holding for the others as well costs wave
// steps and merges no fewer requests (tools/quad_wait_model.py --second sp, profiles/hold_second_model.txt).
//
// Progress.  A lane holds only for an unfinished mate with strictly greater sp, so the unfinished lane of a quad with the
// greatest sp never holds.  HOLD_FIRST = 0: the first step of every vote is quad_hold's, and its argument that every pass of
// the loop steps a lane or runs a leaf phase stands word for word; the second step may step nobody, which costs one empty step
// and harms nothing.  HOLD_FIRST = 1: the same by the greatest-sp argument -- that lane is in `stepping` or parked.  A held
// lane's mate reaches sp <= s or finishes after finitely many of its own tests (pops are LIFO also on a full stack, where
// only pushes are dropped), and either ends the hold.  The lean margin is untouched: a lane that sits out pushes nothing.
// The exact vote's "sits out" rule composes with this one: the second step's mask is PH_STEP && exact_cur(cur) && !hold, and
// a lane that sits out for either reason keeps its phase (PH_STEP_POP stays PH_STEP_POP), as a lane held before the first
// step does.  Each ray's sequence of tests, pushes and pops is unchanged; only the interleaving across lanes changes.
//   RT_TRACE_HOLD_SECOND  1 (shipped): the second step's mask excludes the lanes for which quad_hold_sp is true; 0: it steps
//                         every lane in PH_STEP.
//   RT_TRACE_HOLD_FIRST   1 (shipped): the first step's `go` is quad_hold_sp's -- no ds_read_b128, no branch and no wait in front
//                         of the vote; 0: quad_hold's.
// Both at 0 is the loop before these knobs, instruction for instruction.  Measured (DESIGN section 5,
// profiles/hold_second_bench.txt, hold_second_pmc.txt, hold_second_asm.txt): both on, L1 lookups -43 %, TA busy -12 %, +8 % wave
// steps; +4.1 % on the headline in flight, +1.8 % one frame at a time.  Either knob alone loses somewhere: SECOND alone pays
// quad_hold's LDS read and the new test (no gain one frame at a time, -1.3 % on a pairs tree), FIRST alone holds more lanes
// for nothing (-2.9 %).
#ifndef RT_TRACE_HOLD_SECOND
#define RT_TRACE_HOLD_SECOND 1
#endif
#ifndef RT_TRACE_HOLD_FIRST
#define RT_TRACE_HOLD_FIRST 1
#endif
constexpr int kHoldSecond = RT_TRACE_HOLD_SECOND, kHoldFirst = RT_TRACE_HOLD_FIRST;
static_assert((kHoldSecond == 0 || kHoldSecond == 1) && (kHoldFirst == 0 || kHoldFirst == 1), "RT_TRACE_HOLD_SECOND / RT_TRACE_HOLD_FIRST are 0 or 1");
template <bool ANY>
__device__ __forceinline__ bool quad_hold_sp(const Trav& t)
{
    const bool popped = t.phase == PH_STEP_POP && t.sp < kStackLds;
    const int key = ANY && t.phase == PH_DONE ? 0 : t.sp;
    const int k0 = __builtin_amdgcn_mov_dpp(key, 0x00, 0xF, 0xF, true), k1 = __builtin_amdgcn_mov_dpp(key, 0x55, 0xF, 0xF, true);
    const int k2 = __builtin_amdgcn_mov_dpp(key, 0xAA, 0xF, 0xF, true), k3 = __builtin_amdgcn_mov_dpp(key, 0xFF, 0xF, 0xF, true);
    return popped & ((k0 > t.sp) | (k1 > t.sp) | (k2 > t.sp) | (k3 > t.sp));
}

// The two box steps of a QW vote; `go`: this lane takes the first (in PH_STEP / PH_STEP_POP and not held); the second steps
// every lane in PH_STEP, held ones included (kHoldSecond: but for those quad_hold_sp holds).  lean: the vote's arm; NARROW: both
// steps in the pair-local form (RT_TRACE_PAIR_STEP).
template <bool PF, bool ANY, bool NARROW = false, class Params>
__device__ __forceinline__ void quad_vote_steps(const Params& p, const Ray& r, Trav& t, bool go, bool lean)
{
    if (go) box_step<PF, true, NARROW ? 1 : 0>(p, r, t, lean);
    if constexpr (kHoldSecond != 0) {
        // (bitwise on purpose: quad_hold_sp is evaluated by every lane; the cast tells the compiler so)
        if (((t.phase & 3u) == PH_STEP) & (int)!quad_hold_sp<ANY>(t)) box_step<PF, true, NARROW ? 2 : 0>(p, r, t, lean);
    } else {
        if ((t.phase & 3u) == PH_STEP) box_step<PF, true, NARROW ? 2 : 0>(p, r, t, lean);
    }
}

// The two box steps of an EXACT vote (kPairStep == 2): the first as above -- the vote has seen every unfinished lane's cur --
// the second steps the lanes in PH_STEP whose NEW cur is exact as well (kHoldSecond: and which quad_hold_sp does not hold); the
// others sit it out (progress: at exact_cur and at quad_hold_sp).
template <bool PF, bool ANY, class Params>
__device__ __forceinline__ void exact_vote_steps(const Params& p, const Ray& r, Trav& t, bool go, bool lean)
{
    if (go) box_step<PF, true, 3>(p, r, t, lean);
    if constexpr (kHoldSecond != 0) {
        // (bitwise on purpose: quad_hold_sp is evaluated by every lane; the cast tells the compiler so)
        if (((t.phase & 3u) == PH_STEP) & exact_cur(t.cur) & (int)!quad_hold_sp<ANY>(t)) box_step<PF, true, 3>(p, r, t, lean);
    } else {
        if (((t.phase & 3u) == PH_STEP) & exact_cur(t.cur)) box_step<PF, true, 3>(p, r, t, lean);
    }
}

// The leaf phase's fetch: a leaf (64 bytes) in four 16-byte requests issued together.  The empty asm "uses" all sixteen dwords:
// left alone the compiler narrows the loads to dwordx3 + overlapping dwordx2 pieces and fetches the primitive ids on a hit,
// seven or more requests, and the address path charges per request (+3 % on the headline).
__device__ __forceinline__ void load_leaf_wide(const rt_triangle_pair* leaf, uint4& l0, uint4& l1, uint4& l2, uint4& l3)
{
    const uint4* tp = reinterpret_cast<const uint4*>(leaf);
    l0 = tp[0]; l1 = tp[1]; l2 = tp[2]; l3 = tp[3];
    asm volatile("" : "+v"(l0.x), "+v"(l0.y), "+v"(l0.z), "+v"(l0.w), "+v"(l1.x), "+v"(l1.y), "+v"(l1.z), "+v"(l1.w),
                      "+v"(l2.x), "+v"(l2.y), "+v"(l2.z), "+v"(l2.w), "+v"(l3.x), "+v"(l3.y), "+v"(l3.z), "+v"(l3.w));
}

// Tracer.cu:308-374, restructured as described in trace_kernel.hip's header.  Returns tri_hit.
// steps[0] / steps[1] count the wave's box-phase / leaf-phase iterations (profiling aid).
// ANY (any-hit): a lane whose leaf test hits is done (PH_DONE) -- until that first hit its sequence of tests is the
// closest-hit one, step for step.  Params: anything with nodes, leaves, root, count, park_num, park_den.
// Filter: the hit-filter policy handed to every leaf test (NoFilter: none).
// QW: hold at pop (quad_hold above): a held lane stays in its phase and sits out the vote's first box step; the vote counts the
// lanes that will really step.  t.lds must then be a column of a 16-byte aligned [kStackLds][64] array.  Each vote of a QW
// traversal is also lean or full (kLeanMargin above).
template <bool PF, bool ANY = false, bool QW = false, class Params, class Filter = NoFilter>
__device__ __forceinline__ bool trace_ray(const Params& p, Ray& r, Hit& h, Trav& t, bool active, uint32_t* steps,
                                          Filter flt = Filter())
{
    static_assert(!(PF && QW), "prefetch_pair tests phase == PH_STEP: a PH_STEP_POP lane would step on a stale prefetched pair");
    t.sp = 0;
    t.cur = (p.root & kIndexMask) | (p.count << 29);
    t.near_e = kNoNear;
    t.near_d = __builtin_inff();
    t.phase = (active && p.count > 0) ? PH_STEP : PH_DONE;
    t.box_tests = 0;
    t.tri_tests = 0;
    t.t1 = 0;
    t.e1 = 0;
    t.f1 = t.k1 = 0.0f;
    t.leaf = 0;
    prefetch_pair<PF>(p, t);
    bool tri_hit = false;
    uint32_t nbox = 0, nleaf = 0;
    bool lean = false;    // wave-uniform, QW only: the last vote was a lean one (kLeanMargin)

    while (true) {
        // ---------------------------------------------------- box phase: step while enough lanes want to
        uint64_t stepping, parked;
        while (true) {
            if constexpr (QW) {
                const bool go = ((t.phase & 3u) == PH_STEP) & !(kHoldFirst != 0 ? quad_hold_sp<ANY>(t) : quad_hold<ANY>(t));
                stepping = __builtin_amdgcn_ballot_w64(go);
                parked = __builtin_amdgcn_ballot_w64((t.phase - 1u) < 2u);
                // the lean vote (kLeanMargin): no unfinished lane within the margin of its LDS column's end.  (A finished
                // closest-hit lane has sp = 0; an any-hit lane may finish on a non-empty stack.)
                if constexpr (kLeanStep != 0)
                    lean = __builtin_amdgcn_ballot_w64((t.sp > kStackLds - kLeanMargin) & !(ANY && t.phase == PH_DONE)) == 0;
                // (held lanes counted on the stepping side of this threshold instead: measured, no different -- DESIGN section 5)
                if (stepping == 0 || __popcll(stepping) * p.park_den < __popcll(parked) * p.park_num) break;
                nbox += 2;
                // the vote's form (RT_TRACE_PAIR_STEP).  2, shipped: exact -- no unfinished lane carries a near or sits on anything
                // but an exact pair; 1: narrow -- none sits on more than a pair or carries a near.  Either way the two
                // forms are two `if`s in a row, not if / else, and the compiler must not see that one flag decides both: as
                // alternatives that meet at the loop's end, the general form keeps the lanes' state in registers of its own and
                // eleven of them are copied across on each side of every vote (profiles/pair_step_asm.txt)
                uint64_t wide = ~0ull;
                if constexpr (kPairStep == 2) {
                    // the exact vote (exact_cur): the same ballot, over the same lanes, on the stricter test
                    // (as three ballots of plain compares combined in scalar the flag loses its v_cndmask / v_cmp_ne pair, but
                    // the allocator renumbers the whole kernel: not taken, profiles/exact_pair_asm.txt section 5)
                    wide = __builtin_amdgcn_ballot_w64((t.phase != PH_DONE) & (!exact_cur(t.cur) | (t.near_e != kNoNear)));
                    if (wide == 0) exact_vote_steps<PF, ANY>(p, r, t, go, lean);
                    asm volatile("" : "+s"(wide));
                } else if constexpr (kPairStep != 0) {
                    wide = __builtin_amdgcn_ballot_w64((t.phase != PH_DONE) & (((t.cur >> 29) > 2) | (t.near_e != kNoNear)));
                    if (wide == 0) quad_vote_steps<PF, ANY, true>(p, r, t, go, lean);
                    asm volatile("" : "+s"(wide));
                }
                if (wide != 0) quad_vote_steps<PF, ANY>(p, r, t, go, lean);
                continue;
            }
            stepping = __builtin_amdgcn_ballot_w64(t.phase == PH_STEP);
            parked = __builtin_amdgcn_ballot_w64((t.phase - 1u) < 2u);
            if (stepping == 0 || __popcll(stepping) * p.park_den < __popcll(parked) * p.park_num) break;
            nbox += 2;   // two box steps per vote (below)
            if (t.phase == PH_STEP) box_step<PF>(p, r, t);
            // second step under the same vote: halves the per-step loop overhead (ballots, branch, copies)
            if (t.phase == PH_STEP) box_step<PF>(p, r, t);
        }
        if ((stepping | parked) == 0) break;
        // ---------------------------------------------------- leaf phase (Tracer.cu:333-337, 293-306)
        nleaf++;
        if ((t.phase - 1u) < 2u) {
            t.tri_tests++;
            const uint32_t li = t.leaf & kIndexMask;
            uint4 l0, l1, l2, l3;
            load_leaf_wide(p.leaves + li, l0, l1, l2, l3);
            bool hit_tri = intersect_tri(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
                                         __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                         __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                         r, h, li << 1, l0.w, flt);
            // triangle B = (v2, v1, v3) is requested whenever count > 0; for a single triangle v3 == v2
            // bit for bit, B's edge2 is exactly 0, a == 0 and the reference rejects it: skipped, same result.
            if ((t.leaf >> 29) > 0 && (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z))
                hit_tri |= intersect_tri(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                         __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                         __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z),
                                         r, h, (li << 1) + 1, l1.w, flt);
            tri_hit |= hit_tri;
            if (ANY && hit_tri) {
                t.phase = PH_DONE;
            } else {
                const bool was_first = t.phase == PH_LEAF0;
                t.phase = PH_STEP;
                // (lean: the vote that ended the box phase was lean, so a parked lane is outside the margin)
                if (was_first) t.second_slot(r.tmin, r.tmax, lean);
                if (t.phase == PH_STEP) { t.template advance<QW>(lean); prefetch_pair<PF>(p, t); }
            }
        }
    }
    steps[0] += nbox;
    steps[1] += nleaf;
    return tri_hit;
}

// the primary ray of TraceRays (Tracer.cu:475-494) through sub-pixel (x + ox, y + oy) of a w x h frame; r.ix.. are left unset
__device__ __forceinline__ void camera_ray(const rt_camera& cam, uint32_t w, uint32_t h, uint32_t x, uint32_t y, float ox,
                                           float oy, Ray& r)
{
    const float ndcx = 2 * (((float)x + ox) / (float)w) - 1;
    const float ndcy = 2 * (((float)y + oy) / (float)h) - 1;
    const float px = (ndcx * cam.u.x + ndcy * cam.v.x) + 1.0f * cam.w.x;
    const float py = (ndcx * cam.u.y + ndcy * cam.v.y) + 1.0f * cam.w.y;
    const float pz = (ndcx * cam.u.z + ndcy * cam.v.z) + 1.0f * cam.w.z;
    const float inv_len = 1.0f / sqrtf(px * px + py * py + pz * pz);  // normalize = v * rsqrtf(dot) (helper_math.h:1318)
    r.dx = px * inv_len; r.dy = py * inv_len; r.dz = pz * inv_len;
    r.ox = cam.position.x; r.oy = cam.position.y; r.oz = cam.position.z;
    r.tmin = 0.00001f;
    r.tmax = cam.max_depth;
}

// stratified sub-pixel offset of sample s of spp in {4, 16} (2 x 2 / 4 x 4 grid); spp = 1 is the pixel centre
__device__ __forceinline__ void subpixel_offset(uint32_t s, uint32_t spp, float& ox, float& oy)
{
    const uint32_t side = spp == 4 ? 2u : 4u;
    ox = ((float)(s % side) + 0.5f) / (float)side;
    oy = ((float)((s / side) % side) + 0.5f) / (float)side;
}

}  // namespace rt
