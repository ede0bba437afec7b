// rt_plain_traverse.hpp -- the single-level vote / park loop, written once: trace_ray<false, ANY> of rt_traverse.hpp (its plain
// arm: no hold at pop, no pair prefetch) with the box step and the leaf visit handed in as a policy.  The motion, sphere,
// capsule and sphere-cast queries walk through it; trace_ray itself, the two-level loops and the set-valued queries do not.
// The policy `Walk` comes by reference and holds the lane's hit by reference:
//   w.begin(p)       once, after Trav is set up;
//   w.box(p, r, t)   one box step; called twice per vote, each time only for a lane that is still stepping;
//   w.leaf(p, r, t)  the leaf visit of one parked lane: true when something was accepted.  It counts its own t.tri_tests
//                    (the sphere and capsule leaves count valid primitives only).
// Which spellings hold the kernels' code: DESIGN section 9, "Policies and helpers".  Device code only, force-inlined.
#pragma once

#include "rt_device.hpp"
#include "rt_traverse.hpp"

namespace rt {

namespace {   // (as in the kernels' own file)

// launch position j -> ray index (0xFFFFFFFF: no ray -- num_rays is a uint32, so it is never in range).  Params: anything
// with order / num_indices (read by the INDEXED instantiations only)
template <bool INDEXED, class Params>
__device__ __forceinline__ uint64_t ray_index(const Params& p, uint64_t j)
{
    if constexpr (INDEXED) return j < p.num_indices ? p.order[j] : 0xFFFFFFFFull;
    else return j;
}

// Params: anything with root, count, park_num and park_den.  Returns whether a leaf visit accepted anything; steps[0] /
// steps[1] as trace_ray (the wave's box steps and leaf phases).
template <bool ANY, class Params, class Walk>
__device__ __forceinline__ bool trace_plain(const Params& p, Ray& r, Trav& t, bool active, uint32_t* steps, Walk& w)
{
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
    w.begin(p);
    bool any_hit = false;
    uint32_t nbox = 0, nleaf = 0;

    while (true) {
        // ---------------------------------------------------- box phase: step while enough lanes want to
        uint64_t stepping, parked;
        while (true) {
            stepping = __builtin_amdgcn_ballot_w64(t.phase == PH_STEP);
            parked = __builtin_amdgcn_ballot_w64((t.phase - 1u) < 2u);
            if (stepping == 0 || __popcll(stepping) * p.park_den < __popcll(parked) * p.park_num) break;
            nbox += 2;   // two box steps per vote, as trace_ray
            if (t.phase == PH_STEP) w.box(p, r, t);
            if (t.phase == PH_STEP) w.box(p, r, t);
        }
        if ((stepping | parked) == 0) break;
        // ---------------------------------------------------- leaf phase
        nleaf++;
        if ((t.phase - 1u) < 2u) {
            const bool hit = w.leaf(p, r, t);
            any_hit |= hit;
            if (ANY && hit) {
                t.phase = PH_DONE;
            } else {
                const bool was_first = t.phase == PH_LEAF0;
                t.phase = PH_STEP;
                if (was_first) t.second_slot(r.tmin, r.tmax);
                if (t.phase == PH_STEP) t.advance();
            }
        }
    }
    steps[0] += nbox;
    steps[1] += nleaf;
    return any_hit;
}

}  // namespace

}  // namespace rt
