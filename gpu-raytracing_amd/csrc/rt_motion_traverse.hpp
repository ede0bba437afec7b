// rt_motion_traverse.hpp -- the traversal of the motion-blur ray query of motion_query.hip (rt_intersect_rays_motion): one
// topology, two key poses (nodes0 / leaves0 at time 0, nodes1 / leaves1 at time 1: the same tree, refitted), and a time per
// ray.  A lane sees every box bound and every leaf corner interpolated at its own time and runs trace_ray's tests on the
// interpolated values: the slab test and the ordered compares of box_step_on, intersect_tri, Trav's stack -- all of them
// rt_traverse.hpp's code, called from here.  What this file adds is the fetch of a pair from both poses, the interpolation
// and MotionWalk, the policy that hands the two steps and the lane's weights to trace_plain (rt_plain_traverse.hpp: trace_ray's
// non-QW vote / park loop, written once; no PF arm, no uniform arm).
//
// The interpolation is  w0 = 1 - tau (once per ray);  v = fl(fl(w0 * a) + fl(tau * b))  -- two multiplies and one add, never
// contracted (-ffp-contract=off) and never rewritten as a + tau * (b - a):
//   * rounding is monotone and w0, tau >= 0, so v is monotone in a and in b: a slot's interpolated box bounds the interpolated
//     corners under it, and a parent's interpolated box its children's, EXACTLY in float32, whenever both poses' boxes do
//     (rt_refit's ordered boxes do).  The delta form is not monotone: it puts lower bounds above the values they should bound
//     (tests/test_motion_ref_cpu.py);
//   * tau = 0 gives a (w0 = 1: 1 * a + 0 * b) and tau = 1 gives b, as numbers (a zero may change sign: -0 + +0 = +0).
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"
#include "rt_plain_traverse.hpp"
#include "rt_traverse.hpp"

// waves per SIMD the motion kernel's register allocation must fit: a box step holds eight 16-byte loads in flight instead of
// four, plus tau and w0 (DESIGN section 22 has the compiler's figures for each choice)
#ifndef RT_MOTION_WAVES
#define RT_MOTION_WAVES 5
#endif

namespace rt {

namespace {   // (as in the kernels' own file)

struct MotionParams {
    const rt_node* nodes0;
    const rt_triangle_pair* leaves0;
    const rt_node* nodes1;
    const rt_triangle_pair* leaves1;
    uint32_t root, count;
    const float4* rays;
    const float* times;
    float4* hits;
    uint32_t num_rays;
    unsigned long long* counters;
    static constexpr int park_num = kParkNum, park_den = kParkDen;
};

// a lane's two weights
struct Lerp {
    float w0, tau;
    __device__ __forceinline__ float operator()(uint32_t a, uint32_t b) const
    {
        return w0 * __uint_as_float(a) + tau * __uint_as_float(b);
    }
    // three interpolated floats and pose 0's fourth word (a slot's w12 / w28, a record's id / rotations word)
    __device__ __forceinline__ uint4 word(const uint4& a, const uint4& b) const
    {
        return make_uint4(__float_as_uint((*this)(a.x, b.x)), __float_as_uint((*this)(a.y, b.y)),
                          __float_as_uint((*this)(a.z, b.z)), a.w);
    }
};

// box_step of rt_traverse.hpp on the pair as the lane's time sees it: the pair's four words from each pose (eight loads issued
// together; a lone slot is read twice, as there), interpolated, then the unchanged tests
__device__ __forceinline__ void motion_box_step(const MotionParams& p, const Ray& r, Trav& t, const Lerp& lerp)
{
    const uint32_t cnt = t.cur >> 29, first = t.cur & kIndexMask;
    const uint4* n0 = reinterpret_cast<const uint4*>(p.nodes0 + first);
    const uint4* n1 = reinterpret_cast<const uint4*>(p.nodes1 + first);
    const bool two = cnt > 1;
    const int o1 = two ? 2 : 0;
    const uint4 a00 = n0[0], b00 = n0[1], a10 = n0[o1], b10 = n0[o1 + 1];
    const uint4 a01 = n1[0], b01 = n1[1], a11 = n1[o1], b11 = n1[o1 + 1];
    box_step_on<false>(p, r, t, two, lerp.word(a00, a01), lerp.word(b00, b01), lerp.word(a10, a11), lerp.word(b10, b11));
}

// trace_ray's leaf test on the record as the lane's time sees it
__device__ __forceinline__ bool motion_leaf_test(const MotionParams& p, Ray& r, Hit& h, const Trav& t, const Lerp& lerp)
{
    const uint32_t li = t.leaf & kIndexMask;
    const uint4* t0 = reinterpret_cast<const uint4*>(p.leaves0 + li);
    const uint4* t1 = reinterpret_cast<const uint4*>(p.leaves1 + li);
    uint4 l00 = t0[0], l10 = t0[1], l20 = t0[2], l30 = t0[3];
    uint4 l01 = t1[0], l11 = t1[1], l21 = t1[2], l31 = t1[3];
    // (as load_leaf_wide: the eight loads stay eight 16-byte requests issued together.  Not two calls of it: those interleave
    // loads and barriers differently)
    asm volatile("" : "+v"(l00.x), "+v"(l00.y), "+v"(l00.z), "+v"(l00.w), "+v"(l10.x), "+v"(l10.y), "+v"(l10.z), "+v"(l10.w),
                      "+v"(l20.x), "+v"(l20.y), "+v"(l20.z), "+v"(l20.w), "+v"(l30.x), "+v"(l30.y), "+v"(l30.z), "+v"(l30.w));
    asm volatile("" : "+v"(l01.x), "+v"(l01.y), "+v"(l01.z), "+v"(l01.w), "+v"(l11.x), "+v"(l11.y), "+v"(l11.z), "+v"(l11.w),
                      "+v"(l21.x), "+v"(l21.y), "+v"(l21.z), "+v"(l21.w), "+v"(l31.x), "+v"(l31.y), "+v"(l31.z), "+v"(l31.w));
    const uint4 l0 = lerp.word(l00, l01), l1 = lerp.word(l10, l11), l2 = lerp.word(l20, l21), l3 = lerp.word(l30, l31);
    bool hit_tri = intersect_tri(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
                                 __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                 __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                 r, h, li << 1, l0.w);
    // a single's v3 == v2 bit for bit in both poses, hence in the interpolated record too: B is skipped, as in trace_ray
    if ((t.leaf >> 29) > 0 && (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z))
        hit_tri |= intersect_tri(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                 __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                 __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z),
                                 r, h, (li << 1) + 1, l1.w);
    return hit_tri;
}

// trace_plain's policy: the two steps above at the lane's weights
struct MotionWalk {
    Hit& h;
    const Lerp lerp;
    __device__ __forceinline__ void begin(const MotionParams&) {}
    __device__ __forceinline__ void box(const MotionParams& p, const Ray& r, Trav& t) { motion_box_step(p, r, t, lerp); }
    __device__ __forceinline__ bool leaf(const MotionParams& p, Ray& r, Trav& t)
    {
        t.tri_tests++;
        return motion_leaf_test(p, r, h, t, lerp);
    }
};

// tau: the lane's time, in [0, 1] for an active lane.  Returns tri_hit; steps[0] / steps[1] as trace_ray.
template <bool ANY>
__device__ __forceinline__ bool trace_ray_motion(const MotionParams& p, Ray& r, float tau, Hit& h, Trav& t, bool active,
                                                 uint32_t* steps)
{
    MotionWalk w = {h, {1.0f - tau, tau}};
    return trace_plain<ANY>(p, r, t, active, steps, w);
}

}  // namespace

}  // namespace rt
