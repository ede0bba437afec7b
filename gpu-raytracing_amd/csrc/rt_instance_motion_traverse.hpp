// rt_instance_motion_traverse.hpp -- the TLAS policy of the instance-motion ray query of instance_motion_query.hip
// (rt_intersect_rays_instanced_motion; rt_abi.h, instance-motion block): a TLAS with two key poses and
// instances whose object_to_world moves between two keys, at a time per ray.
//
// The traversal is trace_instanced<false, ANY> (rt_instance_traverse.hpp: the vote / park loop, TLAS leaves as entries, one
// 64-entry stack with the BLAS's base depth, the record's tail and its usability rule, the world ray reloaded on exit, the
// triangle-pair test) with MovingTlas as its `Tlas` policy.  What the policy adds:
//   * a TLAS step fetches the pair from both TLAS poses (eight 16-byte loads) and interpolates it with Lerp
//     (rt_motion_traverse.hpp: fl(fl(w0 * a) + fl(tau * b)), w12 / w28 from pose 0); a BLAS step fetches the lane's static
//     pair alone and tests the stored bits -- the pose-1 fetch and the interpolation sit under the lane's `top` predicate, a
//     BLAS bound is never multiplied by a weight (0 * inf is NaN);
//   * the record is rt_motion_instance_record: two matrices (six 16-byte rows) in front of the tail;
//   * enter interpolates the twelve entries at the lane's time and inverts the result in float32: cofactors and
//     determinant as prepare_instances_kernel writes them, inv_det = 1 / det, W = adj * inv_det, o' = W * (o - T),
//     d' = W * d.  A matrix that is singular AT THIS TIME (det == 0, det or 1 / det not finite) is not entered by this ray;
//   * the TLAS arrays are the params struct's pose-0 ones (both poses hold the same ids).
// No PF arm, no filter.
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"
#include "rt_instance_traverse.hpp"
#include "rt_motion_traverse.hpp"
#include "rt_traverse.hpp"

// waves per SIMD the kernel's register allocation must fit (DESIGN section 23 has the compiler's figures for each choice)
#ifndef RT_INSTANCE_MOTION_WAVES
#define RT_INSTANCE_MOTION_WAVES 4
#endif

namespace rt {

namespace {   // (as in the kernels' own file)

struct InstMotionParams {
    const rt_node* tlas_nodes0;
    const rt_triangle_pair* tlas_leaves0;
    const rt_node* tlas_nodes1;
    uint32_t root, count;
    const rt_motion_instance_record* records;
    uint32_t num_instances, num_blas;
    const rt_accel* blas_table;
    const float4* rays;
    const float* times;
    float4* hits;
    uint32_t* instance_ids;
    uint32_t num_rays;
    unsigned long long* counters;
    static constexpr int park_num = kParkNum, park_den = kParkDen;
};

// inst_box_step with the TLAS seen at the lane's time: in the TLAS the pair comes from both poses and is interpolated
// (motion_box_step's fetch and arithmetic), in a BLAS it is the stored pair
__device__ __forceinline__ void inst_motion_box_step(const LaneNodes& ln, const rt_node* tlas_nodes1, const Ray& r, Trav& t,
                                                     int base, bool top, const Lerp& lerp)
{
    const uint32_t cnt = t.cur >> 29, first = t.cur & kIndexMask;
    const uint4* np = reinterpret_cast<const uint4*>(ln.nodes + first);
    const bool two = cnt > 1;
    const int o1 = two ? 2 : 0;
    uint4 a0 = np[0], b0 = np[1], a1 = np[o1], b1 = np[o1 + 1];
    if (top) {
        const uint4* n1 = reinterpret_cast<const uint4*>(tlas_nodes1 + first);
        const uint4 a01 = n1[0], b01 = n1[1], a11 = n1[o1], b11 = n1[o1 + 1];
        a0 = lerp.word(a0, a01); b0 = lerp.word(b0, b01); a1 = lerp.word(a1, a11); b1 = lerp.word(b1, b11);
    }
    inst_box_step_on<false>(ln, r, t, base, top, two, a0, b0, a1, b1);
}

// The object-space ray of world ray r under the record's matrix at the lane's time (k[0..2] / k[3..5]: the rows of the
// record's two key matrices).  Returns false, r untouched, when that matrix cannot be inverted in float32.
__device__ __forceinline__ bool enter_moving_instance(const float4 (&k)[6], const Lerp& lerp, Ray& r)
{
    auto mix = [&](float a, float b) { return lerp.w0 * a + lerp.tau * b; };
    const float a00 = mix(k[0].x, k[3].x), a01 = mix(k[0].y, k[3].y), a02 = mix(k[0].z, k[3].z), t0 = mix(k[0].w, k[3].w);
    const float a10 = mix(k[1].x, k[4].x), a11 = mix(k[1].y, k[4].y), a12 = mix(k[1].z, k[4].z), t1 = mix(k[1].w, k[4].w);
    const float a20 = mix(k[2].x, k[5].x), a21 = mix(k[2].y, k[5].y), a22 = mix(k[2].z, k[5].z), t2 = mix(k[2].w, k[5].w);
    // prepare_instances_kernel's cofactors and determinant, in float32
    const float c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const float det = (a00 * c00 + a01 * c01) + a02 * c02;
    const float inv_det = 1.0f / det;
    if (det == 0.0f || !__builtin_isfinite(det) || !__builtin_isfinite(inv_det)) return false;
    const float w00 = c00 * inv_det, w01 = (a02 * a21 - a01 * a22) * inv_det, w02 = (a01 * a12 - a02 * a11) * inv_det;
    const float w10 = c01 * inv_det, w11 = (a00 * a22 - a02 * a20) * inv_det, w12 = (a02 * a10 - a00 * a12) * inv_det;
    const float w20 = c02 * inv_det, w21 = (a01 * a20 - a00 * a21) * inv_det, w22 = (a00 * a11 - a01 * a10) * inv_det;
    const float qx = r.ox - t0, qy = r.oy - t1, qz = r.oz - t2, dx = r.dx, dy = r.dy, dz = r.dz;
    r.ox = (w00 * qx + w01 * qy) + w02 * qz;
    r.oy = (w10 * qx + w11 * qy) + w12 * qz;
    r.oz = (w20 * qx + w21 * qy) + w22 * qz;
    r.dx = (w00 * dx + w01 * dy) + w02 * dz;
    r.dy = (w10 * dx + w11 * dy) + w12 * dz;
    r.dz = (w20 * dx + w21 * dy) + w22 * dz;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    return true;
}

// trace_instanced's TLAS policy (StaticTlas: rt_instance_traverse.hpp) for a TLAS and records seen at the lane's time
struct MovingTlas {
    static constexpr bool moving = true;
    Lerp lerp;
    __device__ __forceinline__ static const rt_node* nodes(const InstMotionParams& p) { return p.tlas_nodes0; }
    __device__ __forceinline__ static const rt_triangle_pair* leaves(const InstMotionParams& p) { return p.tlas_leaves0; }
    template <bool PF>
    __device__ __forceinline__ void box_step(const InstMotionParams& p, const LaneNodes& ln, const Ray& r, Trav& t, int base,
                                             bool top) const
    {
        static_assert(!PF, "the instance-motion query has no pair-prefetch arm");
        inst_motion_box_step(ln, p.tlas_nodes1, r, t, base, top, lerp);
    }
    // rt_motion_instance_record: the rows of two key matrices in front of the tail
    __device__ __forceinline__ bool enter(const InstMotionParams& p, uint32_t id, Ray& r, BlasRef& b) const
    {
        float4 k[6];
        if (!load_instance(p, id, b, k[0], k[1], k[2], k[3], k[4], k[5])) return false;
        return enter_moving_instance(k, lerp, r);
    }
};

// tau: the lane's time, in [0, 1] for an active lane
template <bool ANY>
__device__ __forceinline__ bool trace_instanced_motion(const InstMotionParams& p, uint64_t ri, Ray& r, float tau, Hit& h,
                                                       uint32_t& hit_inst, Trav& t, bool active, uint32_t* steps)
{
    return trace_instanced<false, ANY, NoInstanceFilter, MovingTlas>(p, ri, r, h, hit_inst, t, active, steps, NoInstanceFilter(),
                                                                     MovingTlas{{1.0f - tau, tau}});
}

}  // namespace

}  // namespace rt
