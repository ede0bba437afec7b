// rt_instance_motion_traverse.hpp -- the traversal of the instance-motion ray query of instance_motion_query.hip
// (rt_intersect_rays_instanced_motion; rt_abi.h, instance-motion block): trace_instanced's two-level loop
// (rt_instance_traverse.hpp) over a TLAS with two key poses and instances whose object_to_world moves between two keys, at
// a time per ray.  What this file adds to that loop:
//   * a TLAS step fetches the pair from both TLAS poses (eight 16-byte loads) and interpolates it with Lerp
//     (rt_motion_traverse.hpp: fl(fl(w0 * a) + fl(tau * b)), w12 / w28 from pose 0); a BLAS step fetches the lane's static
//     pair alone and tests the stored bits -- the pose-1 fetch and the interpolation sit under the lane's `top` predicate, a
//     BLAS bound is never multiplied by a weight (0 * inf is NaN);
//   * PH_ENTER loads the record's two matrices (six 16-byte loads and the tail), interpolates the twelve entries at the
//     lane's time and inverts the result in float32: cofactors and determinant as prepare_instances_kernel writes them,
//     inv_det = 1 / det, W = adj * inv_det, o' = W * (o - T), d' = W * d.  A matrix that is singular AT THIS TIME (det == 0,
//     det or 1 / det not finite) is not entered by this ray.
// Everything else -- TLAS leaves as entries, one 64-entry stack with the BLAS's base depth, the world ray reloaded on exit,
// the leaf test -- is trace_instanced's, called or restated from there.  No PF arm, no filter.
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

__device__ __forceinline__ void load_world_ray(const InstMotionParams& p, uint64_t i, Ray& r)
{
    const float4 a = p.rays[2 * i], b = p.rays[2 * i + 1];
    r.ox = a.x; r.oy = a.y; r.oz = a.z;
    r.dx = b.x; r.dy = b.y; r.dz = b.z;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
}

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

// The object-space ray of world ray r under the record's matrix at the lane's time (k0 / k1: the rows of the record's two key
// matrices, three 16-byte words each).  Returns false, r untouched, when that matrix cannot be inverted in float32.
__device__ __forceinline__ bool enter_moving_instance(const float4 (&k0)[3], const float4 (&k1)[3], const Lerp& lerp, Ray& r)
{
    auto mix = [&](float a, float b) { return lerp.w0 * a + lerp.tau * b; };
    const float a00 = mix(k0[0].x, k1[0].x), a01 = mix(k0[0].y, k1[0].y), a02 = mix(k0[0].z, k1[0].z), t0 = mix(k0[0].w, k1[0].w);
    const float a10 = mix(k0[1].x, k1[1].x), a11 = mix(k0[1].y, k1[1].y), a12 = mix(k0[1].z, k1[1].z), t1 = mix(k0[1].w, k1[1].w);
    const float a20 = mix(k0[2].x, k1[2].x), a21 = mix(k0[2].y, k1[2].y), a22 = mix(k0[2].z, k1[2].z), t2 = mix(k0[2].w, k1[2].w);
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

// trace_instanced<false, ANY> with the two steps above.  tau: the lane's time, in [0, 1] for an active lane.  Returns tri_hit;
// *hit_inst = the instance of h; steps[0] / steps[1] as trace_ray.
template <bool ANY>
__device__ __forceinline__ bool trace_instanced_motion(const InstMotionParams& p, uint64_t ri, Ray& r, float tau, Hit& h,
                                                       uint32_t& hit_inst, Trav& t, bool active, uint32_t* steps)
{
    const Lerp lerp = {1.0f - tau, tau};
    LaneNodes ln = {p.tlas_nodes0};
    const rt_triangle_pair* leaves = p.tlas_leaves0;
    uint32_t inst = kTop;
    int base = 0;
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
    bool tri_hit = false;
    uint32_t nbox = 0, nleaf = 0;

    while (true) {
        // ---------------------------------------------------- box phase (both levels)
        uint64_t stepping, parked;
        while (true) {
            stepping = __builtin_amdgcn_ballot_w64(t.phase == PH_STEP);
            parked = __builtin_amdgcn_ballot_w64((t.phase != PH_STEP) & (t.phase != PH_DONE));
            if (stepping == 0 || __popcll(stepping) * p.park_den < __popcll(parked) * p.park_num) break;
            nbox += 2;
            if (t.phase == PH_STEP) inst_motion_box_step(ln, p.tlas_nodes1, r, t, base, inst == kTop, lerp);
            if (t.phase == PH_STEP) inst_motion_box_step(ln, p.tlas_nodes1, r, t, base, inst == kTop, lerp);
        }
        if ((stepping | parked) == 0) break;
        // ---------------------------------------------------- leaf phase: triangle tests, leaving and entering instances
        nleaf++;
        if ((t.phase != PH_STEP) & (t.phase != PH_DONE)) {
            if ((t.phase - 1u) < 2u) {   // PH_LEAF0 / PH_LEAF1: a leaf of the static BLAS, as trace_instanced
                t.tri_tests++;
                const uint32_t li = t.leaf & kIndexMask;
                const uint4* tp = reinterpret_cast<const uint4*>(leaves + li);
                const uint4 l0 = tp[0], l1 = tp[1], l2 = tp[2], l3 = tp[3];
                bool hit_tri = intersect_tri(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
                                             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                             __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                             r, h, li << 1, l0.w);
                if ((t.leaf >> 29) > 0 && (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z))
                    hit_tri |= intersect_tri(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                             __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z),
                                             r, h, (li << 1) + 1, l1.w);
                tri_hit |= hit_tri;
                if (hit_tri) hit_inst = inst;
                if (ANY && hit_tri) {
                    t.phase = PH_DONE;
                } else {
                    const bool was_first = t.phase == PH_LEAF0;
                    t.phase = PH_STEP;
                    if (was_first) inst_second_slot(t, r.tmin, r.tmax, false);
                    if (t.phase == PH_STEP) inst_advance(t, base, false);
                }
            }
            if (t.phase == PH_EXIT) {    // the BLAS is done: back to the world ray and the TLAS
                load_world_ray(p, ri, r);
                ln.nodes = p.tlas_nodes0;
                inst = kTop;
                base = 0;
                t.phase = PH_STEP;
                inst_advance(t, 0, true);
            }
            if (t.phase == PH_ENTER) {   // a TLAS leaf (pose 0's: both poses hold the same ids): enter its instance, or go on
                const uint32_t id = reinterpret_cast<const uint4*>(p.tlas_leaves0 + (t.cur & kIndexMask))[0].w;
                bool ok = id < p.num_instances;
                uint32_t nroot = 0, ncount = 0;
                uint64_t ntris = 0, nnodes = 0;
                if (ok) {
                    const float4* rec = reinterpret_cast<const float4*>(p.records + id);
                    const float4 k0[3] = {rec[0], rec[1], rec[2]}, k1[3] = {rec[3], rec[4], rec[5]};
                    const uint4 tail = reinterpret_cast<const uint4*>(rec)[6];   // blas, flags, spare
                    ok = (tail.y == 0u) & (tail.x < p.num_blas);
                    if (ok) {
                        load_accel(p.blas_table, tail.x, ntris, nnodes, nroot, ncount);
                        ok = (ncount - 1u) < 7u;
                    }
                    if (ok) ok = enter_moving_instance(k0, k1, lerp, r);
                }
                if (ok) {
                    ln.nodes = reinterpret_cast<const rt_node*>(nnodes);
                    leaves = reinterpret_cast<const rt_triangle_pair*>(ntris);
                    inst = id;
                    base = t.sp;
                    t.cur = (nroot & kIndexMask) | (ncount << 29);
                    t.phase = PH_STEP;
                } else {
                    t.phase = PH_STEP;
                    inst_advance(t, 0, true);
                }
            }
        }
    }
    steps[0] += nbox;
    steps[1] += nleaf;
    return tri_hit;
}

}  // namespace

}  // namespace rt
