// rt_instance_mixed_traverse.hpp -- the two-level traversal of the mixed instanced ray query of instance_mixed_query.hip
// (rt_intersect_rays_instanced_mixed): a TLAS over placed copies of trees whose leaves hold triangles OR spheres, the kind
// told per BLAS by a table parallel to the BLAS table (semantics: rt_abi.h, mixed-instancing block).
//
// trace_instanced_mixed is trace_instanced<false, ANY> (rt_instance_traverse.hpp: the vote / park loop, the box step of both
// levels, leaving and entering instances) written as a loop of its own.  As a leaf-primitive policy of trace_instanced it
// left the existing kernels untouched, but these four kernels came out neither instruction-identical nor within the parent's
// run-to-run spread in tools/instance_mixed_bench.py, so the loop stays here and shares what leaves it
// identical: the box step (inst_box_step<false>), inst_advance, inst_second_slot, load_world_ray, to_object_ray, load_accel,
// intersect_tri and intersect_sphere are the existing headers' code, called from here.  What this file adds:
//   * three values per lane -- the kind of the BLAS the lane is in, its sphere array and its sphere count --, read as ONE
//     16-byte load of geom_table[blas] when the instance is entered, after its rt_accel;
//   * the entry rules of the table: a kind that is neither RT_GEOM_* value, and a sphere BLAS without a sphere array, are
//     not entered;
//   * a leaf phase of two arms: a lane parked in PH_LEAF0 / PH_LEAF1 runs trace_instanced's triangle arm or
//     sphere_leaf_test's steps (rt_sphere_traverse.hpp) on its object-space ray, by its kind.
// A sphere hit is kept in the lane's Hit as (primitive_id = sphere index, bu = far-root flag); the kernel's write-out picks
// the record shape by the kind of the hit instance's BLAS.  No pair-prefetch arm, no hold at pop.
// The CAPS arm (rt_intersect_rays_instanced_mixed_capsules) adds capsule BLASes as a third kind: the entry
// rule admits RT_GEOM_CAPSULES with a capsule array, and a lane of that kind runs CapsuleWalk::leaf's steps
// (rt_capsule_traverse.hpp: two independent 16-byte loads, intersect_capsule) on its object-space ray, through the same data
// pointer and count.  A capsule hit is kept as (primitive_id = capsule index, bu = far-root flag, bv = axial parameter).
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"
#include "rt_capsule_traverse.hpp"
#include "rt_instance_traverse.hpp"
#include "rt_sphere_traverse.hpp"
#include "rt_traverse.hpp"

// waves per SIMD the mixed kernel's register allocation must fit: instance_query_kernel's (DESIGN section 25 has the
// compiler's figures)
#ifndef RT_INSTANCE_MIXED_WAVES
#define RT_INSTANCE_MIXED_WAVES RT_INSTANCE_QUERY_WAVES
#endif

// ... and the CAPS kernels': one above the highest bound without spills.  At 4 waves (116 to 118 VGPRs) nothing spills, at 5
// (96) 37 to 39 registers do, at 6 (80) 81 to 84; tools/instance_capsule_bench.py put 5 ahead of 3, 4 and 6 in every
// comparison (DESIGN section 33 has the compiler's figures per candidate and the rates)
#ifndef RT_INSTANCE_MIXED_CAPSULE_WAVES
#define RT_INSTANCE_MIXED_CAPSULE_WAVES 5
#endif

namespace rt {

namespace {   // (as in the kernels' own file)

struct MixedInstParams : InstParams {
    const rt_geometry* geom_table;   // parallel to blas_table
};

// rt_geometry of table entry b: one 16-byte load (data, count, kind)
__device__ __forceinline__ void load_geometry(const rt_geometry* table, uint32_t b, uint64_t& data, uint32_t& count,
                                              uint32_t& kind)
{
    const uint4 g = reinterpret_cast<const uint4*>(table + b)[0];
    data = ((uint64_t)g.y << 32) | g.x;
    count = g.z;
    kind = g.w;
}

// The two-level traversal of ray `ri` (r: its world ray, loaded by the caller).  Returns whether a primitive was accepted;
// *hit_inst = the instance of h.  h of a sphere hit: primitive_id = the sphere index, bu = the far-root flag; of a capsule hit
// (CAPS): primitive_id = the capsule index, bu = the far-root flag, bv = the axial parameter.
// CAPS (rt_intersect_rays_instanced_mixed_capsules) admits RT_GEOM_CAPSULES at the entry rule and gives the
// leaf phase its third arm; each of the two places asks `if constexpr (CAPS)` where it stands, so the <ANY, false> code is the
// code from before the arm, instruction for instruction.
template <bool ANY, bool CAPS = false>
__device__ __forceinline__ bool trace_instanced_mixed(const MixedInstParams& p, uint64_t ri, Ray& r, Hit& h, uint32_t& hit_inst,
                                                      Trav& t, bool active, uint32_t* steps)
{
    LaneNodes ln = {p.tlas_nodes};
    const rt_triangle_pair* leaves = p.tlas_leaves;
    uint32_t inst = kTop;
    uint32_t kind = RT_GEOM_TRIANGLES;    // of the BLAS the lane is in
    const float4* data = nullptr;         // ... its sphere or capsule array (every kind but RT_GEOM_TRIANGLES)
    uint32_t count = 0;                   // ... and count
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
    bool any_hit = false;
    uint32_t nbox = 0, nleaf = 0;

    while (true) {
        // ---------------------------------------------------- box phase (both levels)
        uint64_t stepping, parked;
        while (true) {
            stepping = __builtin_amdgcn_ballot_w64(t.phase == PH_STEP);
            parked = __builtin_amdgcn_ballot_w64((t.phase != PH_STEP) & (t.phase != PH_DONE));
            if (stepping == 0 || __popcll(stepping) * p.park_den < __popcll(parked) * p.park_num) break;
            nbox += 2;
            if (t.phase == PH_STEP) inst_box_step<false>(ln, r, t, base, inst == kTop);
            if (t.phase == PH_STEP) inst_box_step<false>(ln, r, t, base, inst == kTop);
        }
        if ((stepping | parked) == 0) break;
        // ---------------------------------------------------- leaf phase: primitive tests, leaving and entering instances
        nleaf++;
        if ((t.phase != PH_STEP) & (t.phase != PH_DONE)) {
            if ((t.phase - 1u) < 2u) {   // PH_LEAF0 / PH_LEAF1: a BLAS leaf
                const uint32_t li = t.leaf & kIndexMask;
                const uint4* tp = reinterpret_cast<const uint4*>(leaves + li);
                bool hit_prim = false;
                bool tri_lane = kind != RT_GEOM_SPHERES;
                if constexpr (CAPS) {            // CapsuleWalk::leaf's steps on the object-space ray
                    tri_lane = kind == RT_GEOM_TRIANGLES;
                    if (kind == RT_GEOM_CAPSULES) {
                        const uint32_t id = tp[0].w;
                        if (id < count) {
                            const float4 c0 = data[2 * (uint64_t)id], c1 = data[2 * (uint64_t)id + 1];
                            if (c0.w >= 0.0f && c0.w != __builtin_inff()) {
                                t.tri_tests++;
                                CapsuleHit ch;
                                hit_prim = intersect_capsule(c0, c1, r, ch, id);
                                if (hit_prim) { h.primitive_id = ch.id; h.tri_id = 0u; h.bu = ch.far_root; h.bv = ch.v; }
                            }
                        }
                    }
                }
                if (kind == RT_GEOM_SPHERES) {   // sphere_leaf_test's steps on the object-space ray
                    const uint32_t id = tp[0].w;
                    if (id < count) {
                        const float4 sp = data[id];
                        if (sp.w >= 0.0f && sp.w != __builtin_inff()) {
                            t.tri_tests++;
                            SphereHit sh;
                            hit_prim = intersect_sphere(sp, r, sh, id);
                            if (hit_prim) { h.primitive_id = sh.id; h.tri_id = 0u; h.bu = sh.far_root; h.bv = 0.0f; }
                        }
                    }
                } else if (tri_lane) {           // trace_instanced's triangle arm
                    t.tri_tests++;
                    const uint4 l0 = tp[0], l1 = tp[1], l2 = tp[2], l3 = tp[3];
                    hit_prim = intersect_tri(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
                                             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                             __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                             r, h, li << 1, l0.w);
                    if ((t.leaf >> 29) > 0 && (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z))
                        hit_prim |= intersect_tri(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                                  __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                                  __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z),
                                                  r, h, (li << 1) + 1, l1.w);
                }
                any_hit |= hit_prim;
                if (hit_prim) hit_inst = inst;
                if (ANY && hit_prim) {
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
                ln.nodes = p.tlas_nodes;
                inst = kTop;
                base = 0;
                t.phase = PH_STEP;
                inst_advance(t, 0, true);
            }
            if (t.phase == PH_ENTER) {   // a TLAS leaf: enter its instance, or go on in the TLAS
                const uint32_t id = reinterpret_cast<const uint4*>(p.tlas_leaves + (t.cur & kIndexMask))[0].w;
                bool ok = id < p.num_instances;
                uint32_t nroot = 0, ncount = 0, gcount = 0, gkind = 0;
                uint64_t ntris = 0, nnodes = 0, gdata = 0;
                float4 w0, w1, w2;
                if (ok) {
                    const float4* rec = reinterpret_cast<const float4*>(p.records + id);
                    w0 = rec[0]; w1 = rec[1]; w2 = rec[2];
                    const uint4 tail = reinterpret_cast<const uint4*>(rec)[3];   // blas, flags, spare
                    ok = (tail.y == 0u) & (tail.x < p.num_blas);
                    if (ok) {
                        load_accel(p.blas_table, tail.x, ntris, nnodes, nroot, ncount);
                        load_geometry(p.geom_table, tail.x, gdata, gcount, gkind);
                        ok = ((ncount - 1u) < 7u) &
                             ((gkind == RT_GEOM_TRIANGLES) | ((gkind == RT_GEOM_SPHERES) & (gdata != 0ull)));
                        if constexpr (CAPS) ok |= ((ncount - 1u) < 7u) & (gkind == RT_GEOM_CAPSULES) & (gdata != 0ull);
                    }
                }
                if (ok) {
                    to_object_ray(w0, w1, w2, r);
                    ln.nodes = reinterpret_cast<const rt_node*>(nnodes);
                    leaves = reinterpret_cast<const rt_triangle_pair*>(ntris);
                    kind = gkind;
                    data = reinterpret_cast<const float4*>(gdata);
                    count = gcount;
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
    return any_hit;
}

}  // namespace

}  // namespace rt
