// rt_sphere_cast_traverse.hpp -- the traversal of the sphere cast of sphere_cast_query.hip (rt_sphere_cast): a ball of radius
// rad whose centre travels along the ray, over any triangle tree the ray query takes.  Trav's stack, second_slot, advance and
// inner_hit, the slab test and the ordered compares of box_step_on, load_leaf_wide and intersect_tri are rt_traverse.hpp's
// code, cap_roots and capsule_crossing rt_capsule_traverse.hpp's, tri_d2 and unrotate rt_point_math.hpp's: called from here.
// What this file adds:
//   * the box phase's one change: both slots of a fetched pair are grown by the lane's e (lo - e, hi + e) before they are
//     handed to box_step_on.  e is made once per ray (cast_grow): 0 for rad == 0, else fl(rad + pad), pad = fl(2^-18 *
//     max(rad, M)), M the largest |bound| of the root run's slots;
//   * the leaf phase: per triangle the test of rt_abi.h's sphere-cast block -- the overlap predicate at tmin (tri_d2 on the
//     caller's corner order, the range query's), else the facing offset face (intersect_tri on an origin shifted by rad along
//     the unit normal) and the near roots of the three edge capsules, accepted in that order against one shrinking tmax;
//     rad == 0: intersect_tri alone, the ray query's leaf test;
//   * CastWalk, the policy that hands the two, the lane's radius and its growth to trace_plain (rt_plain_traverse.hpp: the
//     plain vote / park loop trace_ray_spheres walks through; no PF arm, no hold at pop).
// Every operation is rounded on its own (-ffp-contract=off), the divisions are IEEE and the square roots correctly rounded.
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"
#include "rt_capsule_traverse.hpp"
#include "rt_point_math.hpp"
#include "rt_plain_traverse.hpp"
#include "rt_traverse.hpp"

// waves per SIMD the cast kernel's register allocation must fit.  The leaf holds nine corner coordinates, the re-based ray and
// a capsule evaluation: at 8 waves (64 VGPRs) 160 to 228 registers spill, at 7 (72) 140 to 167, at 6 (80) 124 to 138, at 5 (96)
// 51 to 62, at 4 (128) two.  tools/sphere_cast_bench.py put 4 ahead of 5 and 5 ahead of 6 on every row with a radius (DESIGN
// section 27 has the compiler's figures and the rates)
#ifndef RT_SPHERE_CAST_WAVES
#define RT_SPHERE_CAST_WAVES 4
#endif

namespace rt {

namespace {   // (as in the kernels' own file)

struct CastParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* rays;       // rt_ray = two float4: (origin, tmin), (dir, tmax)
    const float* radii;       // per ray, or null: every ray takes `radius`
    float radius;
    float4* hits;             // rt_hit = one float4: (t, primitive_id bits, u, v)
    uint32_t* features;       // per ray RT_SWEEP_*, or null
    uint32_t num_rays;
    unsigned long long* counters;
    const uint32_t* order;    // INDEXED instantiations only
    uint32_t num_indices;
    static constexpr int park_num = kParkNum, park_den = kParkDen;
};

constexpr float kCastPad = 1.0f / 262144.0f;   // 2^-18 (rt_abi.h, sphere-cast block)

// a ray's contact so far (r.tmax carries t).  h.bu / h.bv weigh the STORED corners 1 and 2 of leaf triangle h.tri_id (the
// kernel maps them through the leaf's rotation, as the ray query does) -- except for RT_SWEEP_OVERLAP, whose weights come from
// the closest-point routine on the caller's corner order and are the record's (u, v) as they are
struct CastHit {
    Hit h;
    uint32_t feature;
};

// the lane's box growth: elo is subtracted from every lo, ehi from every hi.  rad == 0: both +0 (x - +0 == x for every x: the
// boxes are the ray query's, bit for bit); else elo = e, ehi = -e (hi - (-e) is fl(hi + e)).  Every lane reads the root run.
__device__ __forceinline__ void cast_grow(const CastParams& p, float rad, float& elo, float& ehi)
{
    float M = 0.0f;
    const uint4* np = reinterpret_cast<const uint4*>(p.nodes + (p.root & kIndexMask));
    for (uint32_t k = 0; k < p.count; k++) {
        const uint4 a = np[2 * k], b = np[2 * k + 1];
        if ((b.w >> 29) == RT_CHILD_NONE) continue;
        M = fmaxf(M, fmaxf(fmaxf(fabsf(__uint_as_float(a.x)), fabsf(__uint_as_float(a.y))), fabsf(__uint_as_float(a.z))));
        M = fmaxf(M, fmaxf(fmaxf(fabsf(__uint_as_float(b.x)), fabsf(__uint_as_float(b.y))), fabsf(__uint_as_float(b.z))));
    }
    const float pad = kCastPad * fmaxf(rad, M);
    const float e = rad + pad;
    elo = rad == 0.0f ? 0.0f : e;
    ehi = rad == 0.0f ? 0.0f : -e;
}

__device__ __forceinline__ void cast_grow_slot(uint4& a, uint4& b, float elo, float ehi)
{
    a.x = __float_as_uint(__uint_as_float(a.x) - elo);
    a.y = __float_as_uint(__uint_as_float(a.y) - elo);
    a.z = __float_as_uint(__uint_as_float(a.z) - elo);
    b.x = __float_as_uint(__uint_as_float(b.x) - ehi);
    b.y = __float_as_uint(__uint_as_float(b.y) - ehi);
    b.z = __float_as_uint(__uint_as_float(b.z) - ehi);
}

// box_step<false> on grown slots: the same four loads, the same tests (box_step_on itself)
__device__ __forceinline__ void cast_box_step(const CastParams& p, const Ray& r, Trav& t, float elo, float ehi)
{
    const uint32_t cnt = t.cur >> 29;
    const uint4* np = reinterpret_cast<const uint4*>(p.nodes + (t.cur & kIndexMask));
    const bool two = cnt > 1;
    const int o1 = two ? 2 : 0;
    uint4 a0 = np[0], b0 = np[1], a1 = np[o1], b1 = np[o1 + 1];
    cast_grow_slot(a0, b0, elo, ehi);
    cast_grow_slot(a1, b1, elo, ehi);
    box_step_on<false>(p, r, t, two, a0, b0, a1, b1);
}

// the entry root of the capsule (a, b, rad): the capsule block's steps up to its entry, nothing of its exit.  False: no entry
// (a NaN included).  t is the ray's parameter, v the axial position (exactly 0 / 1 on a's / b's end sphere).  a == b: the
// sphere block's near root about a, v = 0.
__device__ __forceinline__ bool cast_edge_entry(float ax, float ay, float az, float bx, float by, float bz, const Ray& r,
                                                float rad, float& t, float& v)
{
    const float nx = bx - ax, ny = by - ay, nz = bz - az;
    const float a = (r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz;
    if ((nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f)) {
        const CapRoots c = cap_roots(r.ox - ax, r.oy - ay, r.oz - az, r, a, rad);
        t = c.near;
        v = 0.0f;
        return c.ok;
    }
    const float fx = r.ox - (ax * 0.5f + bx * 0.5f), fy = r.oy - (ay * 0.5f + by * 0.5f), fz = r.oz - (az * 0.5f + bz * 0.5f);
    const float b = -((fx * r.dx + fy * r.dy) + fz * r.dz);
    const float s = b / a;
    const float qx = fx + s * r.dx, qy = fy + s * r.dy, qz = fz + s * r.dz;
    const float nn = (nx * nx + ny * ny) + nz * nz;
    const float nd = (nx * r.dx + ny * r.dy) + nz * r.dz;
    const float nq = (nx * qx + ny * qy) + nz * qz;
    const float qd = (qx * r.dx + qy * r.dy) + qz * r.dz;
    const float qq = (qx * qx + qy * qy) + qz * qz;
    const float A = nn * a - nd * nd;
    const float C = nn * (qq - rad * rad) - nq * nq;
    const float hn = nn * 0.5f;
    float entry;
    bool ok;
    if (A > 0.0f) {
        const float B = nn * qd - nq * nd;
        const float hd = B * B - A * C;
        if (!(hd >= 0.0f)) return false;
        const float tau1 = (-B - sqrtf(hd)) / A;
        const float y1 = nq + tau1 * nd;
        ok = capsule_crossing<false>(tau1, y1, nn, hn, nx, ny, nz, qx, qy, qz, r, a, rad, entry, v);
    } else {   // parallel to the edge: in through the end sphere the ray meets first
        if (C > 0.0f) return false;
        const float side = nd > 0.0f ? 0.5f : -0.5f;
        const CapRoots ce = cap_roots(qx + side * nx, qy + side * ny, qz + side * nz, r, a, rad);
        entry = ce.near;
        v = nd > 0.0f ? 0.0f : 1.0f;
        ok = ce.ok;
    }
    t = s + entry;
    return ok;
}

// the test of one leaf triangle with stored corners s0, s1, s2 and rotation rot, rad > 0; true: accepted, r.tmax = t
__device__ __forceinline__ bool cast_tri(float s0x, float s0y, float s0z, float s1x, float s1y, float s1z, float s2x, float s2y,
                                         float s2z, uint32_t rot, Ray& r, float rad, CastHit& ch, uint32_t tri_id,
                                         uint32_t prim_id)
{
    // 1. initial overlap: the range query's predicate on (c0, rad*rad)
    {
        const float cx = r.ox + r.tmin * r.dx, cy = r.oy + r.tmin * r.dy, cz = r.oz + r.tmin * r.dz;
        float u = 0.0f, v = 0.0f;
        const float d2 = tri_d2<true>(cx, cy, cz, unrotate(s0x, s0y, s0z, s1x, s1y, s1z, s2x, s2y, s2z, rot), u, v);
        if (d2 <= rad * rad) {
            r.tmax = r.tmin;
            ch.h.primitive_id = prim_id;
            ch.h.tri_id = tri_id;
            ch.h.bu = u;
            ch.h.bv = v;
            ch.feature = RT_SWEEP_OVERLAP;
            return true;
        }
    }
    bool hit = false;
    // 2. the facing offset face
    {
        const float e1x = s1x - s0x, e1y = s1y - s0y, e1z = s1z - s0z;
        const float e2x = s2x - s0x, e2y = s2y - s0y, e2z = s2z - s0z;
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        if (len > 0.0f) {   // (zero area, a NaN: no face)
            const float dn = (r.dx * nx + r.dy * ny) + r.dz * nz;
            const float k = dn < 0.0f ? -rad : rad;
            Ray f = r;
            f.ox = r.ox + k * (nx / len);
            f.oy = r.oy + k * (ny / len);
            f.oz = r.oz + k * (nz / len);
            if (intersect_tri(s0x, s0y, s0z, s1x, s1y, s1z, s2x, s2y, s2z, f, ch.h, tri_id, prim_id)) {
                r.tmax = f.tmax;
                ch.feature = RT_SWEEP_FACE;
                hit = true;
            }
        }
    }
    // 3. the edges s0-s1, s1-s2, s2-s0, in that order
    float t, v;
    if (cast_edge_entry(s0x, s0y, s0z, s1x, s1y, s1z, r, rad, t, v) && (t >= r.tmin) & (t <= r.tmax)) {
        r.tmax = t; ch.h.bu = v; ch.h.bv = 0.0f; hit = true;
        ch.h.primitive_id = prim_id; ch.h.tri_id = tri_id;
        ch.feature = ((v > 0.0f) & (v < 1.0f)) ? RT_SWEEP_EDGE : RT_SWEEP_CORNER;
    }
    if (cast_edge_entry(s1x, s1y, s1z, s2x, s2y, s2z, r, rad, t, v) && (t >= r.tmin) & (t <= r.tmax)) {
        r.tmax = t; ch.h.bu = 1.0f - v; ch.h.bv = v; hit = true;
        ch.h.primitive_id = prim_id; ch.h.tri_id = tri_id;
        ch.feature = ((v > 0.0f) & (v < 1.0f)) ? RT_SWEEP_EDGE : RT_SWEEP_CORNER;
    }
    if (cast_edge_entry(s2x, s2y, s2z, s0x, s0y, s0z, r, rad, t, v) && (t >= r.tmin) & (t <= r.tmax)) {
        r.tmax = t; ch.h.bu = 0.0f; ch.h.bv = 1.0f - v; hit = true;
        ch.h.primitive_id = prim_id; ch.h.tri_id = tri_id;
        ch.feature = ((v > 0.0f) & (v < 1.0f)) ? RT_SWEEP_EDGE : RT_SWEEP_CORNER;
    }
    return hit;
}

// one leaf triangle for a lane of either kind
__device__ __forceinline__ bool cast_leaf_tri(float s0x, float s0y, float s0z, float s1x, float s1y, float s1z, float s2x,
                                              float s2y, float s2z, uint32_t rot, Ray& r, float rad, CastHit& ch,
                                              uint32_t tri_id, uint32_t prim_id)
{
    if (rad == 0.0f) {   // the ray query's leaf test
        const bool hit = intersect_tri(s0x, s0y, s0z, s1x, s1y, s1z, s2x, s2y, s2z, r, ch.h, tri_id, prim_id);
        if (hit) ch.feature = RT_SWEEP_FACE;
        return hit;
    }
    return cast_tri(s0x, s0y, s0z, s1x, s1y, s1z, s2x, s2y, s2z, rot, r, rad, ch, tri_id, prim_id);
}

// trace_plain's policy: the growth made once per ray, the grown box step, trace_ray's leaf phase with the cast's triangle test
struct CastWalk {
    CastHit& ch;
    const float rad;
    float elo, ehi;
    __device__ __forceinline__ void begin(const CastParams& p) { cast_grow(p, rad, elo, ehi); }
    __device__ __forceinline__ void box(const CastParams& p, const Ray& r, Trav& t) { cast_box_step(p, r, t, elo, ehi); }
    __device__ __forceinline__ bool leaf(const CastParams& p, Ray& r, Trav& t)
    {
        t.tri_tests++;
        const uint32_t li = t.leaf & kIndexMask;
        uint4 l0, l1, l2, l3;
        load_leaf_wide(p.leaves + li, l0, l1, l2, l3);
        bool hit = cast_leaf_tri(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z), __uint_as_float(l1.x),
                                 __uint_as_float(l1.y), __uint_as_float(l1.z), __uint_as_float(l2.x), __uint_as_float(l2.y),
                                 __uint_as_float(l2.z), l2.w & 0xFFFFu, r, rad, ch, li << 1, l0.w);
        // triangle B = (v2, v1, v3), skipped when v3 == v2 bit for bit (a single triangle), as the ray query skips it.  Its
        // edge v2-v1 is A's edge v1-v2: tested again, as B's own.  (Any-hit tests B after a hit on A too: the ray query does)
        if ((t.leaf >> 29) > 0 && (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z))
            hit |= cast_leaf_tri(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), __uint_as_float(l1.x),
                                 __uint_as_float(l1.y), __uint_as_float(l1.z), __uint_as_float(l3.x), __uint_as_float(l3.y),
                                 __uint_as_float(l3.z), l2.w >> 16, r, rad, ch, (li << 1) + 1, l1.w);
        return hit;
    }
};

// Returns whether a triangle was accepted; steps[0] / steps[1] as trace_ray.
template <bool ANY>
__device__ __forceinline__ bool trace_sphere_cast(const CastParams& p, Ray& r, float rad, CastHit& ch, Trav& t, bool active,
                                                  uint32_t* steps)
{
    CastWalk w = {ch, rad, 0.0f, 0.0f};
    return trace_plain<ANY>(p, r, t, active, steps, w);
}

}  // namespace

}  // namespace rt
