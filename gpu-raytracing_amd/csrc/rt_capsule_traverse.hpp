// rt_capsule_traverse.hpp -- the traversal of the capsule ray query of capsule_query.hip (rt_intersect_rays_capsules): a tree
// any builder made over rt_prepare_capsules's proxy triangles, walked by trace_ray's box phase, with a capsule test where
// trace_ray tests a leaf's triangles.  The slab test, the ordered compares and the nearest-child choice of box_step, Trav's
// stack and second_slot are rt_traverse.hpp's code and intersect_sphere is rt_sphere_traverse.hpp's, called from here.  What
// this file adds is the leaf phase -- the leaf's first 16 bytes for the capsule index (its primitive_id_0), capsules[id] as
// two independent 16-byte loads, the test below -- as CapsuleWalk, the policy that hands box_step and that leaf phase to
// trace_plain (rt_plain_traverse.hpp: the plain vote / park loop trace_ray_spheres walks through; no PF arm, no hold at pop).
//
// The test (rt_abi.h, capsule block, has it operation by operation): the ray is re-based at its point nearest the capsule's
// midpoint, so no term is of the size of |o - m|^2; the infinite cylinder's roots pick the body or, by the side on which
// they leave it, one end sphere, whose roots come from the sphere block's steps.  Every operation is rounded on its own
// (-ffp-contract=off), the divisions are IEEE and the square roots correctly rounded.
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"
#include "rt_sphere_traverse.hpp"
#include "rt_plain_traverse.hpp"
#include "rt_traverse.hpp"

// waves per SIMD the capsule kernel's register allocation must fit: one step below the sphere kernel's 8.  The leaf keeps the
// re-based ray and the axis live across two cap evaluations: at 8 waves (64 VGPRs) 21 registers spill, at 7 (72) 8, at 6 (79)
// none; tools/capsule_bench.py put 7 ahead of both (DESIGN section 26 has the compiler's figures and the rates)
#ifndef RT_CAPSULE_WAVES
#define RT_CAPSULE_WAVES 7
#endif

namespace rt {

namespace {   // (as in the kernels' own file)

struct CapsuleParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* capsules;   // rt_capsule = two float4: (p0, radius), (p1, pad)
    uint32_t num_capsules;
    const float4* rays;       // rt_ray = two float4: (origin, tmin), (dir, tmax)
    float4* hits;             // rt_hit = one float4: (t, capsule index bits, far-root flag, axial parameter)
    uint32_t num_rays;
    unsigned long long* counters;
    const uint32_t* order;    // INDEXED instantiations only
    uint32_t num_indices;
    static constexpr int park_num = kParkNum, park_den = kParkDen;
};

// a ray's hit so far: the capsule, which root of it and where along its axis (r.tmax carries t)
struct CapsuleHit {
    uint32_t id;
    float far_root;   // 1.0f: t_far was taken (the ray began inside the capsule), else 0.0f
    float v;          // 0 on p0's cap .. 1 on p1's cap
};

// the sphere block's steps on the offset g of the re-based ray's origin from an end point: the roots in tau
struct CapRoots {
    float near, far;
    bool ok;   // disc >= 0
};

__device__ __forceinline__ CapRoots cap_roots(float gx, float gy, float gz, const Ray& r, float a, float rad)
{
    const float b = -((gx * r.dx + gy * r.dy) + gz * r.dz);
    const float s = b / a;
    const float px = gx + s * r.dx, py = gy + s * r.dy, pz = gz + s * r.dz;
    const float l2 = (px * px + py * py) + pz * pz;
    const float disc = rad * rad - l2;
    const float hh = sqrtf(disc / a);
    return CapRoots{s - hh, s + hh, disc >= 0.0f};
}

// one crossing of the capsule's surface: the cylinder root tau at axial position y when that lies in the body, else the
// root (near or far) of the end sphere on y's side
template <bool FAR>
__device__ __forceinline__ bool capsule_crossing(float tau, float y, float nn, float hn, float nx, float ny, float nz, float qx,
                                                 float qy, float qz, const Ray& r, float a, float rad, float& out, float& v)
{
    if ((y > -hn) & (y < hn)) {
        out = tau;
        v = y / nn + 0.5f;
        return true;
    }
    const float side = y <= -hn ? 0.5f : -0.5f;   // +: p0's cap (fa = q + 0.5*n), -: p1's (fb = q - 0.5*n)
    const CapRoots c = cap_roots(qx + side * nx, qy + side * ny, qz + side * nz, r, a, rad);
    out = FAR ? c.far : c.near;
    v = y <= -hn ? 0.0f : 1.0f;
    return c.ok;
}

// the capsule test; true: accepted, r.tmax = t.  A NaN anywhere rejects.
__device__ __forceinline__ bool intersect_capsule(const float4& c0, const float4& c1, Ray& r, CapsuleHit& h, uint32_t id)
{
    const float nx = c1.x - c0.x, ny = c1.y - c0.y, nz = c1.z - c0.z;
    if ((nx == 0.0f) & (ny == 0.0f) & (nz == 0.0f)) {   // a sphere: the sphere block's test, bit for bit
        SphereHit sh = {0u, 0.f};
        if (!intersect_sphere(c0, r, sh, id)) return false;
        h.id = id;
        h.far_root = sh.far_root;
        h.v = 0.0f;
        return true;
    }
    const float rad = c0.w;
    const float fx = r.ox - (c0.x * 0.5f + c1.x * 0.5f), fy = r.oy - (c0.y * 0.5f + c1.y * 0.5f),
                fz = r.oz - (c0.z * 0.5f + c1.z * 0.5f);
    const float a = (r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz;
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
    float entry, exit, ve, vx;
    bool ok;
    if (A > 0.0f) {
        const float B = nn * qd - nq * nd;
        const float hd = B * B - A * C;
        if (!(hd >= 0.0f)) return false;
        const float sq = sqrtf(hd);
        const float tau1 = (-B - sq) / A, tau2 = (-B + sq) / A;
        const float y1 = nq + tau1 * nd, y2 = nq + tau2 * nd;
        ok = capsule_crossing<false>(tau1, y1, nn, hn, nx, ny, nz, qx, qy, qz, r, a, rad, entry, ve);
        ok &= capsule_crossing<true>(tau2, y2, nn, hn, nx, ny, nz, qx, qy, qz, r, a, rad, exit, vx);
    } else {   // parallel to the axis (a rounded-negative or NaN A included): through one cap, out of the other
        if (C > 0.0f) return false;
        const float side = nd > 0.0f ? 0.5f : -0.5f;
        const CapRoots ce = cap_roots(qx + side * nx, qy + side * ny, qz + side * nz, r, a, rad);
        const CapRoots cx = cap_roots(qx - side * nx, qy - side * ny, qz - side * nz, r, a, rad);
        entry = ce.near;
        exit = cx.far;
        ve = nd > 0.0f ? 0.0f : 1.0f;
        vx = nd > 0.0f ? 1.0f : 0.0f;
        ok = ce.ok & cx.ok;
    }
    if (!ok) return false;
    const float t_near = s + entry, t_far = s + exit;
    const bool near_ok = (t_near >= r.tmin) & (t_near <= r.tmax);
    const bool far_ok = (t_far >= r.tmin) & (t_far <= r.tmax);
    if (!(near_ok | far_ok)) return false;
    r.tmax = near_ok ? t_near : t_far;
    h.id = id;
    h.far_root = near_ok ? 0.0f : 1.0f;
    h.v = near_ok ? ve : vx;
    return true;
}

// trace_plain's policy: trace_ray's box step, the capsule test at the leaf
struct CapsuleWalk {
    CapsuleHit& h;
    __device__ __forceinline__ void begin(const CapsuleParams&) {}
    __device__ __forceinline__ void box(const CapsuleParams& p, const Ray& r, Trav& t) { box_step<false>(p, r, t); }
    // the leaf phase's work for one parked lane: the capsule index, the capsule, the test.  A leaf whose index is not below
    // num_capsules and a capsule that is not valid (a negative, NaN or infinite radius) are skipped: no test counted.  (The
    // member is the leaf test itself, not a call of one: a level of calls between them renumbers three VGPRs of the kernels)
    __device__ __forceinline__ bool leaf(const CapsuleParams& p, Ray& r, Trav& t)
    {
        const uint32_t id = reinterpret_cast<const uint4*>(p.leaves + (t.leaf & kIndexMask))[0].w;
        if (id >= p.num_capsules) return false;
        const float4 c0 = p.capsules[2 * (uint64_t)id], c1 = p.capsules[2 * (uint64_t)id + 1];
        if (!(c0.w >= 0.0f) || c0.w == __builtin_inff()) return false;
        t.tri_tests++;
        return intersect_capsule(c0, c1, r, h, id);
    }
};

// Returns whether a capsule was accepted; steps[0] / steps[1] as trace_ray.
template <bool ANY>
__device__ __forceinline__ bool trace_ray_capsules(const CapsuleParams& p, Ray& r, CapsuleHit& h, Trav& t, bool active,
                                                   uint32_t* steps)
{
    CapsuleWalk w = {h};
    return trace_plain<ANY>(p, r, t, active, steps, w);
}

}  // namespace

}  // namespace rt
