// rt_point_math.hpp -- the float32 routines of rt_abi.h's closest-point block, shared by every query that needs a point-triangle
// distance: point_query.hip (closest point, with the weights), knn_query.hip (k nearest), range_query.hip (sphere ranges) and
// sdf_query.hip (the distance phase).  d2 (Ericson, the clamp into the vertex box, the squared distance) with or without the
// weights, the corner un-rotation of pair leaves, boxdist2 of a slot and the entry a slot refers to; and the constants of the
// nearest-first descent that the three ordered queries must agree on.  Float routines only -- no traversal, no kernel scaffold.
// Device code only; every function is force-inlined into its kernel.  Compile with -ffp-contract=off and IEEE division: every
// float operation is the one rt_abi.h writes down.
#pragma once

#include "rt_device.hpp"

namespace rt {

namespace {

__device__ __forceinline__ float pm_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return (ax * bx + ay * by) + az * bz;
}
// a denominator that is not > 0 (0, negative, NaN) gives weight 0; else the IEEE quotient
__device__ __forceinline__ float pm_guard(float num, float den) { return den > 0.0f ? num / den : 0.0f; }
// by selects: NaN -> 0, -0 -> +0
__device__ __forceinline__ float pm_clamp01(float t)
{
    t = t > 0.0f ? t : 0.0f;
    return t < 1.0f ? t : 1.0f;
}

// rt_abi.h's FACE_NOISE: a face sum at or below this share of the magnitudes of its six products is rounding noise
constexpr float kFaceNoise = 0x1p-20f;

struct Tri {
    float ax, ay, az, bx, by, bz, cx, cy, cz;
};

// dist2 of p to q after q is clamped into the triangle's vertex box (fmaxf, then fminf)
__device__ __forceinline__ float pm_clamped(float px, float py, float pz, float qx, float qy, float qz, const Tri& t)
{
    const float lox = fminf(fminf(t.ax, t.bx), t.cx), loy = fminf(fminf(t.ay, t.by), t.cy), loz = fminf(fminf(t.az, t.bz), t.cz);
    const float hix = fmaxf(fmaxf(t.ax, t.bx), t.cx), hiy = fmaxf(fmaxf(t.ay, t.by), t.cy), hiz = fmaxf(fmaxf(t.az, t.bz), t.cz);
    const float dx = px - fminf(fmaxf(qx, lox), hix);
    const float dy = py - fminf(fmaxf(qy, loy), hiy);
    const float dz = pz - fminf(fmaxf(qz, loz), hiz);
    return (dx * dx + dy * dy) + dz * dz;
}

// d2(p, a, b, c) of rt_abi.h's closest-point block: Ericson's ClosestPtPointTriangle (RTCD 5.1.5), the clamp into the vertex
// box, the squared distance.  WEIGHTS: u, v get the weights of b and c (else they are left alone).  One routine for every
// caller, so a fix lands once; the float operations and the value returned do not depend on WEIGHTS.
template <bool WEIGHTS>
__device__ __forceinline__ float tri_d2(float px, float py, float pz, const Tri& t, float& u, float& v)
{
    auto weights = [&](float wu, float wv) { if constexpr (WEIGHTS) { u = wu; v = wv; } };
    const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
    const float acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
    const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
    const float d1 = pm_dot(abx, aby, abz, apx, apy, apz), d2 = pm_dot(acx, acy, acz, apx, apy, apz);
    if (d1 <= 0.0f && d2 <= 0.0f) {                                     // vertex region A
        weights(0.0f, 0.0f);
        return pm_clamped(px, py, pz, t.ax, t.ay, t.az, t);
    }
    const float bpx = px - t.bx, bpy = py - t.by, bpz = pz - t.bz;
    const float d3 = pm_dot(abx, aby, abz, bpx, bpy, bpz), d4 = pm_dot(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0f && d4 <= d3) {                                       // vertex region B
        weights(1.0f, 0.0f);
        return pm_clamped(px, py, pz, t.bx, t.by, t.bz, t);
    }
    const float vc = d1 * d4 - d3 * d2;
    const float t_ab = pm_clamp01(pm_guard(d1, d1 - d3));
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f && d1 - d3 > 0.0f) {    // edge region AB (of an edge that has a length)
        weights(t_ab, 0.0f);
        return pm_clamped(px, py, pz, t.ax + t_ab * abx, t.ay + t_ab * aby, t.az + t_ab * abz, t);
    }
    const float cpx = px - t.cx, cpy = py - t.cy, cpz = pz - t.cz;
    const float d5 = pm_dot(abx, aby, abz, cpx, cpy, cpz), d6 = pm_dot(acx, acy, acz, cpx, cpy, cpz);
    if (d6 >= 0.0f && d5 <= d6) {                                       // vertex region C
        weights(0.0f, 1.0f);
        return pm_clamped(px, py, pz, t.cx, t.cy, t.cz, t);
    }
    const float vb = d5 * d2 - d1 * d6;
    const float t_ac = pm_clamp01(pm_guard(d2, d2 - d6));
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f && d2 - d6 > 0.0f) {    // edge region AC
        weights(0.0f, t_ac);
        return pm_clamped(px, py, pz, t.ax + t_ac * acx, t.ay + t_ac * acy, t.az + t_ac * acz, t);
    }
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const float t_bc = pm_clamp01(pm_guard(e43, e43 + e56));
    const float bcx = t.cx - t.bx, bcy = t.cy - t.by, bcz = t.cz - t.bz;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f && e43 + e56 > 0.0f) {   // edge region BC
        weights(1.0f - t_bc, t_bc);
        return pm_clamped(px, py, pz, t.bx + t_bc * bcx, t.by + t_bc * bcy, t.bz + t_bc * bcz, t);
    }
    // no vertex or edge region holds.  s is the squared area (times 4) as a sum of six products: where it stands clear of their
    // rounding noise, the face point as Ericson takes it
    const float s = (va + vb) + vc;
    const float noise = ((fabsf(d1 * d4) + fabsf(d3 * d2)) + (fabsf(d5 * d2) + fabsf(d1 * d6))) + (fabsf(d3 * d6) + fabsf(d5 * d4));
    const float fv = vb / s, fw = vc / s;
    const float qx = (t.ax + abx * fv) + acx * fw;
    const float qy = (t.ay + aby * fv) + acy * fw;
    const float qz = (t.az + abz * fv) + acz * fw;
    const float g_f = pm_clamped(px, py, pz, qx, qy, qz, t);
    if (s > kFaceNoise * noise) {                                       // (false for a NaN)
        weights(fv, fw);
        return g_f;
    }
    // a face whose area is rounding noise (a collinear triangle: va, vb, vc are residues of any sign): the nearest of the three
    // edge points (ties: AB, then AC), unless the face point is a point of the triangle and no edge point is strictly nearer
    float best = pm_clamped(px, py, pz, t.ax + t_ab * abx, t.ay + t_ab * aby, t.az + t_ab * abz, t);
    weights(t_ab, 0.0f);
    const float g_ac = pm_clamped(px, py, pz, t.ax + t_ac * acx, t.ay + t_ac * acy, t.az + t_ac * acz, t);
    if (g_ac < best) { best = g_ac; weights(0.0f, t_ac); }
    const float g_bc = pm_clamped(px, py, pz, t.bx + t_bc * bcx, t.by + t_bc * bcy, t.bz + t_bc * bcz, t);
    if (g_bc < best) { best = g_bc; weights(1.0f - t_bc, t_bc); }
    if (s > 0.0f && fv >= 0.0f && fw >= 0.0f && fv + fw <= 1.0f && !(best < g_f)) { best = g_f; weights(fv, fw); }
    return best;
}
// d2 alone: what knn_query.hip, range_query.hip and sdf_query.hip ask for
__device__ __forceinline__ float range_tri_d2(float px, float py, float pz, const Tri& t)
{
    float u, v;
    return tri_d2<false>(px, py, pz, t, u, v);
}

// the caller's corners of a leaf triangle stored as (s0, s1, s2) with rotation r (RotateAttributes' corner map):
// r = 1: (c0, c1, c2) = (s1, s2, s0); r = 2: (s2, s0, s1); else as stored
__device__ __forceinline__ Tri unrotate(float s0x, float s0y, float s0z, float s1x, float s1y, float s1z, float s2x, float s2y,
                                        float s2z, uint32_t r)
{
    Tri t;
    if (r == 1) t = {s1x, s1y, s1z, s2x, s2y, s2z, s0x, s0y, s0z};
    else if (r == 2) t = {s2x, s2y, s2z, s0x, s0y, s0z, s1x, s1y, s1z};
    else t = {s0x, s0y, s0z, s1x, s1y, s1z, s2x, s2y, s2z};
    return t;
}

// the two triangles of a 64-byte leaf record (l0 .. l3: its four 16-byte quarters) with the caller's corner order: A = (v0, v1,
// v2) with rotations[0]; B = (v2, v1, v3) with rotations[1], present iff primitive_id_1 == primitive_id_0 + 1
__device__ __forceinline__ Tri leaf_tri_a(const uint4& l0, const uint4& l1, const uint4& l2)
{
    return unrotate(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z), __uint_as_float(l1.x), __uint_as_float(l1.y),
                    __uint_as_float(l1.z), __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), l2.w & 0xFFFFu);
}
__device__ __forceinline__ Tri leaf_tri_b(const uint4& l1, const uint4& l2, const uint4& l3)
{
    return unrotate(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), __uint_as_float(l1.x), __uint_as_float(l1.y),
                    __uint_as_float(l1.z), __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z), l2.w >> 16);
}

// boxdist2 of a slot: g = max(lo - p, p - hi, 0) per axis, squared and summed in d2's order
__device__ __forceinline__ float box_d2(const uint4& a, const uint4& b, float px, float py, float pz)
{
    const float gx = fmaxf(fmaxf(__uint_as_float(a.x) - px, px - __uint_as_float(b.x)), 0.0f);
    const float gy = fmaxf(fmaxf(__uint_as_float(a.y) - py, py - __uint_as_float(b.y)), 0.0f);
    const float gz = fmaxf(fmaxf(__uint_as_float(a.z) - pz, pz - __uint_as_float(b.z)), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

// the entry a slot refers to: a leaf (index : 29 | 0) or a box run (child : 29 | count : 3)
__device__ __forceinline__ uint32_t slot_entry(const uint4& a, const uint4& b)
{
    return (b.w >> 29) == RT_CHILD_TRI ? (b.w & kIndexMask) : ((b.w & kIndexMask) | (a.w & ~kIndexMask));
}

// The nearest-first descent of point_query.hip, knn_query.hip and the distance phase of sdf_query.hip: a stack entry is 8 bytes,
// the first kNearStackLds of a lane's kStackMax entries live in an LDS column (16 x 8 B x 256 lanes = 32 KB per workgroup), the
// rest in private memory; a pass that dropped a push is followed by another from the root with what it found, at most
// kNearRestarts more.  The descent itself is written out in each of the three kernels (shared, two of them measured slower:
// DESIGN section 17).  rt_signed_distance promises rt_closest_points's (dist2, primitive_id), dropped pushes included:
// tests/test_gpu_sdf.py::test_overflowed_distance_equals_closest_points holds the two texts together.
typedef uint64_t NearEntry;         // entry (low word) | boxdist2 bits (high word)
constexpr int kNearStackLds = 16;
constexpr int kNearRestarts = 2;

}  // namespace

}  // namespace rt
