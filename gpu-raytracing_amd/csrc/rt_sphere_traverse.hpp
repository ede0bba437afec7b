// rt_sphere_traverse.hpp -- the traversal of the sphere ray query of sphere_query.hip (rt_intersect_rays_spheres): a tree any
// builder made over rt_prepare_spheres's proxy triangles, walked by trace_ray's box phase, with a sphere test where trace_ray
// tests a leaf's triangles.  The slab test, the ordered compares and the nearest-child choice of box_step, Trav's stack and
// second_slot are rt_traverse.hpp's code, called from here.  What this file adds is the leaf phase -- the leaf's first 16
// bytes for the sphere index (its primitive_id_0, as the TLAS leaf read of rt_instance_traverse.hpp), spheres[id] as one
// 16-byte load, the test below -- and SphereWalk, the policy that hands box_step and that leaf phase to trace_plain
// (rt_plain_traverse.hpp: trace_ray's non-QW vote / park loop, written once; no PF arm).
//
// The test (rt_abi.h, sphere block, has it operation by operation): the discriminant comes from the perpendicular offset
// p = f + s*d of the centre from the ray's line, not from b*b - a*c.  Every operation is rounded on its own
// (-ffp-contract=off), the two divisions are IEEE and the square root is correctly rounded.
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"
#include "rt_plain_traverse.hpp"
#include "rt_traverse.hpp"

// waves per SIMD the sphere kernel's register allocation must fit: ray_query_kernel<false, ..>'s (64 VGPRs; DESIGN section
// 24 has the compiler's figures)
#ifndef RT_SPHERE_WAVES
#define RT_SPHERE_WAVES (RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA)
#endif

namespace rt {

namespace {   // (as in the kernels' own file)

struct SphereParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* spheres;   // rt_sphere = one float4: (centre, radius)
    uint32_t num_spheres;
    const float4* rays;      // rt_ray = two float4: (origin, tmin), (dir, tmax)
    float4* hits;            // rt_hit = one float4: (t, sphere index bits, far-root flag, 0)
    uint32_t num_rays;
    unsigned long long* counters;
    const uint32_t* order;   // INDEXED instantiations only
    uint32_t num_indices;
    static constexpr int park_num = kParkNum, park_den = kParkDen;
};

// a ray's hit so far: the sphere and which root of it (r.tmax carries t)
struct SphereHit {
    uint32_t id;
    float far_root;   // 1.0f: t_far was taken (the ray began inside the sphere), else 0.0f
};

// the sphere test; true: accepted, r.tmax = t.  A NaN anywhere rejects (a ray without a direction: a = 0, s = NaN).
__device__ __forceinline__ bool intersect_sphere(const float4& sp, Ray& r, SphereHit& h, uint32_t id)
{
    const float fx = r.ox - sp.x, fy = r.oy - sp.y, fz = r.oz - sp.z;
    const float a = (r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz;
    const float b = -((fx * r.dx + fy * r.dy) + fz * r.dz);
    const float s = b / a;
    const float px = fx + s * r.dx, py = fy + s * r.dy, pz = fz + s * r.dz;
    const float l2 = (px * px + py * py) + pz * pz;
    const float disc = sp.w * sp.w - l2;
    if (!(disc >= 0.0f)) return false;
    const float hh = sqrtf(disc / a);
    const float t_near = s - hh, t_far = s + hh;
    const bool near_ok = (t_near >= r.tmin) & (t_near <= r.tmax);
    const bool far_ok = (t_far >= r.tmin) & (t_far <= r.tmax);
    if (!(near_ok | far_ok)) return false;
    r.tmax = near_ok ? t_near : t_far;
    h.id = id;
    h.far_root = near_ok ? 0.0f : 1.0f;
    return true;
}

// the leaf phase's work for one parked lane: the sphere index, the sphere, the test.  A leaf whose index is not below
// num_spheres and a sphere that is not valid (a negative, NaN or infinite radius) are skipped: no test counted.
__device__ __forceinline__ bool sphere_leaf_test(const SphereParams& p, Ray& r, SphereHit& h, Trav& t)
{
    const uint32_t id = reinterpret_cast<const uint4*>(p.leaves + (t.leaf & kIndexMask))[0].w;
    if (id >= p.num_spheres) return false;
    const float4 sp = p.spheres[id];
    if (!(sp.w >= 0.0f) || sp.w == __builtin_inff()) return false;
    t.tri_tests++;
    return intersect_sphere(sp, r, h, id);
}

// trace_plain's policy: trace_ray's box step, the leaf phase above
struct SphereWalk {
    SphereHit& h;
    __device__ __forceinline__ void begin(const SphereParams&) {}
    __device__ __forceinline__ void box(const SphereParams& p, const Ray& r, Trav& t) { box_step<false>(p, r, t); }
    __device__ __forceinline__ bool leaf(const SphereParams& p, Ray& r, Trav& t) { return sphere_leaf_test(p, r, h, t); }
};

// Returns whether a sphere was accepted; steps[0] / steps[1] as trace_ray.
template <bool ANY>
__device__ __forceinline__ bool trace_ray_spheres(const SphereParams& p, Ray& r, SphereHit& h, Trav& t, bool active,
                                                  uint32_t* steps)
{
    SphereWalk w = {h};
    return trace_plain<ANY>(p, r, t, active, steps, w);
}

}  // namespace

}  // namespace rt
