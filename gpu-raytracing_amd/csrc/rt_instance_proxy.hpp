// rt_instance_proxy.hpp -- what the two prepare kernels share (prepare_instances_kernel of instances.hip and
// prepare_motion_instances_kernel of instance_motion_query.hip): the object box of an instance's BLAS and the proxy triangle
// of that box under one object_to_world matrix (rt_abi.h, instancing block: corner order, ordered min / max, the 2^-12 pad).
// One copy of the arithmetic, so the proxies of a moving instance are byte for byte rt_prepare_instances's, pose by pose.
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"

namespace rt {

namespace {   // (as in the kernels' own files)

constexpr float kInstancePad = 1.0f / 4096.0f;      // 2^-12 of the box's largest |bound| (rt_abi.h)

// the object box of table entry `blas`: ordered min / max over the non-NONE slots of the root run, as ordered ints.
// (lo_i / hi_i come in as the empty box: INT_MAX / INT_MIN).  Sets RT_INSTANCE_BAD_BLAS in flags when there is no such entry,
// it is unusable or its root run has no slot.
__device__ __forceinline__ void instance_object_box(const rt_accel* blas_table, uint32_t num_blas, uint32_t blas,
                                                    int (&lo_i)[3], int (&hi_i)[3], uint32_t& flags)
{
    bool any = false;
    if (blas >= num_blas) flags |= RT_INSTANCE_BAD_BLAS;
    else {
        const rt_accel a = blas_table[blas];
        if (a.count == 0 || a.count > 7 || !a.nodes || !a.triangles) flags |= RT_INSTANCE_BAD_BLAS;
        else {
            for (uint32_t s = 0; s < a.count; s++) {
                const rt_node nd = a.nodes[(a.root & kIndexMask) + s];
                if ((nd.w28 >> 29) == RT_CHILD_NONE) continue;
                any = true;
                const float mn[3] = {nd.min.x, nd.min.y, nd.min.z}, mx[3] = {nd.max.x, nd.max.y, nd.max.z};
                for (int k = 0; k < 3; k++) {
                    lo_i[k] = min(lo_i[k], float_to_ordered_int(mn[k]));
                    hi_i[k] = max(hi_i[k], float_to_ordered_int(mx[k]));
                }
            }
            if (!any) flags |= RT_INSTANCE_BAD_BLAS;
        }
    }
}

// The padded world box of the object box under m (row-major 3x4): the 8 corners through m as ((m0*x + m1*y) + m2*z) + m3,
// their ordered min / max (-0 below +0: no dependence on fminf's zero rule), every bound moved outward by the pad.  Matrix in
// and box out travel BY VALUE: a caller's locals whose address went into this call would be promoted to registers only after
// inlining, and prepare_instances_kernel would no longer compile to the code it had with this arithmetic written in place.
struct Affine34 { float m[12]; };
struct Box3 { float lo[3], hi[3]; };
__device__ __forceinline__ Box3 instance_proxy(Affine34 mm, const int (&lo_i)[3], const int (&hi_i)[3])
{
    const float* m = mm.m;
    float lo[3], hi[3], b0[3], b1[3];
    int clo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, chi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    for (int k = 0; k < 3; k++) { b0[k] = ordered_int_to_float(lo_i[k]); b1[k] = ordered_int_to_float(hi_i[k]); }
    for (int c = 0; c < 8; c++) {
        const float x = (c & 1) ? b1[0] : b0[0], y = (c & 2) ? b1[1] : b0[1], z = (c & 4) ? b1[2] : b0[2];
        for (int k = 0; k < 3; k++) {
            const float v = ((m[4 * k] * x + m[4 * k + 1] * y) + m[4 * k + 2] * z) + m[4 * k + 3];
            clo[k] = min(clo[k], float_to_ordered_int(v));
            chi[k] = max(chi[k], float_to_ordered_int(v));
        }
    }
    for (int k = 0; k < 3; k++) { lo[k] = ordered_int_to_float(clo[k]); hi[k] = ordered_int_to_float(chi[k]); }
    float e = 0.0f;
    for (int k = 0; k < 3; k++) e = fmaxf(e, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
    const float pad = e * kInstancePad;
    for (int k = 0; k < 3; k++) { lo[k] = lo[k] - pad; hi[k] = hi[k] + pad; }
    return {{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
}

// the proxy triangle of such a box: {lo, hi, midpoint} -- its box is exactly [lo, hi] and its centroid lies inside it
__device__ __forceinline__ rt_triangle proxy_triangle(const Box3& bx)
{
    const float *lo = bx.lo, *hi = bx.hi;
    rt_triangle px;
    px.v0 = {lo[0], lo[1], lo[2]};
    px.v1 = {hi[0], hi[1], hi[2]};
    px.v2 = {lo[0] * 0.5f + hi[0] * 0.5f, lo[1] * 0.5f + hi[1] * 0.5f, lo[2] * 0.5f + hi[2] * 0.5f};
    return px;
}

}  // namespace

}  // namespace rt
