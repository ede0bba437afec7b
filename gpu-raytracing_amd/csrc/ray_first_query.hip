// ray_first_query.hip -- rt_ray_first_hits: the K nearest crossings of each caller ray inside its [tmin, tmax] window, in
// ascending (t, primitive_id) order, through any tree rt_intersect_rays takes (semantics: rt_abi.h, first-K block; DESIGN
// section 19).  The fixed-length sibling of the all-hit query: row i has exactly k records, one launch, nothing counted,
// scanned or read back.
//
// ray_first_kernel is ray_hits_kernel's frame -- one lane per ray, 64 consecutive rays per wave, kTraceWaves waves (256 rays)
// per workgroup, xcd_chunk_block, the ray in two 16-byte loads, a leaf in four 16-byte requests, rt_traverse.hpp's wave-level
// two phases, exact per-workgroup counters, one status ballot per wave -- with slab() and intersect_tri() of rt_traverse.hpp
// unchanged, and knn_query_kernel's list in the place of the CSR segment.  What is new against the all-hit kernel:
//   * the bound b: the ray's original tmax while the list holds fewer than k records, the k-th record's t once it is full.  A
//     slot is entered iff back >= front && front <= b && back >= tmin; a triangle is tested against [tmin, b] (intersect_tri
//     writes r.tmax on acceptance: the kernel puts b back after every test);
//   * the order: the surviving slot of a run with the smallest front is visited next (ties: the lower slot), the others are
//     pushed -- point_query_kernel's nearest-first step with front in the place of boxdist2 -- so the bound falls as fast as
//     the near hits arrive;
//   * the list: a private array of RT_RAY_FIRST_MAX_K 16-byte records in ascending (t, id) order, written to the row once at
//     the end; m, the k-th (t, id) and b live in registers.  A candidate is first tested against the registers alone: not
//     below the k-th of a full list -- most candidates end there.  A survivor finds its position first (a scan down from the
//     top; an equal (t, id) means the record is already listed -- a split tree holds several references -- and the candidate
//     is dropped) and shifts afterwards.  Plain vector loads and stores at lane-private addresses, no atomics;
//   * a NaN t (an overflowed product that Moller-Trumbore's comparisons let through) orders above every number and NaNs are
//     equal to each other; the bound is never NaN: while the k-th t is NaN it stays the original tmax.
// Pending entries, RT_RAY_FIRST_PENDING (rows on decided rays -- rt_abi.h, claim 2 -- are identical in both arms):
//   4  the entry alone, 16 in an LDS column per lane (16 KB per workgroup: ray_hits_kernel's LDS bound of eight waves per
//      SIMD, of which the list's registers leave six) + 48 private; a pop is not re-culled: the slots of a popped run, and the
//      triangles of a popped leaf, meet the current b anyway;
//   8  (entry, front) in 8 bytes, 16 in an LDS column (32 KB per workgroup: five waves per SIMD) + 48 private; a popped entry
//      is dropped iff front > b with the current b.
// Shipped: 4, by measurement (tools/ray_first_bench.py, profiles/ray_first_bench.json): the re-test saves
// at most 1.5 % of the box tests and the wider entries cost up to 45 % more time.  The other arm is a library build:
// csrc/Makefile's librt_amd_exp.so with EXPFLAGS=-DRT_RAY_FIRST_PENDING=8.
// A push onto a full stack of 64 is dropped and flagged (RT_RAY_FIRST_STACK_OVERFLOW): the row is then a sorted subset of the
// all-hit row.  No restart pass.
// Compiled with -ffp-contract=off and IEEE division: every listed record is bit for bit the one rt_ray_hits_collect emits for
// that triangle.
// The kernel's body is rt_ray_first_body.inc, shared as text with the filtered kernels of ray_filter_query.hip.
#include "rt_launch.hpp"
#include "rt_ray_first.hpp"

namespace rt {

namespace {

__global__ __launch_bounds__(kTraceWaves * 64, kRfMinWaves) void ray_first_kernel(RayFirstParams p)
{
#define RT_BODY_FILTER NoFilter
#define RT_BODY_MAKE_FILTER(i, in_range) NoFilter()
#include "rt_ray_first_body.inc"
#undef RT_BODY_FILTER
#undef RT_BODY_MAKE_FILTER
}

}  // namespace

hipError_t launch_ray_first_hits(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, uint32_t k, rt_hit* out,
                                 uint64_t* counters, uint32_t* status, hipStream_t st)
{
    RayFirstParams p;
    p.nodes = as.nodes;
    p.leaves = as.triangles;
    p.root = as.root;
    p.count = as.count;
    p.rays = reinterpret_cast<const float4*>(rays);
    p.out = reinterpret_cast<float4*>(out);
    p.num_rays = num_rays;
    p.k = k;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    const uint32_t per_block = kTraceWaves * 64;
    const dim3 grid((uint32_t)(((uint64_t)num_rays + per_block - 1) / per_block)), block(per_block);
    ray_first_kernel<<<grid, block, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace rt
