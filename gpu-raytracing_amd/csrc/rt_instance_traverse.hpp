// rt_instance_traverse.hpp -- the two-level traversal of the closest / any-hit instanced ray queries: instances.hip
// (rt_intersect_rays_instanced and rt_intersect_rays_instanced_filtered, the two arms of one kernel) and
// instance_motion_query.hip.  Here: the kernel parameters, the TLAS-aware box step, and trace_instanced, the wave-level
// two-phase loop with a second level (what the second level adds to a lane: instances.hip's header; DESIGN sections 9 and 21).
//
// What is shared, each defined once: the Trav initialisation and the vote / park box phase; the triangle-pair leaf test with
// its was_first / second-slot / advance tail; the exit to the TLAS (load_world_ray, for any params struct with `rays`); the
// skeleton of entering an instance -- the id bound, load_instance (the record's rows and tail, the usability rule, load_accel,
// the root-run rule), to_object_ray, the commit of the lane's BLAS.  What differs travels as two policies, by value, the way
// trace_ray takes its hit-filter policy: the instance filter (rt_instance_filter.hpp) and the TLAS (StaticTlas here, MovingTlas
// in rt_instance_motion_traverse.hpp).  With the defaults the code is instance_query_kernel's, instruction for instruction;
// how each policy is spelled is what keeps it so, and the motion kernels too ("Policies and helpers").
// Three traversals keep loops of their own and use the small helpers from here: rt_instance_mixed_traverse.hpp (a policy for
// its leaf primitives left its kernels neither identical nor within the measured bar: DESIGN section 25), and
// ray_hits_instanced_query.hip and ray_first_instanced_query.hip (an unordered and a nearest-first traversal).
// Device code only; every function is force-inlined into its kernel.
#pragma once

#include "rt_device.hpp"
#include "rt_traverse.hpp"

// waves per SIMD the query kernels' register allocation (filtered or not) must fit (see DESIGN section 9 for the measured choice)
#ifndef RT_INSTANCE_QUERY_WAVES
#define RT_INSTANCE_QUERY_WAVES 4
#endif

namespace rt {

namespace {   // (as in the kernels' own file)

constexpr uint32_t kTop = 0xFFFFFFFFu;              // "in the TLAS" (the lane's current instance)
enum : uint32_t { PH_ENTER = 4, PH_EXIT = 5 };      // parked phases of the second level (PH_STEP .. PH_DONE: rt_traverse.hpp)

struct InstParams {
    const rt_node* tlas_nodes;
    const rt_triangle_pair* tlas_leaves;
    uint32_t root, count;
    const rt_instance_record* records;
    uint32_t num_instances, num_blas;
    const rt_accel* blas_table;
    const float4* rays;
    float4* hits;
    uint32_t* instance_ids;
    uint32_t num_rays;
    unsigned long long* counters;
    static constexpr int park_num = kParkNum, park_den = kParkDen;
};

struct LaneNodes { const rt_node* nodes; };   // prefetch_pair's Params: the lane's own node array

// trace_ray's advance() with the stack bottom at `base` (the depth at which the lane entered its BLAS; 0 in the TLAS).  An
// empty BLAS parks the lane in PH_EXIT; in the TLAS an entry of count 0 (a TLAS leaf) parks it in PH_ENTER.
__device__ __forceinline__ void inst_advance(Trav& t, int base, bool top)
{
    const uint32_t cnt = t.cur >> 29;
    if (cnt > 2) { t.cur = ((t.cur & kIndexMask) + 2) | ((cnt - 2) << 29); return; }
    const bool keep = (t.near_e != kNoNear) & (t.sp < kStackMax);
    if (keep) t.cur = t.near_e;
    else if (t.sp == base) t.phase = top ? PH_DONE : PH_EXIT;
    else { --t.sp; t.cur = t.sp < kStackLds ? t.lds[t.sp * 64] : t.spill[t.sp - kStackLds]; }
    t.near_e = kNoNear;
    t.near_d = __builtin_inff();
    if (top & (t.phase == PH_STEP) & ((t.cur >> 29) == 0u)) t.phase = PH_ENTER;
}

// Trav::second_slot, with a TLAS leaf taken as an entry of count 0 instead of parking the lane
__device__ __forceinline__ void inst_second_slot(Trav& t, float tmin, float tmax, bool top)
{
    const bool valid = t.t1 != RT_CHILD_NONE;
    const bool hit = valid & (t.k1 >= t.f1) & (t.f1 <= tmax) & (t.k1 >= tmin);
    t.box_tests += valid ? 1u : 0u;
    const bool tri = t.t1 == RT_CHILD_TRI;
    const bool is_leaf = hit & tri & !top;
    t.inner_hit(hit & !is_leaf, (tri & top) ? (t.e1 & kIndexMask) : t.e1, t.f1);
    if (is_leaf) { t.leaf = t.e1; t.phase = PH_LEAF1; }
}

// box_step_on of rt_traverse.hpp on a fetched pair of the lane's own node array, TLAS leaves as entries
template <bool PF>
__device__ __forceinline__ void inst_box_step_on(const LaneNodes& ln, const Ray& r, Trav& t, int base, bool top, bool two,
                                                 const uint4& a0, const uint4& b0, const uint4& a1, const uint4& b1)
{
    float f0, k0;
    slab(a0, b0, r, f0, k0);
    slab(a1, b1, r, t.f1, t.k1);
    t.e1 = (b1.w & kIndexMask) | (a1.w & ~kIndexMask);
    t.t1 = two ? (b1.w >> 29) : (uint32_t)RT_CHILD_NONE;
    const uint32_t type0 = b0.w >> 29;
    const uint32_t e0 = (b0.w & kIndexMask) | (a0.w & ~kIndexMask);
    const bool valid0 = type0 != RT_CHILD_NONE;
    const bool hit0 = valid0 & (k0 >= f0) & (f0 <= r.tmax) & (k0 >= r.tmin);
    t.box_tests += valid0 ? 1u : 0u;
    const bool tri0 = type0 == RT_CHILD_TRI;
    const bool leaf0 = hit0 & tri0 & !top;
    t.inner_hit(hit0 & !leaf0, (tri0 & top) ? (e0 & kIndexMask) : e0, f0);
    if (leaf0) { t.leaf = e0; t.phase = PH_LEAF0; }
    else {
        inst_second_slot(t, r.tmin, r.tmax, top);
        if (t.phase == PH_STEP) { inst_advance(t, base, top); prefetch_pair<PF>(ln, t); }
    }
}

// the fetch of the pair (from the prefetch registers under PF) and the step on it
template <bool PF>
__device__ __forceinline__ void inst_box_step(const LaneNodes& ln, const Ray& r, Trav& t, int base, bool top)
{
    const uint32_t cnt = t.cur >> 29;
    const uint4* np = reinterpret_cast<const uint4*>(ln.nodes + (t.cur & kIndexMask));
    const bool two = cnt > 1;
    const int o1 = two ? 2 : 0;
    uint4 a0, b0, a1, b1;
    if constexpr (PF) { a0 = t.pf0; b0 = t.pf1; a1 = t.pf2; b1 = t.pf3; }
    else { a0 = np[0]; b0 = np[1]; a1 = np[o1]; b1 = np[o1 + 1]; }
    inst_box_step_on<PF>(ln, r, t, base, top, two, a0, b0, a1, b1);
}

// the world ray of ray i (origin, direction and its reciprocal; tmin / tmax are not the transform's and stay), for any
// params struct that has `rays`
template <class P>
__device__ __forceinline__ void load_world_ray(const P& p, uint64_t i, Ray& r)
{
    const float4 a = p.rays[2 * i], b = p.rays[2 * i + 1];
    r.ox = a.x; r.oy = a.y; r.oz = a.z;
    r.dx = b.x; r.dy = b.y; r.dz = b.z;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
}

// world ray r to the object ray of an instance: w0, w1, w2 are the rows of the record's world_to_object
__device__ __forceinline__ void to_object_ray(const float4& w0, const float4& w1, const float4& w2, Ray& r)
{
    const float ox = r.ox, oy = r.oy, oz = r.oz, dx = r.dx, dy = r.dy, dz = r.dz;
    r.ox = ((w0.x * ox + w0.y * oy) + w0.z * oz) + w0.w;
    r.oy = ((w1.x * ox + w1.y * oy) + w1.z * oz) + w1.w;
    r.oz = ((w2.x * ox + w2.y * oy) + w2.z * oz) + w2.w;
    r.dx = (w0.x * dx + w0.y * dy) + w0.z * dz;
    r.dy = (w1.x * dx + w1.y * dy) + w1.z * dz;
    r.dz = (w2.x * dx + w2.y * dy) + w2.z * dz;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
}

// a BLAS as its rt_accel tells it: the root run, the leaf and node arrays
struct BlasRef {
    uint32_t root, count;
    uint64_t tris, nodes;
};

// rt_accel of table entry b: three 8-byte loads (the entries are 24 bytes apart)
__device__ __forceinline__ void load_accel(const rt_accel* table, uint32_t b, uint64_t& tris, uint64_t& nodes, uint32_t& root,
                                           uint32_t& count)
{
    const uint2* q = reinterpret_cast<const uint2*>(table + b);
    const uint2 x = q[0], y = q[1], z = q[2];
    tris = ((uint64_t)x.y << 32) | x.x;
    nodes = ((uint64_t)y.y << 32) | y.x;
    root = z.x;
    count = z.y;
}

// The two policies of trace_instanced.  Both travel by value, as NoFilter does, and every difference is taken under
// `if constexpr` or inside a policy's force-inlined members: the defaults leave no trace in instance_query_kernel.
//
// The instance filter.  NoInstanceFilter: every usable instance is entered and every triangle Moller-Trumbore accepts is
// accepted.  A policy with active = true (rt_instance_filter.hpp) supplies enter(id), asked at the TLAS leaf before the
// instance record is read, set_instance(id, w0, w1, w2), called once the instance is entered, and `tri`, the intersect_tri
// policy of the entered instance.
struct NoInstanceFilter {
    static constexpr bool active = false;
};

// The record of instance `id` -- its rows w..., as many as are handed in, then (blas, flags, spare) -- and its BLAS's table
// entry.  False: the instance is unusable -- flags set, a BLAS index past the table, a root run of 0 or more than 7 slots.
template <class P, class... Rows>
__device__ __forceinline__ bool load_instance(const P& p, uint32_t id, BlasRef& b, Rows&... w)
{
    const float4* rec = reinterpret_cast<const float4*>(p.records + id);
    int k = 0;
    ((w = rec[k++]), ...);
    const uint4 tail = reinterpret_cast<const uint4*>(rec)[sizeof...(Rows)];   // blas, flags, spare
    bool ok = (tail.y == 0u) & (tail.x < p.num_blas);
    if (ok) {
        load_accel(p.blas_table, tail.x, b.tris, b.nodes, b.root, b.count);
        ok = (b.count - 1u) < 7u;
    }
    return ok;
}

// The TLAS.  StaticTlas: one pose (p.tlas_nodes / p.tlas_leaves) and rt_instance_record, three rows of world_to_object, which
// trace_instanced loads and applies itself (the filter is shown them).  A policy names the TLAS arrays of its params struct and
// takes the box step of both levels; one with moving = true (MovingTlas, rt_instance_motion_traverse.hpp) also supplies
// enter(...): load_instance with its own record's rows and the world ray r made the object ray, or false, r untouched.
struct StaticTlas {
    static constexpr bool moving = false;
    template <class P> __device__ __forceinline__ static const rt_node* nodes(const P& p) { return p.tlas_nodes; }
    template <class P> __device__ __forceinline__ static const rt_triangle_pair* leaves(const P& p) { return p.tlas_leaves; }
    template <bool PF, class P>
    __device__ __forceinline__ static void box_step(const P&, const LaneNodes& ln, const Ray& r, Trav& t, int base, bool top)
    {
        inst_box_step<PF>(ln, r, t, base, top);
    }
};

// The two-level traversal of ray `ri` (r: its world ray, loaded by the caller).  Returns tri_hit; *hit_inst = the instance of
// h; steps[0] / steps[1] as trace_ray.
template <bool PF, bool ANY, class IFilter = NoInstanceFilter, class Tlas = StaticTlas, class P>
__device__ __forceinline__ bool trace_instanced(const P& p, uint64_t ri, Ray& r, Hit& h, uint32_t& hit_inst, Trav& t,
                                                bool active, uint32_t* steps, IFilter flt = IFilter(), Tlas tlas = Tlas())
{
    LaneNodes ln = {tlas.nodes(p)};
    const rt_triangle_pair* leaves = tlas.leaves(p);
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
    prefetch_pair<PF>(ln, t);
    bool tri_hit = false;
    uint32_t nbox = 0, nleaf = 0;
    // the entered instance's intersect_tri policy, or none
    auto tri_flt = [&] { if constexpr (IFilter::active) return flt.tri; else return NoFilter(); };

    while (true) {
        // ---------------------------------------------------- box phase (both levels)
        uint64_t stepping, parked;
        while (true) {
            stepping = __builtin_amdgcn_ballot_w64(t.phase == PH_STEP);
            parked = __builtin_amdgcn_ballot_w64((t.phase != PH_STEP) & (t.phase != PH_DONE));
            if (stepping == 0 || __popcll(stepping) * p.park_den < __popcll(parked) * p.park_num) break;
            nbox += 2;
            if (t.phase == PH_STEP) tlas.template box_step<PF>(p, ln, r, t, base, inst == kTop);
            if (t.phase == PH_STEP) tlas.template box_step<PF>(p, ln, r, t, base, inst == kTop);
        }
        if ((stepping | parked) == 0) break;
        // ---------------------------------------------------- leaf phase: triangle tests, leaving and entering instances
        nleaf++;
        if ((t.phase != PH_STEP) & (t.phase != PH_DONE)) {
            if ((t.phase - 1u) < 2u) {   // PH_LEAF0 / PH_LEAF1: a BLAS leaf, as trace_ray
                // triangle A = (v0, v1, v2) and, unless v3 == v2 bit for bit (a single triangle), B = (v2, v1, v3)
                t.tri_tests++;
                const uint32_t li = t.leaf & kIndexMask;
                const uint4* tp = reinterpret_cast<const uint4*>(leaves + li);
                const uint4 l0 = tp[0], l1 = tp[1], l2 = tp[2], l3 = tp[3];
                bool hit_tri = intersect_tri(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
                                             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                             __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                             r, h, li << 1, l0.w, tri_flt());
                if ((t.leaf >> 29) > 0 && (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z))
                    hit_tri |= intersect_tri(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                                             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                                             __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z),
                                             r, h, (li << 1) + 1, l1.w, tri_flt());
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
                ln.nodes = tlas.nodes(p);
                inst = kTop;
                base = 0;
                t.phase = PH_STEP;
                inst_advance(t, 0, true);
            }
            if (t.phase == PH_ENTER) {   // a TLAS leaf: enter its instance, or go on in the TLAS
                const uint32_t id = reinterpret_cast<const uint4*>(tlas.leaves(p) + (t.cur & kIndexMask))[0].w;
                bool ok = id < p.num_instances;
                if constexpr (IFilter::active) {
                    if (ok) ok = flt.enter(id);   // the instance rule: asked first, a masked-out instance makes no further load
                }
                BlasRef b = {0u, 0u, 0ull, 0ull};
                if constexpr (Tlas::moving) {
                    if (ok) ok = tlas.enter(p, id, r, b);
                } else {
                    float4 w0, w1, w2;
                    if (ok) ok = load_instance(p, id, b, w0, w1, w2);
                    if (ok) {
                        if constexpr (IFilter::active) flt.set_instance(id, w0, w1, w2);
                        to_object_ray(w0, w1, w2, r);
                    }
                }
                if (ok) {
                    ln.nodes = reinterpret_cast<const rt_node*>(b.nodes);
                    leaves = reinterpret_cast<const rt_triangle_pair*>(b.tris);
                    inst = id;
                    base = t.sp;
                    t.cur = (b.root & kIndexMask) | (b.count << 29);
                    t.phase = PH_STEP;
                } else {
                    t.phase = PH_STEP;
                    inst_advance(t, 0, true);
                }
            }
            prefetch_pair<PF>(ln, t);
        }
    }
    steps[0] += nbox;
    steps[1] += nleaf;
    return tri_hit;
}

}  // namespace

}  // namespace rt
