// instances.hip -- rt_prepare_instances and rt_intersect_rays_instanced: ray queries over placed copies of built trees
// (semantics: rt_abi.h, instancing block).
//
// prepare_instances_kernel, one thread per instance: the world box of the BLAS's root run through object_to_world, the
// padded box as a proxy triangle (the TLAS build input), world_to_object in double.
//
// instance_query_kernel<PF, ANY>: rt_traverse.hpp's wave-level two-phase loop with a second level.  One lane per ray, the
// launch geometry, LDS stack, XCD remap and counters of ray_query_kernel.  What the second level adds to a lane:
//   * per-lane node / leaf base pointers: the lanes of one wave sit in different BLASes (and in the TLAS);
//   * TLAS leaves are ordered with the box children: a leaf hit in the TLAS becomes an entry of count 0 (child : 29 | 0,
//     never a box run, whose count is 1..7) that takes part in the nearest-child choice or is pushed like a box child, so
//     the second slot of a TLAS pair is always evaluated in world space before any instance is entered, and nothing of the
//     TLAS is pending while a BLAS is traversed except its stack;
//   * when advance() picks such an entry the lane parks in PH_ENTER; the leaf phase loads the TLAS leaf's instance index,
//     the instance record and the BLAS's rt_accel, transforms the ray, switches the base pointers and remembers the stack
//     depth (base).  BLAS traversal is trace_ray's, with its stack starting at base;
//   * a BLAS whose advance() finds no near child and the stack back at base parks in PH_EXIT; the leaf phase reloads the
//     world ray from the ray array (the original bits), switches back to the TLAS and advances there -- which may enter the
//     next instance in the same leaf phase.
// tmax is shared by both spaces (an affine map preserves t): one closest hit across all instances.
// Compiled with -ffp-contract=off: every float operation is the documented one.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_instance) == 64 && offsetof(rt_instance, blas) == 48, "rt_instance: 3x4 matrix, blas, 3 pads");
static_assert(sizeof(rt_instance_record) == 64 && offsetof(rt_instance_record, blas) == 48 &&
              offsetof(rt_instance_record, flags) == 52, "rt_instance_record: 3x4 matrix, blas, flags, 2 spare");
static_assert(sizeof(rt_accel) == 24, "rt_accel: two pointers, root, count");

// waves per SIMD the query kernel's register allocation must fit (see DESIGN section 9 for the measured choice)
#ifndef RT_INSTANCE_QUERY_WAVES
#define RT_INSTANCE_QUERY_WAVES 4
#endif

namespace rt {

namespace {

constexpr float kInstancePad = 1.0f / 4096.0f;      // 2^-12 of the box's largest |bound| (rt_abi.h)
constexpr uint32_t kTop = 0xFFFFFFFFu;              // "in the TLAS" (the lane's current instance)
enum : uint32_t { PH_ENTER = 4, PH_EXIT = 5 };      // parked phases of the second level (PH_STEP .. PH_DONE: rt_traverse.hpp)

// ---------------------------------------------------------------- prepare
__global__ __launch_bounds__(256) void prepare_instances_kernel(const rt_instance* instances, uint32_t num_instances,
                                                                const rt_accel* blas_table, uint32_t num_blas,
                                                                rt_triangle* proxies, rt_instance_record* records,
                                                                uint32_t* status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= num_instances) return;
    const rt_instance in = instances[i];
    const float* m = in.object_to_world;
    uint32_t flags = 0;

    // the object box: ordered min / max over the non-NONE slots of the root run
    int lo_i[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi_i[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    bool any = false;
    if (in.blas >= num_blas) flags |= RT_INSTANCE_BAD_BLAS;
    else {
        const rt_accel a = blas_table[in.blas];
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

    // world_to_object in double: adjugate / det of the 3x3 part, translation -W3 * t
    bool finite = true;
    for (int k = 0; k < 12; k++) finite &= __builtin_isfinite(m[k]);
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    float w[12];
    if (!finite || det == 0.0) flags |= RT_INSTANCE_SINGULAR;
    else {
        const double r = 1.0 / det;
        const double inv[9] = {c00 * r, (a02 * a21 - a01 * a22) * r, (a01 * a12 - a02 * a11) * r,
                               c01 * r, (a00 * a22 - a02 * a20) * r, (a02 * a10 - a00 * a12) * r,
                               c02 * r, (a01 * a20 - a00 * a21) * r, (a00 * a11 - a01 * a10) * r};
        const double t0 = m[3], t1 = m[7], t2 = m[11];
        bool fits = true;
        for (int k = 0; k < 3; k++) {
            const double* row = inv + 3 * k;
            const double tr = -(row[0] * t0 + row[1] * t1 + row[2] * t2);
            w[4 * k + 0] = (float)row[0]; w[4 * k + 1] = (float)row[1]; w[4 * k + 2] = (float)row[2]; w[4 * k + 3] = (float)tr;
        }
        for (int k = 0; k < 12; k++) fits &= __builtin_isfinite(w[k]);
        if (!fits) flags |= RT_INSTANCE_SINGULAR;
    }

    rt_instance_record rec;
    for (int k = 0; k < 12; k++) rec.world_to_object[k] = flags ? 0.0f : w[k];
    rec.blas = in.blas;
    rec.flags = flags;
    rec.spare[0] = rec.spare[1] = 0;
    records[i] = rec;

    rt_triangle px = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};   // flagged: a point proxy at the origin
    if (!flags) {
        // corners through object_to_world; their ordered min / max (-0 below +0: no dependence on fminf's zero rule)
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
        px.v0 = {lo[0], lo[1], lo[2]};
        px.v1 = {hi[0], hi[1], hi[2]};
        px.v2 = {lo[0] * 0.5f + hi[0] * 0.5f, lo[1] * 0.5f + hi[1] * 0.5f, lo[2] * 0.5f + hi[2] * 0.5f};
    }
    proxies[i] = px;
    if (flags) atomicOr(status, flags);
}

// ---------------------------------------------------------------- query
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

// box_step of rt_traverse.hpp on the lane's own node array, TLAS leaves as entries
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

__device__ __forceinline__ void load_world_ray(const InstParams& p, uint64_t i, Ray& r)
{
    const float4 a = p.rays[2 * i], b = p.rays[2 * i + 1];
    r.ox = a.x; r.oy = a.y; r.oz = a.z;
    r.dx = b.x; r.dy = b.y; r.dz = b.z;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
}

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

// The two-level traversal of ray `ri` (r: its world ray, loaded by the caller).  Returns tri_hit; *hit_inst = the instance of h.
template <bool PF, bool ANY>
__device__ __forceinline__ bool trace_instanced(const InstParams& p, uint64_t ri, Ray& r, Hit& h, uint32_t& hit_inst, Trav& t,
                                                bool active, uint32_t* steps)
{
    LaneNodes ln = {p.tlas_nodes};
    const rt_triangle_pair* leaves = p.tlas_leaves;
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

    while (true) {
        // ---------------------------------------------------- box phase (both levels)
        uint64_t stepping, parked;
        while (true) {
            stepping = __builtin_amdgcn_ballot_w64(t.phase == PH_STEP);
            parked = __builtin_amdgcn_ballot_w64((t.phase != PH_STEP) & (t.phase != PH_DONE));
            if (stepping == 0 || __popcll(stepping) * p.park_den < __popcll(parked) * p.park_num) break;
            nbox += 2;
            if (t.phase == PH_STEP) inst_box_step<PF>(ln, r, t, base, inst == kTop);
            if (t.phase == PH_STEP) inst_box_step<PF>(ln, r, t, base, inst == kTop);
        }
        if ((stepping | parked) == 0) break;
        // ---------------------------------------------------- leaf phase: triangle tests, leaving and entering instances
        nleaf++;
        if ((t.phase != PH_STEP) & (t.phase != PH_DONE)) {
            if ((t.phase - 1u) < 2u) {   // PH_LEAF0 / PH_LEAF1: a BLAS leaf, as trace_ray
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
                ln.nodes = p.tlas_nodes;
                inst = kTop;
                base = 0;
                t.phase = PH_STEP;
                inst_advance(t, 0, true);
            }
            if (t.phase == PH_ENTER) {   // a TLAS leaf: enter its instance, or go on in the TLAS
                const uint32_t id = reinterpret_cast<const uint4*>(p.tlas_leaves + (t.cur & kIndexMask))[0].w;
                bool ok = id < p.num_instances;
                uint32_t nroot = 0, ncount = 0;
                uint64_t ntris = 0, nnodes = 0;
                float4 w0, w1, w2;
                if (ok) {
                    const float4* rec = reinterpret_cast<const float4*>(p.records + id);
                    w0 = rec[0]; w1 = rec[1]; w2 = rec[2];
                    const uint4 tail = reinterpret_cast<const uint4*>(rec)[3];   // blas, flags, spare
                    ok = (tail.y == 0u) & (tail.x < p.num_blas);
                    if (ok) {
                        load_accel(p.blas_table, tail.x, ntris, nnodes, nroot, ncount);
                        ok = (ncount - 1u) < 7u;
                    }
                }
                if (ok) {
                    const float ox = r.ox, oy = r.oy, oz = r.oz, dx = r.dx, dy = r.dy, dz = r.dz;
                    r.ox = ((w0.x * ox + w0.y * oy) + w0.z * oz) + w0.w;
                    r.oy = ((w1.x * ox + w1.y * oy) + w1.z * oz) + w1.w;
                    r.oz = ((w2.x * ox + w2.y * oy) + w2.z * oz) + w2.w;
                    r.dx = (w0.x * dx + w0.y * dy) + w0.z * dz;
                    r.dy = (w1.x * dx + w1.y * dy) + w1.z * dz;
                    r.dz = (w2.x * dx + w2.y * dy) + w2.z * dz;
                    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
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
            prefetch_pair<PF>(ln, t);
        }
    }
#ifndef RT_TRACE_NO_STEPS
    steps[0] += nbox;
    steps[1] += nleaf;
#endif
    return tri_hit;
}

template <bool PF, bool ANY>
__global__ __launch_bounds__(kTraceWaves * 64, RT_INSTANCE_QUERY_WAVES)
void instance_query_kernel(InstParams p)
{
    __shared__ uint32_t stack_lds[kTraceWaves][kStackLds][64];
    __shared__ unsigned long long csum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p.counters) {
        if (threadIdx.x < 4) csum[threadIdx.x] = 0ull;
        __syncthreads();
    }
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_rays;

    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    r.tmin = 0.0f;
    r.tmax = -1.0f;
    if (in_range) {
        load_world_ray(p, i, r);
        r.tmin = p.rays[2 * i].w;
        r.tmax = p.rays[2 * i + 1].w;
    }
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray;

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    Hit h = {0u, 0u, 0.f, 0.f};
    uint32_t hit_inst = RT_MISS;
    const bool hit = trace_instanced<PF, ANY>(p, i, r, h, hit_inst, t, active, steps);

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            // the hit instance's BLAS leaves; (u, v) back to the caller's corners as ray_query_kernel does
            const uint32_t b = reinterpret_cast<const uint4*>(p.records + hit_inst)[3].x;
            const rt_triangle_pair* lv = reinterpret_cast<const rt_triangle_pair*>(
                *reinterpret_cast<const uint64_t*>(p.blas_table + b));
            const uint32_t rot = lv[h.tri_id >> 1].rotations[h.tri_id & 1];
            const float w0 = 1 - h.bu - h.bv;
            o.x = r.tmax;
            o.y = __uint_as_float(h.primitive_id);
            o.z = rot == 1 ? h.bv : (rot == 2 ? w0 : h.bu);
            o.w = rot == 1 ? w0 : (rot == 2 ? h.bu : h.bv);
        }
        p.hits[i] = o;
        p.instance_ids[i] = hit ? hit_inst : RT_MISS;
    }
    if (p.counters) {
        const uint32_t bsum = wave_sum_u32(t.box_tests), tsum = wave_sum_u32(t.tri_tests);
        if (lane == 0) {
            atomicAdd(&csum[0], (unsigned long long)bsum);
            atomicAdd(&csum[1], (unsigned long long)tsum);
            atomicAdd(&csum[2], (unsigned long long)steps[0]);
            atomicAdd(&csum[3], (unsigned long long)steps[1]);
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const unsigned long long v = csum[threadIdx.x];
            if (v) atomicAdd(&p.counters[threadIdx.x], v);
        }
    }
}

}  // namespace

hipError_t launch_prepare_instances(const rt_instance* instances, uint32_t num_instances, const rt_accel* blas_table,
                                    uint32_t num_blas, rt_triangle* proxies, rt_instance_record* records, uint32_t* status,
                                    hipStream_t st)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || num_instances == 0) return e;
    prepare_instances_kernel<<<dim3((num_instances + 255) / 256), dim3(256), 0, st>>>(instances, num_instances, blas_table,
                                                                                      num_blas, proxies, records, status);
    return hipGetLastError();
}

hipError_t launch_instance_query(const InstanceQuery& q, hipStream_t st)
{
    InstParams p;
    p.tlas_nodes = q.tlas.nodes;
    p.tlas_leaves = q.tlas.triangles;
    p.root = q.tlas.root;
    p.count = q.tlas.count;
    p.records = q.records;
    p.num_instances = q.num_instances;
    p.num_blas = q.num_blas;
    p.blas_table = q.blas_table;
    p.rays = reinterpret_cast<const float4*>(q.rays);
    p.hits = reinterpret_cast<float4*>(q.hits);
    p.instance_ids = q.instance_ids;
    p.num_rays = q.num_rays;
    p.counters = reinterpret_cast<unsigned long long*>(q.counters);
    const uint32_t rays_per_block = kTraceWaves * 64;
    const dim3 grid((uint32_t)(((uint64_t)q.num_rays + rays_per_block - 1) / rays_per_block)), block(rays_per_block);
    const bool pf = q.num_primitives >= kPrefetchMinPrims;
    if (pf) {
        if (q.any_hit) instance_query_kernel<true, true><<<grid, block, 0, st>>>(p);
        else instance_query_kernel<true, false><<<grid, block, 0, st>>>(p);
    } else {
        if (q.any_hit) instance_query_kernel<false, true><<<grid, block, 0, st>>>(p);
        else instance_query_kernel<false, false><<<grid, block, 0, st>>>(p);
    }
    return hipGetLastError();
}

}  // namespace rt
