// refit.hip -- rt_build_refit_plan / rt_refit: keep a built tree's topology and leaf assignment, recompute its geometry from
// moved vertices (no reference counterpart; the reference's bottom-up box pass exists only inside its LBVH build,
// BottomUpBuilder.cu:217-285).
//
// Plan (once per build).  Parent pointers exist in LBVH slots only (SAH and hybrid-top slots carry parent 0), so the plan
// walks the tree top-down from (root, count), level-synchronously over a frontier of runs (first slot : 29 | length : 3)
// whose bounds stay on the device:
//   refit_plan_init_kernel    zero the per-slot words, claim the root run, frontier = {root run}, fingerprint
//   refit_walk_kernel x K     one wide launch per level (K = ceil(log2 n) + 2); the last workgroup to finish (ticket)
//                             moves the frontier bounds on
//   refit_walk_kernel x 1     one workgroup, a device-side loop over whatever levels remain (deep trees: fractal)
//   refit_leaves_kernel       the reached leaf slots, compacted in slot order, their records checked
// A child run is claimed with one CAS on the word of its first slot (parent slot : 29 | expected arrivals : 3, expected
// arrivals = its non-NONE slots); the other slots of the run get their offset in the run (a CAS too, so that overlapping runs
// are caught).  A CAS that finds the word taken means the walk reached a slot twice: RT_REFIT_BAD_TREE.
//
// Refit (every frame, one launch).  One thread per leaf slot rewrites the record from the caller's triangles, stores the
// slot's box and climbs: at each run it takes a ticket (agent-scope fetch_add on the run's arrival byte); the last arrival
// reads the run's slot boxes, writes the parent slot's box and goes on; every other arrival exits.  Nobody waits.  The last
// arrival also takes its arrivals back off the byte, so the counters are zero again when the launch ends.
// Hand-off (cdna_hip_programming.md section 6, Guideline 16): the boxes cross XCDs, whose L2s are not coherent, so the
// producer stores them write-through (sc1: relaxed agent-scope atomic stores), drains them (s_waitcnt vmcnt(0)) before its
// ticket, and the climbing thread reads them with sc1 loads (relaxed agent-scope atomic loads) -- the protocol of the LBVH
// builder's hand-off stores (lbvh_levels.hip, store_sc1).
// Boxes are ordered min / max (the integer image of the floats, -0 below +0): associative and commutative bit for bit, so
// the result does not depend on which thread arrives last.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_pairing.hpp"

namespace rt {

namespace {

// plan header words (the first 256 bytes of the plan)
enum : uint32_t {
    kHdrStatus = 0,   // RT_REFIT_* flags
    kHdrLeaves = 1,   // number of leaf slots in the list
    kHdrBegin = 2,    // frontier [begin, end) in the list
    kHdrEnd = 3,
    kHdrTail = 4,     // next free list entry (appends of the level being walked)
    kHdrDone = 5,     // workgroups of the current wide launch that have finished
    kHdrNodesLo = 8,  // fingerprint: nodes, root, count, n
    kHdrNodesHi = 9,
    kHdrRoot = 10,
    kHdrCount = 11,
    kHdrN = 12,
};
constexpr uint32_t kRootParent = kIndexMask;   // the parent field of the root run (no slot has this index: slots < 2^29 - 1)
constexpr uint32_t kWalkThreads = 256, kTailThreads = 1024, kRefitThreads = 256;

struct PlanPtrs {
    uint32_t* hdr;
    uint32_t* parents;   // [slots] run-first slot: parent : 29 | expected : 3;  other reached slot: its offset in the run
    uint32_t* arrive;    // [slots] bytes: arrivals (bits 0-2) at a run-first slot; bit 7 = the slot is a reached leaf
    uint32_t* list;      // [slots] runs of the walk, then the leaf slots
    uint32_t slots;
};

PlanPtrs plan_ptrs(void* plan, uint32_t n)
{
    const RefitLayout L = refit_layout(n);
    char* p = static_cast<char*>(plan);
    return PlanPtrs{reinterpret_cast<uint32_t*>(p + L.status), reinterpret_cast<uint32_t*>(p + L.parents),
                    reinterpret_cast<uint32_t*>(p + L.arrive), reinterpret_cast<uint32_t*>(p + L.list), L.slots};
}

__device__ __forceinline__ uint32_t node_w12(const rt_node* nodes, uint32_t s) { return nodes[s].w12; }
__device__ __forceinline__ uint32_t node_w28(const rt_node* nodes, uint32_t s) { return nodes[s].w28; }

__device__ __forceinline__ void flag(uint32_t* hdr, uint32_t f) { atomicOr(hdr + kHdrStatus, f); }

__device__ __forceinline__ float fmin_ord(float a, float b) { return float_to_ordered_int(a) < float_to_ordered_int(b) ? a : b; }
__device__ __forceinline__ float fmax_ord(float a, float b) { return float_to_ordered_int(a) > float_to_ordered_int(b) ? a : b; }

// ------------------------------------------------------------------------------------------------------------ plan
__global__ __launch_bounds__(256) void refit_plan_init_kernel(PlanPtrs p, const rt_node* nodes, uint32_t root, uint32_t count,
                                                              uint32_t n, uint32_t slots)
{
    const bool root_ok = root <= slots && count <= slots - root;
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < slots; i += stride)
        if (!root_ok || i - root >= count) p.parents[i] = 0u;     // (the root run's words are written below)
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < (slots + 3) / 4; i += stride) p.arrive[i] = 0u;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t* h = p.hdr;
    const bool walk = root_ok && count > 0;
    uint32_t exp = 0;
    for (uint32_t i = 0; walk && i < count; i++) {
        exp += (node_w28(nodes, root + i) >> 29) != RT_CHILD_NONE ? 1u : 0u;
        if (i) p.parents[root + i] = i;
    }
    if (walk) {
        p.parents[root] = kRootParent | (exp << 29);
        p.list[0] = root | (count << 29);
    }
    h[kHdrStatus] = root_ok ? 0u : (uint32_t)RT_REFIT_BAD_TREE;
    h[kHdrLeaves] = 0;
    h[kHdrBegin] = 0;
    h[kHdrEnd] = h[kHdrTail] = walk ? 1u : 0u;
    h[kHdrDone] = 0;
    h[kHdrNodesLo] = (uint32_t)reinterpret_cast<uintptr_t>(nodes);
    h[kHdrNodesHi] = (uint32_t)(reinterpret_cast<uintptr_t>(nodes) >> 32);
    h[kHdrRoot] = root;
    h[kHdrCount] = count;
    h[kHdrN] = n;
}

// One run of the frontier (`live` lanes; all 64 lanes of the wave call it: the appends are one atomic per wave and slot).
// Leaf slots get their mark, box slots claim their child run and append it to the list.
__device__ __forceinline__ void walk_run(const PlanPtrs& p, const rt_node* nodes, uint32_t n, uint32_t slots, bool live,
                                         uint32_t run)
{
    const uint32_t f = run & kIndexMask, k = live ? run >> 29 : 0u;
    bool bad = false;
    for (uint32_t i = 0; i < 7; i++) {       // uniform trip count: the ballots below see the whole wave
        bool app = false;
        uint32_t entry = 0;
        if (i < k) {
            const uint32_t s = f + i, w28 = node_w28(nodes, s), type = w28 >> 29;
            if (type == RT_CHILD_TRI) {
                if ((w28 & kIndexMask) >= n) bad = true;
                else atomicOr(p.arrive + (s >> 2), 0x80u << ((s & 3u) * 8u));
            } else if (type == RT_CHILD_BOX) {
                const uint32_t c = w28 & kIndexMask, kc = node_w12(nodes, s) >> 29;
                if (kc == 0 || c + kc > slots) {
                    bad = true;
                } else {
                    uint32_t exp = 0;
                    for (uint32_t j = 0; j < kc; j++) exp += (node_w28(nodes, c + j) >> 29) != RT_CHILD_NONE ? 1u : 0u;
                    bool ok = exp > 0 && atomicCAS(p.parents + c, 0u, s | (exp << 29)) == 0u;
                    for (uint32_t j = 1; ok && j < kc; j++) ok = atomicCAS(p.parents + c + j, 0u, j) == 0u;
                    bad |= !ok;
                    app = ok;
                    entry = c | (kc << 29);
                }
            } else if (type != RT_CHILD_NONE) {
                bad = true;
            }
        }
        const uint64_t m = __ballot(app);
        if (m) {
            const int lead = __ffsll((unsigned long long)m) - 1;
            uint32_t base = 0;
            if (lane_id() == lead) base = atomicAdd(p.hdr + kHdrTail, (uint32_t)__popcll(m));
            base = (uint32_t)__builtin_amdgcn_readlane((int)base, lead);
            if (app) {
                const uint32_t pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (pos < slots) p.list[pos] = entry;
                else bad = true;
            }
        }
    }
    if (bad) flag(p.hdr, RT_REFIT_BAD_TREE);
}

// WIDE: one level, grid-stride over the frontier; the last workgroup to finish moves the frontier bounds on.
// !WIDE (one workgroup of kTailThreads): every remaining level, a device-side loop.
template <bool WIDE>
__global__ __launch_bounds__(WIDE ? kWalkThreads : kTailThreads) void refit_walk_kernel(PlanPtrs p, const rt_node* nodes,
                                                                                       uint32_t n, uint32_t slots)
{
    constexpr uint32_t NT = WIDE ? kWalkThreads : kTailThreads;
    __shared__ uint32_t s_be[2];
    if (threadIdx.x == 0) { s_be[0] = p.hdr[kHdrBegin]; s_be[1] = p.hdr[kHdrEnd]; }
    __syncthreads();
    while (true) {
        const uint32_t b = s_be[0], e = min(s_be[1], slots);   // (appends never pass `slots`: each follows a claim)
        if (!WIDE && b >= e) break;
        for (uint32_t base = b + blockIdx.x * NT; base < e; base += gridDim.x * NT) {
            const uint32_t i = base + threadIdx.x;
            const bool live = i < e;
            walk_run(p, nodes, n, slots, live, live ? p.list[i] : 0u);
        }
        __syncthreads();   // (the appends' tail atomics of this workgroup have all returned)
        if (WIDE) {
            if (threadIdx.x == 0) {
                const uint32_t t = atomicAdd(p.hdr + kHdrDone, 1u);
                if (t == gridDim.x - 1) {
                    const uint32_t tail = __hip_atomic_load(p.hdr + kHdrTail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    p.hdr[kHdrBegin] = e;
                    p.hdr[kHdrEnd] = tail;
                    p.hdr[kHdrDone] = 0;
                }
            }
            return;
        }
        if (threadIdx.x == 0) {
            s_be[0] = e;
            s_be[1] = __hip_atomic_load(p.hdr + kHdrTail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) p.hdr[kHdrBegin] = p.hdr[kHdrEnd] = s_be[1];
}

// The marked leaf slots, compacted into the list: four slots (one arrival word) per thread, in slot order inside a workgroup
// (coalesced record and triangle traffic in the refit); one atomic per workgroup for its place.  Each record is checked:
// a single (id1 = 0) or a pair (id1 = id0 + 1), ids < n.
__global__ __launch_bounds__(256) void refit_leaves_kernel(PlanPtrs p, const rt_node* nodes, const rt_triangle_pair* leaves,
                                                           uint32_t n, uint32_t slots)
{
    __shared__ uint32_t ws[256 / 64 + 2];
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    const uint32_t bits = w < (slots + 3) / 4 ? p.arrive[w] & 0x80808080u : 0u;
    uint32_t total;
    const uint32_t excl = block_excl_scan_u32<256>((uint32_t)__popc(bits), ws, &total);
    if (threadIdx.x == 0) ws[0] = total ? atomicAdd(p.hdr + kHdrLeaves, total) : 0u;
    __syncthreads();
    uint32_t pos = ws[0] + excl;
    bool bad = false;
    for (uint32_t j = 0; j < 4; j++) {
        if (!((bits >> (8 * j + 7)) & 1u)) continue;
        const uint32_t s = w * 4 + j;
        if (pos < slots) p.list[pos] = s;
        pos++;
        const uint32_t rec = node_w28(nodes, s) & kIndexMask;
        const uint32_t id0 = leaves[rec].primitive_id_0, id1 = leaves[rec].primitive_id_1;
        bad |= id0 >= n || (id1 != 0u && (id1 != id0 + 1u || id1 >= n));
    }
    if (bad) flag(p.hdr, RT_REFIT_BAD_TREE);
}

// ------------------------------------------------------------------------------------------------------------ refit
// box stores / loads of the hand-off (sc1: relaxed agent-scope atomics); the w12 / w28 words are neither read nor written
__device__ __forceinline__ void store_box_sc1(rt_node* node, const float* lo, const float* hi)
{
    unsigned long long* q = reinterpret_cast<unsigned long long*>(node);
    uint32_t* w = reinterpret_cast<uint32_t*>(node);
    __hip_atomic_store(q, (unsigned long long)__float_as_uint(lo[0]) | ((unsigned long long)__float_as_uint(lo[1]) << 32),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 2, __float_as_uint(lo[2]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 2, (unsigned long long)__float_as_uint(hi[0]) | ((unsigned long long)__float_as_uint(hi[1]) << 32),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 6, __float_as_uint(hi[2]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void load_box_sc1(const rt_node* node, float* lo, float* hi)
{
    unsigned long long* q = reinterpret_cast<unsigned long long*>(const_cast<rt_node*>(node));
    uint32_t* w = reinterpret_cast<uint32_t*>(const_cast<rt_node*>(node));
    const unsigned long long a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t az = __hip_atomic_load(w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b = __hip_atomic_load(q + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t bz = __hip_atomic_load(w + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lo[0] = __uint_as_float((uint32_t)a); lo[1] = __uint_as_float((uint32_t)(a >> 32)); lo[2] = __uint_as_float(az);
    hi[0] = __uint_as_float((uint32_t)b); hi[1] = __uint_as_float((uint32_t)(b >> 32)); hi[2] = __uint_as_float(bz);
}

struct RefitArgs {
    PlanPtrs p;
    const float* tris;
    rt_triangle_pair* leaves;
    rt_node* nodes;
    uint32_t root, count, n;
};

__global__ __launch_bounds__(kRefitThreads) void refit_kernel(RefitArgs a)
{
    const uint32_t* h = a.p.hdr;
    if (h[kHdrStatus] & RT_REFIT_BAD_TREE) return;
    const uintptr_t np = reinterpret_cast<uintptr_t>(a.nodes);
    if (h[kHdrNodesLo] != (uint32_t)np || h[kHdrNodesHi] != (uint32_t)(np >> 32) || h[kHdrRoot] != a.root ||
        h[kHdrCount] != a.count || h[kHdrN] != a.n) {
        if (blockIdx.x == 0 && threadIdx.x == 0) flag(a.p.hdr, RT_REFIT_PLAN_MISMATCH);
        return;
    }
    const uint32_t nleaf = min(h[kHdrLeaves], a.p.slots);
    bool broken = false;
    for (uint32_t i = blockIdx.x * kRefitThreads + threadIdx.x; i < nleaf; i += gridDim.x * kRefitThreads) {
        const uint32_t s = a.p.list[i];
        const uint32_t rec = node_w28(a.nodes, s) & kIndexMask;
        if (rec >= a.n) {   // the tree changed since the plan walked it: the plan is unusable
            flag(a.p.hdr, RT_REFIT_BAD_TREE);
            continue;
        }
        uint32_t* rw = reinterpret_cast<uint32_t*>(a.leaves + rec);
        const uint32_t id0 = rw[3], id1 = rw[7], rot = rw[11], pad = rw[15];
        const bool pair = id1 != 0u;
        float lo[3], hi[3];
        if (id0 >= a.n || (pair && (id1 != id0 + 1u || id1 >= a.n))) {
            // the record changed since the plan checked it: not read, not written; the slot keeps its box
            flag(a.p.hdr, RT_REFIT_BAD_TREE);
            load_box_sc1(a.nodes + s, lo, hi);
        } else {
            float A[9], r[9], v3[3];
            load_tri9(a.tris + (size_t)id0 * 9, A);
#pragma unroll
            for (int k = 0; k < 3; k++) { lo[k] = fmin_ord(fmin_ord(A[k], A[3 + k]), A[6 + k]); hi[k] = fmax_ord(fmax_ord(A[k], A[3 + k]), A[6 + k]); }
            if (pair) {
                // CreateTrianglePair's layout (Pairing.cuh:60-77; lbvh_levels.hip and sah_build.hip write it the same way):
                // A rotated by rotations[0], v3 = B's corner off the shared edge, picked by rotations[1]
                float B[9];
                load_tri9(a.tris + (size_t)id1 * 9, B);
                const uint32_t ra = rot & 0xFFFFu, rb = rot >> 16;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    r[k] = ra == 1 ? A[6 + k] : (ra == 2 ? A[3 + k] : A[k]);
                    r[3 + k] = ra == 1 ? A[k] : (ra == 2 ? A[6 + k] : A[3 + k]);
                    r[6 + k] = ra == 1 ? A[3 + k] : (ra == 2 ? A[k] : A[6 + k]);
                    v3[k] = rb == 2 ? B[k] : (rb == 1 ? B[3 + k] : B[6 + k]);
                    lo[k] = fmin_ord(lo[k], fmin_ord(fmin_ord(B[k], B[3 + k]), B[6 + k]));
                    hi[k] = fmax_ord(hi[k], fmax_ord(fmax_ord(B[k], B[3 + k]), B[6 + k]));
                }
                // the shared edge r2 -> r1 must still be B's edge rb (0: B0 B1, 2: B1 B2, 1: B2 B0), compared as the
                // pairing test compares corners (vequal: float ==)
                float ea[3], eb[3];   // (selects, not a runtime index: B stays in registers)
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    ea[k] = rb == 2 ? B[3 + k] : (rb == 1 ? B[6 + k] : B[k]);
                    eb[k] = rb == 2 ? B[6 + k] : (rb == 1 ? B[k] : B[3 + k]);
                }
                broken |= !(vequal(r + 6, ea) && vequal(r + 3, eb));
            } else {
#pragma unroll
                for (int k = 0; k < 9; k++) r[k] = A[k];
#pragma unroll
                for (int k = 0; k < 3; k++) v3[k] = A[6 + k];
            }
            uint4* out = reinterpret_cast<uint4*>(rw);
            out[0] = make_uint4(__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]), id0);
            out[1] = make_uint4(__float_as_uint(r[3]), __float_as_uint(r[4]), __float_as_uint(r[5]), id1);
            out[2] = make_uint4(__float_as_uint(r[6]), __float_as_uint(r[7]), __float_as_uint(r[8]), rot);
            out[3] = make_uint4(__float_as_uint(v3[0]), __float_as_uint(v3[1]), __float_as_uint(v3[2]), pad);
            store_box_sc1(a.nodes + s, lo, hi);
        }
        // climb
        uint32_t cur = s;
        while (true) {
            uint32_t e = a.p.parents[cur], run = cur;
            if ((e >> 29) == 0u) { run = cur - (e & 7u); e = a.p.parents[run]; }
            const uint32_t parent = e & kIndexMask, exp = e >> 29;
            if (parent == kRootParent) break;
            if (exp > 1) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's sc1 box stores are in memory
                const uint32_t sh = (run & 3u) * 8u;
                uint32_t* ctr = a.p.arrive + (run >> 2);
                const uint32_t old = __hip_atomic_fetch_add(ctr, 1u << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (((old >> sh) & 0x7Fu) != exp - 1u) break;
                __hip_atomic_fetch_sub(ctr, exp << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next refit
            }
            const uint32_t k = min(node_w12(a.nodes, parent) >> 29, a.p.slots - run);
            bool first = true;
            for (uint32_t j = 0; j < k; j++) {
                if ((node_w28(a.nodes, run + j) >> 29) == RT_CHILD_NONE) continue;
                float cl[3], ch[3];
                load_box_sc1(a.nodes + run + j, cl, ch);
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    lo[q] = first ? cl[q] : fmin_ord(lo[q], cl[q]);
                    hi[q] = first ? ch[q] : fmax_ord(hi[q], ch[q]);
                }
                first = false;
            }
            store_box_sc1(a.nodes + parent, lo, hi);
            cur = parent;
        }
    }
    if (broken) flag(a.p.hdr, RT_REFIT_PAIR_BROKEN);
}

uint32_t ceil_log2(uint32_t v)
{
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < v) l++;
    return l;
}

}  // namespace

RefitLayout refit_layout(uint32_t n)
{
    RefitLayout L;
    const size_t slots = rt_nodes_bytes(n) / sizeof(rt_node);
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    L.slots = (uint32_t)slots;
    L.status = 0;
    L.parents = 256;
    L.arrive = L.parents + up(slots * 4);
    L.list = L.arrive + up(slots);
    L.total = L.list + up(slots * 4);
    return L;
}

uint32_t refit_plan_wide_levels(uint32_t n) { return ceil_log2(n) + 2; }

hipError_t launch_refit_plan(const rt_build_input& in, uint32_t root, uint32_t count, void* plan, hipStream_t st)
{
    const uint32_t n = in.num_triangles, slots = refit_layout(n).slots;
    const PlanPtrs p = plan_ptrs(plan, n);
    const rt_node* nodes = in.nodes_out;
    refit_plan_init_kernel<<<min((slots + 255) / 256, 2048u), 256, 0, st>>>(p, nodes, root, count, n, slots);
    hipError_t e = hipGetLastError();
    // the widest level of a tree over n leaves holds fewer than n runs
    const uint32_t wide_blocks = min((n + kWalkThreads - 1) / kWalkThreads, 1024u);
    const uint32_t levels = refit_plan_wide_levels(n);
    for (uint32_t l = 0; e == hipSuccess && l < levels; l++) {
        refit_walk_kernel<true><<<wide_blocks, kWalkThreads, 0, st>>>(p, nodes, n, slots);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        refit_walk_kernel<false><<<1, kTailThreads, 0, st>>>(p, nodes, n, slots);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        refit_leaves_kernel<<<(slots + 1023) / 1024, 256, 0, st>>>(p, nodes, in.triangles_out, n, slots);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_refit(const rt_build_input& in, uint32_t root, uint32_t count, void* plan, hipStream_t st)
{
    const uint32_t n = in.num_triangles;
    const uint32_t slots = refit_layout(n).slots;
    RefitArgs a;
    a.p = plan_ptrs(plan, n);
    a.tris = reinterpret_cast<const float*>(in.triangles_in);
    a.leaves = in.triangles_out;
    a.nodes = in.nodes_out;
    a.root = root;
    a.count = count;
    a.n = n;
    // leaf slots: at most n (+ n/5 split references); a grid-stride loop covers any more
    const uint32_t bound = min(slots, n + n / 4 + 64);
    refit_kernel<<<(bound + kRefitThreads - 1) / kRefitThreads, kRefitThreads, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace rt
