// sdf_query.hip -- rt_signed_distance / rt_occupancy: for each caller point, how far the nearest triangle is and whether the
// point is inside the closed mesh -- one launch, through any tree rt_intersect_rays takes (semantics: rt_abi.h, signed distance
// and occupancy block).  Plus rt_generate_grid_points, the lattice those queries are usually run on.
//
// sdf_kernel<DIST, VOTES> is the frame of the sibling queries: one lane per query, 64 consecutive queries per wave, kTraceWaves
// waves (256 queries) per workgroup, xcd_chunk_block, the query in one 16-byte load, the record in one 8-byte vector store
// (DIST) or one byte store (occupancy), no atomics on the output, exact per-workgroup counters, the status word through one
// ballot per wave.  A lane runs its phases one after the other on ONE stack: the LDS column of the lane (16 slots) and one
// private tail (48 slots) serve every phase.
//   1. distance (DIST only): point_query_kernel's descent -- the k = 1 case of knn_query_kernel -- with rt_point_math.hpp's
//      routines and constants and d2 without the weights: the nearest surviving slot next, the others pushed as 8-byte
//      (entry, boxdist2) entries, pops re-culled against the best, (dist2, id) kept in registers, ties to the lower id, a pass
//      that dropped a push followed by at most kNearRestarts more from the root.  Operation for operation the traversal of
//      rt_closest_points, so (dist2, primitive_id) is that call's record bit for bit, overflowed passes included
//      (tests/test_gpu_sdf.py::test_overflowed_distance_equals_closest_points): a change to one text is a change to the other.
//   2. parity, VOTES times: ray_hits_kernel<false>'s traversal without its scan.  The ray is (p, 0, D[j], +inf); slab() and
//      intersect_tri() are rt_traverse.hpp's, unchanged, the window put back after every test; 4-byte entries, the first
//      surviving slot visited next and the others pushed in slot order, a leaf in four 16-byte requests, B tested iff
//      v3 != v2.  An unordered descent that keeps a counter and nothing else: its row length is rt_ray_hits_count's.
//      The third vote runs under the lane mask "the first two disagree"; a wave without such a lane skips the phase.
// Both phases use rt_traverse.hpp's wave-level two phases (box steps while enough lanes hold a box run, then one leaf step).
// Registers: the distance phase is the widest (Ericson's products); the DIST instantiations are held to kSdfDistWaves waves per
// SIMD, which their 32 KB of LDS per workgroup allows anyway (160 KB per CU: five workgroups of four waves); the occupancy
// instantiations keep ray_hits_kernel's bound (16 KB of LDS, eight waves per SIMD).
// Compiled with -ffp-contract=off, IEEE division and square root: every float operation is the one rt_abi.h writes down.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_point_math.hpp"
#include "rt_traverse.hpp"

static_assert(sizeof(rt_point_query) == 16 && offsetof(rt_point_query, dist2_max) == 12, "rt_point_query: p, dist2_max");
static_assert(sizeof(rt_sdf_hit) == 8 && offsetof(rt_sdf_hit, primitive_id) == 4, "rt_sdf_hit: one 8-byte record");

#ifndef RT_SDF_DIST_WAVES
#define RT_SDF_DIST_WAVES 5
#endif

namespace rt {

namespace {

// both phases share one stack: kNearStackLds entries per lane in LDS (8 bytes each with DIST: 32 KB per workgroup; else 4:
// 16 KB), the rest of kStackMax in the private tail
static_assert(kQueryBlock == kTraceWaves * 64, "rt_launch.hpp: one lane per query, kTraceWaves waves per workgroup");
constexpr int kSdfDistWaves = RT_SDF_DIST_WAVES;

struct SdfParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    uint32_t root, count;
    const float4* queries;   // rt_point_query = one float4: (p, dist2_max)
    uint2* out;              // DIST: rt_sdf_hit = one uint2: (sdist bits, primitive_id)
    uint8_t* inside;         // occupancy
    uint32_t num_queries;
    unsigned long long* counters;
    uint32_t* status;
    float dirs[3 * RT_SDF_MAX_VOTES];
};

typedef __attribute__((address_space(3))) NearEntry lds_sdf_entry;   // distance phase

template <bool DIST, int VOTES>
__global__ __launch_bounds__(kTraceWaves * 64, DIST ? kSdfDistWaves : RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA)
void sdf_kernel(SdfParams p)
{
    // one slot per (wave, entry, lane), wide enough for the widest phase; the counters' workgroup sums reuse it at the end
    constexpr int kSlotWords = DIST ? 2 : 1;
    static_assert(sizeof(NearEntry) == 2 * sizeof(uint32_t), "a distance-phase entry fills a slot of two words, in LDS and in the tail");
    __shared__ alignas(8) uint32_t stack_lds[kTraceWaves][kNearStackLds][64 * kSlotWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_queries;

    float4 q = {0.f, 0.f, 0.f, -1.f};
    if (in_range) q = p.queries[i];
    const float px = q.x, py = q.y, pz = q.z;
    // not traced (a miss, outside, no tests): lanes past the batch, a non-finite p, a NaN or negative dist2_max
    const bool finite_p = __builtin_isfinite(px) & __builtin_isfinite(py) & __builtin_isfinite(pz);
    const bool traced = in_range && finite_p && q.w >= 0.0f && p.count > 0;   // (q.w >= 0 is false for NaN)

    uint32_t spill[(kStackMax - kNearStackLds) * kSlotWords];   // the private tail: 8-byte entries in word pairs, 4-byte ones in words
    uint32_t box_tests = 0, tri_tests = 0;
    bool flagged = false;             // RT_SDF_STACK_OVERFLOW for this query
    const uint32_t root_entry = (p.root & kIndexMask) | (p.count << 29);

    // ---- phase 1: the nearest triangle
    float best = q.w;
    uint32_t best_id = RT_MISS;
    if constexpr (DIST) {
        lds_sdf_entry* const col = (lds_sdf_entry*)&stack_lds[wave][0][lane * kSlotWords];
        bool live = traced;
        int sp = 0;
        bool overflow = false;        // a push of the current pass was dropped
        int restarts = 0;
        uint32_t cur = root_entry;

        auto next_from_stack = [&]() {
            while (sp > 0) {
                --sp;
                NearEntry se;
                if (sp < kNearStackLds) se = col[sp * 64];
                else se = (uint64_t)spill[2 * (sp - kNearStackLds)] | ((uint64_t)spill[2 * (sp - kNearStackLds) + 1] << 32);
                if (__uint_as_float((uint32_t)(se >> 32)) <= best) { cur = (uint32_t)se; return; }
            }
            if (!overflow || restarts == kNearRestarts) { live = false; return; }
            restarts++;
            overflow = false;
            cur = root_entry;
        };
        auto leaf_step = [&]() {
            tri_tests++;
            const uint4* tp = reinterpret_cast<const uint4*>(p.leaves + (cur & kIndexMask));
            const uint4 l0 = tp[0], l1 = tp[1], l2 = tp[2], l3 = tp[3];
            {
                const float d = range_tri_d2(px, py, pz, leaf_tri_a(l0, l1, l2));
                if (d < best || (d == best && l0.w < best_id)) { best = d; best_id = l0.w; }
            }
            if (l1.w == l0.w + 1u) {          // a pair record: B = (v2, v1, v3) with rotations[1]
                const float d = range_tri_d2(px, py, pz, leaf_tri_b(l1, l2, l3));
                if (d < best || (d == best && l1.w < best_id)) { best = d; best_id = l1.w; }
            }
            next_from_stack();
        };
        auto box_step = [&]() {
            const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
            uint32_t near_e = kNoNear;
            float near_d = __builtin_inff();
            for (uint32_t s = 0; s < cnt; s++) {
                const uint4* np = reinterpret_cast<const uint4*>(p.nodes + first + s);
                const uint4 a = np[0], b = np[1];
                const uint32_t type = b.w >> 29;
                if (type == RT_CHILD_NONE) continue;
                box_tests++;
                const float bd = box_d2(a, b, px, py, pz);
                const uint32_t e = slot_entry(a, b);
                if (bd > best || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // pruned, or an empty run
                uint32_t pe = e;
                float pd = bd;
                if (bd < near_d) {            // the new nearest; the old one (if any) is pushed
                    pe = near_e; pd = near_d;
                    near_e = e; near_d = bd;
                }
                if (pe != kNoNear) {
                    if (sp < kNearStackLds) col[sp * 64] = (uint64_t)pe | ((uint64_t)__float_as_uint(pd) << 32);
                    else if (sp < kStackMax) {
                        spill[2 * (sp - kNearStackLds)] = pe;
                        spill[2 * (sp - kNearStackLds) + 1] = __float_as_uint(pd);
                    } else overflow = true;   // dropped: this pass may miss the nearest triangle
                    sp = min(sp + 1, kStackMax);
                }
            }
            if (near_e != kNoNear) cur = near_e;
            else next_from_stack();
        };

        while (true) {
            uint64_t stepping, parked;
            while (true) {                    // box phase: step while enough lanes hold a box run
                stepping = __builtin_amdgcn_ballot_w64(live && (cur >> 29) != 0);
                parked = __builtin_amdgcn_ballot_w64(live && (cur >> 29) == 0);
                if (stepping == 0 || __popcll(stepping) * kParkDen < __popcll(parked) * kParkNum) break;
                if (live && (cur >> 29) != 0) box_step();
            }
            if ((stepping | parked) == 0) break;
            if (live && (cur >> 29) == 0) leaf_step();   // leaf phase: every lane that holds a leaf
        }
        flagged = overflow;           // the last pass still dropped a push
    }

    // ---- phase 2: the votes.  odd = the votes so far whose crossing count is odd
    uint32_t odd = 0;
#pragma unroll 1
    for (int j = 0; j < VOTES; j++) {
        // the third vote only where the first two disagree (the majority is decided elsewhere); a wave without such a lane skips it
        const bool cast = traced && (j < 2 || odd == 1);
        if (j == 2 && __builtin_amdgcn_ballot_w64(cast) == 0) break;
        Ray r;
        r.ox = px; r.oy = py; r.oz = pz; r.tmin = 0.0f;
        r.dx = p.dirs[3 * j]; r.dy = p.dirs[3 * j + 1]; r.dz = p.dirs[3 * j + 2]; r.tmax = __builtin_inff();
        r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
        const float tmax0 = r.tmax;   // the window never shrinks: put back after every triangle test
        // a NaN direction makes the vote's ray dead (rt_ray_hits_count's rule): count 0, even
        bool live = cast && !(__builtin_isnan(r.dx) | __builtin_isnan(r.dy) | __builtin_isnan(r.dz));

        lds_u32* const col = (lds_u32*)&stack_lds[wave][0][lane];   // entry k: word `lane` of row k (conflict-free either way)
        int sp = 0;
        bool overflow = false;        // a push was dropped: the count is a lower bound
        uint32_t found = 0;
        uint32_t cur = root_entry;

        auto next_from_stack = [&]() {
            if (sp == 0) { live = false; return; }
            --sp;
            cur = sp < kNearStackLds ? col[sp * 64 * kSlotWords] : spill[sp - kNearStackLds];
        };
        auto test = [&](float c0x, float c0y, float c0z, float c1x, float c1y, float c1z, float c2x, float c2y, float c2z) {
            Hit h;
            if (!intersect_tri(c0x, c0y, c0z, c1x, c1y, c1z, c2x, c2y, c2z, r, h, 0u, 0u)) return;
            r.tmax = tmax0;
            found++;
        };
        auto leaf_step = [&]() {
            tri_tests++;
            uint4 l0, l1, l2, l3;
            load_leaf_wide(p.leaves + (cur & kIndexMask), l0, l1, l2, l3);
            test(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
                 __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                 __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z));
            // triangle B = (v2, v1, v3); for a single triangle v3 == v2 bit for bit and B is skipped (as trace_ray)
            if (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z)
                test(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                     __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                     __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z));
            next_from_stack();
        };
        auto box_step = [&]() {
            const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
            uint32_t next = kNoNear;
            for (uint32_t k = 0; k < cnt; k++) {
                const uint4* np = reinterpret_cast<const uint4*>(p.nodes + first + k);
                const uint4 a = np[0], b = np[1];
                const uint32_t type = b.w >> 29;
                if (type == RT_CHILD_NONE) continue;
                box_tests++;
                const uint32_t e = slot_entry(a, b);
                float front, back;
                slab(a, b, r, front, back);
                const bool in = (back >= front) & (front <= tmax0) & (back >= r.tmin);
                if (!in || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // missed by the ray, or an empty run
                if (next == kNoNear) { next = e; continue; }   // the first survivor is visited next, the others wait
                if (sp < kNearStackLds) col[sp * 64 * kSlotWords] = e;
                else if (sp < kStackMax) spill[sp - kNearStackLds] = e;
                else overflow = true;         // dropped: what lies below it is not counted
                sp = min(sp + 1, kStackMax);
            }
            if (next != kNoNear) cur = next;
            else next_from_stack();
        };

        while (true) {
            uint64_t stepping, parked;
            while (true) {                    // box phase: step while enough lanes hold a box run
                stepping = __builtin_amdgcn_ballot_w64(live && (cur >> 29) != 0);
                parked = __builtin_amdgcn_ballot_w64(live && (cur >> 29) == 0);
                if (stepping == 0 || __popcll(stepping) * kParkDen < __popcll(parked) * kParkNum) break;
                if (live && (cur >> 29) != 0) box_step();
            }
            if ((stepping | parked) == 0) break;
            if (live && (cur >> 29) == 0) leaf_step();   // leaf phase: every lane that holds a leaf
        }
        odd += found & 1u;
        flagged |= overflow;
    }
    const bool inside = odd * 2u > (uint32_t)VOTES;

    if (in_range) {
        if constexpr (DIST) {
            // |sdist| = sqrtf(dist2) (+inf for a miss); negated inside, but a point on the surface is +0
            float sd = best_id != RT_MISS ? sqrtf(best) : __builtin_inff();
            if (inside && sd != 0.0f) sd = -sd;
            p.out[i] = make_uint2(__float_as_uint(sd), best_id);
        } else {
            p.inside[i] = inside ? 1 : 0;
        }
    }
    if (p.status && __builtin_amdgcn_ballot_w64(flagged) != 0 && lane == 0) atomicOr(p.status, (uint32_t)RT_SDF_STACK_OVERFLOW);
    // (finish_counters of rt_device.hpp, written out: through the helper the VOTES = 3 kernels compiled to other code)
    if (p.counters) {                         // (kernel argument: the same for every thread)
        const uint32_t bsum = wave_sum_u32(box_tests), tsum = wave_sum_u32(tri_tests);
        unsigned long long* const csum = reinterpret_cast<unsigned long long*>(&stack_lds[0][0][0]);
        __syncthreads();                      // every lane is done with its stack column
        if (threadIdx.x < 2) csum[threadIdx.x] = 0ull;
        __syncthreads();
        if (lane == 0) {
            atomicAdd(&csum[0], (unsigned long long)bsum);
            atomicAdd(&csum[1], (unsigned long long)tsum);
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const unsigned long long v = csum[threadIdx.x];
            if (v) atomicAdd(&p.counters[threadIdx.x], v);
        }
    }
}

struct GridParams {
    float ox, oy, oz, sx, sy, sz;
    uint32_t dx, dy, dz;       // lattice dimensions
    uint32_t nbx, nby;         // bricks per axis (RT_GRID_BRICKS)
    float dist2_max;
    float4* queries;
    uint32_t n;                // records to write
};

// one lane per record, one 16-byte store
template <bool BRICKS>
__global__ __launch_bounds__(256) void grid_points_kernel(GridParams g)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= g.n) return;
    uint32_t ix, iy, iz;
    if (BRICKS) {
        const uint32_t lane = (uint32_t)t & 63u, brick = (uint32_t)(t >> 6);
        const uint32_t bx = brick % g.nbx, by = (brick / g.nbx) % g.nby, bz = brick / g.nbx / g.nby;
        // the 3-D Morton code of the offset inside the brick: lx = lane bits 0, 3; ly = bits 1, 4; lz = bits 2, 5
        ix = 4u * bx + ((lane & 1u) | ((lane >> 2) & 2u));
        iy = 4u * by + (((lane >> 1) & 1u) | ((lane >> 3) & 2u));
        iz = 4u * bz + (((lane >> 2) & 1u) | ((lane >> 4) & 2u));
    } else {
        ix = (uint32_t)t % g.dx;
        iy = ((uint32_t)t / g.dx) % g.dy;
        iz = (uint32_t)t / g.dx / g.dy;
    }
    float4 o = {0.f, 0.f, 0.f, -1.f};         // an off-lattice lane of an edge brick: a negative radius, not traced
    if (ix < g.dx && iy < g.dy && iz < g.dz)
        o = {g.ox + (float)ix * g.sx, g.oy + (float)iy * g.sy, g.oz + (float)iz * g.sz, g.dist2_max};
    g.queries[t] = o;
}

template <bool DIST>
hipError_t launch_sdf(const rt_accel& as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes, const float* dirs,
                      rt_sdf_hit* out, uint8_t* inside, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    SdfParams p = {};
    set_tree(p, as);
    p.queries = reinterpret_cast<const float4*>(queries);
    p.out = reinterpret_cast<uint2*>(out);
    p.inside = inside;
    p.num_queries = num_queries;
    p.counters = reinterpret_cast<unsigned long long*>(counters);
    p.status = status;
    for (uint32_t k = 0; k < 3 * votes; k++) p.dirs[k] = dirs[k];
    const dim3 grid(query_blocks(num_queries)), block(kQueryBlock);
    if (votes == 1) sdf_kernel<DIST, 1><<<grid, block, 0, st>>>(p);
    else sdf_kernel<DIST, RT_SDF_MAX_VOTES><<<grid, block, 0, st>>>(p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_signed_distance(const rt_accel& as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes,
                                  const float* dirs, rt_sdf_hit* out, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    return launch_sdf<true>(as, queries, num_queries, votes, dirs, out, nullptr, counters, status, st);
}

hipError_t launch_occupancy(const rt_accel& as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes,
                            const float* dirs, uint8_t* inside, uint64_t* counters, uint32_t* status, hipStream_t st)
{
    return launch_sdf<false>(as, queries, num_queries, votes, dirs, nullptr, inside, counters, status, st);
}

hipError_t launch_grid_points(const float origin[3], const float spacing[3], const uint32_t dims[3], float dist2_max, bool bricks,
                              uint32_t num_points, rt_point_query* queries, hipStream_t st)
{
    GridParams g;
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2];
    g.sx = spacing[0]; g.sy = spacing[1]; g.sz = spacing[2];
    g.dx = dims[0]; g.dy = dims[1]; g.dz = dims[2];
    g.nbx = (uint32_t)(((uint64_t)dims[0] + 3u) / 4u);
    g.nby = (uint32_t)(((uint64_t)dims[1] + 3u) / 4u);
    g.dist2_max = dist2_max;
    g.queries = reinterpret_cast<float4*>(queries);
    g.n = num_points;
    const uint32_t blocks = (uint32_t)(((uint64_t)num_points + 255u) / 256u);
    if (bricks) grid_points_kernel<true><<<blocks, 256, 0, st>>>(g);
    else grid_points_kernel<false><<<blocks, 256, 0, st>>>(g);
    return hipGetLastError();
}

}  // namespace rt
