// rt_launch.hpp -- host-side launch functions of each kernel group and the scratch layout.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "rt_abi.h"

namespace rt {

// hipFuncSetAttribute is a per-DEVICE setting: run `fn` the first time a launch is made on each device of the process
// (a single-process multi-GPU caller, main.cu's ncclCommInitAll shape, builds on every device).  `fn` is idempotent,
// so two threads racing on the same device only repeat it.
constexpr int kMaxDevices = 64;
struct PerDeviceOnce {
    std::atomic<unsigned char> done[kMaxDevices] = {};
    template <class F> hipError_t operator()(F fn)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= kMaxDevices) return fn();
        if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
        e = fn();
        if (e == hipSuccess) done[dev].store(1, std::memory_order_release);
        return e;
    }
};

// ---- radix sort geometry (radix_sort.hip)
// keys per workgroup (tile).  4096 shipped; -DRT_SORT_TILE=2048 / 1024 and -DRT_SORT_DS_NT=<threads of the few-tiles down-sweep>
// are experiment arms (profiles/r04_sort_experiments.txt (b)): every table and threshold below scales with the tile
#ifndef RT_SORT_TILE
#define RT_SORT_TILE 4096
#endif
constexpr uint32_t kSortTile = RT_SORT_TILE;
constexpr uint32_t kSortTileScale = 4096 / kSortTile;      // tiles per 4096 keys
static_assert(kSortTile == 4096 || kSortTile == 2048 || kSortTile == 1024, "tile sizes the kernels are written for");
constexpr uint32_t kRadixBits = 8;
constexpr uint32_t kRadix = 1u << kRadixBits;
constexpr uint32_t kSortPasses = 4;
constexpr uint32_t kRadixMax = 1024;   // the 10-bit passes of the Morton-key sort; tables are sized for it
// The down-sweep addresses keys and values through buffer descriptors of n * 4 bytes with 32-bit byte offsets: n * 4 must
// not wrap.  The builder stays far below (29-bit indices: n <= 2^28); the public sort entry points refuse larger counts.
constexpr uint32_t kSortMaxCount = 0x3FFFFFFFu;

inline uint32_t sort_num_tiles(uint32_t n) { return (n + kSortTile - 1) / kSortTile; }
// the sort's tables hold one word per (digit, tile); a row is padded to a multiple of 4 words (one aligned 16-byte access
// covers four tiles)
inline uint32_t sort_table_stride(uint32_t tiles) { return tiles ? (tiles + 3u) & ~3u : 4u; }
// many tiles: the histogram kernels take four tiles per workgroup and publish 16 bytes per digit
inline bool sort_upsweep_quads(uint32_t tiles) { return tiles > 512 * kSortTileScale; }

struct SortScratch {
    size_t digit_total;  // uint32[kSortPasses][kRadixMax]
    size_t hist;         // uint32[radix][num_tiles]
    size_t offs;         // uint32[radix][num_tiles]
    size_t total;
};
SortScratch sort_scratch_layout(uint32_t n);

// ---- LBVH level geometry (lbvh_levels.hip)
constexpr uint32_t kLeafCap = 512;    // leaves per workgroup at the leaf level
constexpr uint32_t kLeafThreads = 512;
constexpr uint32_t kUpperCap = 2048;  // open roots one upper-level pass holds in LDS
constexpr uint32_t kUpperFan = 64;    // previous-level blocks folded by one upper-level block (when their open roots fit one pass)
constexpr uint32_t kSubFan = 16;      // ... else in sub-passes of this many blocks (kSubFan * kMaxOpen always fits)
constexpr uint32_t kMaxOpen = 128;    // open sub-tree roots a block can emit (>= 2 * max tree depth 62)
constexpr uint32_t kRecDwords = 12;   // segment record: f, l, desc, cc, min[3], max[3], delta at its left end, delta at its right end
constexpr uint32_t kMaxLevels = 6;    // 2^28 leaves -> 2^19 blocks -> 8192 -> 128 -> 2 -> 1

struct LevelPlan {
    uint32_t num_levels;
    uint32_t fan;                    // previous-level blocks folded by one upper-level block (<= kUpperFan)
    uint32_t blocks[kMaxLevels];
    size_t cnt_off[kMaxLevels];      // uint32[blocks]
    size_t rec_off[kMaxLevels];      // uint32[blocks][kMaxOpen][kRecDwords]
    size_t arrive_lvl[kMaxLevels];   // uint32[blocks] tickets taken at this level's blocks (inside the arrive region)
    size_t sub_cnt_off[kMaxLevels];  // fallback scratch of the upper levels
    size_t sub_rec_off[kMaxLevels];
    size_t arrive_off, arrive_bytes; // all arrival counters, contiguous: must be zero when the build kernel starts
    size_t sink_off;                 // 64 bytes nobody reads: where the upper passes' predicated-off stores land
    size_t total;
};
LevelPlan lbvh_level_plan(uint32_t n);

// ---- whole-build scratch layout
struct BuLayout {
    size_t p_aabb;          // int32[6]
    size_t status;          // uint32[8]: [0] error flags, [1] number of leaves L of the last build
    size_t morton;          // uint32[n]
    size_t sorted_indices;  // uint32[n]
    size_t tmp_keys;        // uint32[n]
    size_t tmp_vals;        // uint32[n]
    size_t sort;            // SortScratch
    size_t levels;          // LevelPlan
    size_t hybrid;          // hybrid top-tree work area
    size_t pair_flags;      // uint8[(n+1)/2] merge decision per candidate (--pairs)
    size_t pair_sums;       // uint32[ceil((n+1)/2 / 256)] leaf counts / offsets per workgroup (--pairs)
    size_t aabb_parts;      // int32[kAabbParts][6] partial scene boxes (one per workgroup of the scene-box kernel)
    size_t total;
};
BuLayout bu_layout(uint32_t n);

// ---- SAH build scratch (sah_build.hip)
struct SahLayout {
    size_t header, aabbs, ids0, ids1, task_of0, task_of1, binof, tasks0, tasks1, splits, bins0, bins1, chunk_hist,
        chunk_prefix, small, sort, pair_flags, pair_sums, item_leaf, split_flags, split_sums_a, split_sums_b;
    size_t status;       // uint32[8] inside the header: [0] error flags, [1] number of leaves L
    size_t cell_counts;  // uint32[64] inside the header
    size_t total;
};
SahLayout sah_layout(uint32_t n);

// ---- launches
hipError_t launch_reset_aabb(int* aabb, hipStream_t st);
// scene box: `aabb` holds nparts ordered-int boxes (6 ints each, reset to empty by the caller); workgroup b folds into box
// b mod nparts.  The Morton kernels fold the nparts boxes and (aabb_out != null) publish the result.
constexpr uint32_t kAabbParts = 510;   // at most this many partial boxes (one per workgroup of the build's scene-box kernel)
hipError_t launch_scene_aabb(const rt_triangle* tris, uint32_t n, int* aabb, hipStream_t st, uint32_t nparts = 1);
// the build's first launch (n > 0): partial boxes by plain stores, *nparts_out of them, + status words and the LBVH level
// hand-off counters zeroed
hipError_t launch_scene_aabb_build(const rt_triangle* tris, uint32_t n, int* aabb_parts, uint32_t* nparts_out, uint32_t* status,
                                   uint32_t* arrive, uint32_t arrive_words, hipStream_t st);
hipError_t launch_morton(uint32_t* codes, uint32_t* values, const rt_triangle* tris, const int* aabb, uint32_t n,
                         hipStream_t st, uint32_t nparts = 1, int* aabb_out = nullptr);
// the same codes / values plus the first sort pass's tile histograms (digit = low `bits` bits, bits = 8 or 10) in one
// launch: one workgroup per sort tile
// values == nullptr: they are not written (the sort's first pass then takes them as the identity)
hipError_t launch_morton_hist(uint32_t* codes, uint32_t* values, const rt_triangle* tris, const int* aabb, uint32_t n,
                              hipStream_t st, uint32_t nparts, int* aabb_out, uint32_t* hist, uint32_t bits);
hipError_t launch_morton_pairs(uint32_t* codes, uint32_t* values, const rt_triangle* tris, const int* aabb, uint32_t n,
                               uint8_t* flags, uint32_t* block_sums, uint32_t* num_leaves, hipStream_t st,
                               uint32_t nparts = 1, int* aabb_out = nullptr);
// n_dev (may be null): device word holding the real element count (<= n); n then only sizes the grids.
// key_bits <= 30 (Morton keys): 3 passes of 10 bits, and the INPUT is taken from (tmp_keys, tmp_vals); the sorted result
// is in (keys, vals) either way.
// have_hist0: the first pass's tile histograms are already in the sort scratch (launch_morton_hist wrote them).
// ident0: the input values are the identity (values[i] = i) and are not read.
hipError_t launch_radix_sort(uint32_t* keys, uint32_t* vals, uint32_t* tmp_keys, uint32_t* tmp_vals, uint32_t n,
                             void* sort_scratch, hipStream_t st, const uint32_t* n_dev = nullptr, uint32_t key_bits = 32,
                             bool have_hist0 = false, bool ident0 = false);
bool sort_three_passes(uint32_t tiles);          // keys of <= 30 bits: 3 x 10-bit passes (else 4 x 8)
// the builder's choice: tiles of the Morton-key sort up to which 3 x 10-bit passes beat 4 x 8-bit (measured: 85 vs 93 us at
// 245 tiles, 420 vs 300 us at 2444 -- the 1024-digit tables and 16-byte runs cost more than the saved pass)
constexpr uint32_t kSort3PassMaxTiles = 512 * kSortTileScale;
uint32_t* sort_hist_table(void* sort_scratch, uint32_t n);   // hist[radix][tiles] of the sort scratch
hipError_t launch_lbvh_levels(const rt_triangle* tris, const uint32_t* codes, const uint32_t* sorted_indices,
                              uint32_t n, rt_triangle_pair* leaves, rt_node* nodes, void* level_scratch,
                              uint32_t* status, hipStream_t st, const uint32_t* n_dev = nullptr);

// one stable 8-bit pass (keys_in, vals_in) -> (keys_out, vals_out) on bits [shift, shift+8); *digit_total (device,
// uint32[256], valid after the pass) = number of keys per digit
hipError_t launch_radix_pass(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                             uint32_t n, uint32_t shift, void* sort_scratch, hipStream_t st, const uint32_t* n_dev,
                             uint32_t** digit_total);
// --pairs leaf slots: merge flag per candidate (2k, 2k+1), per-workgroup slot offsets, *num_leaves = L
hipError_t launch_pair_slots(const rt_triangle* tris, uint32_t n, uint8_t* flags, uint32_t* block_sums,
                             uint32_t* num_leaves, hipStream_t st);
// RunSahBuild.  Asynchronous (a fixed number of launches; nothing is read back).  *levels_run (may be null) = level launches
// enqueued; *status0 (may be null) is set to 0 -- the error flags live in the scratch status word.
hipError_t launch_sah_build(const rt_triangle* tris, uint32_t n, bool pairs, bool splits, rt_triangle_pair* leaves,
                            rt_node* nodes, void* scratch, hipStream_t st, uint32_t* levels_run, uint32_t* status0 = nullptr);
// in-place exclusive scan of per-workgroup sums (one workgroup); *total = their sum
hipError_t launch_block_scan(uint32_t* sums, uint32_t count, uint32_t* total, hipStream_t st);

hipError_t launch_hybrid_top(rt_node* nodes, const int* aabb_ordered, uint32_t n, hipStream_t st,
                             const uint32_t* n_dev = nullptr);

struct TraceLaunch {
    rt_accel as;
    rt_scene scene;
    uint64_t* counters;
    int render_type;
    uint8_t* rgba8;
    uint32_t w, h, y0, y1, spp;
    uint32_t strip_rows = 0, strip_first = 0, strip_stride = 1;   // strip_rows > 0: interleaved strips, compact output
};
hipError_t launch_trace(const TraceLaunch& t, hipStream_t st);

// ---- what the launches of the ray query families share (ray_query.hip, ray_hits_query.hip, ray_first_query.hip,
// instances.hip).  Each of them takes a filter pointer: null launches the unfiltered instantiation of its kernel, anything
// else (checked by the entry point: flags, alignments) the FILTERED one.
constexpr uint32_t kQueryBlock = 256;   // one lane per ray, four waves per workgroup (the files assert it against kTraceWaves)
inline uint32_t query_blocks(uint64_t n) { return (uint32_t)((n + kQueryBlock - 1) / kQueryBlock); }
// the tree's four fields, which every params struct of these kernels begins with
template <class P> inline void set_tree(P& p, const rt_accel& as)
{
    p.nodes = as.nodes;
    p.leaves = as.triangles;
    p.root = as.root;
    p.count = as.count;
}
// the pair-prefetch x any-hit choice of a kernel instantiation: launch(pf, any) gets two std::bool_constant values
template <class F> inline void dispatch_pf_any(bool pf, bool any_hit, F launch)
{
    if (pf) {
        if (any_hit) launch(std::true_type(), std::true_type());
        else launch(std::true_type(), std::false_type());
    } else {
        if (any_hit) launch(std::false_type(), std::true_type());
        else launch(std::false_type(), std::false_type());
    }
}

// ray_query.hip: rt_intersect_rays[_filtered] / rt_generate_camera_rays after their argument checks (num_rays > 0, w * h > 0)
hipError_t launch_ray_query(const rt_accel& as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, bool any_hit,
                            uint32_t num_primitives, const rt_hit_filter* filter, uint64_t* counters, hipStream_t st);
hipError_t launch_camera_rays(const rt_camera* camera, uint32_t w, uint32_t h, uint32_t spp, bool tiled, rt_ray* rays,
                              hipStream_t st);

// ray_query.hip: rt_intersect_rays_indexed after its argument checks (num_indices > 0)
hipError_t launch_ray_query_indexed(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const uint32_t* order,
                                    uint32_t num_indices, rt_hit* hits, bool any_hit, uint32_t num_primitives,
                                    uint64_t* counters, hipStream_t st);

// motion_query.hip: rt_intersect_rays_motion[_indexed] (num_rays > 0) / rt_motion_validate after their argument checks
// order == null: lane j takes ray j; else (rt_intersect_rays_motion_indexed, num_indices > 0) lane j takes ray order[j]
hipError_t launch_motion_query(const rt_motion_accel& as, const rt_ray* rays, const float* times, rt_hit* hits, uint32_t num_rays,
                               const uint32_t* order, uint32_t num_indices, bool any_hit, uint64_t* counters, hipStream_t st);
hipError_t launch_motion_validate(const rt_motion_accel& as, uint32_t num_triangles, uint32_t* status, hipStream_t st);

// instance_motion_query.hip: rt_prepare_motion_instances / rt_intersect_rays_instanced_motion[_indexed] (num_rays > 0) after
// their argument checks (order: as launch_motion_query's)
hipError_t launch_prepare_motion_instances(const rt_motion_instance* instances, uint32_t num_instances,
                                           const rt_accel* blas_table, uint32_t num_blas, rt_triangle* proxies0,
                                           rt_triangle* proxies1, rt_motion_instance_record* records, uint32_t* status,
                                           hipStream_t st);
hipError_t launch_instance_motion_query(const rt_motion_accel& tlas, const rt_motion_instance_record* records,
                                        uint32_t num_instances, const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays,
                                        const float* times, rt_hit* hits, uint32_t* instance_ids, uint32_t num_rays,
                                        const uint32_t* order, uint32_t num_indices, bool any_hit, uint64_t* counters,
                                        hipStream_t st);

// sphere_query.hip: rt_prepare_spheres / rt_intersect_rays_spheres after their argument checks (the query: a launch of at
// least one lane; order == null: lane j takes ray j)
hipError_t launch_prepare_spheres(const rt_sphere* spheres, uint32_t num_spheres, rt_triangle* proxies, uint32_t* status,
                                  hipStream_t st);
hipError_t launch_sphere_query(const rt_accel& as, const rt_sphere* spheres, uint32_t num_spheres, const rt_ray* rays,
                               uint32_t num_rays, const uint32_t* order, uint32_t num_indices, rt_hit* hits, bool any_hit,
                               uint64_t* counters, hipStream_t st);

// capsule_query.hip: rt_prepare_capsules / rt_intersect_rays_capsules after their argument checks (as the sphere pair)
hipError_t launch_prepare_capsules(const rt_capsule* capsules, uint32_t num_capsules, rt_triangle* proxies, uint32_t* status,
                                   hipStream_t st);
hipError_t launch_capsule_query(const rt_accel& as, const rt_capsule* capsules, uint32_t num_capsules, const rt_ray* rays,
                                uint32_t num_rays, const uint32_t* order, uint32_t num_indices, rt_hit* hits, bool any_hit,
                                uint64_t* counters, hipStream_t st);

// sphere_cast_query.hip: rt_sphere_cast after its argument checks (a launch of at least one lane; order == null: lane j takes
// ray j; radii == null: every ray takes `radius`; features may be null)
hipError_t launch_sphere_cast(const rt_accel& as, const rt_ray* rays, const float* radii, float radius, uint32_t num_rays,
                              const uint32_t* order, uint32_t num_indices, rt_hit* hits, uint32_t* features, bool any_hit,
                              uint64_t* counters, hipStream_t st);

// ray_sort.hip: rt_sort_rays after its argument checks (num_rays > 0)
struct RaySortLayout {
    size_t box;         // float lo[4], hi[4] at the start of the 256-byte header
    size_t num_live;    // uint32 inside the header
    size_t keys;        // uint32[n]: the sorted keys after the call
    size_t tmp_keys;    // uint32[n]
    size_t tmp_values;  // uint32[n]
    size_t sort;        // SortScratch
    size_t total;
};
RaySortLayout ray_sort_layout(uint32_t num_rays);
hipError_t launch_sort_rays(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, uint32_t* order, void* scratch,
                            hipStream_t st);

// refit.hip: rt_build_refit_plan / rt_refit after their argument checks (n > 0)
struct RefitLayout {
    size_t status;    // the plan header (256 bytes; word 0 = RT_REFIT_* flags)
    size_t parents;   // uint32[slots]
    size_t arrive;    // uint8[slots]
    size_t list;      // uint32[slots]
    size_t total;
    uint32_t slots;   // rt_nodes_bytes(n) / 32
};
RefitLayout refit_layout(uint32_t n);
uint32_t refit_plan_wide_levels(uint32_t n);   // wide walk launches of a plan build (then one single-workgroup launch)
hipError_t launch_refit_plan(const rt_build_input& in, uint32_t root, uint32_t count, void* plan, hipStream_t st);
hipError_t launch_refit(const rt_build_input& in, uint32_t root, uint32_t count, void* plan, hipStream_t st);

// shade.hip: rt_generate_shadow_rays / rt_shade_frame after their argument checks (num_rays > 0, w * h > 0)
hipError_t launch_shadow_rays(const rt_ray* rays, const rt_hit* hits, uint32_t num_rays, uint32_t num_triangles,
                              const float light[3], rt_ray* shadow_rays, hipStream_t st);
struct ShadeLaunch {
    rt_scene scene;                // attributes, materials, textures, light (the camera pointer is not read)
    const rt_triangle* triangles;  // the caller's triangles
    uint32_t num_triangles;
    const rt_ray* rays;
    const rt_hit* hits;
    const rt_hit* shadow_hits;     // RT_RENDER_TEXTURE_LIT_SHADOWS only
    uint32_t w, h, spp;
    bool tiled;
    int render_type;
    uint8_t* rgba8;
};
hipError_t launch_shade_frame(const ShadeLaunch& t, hipStream_t st);
// shade_instanced.hip: rt_shade_frame_instanced after its argument checks (w * h > 0; num_instances > 0: geometry, instances
// and records non-null)
struct ShadeInstancedLaunch {
    rt_scene scene;                       // materials, textures, light and their counts (attributes come from `geometry`)
    const rt_shade_geometry* geometry;    // parallel to the BLAS table
    uint32_t num_blas;
    const rt_instance* instances;
    const rt_instance_record* records;
    uint32_t num_instances;
    const int32_t* instance_materials;    // optional
    const rt_ray* rays;
    const rt_hit* hits;
    const uint32_t* instance_ids;
    const uint32_t* shadow_instance_ids;  // RT_RENDER_TEXTURE_LIT_SHADOWS only
    uint32_t w, h, spp;
    bool tiled;
    int render_type;
    uint32_t flags;                       // RT_SHADE_*
    uint8_t* rgba8;
};
hipError_t launch_shade_frame_instanced(const ShadeInstancedLaunch& t, hipStream_t st);

// instances.hip: rt_prepare_instances / rt_intersect_rays_instanced[_filtered | _indexed] after their argument checks (the
// query: num_rays > 0)
hipError_t launch_prepare_instances(const rt_instance* instances, uint32_t num_instances, const rt_accel* blas_table,
                                    uint32_t num_blas, rt_triangle* proxies, rt_instance_record* records, uint32_t* status,
                                    hipStream_t st);
struct InstanceQuery {
    rt_accel tlas;
    const rt_instance_record* records;
    uint32_t num_instances;
    const rt_accel* blas_table;
    uint32_t num_blas;
    const rt_ray* rays;
    rt_hit* hits;
    uint32_t* instance_ids;
    uint32_t num_rays;
    bool any_hit;
    uint32_t num_primitives;
    uint64_t* counters;
    // the index list of rt_intersect_rays_instanced_indexed / _mixed_indexed (num_indices > 0); null: lane j takes ray j.
    // The set-valued launches do not read it.
    const uint32_t* order = nullptr;
    uint32_t num_indices = 0;
};
hipError_t launch_instance_query(const InstanceQuery& q, const rt_instance_hit_filter* filter, hipStream_t st);
// instance_mixed_query.hip: rt_intersect_rays_instanced_mixed[_indexed] after its argument checks (num_rays > 0, geom_table non-null;
// q.num_primitives is not read: no pair-prefetch arm).  capsules: rt_intersect_rays_instanced_mixed_capsules's kernels, which
// also enter RT_GEOM_CAPSULES entries
hipError_t launch_instance_mixed_query(const InstanceQuery& q, const rt_geometry* geom_table, bool capsules, hipStream_t st);

// point_query.hip: rt_closest_points after its argument checks (num_queries > 0)
hipError_t launch_point_query(const rt_accel& as, const rt_point_query* queries, rt_point_hit* hits, uint32_t num_queries,
                              uint64_t* counters, uint32_t* status, hipStream_t st);

// csr_scan.hip: the tail of every CSR count call.  offsets[0..n) hold workgroup-local exclusive prefixes and block_sums one
// total per workgroup of 256 queries (rt_csr.hpp); afterwards offsets[0..n] are the exclusive prefixes of the whole batch.
// Runs for n = 0 too (offsets[0] = 0).
hipError_t launch_csr_offsets(uint64_t* offsets, uint64_t* block_sums, uint32_t n, hipStream_t st);

// range_query.hip: rt_range_count / rt_range_collect after their argument checks.  Count runs for num_queries = 0 too (it
// writes offsets[0] = 0); collect is called with num_queries > 0.  queries: rt_point_query (sphere) or rt_range_box (box).
size_t range_scratch_bytes(uint32_t num_queries);   // uint64 per workgroup of 256 queries, 256-byte aligned
hipError_t launch_range_count(const rt_accel& as, const void* queries, uint32_t num_queries, int shape, uint64_t* offsets,
                              void* scratch, uint64_t* counters, uint32_t* status, hipStream_t st);
hipError_t launch_range_collect(const rt_accel& as, const void* queries, uint32_t num_queries, int shape,
                                const uint64_t* offsets, uint32_t* ids, uint32_t* counts, uint64_t* counters, uint32_t* status,
                                hipStream_t st);

// knn_query.hip: rt_k_nearest after its argument checks (num_queries > 0, 1 <= k <= RT_KNN_MAX_K)
hipError_t launch_knn_query(const rt_accel& as, const rt_point_query* queries, uint32_t num_queries, uint32_t k, rt_knn_hit* out,
                            uint64_t* counters, uint32_t* status, hipStream_t st);

// ray_hits_query.hip: rt_ray_hits_count[_filtered] / rt_ray_hits_collect[_filtered] after their argument checks.  Count runs
// for num_rays = 0 too (it writes offsets[0] = 0); collect is called with num_rays > 0.
size_t ray_hits_scratch_bytes(uint32_t num_rays);   // uint64 per workgroup of 256 rays, 256-byte aligned
hipError_t launch_ray_hits_count(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                                 uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, hipStream_t st);
hipError_t launch_ray_hits_collect(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                                   const uint64_t* offsets, rt_hit* hits, uint32_t* counts, uint64_t* counters,
                                   uint32_t* status, hipStream_t st);

// ray_hits_instanced_query.hip: rt_ray_hits_count_instanced[_filtered] / rt_ray_hits_collect_instanced[_filtered] after their
// argument checks (both are called with num_rays > 0).  q.hits / q.instance_ids: the collect call's rows; q.any_hit and
// q.num_primitives are not read.  filter: null runs the unfiltered kernel, else (checked by the entry point: flags, alignments)
// the FILTERED one.
hipError_t launch_ray_hits_count_instanced(const InstanceQuery& q, const rt_instance_hit_filter* filter, uint64_t* offsets,
                                           void* scratch, uint32_t* status, hipStream_t st);
hipError_t launch_ray_hits_collect_instanced(const InstanceQuery& q, const rt_instance_hit_filter* filter,
                                             const uint64_t* offsets, uint32_t* counts, uint32_t* status, hipStream_t st);

// ray_first_query.hip: rt_ray_first_hits[_filtered] after its argument checks (num_rays > 0, 1 <= k <= RT_RAY_FIRST_MAX_K)
hipError_t launch_ray_first_hits(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, uint32_t k,
                                 const rt_hit_filter* filter, rt_hit* out, uint64_t* counters, uint32_t* status, hipStream_t st);

// ray_first_instanced_query.hip: rt_ray_first_hits_instanced[_filtered] after its argument checks (num_rays > 0, 1 <= k <=
// RT_RAY_FIRST_MAX_K).  q.hits / q.instance_ids: the rows of k; q.any_hit and q.num_primitives are not read.  filter: as above.
hipError_t launch_ray_first_hits_instanced(const InstanceQuery& q, uint32_t k, const rt_instance_hit_filter* filter,
                                           uint32_t* status, hipStream_t st);

// tri_overlap_query.hip: rt_tri_overlaps_count / rt_tri_overlaps_collect after their argument checks.  Count runs for
// num_queries = 0 too (it writes offsets[0] = 0); collect is called with num_queries > 0.  self: RT_TRI_SELF.
size_t tri_overlaps_scratch_bytes(uint32_t num_queries);   // uint64 per workgroup of 256 queries, 256-byte aligned
hipError_t launch_tri_overlaps_count(const rt_accel& as, const rt_triangle* queries, uint32_t num_queries, bool self,
                                     uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, hipStream_t st);
hipError_t launch_tri_overlaps_collect(const rt_accel& as, const rt_triangle* queries, uint32_t num_queries, bool self,
                                       const uint64_t* offsets, uint32_t* ids, uint32_t* counts, uint64_t* counters,
                                       uint32_t* status, hipStream_t st);

// sdf_query.hip: rt_signed_distance / rt_occupancy after their argument checks (num_queries > 0, votes 1 or 3, dirs: host
// float[3 * votes], never null here), rt_generate_grid_points after its checks (num_points > 0 records to write)
hipError_t launch_signed_distance(const rt_accel& as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes,
                                  const float* dirs, rt_sdf_hit* out, uint64_t* counters, uint32_t* status, hipStream_t st);
hipError_t launch_occupancy(const rt_accel& as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes,
                            const float* dirs, uint8_t* inside, uint64_t* counters, uint32_t* status, hipStream_t st);
hipError_t launch_grid_points(const float origin[3], const float spacing[3], const uint32_t dims[3], float dist2_max, bool bricks,
                              uint32_t num_points, rt_point_query* queries, hipStream_t st);

}  // namespace rt
