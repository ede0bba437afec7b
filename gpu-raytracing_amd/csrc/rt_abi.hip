// rt_abi.hip -- the extern "C" entry points declared in include/rt_abi.h.
// Host orchestration only: scratch carving and kernel order (the role of BuildWrapper.cu:68-136,
// 253-362 and main.cu:125-192 in the reference).  No allocation, no host<->device copies of data: every call is a
// sequence of asynchronous launches on the caller's stream (rt_run_sah_build too: its number of launches is fixed by
// n, the data-dependent tail is a device-side loop, sah_build.hip).
#include "rt_device.hpp"
#include "rt_launch.hpp"

namespace rt {

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

BuLayout bu_layout(uint32_t n)
{
    BuLayout L;
    const size_t nn = n ? n : 1;
    size_t off = 0;
    L.p_aabb = off;         off += 32;
    L.status = off;         off += 32;
    off = align_up(off, 256);
    L.morton = off;         off = align_up(off + nn * 4, 256);
    L.sorted_indices = off; off = align_up(off + nn * 4, 256);
    L.tmp_keys = off;       off = align_up(off + nn * 4, 256);
    L.tmp_vals = off;       off = align_up(off + nn * 4, 256);
    L.sort = off;           off = align_up(off + sort_scratch_layout(n).total, 256);
    L.levels = off;         off = align_up(off + lbvh_level_plan(n).total, 256);
    L.hybrid = off;         off = align_up(off + 64 * 1024, 256);
    L.pair_flags = off;     off = align_up(off + (nn + 1) / 2, 256);
    L.pair_sums = off;      off = align_up(off + ((nn + 1) / 2 / 256 + 2) * 4, 256);
    L.aabb_parts = off;     off = align_up(off + kAabbParts * 6 * 4, 256);
    L.total = off;
    return L;
}

static inline int hip_rc(hipError_t e) { return e == hipSuccess ? RT_OK : RT_ERR_HIP_BASE - (int)e; }

// one launch for the build's tiny initialisations: status words = 0, the ordered-int "empty" scene box
// (BuildWrapper.cu:288-303 does these with 6 memset / memcpy calls) and the LBVH hierarchy's arrival counters = 0
__global__ __launch_bounds__(256) void build_init_kernel(uint32_t* status, int* aabb, int* aabb_parts, uint32_t n,
                                                         uint32_t* arrive, uint32_t arrive_words)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < arrive_words; i += gridDim.x * 256) arrive[i] = 0;
    if (blockIdx.x != 0) return;
    if (threadIdx.x < 8) status[threadIdx.x] = threadIdx.x == 1 ? n : 0;   // [1] = number of leaves (pairs: overwritten)
    if (threadIdx.x < 6) aabb[threadIdx.x] = threadIdx.x < 3 ? 0x7f7fffff : (int)0x80800000;
    for (uint32_t i = threadIdx.x; i < 6; i += blockDim.x) aabb_parts[i] = (i % 6) < 3 ? 0x7f7fffff : (int)0x80800000;
}

}  // namespace rt

using namespace rt;

extern "C" {

size_t rt_bu_memory_requirements(uint32_t num_triangles) { return bu_layout(num_triangles).total; }

size_t rt_nodes_bytes(uint32_t num_triangles)
{
    // main.cu:235-237: sizeof(Node) * (n + max(512, NUM_BLOCKS)) * 2 * 2
    return sizeof(rt_node) * ((size_t)num_triangles + 512) * 4;
}

int rt_bu_scratch_layout_get(uint32_t num_triangles, rt_bu_scratch_layout* out)
{
    if (!out) return RT_ERR_INVALID_ARGUMENT;
    const BuLayout L = bu_layout(num_triangles);
    out->p_aabb = L.p_aabb;
    out->status = L.status;
    out->num_leaves = L.status + 4;
    out->morton = L.morton;
    out->sorted_indices = L.sorted_indices;
    out->total = L.total;
    return RT_OK;
}

int rt_calculate_scene_aabb(const rt_triangle* triangles, uint32_t n, int32_t* aabb_ordered, void* stream)
{
    if (!aabb_ordered || (n && !triangles)) return RT_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = launch_reset_aabb(aabb_ordered, st);
    if (e == hipSuccess) e = launch_scene_aabb(triangles, n, aabb_ordered, st);
    return hip_rc(e);
}

int rt_generate_morton_codes(uint32_t* codes, uint32_t* values, const rt_triangle* triangles,
                             const int32_t* aabb_ordered, uint32_t n, void* stream)
{
    if (n && (!codes || !values || !triangles || !aabb_ordered)) return RT_ERR_INVALID_ARGUMENT;
    return hip_rc(launch_morton(codes, values, triangles, aabb_ordered, n, static_cast<hipStream_t>(stream)));
}

size_t rt_radix_sort_scratch_bytes(uint32_t count) { return sort_scratch_layout(count).total; }

int rt_radix_sort_u32_pairs(uint32_t* keys, uint32_t* values, uint32_t* tmp_keys, uint32_t* tmp_values,
                            uint32_t count, void* sort_scratch, void* stream)
{
    if (count && (!keys || !values || !tmp_keys || !tmp_values || !sort_scratch)) return RT_ERR_INVALID_ARGUMENT;
    if (count > kSortMaxCount) return RT_ERR_TOO_LARGE;   // 32-bit byte offsets of the buffer descriptors (rt_abi.h)
    return hip_rc(launch_radix_sort(keys, values, tmp_keys, tmp_values, count, sort_scratch,
                                    static_cast<hipStream_t>(stream)));
}

int rt_radix_sort_u32_pairs_bits(uint32_t* keys, uint32_t* values, uint32_t* tmp_keys, uint32_t* tmp_values,
                                 uint32_t count, uint32_t key_bits, int input_in_tmp, void* sort_scratch, void* stream)
{
    if (count && (!keys || !values || !tmp_keys || !tmp_values || !sort_scratch)) return RT_ERR_INVALID_ARGUMENT;
    if (key_bits == 0 || key_bits > 32) return RT_ERR_INVALID_ARGUMENT;
    if (count > kSortMaxCount) return RT_ERR_TOO_LARGE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // an odd number of passes (3 x 10 bits) reads its input from the temporaries, an even one (4 x 8) from keys / values:
    // the result is in keys / values either way.  The input is moved only when it sits on the other side.
    const bool wants_tmp = key_bits <= 30 && sort_three_passes(sort_num_tiles(count));
    if (count && wants_tmp != (input_in_tmp != 0)) {
        uint32_t *sk = input_in_tmp ? tmp_keys : keys, *sv = input_in_tmp ? tmp_values : values;
        uint32_t *dk = input_in_tmp ? keys : tmp_keys, *dv = input_in_tmp ? values : tmp_values;
        hipError_t e = hipMemcpyAsync(dk, sk, (size_t)count * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(dv, sv, (size_t)count * 4, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return hip_rc(e);
    }
    return hip_rc(launch_radix_sort(keys, values, tmp_keys, tmp_values, count, sort_scratch, st, nullptr, key_bits));
}

int rt_radix_sort_input_in_tmp(uint32_t count, uint32_t key_bits)
{
    return key_bits <= 30 && sort_three_passes(sort_num_tiles(count)) ? 1 : 0;
}

int rt_run_bottom_up_build(const rt_build_input* input, const rt_arguments* args, int hybrid, void* stream)
{
    if (!input || !input->nodes_out || !input->scratch) return RT_ERR_INVALID_ARGUMENT;
    const uint32_t n = input->num_triangles;
    if (n && (!input->triangles_in || !input->triangles_out)) return RT_ERR_INVALID_ARGUMENT;
    if (n > (1u << 28)) return RT_ERR_TOO_LARGE;  // 2(n-1) slots must fit the 29-bit child field
    // args->enable_splits is ignored here, as in the reference: only RunSahBuild has a split pre-pass (BuildWrapper.cu:188-210)
    const bool pairs = args && args->enable_pairs;
    if ((reinterpret_cast<uintptr_t>(input->scratch) & 255u) || (reinterpret_cast<uintptr_t>(input->triangles_in) & 15u) ||
        (reinterpret_cast<uintptr_t>(input->triangles_out) & 63u) || (reinterpret_cast<uintptr_t>(input->nodes_out) & 63u))
        return RT_ERR_INVALID_ARGUMENT;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const BuLayout L = bu_layout(n);
    char* s = static_cast<char*>(input->scratch);
    int* p_aabb = reinterpret_cast<int*>(s + L.p_aabb);
    uint32_t* status = reinterpret_cast<uint32_t*>(s + L.status);
    uint32_t* morton = reinterpret_cast<uint32_t*>(s + L.morton);
    uint32_t* sorted = reinterpret_cast<uint32_t*>(s + L.sorted_indices);
    uint32_t* tmpk = reinterpret_cast<uint32_t*>(s + L.tmp_keys);
    uint32_t* tmpv = reinterpret_cast<uint32_t*>(s + L.tmp_vals);

    int* aabb_parts = reinterpret_cast<int*>(s + L.aabb_parts);
    const LevelPlan lp = lbvh_level_plan(n);
    const uint32_t arrive_words = (uint32_t)(lp.arrive_bytes / 4);
    uint32_t* arrive = reinterpret_cast<uint32_t*>(s + L.levels + lp.arrive_off);
    uint32_t nparts = 1;
    hipError_t e;
    if (n) {
        // the first launch: scene bounds (partial boxes, folded by the Morton kernels) + the build's initialisations
        e = launch_scene_aabb_build(input->triangles_in, n, aabb_parts, &nparts, status, arrive, arrive_words, st);
    } else {
        build_init_kernel<<<1, 256, 0, st>>>(status, p_aabb, aabb_parts, n, arrive, arrive_words);
        e = hipGetLastError();
    }
    // with --pairs the number of leaves L <= n is only known on the device (status[1]); the reference copies it
    // back to the host (BuildWrapper.cu:317-321, a sync) -- here the downstream kernels read it from memory and the
    // grids are sized for n
    uint32_t* num_leaves = status + 1;
    const uint32_t* n_dev = pairs ? num_leaves : nullptr;
    // The sort of the 30-bit Morton keys: 3 passes x 10 bits while the tables stay small (kSort3PassMaxTiles), else 4 x 8.
    // An odd number of passes ends in the other buffer pair, so the Morton kernels then write into the temporaries.
    // Without --pairs the Morton kernel also produces the first pass's tile histograms (one launch fewer).
    const bool three = sort_three_passes(sort_num_tiles(n));
    uint32_t* code_dst = three ? tmpk : morton;
    uint32_t* value_dst = three ? tmpv : sorted;
    if (e == hipSuccess) {
        if (pairs)
            e = launch_morton_pairs(code_dst, value_dst, input->triangles_in, aabb_parts, n, reinterpret_cast<uint8_t*>(s + L.pair_flags),
                                    reinterpret_cast<uint32_t*>(s + L.pair_sums), num_leaves, st, nparts, p_aabb);
        else
            // (the values of this path are the identity, BottomUpBuilder.cu:113: not written, the sort's first pass regenerates them)
            e = launch_morton_hist(code_dst, nullptr, input->triangles_in, aabb_parts, n, st, nparts, p_aabb,
                                   sort_hist_table(s + L.sort, n), three ? 10 : 8);
    }
    if (e == hipSuccess)
        e = launch_radix_sort(morton, sorted, tmpk, tmpv, n, s + L.sort, st, n_dev, three ? 30 : 32, !pairs, !pairs);
    if (e == hipSuccess)
        e = launch_lbvh_levels(input->triangles_in, morton, sorted, n, input->triangles_out, input->nodes_out,
                               s + L.levels, status, st, n_dev);
    if (e == hipSuccess && hybrid) e = launch_hybrid_top(input->nodes_out, p_aabb, n, st, n_dev);   // BuildWrapper.cu:350-361
    return hip_rc(e);
}

size_t rt_sah_memory_requirements(uint32_t num_triangles) { return sah_layout(num_triangles).total; }

int rt_sah_scratch_layout_get(uint32_t num_triangles, rt_sah_scratch_layout* out)
{
    if (!out) return RT_ERR_INVALID_ARGUMENT;
    const SahLayout L = sah_layout(num_triangles);
    out->p_aabb = L.header;          // SahHeader starts with gp[6], gc[6]
    out->c_aabb = L.header + 24;
    out->status = L.status;
    out->num_leaves = L.status + 4;
    out->cell_counts = L.cell_counts;
    out->total = L.total;
    return RT_OK;
}

int rt_run_sah_build(const rt_build_input* input, const rt_arguments* args, void* stream)
{
    if (!input || !input->nodes_out || !input->scratch) return RT_ERR_INVALID_ARGUMENT;
    const uint32_t n = input->num_triangles;
    if (n && (!input->triangles_in || !input->triangles_out)) return RT_ERR_INVALID_ARGUMENT;
    const bool splits = args && args->enable_splits;
    if (n > (splits ? (1u << 25) : (1u << 28) - 64)) return RT_ERR_TOO_LARGE;   // splits: the 32-bit budget prefix sums 63 per leaf
    if ((reinterpret_cast<uintptr_t>(input->scratch) & 255u) || (reinterpret_cast<uintptr_t>(input->triangles_in) & 15u) ||
        (reinterpret_cast<uintptr_t>(input->triangles_out) & 63u) || (reinterpret_cast<uintptr_t>(input->nodes_out) & 63u))
        return RT_ERR_INVALID_ARGUMENT;
    // asynchronous, like the bottom-up build: the error flags stay in the scratch status word (rt_sah_scratch_layout.status)
    return hip_rc(launch_sah_build(input->triangles_in, n, args && args->enable_pairs, splits, input->triangles_out,
                                   input->nodes_out, input->scratch, static_cast<hipStream_t>(stream), nullptr, nullptr));
}

static int trace_common(const rt_accel* as, const rt_scene* scene, uint64_t* counters, int render_type, uint8_t* rgba8,
                        uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, uint32_t spp, uint32_t strip_rows,
                        uint32_t strip_first, uint32_t strip_stride, void* stream)
{
    if (!as || !scene || !rgba8 || !as->nodes || !scene->camera) return RT_ERR_INVALID_ARGUMENT;
    if (w == 0 || h == 0 || y0 > y1 || y1 > h || as->count > 7) return RT_ERR_INVALID_ARGUMENT;
    if (spp == 0) spp = 1;
    if (spp != 1 && spp != 4 && spp != 16) return RT_ERR_INVALID_ARGUMENT;
    switch (render_type) {
    case RT_RENDER_DEPTH: case RT_RENDER_BOXTESTS: case RT_RENDER_TRIANGLE_TESTS: break;
#ifdef RT_TRACE_TUNING
    case 100: break;   // tuning build only: raw box-test count per pixel
#endif
    case RT_RENDER_MATERIAL_ID: case RT_RENDER_DIFFUSE:
        if (!scene->attributes || !scene->materials || scene->num_materials == 0) return RT_ERR_INVALID_ARGUMENT;
        break;
    case RT_RENDER_LODS: case RT_RENDER_TEXTURE: case RT_RENDER_TEXTURE_LIT: case RT_RENDER_TEXTURE_LIT_SHADOWS:
        if (!scene->attributes || !scene->materials || scene->num_materials == 0) return RT_ERR_INVALID_ARGUMENT;
        if (scene->num_textures && !scene->textures) return RT_ERR_INVALID_ARGUMENT;
        break;
    default: return RT_ERR_INVALID_ARGUMENT;
    }
    TraceLaunch t;
    t.as = *as;
    t.scene = *scene;
    t.counters = counters;
    t.render_type = render_type;
    t.rgba8 = rgba8;
    t.w = w; t.h = h; t.y0 = y0; t.y1 = y1; t.spp = spp;
    t.strip_rows = strip_rows; t.strip_first = strip_first; t.strip_stride = strip_stride;
    return hip_rc(launch_trace(t, static_cast<hipStream_t>(stream)));
}

int rt_trace(const rt_accel* as, const rt_scene* scene, uint64_t* counters, int render_type, uint8_t* rgba8,
             uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, uint32_t spp, void* stream)
{
    return trace_common(as, scene, counters, render_type, rgba8, w, h, y0, y1, spp, 0, 0, 1, stream);
}

int rt_trace_strips(const rt_accel* as, const rt_scene* scene, uint64_t* counters, int render_type, uint8_t* rgba8_compact,
                    uint32_t w, uint32_t h, uint32_t strip_rows, uint32_t first_strip, uint32_t strip_stride,
                    uint32_t spp, void* stream)
{
    if (strip_rows == 0 || (strip_rows & 7u) || strip_stride == 0) return RT_ERR_INVALID_ARGUMENT;
    return trace_common(as, scene, counters, render_type, rgba8_compact, w, h, 0, h, spp, strip_rows, first_strip,
                        strip_stride, stream);
}

static inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// a tree a query can walk: count = 0 is an empty tree, nothing is read through it
static inline bool tree_args(const rt_accel* as) { return as && as->count <= 7 && (!as->count || (as->nodes && as->triangles)); }

static_assert(sizeof(rt_ray_filter) == 8 && sizeof(rt_hit_filter) == 32, "rt_abi.h: the filter records' sizes");

// the filter's own checks; no filter (the unfiltered entry points, a null pointer at the filtered ones) passes
static inline bool filter_args(const rt_hit_filter* f)
{
    return !f || (!(f->flags & ~(uint32_t)(RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT)) && !misaligned(f->prim_masks, 4) &&
                  !misaligned(f->per_ray, 8));
}

// An unfiltered ray query is its filtered entry point with no filter: one set of checks, and a null filter launches the
// unfiltered kernel.
int rt_intersect_rays_filtered(const rt_accel* as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, int mode,
                               uint32_t num_primitives, const rt_hit_filter* filter, uint64_t* counters, void* stream)
{
    if (!tree_args(as) || !rays || !hits || !filter_args(filter)) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16)) return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0) return RT_OK;
    return hip_rc(launch_ray_query(*as, rays, hits, num_rays, mode == RT_RAY_ANY_HIT, num_primitives, filter, counters,
                                   static_cast<hipStream_t>(stream)));
}

int rt_intersect_rays(const rt_accel* as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, int mode,
                      uint32_t num_primitives, uint64_t* counters, void* stream)
{
    return rt_intersect_rays_filtered(as, rays, hits, num_rays, mode, num_primitives, nullptr, counters, stream);
}

int rt_intersect_rays_indexed(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, const uint32_t* order,
                              uint32_t num_indices, rt_hit* hits, int mode, uint32_t num_primitives, uint64_t* counters,
                              void* stream)
{
    if (!tree_args(as) || !rays || !hits || !order) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(order, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (num_indices == 0) return RT_OK;
    return hip_rc(launch_ray_query_indexed(*as, rays, num_rays, order, num_indices, hits, mode == RT_RAY_ANY_HIT,
                                           num_primitives, counters, static_cast<hipStream_t>(stream)));
}

size_t rt_ray_sort_scratch_bytes(uint32_t num_rays) { return ray_sort_layout(num_rays).total; }

int rt_ray_sort_layout_get(uint32_t num_rays, rt_ray_sort_layout* out)
{
    if (!out) return RT_ERR_INVALID_ARGUMENT;
    const RaySortLayout L = ray_sort_layout(num_rays);
    out->box = L.box;
    out->num_live = L.num_live;
    out->keys = L.keys;
    out->tmp_keys = L.tmp_keys;
    out->tmp_values = L.tmp_values;
    out->sort = L.sort;
    out->total = L.total;
    return RT_OK;
}

int rt_sort_rays(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, uint32_t* order, void* scratch, void* stream)
{
    if (!as || !rays || !order || !scratch || as->count > 7) return RT_ERR_INVALID_ARGUMENT;
    if (as->count && !as->nodes) return RT_ERR_INVALID_ARGUMENT;   // (the root run's boxes are all the call reads)
    if (misaligned(rays, 16) || misaligned(order, 4) || misaligned(scratch, 256)) return RT_ERR_INVALID_ARGUMENT;
    if (num_rays > kSortMaxCount) return RT_ERR_TOO_LARGE;
    if (num_rays == 0) return RT_OK;
    return hip_rc(launch_sort_rays(*as, rays, num_rays, order, scratch, static_cast<hipStream_t>(stream)));
}

int rt_generate_camera_rays(const rt_camera* camera, uint32_t w, uint32_t h, uint32_t spp, int layout, rt_ray* rays,
                            void* stream)
{
    if (!camera || !rays || (reinterpret_cast<uintptr_t>(rays) & 15u)) return RT_ERR_INVALID_ARGUMENT;
    if (layout != RT_RAYS_ROW_MAJOR && layout != RT_RAYS_TILED) return RT_ERR_INVALID_ARGUMENT;
    if (spp != 1 && spp != 4 && spp != 16) return RT_ERR_INVALID_ARGUMENT;
    if (w == 0 || h == 0) return RT_OK;
    return hip_rc(launch_camera_rays(camera, w, h, spp, layout == RT_RAYS_TILED, rays, static_cast<hipStream_t>(stream)));
}

size_t rt_refit_plan_bytes(uint32_t num_triangles) { return refit_layout(num_triangles).total; }

int rt_refit_plan_layout_get(uint32_t num_triangles, rt_refit_plan_layout* out)
{
    if (!out) return RT_ERR_INVALID_ARGUMENT;
    const RefitLayout L = refit_layout(num_triangles);
    out->status = L.status;
    out->parents = L.parents;
    out->arrivals = L.arrive;
    out->leaves = L.list;
    out->total = L.total;
    return RT_OK;
}

// the checks both refit entry points share; 1 = valid and there is work, 0 = valid and n = 0, < 0 = an RT_ERR_*
static int refit_args(const rt_build_input* input, uint32_t count, const void* plan, bool need_positions)
{
    if (!input || !plan || count > 7) return RT_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(plan) & 255u) return RT_ERR_INVALID_ARGUMENT;
    const uint32_t n = input->num_triangles;
    if (n > RT_REFIT_MAX_TRIANGLES) return RT_ERR_TOO_LARGE;
    if (n == 0) return 0;
    if (!input->nodes_out || !input->triangles_out || (need_positions && !input->triangles_in)) return RT_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(input->triangles_in) & 15u) || (reinterpret_cast<uintptr_t>(input->triangles_out) & 63u) ||
        (reinterpret_cast<uintptr_t>(input->nodes_out) & 63u))
        return RT_ERR_INVALID_ARGUMENT;
    return 1;
}

int rt_build_refit_plan(const rt_build_input* input, uint32_t root, uint32_t count, void* plan, void* stream)
{
    const int rc = refit_args(input, count, plan, false);
    if (rc <= 0) return rc;
    return hip_rc(launch_refit_plan(*input, root, count, plan, static_cast<hipStream_t>(stream)));
}

int rt_refit(const rt_build_input* input, uint32_t root, uint32_t count, void* plan, void* stream)
{
    const int rc = refit_args(input, count, plan, true);
    if (rc <= 0) return rc;
    return hip_rc(launch_refit(*input, root, count, plan, static_cast<hipStream_t>(stream)));
}

static_assert(sizeof(rt_motion_accel) == 40 && offsetof(rt_motion_accel, root) == 32, "rt_abi.h: rt_motion_accel's layout");

// two poses a motion query can walk: count = 0 is an empty tree, nothing is read through it
static inline bool motion_tree_args(const rt_motion_accel* as)
{
    return as && as->count <= 7 && (!as->count || (as->nodes0 && as->triangles0 && as->nodes1 && as->triangles1));
}

int rt_motion_validate(const rt_motion_accel* as, uint32_t num_triangles, uint32_t* status, void* stream)
{
    if (!motion_tree_args(as) || !status || misaligned(status, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (as->count && (misaligned(as->nodes0, 16) || misaligned(as->nodes1, 16) || misaligned(as->triangles0, 16) ||
                      misaligned(as->triangles1, 16)))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_triangles > RT_REFIT_MAX_TRIANGLES) return RT_ERR_TOO_LARGE;
    return hip_rc(launch_motion_validate(*as, num_triangles, status, static_cast<hipStream_t>(stream)));
}

// The indexed form of a ray query is its sibling with an index list: one set of checks per family, `indexed` adds the
// list's own (non-null, 4-byte aligned) and an empty list is an empty call.  A launch function given no list runs the
// sibling's instantiation of its kernel.
static inline bool order_args(bool indexed, const uint32_t* order) { return !indexed || (order && !misaligned(order, 4)); }

static int motion_query(const rt_motion_accel* as, const rt_ray* rays, const float* times, rt_hit* hits, uint32_t num_rays,
                        bool indexed, const uint32_t* order, uint32_t num_indices, int mode, uint64_t* counters, void* stream)
{
    if (!motion_tree_args(as) || !rays || !times || !hits || !order_args(indexed, order)) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(times, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0 || (indexed && num_indices == 0)) return RT_OK;
    return hip_rc(launch_motion_query(*as, rays, times, hits, num_rays, indexed ? order : nullptr, num_indices,
                                      mode == RT_RAY_ANY_HIT, counters, static_cast<hipStream_t>(stream)));
}

int rt_intersect_rays_motion(const rt_motion_accel* as, const rt_ray* rays, const float* times, rt_hit* hits, uint32_t num_rays,
                             int mode, uint64_t* counters, void* stream)
{
    return motion_query(as, rays, times, hits, num_rays, false, nullptr, 0, mode, counters, stream);
}

int rt_intersect_rays_motion_indexed(const rt_motion_accel* as, const rt_ray* rays, const float* times, uint32_t num_rays,
                                     const uint32_t* order, uint32_t num_indices, rt_hit* hits, int mode, uint64_t* counters,
                                     void* stream)
{
    return motion_query(as, rays, times, hits, num_rays, true, order, num_indices, mode, counters, stream);
}

int rt_prepare_instances(const rt_instance* instances, uint32_t num_instances, const rt_accel* blas_table, uint32_t num_blas,
                         rt_triangle* proxies, rt_instance_record* records, uint32_t* status, void* stream)
{
    if (!status || misaligned(status, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (num_instances) {
        if (!instances || !proxies || !records || !blas_table || num_blas == 0) return RT_ERR_INVALID_ARGUMENT;
        if (misaligned(instances, 16) || misaligned(proxies, 16) || misaligned(records, 16) || misaligned(blas_table, 8))
            return RT_ERR_INVALID_ARGUMENT;
    }
    return hip_rc(launch_prepare_instances(instances, num_instances, blas_table, num_blas, proxies, records, status,
                                           static_cast<hipStream_t>(stream)));
}

static_assert(sizeof(rt_instance_filter) == 8 && sizeof(rt_instance_ray_filter) == 16 && sizeof(rt_instance_hit_filter) == 32,
              "rt_abi.h: the instance filter records' sizes");

static int instanced_query(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                           const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, rt_hit* hits,
                           uint32_t* instance_ids, uint32_t num_rays, bool indexed, const uint32_t* order, uint32_t num_indices,
                           int mode, uint32_t num_primitives, const rt_instance_hit_filter* filter, uint64_t* counters,
                           void* stream)
{
    if (!tree_args(tlas) || !rays || !hits || !instance_ids || !order_args(indexed, order)) return RT_ERR_INVALID_ARGUMENT;
    if (num_instances && (!records || !blas_table || num_blas == 0)) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(instance_ids, 4) || misaligned(records, 16) ||
        misaligned(blas_table, 8))
        return RT_ERR_INVALID_ARGUMENT;
    // the filter's own checks (none: the unfiltered kernel)
    if (filter && ((filter->flags & ~(uint32_t)(RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT)) ||
                   misaligned(filter->per_instance, 8) || misaligned(filter->per_ray, 16)))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0 || (indexed && num_indices == 0)) return RT_OK;
    InstanceQuery q;
    q.tlas = *tlas;
    q.records = records;
    q.num_instances = num_instances;
    q.blas_table = blas_table;
    q.num_blas = num_blas;
    q.rays = rays;
    q.hits = hits;
    q.instance_ids = instance_ids;
    q.num_rays = num_rays;
    q.any_hit = mode == RT_RAY_ANY_HIT;
    q.num_primitives = num_primitives;
    q.counters = counters;
    q.order = indexed ? order : nullptr;
    q.num_indices = num_indices;
    return hip_rc(launch_instance_query(q, filter, static_cast<hipStream_t>(stream)));
}

int rt_intersect_rays_instanced_filtered(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                         const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, rt_hit* hits,
                                         uint32_t* instance_ids, uint32_t num_rays, int mode, uint32_t num_primitives,
                                         const rt_instance_hit_filter* filter, uint64_t* counters, void* stream)
{
    return instanced_query(tlas, records, num_instances, blas_table, num_blas, rays, hits, instance_ids, num_rays, false, nullptr,
                           0, mode, num_primitives, filter, counters, stream);
}

int rt_intersect_rays_instanced_indexed(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                        const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                        const uint32_t* order, uint32_t num_indices, rt_hit* hits, uint32_t* instance_ids,
                                        int mode, uint32_t num_primitives, const rt_instance_hit_filter* filter,
                                        uint64_t* counters, void* stream)
{
    return instanced_query(tlas, records, num_instances, blas_table, num_blas, rays, hits, instance_ids, num_rays, true, order,
                           num_indices, mode, num_primitives, filter, counters, stream);
}

int rt_intersect_rays_instanced(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, rt_hit* hits,
                                uint32_t* instance_ids, uint32_t num_rays, int mode, uint32_t num_primitives,
                                uint64_t* counters, void* stream)
{
    return rt_intersect_rays_instanced_filtered(tlas, records, num_instances, blas_table, num_blas, rays, hits, instance_ids,
                                                num_rays, mode, num_primitives, nullptr, counters, stream);
}

int rt_prepare_motion_instances(const rt_motion_instance* instances, uint32_t num_instances, const rt_accel* blas_table,
                                uint32_t num_blas, rt_triangle* proxies0, rt_triangle* proxies1,
                                rt_motion_instance_record* records, uint32_t* status, void* stream)
{
    if (!status || misaligned(status, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (num_instances) {
        if (!instances || !proxies0 || !proxies1 || !records || !blas_table || num_blas == 0) return RT_ERR_INVALID_ARGUMENT;
        if (misaligned(instances, 16) || misaligned(proxies0, 16) || misaligned(proxies1, 16) || misaligned(records, 16) ||
            misaligned(blas_table, 8))
            return RT_ERR_INVALID_ARGUMENT;
    }
    return hip_rc(launch_prepare_motion_instances(instances, num_instances, blas_table, num_blas, proxies0, proxies1, records,
                                                  status, static_cast<hipStream_t>(stream)));
}

static int instanced_motion_query(const rt_motion_accel* tlas, const rt_motion_instance_record* records, uint32_t num_instances,
                                  const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, const float* times,
                                  rt_hit* hits, uint32_t* instance_ids, uint32_t num_rays, bool indexed, const uint32_t* order,
                                  uint32_t num_indices, int mode, uint64_t* counters, void* stream)
{
    if (!motion_tree_args(tlas) || !rays || !times || !hits || !instance_ids || !order_args(indexed, order))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_instances && (!records || !blas_table || num_blas == 0)) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(times, 4) || misaligned(instance_ids, 4) ||
        misaligned(records, 16) || misaligned(blas_table, 8))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0 || (indexed && num_indices == 0)) return RT_OK;
    return hip_rc(launch_instance_motion_query(*tlas, records, num_instances, blas_table, num_blas, rays, times, hits,
                                               instance_ids, num_rays, indexed ? order : nullptr, num_indices,
                                               mode == RT_RAY_ANY_HIT, counters, static_cast<hipStream_t>(stream)));
}

int rt_intersect_rays_instanced_motion(const rt_motion_accel* tlas, const rt_motion_instance_record* records,
                                       uint32_t num_instances, const rt_accel* blas_table, uint32_t num_blas,
                                       const rt_ray* rays, const float* times, rt_hit* hits, uint32_t* instance_ids,
                                       uint32_t num_rays, int mode, uint64_t* counters, void* stream)
{
    return instanced_motion_query(tlas, records, num_instances, blas_table, num_blas, rays, times, hits, instance_ids, num_rays,
                                  false, nullptr, 0, mode, counters, stream);
}

int rt_intersect_rays_instanced_motion_indexed(const rt_motion_accel* tlas, const rt_motion_instance_record* records,
                                               uint32_t num_instances, const rt_accel* blas_table, uint32_t num_blas,
                                               const rt_ray* rays, const float* times, uint32_t num_rays, const uint32_t* order,
                                               uint32_t num_indices, rt_hit* hits, uint32_t* instance_ids, int mode,
                                               uint64_t* counters, void* stream)
{
    return instanced_motion_query(tlas, records, num_instances, blas_table, num_blas, rays, times, hits, instance_ids, num_rays,
                                  true, order, num_indices, mode, counters, stream);
}

static_assert(sizeof(rt_sphere) == 16, "rt_abi.h: rt_sphere is one 16-byte record");

int rt_prepare_spheres(const rt_sphere* spheres, uint32_t num_spheres, rt_triangle* proxies, uint32_t* status, void* stream)
{
    if (!status || misaligned(status, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(spheres, 16) || misaligned(proxies, 16)) return RT_ERR_INVALID_ARGUMENT;
    if (num_spheres && (!spheres || !proxies)) return RT_ERR_INVALID_ARGUMENT;
    return hip_rc(launch_prepare_spheres(spheres, num_spheres, proxies, status, static_cast<hipStream_t>(stream)));
}

int rt_intersect_rays_spheres(const rt_accel* as, const rt_sphere* spheres, uint32_t num_spheres, const rt_ray* rays,
                              uint32_t num_rays, const uint32_t* order, uint32_t num_indices, rt_hit* hits, int mode,
                              uint64_t* counters, void* stream)
{
    if (!tree_args(as)) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(spheres, 16) || misaligned(rays, 16) || misaligned(hits, 16) || misaligned(order, 4))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_spheres && !spheres) return RT_ERR_INVALID_ARGUMENT;
    if (num_rays && (!rays || !hits)) return RT_ERR_INVALID_ARGUMENT;
    // nothing to launch: no ray, or an index list without an entry
    if (num_rays == 0 || (order && num_indices == 0)) return RT_OK;
    return hip_rc(launch_sphere_query(*as, spheres, num_spheres, rays, num_rays, order, num_indices, hits,
                                      mode == RT_RAY_ANY_HIT, counters, static_cast<hipStream_t>(stream)));
}

static_assert(sizeof(rt_capsule) == 32, "rt_abi.h: rt_capsule is one 32-byte record");

int rt_prepare_capsules(const rt_capsule* capsules, uint32_t num_capsules, rt_triangle* proxies, uint32_t* status, void* stream)
{
    if (!status || misaligned(status, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(capsules, 16) || misaligned(proxies, 16)) return RT_ERR_INVALID_ARGUMENT;
    if (num_capsules && (!capsules || !proxies)) return RT_ERR_INVALID_ARGUMENT;
    return hip_rc(launch_prepare_capsules(capsules, num_capsules, proxies, status, static_cast<hipStream_t>(stream)));
}

int rt_intersect_rays_capsules(const rt_accel* as, const rt_capsule* capsules, uint32_t num_capsules, const rt_ray* rays,
                               uint32_t num_rays, const uint32_t* order, uint32_t num_indices, rt_hit* hits, int mode,
                               uint64_t* counters, void* stream)
{
    if (!tree_args(as)) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(capsules, 16) || misaligned(rays, 16) || misaligned(hits, 16) || misaligned(order, 4))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_capsules && !capsules) return RT_ERR_INVALID_ARGUMENT;
    if (num_rays && (!rays || !hits)) return RT_ERR_INVALID_ARGUMENT;
    // nothing to launch: no ray, or an index list without an entry
    if (num_rays == 0 || (order && num_indices == 0)) return RT_OK;
    return hip_rc(launch_capsule_query(*as, capsules, num_capsules, rays, num_rays, order, num_indices, hits,
                                       mode == RT_RAY_ANY_HIT, counters, static_cast<hipStream_t>(stream)));
}

int rt_sphere_cast(const rt_accel* as, const rt_ray* rays, const float* radii, float radius, uint32_t num_rays,
                   const uint32_t* order, uint32_t num_indices, rt_hit* hits, uint32_t* features, int mode, uint64_t* counters,
                   void* stream)
{
    if (!tree_args(as)) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(order, 4) || misaligned(radii, 4) || misaligned(features, 4))
        return RT_ERR_INVALID_ARGUMENT;
    // the one radius of a call without radii: finite and not negative (a NaN fails the first compare)
    if (!radii && (!(radius >= 0.0f) || radius == __builtin_inff())) return RT_ERR_INVALID_ARGUMENT;
    if (num_rays && (!rays || !hits)) return RT_ERR_INVALID_ARGUMENT;
    // nothing to launch: no ray, or an index list without an entry
    if (num_rays == 0 || (order && num_indices == 0)) return RT_OK;
    return hip_rc(launch_sphere_cast(*as, rays, radii, radius, num_rays, order, num_indices, hits, features,
                                     mode == RT_RAY_ANY_HIT, counters, static_cast<hipStream_t>(stream)));
}

static_assert(sizeof(rt_geometry) == 16, "rt_abi.h: rt_geometry is one 16-byte record");

static int instanced_mixed_query(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                 const rt_accel* blas_table, const rt_geometry* geom_table, uint32_t num_blas,
                                 const rt_ray* rays, rt_hit* hits, uint32_t* instance_ids, uint32_t num_rays, bool indexed,
                                 const uint32_t* order, uint32_t num_indices, int mode, uint64_t* counters, void* stream,
                                 bool capsules = false)
{
    // no table: every BLAS holds triangles (the sibling, without the pair-prefetch arm); the capsule call has no such shortcut
    if (!geom_table && capsules) return RT_ERR_INVALID_ARGUMENT;
    if (!geom_table)
        return instanced_query(tlas, records, num_instances, blas_table, num_blas, rays, hits, instance_ids, num_rays, indexed,
                               order, num_indices, mode, 0u, nullptr, counters, stream);
    if (!tree_args(tlas) || !rays || !hits || !instance_ids || !order_args(indexed, order)) return RT_ERR_INVALID_ARGUMENT;
    if (num_instances && (!records || !blas_table || num_blas == 0)) return RT_ERR_INVALID_ARGUMENT;
    if (mode != RT_RAY_CLOSEST_HIT && mode != RT_RAY_ANY_HIT) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(instance_ids, 4) || misaligned(records, 16) ||
        misaligned(blas_table, 8) || misaligned(geom_table, 16))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0 || (indexed && num_indices == 0)) return RT_OK;
    InstanceQuery q;
    q.tlas = *tlas;
    q.records = records;
    q.num_instances = num_instances;
    q.blas_table = blas_table;
    q.num_blas = num_blas;
    q.rays = rays;
    q.hits = hits;
    q.instance_ids = instance_ids;
    q.num_rays = num_rays;
    q.any_hit = mode == RT_RAY_ANY_HIT;
    q.num_primitives = 0;
    q.counters = counters;
    q.order = indexed ? order : nullptr;
    q.num_indices = num_indices;
    return hip_rc(launch_instance_mixed_query(q, geom_table, capsules, static_cast<hipStream_t>(stream)));
}

int rt_intersect_rays_instanced_mixed(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                      const rt_accel* blas_table, const rt_geometry* geom_table, uint32_t num_blas,
                                      const rt_ray* rays, rt_hit* hits, uint32_t* instance_ids, uint32_t num_rays, int mode,
                                      uint64_t* counters, void* stream)
{
    return instanced_mixed_query(tlas, records, num_instances, blas_table, geom_table, num_blas, rays, hits, instance_ids,
                                 num_rays, false, nullptr, 0, mode, counters, stream);
}

int rt_intersect_rays_instanced_mixed_indexed(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                              const rt_accel* blas_table, const rt_geometry* geom_table, uint32_t num_blas,
                                              const rt_ray* rays, uint32_t num_rays, const uint32_t* order, uint32_t num_indices,
                                              rt_hit* hits, uint32_t* instance_ids, int mode, uint64_t* counters, void* stream)
{
    return instanced_mixed_query(tlas, records, num_instances, blas_table, geom_table, num_blas, rays, hits, instance_ids,
                                 num_rays, true, order, num_indices, mode, counters, stream);
}

int rt_intersect_rays_instanced_mixed_capsules(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                               const rt_accel* blas_table, const rt_geometry* geom_table, uint32_t num_blas,
                                               const rt_ray* rays, uint32_t num_rays, const uint32_t* order, uint32_t num_indices,
                                               rt_hit* hits, uint32_t* instance_ids, int mode, uint64_t* counters, void* stream)
{
    // a null order is the direct form, as in rt_intersect_rays_capsules
    return instanced_mixed_query(tlas, records, num_instances, blas_table, geom_table, num_blas, rays, hits, instance_ids,
                                 num_rays, order != nullptr, order, num_indices, mode, counters, stream, true);
}

int rt_closest_points(const rt_accel* as, const rt_point_query* queries, rt_point_hit* hits, uint32_t num_queries,
                      uint64_t* counters, uint32_t* status, void* stream)
{
    if (!tree_args(as) || !queries || !hits) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(queries, 16) || misaligned(hits, 16) || misaligned(status, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (num_queries == 0) return RT_OK;
    return hip_rc(launch_point_query(*as, queries, hits, num_queries, counters, status, static_cast<hipStream_t>(stream)));
}

size_t rt_range_scratch_bytes(uint32_t num_queries) { return range_scratch_bytes(num_queries); }

// the checks the CSR entry points share (every failure is RT_ERR_INVALID_ARGUMENT, so their order cannot be observed).
// extra_ok: the family's own test (the range shape, the overlap flags); query_align: of its query records
static bool csr_args(const rt_accel* as, const void* queries, uintptr_t query_align, bool extra_ok, const uint64_t* offsets,
                     const uint32_t* status)
{
    return tree_args(as) && queries && offsets && extra_ok && !misaligned(queries, query_align) && !misaligned(offsets, 8) &&
           !misaligned(status, 4);
}
// ... the count side: the scratch of rt_*_scratch_bytes
static bool csr_count_args(const void* scratch) { return scratch && !misaligned(scratch, 256); }
// ... the collect side: rows of row_align bytes, the optional true counts
static bool csr_collect_args(const void* rows, uintptr_t row_align, const uint32_t* counts)
{
    return rows && !misaligned(rows, row_align) && !misaligned(counts, 4);
}

int rt_range_count(const rt_accel* as, const void* queries, uint32_t num_queries, int shape, uint64_t* offsets, void* scratch,
                   uint64_t* counters, uint32_t* status, void* stream)
{
    const bool shape_ok = shape == RT_RANGE_SPHERE || shape == RT_RANGE_BOX;
    if (!csr_args(as, queries, 16, shape_ok, offsets, status) || !csr_count_args(scratch)) return RT_ERR_INVALID_ARGUMENT;
    // (num_queries = 0 still launches the scan's one workgroup: offsets[0] = 0)
    return hip_rc(launch_range_count(*as, queries, num_queries, shape, offsets, scratch, counters, status,
                                     static_cast<hipStream_t>(stream)));
}

int rt_range_collect(const rt_accel* as, const void* queries, uint32_t num_queries, int shape, const uint64_t* offsets,
                     uint32_t* ids, uint32_t* counts, uint64_t* counters, uint32_t* status, void* stream)
{
    const bool shape_ok = shape == RT_RANGE_SPHERE || shape == RT_RANGE_BOX;
    if (!csr_args(as, queries, 16, shape_ok, offsets, status) || !csr_collect_args(ids, 4, counts)) return RT_ERR_INVALID_ARGUMENT;
    if (num_queries == 0) return RT_OK;
    return hip_rc(launch_range_collect(*as, queries, num_queries, shape, offsets, ids, counts, counters, status,
                                       static_cast<hipStream_t>(stream)));
}

int rt_k_nearest(const rt_accel* as, const rt_point_query* queries, uint32_t num_queries, uint32_t k, rt_knn_hit* out,
                 uint64_t* counters, uint32_t* status, void* stream)
{
    if (!tree_args(as) || !queries || !out) return RT_ERR_INVALID_ARGUMENT;
    if (k == 0 || k > RT_KNN_MAX_K) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(queries, 16) || misaligned(out, 8) || misaligned(status, 4)) return RT_ERR_INVALID_ARGUMENT;
    if (num_queries == 0) return RT_OK;
    return hip_rc(launch_knn_query(*as, queries, num_queries, k, out, counters, status, static_cast<hipStream_t>(stream)));
}

size_t rt_ray_hits_scratch_bytes(uint32_t num_rays) { return ray_hits_scratch_bytes(num_rays); }

int rt_ray_hits_count_filtered(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                               uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, void* stream)
{
    if (!csr_args(as, rays, 16, filter_args(filter), offsets, status) || !csr_count_args(scratch)) return RT_ERR_INVALID_ARGUMENT;
    // (num_rays = 0 still launches the scan's one workgroup: offsets[0] = 0)
    return hip_rc(launch_ray_hits_count(*as, rays, num_rays, filter, offsets, scratch, counters, status,
                                        static_cast<hipStream_t>(stream)));
}

int rt_ray_hits_count(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, uint64_t* offsets, void* scratch,
                      uint64_t* counters, uint32_t* status, void* stream)
{
    return rt_ray_hits_count_filtered(as, rays, num_rays, nullptr, offsets, scratch, counters, status, stream);
}

int rt_ray_hits_collect_filtered(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                                 const uint64_t* offsets, rt_hit* hits, uint32_t* counts, uint64_t* counters, uint32_t* status,
                                 void* stream)
{
    if (!csr_args(as, rays, 16, filter_args(filter), offsets, status) || !csr_collect_args(hits, 16, counts))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0) return RT_OK;
    return hip_rc(launch_ray_hits_collect(*as, rays, num_rays, filter, offsets, hits, counts, counters, status,
                                          static_cast<hipStream_t>(stream)));
}

int rt_ray_hits_collect(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, const uint64_t* offsets, rt_hit* hits,
                        uint32_t* counts, uint64_t* counters, uint32_t* status, void* stream)
{
    return rt_ray_hits_collect_filtered(as, rays, num_rays, nullptr, offsets, hits, counts, counters, status, stream);
}

// what rt_ray_hits_count_instanced and rt_ray_hits_collect_instanced check alike: the instancing block's arguments and the CSR
// block's; on success `q` holds what both launches read
static bool hits_instanced_args(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                const uint64_t* offsets, uint64_t* counters, const uint32_t* status, InstanceQuery& q)
{
    if (!csr_args(tlas, rays, 16, true, offsets, status)) return false;
    if (num_instances && (!records || !blas_table || num_blas == 0)) return false;
    if (misaligned(records, 16) || misaligned(blas_table, 8)) return false;
    q = InstanceQuery();
    q.tlas = *tlas;
    q.records = records;
    q.num_instances = num_instances;
    q.blas_table = blas_table;
    q.num_blas = num_blas;
    q.rays = rays;
    q.num_rays = num_rays;
    q.counters = counters;
    return true;
}

// the instance filter's own checks (none: the unfiltered kernel), as rt_intersect_rays_instanced_filtered makes them
static inline bool instance_filter_args(const rt_instance_hit_filter* f)
{
    return !f || !((f->flags & ~(uint32_t)(RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT)) || misaligned(f->per_instance, 8) ||
                   misaligned(f->per_ray, 16));
}

int rt_ray_hits_count_instanced_filtered(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                         const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                         const rt_instance_hit_filter* filter, uint64_t* offsets, void* scratch,
                                         uint64_t* counters, uint32_t* status, void* stream)
{
    InstanceQuery q;
    if (!hits_instanced_args(tlas, records, num_instances, blas_table, num_blas, rays, num_rays, offsets, counters, status, q) ||
        !csr_count_args(scratch) || !instance_filter_args(filter))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0) return RT_OK;
    return hip_rc(launch_ray_hits_count_instanced(q, filter, offsets, scratch, status, static_cast<hipStream_t>(stream)));
}

int rt_ray_hits_count_instanced(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, void* stream)
{
    return rt_ray_hits_count_instanced_filtered(tlas, records, num_instances, blas_table, num_blas, rays, num_rays, nullptr,
                                                offsets, scratch, counters, status, stream);
}

int rt_ray_hits_collect_instanced_filtered(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                           const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays,
                                           uint32_t num_rays, const rt_instance_hit_filter* filter, const uint64_t* offsets,
                                           rt_hit* hits, uint32_t* instance_ids, uint32_t* counts, uint64_t* counters,
                                           uint32_t* status, void* stream)
{
    InstanceQuery q;
    if (!hits_instanced_args(tlas, records, num_instances, blas_table, num_blas, rays, num_rays, offsets, counters, status, q) ||
        !csr_collect_args(hits, 16, counts) || !instance_ids || misaligned(instance_ids, 4) || !instance_filter_args(filter))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0) return RT_OK;
    q.hits = hits;
    q.instance_ids = instance_ids;
    return hip_rc(launch_ray_hits_collect_instanced(q, filter, offsets, counts, status, static_cast<hipStream_t>(stream)));
}

int rt_ray_hits_collect_instanced(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                  const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                  const uint64_t* offsets, rt_hit* hits, uint32_t* instance_ids, uint32_t* counts,
                                  uint64_t* counters, uint32_t* status, void* stream)
{
    return rt_ray_hits_collect_instanced_filtered(tlas, records, num_instances, blas_table, num_blas, rays, num_rays, nullptr,
                                                  offsets, hits, instance_ids, counts, counters, status, stream);
}

int rt_ray_first_hits_filtered(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, uint32_t k,
                               const rt_hit_filter* filter, rt_hit* out, uint64_t* counters, uint32_t* status, void* stream)
{
    if (!tree_args(as) || !rays || !out || !filter_args(filter)) return RT_ERR_INVALID_ARGUMENT;
    if (k == 0 || k > RT_RAY_FIRST_MAX_K) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(out, 16) || misaligned(status, 4) || misaligned(counters, 8))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0) return RT_OK;
    return hip_rc(launch_ray_first_hits(*as, rays, num_rays, k, filter, out, counters, status, static_cast<hipStream_t>(stream)));
}

int rt_ray_first_hits(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, uint32_t k, rt_hit* out, uint64_t* counters,
                      uint32_t* status, void* stream)
{
    return rt_ray_first_hits_filtered(as, rays, num_rays, k, nullptr, out, counters, status, stream);
}

int rt_ray_first_hits_instanced_filtered(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                         const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                         uint32_t k, const rt_instance_hit_filter* filter, rt_hit* hits, uint32_t* instance_ids,
                                         uint64_t* counters, uint32_t* status, void* stream)
{
    if (!tree_args(tlas) || !rays || !hits || !instance_ids || !instance_filter_args(filter)) return RT_ERR_INVALID_ARGUMENT;
    if (num_instances && (!records || !blas_table || num_blas == 0)) return RT_ERR_INVALID_ARGUMENT;
    if (k == 0 || k > RT_RAY_FIRST_MAX_K) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(records, 16) || misaligned(blas_table, 8) ||
        misaligned(instance_ids, 4) || misaligned(status, 4) || misaligned(counters, 8))
        return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0) return RT_OK;
    InstanceQuery q = InstanceQuery();
    q.tlas = *tlas;
    q.records = records;
    q.num_instances = num_instances;
    q.blas_table = blas_table;
    q.num_blas = num_blas;
    q.rays = rays;
    q.hits = hits;
    q.instance_ids = instance_ids;
    q.num_rays = num_rays;
    q.counters = counters;
    return hip_rc(launch_ray_first_hits_instanced(q, k, filter, status, static_cast<hipStream_t>(stream)));
}

int rt_ray_first_hits_instanced(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                uint32_t k, rt_hit* hits, uint32_t* instance_ids, uint64_t* counters, uint32_t* status,
                                void* stream)
{
    return rt_ray_first_hits_instanced_filtered(tlas, records, num_instances, blas_table, num_blas, rays, num_rays, k, nullptr,
                                                hits, instance_ids, counters, status, stream);
}

size_t rt_tri_overlaps_scratch_bytes(uint32_t num_queries) { return tri_overlaps_scratch_bytes(num_queries); }

int rt_tri_overlaps_count(const rt_accel* as, const rt_triangle* queries, uint32_t num_queries, uint32_t flags,
                          uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, void* stream)
{
    const bool flags_ok = !(flags & ~(uint32_t)RT_TRI_SELF);
    if (!csr_args(as, queries, 4, flags_ok, offsets, status) || !csr_count_args(scratch)) return RT_ERR_INVALID_ARGUMENT;
    // (num_queries = 0 still launches the scan's one workgroup: offsets[0] = 0)
    return hip_rc(launch_tri_overlaps_count(*as, queries, num_queries, (flags & RT_TRI_SELF) != 0, offsets, scratch, counters,
                                            status, static_cast<hipStream_t>(stream)));
}

int rt_tri_overlaps_collect(const rt_accel* as, const rt_triangle* queries, uint32_t num_queries, uint32_t flags,
                            const uint64_t* offsets, uint32_t* ids, uint32_t* counts, uint64_t* counters, uint32_t* status,
                            void* stream)
{
    const bool flags_ok = !(flags & ~(uint32_t)RT_TRI_SELF);
    if (!csr_args(as, queries, 4, flags_ok, offsets, status) || !csr_collect_args(ids, 4, counts)) return RT_ERR_INVALID_ARGUMENT;
    if (num_queries == 0) return RT_OK;
    return hip_rc(launch_tri_overlaps_collect(*as, queries, num_queries, (flags & RT_TRI_SELF) != 0, offsets, ids, counts,
                                              counters, status, static_cast<hipStream_t>(stream)));
}

// rt_signed_distance / rt_occupancy: the default vote directions of rt_abi.h
static const float kSdfDefaultDirs[3 * RT_SDF_MAX_VOTES] = {0.577f, 0.211f, 0.789f, -0.683f, 0.619f, 0.387f, 0.259f, -0.857f, 0.446f};

static bool sdf_args(const rt_accel* as, const rt_point_query* queries, uint32_t votes, const void* result, uintptr_t result_align,
                     const uint32_t* status)
{
    return tree_args(as) && queries && result && (votes == 1 || votes == RT_SDF_MAX_VOTES) && !misaligned(queries, 16) &&
           !misaligned(result, result_align) && !misaligned(status, 4);
}

int rt_signed_distance(const rt_accel* as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes,
                       const float* dirs, rt_sdf_hit* out, uint64_t* counters, uint32_t* status, void* stream)
{
    if (!sdf_args(as, queries, votes, out, 8, status)) return RT_ERR_INVALID_ARGUMENT;
    if (num_queries == 0) return RT_OK;
    return hip_rc(launch_signed_distance(*as, queries, num_queries, votes, dirs ? dirs : kSdfDefaultDirs, out, counters, status,
                                         static_cast<hipStream_t>(stream)));
}

int rt_occupancy(const rt_accel* as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes,
                 const float* dirs, uint8_t* inside, uint64_t* counters, uint32_t* status, void* stream)
{
    if (!sdf_args(as, queries, votes, inside, 1, status)) return RT_ERR_INVALID_ARGUMENT;
    if (num_queries == 0) return RT_OK;
    return hip_rc(launch_occupancy(*as, queries, num_queries, votes, dirs ? dirs : kSdfDefaultDirs, inside, counters, status,
                                   static_cast<hipStream_t>(stream)));
}

int rt_generate_grid_points(const float origin[3], const float spacing[3], const uint32_t dims[3], float dist2_max,
                            int layout, rt_point_query* queries, void* stream)
{
    if (!origin || !spacing || !dims || !queries || misaligned(queries, 16)) return RT_ERR_INVALID_ARGUMENT;
    if (layout != RT_GRID_ROW_MAJOR && layout != RT_GRID_BRICKS) return RT_ERR_INVALID_ARGUMENT;
    if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return RT_OK;
    // the record count, checked factor by factor: every partial product is below 2^64
    const bool bricks = layout == RT_GRID_BRICKS;
    uint64_t n = bricks ? 64u : 1u;
    for (int a = 0; a < 3; a++) {
        n *= bricks ? ((uint64_t)dims[a] + 3u) / 4u : (uint64_t)dims[a];
        if (n > 0xFFFFFFFFull) return RT_ERR_TOO_LARGE;
    }
    return hip_rc(launch_grid_points(origin, spacing, dims, dist2_max, bricks, (uint32_t)n, queries,
                                     static_cast<hipStream_t>(stream)));
}

int rt_generate_shadow_rays(const rt_ray* rays, const rt_hit* hits, uint32_t num_rays, uint32_t num_triangles,
                            const float* light, rt_ray* shadow_rays, void* stream)
{
    if (!rays || !hits || !light || !shadow_rays) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(shadow_rays, 16)) return RT_ERR_INVALID_ARGUMENT;
    if (num_rays == 0) return RT_OK;
    return hip_rc(launch_shadow_rays(rays, hits, num_rays, num_triangles, light, shadow_rays, static_cast<hipStream_t>(stream)));
}

int rt_shade_frame(const rt_scene* scene, const rt_triangle* triangles, uint32_t num_triangles, const rt_ray* rays,
                   const rt_hit* hits, const rt_hit* shadow_hits, uint32_t w, uint32_t h, uint32_t spp, int layout,
                   int render_type, uint8_t* rgba8, void* stream)
{
    if (!scene || !triangles || !rays || !hits || !rgba8) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(rays, 16) || misaligned(hits, 16) || misaligned(shadow_hits, 16) || misaligned(rgba8, 4) ||
        misaligned(triangles, 4))
        return RT_ERR_INVALID_ARGUMENT;
    if (layout != RT_RAYS_ROW_MAJOR && layout != RT_RAYS_TILED) return RT_ERR_INVALID_ARGUMENT;
    if (spp != 1 && spp != 4 && spp != 16) return RT_ERR_INVALID_ARGUMENT;
    switch (render_type) {
    case RT_RENDER_DEPTH: break;
    case RT_RENDER_BOXTESTS: case RT_RENDER_TRIANGLE_TESTS: return RT_ERR_UNSUPPORTED;   // a hit record carries no test counts
    case RT_RENDER_MATERIAL_ID: case RT_RENDER_DIFFUSE:
        if (!scene->attributes || !scene->materials || scene->num_materials == 0) return RT_ERR_INVALID_ARGUMENT;   // as rt_trace
        break;
    case RT_RENDER_LODS: case RT_RENDER_TEXTURE: case RT_RENDER_TEXTURE_LIT: case RT_RENDER_TEXTURE_LIT_SHADOWS:
        if (!scene->attributes || !scene->materials || scene->num_materials == 0) return RT_ERR_INVALID_ARGUMENT;
        if (scene->num_textures && !scene->textures) return RT_ERR_INVALID_ARGUMENT;
        if (render_type == RT_RENDER_TEXTURE_LIT_SHADOWS && !shadow_hits) return RT_ERR_INVALID_ARGUMENT;
        break;
    default: return RT_ERR_INVALID_ARGUMENT;
    }
    if (w == 0 || h == 0) return RT_OK;
    ShadeLaunch t;
    t.scene = *scene;
    t.triangles = triangles;
    t.num_triangles = num_triangles;
    t.rays = rays;
    t.hits = hits;
    t.shadow_hits = shadow_hits;
    t.w = w; t.h = h; t.spp = spp;
    t.tiled = layout == RT_RAYS_TILED;
    t.render_type = render_type;
    t.rgba8 = rgba8;
    return hip_rc(launch_shade_frame(t, static_cast<hipStream_t>(stream)));
}

int rt_shade_frame_instanced(const rt_scene* scene, const rt_shade_geometry* geometry, uint32_t num_blas,
                             const rt_instance* instances, const rt_instance_record* records, uint32_t num_instances,
                             const int32_t* instance_materials, const rt_ray* rays, const rt_hit* hits,
                             const uint32_t* instance_ids, const uint32_t* shadow_instance_ids, uint32_t w, uint32_t h,
                             uint32_t spp, int layout, int render_type, uint32_t flags, uint8_t* rgba8, void* stream)
{
    if (!scene || !rays || !hits || !instance_ids || !rgba8) return RT_ERR_INVALID_ARGUMENT;
    if (num_instances > 0 && (!geometry || !instances || !records || num_blas == 0)) return RT_ERR_INVALID_ARGUMENT;
    if (misaligned(geometry, 16) || misaligned(instances, 16) || misaligned(records, 16) || misaligned(rays, 16) ||
        misaligned(hits, 16) || misaligned(instance_ids, 4) || misaligned(shadow_instance_ids, 4) ||
        misaligned(instance_materials, 4) || misaligned(rgba8, 4))
        return RT_ERR_INVALID_ARGUMENT;
    if (layout != RT_RAYS_ROW_MAJOR && layout != RT_RAYS_TILED) return RT_ERR_INVALID_ARGUMENT;
    if (spp != 1 && spp != 4 && spp != 16) return RT_ERR_INVALID_ARGUMENT;
    if (flags & ~(uint32_t)RT_SHADE_RENORMALIZE) return RT_ERR_INVALID_ARGUMENT;
    switch (render_type) {
    case RT_RENDER_DEPTH: break;
    case RT_RENDER_BOXTESTS: case RT_RENDER_TRIANGLE_TESTS: return RT_ERR_UNSUPPORTED;   // a hit record carries no test counts
    case RT_RENDER_MATERIAL_ID: case RT_RENDER_DIFFUSE:
        if (!scene->materials || scene->num_materials == 0) return RT_ERR_INVALID_ARGUMENT;   // (attributes: per BLAS)
        break;
    case RT_RENDER_LODS: case RT_RENDER_TEXTURE: case RT_RENDER_TEXTURE_LIT: case RT_RENDER_TEXTURE_LIT_SHADOWS:
        if (!scene->materials || scene->num_materials == 0) return RT_ERR_INVALID_ARGUMENT;
        if (scene->num_textures && !scene->textures) return RT_ERR_INVALID_ARGUMENT;
        if (render_type == RT_RENDER_TEXTURE_LIT_SHADOWS && !shadow_instance_ids) return RT_ERR_INVALID_ARGUMENT;
        break;
    default: return RT_ERR_INVALID_ARGUMENT;
    }
    if (w == 0 || h == 0) return RT_OK;
    ShadeInstancedLaunch t;
    t.scene = *scene;
    t.geometry = geometry;
    t.num_blas = num_blas;
    t.instances = instances;
    t.records = records;
    t.num_instances = num_instances;
    t.instance_materials = instance_materials;
    t.rays = rays;
    t.hits = hits;
    t.instance_ids = instance_ids;
    t.shadow_instance_ids = shadow_instance_ids;
    t.w = w; t.h = h; t.spp = spp;
    t.tiled = layout == RT_RAYS_TILED;
    t.render_type = render_type;
    t.flags = flags;
    t.rgba8 = rgba8;
    return hip_rc(launch_shade_frame_instanced(t, static_cast<hipStream_t>(stream)));
}

const char* rt_error_string(int code)
{
    switch (code) {
    case RT_OK: return "ok";
    case RT_ERR_INVALID_ARGUMENT: return "invalid argument";
    case RT_ERR_UNSUPPORTED: return "unsupported option";
    case RT_ERR_TOO_LARGE: return "too many triangles for the 29-bit node index";
    case RT_ERR_BUILD_INCOMPLETE: return "SAH build incomplete (error flags in the scratch status word)";
    default: break;
    }
    if (code <= RT_ERR_HIP_BASE) return hipGetErrorString(static_cast<hipError_t>(RT_ERR_HIP_BASE - code));
    return "unknown error";
}

const char* rt_version_string(void)
{
    return "rt_amd gfx950 | sort: LSD 3x10bit Morton keys (4x8bit generic), tile 4096 | lbvh: LDS agglomerative, 512 leaves/wg (4 wg per CU), leaves and node pairs staged in LDS and streamed out + one chained launch for all upper levels (last-arriver tickets, fan 48 or 64; passes of <= 1023 open roots by range searches over sparse tables), hybrid SAH top | "
           "sah: 4x4x4 grid + level-synchronous binned SAH (fixed launch count, no host round trip), workgroup-per-task stragglers, wave-per-task below 64 items, pairs, splits | "
           "trace: wave64 8x8 tiles, two-phase schedule, LDS stack 16, XCD chunks of 8 workgroups, pair prefetch from 8M primitives, counters through 16-row slots | "
           "rays: caller rays through the same traversal, 64 consecutive rays per wave, closest / any hit, 16-byte records, camera rays row-major or 8x8-tiled | "
           "raysort: 27-bit keys (7 origin bits per axis in the root box, Morton, above 2 direction bits per axis of d / max|d|), dead rays "
           "last, the 3x10bit sort with identity values, indexed queries through the ray-query kernel body | "
           "refit: top-down plan walk (one wide launch per level + one-workgroup tail, one CAS per run), one thread per leaf slot "
           "climbing by last-arrival tickets, sc1 box hand-off, ordered min / max | "
           "motion: a time per ray over two refitted poses of one tree, boxes and corners interpolated per lane as "
           "fl(fl(w0*a) + fl(t*b)) (monotone: interpolated boxes bound exactly), eight 16-byte requests per box step, the "
           "ray query's loop and tests | "
           "instances: proxy boxes + double inverse per instance (one launch), TLAS by the existing builders, two-level query "
           "on one 64-entry stack, TLAS leaves as stack entries, per-lane BLAS base pointers, world ray reloaded on exit | "
           "instance_motion: a time per ray over two key transforms of each instance, proxies of both keys by the instances' "
           "own arithmetic (one launch), TLAS pose 1 by refit, TLAS steps interpolated as the motion query's (eight 16-byte "
           "requests), the record's two matrices interpolated and inverted in float32 at the ray's time on entry, static BLAS "
           "steps on stored bits | "
           "spheres: ray queries over a tree built on sphere proxies (one prepare launch, padded boxes, any builder, refit "
           "for moving spheres), the ray query's box phase with a sphere test at the leaf (two dependent 16-byte loads, the "
           "discriminant from the perpendicular offset), closest / any hit, direct or through an index list | "
           "capsules: ray queries over a tree built on capsule proxies (round linear segments; one prepare launch, the padded "
           "box of both end spheres, any builder, refit for moving capsules), the sphere query's loop with a capsule test at "
           "the leaf (one 16-byte load, then two independent ones; the ray re-based at its point nearest the midpoint, the "
           "infinite cylinder's roots choose the body or one end sphere by side), closest / any hit, direct or indexed | "
           "spherecast: a ball swept along each ray over any triangle tree (no prepare step), the ray query's box phase on "
           "boxes grown by the lane's radius plus a 2^-18 pad, at the leaf the overlap predicate at tmin (the range query's "
           "d2), else the facing offset face and the near roots of the three edge capsules against one shrinking tmax, radius "
           "0 lanes run the ray query's tests, closest / any hit, direct or indexed, a feature word per ray | "
           "instance_mixed: the instanced ray query over triangle and sphere BLASes in one TLAS, a 16-byte geometry record per "
           "BLAS read on entry (kind, sphere array, count kept per lane), the leaf phase tests a triangle pair or a sphere by "
           "the lane's kind on the object-space ray, one tmax across both, the record shape by the hit instance's kind | "
           "instance_mixed_capsules: the mixed instanced query with capsule BLASes as a third kind, a CAPS template arm of "
           "the mixed kernels (the capsule query's leaf test on the object-space ray, the capsule record), kernels and a "
           "register bound of its own, direct or indexed | "
           "points: closest-point queries, one lane per query, distance-ordered traversal with re-culled pops (64-entry stack, "
           "16 entries + distances in LDS), exact d2 = Ericson + vertex-box clamp, lexicographic (dist2, id) | "
           "range: sphere / box range queries, one lane per query, unordered traversal on a 64-entry stack of 4-byte entries "
           "(16 in LDS), one traversal compiled for count and collect, CSR output by a 64-bit device scan (workgroup scan in "
           "the count kernel + one workgroup over the sums + add), ids by plain stores into the query's own segment | "
           "knn: k-nearest queries (k <= 32), the point query's traversal pruned against the k-th record, a sorted per-lane list "
           "(registers hold its length, k-th record and bound; find the position, then shift; duplicates dropped), rows of 8-byte "
           "records | "
           "rayhits: all-hit ray queries, every triangle a ray crosses in a fixed [tmin, tmax] window, the range query's frame "
           "(one lane per ray, unordered traversal, 64-entry stack of 4-byte entries, 16 in LDS) with the tracer's slab and "
           "Moller-Trumbore tests, CSR output by the 64-bit device scan, 16-byte hit records by plain stores into the ray's "
           "own segment | "
           "rayfirst: first-K ray queries (k <= 32), the all-hit frame pruned against the k-th record's t, nearest-first box "
           "steps, 64-entry stack of 4-byte entries (16 in LDS), knn's sorted per-lane list of 16-byte hit "
           "records, one launch | "
           "rayfilter: hit filters for the closest / any, all-hit and first-K ray queries (face culling by the sign of the "
           "stored-corner determinant, a skip id and a mask per ray, a mask per primitive), asked inside the leaf test after the "
           "t window test: the siblings' traversals, one 8-byte load per ray and one 4-byte load per surviving candidate | "
           "instancefilter: the instanced ray query with an instance mask asked at the TLAS leaf before the record is read (one "
           "8-byte load, a masked instance costs no BLAS descent), world-space face culling (the sign of the record's 3x3 "
           "determinant swaps the cull bits, per-instance disable / flip) and a per-ray (instance, primitive) skip: the sibling's "
           "two-level loop, one 16-byte load per ray | "
           "trioverlap: triangle-overlap queries, every triangle a caller triangle cuts (vertex boxes + seventeen separating "
           "axes in three rolled loops, first separating axis leaves), optional self mode (j > i, no shared corner), the "
           "range query's frame and CSR output | "
           "sdf: signed distance and occupancy in one launch, one lane per query, the point query's distance-ordered traversal "
           "(weight-free d2) then 1 or 3 parity votes by the all-hit traversal (fixed window, a counter instead of a row) on one "
           "64-entry stack (16 in LDS), third vote only where the first two disagree, 8-byte records or one byte, grid points "
           "row-major or in 4x4x4 Morton bricks | "
           "shade: deferred shading from hit records, one thread per pixel, no stack, no LDS, no scratch, per-render-type "
           "instantiations, shadow rays as a ray batch for the any-hit query | "
           "instance_shade: deferred shading from instanced hit records, the shade kernel's frame with a gather per sample "
           "(record tail, 32-byte geometry entry, object_to_world rows where corners are read, world_to_object rows where "
           "normals are read), corners and normals placed in float32 per lane, the same shaders: the flattened scene's frame | "
           "ray_hits_instanced: instanced all-hit ray queries, every crossing of every placed copy with its instance, the "
           "all-hit frame (fixed window, unordered 64-entry stack of 4-byte entries, 16 in LDS, CSR by the 64-bit device scan) "
           "with the instanced query's second level in its loop (an entry of count 0 is an instance in the TLAS and a leaf in a "
           "BLAS, per-lane base pointers, world ray reloaded on exit), hit records and instance ids in parallel segments | "
           "ray_first_instanced: instanced first-K ray queries, the k <= 32 nearest crossings over placed copies in "
           "(t, instance, primitive_id) order with their instances, the first-K frame (shrinking bound, nearest-first step, "
           "4-byte pending entries, private list) with the instanced all-hit query's second level in its loop, one bound for "
           "both levels, the instances in an array parallel to the list's records, one launch | "
           "instance_set_filter: the instanced all-hit and first-K queries with the instanced query's filter (instance mask "
           "asked at the TLAS leaf before the record is read, world-space face culling, a per-ray (instance, primitive) skip) "
           "as a FILTERED template arm of the siblings' kernels, a rejected crossing never enters the first-K list or moves "
           "its bound | "
           "instance_indexed: the instanced (plain and filtered), instanced-motion, mixed-instanced and motion ray queries "
           "through an index list as an INDEXED template arm of the siblings' kernels (lane j takes ray order[j]; rays, times, "
           "per-ray filter records, hits and instance ids go by the ray index), the sorted order of rt_sort_rays over the TLAS "
           "or any list of live rays";
}

}  // extern "C"
