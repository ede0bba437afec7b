/*
 * rt_abi.h -- C ABI of the MI355X-native LBVH builder + primary-ray tracer (librt_amd.so).
 *
 * This is the drop-in boundary for the hot path of gregc-91/GPU-Raytracing.  Every entry point
 * names the reference interface it replaces (file:line relative to /root/reference/src).  All
 * pointers are DEVICE pointers unless said otherwise; the caller allocates and owns every buffer
 * (as the reference's Display() does, main.cu:226-240); `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Nothing here allocates, frees or synchronises, so a call sequence can be
 * captured in a hipGraph.  Return value: 0 on success, RT_ERR_* (<0) on bad arguments, or
 * -(hipError_t) - 1000 when a HIP call failed (the reference calls exit() instead, Common.cuh:358-366).
 *
 * POD layouts are byte-identical to the reference's (sizes checked by static_assert in the library):
 *   rt_triangle 36, rt_node 32, rt_triangle_pair 64, rt_camera 64, rt_attributes 72 (rt_ray 32, rt_hit 16: no reference
 *   counterpart).
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_float3 { float x, y, z; } rt_float3;

/* Common.cuh:199-243 Triangle */
typedef struct rt_triangle { rt_float3 v0, v1, v2; } rt_triangle;

/* Common.cuh:152-159 Node: a child-descriptor slot; slots come in sibling pairs (2i, 2i+1).
 * w12 = parent:29 (LSBs) | count:3     w28 = child:29 (LSBs) | type:3 (rt_child_type) */
typedef struct rt_node { rt_float3 min; uint32_t w12; rt_float3 max; uint32_t w28; } rt_node;

/* Common.cuh:161-197 TrianglePair */
typedef struct rt_triangle_pair {
    rt_float3 v0; uint32_t primitive_id_0;
    rt_float3 v1; uint32_t primitive_id_1;
    rt_float3 v2; uint16_t rotations[2];
    rt_float3 v3; float pad3;
} rt_triangle_pair;

/* Common.cuh:44-53 Camera */
typedef struct rt_camera {
    rt_float3 position; float pitch;
    rt_float3 w;        float yaw;
    rt_float3 u;        float scale;
    rt_float3 v;        float max_depth;
} rt_camera;

/* Common.cuh:55-59 Attributes (float2 is 8-byte aligned in CUDA, hence the pads) */
typedef struct rt_attributes {
    rt_float3 normal[3]; uint32_t pad0;
    float uv[3][2];
    int32_t material_id; uint32_t pad1;
} rt_attributes;

/* POD mirror of the device-read fields of Material (Common.cuh:93-129; the reference memcpy's a
 * struct holding a std::string to the device) */
typedef struct rt_material {
    rt_float3 ambient, diffuse, specular;
    float specular_exp;
    int32_t texture, bump, disp;
} rt_material;

/* POD mirror of the device-read fields of Texture (Common.cuh:61-91): an RGBA8 mip chain.  mips[l] is a DEVICE pointer to
 * size_x[l] * size_y[l] texels (row 0 first), levels 0..max_lod as Texture::GenerateLODs makes them (FileIO.cpp:121-150). */
#define RT_NUM_LODS 13
typedef struct rt_texture {
    const uint32_t* mips[RT_NUM_LODS];
    int32_t size_x[RT_NUM_LODS], size_y[RT_NUM_LODS];
    uint32_t max_lod, pad;
} rt_texture;

typedef enum rt_child_type { RT_CHILD_NONE = 0, RT_CHILD_BOX = 1, RT_CHILD_TRI = 2 } rt_child_type; /* Common.cuh:35-41 */

/* Arguments.h:8-26 */
typedef enum rt_build_type { RT_BUILD_SAH = 0, RT_BUILD_BOTTOM_UP = 1, RT_BUILD_HYBRID = 2, RT_BUILD_NONE = 3 } rt_build_type;
typedef enum rt_render_type {
    RT_RENDER_DEPTH = 0, RT_RENDER_BOXTESTS = 1, RT_RENDER_TRIANGLE_TESTS = 2, RT_RENDER_MATERIAL_ID = 3,
    RT_RENDER_LODS = 4, RT_RENDER_DIFFUSE = 5, RT_RENDER_TEXTURE = 6, RT_RENDER_TEXTURE_LIT = 7,
    RT_RENDER_TEXTURE_LIT_SHADOWS = 8, RT_RENDER_COUNT = 9
} rt_render_type;

/* Arguments.h:28-33 Arguments */
typedef struct rt_arguments { int32_t build_type; int32_t enable_splits; int32_t enable_pairs; int32_t render_type; } rt_arguments;

/* BuildWrapper.cuh:6-12 BuildInput */
typedef struct rt_build_input {
    const rt_triangle* triangles_in;   /* 36 n bytes */
    rt_triangle_pair*  triangles_out;  /* >= 64 n bytes (reference allocates 64*2n, main.cu:232-233) */
    uint32_t           num_triangles;
    rt_node*           nodes_out;      /* >= rt_nodes_bytes(n) */
    void*              scratch;        /* >= rt_bu_memory_requirements(n), 256-byte aligned */
} rt_build_input;

/* Common.cuh:335-340 DeviceAccelerationStructure */
typedef struct rt_accel { const rt_triangle_pair* triangles; const rt_node* nodes; uint32_t root; uint32_t count; } rt_accel;

/* Common.cuh:342-351 DeviceScene.  textures: device array indexed by rt_material.texture / .bump / .disp; only the
 * textured render types (kLODs, kTexture, kTextureLit, kTextureLitShadows) read it. */
typedef struct rt_scene {
    const rt_attributes* attributes;
    const rt_material*   materials;
    const rt_texture*    textures;
    const rt_camera*     camera;        /* device pointer, as in the reference (main.cu:151,161) */
    float                light[3];
    uint32_t             num_attributes, num_materials, num_textures;   /* num_attributes = number of primitives (main.cu:166); also
                                                                          the scene-size hint of rt_trace (0 = unknown): from 8M
                                                                          primitives on the tracer takes its pair-prefetch form */
} rt_scene;

enum {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = -1,
    RT_ERR_UNSUPPORTED = -2,       /* rt_shade_frame: RT_RENDER_BOXTESTS / RT_RENDER_TRIANGLE_TESTS (a hit record carries no test
                                    * counts); no option of the build and trace paths returns it */
    RT_ERR_TOO_LARGE = -3,         /* n exceeds the 29-bit child index of Node (Common.cuh:152-159) */
    RT_ERR_BUILD_INCOMPLETE = -4,  /* (kept for ABI stability: rt_run_sah_build is asynchronous since round 4 and reports through the status word) */
    RT_ERR_HIP_BASE = -1000        /* -(hipError_t) + RT_ERR_HIP_BASE */
};

/* replaces BuMemoryRequirements (BuildWrapper.cu:132-136).  Scratch also holds what the reference
 * cudaMalloc's inside RadixSort (RadixSort.cu:187-190). */
size_t rt_bu_memory_requirements(uint32_t num_triangles);

/* bytes the caller must provide for nodes_out; same rule as main.cu:235-237: 32 * 4 * (n + 512) */
size_t rt_nodes_bytes(uint32_t num_triangles);

/* replaces RunBottomUpBuild (BuildWrapper.cu:253-362).  hybrid != 0 additionally builds the SAH top
 * tree above the 8-level-deep LBVH sub-roots (ExtractDepth + SharedTaskBuild, BuildWrapper.cu:350-361);
 * trace root is then (2n+1, 2) instead of (0, 2) (main.cu:222-223).  The top tree is built deterministically
 * (the reference's numbering depends on atomic arrival order); it occupies slots [2L, 2L + 2*256 + 2).
 * args->enable_pairs (Pairing.cuh, GenerateMortonCodesPairs): triangles 2k, 2k+1 sharing an edge become one quad
 * leaf; leaf slots are assigned by a prefix sum in input order (the reference uses atomicAdd arrival order), the
 * leaf count L lands in scratch (rt_bu_scratch_layout.num_leaves); hybrid + pairs roots at (2L+1, 2). */
int rt_run_bottom_up_build(const rt_build_input* input, const rt_arguments* args, int hybrid, void* stream);

/* replaces SahMemoryRequirements (BuildWrapper.cu:126-130); about 90 bytes per triangle */
size_t rt_sah_memory_requirements(uint32_t num_triangles);

/* replaces RunSahBuild (BuildWrapper.cu:140-251), the reference's default --type: leaves bucketed into a 4x4x4 grid
 * by centroid (Setup, GridBlockCounts/Scan/Distribute, Multiblock.cu:139-207,427-546), one binned-SAH sub-tree per
 * cell and a SAH top tree over the cells (SharedTaskBuild, SharedTaskBuilder.cu:93-607,909-967).  Trace root =
 * (slot 0, count 1) (main.cu:222-223).  input->scratch holds rt_sah_memory_requirements(n) bytes, nodes_out
 * rt_nodes_bytes(n); the tree uses slots [0, 128 + 2L), L = number of items.  args->enable_pairs as in
 * rt_run_bottom_up_build.  args->enable_splits (SetupSplits / SetupPairSplits, Multiblock.cu:209-425): a leaf whose
 * box spans several cells of the 4x4x4 grid over the scene box is referenced once per cell, box clipped to the cell,
 * while the running total of extra references -- taken in input order; an atomic counter in the reference -- stays
 * below n/5 (so L < n + n/5; n <= 2^25 with splits).
 * Same tree as the reference up to numbering, which is deterministic here: leaf slots in input order, node slots
 * = f(split position) (see gpu-raytracing_amd/csrc/sah_build.hip).  The depth of the trees is data dependent and the
 * reference loops on the host (cudaMemcpy of num_leaves, BuildWrapper.cu:229); here the number of launches is fixed by n
 * and the data-dependent tail runs as a device-side loop: the call neither copies nor synchronises (hipGraph-capturable,
 * like rt_run_bottom_up_build).  Error flags: the status word of the scratch (rt_sah_scratch_layout.status), 0 = complete
 * tree, to be read by the caller after the stream has run. */
int rt_run_sah_build(const rt_build_input* input, const rt_arguments* args, void* stream);

typedef struct rt_sah_scratch_layout {
    size_t p_aabb, c_aabb;  /* int32[6] each: ordered-int primitive / centroid bounds of the scene (BuildWrapper.cu:170-176) */
    size_t status;          /* uint32[8]: [0] error flags of the last build (0 = ok), [1] number of items L (leaves, or
                             * leaf references with splits), [2] number of TrianglePair records written */
    size_t num_leaves;      /* = status + 4 (items) */
    size_t cell_counts;     /* uint32[64]: leaves per grid cell (block_counts, Multiblock.cu:427) */
    size_t total;
} rt_sah_scratch_layout;
int rt_sah_scratch_layout_get(uint32_t num_triangles, rt_sah_scratch_layout* out);

/* Where the build's intermediates live inside `scratch` (for parity tests and callers that want the
 * sorted Morton codes).  Offsets in bytes. */
typedef struct rt_bu_scratch_layout {
    size_t p_aabb;          /* int32[6] ordered-int scene box (BuildWrapper.cu:288-289, Multiblock.cu:104) */
    size_t status;          /* uint32[8]: [0] = error flags of the last build, 0 = ok (bit 0: a workgroup found more
                               than 128 unfinished sub-trees -- impossible for a tree of depth <= 62) */
    size_t num_leaves;      /* uint32: number of leaves L of the last build (= n unless args.enable_pairs merged triangles) */
    size_t morton;          /* uint32[n] sorted Morton codes after the build */
    size_t sorted_indices;  /* uint32[n] original triangle index per sorted position */
    size_t total;
} rt_bu_scratch_layout;
int rt_bu_scratch_layout_get(uint32_t num_triangles, rt_bu_scratch_layout* out);

/* replaces the CalculateSceneAabb launch (Multiblock.cu:104-114, BuildWrapper.cu:305-308).
 * aabb_ordered: int32[6]; this call first resets it to the ordered-int empty box. */
int rt_calculate_scene_aabb(const rt_triangle* triangles, uint32_t n, int32_t* aabb_ordered, void* stream);

/* replaces the GenerateMortonCodes launch (BottomUpBuilder.cu:98-115, BuildWrapper.cu:324-328) */
int rt_generate_morton_codes(uint32_t* codes, uint32_t* values, const rt_triangle* triangles,
                             const int32_t* aabb_ordered, uint32_t n, void* stream);

/* replaces RadixSort (RadixSort.cuh:6-7, RadixSort.cu:171-225): stable ascending sort of (key,value)
 * pairs, result in keys/values, tmp_* are n-entry temporaries.  sort_scratch: >= rt_radix_sort_scratch_bytes(n).
 * count <= 0x3FFFFFFF (the kernels address the arrays with 32-bit byte offsets); larger -> RT_ERR_TOO_LARGE, nothing runs. */
size_t rt_radix_sort_scratch_bytes(uint32_t count);
int rt_radix_sort_u32_pairs(uint32_t* keys, uint32_t* values, uint32_t* tmp_keys, uint32_t* tmp_values,
                            uint32_t count, void* sort_scratch, void* stream);
/* The same sort for keys whose bits [key_bits, 32) are all zero (RunBottomUpBuild's Morton codes have 30,
 * BottomUpBuilder.cu:23-32; the reference's RadixSort always runs its four 8-bit passes, RadixSort.cu:192-219).
 * Up to 30 bits and a moderate count it runs three 10-bit passes, which read their input from the temporaries:
 * input_in_tmp = 1 says the unsorted pairs are in tmp_keys / tmp_values (0: in keys / values); when that is not where
 * the chosen pass count reads from, the pairs are copied across first (rt_radix_sort_input_in_tmp tells a caller that
 * wants to avoid the copy where to put them).  The sorted result is in keys / values either way. */
int rt_radix_sort_u32_pairs_bits(uint32_t* keys, uint32_t* values, uint32_t* tmp_keys, uint32_t* tmp_values,
                                 uint32_t count, uint32_t key_bits, int input_in_tmp, void* sort_scratch, void* stream);
int rt_radix_sort_input_in_tmp(uint32_t count, uint32_t key_bits);

/* replaces Trace()/TraceRays (main.cu:125-192, Tracer.cu:471-595) for rows [y0, y1) of a w x h frame.
 * rgba8: full-frame linear RGBA8 buffer, pitch 4*w, row 0 first (= the surface contents, SURVEY A).
 * counters: optional device uint64[4], [0] += sum of box tests, [1] += sum of triangle tests (the reference's
 * num_tests is [0], Tracer.cu:503); [2] / [3] += wave-level box-phase / leaf-phase steps (profiling aid).  spp = 1 is the reference; spp in {4,16} is the
 * SURVEY 8(d) config-5 extension (2x2 / 4x4 stratified sub-pixel offsets, averaged before the u8 truncation). */
int rt_trace(const rt_accel* as, const rt_scene* scene, uint64_t* counters, int render_type, uint8_t* rgba8,
             uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, uint32_t spp, void* stream);

/* Multi-GPU partition into INTERLEAVED STRIPS (no reference counterpart: the reference traces on one GPU,
 * main.cu:169).  A strip = strip_rows rows (a multiple of 8); this call renders strips first_strip, first_strip +
 * strip_stride, ... of the w x h frame in ONE launch and stores them COMPACTLY: its j-th strip occupies rows
 * [j*strip_rows, (j+1)*strip_rows) of rgba8_compact (pitch 4*w), which must hold
 * ceil(ceil(h / strip_rows) / strip_stride) strips.  Rank r of P calls it with (first_strip, strip_stride) = (r, P);
 * rank 0 gathers the compact buffers and de-interleaves them (gpu-raytracing_amd/sharding.py). */
int rt_trace_strips(const rt_accel* as, const rt_scene* scene, uint64_t* counters, int render_type,
                    uint8_t* rgba8_compact, uint32_t w, uint32_t h, uint32_t strip_rows, uint32_t first_strip,
                    uint32_t strip_stride, uint32_t spp, void* stream);

/* ---- ray queries (no reference counterpart: the reference only traces its own camera rays, Tracer.cu:471-595).
 * rt_ray: origin, tmin, direction, tmax -- 32 bytes, two 16-byte halves.  The direction need not be normalised; t is in units
 * of |dir|; tmax = +inf is allowed.  A ray with tmin > tmax or a NaN component is not traced (a miss, no tests counted).
 * rt_hit: closest hit (or, RT_RAY_ANY_HIT, some hit) of a ray -- 16 bytes:
 *   t             hit distance, in [tmin, tmax]
 *   primitive_id  the caller's triangle index (the leaf's primitive_id_0/1: split references report their original triangle)
 *   u, v          barycentric weights of the caller's corners v1 and v2: o + t*d ~= (1-u-v)*v0 + u*v1 + v*v2 (pair leaves
 *                 store rotated triangles; the weights are mapped back through rt_triangle_pair.rotations as the shading does)
 *   a miss is {+inf, RT_MISS, 0, 0}. */
typedef struct rt_ray { rt_float3 origin; float tmin; rt_float3 dir; float tmax; } rt_ray;
typedef struct rt_hit { float t; uint32_t primitive_id; float u, v; } rt_hit;
#define RT_MISS 0xFFFFFFFFu
enum { RT_RAY_CLOSEST_HIT = 0, RT_RAY_ANY_HIT = 1 };
enum { RT_RAYS_ROW_MAJOR = 0, RT_RAYS_TILED = 1 };

/* hits[i] for rays[i], i < num_rays, through any tree rt_trace takes.  Per-ray semantics are rt_trace's exactly (slab test,
 * Moller-Trumbore with the same epsilon, slot order, nearest child first, 64-entry stack with dropped pushes, pops not
 * re-culled), so through the same rays the closest-hit records and test counts equal rt_trace's.  mode RT_RAY_ANY_HIT ends a
 * ray's traversal at its first accepted triangle.  rays / hits: 16-byte aligned device arrays; hits[i >= num_rays] are not
 * written.  counters: optional device uint64[4], as for rt_trace ([0] += sum of box tests, [1] += sum of triangle tests,
 * [2] / [3] += wave-level box-phase / leaf-phase steps); one LDS reduction + 4 device atomics per workgroup of 256 rays.
 * num_primitives: scene-size hint as rt_scene.num_attributes (0 = unknown; from 8M on the pair-prefetch traversal).
 * num_rays = 0: nothing runs. */
int rt_intersect_rays(const rt_accel* as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, int mode,
                      uint32_t num_primitives, uint64_t* counters, void* stream);

/* The primary rays rt_trace traces for a w x h frame at spp in {1, 4, 16}, bit for bit (direction, origin = camera position,
 * tmin = 0.00001, tmax = camera->max_depth; the same stratified sub-pixel offsets).  camera: device pointer.  Layouts:
 *   RT_RAYS_ROW_MAJOR  w*h*spp rays; ray (y*w + x)*spp + s is sample s of pixel (x, y)
 *   RT_RAYS_TILED      tiles_x*tiles_y*spp*64 rays, tiles_x = ceil(w/8), tiles_y = ceil(h/8); ray (tile*spp + s)*64 + lane,
 *                      tile = ty*tiles_x + tx, pixel (8*tx + lx, 8*ty + ly) with lane = Morton(lx, ly): lx = lane bits 0, 2, 4,
 *                      ly = lane bits 1, 3, 5 -- one wave of rt_intersect_rays gets one 8 x 8 tile and one sample, rt_trace's
 *                      coherence.  Off-frame lanes of edge tiles get a ray with tmax = -1 < tmin (a miss, nothing traced).
 * rays: 16-byte aligned.  w*h = 0: nothing runs. */
int rt_generate_camera_rays(const rt_camera* camera, uint32_t w, uint32_t h, uint32_t spp, int layout, rt_ray* rays,
                            void* stream);

/* ---- refit (no reference counterpart: the reference's bottom-up box pass exists only inside its LBVH build,
 * BottomUpBuilder.cu:217-285).  Keeps the topology and leaf assignment of a built tree and recomputes its geometry after the
 * caller's vertices moved: the leaf records' vertices and the box of every slot reachable from (root, count).
 *
 * rt_build_refit_plan, once per build: walks the tree top-down from (root, count) and fills `plan` (the parent of every
 * reachable slot run, its expected arrivals, the leaf-slot list, a status word and a fingerprint of nodes_out, root, count and
 * n).  It reads input->nodes_out and input->triangles_out only.
 * rt_refit, every frame: input->triangles_in holds the NEW positions (same count, same order as at build time).  It rewrites
 * the vertices of the leaf records in input->triangles_out and the boxes of the reachable slots in input->nodes_out; every
 * other byte is left as it is (the w12 / w28 words, primitive ids, rotations, pad3, NONE slots, unreachable slots).
 * Both are asynchronous (no host copy, no synchronisation: hipGraph-capturable), with a fixed number of launches for a given
 * n: the plan 5 + ceil(log2 n) launches, the refit one.
 *
 * Leaf records.  A record is rebuilt from input->triangles_in; its ids and rotations stay as the build wrote them.  Every
 * builder writes a single-triangle record with primitive_id_1 = 0 and a pair record with primitive_id_1 = primitive_id_0 + 1
 * (lbvh_levels.hip, sah_build.hip, the oracle): that is how the two are told apart.
 *   single: v0..v2 = triangle primitive_id_0, v3 = v2 bit for bit (the traversal relies on v3 == v2).
 *   pair:   A = triangle primitive_id_0 rotated by rotations[0] (1: (v2, v0, v1), 2: (v1, v2, v0), else as is), v3 = corner
 *           v0 (rotations[1] = 2), v1 (1) or v2 (else) of B = triangle primitive_id_0 + 1 -- CreateTrianglePair's layout.
 *   With splits (rt_run_sah_build, enable_splits) a record is shared by several leaf slots: each writes the same bytes.
 * Boxes.  A leaf slot gets the ordered min / max of its record's triangle corners (A, plus B for a pair); a box slot the
 * ordered union of the boxes of the non-NONE slots of its child run [child, child + count) (any run length 1..7).  Ordered
 * min / max compare the floats' monotone integer image, -0 below +0: the result does not depend on arrival order and is
 * bit-identical from run to run.
 *   An identity refit (the build's own positions) gives back the build's bytes, with two documented exceptions:
 *   - signed zeros: the LBVH builder's leaf boxes use fminf / fmaxf, so where a box bound is a zero whose sign differs
 *     between corners the refitted box may carry the other zero.  The boxes are equal as numbers.
 *   - split trees: a refit writes UNCLIPPED leaf boxes (the record's own bound), where the build clipped each reference to
 *     its grid cell.  Conservative and correct, but looser than the build's boxes.
 *
 * Status word (rt_refit_plan_layout.status, uint32, RT_REFIT_* flags), to be read after the stream has run.  The flags are
 * sticky: rt_build_refit_plan clears them, every later rt_refit on the plan only adds to them.
 *   RT_REFIT_BAD_TREE       the walk found something that is not a tree: a run reached twice (or two runs sharing a slot), a
 *                           slot index at or beyond rt_nodes_bytes(n)/32, a box slot with count 0 or whose run has no
 *                           non-NONE slot, a child type above 2, a record index at or beyond n, or a record whose ids are
 *                           neither a single's nor a pair's.  The plan is unusable: rt_refit writes nothing.
 *   RT_REFIT_PLAN_MISMATCH  rt_refit was given nodes_out, root, count or n other than the plan's.  Nothing is written.
 *   RT_REFIT_PAIR_BROKEN    after the update a pair record's B no longer shares A's edge: B's corners on the edge named by
 *                           rotations[1] differ from (v2, v1) of the rotated A, compared as the pairing test compares
 *                           corners (float ==).  The record cannot represent B; boxes still bound both triangles.  Rebuild.
 *
 * plan: rt_refit_plan_bytes(n) bytes of device memory, 256-byte aligned, owned by the caller; no initialisation needed.
 * Size: with S = rt_nodes_bytes(n) / 32 = 4 (n + 512) slots, 256 + 9 S bytes rounded up to three 256-byte aligned arrays --
 * 36 bytes per triangle + about 18 KB.
 * Argument errors, returned before any GPU work: RT_ERR_INVALID_ARGUMENT for a null input / plan / buffer, a plan not
 * 256-byte aligned, triangles_in not 16-, triangles_out or nodes_out not 64-byte aligned, count > 7; RT_ERR_TOO_LARGE for
 * n > RT_REFIT_MAX_TRIANGLES (every slot index must fit 29 bits with one value to spare).  n = 0: nothing runs. */
#define RT_REFIT_MAX_TRIANGLES ((1u << 27) - 1024u)
enum { RT_REFIT_BAD_TREE = 1, RT_REFIT_PLAN_MISMATCH = 2, RT_REFIT_PAIR_BROKEN = 4 };
size_t rt_refit_plan_bytes(uint32_t num_triangles);
typedef struct rt_refit_plan_layout {
    size_t status;    /* uint32: RT_REFIT_* flags (the first word of a 256-byte header) */
    size_t parents;   /* uint32[S]: run-first slot: parent slot : 29 | expected arrivals : 3; other reached slot: its offset */
    size_t arrivals;  /* uint8[S]: arrivals so far at a run-first slot (0 between refits); bit 7: the slot is a reached leaf */
    size_t leaves;    /* uint32[S]: the reached leaf slots (their number: header word 1) */
    size_t total;     /* = rt_refit_plan_bytes(n) */
} rt_refit_plan_layout;
int rt_refit_plan_layout_get(uint32_t num_triangles, rt_refit_plan_layout* out);
int rt_build_refit_plan(const rt_build_input* input, uint32_t root, uint32_t count, void* plan, void* stream);
int rt_refit(const rt_build_input* input, uint32_t root, uint32_t count, void* plan, void* stream);

/* ---- motion-blur ray queries (no reference counterpart: the reference traces one frozen mesh, main.cu:125-192).  A time per
 * ray over TWO key poses of one tree: what motion blur and any time-sampled visibility query of a deforming mesh need.
 *
 * Poses.  Pose 0 is a built tree (any tree rt_intersect_rays takes).  Pose 1 is a byte copy of pose 0's nodes_out /
 * triangles_out, refitted (rt_refit) with the moved vertices through a plan of its OWN (a plan fingerprints its nodes_out).
 * Refit keeps topology, ids and rotations, so both poses are one tree with two geometries.  Both poses must have refit status
 * 0 (a broken pair cannot be represented) and all coordinates must be finite (0 * inf is NaN).
 *   SPLIT TREES (rt_run_sah_build, enable_splits): pose 0 must be identity-refitted first.  The build clips a split
 *   reference's leaf box to its grid cell, a refit writes the record's unclipped bound; a clipped box interpolated with an
 *   unclipped one bounds nothing.
 *
 * rt_intersect_rays_motion: hits[i] for rays[i] at times[i], i < num_rays.  times[i] lies in [0, 1].  Ray i sees every box
 * bound and every leaf-record corner of the tree as
 *       w0 = 1 - times[i]  (computed once per ray);   v = fl(fl(w0 * a) + fl(times[i] * b))
 * in float32, a from pose 0 and b from pose 1, the three operations rounded separately (no fused multiply-add).  This form is
 * monotone in a and in b, so an interpolated box bounds the interpolated corners and boxes under it exactly, and it gives a
 * at time 0 and b at time 1 (as numbers: a zero may change sign).  a + t * (b - a) has neither property and is not used.
 * The slots' w12 / w28 words, primitive ids and rotations are read from pose 0.
 *   Everything else is rt_intersect_rays's contract, applied to the interpolated values: the slab test, Moller-Trumbore with
 *   the same epsilon, slot order, nearest child first, the 64-entry stack with dropped pushes, pops not re-culled, RT_RAY_ANY_HIT
 *   ending a ray at its first accepted triangle, a single-triangle record's second triangle skipped (v3 == v2, compared on the
 *   interpolated corners), (u, v) mapped through rotations, the miss record {+inf, RT_MISS, 0, 0}, and the counters ([0] box
 *   tests, [1] triangle tests, [2] / [3] wave steps).  With every time 0 (1) the records and counters [0], [1] are
 *   rt_intersect_rays's over pose 0 (pose 1); t, u, v may differ in the sign of a zero.
 *   A ray rt_intersect_rays would not trace, and a ray whose time is NaN or outside [0, 1], is not traced: a miss, no tests
 *   counted.  hits[i >= num_rays] are not written.
 *   rays / hits: 16-byte aligned device arrays; times: a 4-byte aligned device array of num_rays floats; counters: optional
 *   device uint64[4].  Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null as / rays / times / hits,
 *   a null tree pointer with count > 0, count > 7, rays or hits not 16-byte aligned, times not 4-byte aligned, a mode other than
 *   the two.  num_rays = 0: nothing runs.  Asynchronous, no host copy: hipGraph-capturable.
 *   Cost: every step fetches from both poses, twice rt_intersect_rays's requests (DESIGN section 22 has the measured ratio).
 *
 * rt_motion_validate, once per pair of poses, off the hot path (a memset and one streaming launch): sets
 * RT_MOTION_TOPOLOGY_MISMATCH in *status (a 4-byte aligned device uint32; read it after the stream has run) when a w12 / w28
 * word of any of the rt_nodes_bytes(num_triangles) / 32 slots, or the primitive ids or rotations of any of the num_triangles
 * leaf records, differ between the poses; clears the word otherwise.  count = 0: the word is cleared, nothing is compared.
 * Argument errors: RT_ERR_INVALID_ARGUMENT for a null as / status, a null tree pointer with count > 0, count > 7, a status not
 * 4-byte or a tree pointer not 16-byte aligned; RT_ERR_TOO_LARGE for num_triangles > RT_REFIT_MAX_TRIANGLES.
 *
 * Out of scope: more than two key poses (motion of instance transforms: the instance-motion block below); filtered, all-hit
 * and first-K motion forms (the indexed form: rt_intersect_rays_motion_indexed, the indexed-instanced block below);
 * the pair-prefetch traversal; shading of motion hits; the C++ host mirror and rt_cli. */
typedef struct rt_motion_accel {
    const rt_triangle_pair* triangles0; const rt_node* nodes0;   /* key pose at time 0 */
    const rt_triangle_pair* triangles1; const rt_node* nodes1;   /* key pose at time 1: the same tree, refitted */
    uint32_t root, count;
} rt_motion_accel;
enum { RT_MOTION_TOPOLOGY_MISMATCH = 1 };
int rt_motion_validate(const rt_motion_accel* as, uint32_t num_triangles, uint32_t* status, void* stream);
int rt_intersect_rays_motion(const rt_motion_accel* as, const rt_ray* rays, const float* times, rt_hit* hits,
                             uint32_t num_rays, int mode, uint64_t* counters, void* stream);

/* ---- instancing (no reference counterpart: the reference traces one mesh, main.cu:125-192).  A scene of placed copies of
 * a few meshes: every mesh has its own built tree (a bottom-level tree, BLAS: any tree rt_trace takes -- LBVH, pairs, hybrid,
 * SAH, splits, mixed kinds in one table), and a small top-level tree (TLAS) is built over the placed copies.
 *
 * rt_instance (caller input, 64 bytes): object_to_world, row-major 3x4: world = M[:, :3] * p + M[:, 3]; blas indexes the
 * BLAS table (a DEVICE array of rt_accel).
 * rt_instance_record (64 bytes, written by rt_prepare_instances, read by the query): world_to_object, row-major 3x4 (the
 * inverse of object_to_world, computed in double and rounded to float), blas, flags (the instance's RT_INSTANCE_* flags;
 * non-zero: the query never enters the instance), two spare words (0).
 *
 * rt_prepare_instances, one launch after a clear of *status, one thread per instance:
 *   - the object box: the ordered min / max over the non-NONE slots of the BLAS's root run [root, root + count);
 *   - its 8 corners go through object_to_world in float32, in the order ((m0*x + m1*y) + m2*z) + m3 per row;
 *   - lo / hi = min / max of the transformed corners, then every bound moves outward by pad = 2^-12 * E, E = the largest
 *     |lo| or |hi| over the three axes (lo - pad, hi + pad in float32): a box conservative against the rounding of the
 *     object-space ray (below) for rays that start within a few box magnitudes of the instance;
 *   - proxies[i] = {v0 = lo, v1 = hi, v2 = lo*0.5f + hi*0.5f}: its box is exactly [lo, hi] and its centroid lies inside it,
 *     so it is a valid input for every builder (Morton codes, SAH centroids);
 *   - records[i] as above.
 * Status flags (OR over the instances, written to *status, a device uint32 the call clears; read it after the stream ran):
 *   RT_INSTANCE_BAD_BLAS   blas >= num_blas, or the table entry has count 0 or > 7, a null node or leaf pointer, or no
 *                          non-NONE slot in its root run;
 *   RT_INSTANCE_SINGULAR   object_to_world has a non-finite entry, its 3x3 part has determinant 0 (in double), or an entry of
 *                          world_to_object does not fit a float.
 *   A flagged instance gets a point proxy at the origin (v0 = v1 = v2 = 0) and its flags in its record.
 *
 * TLAS build: rt_run_bottom_up_build (plain or hybrid) or rt_run_sah_build over `proxies` (num_triangles = num_instances) with
 * enable_pairs = enable_splits = 0.  A TLAS leaf's primitive_id_0 is then the instance index.  No other builder is needed.
 *
 * rt_intersect_rays_instanced: rays, hits, mode, num_primitives (the scene-size hint: instanced triangles in total), counters,
 * alignment and the NaN / empty-range rules are rt_intersect_rays's.  Per ray:
 *   instance_ids[i]  the instance of the hit, or RT_MISS (a DEVICE uint32 array, 4-byte aligned);
 *   hits[i]          primitive_id, u, v of the BLAS's own triangles (the caller's corners, as rt_intersect_rays); t is the
 *                    world-space hit distance in units of |dir|.  An affine map preserves t, so tmin / tmax apply unchanged
 *                    in object space and one tmax is carried across instances.
 *   The world ray is tested against the TLAS; entering an instance loads its record and its rt_accel and transforms the ray:
 *   o' = W*(o, 1), d' = W3x3*d, each row ((w0*x + w1*y) + w2*z) [+ w3] in float32, 1/d' by IEEE division.  On leaving the
 *   instance the world ray is reloaded from rays[i] (never transformed back): the original bits.  An instance is never
 *   entered when its TLAS leaf's primitive_id_0 >= num_instances, its record's flags are non-zero, its blas >= num_blas, or
 *   the table entry's count is 0 or > 7.  mode RT_RAY_ANY_HIT ends the ray at its first accepted triangle in any instance.
 *   Counters: [0] box tests of both levels together, [1] triangle tests, [2] / [3] wave steps, as rt_intersect_rays.
 *   Stack: ONE 64-entry stack serves both levels (the BLAS's entries sit above the TLAS's); pushes beyond 64 are dropped, as in
 *   rt_intersect_rays, so a BLAS entered at depth k has 64 - k entries.  Identity instance over a tree: the same hit records and
 *   triangle tests as rt_intersect_rays on that tree for rays without -0 components (a transformed -0 may come out +0).
 * Both calls are asynchronous (no host copy, no synchronisation: hipGraph-capturable).
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): null pointers (blas_table may be null only when
 * num_instances = 0), instances / records / proxies / rays / hits not 16-byte aligned, blas_table not 8-, status / instance_ids
 * not 4-byte aligned, tlas->count > 7, a bad mode, num_instances > 0 with num_blas = 0.  num_instances = 0 (prepare) or num_rays = 0 (query):
 * nothing runs, except that prepare still clears *status. */
typedef struct rt_instance {
    float    object_to_world[12];   /* row-major 3x4 */
    uint32_t blas;                  /* index into the BLAS table */
    uint32_t pad[3];
} rt_instance;
typedef struct rt_instance_record {
    float    world_to_object[12];   /* row-major 3x4 */
    uint32_t blas;
    uint32_t flags;                 /* RT_INSTANCE_* of the instance; non-zero: never entered */
    uint32_t spare[2];
} rt_instance_record;
enum { RT_INSTANCE_BAD_BLAS = 1, RT_INSTANCE_SINGULAR = 2 };
int rt_prepare_instances(const rt_instance* instances, uint32_t num_instances, const rt_accel* blas_table, uint32_t num_blas,
                         rt_triangle* proxies, rt_instance_record* records, uint32_t* status, void* stream);
int rt_intersect_rays_instanced(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, rt_hit* hits,
                                uint32_t* instance_ids, uint32_t num_rays, int mode, uint32_t num_primitives,
                                uint64_t* counters, void* stream);

/* ---- instance motion (no reference counterpart).  The instanced query with a time per ray over TWO key transforms of every
 * instance: motion blur of rigid (or affinely deforming) placed meshes.  The BLASes are static trees, as in the instancing
 * block; what moves is object_to_world, and with it the TLAS.
 *
 * rt_motion_instance (caller input, 128 bytes): object_to_world0 / object_to_world1, row-major 3x4, the placement at time 0
 * and at time 1; blas as in rt_instance.  At time tau the instance is placed by the entrywise interpolated matrix
 *       w0 = 1 - tau  (once per ray);   M(tau)[k] = fl(fl(w0 * M0[k]) + fl(tau * M1[k])),  k = 0 .. 11
 * in float32, no fused multiply-add: a world point of the instance moves on the straight line between its two key positions.
 * Rotations are NOT interpolated as rotations; callers subdivide large rotations, as with any matrix-motion interface.
 * rt_motion_instance_record (128 bytes, written by rt_prepare_motion_instances, read by the query): the validated copy of the
 * input -- both matrices, blas, flags (RT_INSTANCE_*; non-zero: never entered), six spare words (0).  It holds no inverse:
 * the inverse depends on the ray's time.
 *
 * rt_prepare_motion_instances, one launch after a clear of *status, one thread per instance:
 *   - proxies0[i] / proxies1[i] are byte for byte what rt_prepare_instances writes for object_to_world0 / object_to_world1:
 *     the same object box, corner order, ordered min / max and 2^-12 pad (one copy of the arithmetic serves both calls);
 *   - RT_INSTANCE_BAD_BLAS as in rt_prepare_instances;
 *   - RT_INSTANCE_SINGULAR: a non-finite entry in either matrix, a 3x3 determinant (in double) that is 0 at either key, or
 *     determinants of opposite sign (such a motion passes through a singular matrix);
 *   - a flagged instance gets the point proxy at the origin in BOTH poses, and its flags in its record and in *status.
 *
 * TLAS: no new builder.  Build any TLAS kind over proxies0 (as in the instancing block), byte-copy its nodes_out /
 * triangles_out, rt_refit the copy with proxies1 through a plan of its own, and hand the two poses to the query as an
 * rt_motion_accel (motion block); rt_motion_validate applies as it is.  The interpolated proxy boxes bound the moving instance
 * at every time (DESIGN section 23 has the argument).
 *
 * rt_intersect_rays_instanced_motion: rt_intersect_rays_instanced with times[i] for rays[i].
 *   A ray the instanced query would not trace, and a ray whose time is NaN or outside [0, 1], is not traced: the miss record,
 *   instance id RT_MISS, no tests counted.
 *   TLAS steps read each node pair from both TLAS poses and interpolate the six bounds as the motion block does
 *   (fl(fl(w0 * a) + fl(tau * b)), w12 / w28 from pose 0).  TLAS leaves are entries as in rt_intersect_rays_instanced; the
 *   instance index is primitive_id_0 of pose 0's leaf.  An instance is not entered in the cases listed there.  Otherwise,
 *   with m = M(tau) as above, A its 3x3 part and T its translation column, all in float32 and without contraction:
 *       c00 = a11*a22 - a12*a21, c01 = a12*a20 - a10*a22, c02 = a10*a21 - a11*a20;  det = (a00*c00 + a01*c01) + a02*c02
 *       (and the other six cofactors as rt_prepare_instances's adjugate);  inv_det = 1.0f / det
 *       the instance is NOT ENTERED BY THIS RAY when det == 0, or det or inv_det is not finite
 *       W[k][j] = adj[k][j] * inv_det;   q = o - T;   o' = W*q, d' = W*d, each row (w0*x + w1*y) + w2*z;   1/d' by IEEE division
 *   Inside a BLAS the walk is rt_intersect_rays_instanced's on the static tree: stored bounds and corners (never multiplied
 *   by a weight), the one 64-entry stack, the world ray reloaded on exit, t preserved, RT_RAY_ANY_HIT ending the ray at its
 *   first accepted triangle.  Identity at both keys and a time in {0, 1/4, 1/2, 1}: W is the identity exactly.
 *   hits, instance_ids, counters, alignments and argument errors are rt_intersect_rays_instanced's, plus: times is non-null
 *   and 4-byte aligned; the four TLAS pointers are non-null when tlas->count > 0.  All argument errors are returned before
 *   any GPU work; errors win over num_rays = 0, which runs nothing.  Both calls are asynchronous and hipGraph-capturable.
 *   Cost: DESIGN section 23 has the measured ratio to rt_intersect_rays_instanced.
 *
 * Out of scope: a deforming BLAS inside a moving instance; filters; the pair-prefetch traversal; more than two key poses;
 * rotations interpolated as rotations; the C++ host mirror and rt_cli. */
typedef struct rt_motion_instance {
    float    object_to_world0[12];  /* row-major 3x4, time 0 */
    float    object_to_world1[12];  /* row-major 3x4, time 1 */
    uint32_t blas;                  /* index into the BLAS table */
    uint32_t pad[7];
} rt_motion_instance;
typedef struct rt_motion_instance_record {
    float    object_to_world0[12];
    float    object_to_world1[12];
    uint32_t blas;
    uint32_t flags;                 /* RT_INSTANCE_* of the instance; non-zero: never entered */
    uint32_t spare[6];
} rt_motion_instance_record;
int rt_prepare_motion_instances(const rt_motion_instance* instances, uint32_t num_instances, const rt_accel* blas_table,
                                uint32_t num_blas, rt_triangle* proxies0, rt_triangle* proxies1,
                                rt_motion_instance_record* records, uint32_t* status, void* stream);
int rt_intersect_rays_instanced_motion(const rt_motion_accel* tlas, const rt_motion_instance_record* records,
                                       uint32_t num_instances, const rt_accel* blas_table, uint32_t num_blas,
                                       const rt_ray* rays, const float* times, rt_hit* hits, uint32_t* instance_ids,
                                       uint32_t num_rays, int mode, uint64_t* counters, void* stream);

/* ---- sphere primitives (no reference counterpart: the reference knows triangles only).  Ray queries over a set of spheres --
 * particles, atoms, splats, proxies -- through a tree any builder makes over one PROXY TRIANGLE per sphere, the construction
 * of the instancing block with a cheaper leaf: one 16-byte record and a dozen float operations.
 *
 * rt_sphere (caller input, 16 bytes): centre, radius.  A sphere is VALID when its centre is finite and 0 <= radius < +inf.
 *
 * rt_prepare_spheres, one launch after a clear of *status, one thread per sphere.  For a valid sphere, in float32:
 *   - per axis lo = fl(c - r), hi = fl(c + r);
 *   - E = the largest |lo| or |hi| over the three axes; pad = fl(E * 2^-18); the box is [fl(lo - pad), fl(hi + pad)];
 *   - why 2^-18: the query's slab test carries at most 1.5 ulp of relative error in (bound - o) * inv, which for an origin
 *     within eight box magnitudes is about 2^-19.4 * E in space; the pad covers it with margin.  As in the instancing block,
 *     the guarantee is for rays that start within a few box magnitudes of the sphere;
 *   - proxies[i] = {v0 = lo, v1 = hi, v2 = lo*0.5f + hi*0.5f} of that box: its box is exactly the padded box and its centroid
 *     lies inside it, so it is a valid input for every builder.
 * An invalid sphere ORs RT_SPHERE_BAD into *status (a device uint32 the call clears; read it after the stream ran) and gets the
 * point proxy at the origin (v0 = v1 = v2 = 0), as a flagged instance does.
 *
 * Tree: rt_run_bottom_up_build (plain or hybrid) or rt_run_sah_build over `proxies` (num_triangles = num_spheres) with
 * enable_pairs = enable_splits = 0.  A leaf's primitive_id_0 is then the sphere index.  Pairs and splits are the caller's
 * error: the query ignores a leaf's second primitive.  Moving spheres: rt_prepare_spheres into the same proxies again, then
 * rt_refit through a plan of rt_build_refit_plan (refit block, unchanged: it refits whatever triangles_in holds), or a rebuild.
 *
 * rt_intersect_rays_spheres: rays, the [tmin, tmax] window, the NaN and empty-range rules, the miss record, the counters'
 * layout, alignment and asynchrony are rt_intersect_rays's.
 *   order == NULL: lane j takes ray j, j < num_rays; num_indices is ignored.
 *   Otherwise lane j (j < num_indices) takes i = order[j] and does nothing when i >= num_rays: rt_intersect_rays_indexed's
 *   rule, word for word (unlisted records are not written; a ray listed twice is traced twice).  rt_sort_rays reads only the
 *   root run of the tree it is given, so its order is usable on a sphere tree as it is.
 *   Box phase: the tracer's -- slab test, nearest child first, one 64-entry stack, pushes beyond 64 dropped.
 *   At a leaf: id = primitive_id_0.  The leaf is skipped when id >= num_spheres or the sphere is not valid for the query
 *   (!(r >= 0) || r == +inf; a non-finite centre rejects itself in the test).  Otherwise, with c, r the sphere, o, d the ray,
 *   in float32, every operation rounded on its own, IEEE division, correctly rounded square root:
 *       f  = o - c                                   (per axis)
 *       a  = (dx*dx + dy*dy) + dz*dz
 *       b  = -((fx*dx + fy*dy) + fz*dz)
 *       s  = b / a                                   (the parameter of closest approach)
 *       p  = f + s*d                                 (per axis fl(fx + fl(s*dx)): centre -> closest point of the line)
 *       l2 = (px*px + py*py) + pz*pz
 *       disc = r*r - l2;   !(disc >= 0): rejected (a NaN rejects)
 *       h  = sqrt(disc / a)
 *       t_near = s - h;   t_far = s + h
 *       t = t_near if tmin <= t_near <= tmax, else t_far if tmin <= t_far <= tmax, else rejected
 *   The discriminant is taken from the perpendicular offset p, not from b*b - a*c: the textbook form subtracts two numbers of
 *   the size of |f|^2 and loses all precision for a small sphere far from the ray's origin.
 *   An accepted t becomes the ray's tmax; an equal t is accepted, as for triangles, so ties go to the sphere tested later.
 *   hits[i]: t, primitive_id = the sphere index, u = 1.0f when t_far was taken (the ray began inside the sphere) else 0.0f,
 *   v = 0.  mode RT_RAY_ANY_HIT ends the ray at its first accepted sphere.
 *   Counters (optional, added to): [0] box tests, [1] sphere tests (leaves whose sphere was tested), [2] / [3] wave steps.
 * Both calls are asynchronous (no host copy, no synchronisation: hipGraph-capturable).
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null status or as; null spheres / proxies with
 * num_spheres > 0; null rays / hits with num_rays > 0; spheres / proxies / rays / hits not 16-byte aligned; status / order not
 * 4-byte aligned; as->count > 7 (or a null tree pointer with count > 0); a bad mode.  Zero counts run nothing, except that
 * prepare still clears *status.
 *
 * Spheres as a BLAS kind under a TLAS, beside triangle BLASes: the mixed-instancing block below.
 * Out of scope: mixed triangle / sphere trees (both kinds of leaf inside ONE tree); motion, filters, all-hit and first-K
 * forms; point queries against spheres; the C++ host mirror and rt_cli. */
typedef struct rt_sphere { rt_float3 center; float radius; } rt_sphere;   /* 16 bytes */
enum { RT_SPHERE_BAD = 1 };
int rt_prepare_spheres(const rt_sphere* spheres, uint32_t num_spheres, rt_triangle* proxies, uint32_t* status, void* stream);
int rt_intersect_rays_spheres(const rt_accel* as, const rt_sphere* spheres, uint32_t num_spheres, const rt_ray* rays,
                              uint32_t num_rays, const uint32_t* order, uint32_t num_indices, rt_hit* hits, int mode,
                              uint64_t* counters, void* stream);

/* ---- capsule primitives (no reference counterpart).  Ray queries over a set of CAPSULES -- round linear curve segments: a
 * segment p0..p1 swept by a sphere of one radius; bonds between atoms, fibres, hair, streamlines, cables, the link capsules of
 * a robot cell -- through a tree any builder makes over one PROXY TRIANGLE per capsule.  The sibling of the sphere block: every
 * convention not restated here is that block's.
 *
 * rt_capsule (caller input, 32 bytes, 16-byte aligned): p0, radius, p1, pad (never read).  A capsule is VALID when both end
 * points are finite and 0 <= radius < +inf.  p0 == p1 is valid (a sphere); radius == 0 is valid (a segment, which only a ray
 * through it hits).
 *
 * rt_prepare_capsules, one launch after a clear of *status, one thread per capsule.  For a valid capsule, in float32:
 *   - per axis lo = min(fl(p0 - r), fl(p1 - r)), hi = max(fl(p0 + r), fl(p1 + r));
 *   - E = the largest |lo| or |hi| over the three axes; pad = fl(E * 2^-18); the box is [fl(lo - pad), fl(hi + pad)] (the
 *     sphere block's pad and its reason: the box bounds both end spheres, hence their convex hull, and the slab test's error
 *     is a matter of the box's magnitude alone);
 *   - proxies[i] = {v0 = lo, v1 = hi, v2 = lo*0.5f + hi*0.5f} of that box.
 *   For p0 == p1 this is rt_prepare_spheres's proxy of (p0, r), bit for bit.
 * An invalid capsule ORs RT_CAPSULE_BAD into *status and gets the point proxy at the origin (v0 = v1 = v2 = 0).
 *
 * Tree: any of the three builders over `proxies` (num_triangles = num_capsules) with enable_pairs = enable_splits = 0.  A leaf's
 * primitive_id_0 is then the capsule index.  Moving capsules: rt_prepare_capsules into the same proxies again, then rt_refit
 * through a plan, or a rebuild.
 *
 * rt_intersect_rays_capsules: rays, the [tmin, tmax] window, the NaN and empty-range rules, the miss record, closest hit and
 * RT_RAY_ANY_HIT, the order list (out-of-range entries skipped; rt_sort_rays's order usable as it is), the box phase, the
 * counters' layout, alignment and asynchrony are rt_intersect_rays_spheres's.
 *   At a leaf: id = primitive_id_0.  The leaf is skipped and not counted when id >= num_capsules or !(r >= 0) || r == +inf (a
 *   non-finite end point rejects itself in the test).  Otherwise, with p0, p1, r the capsule and o, d the ray, in float32,
 *   every operation rounded on its own, IEEE division, correctly rounded square root, every dot product x.y summed as
 *   (x0*y0 + x1*y1) + x2*y2:
 *       n = p1 - p0                                  (per axis)
 *     Degenerate capsule -- nx == 0, ny == 0 and nz == 0: the sphere block's test on (c = p0, r), bit for bit; v = 0.
 *     Otherwise the ray is re-based at its point nearest the capsule's midpoint, so that no later term is of the size of
 *     |o - m|^2 (the sphere block's argument); all roots below are in tau = t - s on the ray q + tau*d:
 *       m  = p0*0.5 + p1*0.5                         (per axis fl(fl(p0*0.5) + fl(p1*0.5)))
 *       f  = o - m
 *       a  = d.d;   b = -(f.d);   s = b / a
 *       q  = f + s*d                                 (per axis fl(fx + fl(s*dx)))
 *       nn = n.n;  nd = n.d;  nq = n.q;  qd = q.d;  qq = q.q
 *       A  = nn*a - nd*nd                            (fl(fl(nn*a) - fl(nd*nd)), and so below)
 *       C  = nn*(qq - r*r) - nq*nq
 *       hn = nn*0.5                                  (the body spans -hn < y < hn, y = n.(point - m))
 *     cap(g), the roots of an end sphere whose centre lies at -g from q -- the sphere block's steps with f = g:
 *       bg = -(g.d);  sg = bg / a;  pg = g + sg*d;  l2 = pg.pg;  disc = r*r - l2;  ok = disc >= 0
 *       hh = sqrt(disc / a);  near = sg - hh;  far = sg + hh
 *       p0's cap is cap(fa), fa = q + 0.5*n (per axis fl(qx + fl(0.5*nx))); p1's is cap(fb), fb = q - 0.5*n.
 *     A > 0 (the ray is not parallel to the axis):
 *       B  = nn*qd - nq*nd;   h = B*B - A*C;   !(h >= 0): rejected
 *       tau1 = (-B - sqrt(h)) / A;   tau2 = (-B + sqrt(h)) / A
 *       y1 = nq + tau1*nd;   y2 = nq + tau2*nd
 *       entry: tau1 with v = y1/nn + 0.5 (fl(fl(y1/nn) + 0.5)) when y1 > -hn and y1 < hn; else p0's cap's near root with v = 0
 *              when y1 <= -hn; else p1's cap's near root with v = 1.  A cap that is not ok: rejected.
 *       exit:  the same with tau2, y2 and the caps' far roots.
 *       The cap is chosen by the cylinder root's side and a cap root is never tested for its own side: no crack at the seams.
 *     !(A > 0) (parallel; a rounded-negative or NaN A included):
 *       C > 0: rejected.  entry = the near root of p0's cap (v = 0) when nd > 0, else of p1's cap (v = 1); exit = the far root
 *       of the other cap (v = 1 when nd > 0, else 0).  Either cap not ok: rejected.
 *     Window:
 *       t_near = s + entry;   t_far = s + exit
 *       t = t_near if tmin <= t_near <= tmax, else t_far if tmin <= t_far <= tmax (the ray began inside), else rejected
 *   An accepted t becomes the ray's tmax; an equal t is accepted, so ties go to the capsule tested later.
 *   hits[i]: t, primitive_id = the capsule index, u = 1.0f when t_far was taken else 0.0f (the sphere record's u), v = the
 *   axial parameter of the crossing taken: in (0, 1) on the body, exactly 0.0f on p0's cap, exactly 1.0f on p1's cap, 0.0f for
 *   a degenerate capsule -- whose record is therefore rt_intersect_rays_spheres's, byte for byte.
 *   Counters (optional, added to): [0] box tests, [1] capsule tests (leaves whose capsule was tested), [2] / [3] wave steps.
 * Both calls are asynchronous (no host copy, no synchronisation: hipGraph-capturable).
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null status or as; null capsules / proxies with
 * num_capsules > 0; null rays / hits with num_rays > 0; capsules / proxies / rays / hits not 16-byte aligned; status / order
 * not 4-byte aligned; as->count > 7 (or a null tree pointer with count > 0); a bad mode.  Zero counts run nothing, except that
 * prepare still clears *status.
 *
 * Capsules as a BLAS kind under a TLAS, beside triangle and sphere BLASes (rt_geometry's RT_GEOM_CAPSULES):
 * rt_intersect_rays_instanced_mixed_capsules below.
 * Out of scope: per-vertex radii (cone-spheres); motion, filters, all-hit and first-K forms; point queries against capsules;
 * capsules and other kinds in one tree; the C++ host mirror and rt_cli. */
typedef struct rt_capsule { rt_float3 p0; float radius; rt_float3 p1; uint32_t pad; } rt_capsule;   /* 32 bytes; pad not read */
enum { RT_CAPSULE_BAD = 1 };
int rt_prepare_capsules(const rt_capsule* capsules, uint32_t num_capsules, rt_triangle* proxies, uint32_t* status, void* stream);
int rt_intersect_rays_capsules(const rt_accel* as, const rt_capsule* capsules, uint32_t num_capsules, const rt_ray* rays,
                               uint32_t num_rays, const uint32_t* order, uint32_t num_indices, rt_hit* hits, int mode,
                               uint64_t* counters, void* stream);

/* ---- sphere cast (no reference counterpart).  How far can a BALL of radius rad travel along a ray before it touches the mesh,
 * and where does it touch: the sweep of collision and motion-planning callers (character controllers, camera booms, continuous
 * collision of sphere-swept links).  A query over the triangle trees rt_intersect_rays takes -- LBVH, pairs, hybrid, SAH, SAH
 * with pairs and / or splits, refitted trees, runs of 1 to 7 slots, the empty tree.  No builder, no prepare step.  A ball
 * swept against a triangle is a ray against the triangle's Minkowski sum with the ball: two offset faces, three edge capsules
 * whose end spheres are the corners.  Every convention not restated here is rt_intersect_rays_spheres's (sphere block).
 *
 * rays: rt_intersect_rays's; t is in units of |dir|.  radii[i] is the world-space radius of the ball whose centre travels
 * along rays[i]; radii == NULL gives every ray `radius`.  A ray is NOT TRACED (the miss record, RT_SWEEP_NONE, no test
 * counted) when the ray query would not trace it or its radius is negative, NaN or +inf.  order, num_indices and mode are
 * rt_intersect_rays_spheres's; radii, hits and features are indexed by ray index.
 *
 * Box phase: the tracer's -- slab test, ordered compares, nearest child first with the index tie rule, one 64-entry stack,
 * pushes beyond 64 dropped -- on GROWN boxes: every slot's box is [fl(lo - e), fl(hi + e)] per axis, e made once per ray:
 *       rad == 0: the boxes as stored (growth exactly 0)
 *       else      M   = the largest |lo| or |hi| over the three axes of the slots of the root run (as->root, as->count) whose
 *                       type is not "none"
 *                 pad = fl(2^-18 * max(rad, M));   e = fl(rad + pad)
 *   The contact point lies on the triangle, hence in the leaf's box (in a split tree: in some reference's clipped box), so the
 *   centre at contact lies in that box grown by rad.  pad plays the sphere block's role: the slab test carries about 1.5 ulp
 *   of relative error in (bound - o) * inv, and a grown bound is no larger than M + rad in magnitude, so for an origin within
 *   a few such magnitudes 2^-18 * max(rad, M) covers it with margin.
 *
 * At a leaf: one test is counted per leaf visited, as in the ray query.  Triangle A = (v0, v1, v2) is tested, then triangle
 * B = (v2, v1, v3) unless v3 == v2 bit for bit (the ray query's skip); any-hit tests B after a hit on A as well, as the ray
 * query does.  A pair's shared edge v1-v2 is tested TWICE, once as A's and once as B's.
 * Per triangle with STORED corners s0, s1, s2, primitive id and rotation, in float32, every operation rounded on its own, IEEE
 * division, correctly rounded square root, every dot product x.y summed as (x0*y0 + x1*y1) + x2*y2:
 *   rad == 0: rt_intersect_rays's triangle test alone (Moller-Trumbore on the stored corners, epsilon 1e-9, t in [tmin, tmax]).
 *     The records, counters[0] and counters[1] of such rays are rt_intersect_rays's, byte for byte.  Feature: RT_SWEEP_FACE.
 *   rad > 0:
 *   1. Initial overlap.
 *       c0 = o + tmin*d                              (per axis fl(ox + fl(tmin*dx)))
 *       D  = d2(c0, a, b, c) of the closest-point block, (a, b, c) the CALLER's corners (the stored ones un-rotated, as the
 *            range query takes them), with its weights (u, v) of b and c
 *       D <= fl(rad*rad): accepted with t = tmin, the record's (u, v) = those weights (+ 0: a -0 is written as +0, as
 *       rt_closest_points writes them), RT_SWEEP_OVERLAP.  This is
 *       rt_range_count's predicate in sphere shape on (c0, fl(rad*rad)), bit for bit.  Nothing else of the triangle is tested.
 *   2. Otherwise the ball starts outside the convex sum and the candidates below are tried IN THIS ORDER, each against the
 *      current tmax: a candidate t is accepted when tmin <= t <= tmax and becomes tmax, so of equal candidates the later wins.
 *      Only entry roots are candidates; no far root is ever taken.
 *     a. The facing offset face.
 *       e1 = s1 - s0;  e2 = s2 - s0;  n = e1 x e2    (nx = fl(fl(e1y*e2z) - fl(e1z*e2y)), cyclic)
 *       len = sqrt(n.n);   !(len > 0): no face candidate (zero area, a NaN)
 *       dn = d.n;   k = -rad when dn < 0, else rad
 *       o' = o + k*(n/len)                           (per axis fl(ox + fl(k * fl(nx/len))): the origin shifted TOWARD the triangle
 *                                                     by rad, so the shifted ray meets the triangle where the centre's ray meets
 *                                                     the offset face that looks at it)
 *       rt_intersect_rays's triangle test on (o', d, tmin, tmax) and the stored corners: its t, and its (bu, bv) as the weights of
 *       s1 and s2.  RT_SWEEP_FACE.
 *     b. The edges (s0, s1), (s1, s2), (s2, s0).  For an edge (pa, pb): the ENTRY of the capsule block's test of (p0 = pa,
 *        p1 = pb, r = rad), that block's steps and names:
 *       n == 0 exactly (a degenerate edge): the sphere block's steps about c = pa: t = t_near when disc >= 0, axial v = 0.
 *       else m, f, a, b, s, q, nn, nd, nq, qd, qq, A, C, hn as there, and
 *         A > 0:   B, h as there; !(h >= 0): none.  tau1, y1 as there; entry = tau1 with v = fl(fl(y1/nn) + 0.5) when
 *                  -hn < y1 < hn, else the NEAR root of pa's end sphere (y1 <= -hn; v = 0) or pb's (v = 1); not ok: none
 *         else:    C > 0: none.  entry = the near root of pa's end sphere (v = 0) when nd > 0, else of pb's (v = 1); not ok: none
 *         t = fl(s + entry)
 *       The block's exit (tau2, the far roots) is not evaluated.  Weights of (s1, s2) at axial v: (v, 0) on (s0, s1);
 *       (fl(1 - v), v) on (s1, s2); (0, fl(1 - v)) on (s2, s0).  RT_SWEEP_EDGE when 0 < v < 1, else RT_SWEEP_CORNER (v is exactly
 *       0 or 1 there: the capsule block's guarantee).
 *   3. An accepted t becomes the ray's tmax for every later part, triangle and box; RT_RAY_ANY_HIT ends the ray after the leaf
 *      of its first accepted triangle.
 * hits[i]: t = the centre's parameter at first contact; primitive_id = the caller's triangle; (u, v) = the weights of the
 * CONTACT POINT ON THE TRIANGLE for the caller's corners v1 and v2 -- for an overlap as step 1 gives them, else the stored
 * corners' (bu, bv) mapped through the leaf's rotations exactly as rt_intersect_rays maps its own.  The contact normal is
 * (o + t*d - contact) / rad.  A miss is rt_intersect_rays's miss record.
 * features (optional, 4-byte aligned device uint32 per ray): which part was touched, RT_SWEEP_NONE on a miss.
 * Counters (optional, added to): [0] box tests, [1] leaves visited, [2] / [3] wave steps.
 * The call is asynchronous (no host copy, no synchronisation: hipGraph-capturable).
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT), also when num_rays == 0: a null as; as->count > 7 (or
 * a null tree pointer with count > 0); a bad mode; rays / hits not 16-byte aligned; order / radii / features not 4-byte aligned;
 * radii == NULL with a radius that is negative, NaN or infinite; null rays / hits with num_rays > 0.  num_rays == 0, or an
 * order list with num_indices == 0, runs nothing.
 *
 * Out of scope: swept capsules or boxes; instanced, motion, filtered, all-hit and first-K forms; sweeps over sphere or capsule
 * trees; the C++ host mirror and rt_cli. */
enum { RT_SWEEP_NONE = 0, RT_SWEEP_FACE = 1, RT_SWEEP_EDGE = 2, RT_SWEEP_CORNER = 3, RT_SWEEP_OVERLAP = 4 };
int rt_sphere_cast(const rt_accel* as, const rt_ray* rays, const float* radii, float radius, uint32_t num_rays,
                   const uint32_t* order, uint32_t num_indices, rt_hit* hits, uint32_t* features, int mode,
                   uint64_t* counters, void* stream);

/* ---- mixed instancing (no reference counterpart).  The instanced ray query over a BLAS table whose trees hold triangles OR
 * spheres: a surface mesh with atoms, particles inside geometry, sphere-swept obstacles in a robot cell -- one TLAS, one walk,
 * one tmax across both kinds, an any-hit ray that stops at the first primitive of either.  Nothing new is prepared or built:
 * rt_prepare_instances reads only the root run's boxes of a BLAS, so a sphere tree (sphere block) is a valid BLAS for it as it
 * is, and the TLAS is the instancing block's.
 *
 * rt_geometry (16 bytes; a DEVICE array parallel to the BLAS table, 16-byte aligned): what the leaves of blas_table[b] hold.
 *   kind   RT_GEOM_TRIANGLES: any tree rt_intersect_rays_instanced takes; data and count are not read.
 *          RT_GEOM_SPHERES: a tree built by any builder over rt_prepare_spheres's proxies with enable_pairs = enable_splits = 0
 *          (sphere block); data = the const rt_sphere* array the proxies were made from (16-byte aligned: the caller's duty, it
 *          is a device value no host check sees), count = num_spheres.
 *
 * rt_intersect_rays_instanced_mixed: everything rt_intersect_rays_instanced says holds word for word -- the records and the TLAS
 * over rt_prepare_instances's proxies, rays, hits, instance_ids, mode, alignment, the NaN and empty-range rules, ONE 64-entry
 * stack shared by both levels, the object-space ray (o' = W*(o, 1), d' = W3x3*d, row by row, 1/d' by IEEE division), the world
 * ray reloaded from rays[i] on leaving an instance, the cases in which an instance is never entered, asynchronous execution and
 * hipGraph capture.  There is NO num_primitives hint and no pair-prefetch arm, as in the sphere and instance-motion queries.
 *   Entering an instance: its record, then blas_table[blas] (three 8-byte loads), then geom_table[blas] as ONE 16-byte load.
 *   Besides rt_intersect_rays_instanced's cases an instance is NOT ENTERED when kind is neither RT_GEOM_TRIANGLES nor
 *   RT_GEOM_SPHERES (an RT_GEOM_CAPSULES entry included: the capsule block of mixed instancing below has the call that enters
 *   it), or kind == RT_GEOM_SPHERES and data is null.  count == 0 enters the instance and tests nothing.
 *   Triangle BLAS: the walk, the leaf test and the record are rt_intersect_rays_instanced's: t, primitive_id, (u, v) for the
 *   caller's corners through the leaf's rotations.
 *   Sphere BLAS: the box phase is the same, on the object-space ray.  At a leaf, with the object-space ray, the sphere
 *   block's steps in its order: id = the leaf's primitive_id_0 (its first 16 bytes); the leaf is skipped when id >= count;
 *   data[id] as one 16-byte load; the sphere is skipped when !(r >= 0) || r == +inf; one test is counted; the sphere block's
 *   test, operation by operation.  An affine map preserves t and the test never assumes a unit direction (a = |d'|^2), so t is
 *   the world-space distance in units of |dir|; under a non-uniform object_to_world the sphere is an ellipsoid in the world.
 *   The record is rt_intersect_rays_spheres's: t, primitive_id = the sphere index, u = 1.0f when t_far was taken else 0.0f,
 *   v = 0.  The caller tells the two record shapes apart by instance_ids[i] -> records[].blas -> geom_table[].kind.
 *   One tmax runs across all instances of both kinds; an equal t is accepted, so ties go to the primitive tested later.
 *   mode RT_RAY_ANY_HIT ends the ray at the first accepted primitive of either kind.
 *   Counters (optional, added to): [0] box tests of both levels together, [1] triangle-leaf tests plus sphere tests, each
 *   counted as rt_intersect_rays_instanced / rt_intersect_rays_spheres counts them, [2] / [3] wave steps.
 *   Identity instance over a sphere tree: the same hit records and sphere tests as rt_intersect_rays_spheres on that tree for
 *   rays without -0 components.  A table of RT_GEOM_TRIANGLES only: the same hits, instance ids, box and triangle tests as
 *   rt_intersect_rays_instanced with num_primitives = 0.
 * geom_table == NULL: every BLAS holds triangles -- the call IS rt_intersect_rays_instanced with num_primitives = 0 (its
 * argument checks, its kernel), as filter == NULL in the filtered calls.
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): rt_intersect_rays_instanced's, and geom_table not
 * 16-byte aligned.  Errors win over num_rays = 0, which runs nothing.
 *
 * Out of scope: filtered, motion, indexed, all-hit and first-K mixed forms of THIS call (the indexed one is an entry point of its
 * own, rt_intersect_rays_instanced_mixed_indexed: the indexed-instanced block below); triangles and spheres inside one BLAS; the
 * C++ host mirror and rt_cli. */
enum { RT_GEOM_TRIANGLES = 0, RT_GEOM_SPHERES = 1 };
typedef struct rt_geometry {      /* 16 bytes; DEVICE array parallel to the BLAS table */
    const void* data;             /* RT_GEOM_SPHERES: const rt_sphere*, 16-byte aligned (caller's duty); TRIANGLES: not read */
    uint32_t    count;            /* RT_GEOM_SPHERES: num_spheres; TRIANGLES: not read */
    uint32_t    kind;             /* RT_GEOM_* (RT_GEOM_CAPSULES: the capsule block of mixed instancing, below) */
} rt_geometry;
int rt_intersect_rays_instanced_mixed(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                      const rt_accel* blas_table, const rt_geometry* geom_table, uint32_t num_blas,
                                      const rt_ray* rays, rt_hit* hits, uint32_t* instance_ids, uint32_t num_rays,
                                      int mode, uint64_t* counters, void* stream);

/* ---- mixed instancing with capsules (no reference counterpart).  Capsule BLASes as a third kind of the mixed instanced query:
 * bonds between atoms, fibres on a mesh, cables, the link capsules of a robot cell are capsule sets PLACED by a transform next to
 * meshes and sphere sets -- one TLAS, one walk, one tmax across the three kinds, an any-hit ray that stops at the first primitive
 * of any of them.  Nothing new is prepared or built: rt_prepare_instances reads only a BLAS's root run, so a capsule tree
 * (capsule block) is a valid BLAS as it is.
 *
 * RT_GEOM_CAPSULES (a third value of rt_geometry's kind): a tree built by any builder over rt_prepare_capsules's proxies with
 * enable_pairs = enable_splits = 0; data = the const rt_capsule* array the proxies were prepared from (16-byte aligned: the
 * caller's duty), count = num_capsules.
 *
 * rt_intersect_rays_instanced_mixed_capsules: order == NULL is the direct form (num_indices is not read) and everything
 * rt_intersect_rays_instanced_mixed says holds word for word; with order != NULL everything
 * rt_intersect_rays_instanced_mixed_indexed says holds (launch position j takes ray order[j]; positions past num_indices and
 * entries >= num_rays do nothing; hits and instance_ids are written at the ray's index, unlisted records untouched).
 *   Entering an instance: an instance is NOT ENTERED when kind is none of the three RT_GEOM_* values, or kind is
 *   RT_GEOM_SPHERES or RT_GEOM_CAPSULES and data is null.  count == 0 enters the instance and tests nothing.
 *   Triangle and sphere BLASes: as in rt_intersect_rays_instanced_mixed, bit for bit -- a table without capsule entries gives
 *   that call's hits, instance ids, box tests and primitive tests.
 *   Capsule BLAS: the box phase is the same, on the object-space ray.  At a leaf, with the object-space ray, the capsule
 *   block's steps in its order: id = the leaf's primitive_id_0 (its first 16 bytes); the leaf is skipped when id >= count;
 *   data[id] as two independent 16-byte loads; the capsule is skipped when !(r >= 0) || r == +inf; one test is counted; the
 *   capsule block's test, operation by operation.  The test never assumes a unit direction (a = d'.d' stands in every root)
 *   and an affine map preserves t, so t is the world-space distance in units of |dir|; under a non-uniform or sheared
 *   object_to_world the world shape is the affine image of the capsule (an elliptic cylinder with ellipsoidal caps), not a
 *   capsule.  The record is rt_intersect_rays_capsules's: t, primitive_id = the capsule index, u = 1.0f when t_far was taken
 *   else 0.0f, v = the axial parameter (of the object-space capsule).  A capsule with p0 == p1 gives the sphere arm's record
 *   for the sphere (p0, r), byte for byte.  The caller tells the three record shapes apart by instance_ids[i] ->
 *   records[].blas -> geom_table[].kind.
 *   One tmax runs across all instances of the three kinds; an equal t is accepted, so ties go to the primitive tested later.
 *   mode RT_RAY_ANY_HIT ends the ray at the first accepted primitive of any kind.
 *   Counters (optional, added to): [0] box tests of both levels together, [1] triangle-leaf tests plus sphere tests plus
 *   capsule tests, each counted as its own query counts them, [2] / [3] wave steps.
 *   Identity instance over a capsule tree: the same hit records and capsule tests as rt_intersect_rays_capsules on that tree
 *   for rays without -0 components.
 * The kernels are this call's own (a register bound of their own): rt_intersect_rays_instanced_mixed[_indexed] run the kernels
 * they ran before this call existed and still do not enter an RT_GEOM_CAPSULES entry.
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): geom_table == NULL (there is no all-triangle
 * shortcut here) or not 16-byte aligned; order not 4-byte aligned; every other error of the two siblings.  Errors win over
 * num_rays = 0 and over num_indices = 0 with an order list, which run nothing.
 *
 * Out of scope: filtered, motion, all-hit and first-K forms; a stack-depth pin for a capsule BLAS entered deep in a TLAS (it
 * needs a mixed two-level walker in the test oracle); kinds mixed inside one BLAS; shading of capsule hits; the C++ host mirror
 * and rt_cli. */
enum { RT_GEOM_CAPSULES = 2 };    /* rt_geometry.kind: data = const rt_capsule*, 16-byte aligned; count = num_capsules */
int rt_intersect_rays_instanced_mixed_capsules(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                               const rt_accel* blas_table, const rt_geometry* geom_table, uint32_t num_blas,
                                               const rt_ray* rays, uint32_t num_rays, const uint32_t* order, uint32_t num_indices,
                                               rt_hit* hits, uint32_t* instance_ids, int mode, uint64_t* counters, void* stream);

/* ---- closest-point queries (no reference counterpart).  For each caller point: which triangle is nearest, where on it, and
 * how far away -- through any tree rt_intersect_rays takes (runs of 1..7 slots; an empty tree, count = 0, is accepted and
 * every query misses).
 *
 * rt_point_query (16 bytes): p, dist2_max -- a squared search radius, +inf allowed.  A query with a non-finite component of p,
 * a NaN dist2_max or a negative dist2_max is not traced: its record is a miss and no tests are counted for it.
 * rt_point_hit (16 bytes): dist2, primitive_id (the caller's triangle index; a split reference reports its original triangle),
 * u, v (the weights of the caller's corners v1 and v2 at the closest point, from d2 below).  A miss is {+inf, RT_MISS, 0, 0}.
 *
 * d2(p, v0, v1, v2), float32, evaluated on the caller's corners in the caller's order (pair leaves: the stored corners are put
 * back through rt_triangle_pair.rotations first, A with rotations[0], B = (v2, v1, v3) with rotations[1]; r = 1: caller
 * corners = stored (s1, s2, s0), r = 2: (s2, s0, s1), else as stored).  With a = v0, b = v1, c = v2, every subtraction
 * componentwise, dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z, guard(n, d) = (d > 0 ? n / d : 0) (IEEE division) and
 * clamp01(t) = min(max(t, 0), 1) by selects (NaN -> 0):
 *   1. closest point q, Ericson's ClosestPtPointTriangle (Real-Time Collision Detection 5.1.5), first region that holds:
 *        ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap)
 *        d1 <= 0 && d2 <= 0                      q = a                       (u, v) = (0, 0)
 *        bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp)
 *        d3 >= 0 && d4 <= d3                     q = b                       (1, 0)
 *        vc = d1*d4 - d3*d2, t_ab = clamp01(guard(d1, d1 - d3))
 *        vc <= 0 && d1 >= 0 && d3 <= 0 && d1 - d3 > 0            q = a + t_ab*ab     (t_ab, 0)
 *        cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp)
 *        d6 >= 0 && d5 <= d6                     q = c                       (0, 1)
 *        vb = d5*d2 - d1*d6, t_ac = clamp01(guard(d2, d2 - d6))
 *        vb <= 0 && d2 >= 0 && d6 <= 0 && d2 - d6 > 0            q = a + t_ac*ac     (0, t_ac)
 *        va = d3*d6 - d5*d4, e43 = d4 - d3, e56 = d5 - d6, t_bc = clamp01(guard(e43, e43 + e56)), bc = c - b
 *        va <= 0 && e43 >= 0 && e56 >= 0 && e43 + e56 > 0        q = b + t_bc*bc     (1 - t_bc, t_bc)
 *      (the fourth term of an edge region is the edge's squared length: an edge of two equal corners has no region, so a
 *      triangle with a repeated corner is answered through its other edges)
 *        s = (va + vb) + vc, fv = vb / s, fw = vc / s, face point f = (a + ab*fv) + ac*fw,
 *        noise = ((|d1*d4| + |d3*d2|) + (|d5*d2| + |d1*d6|)) + (|d3*d6| + |d5*d4|), FACE_NOISE = 2^-20
 *        s > FACE_NOISE * noise                  q = f                       (fv, fw)
 *                                                (false for a NaN and for an infinite noise: products beyond float range)
 *        otherwise                               s is the rounding noise of its six products (a collinear triangle: va, vb, vc
 *                                                are residues of any sign, and f alone may lie anywhere along the triangle or
 *                                                off it): the nearest of the three edge points a + t_ab*ab, a + t_ac*ac,
 *                                                b + t_bc*bc by the float dist2 of steps 2-3 (ties: AB, then AC), with their
 *                                                weights -- unless s > 0, fv >= 0, fw >= 0, fv + fw <= 1 and no edge point is
 *                                                strictly nearer than f: then f, (fv, fw);
 *   2. clamp: q = fminf(fmaxf(q, lo), hi) componentwise, lo / hi = fminf / fmaxf of the three corners (the vertex box);
 *   3. dist2 = (dx*dx + dy*dy) + dz*dz, d = p - q.  u, v are returned + 0 (a -0 becomes +0).
 * The clamp is a projection onto a convex set that holds the triangle, so it only moves q toward the true closest point.  It
 * also makes pruning exact: a slot box that contains the vertex box gives boxdist2 = (gx*gx + gy*gy) + gz*gz, g = max(lo - p,
 * p - hi, 0) per axis, and since float subtraction, squaring and addition are monotone, dist2 >= boxdist2 holds in float32
 * exactly, for any input (a NaN from overflow still clamps into the box).
 *
 * Result: the lexicographic minimum of (dist2, primitive_id) over every triangle with dist2 <= dist2_max (ties on dist2 go to
 * the lower id; the search starts from (dist2_max, RT_MISS), so a triangle exactly at the radius is accepted).  A slot or a
 * popped entry is skipped only when boxdist2 > best (never on equality).  The result does not depend on the visiting order:
 *   - exact (bit for bit the brute force over the caller's triangles) on every tree whose slot boxes contain the vertex boxes
 *     below them: LBVH, pairs, hybrid, hybrid + pairs, SAH, SAH + pairs, and every refitted tree (refit writes unclipped boxes);
 *   - spatial-split trees (rt_run_sah_build with enable_splits) clip leaf boxes to grid cells, so a triangle may be pruned
 *     through a reference whose clipped box is farther than the triangle.  There dist2 is still d2(p, tri[primitive_id]) bit
 *     for bit, and sqrt(dist2) exceeds the brute-force minimum by at most 2^-20 * M, M = the largest coordinate magnitude of
 *     p and the scene box.  Refitting a split tree restores exactness.
 * Range: with coordinate differences beyond about 2^31 Ericson's products (degree 4) overflow; results there stay
 * deterministic and equal to the restatement above, but are not accurate.
 *
 * rt_closest_points: hits[i] for queries[i], i < num_queries; hits[i >= num_queries] are not written.  queries / hits:
 * 16-byte aligned device arrays.  counters: optional device uint64[4], rt_intersect_rays's layout: [0] += box tests (non-NONE
 * slots examined), [1] += triangle tests (leaf records visited); [2] / [3] are not touched (no wave phases); one LDS
 * reduction + 2 device atomics per workgroup of 256 queries.  status: optional device uint32 the call ORs flags into (the
 * caller clears it).  Stack: 64 pending entries per query; a push beyond them is dropped.  A traversal that dropped a push is
 * run again from the root with the best record so far (which prunes everything farther), at most twice; a traversal that
 * drops nothing makes the record exact.  RT_POINT_STACK_OVERFLOW: the last traversal of a query still dropped a push -- its
 * record is an exact (d2, id) of a real triangle but may not be the nearest.  Asynchronous (no host copy, no synchronisation:
 * hipGraph-capturable).
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null as / queries / hits, a tree with count > 0
 * and a null node or leaf pointer, count > 7, queries or hits not 16-byte aligned, status not 4-byte aligned.
 * num_queries = 0: nothing runs. */
typedef struct rt_point_query { rt_float3 p; float dist2_max; } rt_point_query;
typedef struct rt_point_hit { float dist2; uint32_t primitive_id; float u, v; } rt_point_hit;
enum { RT_POINT_STACK_OVERFLOW = 1 };
int rt_closest_points(const rt_accel* as, const rt_point_query* queries, rt_point_hit* hits, uint32_t num_queries,
                      uint64_t* counters, uint32_t* status, void* stream);

/* ---- range queries (no reference counterpart).  For each caller region: WHICH triangles touch it -- the set-valued query,
 * through any tree rt_intersect_rays takes (runs of 1..7 slots; an empty tree, count = 0, is accepted and every set is empty).
 * The output length depends on the data, so the result is compressed sparse rows (CSR): offsets[0 .. n] (uint64) and one id
 * array; query i owns ids[offsets[i] .. offsets[i+1]).
 *
 * shape RT_RANGE_SPHERE: queries is an array of rt_point_query (p, dist2_max; 16 bytes).  Triangle k matches iff
 *   d2(p, tri[k]) <= dist2_max, with d2 EXACTLY the closest-point block's float32 routine (Ericson, the clamp into the vertex
 *   box, the squared distance), evaluated on the caller's corners in the caller's order (pair leaves go back through
 *   rt_triangle_pair.rotations, as there).  A triangle exactly at the radius matches; a NaN d2 (overflow) does not.
 *   A slot is skipped iff boxdist2 > dist2_max (the closest-point block's boxdist2; never on equality).  Since
 *   d2 >= boxdist2 holds in float32 for every box that contains the vertex box, skipping loses nothing.
 *   Not traced (count 0, no tests counted): a non-finite component of p, a NaN dist2_max or a negative dist2_max.  +inf is a
 *   legal radius: every triangle with a non-NaN d2 matches.
 * shape RT_RANGE_BOX: queries is an array of rt_range_box (lo, hi; 32 bytes, the pad words are not read).  Triangle k matches
 *   iff its vertex box overlaps [lo, hi] on every axis with closed comparisons: tlo <= hi && thi >= lo, tlo / thi = fminf /
 *   fmaxf of the three corners (a NaN coordinate is dropped by fminf / fmaxf; -0 equals +0).  This is the broad-phase candidate
 *   set: nothing but min, max and comparisons, so nothing rounds.  A slot is skipped iff its box fails the same closed test
 *   against [lo, hi].
 *   Not traced: a NaN component of lo or hi, or lo > hi on an axis.
 *
 * Result: a SET -- no ordering promise and no tie rule.
 *   - exact (the brute-force set over the caller's triangles, each id once) on every tree whose slot boxes contain the vertex
 *     boxes below them: LBVH, pairs, hybrid, hybrid + pairs, SAH, SAH + pairs, and every refitted tree;
 *   - spatial-split trees (rt_run_sah_build with enable_splits): the leaf test is on the whole triangle, so every reported id
 *     is a true match; but an id appears once per REFERENCE that is reached (duplicates are possible), and in box mode a
 *     triangle is missed when every one of its clipped references lies outside the query (sphere mode: when every clipped
 *     reference box is farther than dist2_max).  Refitting a split tree restores exactness up to the duplicates: refit writes
 *     unclipped boxes, but the references stay.
 *   Order: the ids of a query come in the traversal order of its lane -- deterministic for a given tree, the same in
 *   rt_range_count and rt_range_collect (one traversal, compiled twice), otherwise unspecified.
 *
 * rt_range_count: offsets[0 .. num_queries] = the exclusive prefix sum of the per-query match counts; offsets[num_queries] is
 *   the total.  64-bit: no overflow case exists.  scratch: rt_range_scratch_bytes(num_queries) bytes of device memory,
 *   256-byte aligned, no initialisation needed (one uint64 per 256 queries: the workgroup sums of the scan).  Launches: the
 *   traversal (which also scans the counts inside each workgroup), one workgroup over the workgroup sums, one add.
 *   num_queries = 0 still writes offsets[0] = 0.
 * rt_range_collect: query i writes its first min(matches, offsets[i+1] - offsets[i]) ids at ids + offsets[i] and never writes
 *   beyond them (offsets[i+1] < offsets[i] counts as no room); ids past the last segment and segments of other queries are not
 *   touched.  counts (optional, device uint32[num_queries]): the query's true match count, room or not.  A query with more
 *   matches than room ORs RT_RANGE_TRUNCATED into *status; its segment then holds the first matches in traversal order.
 *   Two call patterns: (a) everything: rt_range_count, read offsets[num_queries] back, allocate ids, rt_range_collect with the
 *   same offsets; (b) a fixed K per query: fill offsets[i] = i * K once, one rt_range_collect pass, counts says how many of
 *   each segment are valid (min(counts[i], K)).  num_queries = 0: nothing runs.
 * Both calls: counters, optional device uint64[4], rt_closest_points's layout: [0] += box tests (non-NONE slots examined), [1]
 * += triangle tests (leaf records visited); [2] / [3] are not touched.  The same query set gives the same counters in both
 * calls.  status: optional device uint32 the calls OR flags into (the caller clears it).  Stack: 64 pending entries per query;
 * a push beyond them is dropped and sets RT_RANGE_STACK_OVERFLOW: the result is then a subset of the true set, and since both
 * calls drop the same pushes they still agree with each other.  Asynchronous (no host copy, no synchronisation:
 * hipGraph-capturable).
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null as / queries / offsets / scratch (count) /
 * ids (collect), a tree with count > 0 and a null node or leaf pointer, count > 7, an unknown shape, queries not 16-byte,
 * offsets not 8-byte, ids / counts / status not 4-byte, scratch not 256-byte aligned. */
typedef struct rt_range_box { rt_float3 lo; uint32_t pad0; rt_float3 hi; uint32_t pad1; } rt_range_box;
enum { RT_RANGE_SPHERE = 0, RT_RANGE_BOX = 1 };
enum { RT_RANGE_STACK_OVERFLOW = 1, RT_RANGE_TRUNCATED = 2 };
size_t rt_range_scratch_bytes(uint32_t num_queries);
int rt_range_count(const rt_accel* as, const void* queries, uint32_t num_queries, int shape, uint64_t* offsets, void* scratch,
                   uint64_t* counters, uint32_t* status, void* stream);
int rt_range_collect(const rt_accel* as, const void* queries, uint32_t num_queries, int shape, const uint64_t* offsets,
                     uint32_t* ids, uint32_t* counts, uint64_t* counters, uint32_t* status, void* stream);

/* ---- k-nearest queries (no reference counterpart).  For each caller point: the K nearest triangles, in order -- through any
 * tree rt_intersect_rays takes (runs of 1..7 slots; an empty tree, count = 0, is accepted and every row is misses).  The
 * fixed-length sibling of the sphere range query: row i of the output has exactly k records, so nothing is counted, scanned or
 * read back.
 *
 * Candidate set.  For query i = (p, dist2_max), an rt_point_query: S_i = { (d2(p, tri[t]), t) : d2 <= dist2_max }, with d2
 * EXACTLY the closest-point block's float32 routine (Ericson, the clamp into the vertex box, the squared distance), evaluated on
 * the caller's corners in the caller's order (pair leaves go back through rt_triangle_pair.rotations, as there).  A NaN d2
 * (overflow) is not in S_i; a triangle exactly at the radius is.  +inf is a legal radius.
 * Output row.  Row i is out[i*k .. i*k + k) (64-bit indexing), rt_knn_hit records of 8 bytes (dist2, primitive_id).  It holds
 * the m = min(k, |S_i|) smallest elements of S_i in ascending (dist2, primitive_id) order: ties on dist2 go to the lower id.
 * Entries j >= m are {+inf, RT_MISS}.  Rows at i >= num_queries are not written.  The row holds no u, v: a caller who needs the
 * weights of neighbour t has t.
 * Not traced (the whole row is misses, no tests counted): a non-finite component of p, a NaN dist2_max or a negative dist2_max.
 *
 * Pruning.  bound = dist2_max while the list holds fewer than k entries, the dist2 of the k-th entry once it is full.  A slot or
 * a popped entry is skipped iff boxdist2 > bound (the closest-point block's boxdist2; never on equality).  A candidate enters
 * iff d <= dist2_max, and the list is not full or (d, id) is lexicographically below the k-th entry, and (d, id) is not already
 * in the list.  The duplicate rule is part of the definition: it makes a restart (below) harmless, which re-visits triangles
 * already listed, and it makes rows on spatial-split trees hold each id at most once (one id always has one d2).
 * The k smallest pairs (dist2, id) of a set under a strict total order do not depend on the visiting order, and since
 * d2 >= boxdist2 holds in float32 for every box that contains the vertex box, a skipped subtree holds no element below the bound
 * -- for any k.  So:
 *   - exact (bit for bit the brute force over the caller's triangles, sorted) on every tree whose slot boxes contain the vertex
 *     boxes below them: LBVH, pairs, hybrid, hybrid + pairs, SAH, SAH + pairs, and every refitted tree;
 *   - spatial-split trees (rt_run_sah_build with enable_splits): every record is d2(p, tri[id]) bit for bit, ids are distinct
 *     and the order is ascending; rank j's sqrt(dist2) exceeds the brute force's rank j by at most the closest-point block's
 *     2^-20 * M (the same argument rank by rank: the reference whose clipped box holds the triangle's closest point is pruned
 *     only against a bound that is at least the final rank-j distance).  Refitting a split tree restores exactness;
 *   - k = 1: (dist2, primitive_id) of out[i] equals rt_closest_points's record.
 *
 * Stack: 64 pending entries per query; a push beyond them is dropped.  A pass that dropped a push is followed by another pass
 * from the root that keeps the list so far, at most twice (rt_closest_points's rule); a pass that drops nothing makes the row
 * exact.  RT_KNN_STACK_OVERFLOW: the last pass of a query still dropped a push -- its row then holds real, distinct, sorted
 * records that may not be the nearest.
 * counters: optional device uint64[4], rt_closest_points's layout: [0] += box tests (non-NONE slots examined), [1] += triangle
 * tests (leaf records visited); [2] / [3] are not touched.  status: optional device uint32 the call ORs flags into (the caller
 * clears it).  Asynchronous (no allocation, no host copy, no synchronisation: hipGraph-capturable).  num_queries = 0: nothing
 * runs.
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null as / queries / out, k = 0 or
 * k > RT_KNN_MAX_K, a tree with count > 0 and a null node or leaf pointer, count > 7, queries not 16-byte aligned, out not
 * 8-byte aligned, status not 4-byte aligned. */
#define RT_KNN_MAX_K 32
typedef struct rt_knn_hit { float dist2; uint32_t primitive_id; } rt_knn_hit;
enum { RT_KNN_STACK_OVERFLOW = 1 };
int rt_k_nearest(const rt_accel* as, const rt_point_query* queries, uint32_t num_queries, uint32_t k, rt_knn_hit* out,
                 uint64_t* counters, uint32_t* status, void* stream);

/* ---- ray sorting and indexed ray queries (no reference counterpart).  rt_intersect_rays gives a wave 64 consecutive rays, so
 * its speed depends on the caller's ray order.  rt_sort_rays computes a coherence order of a batch, rt_intersect_rays_indexed
 * traces a batch through an index list -- that order, or any list of rays still alive.
 *
 * rt_sort_rays writes into order[0 .. num_rays) the ray indices in ascending key order; ties go to the lower index (the sort
 * is stable).  One sort serves any number of queries on the same rays (closest, any hit, other tmax windows that keep the
 * live set).
 *   Liveness.  A ray is dead exactly when rt_intersect_rays would not trace it: tmin > tmax, or a NaN in tmin, tmax, origin
 *   or direction.  A dead ray's key is RT_RAY_KEY_DEAD and nothing else: dead rays follow every live ray, in index order.
 *   The number of live rays lands in the scratch (rt_ray_sort_layout.num_live, a device uint32; read it after the stream ran).
 *   Box.  lo / hi = the ordered min / max (the floats' monotone integer image, -0 below +0) of min / max over the non-NONE
 *   slots of the root run [root, root + count); lo = hi = 0 when there is no such slot (an empty tree, count = 0).  Stored in
 *   the scratch (rt_ray_sort_layout.box: float lo[3], one unused float, float hi[3], one unused float).  Nothing else of
 *   the tree is read, so `as` may be a TLAS.
 *   Key of a live ray, float32, every operation rounded on its own (no fused multiply-add), IEEE division:
 *     cell(q, C) = (q > 0) ? (q >= C - 1 ? C - 1 : trunc(q)) : 0              -- selects; a NaN q gives cell 0
 *     per axis k: e = hi[k] - lo[k];  oc[k] = cell(((origin[k] - lo[k]) / e) * 128, 128)
 *     m = |dir.x|; if (|dir.y| > m) m = |dir.y|; if (|dir.z| > m) m = |dir.z|
 *     per axis k: dc[k] = cell((dir[k] / m) * 2 + 2, 4)
 *     key = morton3(oc) << 6 | morton3(dc),  morton3(c) = bit j of c[0] at position 3j + 2, of c[1] at 3j + 1, of c[2] at 3j
 *   27 bits: 7 origin bits per axis above 2 direction bits per axis (the direction's sign is the higher of the two).  The
 *   recipe is total: an origin outside the box, +-inf included, clamps to a border cell; a degenerate axis (hi == lo: e = 0)
 *   gives cell 127 above lo, cell 0 at or below it; a zero direction (0 / 0) gives dc = 0; the direction's length does not
 *   matter (dir / m is exact under scaling by a power of two while no component leaves the normal range).
 *   Scratch: rt_ray_sort_scratch_bytes(num_rays) bytes, 256-byte aligned, no initialisation needed: a 256-byte header (box,
 *   num_live), three uint32[num_rays] arrays (keys -- the sorted keys after the call -- and the sort's two temporaries), and
 *   the sort's tables (rt_radix_sort_scratch_bytes).  `order` is the sort's value array.
 *   Launches: 2 + the sort's (three 10-bit passes up to 2M rays, else four 8-bit ones), fixed by num_rays.
 *   Argument errors, returned before any GPU work: RT_ERR_INVALID_ARGUMENT for a null as / rays / order / scratch, rays not
 *   16-byte, order not 4-byte, scratch not 256-byte aligned, count > 7, or a tree with count > 0 and a null node pointer;
 *   RT_ERR_TOO_LARGE for num_rays > 0x3FFFFFFF (the sort's limit).  num_rays = 0: nothing runs.
 *
 * rt_intersect_rays_indexed: lane j of the launch (j < num_indices, 64 consecutive j per wave) takes i = order[j].  If
 * i < num_rays it traces rays[i] and writes hits[i], with rt_intersect_rays's semantics in every respect (the same kernel body);
 * if i >= num_rays (0xFFFFFFFF for instance) it does nothing.  Records whose index is not listed are not written; a
 * duplicated index writes the same bytes twice.  For any index list each written hits[i] equals rt_intersect_rays's record
 * bit for bit (a ray's result does not depend on its wave neighbours); when order is a permutation counters[0] and [1]
 * equal rt_intersect_rays's too, while [2] / [3] (wave steps) depend on the order: they measure its coherence.
 * Argument errors: rt_intersect_rays's, plus a null order or one not 4-byte aligned.  num_indices = 0: nothing runs.
 * Both calls are asynchronous (no host copy, no synchronisation: hipGraph-capturable). */
#define RT_RAY_KEY_BITS 30
#define RT_RAY_KEY_DEAD (1u << 29)
typedef struct rt_ray_sort_layout {
    size_t box;         /* float[8]: lo.xyz, -, hi.xyz, - (the start of the 256-byte header) */
    size_t num_live;    /* uint32: live rays of the last rt_sort_rays */
    size_t keys;        /* uint32[num_rays]: the sorted keys after the call (keys[j] is the key of ray order[j]) */
    size_t tmp_keys;    /* uint32[num_rays] */
    size_t tmp_values;  /* uint32[num_rays] */
    size_t sort;        /* rt_radix_sort_scratch_bytes(num_rays) bytes */
    size_t total;       /* = rt_ray_sort_scratch_bytes(num_rays) */
} rt_ray_sort_layout;
size_t rt_ray_sort_scratch_bytes(uint32_t num_rays);
int rt_ray_sort_layout_get(uint32_t num_rays, rt_ray_sort_layout* out);
int rt_sort_rays(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, uint32_t* order, void* scratch, void* stream);
int rt_intersect_rays_indexed(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, const uint32_t* order,
                              uint32_t num_indices, rt_hit* hits, int mode, uint32_t num_primitives, uint64_t* counters,
                              void* stream);

/* ---- all-hit ray queries (no reference counterpart).  For each caller ray: WHICH triangles it crosses inside its
 * [tmin, tmax] window, and how many -- the set-valued ray query (transparency, penetration counts, parity / inside tests, CSG),
 * through any tree rt_intersect_rays takes (runs of 1..7 slots; an empty tree, count = 0, is accepted and every row is empty).
 * The output length depends on the data, so the result is compressed sparse rows (CSR), as for the range queries: offsets[0 .. n]
 * (uint64) and one rt_hit array; ray i owns hits[offsets[i] .. offsets[i+1]).
 *
 * Rays.  An rt_ray, with rt_intersect_rays's liveness rule: a ray with tmin > tmax, or a NaN in origin, direction, tmin or
 * tmax, is not traced -- its row is empty and no tests are counted for it.  tmax = +inf is allowed.  1/dir is computed once per
 * ray by IEEE division.
 * Slot test.  A non-NONE slot is entered iff back >= front && front <= tmax && back >= tmin, front / back from rt_trace's slab
 * test (float32: t1 = (min - o) * (1/d), t2 = (max - o) * (1/d) per axis, front = the largest fminf(t1, t2), back = the smallest
 * fmaxf(t1, t2)).  tmin and tmax are the ray's ORIGINAL values for the whole traversal: the window is never updated.
 * Leaf test.  rt_trace's Moller-Trumbore (same epsilon, same operation order, same acceptance rule: not (|a| < epsilon), not
 * (u < 0 || u > 1), not (v < 0 || u + v > 1), not (t < tmin || t > tmax)) on the STORED corners of the leaf record: A =
 * (v0, v1, v2) with primitive_id_0, and B = (v2, v1, v3) with primitive_id_1 when v3 != v2 bit for bit (a single-triangle record
 * has v3 == v2, see the refit block; every builder gives a leaf slot a count >= 1, so this is the closest-hit traversal's rule
 * "count > 0 and v3 != v2" on every record the library writes).  Every test uses the original tmax.  Every accepted triangle
 * emits one rt_hit (t, primitive_id, u, v), (u, v) mapped back to the caller's corners through rt_triangle_pair.rotations
 * exactly as rt_intersect_rays maps them.
 *
 * Result: a SET of records per ray -- no ordering promise.  The row of ray i is the set of accepted triangles in the leaves
 * reached through entered slots.  With a fixed window whether a slot is entered does not depend on what was visited before it,
 * so the row is a function of the tree's bytes and the ray alone: any visiting order gives the same set.
 *   It is NOT promised to equal a brute force over the caller's triangles: the float32 slab test and the float32 triangle test
 *   are separate computations, and a grazing ray may fail a box whose triangle it would accept.  What does hold, when no push
 *   was dropped (status 0):
 *   1. some record of the row has the (t, u, v) bits of rt_intersect_rays's closest-hit record for the same ray and tree: the
 *      closest hit's triangle was reached through slots that passed with a smaller tmax, so they pass with the original one
 *      too, and the triangle test is the same arithmetic.  (On split trees and among coincident triangles two records at the
 *      same t can differ in primitive_id; the closest-hit query reports one of them.)  A closest-hit miss has an empty row and
 *      the other way round;
 *   2. hence the minimum t over the row is at most the closest-hit t.
 *   Spatial-split trees (rt_run_sah_build with enable_splits): a triangle appears once per REFERENCE that is reached, so
 *   duplicates are possible and the parity of a row means nothing there.  Refit does not remove them: the references stay.
 *   On the other trees every triangle is in one leaf and appears at most once.
 *   Order: the records of a ray come in the traversal order of its lane -- deterministic for a given tree, the same in
 *   rt_ray_hits_count and rt_ray_hits_collect (one traversal, compiled twice), otherwise unspecified.
 *
 * rt_ray_hits_count: offsets[0 .. num_rays] = the exclusive prefix sum of the row lengths; offsets[num_rays] is the total.
 *   64-bit: no overflow case exists.  scratch: rt_ray_hits_scratch_bytes(num_rays) bytes of device memory, 256-byte aligned, no
 *   initialisation needed (one uint64 per 256 rays: the workgroup sums of the scan).  Launches: the traversal (which also scans
 *   the counts inside each workgroup), one workgroup over the workgroup sums, one add.  num_rays = 0 still writes
 *   offsets[0] = 0.
 * rt_ray_hits_collect: ray i writes its first min(matches, offsets[i+1] - offsets[i]) records at hits + offsets[i] and writes
 *   nothing else (offsets[i+1] < offsets[i] counts as no room); records past the last segment and segments of other rays are
 *   not touched.  counts (optional, device uint32[num_rays]): the ray's true row length, room or not.  A ray with more records
 *   than room ORs RT_RAY_HITS_TRUNCATED into *status; its segment then holds the first records in traversal order.
 *   Two call patterns: (a) everything: rt_ray_hits_count, read offsets[num_rays] back, allocate hits, rt_ray_hits_collect with
 *   the same offsets; (b) a fixed K per ray: fill offsets[i] = i * K once, one rt_ray_hits_collect pass, counts says how many
 *   of each segment are valid (min(counts[i], K)).  num_rays = 0: nothing runs.
 * Both calls: counters, optional device uint64[4]: [0] += box tests (non-NONE slots examined), [1] += leaf records visited;
 * [2] / [3] are not touched.  The same rays give the same counters in both calls.  status: optional device uint32 the calls OR
 * flags into (the caller clears it).  Stack: 64 pending four-byte entries per ray; a push beyond them is dropped and sets
 * RT_RAY_HITS_STACK_OVERFLOW: the row is then a subset of the full row, and since both calls drop the same pushes they still
 * agree with each other.  Asynchronous (no allocation, no host copy, no synchronisation: hipGraph-capturable).
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null as / rays / offsets / scratch (count) / hits
 * (collect), a tree with count > 0 and a null node or leaf pointer, count > 7, rays or hits not 16-byte, offsets not 8-byte,
 * counts / status not 4-byte, scratch not 256-byte aligned. */
enum { RT_RAY_HITS_STACK_OVERFLOW = 1, RT_RAY_HITS_TRUNCATED = 2 };
size_t rt_ray_hits_scratch_bytes(uint32_t num_rays);
int rt_ray_hits_count(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, uint64_t* offsets, void* scratch,
                      uint64_t* counters, uint32_t* status, void* stream);
int rt_ray_hits_collect(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, const uint64_t* offsets, rt_hit* hits,
                        uint32_t* counts, uint64_t* counters, uint32_t* status, void* stream);

/* ---- instanced all-hit ray queries (no reference counterpart).  The all-hit query over a scene of placed copies of built
 * trees: for each caller ray EVERY triangle it crosses inside its [tmin, tmax] window in every instance, each record with the
 * instance it lies in -- layered transparency, thickness and entry / exit pairs, parity tests on placed closed meshes, CSG over
 * placed parts, X-ray picking -- without flattening the scene.  The scene is the instancing block's (rt_prepare_instances, a
 * TLAS over its proxies built WITHOUT pairs or splits, the records, the BLAS table of triangle trees); the result is the
 * all-hit block's CSR with a second, parallel array: ray i owns hits[offsets[i] .. offsets[i+1]) and
 * instance_ids[offsets[i] .. offsets[i+1]); record j of ray i is hits[offsets[i] + j] in instance instance_ids[offsets[i] + j],
 * as rt_intersect_rays_instanced pairs hits[i] with instance_ids[i].
 *
 * Rays, window.  The all-hit block's liveness rule (a ray with tmin > tmax, or a NaN in origin, direction, tmin or tmax, is not
 * traced: an empty row, no tests counted) and its fixed window: every slab test of both levels and every triangle test uses the
 * ray's ORIGINAL tmin / tmax.  An affine map preserves t, so the window applies unchanged in object space and the t of a record
 * needs no conversion.
 * TLAS.  A non-NONE TLAS slot is examined with rt_trace's float32 slab test on the world ray and entered iff back >= front &&
 * front <= tmax && back >= tmin.  A TLAS triangle slot that passes names instance primitive_id_0 of its leaf record.
 * Entering an instance: under exactly rt_intersect_rays_instanced's conditions (the id < num_instances, the record's flags 0,
 * its blas < num_blas, the table entry's count in 1..7), with that block's arithmetic: o' = W*(o, 1), d' = W3x3*d, each row
 * ((w0*x + w1*y) + w2*z) [+ w3] in float32, 1/d' by IEEE division.  On leaving the instance the world ray is reloaded from
 * rays[i]: the original bits.
 * Inside the BLAS the walk is the all-hit block's on the object ray: its slot test, its leaf test on the stored corners,
 * B = (v2, v1, v3) tested iff v3 != v2 bit for bit, and a record is rt_ray_hits_collect's for that object ray and tree -- t,
 * the BLAS's own primitive_id, (u, v) mapped back through rt_triangle_pair.rotations.
 *
 * Result: per ray the MULTISET of (instance, record) over the entered instances; no ordering promise.  The TLAS is built
 * without pairs or splits, so each instance sits in one TLAS leaf and is entered at most once; whether a TLAS slot, an instance
 * or a BLAS slot is entered depends on the bytes and the ray alone (the window never moves), so the row does not depend on the
 * visiting order, and rt_ray_hits_count_instanced and rt_ray_hits_collect_instanced -- one traversal, compiled twice -- cannot
 * disagree.  What holds when no push was dropped:
 *   1. composition: the row is the union, over the entered instances, of rt_ray_hits_collect's row on the instance's BLAS for
 *      the object ray, each record tagged with the instance;
 *   2. closest hit: some record of the row has the (instance, t, u, v) bits of rt_intersect_rays_instanced's closest-hit answer
 *      for the same ray (every slot and instance that query entered with a smaller tmax is entered with the original one, and
 *      the arithmetic is the same); a miss there has an empty row and the other way round;
 *   3. an identity instance over a tree gives rt_ray_hits_collect's row on that tree, all ids 0 and the same counters[1], for
 *      rays without -0 components (a transformed -0 may come out +0).
 *   Split BLASes repeat a triangle once per reference reached, as in the all-hit block; two instances in the same place both
 *   report.  It is not promised to equal a float64 brute force over the placed triangles (the all-hit block says why; here the
 *   float32 ray transform and the padded proxy box come on top).
 *
 * rt_ray_hits_count_instanced: offsets[0 .. num_rays] = the exclusive prefix sum of the row lengths.  scratch:
 *   rt_ray_hits_scratch_bytes(num_rays) bytes, 256-byte aligned, no initialisation needed.  Three launches, nothing read back.
 * rt_ray_hits_collect_instanced: ray i writes its first min(matches, offsets[i+1] - offsets[i]) records at hits + offsets[i] and
 *   their instances at instance_ids + offsets[i] and nothing else; counts (optional) gets the true row length; a ray with more
 *   records than room ORs RT_RAY_HITS_TRUNCATED into *status.  offsets[i] = i * K is the one-pass fixed-K mode: exact counts,
 *   the first min(counts[i], K) records of each segment valid.
 * Both calls: counters, optional device uint64[4]: [0] += non-NONE slots examined, both levels together, [1] += BLAS leaf
 * records visited; [2] / [3] are not touched.  status: optional device uint32 the calls OR RT_RAY_HITS_* flags into (never
 * cleared).  Stack: ONE stack of 64 four-byte entries serves both levels, the BLAS's entries above the TLAS's: a BLAS entered at
 * depth k has 64 - k entries.  A dropped push sets RT_RAY_HITS_STACK_OVERFLOW; the row is then a subset of the full row and the
 * two calls still agree.  Asynchronous (no allocation, no host copy, no synchronisation: hipGraph-capturable).  num_rays = 0:
 * nothing runs (offsets[0] is not written).
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null tlas / rays / offsets / scratch (count) /
 * hits / instance_ids (collect); with num_instances > 0 a null records or blas_table, or num_blas = 0 (blas_table may be null
 * only when num_instances = 0); a TLAS with count > 0 and a null node or leaf pointer, tlas->count > 7; rays / hits / records
 * not 16-byte, offsets / blas_table not 8-byte, instance_ids / counts / status not 4-byte, scratch not 256-byte aligned.
 * Hit filters and instance masks: rt_ray_hits_count_instanced_filtered / rt_ray_hits_collect_instanced_filtered, the instanced
 * set-filter block below.
 * Out of scope: instance motion, mixed / sphere BLASes, an indexed form, the host mirror and rt_cli.  (The first-K form is
 * rt_ray_first_hits_instanced, the instanced first-K block below.) */
int rt_ray_hits_count_instanced(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, void* stream);
int rt_ray_hits_collect_instanced(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                  const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                  const uint64_t* offsets, rt_hit* hits, uint32_t* instance_ids, uint32_t* counts,
                                  uint64_t* counters, uint32_t* status, void* stream);

/* ---- first-K ray queries (no reference counterpart).  For each caller ray: the K nearest triangles it crosses inside its
 * [tmin, tmax] window, in order -- layered transparency, depth peeling, "skip the first surface" picking, thickness (entry /
 * exit pairs), CSG -- through any tree rt_intersect_rays takes (runs of 1..7 slots; an empty tree, count = 0, is accepted and
 * every row is misses).  The fixed-length sibling of the all-hit query, as rt_k_nearest is of the sphere range query: row i of
 * the output has exactly k records, so nothing is counted, scanned, allocated or read back, and the window shrinks while the
 * ray is traced: ONE launch.
 *
 * Rays, slab arithmetic, leaf test.  The all-hit block's, word for word: the liveness rule (a ray with tmin > tmax, or a NaN in
 * origin, direction, tmin or tmax, is not traced), 1/dir by IEEE division, front / back from rt_trace's float32 slab test,
 * rt_trace's Moller-Trumbore on the STORED corners, triangle B = (v2, v1, v3) tested iff v3 != v2 bit for bit, (u, v) mapped
 * back to the caller's corners through rt_triangle_pair.rotations.  Let W be the all-hit row of the ray: the row
 * rt_ray_hits_collect defines for the same tree and the ray's original window.
 * Bound.  Each ray carries a bound b: its original tmax while its list holds fewer than k records, the t of the k-th record
 *   once the list is full.
 * Slot test.  A non-NONE slot is entered iff back >= front && front <= b && back >= tmin -- the all-hit rule with b in the
 *   place of tmax, b being the bound at the moment the slot is examined.  A pending entry that is re-tested when it is popped
 *   is dropped iff front > b with the bound of that moment.  Equality never prunes.
 * Leaf test.  A triangle is accepted by the all-hit block's test against the window [tmin, b]: t > b rejects, t == b does not.
 * List.  An accepted candidate (t, primitive_id, u, v) enters the list iff
 *   - the list is not full, or (t, primitive_id) is lexicographically below the k-th entry, and
 *   - no listed entry has the same (t, primitive_id).
 *   The second clause keeps a record once on spatial-split trees, where a triangle has several references (rt_k_nearest's
 *   rule).  A full list loses its k-th entry to a newcomer.  Floats compare as floats (-0 equals +0).  A NaN t -- products that
 *   overflowed; Moller-Trumbore's comparisons let it through, and W holds such records too -- orders above every number, NaNs
 *   are equal to each other, and while the k-th t is NaN the bound stays the original tmax: the bound is never NaN.
 * Output row.  Row i is out[i*k .. i*k + k) (64-bit indexing), rt_hit records of 16 bytes.  It holds the list, ascending by
 *   (t, primitive_id): ties on t go to the lower id.  Behind the list come rt_intersect_rays's miss records
 *   {+inf, RT_MISS, 0, 0}.  A ray that is not traced, and every ray of an empty tree, gets k miss records and counts nothing.
 *   Rows at i >= num_rays are not written.
 * Order.  The surviving slot of a run with the smallest front is visited next (ties: the lower slot), the others wait.  The
 *   order is an implementation matter that the claims below do not depend on; only the counters and the rows of undecided
 *   rays (below) can see it.
 *
 * What is promised.  The slab test and the triangle test are separate float32 computations, so a box's front can round to a
 * value beyond the t of a hit inside the box.  For the all-hit query, whose window is fixed, that is harmless; here a bound
 * that has fallen to such a t prunes the box although it holds a nearer hit.  That is why "equals the brute force, sorted" cannot
 * be promised for rays, and why the contract names the rounding: for a record w of W let its GATE g(w) be the largest slab
 * front over the slots on the path from the root run to w's leaf slot, the leaf slot included (the smallest over its paths
 * if a split tree reaches the record through several) -- a function of the tree's bytes and the ray.  Let Ws be W with
 * duplicates by (t, id) removed, sorted by (t, id); E its first min(k, |Ws|) records; T1 the t of its (k+1)-th record, or the
 * original tmax if there is none.  With status 0 (DESIGN section 19 has the proofs):
 *   1. every live record of the row is a record of W, bit for bit in all 16 bytes; the row is strictly ascending in (t, id);
 *      misses come only at the end;
 *   2. DECIDED rays: if every w in E has g(w) <= T1, the row is E, bit for bit.  (Before w is offered the list holds only
 *      records of W without w, so b >= T1: every slot above w passes whenever it is examined or popped, w is accepted, and the
 *      list keeps the k smallest of what it is offered.)  In particular a ray with |Ws| <= k is decided: its row is all of Ws;
 *   3. EVERY ray: with T the final bound (the last live t of a full row -- the original tmax if that t is NaN -- else the
 *      original tmax), every w in W with g(w) <= T and (t, id) below the row's last live record is in the row.  So a full row
 *      can miss a record only where the float32 slab test put a box's front BEYOND a hit inside that box;
 *   4. counters[0] and counters[1] are at most rt_ray_hits_count's for the same rays (every slot entered here is entered
 *      there).  They are equal when every ray has |Ws| < k: the bound never moves and the set of entered slots is the all-hit
 *      one.  Otherwise they depend on the visiting order and on which pending entries are re-tested -- implementation
 *      matters, not part of the contract.
 * Further, without a promise beyond the above: on decided rays the row's first t is at most rt_intersect_rays's closest-hit t
 * (all-hit claim 1: that record is in W); among coincident triangles the primitive_id at a tied t is the LOWER one here and
 * whichever was met first there; on split trees the records of a row are distinct in (t, id) -- the references of one triangle
 * that store its corners in one order give one t, and the row then holds that id once -- and everything above is stated on Ws.
 *
 * Stack: 64 pending entries per ray; a push beyond them is dropped and sets RT_RAY_FIRST_STACK_OVERFLOW: the row is then a
 * sorted subset of W (claim 1 still holds).  There is no restart pass: a shrinking bound keeps fewer entries pending than the
 * all-hit query, which has none either.
 * counters: optional device uint64[4]: [0] += box tests (non-NONE slots examined), [1] += leaf records visited; [2] / [3] are
 * not touched.  status: optional device uint32 the call ORs flags into (the caller clears it).  Asynchronous (no allocation, no
 * scratch, no host copy, no synchronisation: hipGraph-capturable).  num_rays = 0: nothing runs.
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null as / rays / out, k = 0 or
 * k > RT_RAY_FIRST_MAX_K, count > 7, a tree with count > 0 and a null node or leaf pointer, rays or out not 16-byte aligned,
 * status not 4-byte aligned, counters not 8-byte aligned. */
#define RT_RAY_FIRST_MAX_K 32
enum { RT_RAY_FIRST_STACK_OVERFLOW = 1 };
int rt_ray_first_hits(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, uint32_t k, rt_hit* out,
                      uint64_t* counters, uint32_t* status, void* stream);

/* ---- instanced first-K ray queries (no reference counterpart).  The first-K query over a scene of placed copies of built
 * trees: for each caller ray the K nearest crossings inside its [tmin, tmax] window over every instance, in order, each with
 * the instance it lies in -- layered transparency, depth peeling, "skip the first surface" picking and thickness on a placed
 * scene -- without flattening the scene and without the count pass, read-back, allocation, collect pass and sorts of
 * rt_ray_hits_count_instanced / rt_ray_hits_collect_instanced cut to K.  ONE launch.  The scene is the instanced all-hit
 * block's: rt_prepare_instances, a TLAS over its proxies built WITHOUT pairs or splits, the records, the BLAS table of triangle
 * trees.
 *
 * Let W be the instanced all-hit row of the ray for its original window, as rt_ray_hits_collect_instanced defines it: a
 * multiset of 20-byte items (instance, t, primitive_id, u, v).  The definition is the first-K block's with three changes.
 * Key.  Items order by (t, instance, primitive_id).  Floats compare as floats; a NaN t orders above every number and NaNs are
 *   equal to each other.  An accepted candidate enters the list iff
 *   - the list is not full, or its key is below the k-th entry's, and
 *   - no listed item has the same key.
 *   Two instances of one BLAS in the same place therefore both report, the lower instance first; a split BLAS reports a triangle
 *   once per instance.
 * Bound on both levels.  b is the original tmax while the list holds fewer than k items, the t of the k-th item after (the
 *   original tmax while that t is NaN): never NaN.  A non-NONE slot is entered iff back >= front && front <= b && back >= tmin
 *   with the b of that moment -- in the TLAS on the world ray, in a BLAS on the object ray.  A pending entry that is re-tested
 *   when it is popped is dropped iff front > b.  Equality never prunes.  The triangle test is the all-hit test against
 *   [tmin, b].  An affine map keeps t, so one b serves both levels without conversion.
 * Entering an instance.  The instanced all-hit block's, word for word: a TLAS triangle slot that passes names instance
 *   primitive_id_0 of its leaf record; it is entered iff the id < num_instances, the record's flags are 0, its blas < num_blas
 *   and the table entry's count is in 1..7; o' = W*(o, 1), d' = W3x3*d, each row ((w0*x + w1*y) + w2*z) [+ w3] in float32, 1/d'
 *   by IEEE division; on leaving the instance the world ray is reloaded from rays[i], the original bits.
 * Output.  hits[i*k .. i*k + k) and instance_ids[i*k .. i*k + k) (64-bit indexing) hold the list ascending by key, then
 *   padding: {+inf, RT_MISS, 0, 0} with instance RT_MISS.  A ray that is not traced (the first-K block's liveness rule) gets k
 *   pads and counts nothing; so does every ray when num_instances = 0 or the TLAS is empty (count = 0).  Rows at i >= num_rays
 *   are not written.
 * Gate.  For an item w of W, g(w) is the largest slab front over the TLAS slots on the path from the TLAS root run to the
 *   instance's leaf slot, that slot included (world-ray fronts), and the BLAS slots from its root run to w's leaf slot, that slot
 *   included (object-ray fronts); on a split BLAS the smallest such value over the paths.  Ws is W with duplicates by key removed,
 *   sorted by key; E its first min(k, |Ws|) items; T1 the t of its (k+1)-th item, or the original tmax if there is none.
 * Order.  An implementation matter, as in the first-K block: the surviving slot of a run with the smallest front goes next
 *   (ties: the lower slot) on both levels, and an instance is walked to the end before the next TLAS entry is popped.
 *
 * What is promised with status 0 (DESIGN section 30 has the proofs; they are the first-K block's, because b never rises and
 * the TLAS proxy's front is one more slot on the path):
 *   1. every live item of the row is an item of W, bit for bit in all 20 bytes; the row is strictly ascending by key; pads come
 *      only at the end;
 *   2. DECIDED rays: if every w in E has g(w) <= T1, the row is E, bit for bit.  A ray with |Ws| <= k is decided;
 *   3. EVERY ray: with T the final bound (the last live t of a full row -- the original tmax if that t is NaN -- else the
 *      original tmax), every w in W with g(w) <= T and a key below the row's last live item is in the row;
 *   4. counters[0] and counters[1] are at most rt_ray_hits_count_instanced's for the same rays, and equal when every ray has
 *      |Ws| < k.
 * Further, without a promise beyond the above: k = 1 on a decided ray gives a t at most rt_intersect_rays_instanced's
 * closest-hit t, a miss there is a row of pads and the other way round; an identity instance over a tree gives
 * rt_ray_first_hits's row on that tree with all instances 0, on rays decided for both and without -0 components.
 *
 * Stack: ONE stack of 64 four-byte entries serves both levels, the BLAS's entries above the TLAS's (the instanced all-hit
 * block's).  A dropped push sets RT_RAY_FIRST_STACK_OVERFLOW; the row is then a sorted subset of W (claim 1 still holds).
 * counters: optional device uint64[4]: [0] += non-NONE slots examined, both levels together, [1] += BLAS leaf records visited;
 * [2] / [3] are not touched.  status: optional device uint32 the call ORs flags into (the caller clears it).  Asynchronous (no
 * allocation, no scratch, no host copy, no synchronisation: hipGraph-capturable).  num_rays = 0: nothing runs.
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null tlas / rays / hits / instance_ids; with
 * num_instances > 0 a null records or blas_table, or num_blas = 0 (blas_table may be null only when num_instances = 0); a TLAS
 * with count > 0 and a null node or leaf pointer, tlas->count > 7; k = 0 or k > RT_RAY_FIRST_MAX_K; rays / hits / records not
 * 16-byte, blas_table / counters not 8-byte, instance_ids / status not 4-byte aligned.
 * Hit filters and instance masks: rt_ray_first_hits_instanced_filtered, the instanced set-filter block below.
 * Out of scope: instance motion, mixed / sphere BLASes, an indexed form, the host mirror and rt_cli. */
int rt_ray_first_hits_instanced(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                uint32_t k, rt_hit* hits, uint32_t* instance_ids,
                                uint64_t* counters, uint32_t* status, void* stream);

/* ---- hit filters for the ray queries (no reference counterpart).  The four ray queries above accept every triangle that
 * Moller-Trumbore accepts.  Their filtered siblings take one more argument, an rt_hit_filter, that says which of those
 * candidates count: "front faces only" (face culling), "not the triangle I am standing on" (a per-ray skip id), "only the
 * triangles of these groups" (a mask per primitive against a mask per ray) -- the ray flags, masks and filters of the other
 * ray APIs.  The filter sits at the one place where a candidate is accepted, inside the traversal: a closest-hit ray that meets
 * a filtered-out triangle first does not shrink its window on it and does not prune what lies behind it, which no pass over
 * the unfiltered result can undo.  Every argument other than `filter` keeps the type and meaning it has in the unfiltered
 * sibling (rt_intersect_rays, rt_ray_hits_count, rt_ray_hits_collect, rt_ray_first_hits); box tests, leaf visits, the liveness
 * rule, the stack and the status flags are the sibling's.
 *
 * rt_hit_filter is a HOST struct holding device pointers, like rt_accel; it is read during the call and need not outlive it.
 *   flags: RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT; both together are legal.
 *   ray_mask: the mask of every ray when per_ray is null.
 *   prim_masks: optional DEVICE uint32[num_primitives], indexed by primitive_id.  A null prim_masks is an absent array whatever
 *     num_primitives says.
 *   per_ray: optional DEVICE rt_ray_filter[num_rays], indexed by the ray's index i (the index of rays[i] and of its result):
 *     the ray's own mask and the primitive_id it skips, RT_MISS for none.  One 8-byte load per ray.
 *   pad: 0 (not read).
 * Acceptance rule.  A candidate is a triangle A = (v0, v1, v2) or B = (v2, v1, v3) of a leaf record that the sibling's leaf
 * test accepts (its Moller-Trumbore on the STORED corners, against the window the sibling tests it against), with the
 * determinant a = e1 . (dir x e2), e1 = c1 - c0, e2 = c2 - c0, exactly as that test computes it in float32 on the stored
 * corners (c0, c1, c2), and the record's primitive_id.  It is KEPT iff all four hold:
 *   1. not (RT_FILTER_CULL_BACK and a < 0);
 *   2. not (RT_FILTER_CULL_FRONT and a > 0).  a = -dir . n with n = (c1 - c0) x (c2 - c0), the counter-clockwise normal: a > 0
 *      means the ray meets the side that normal points to, the FRONT.  A NaN a (overflowed products) is neither front nor
 *      back and is never culled; with both bits set only such records survive;
 *   3. primitive_id != the ray's skip_id.  skip_id = RT_MISS skips nothing; with a null per_ray nothing is skipped;
 *   4. (pm & rm) != 0, rm the ray's mask (ray_mask when per_ray is null), pm = prim_masks[primitive_id] when prim_masks is
 *      non-null and primitive_id < num_primitives, else pm = 0xFFFFFFFF and nothing is read.
 *   The tests run in this order, so prim_masks is read only for a candidate that passed 1-3.
 *   A candidate that is not kept is treated exactly as if the leaf test had rejected it: no record, no window or bound update,
 *   no list entry, and an any-hit ray does not end on it.
 * Facing and the caller's winding.  A leaf record stores cyclic rotations of the caller's corners (rt_triangle_pair.rotations),
 *   and a pair forms only across an edge its two triangles traverse in opposite directions (the pairing asks for A's edge
 *   reversed in B), so the stored A = (v0, v1, v2) and B = (v2, v1, v3) both keep the caller's winding: front and back are the
 *   caller's, on every tree.  Near a = 0 the sign of the stored-corner determinant decides, not a recomputation on the caller's
 *   corner order (a rotation changes the rounding, not the winding).
 *
 * Contracts.  Let W be the all-hit row of the ray (all-hit block) and W_f the kept records of W.
 *   rt_ray_hits_count_filtered / rt_ray_hits_collect_filtered: the all-hit block with W_f in the place of the row: the row is
 *     W_f as a set; its claims hold with the filtered closest hit in the place of the closest hit.  The window is fixed and the
 *     filter acts after the leaf test, so counters [0] and [1] equal the unfiltered call's exactly.
 *   rt_ray_first_hits_filtered: the first-K block with W_f for W throughout: Ws, E, T1, gates, decided rays and claims 1-4,
 *     claim 4 against rt_ray_hits_count_filtered's row lengths (|Ws| < k on every ray: the counters equal the all-hit
 *     counters).  The bound only ever falls to the t of a kept record.
 *   rt_intersect_rays_filtered: rt_intersect_rays's traversal with the rule above.  With no dropped push: the record is a record
 *     of W_f, bit for bit in (t, u, v); a miss iff W_f is empty; any-hit hits iff closest-hit hits; on a ray that is decided
 *     for k = 1 on W_f the record's t is E's t, bit for bit (before E is offered the window's end is the t of another kept
 *     record, so it is at least T1 and at least g(E), and slot tests pass on equality).
 *   filter == NULL forwards to the unfiltered entry point.  A filter that keeps everything -- flags 0 with null arrays, or with
 *     arrays of all-ones masks and skip_id = RT_MISS -- gives the unfiltered call's bytes and counters.
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): all of the sibling's; a flag bit other than
 * RT_FILTER_CULL_BACK / RT_FILTER_CULL_FRONT; prim_masks not 4-byte aligned; per_ray not 8-byte aligned.  num_primitives > 0
 * with a null prim_masks is fine.  Asynchronous and hipGraph-capturable like the siblings.
 * Out of scope: rt_hit_filter is the filter of the four single-tree ray queries only.  The instanced ray query has a filter of
 * its own (rt_intersect_rays_instanced_filtered, the instance-filter block below); the indexed ray query, rt_trace, and the
 * point, range and overlap queries take no filter. */
enum { RT_FILTER_CULL_BACK = 1, RT_FILTER_CULL_FRONT = 2 };
typedef struct rt_ray_filter {
    uint32_t mask;                        /* rm of rule 4 */
    uint32_t skip_id;                     /* rule 3; RT_MISS: nothing */
} rt_ray_filter;                          /* 8 bytes, per ray */
typedef struct rt_hit_filter {
    uint32_t flags;                       /* RT_FILTER_*; any other bit: RT_ERR_INVALID_ARGUMENT */
    uint32_t ray_mask;                    /* the mask of every ray when per_ray is null */
    uint32_t num_primitives;              /* length of prim_masks */
    uint32_t pad;                         /* 0 */
    const uint32_t* prim_masks;           /* optional DEVICE uint32[num_primitives], indexed by primitive_id */
    const rt_ray_filter* per_ray;         /* optional DEVICE array [num_rays], indexed by the ray's index */
} rt_hit_filter;                          /* 32 bytes */
int rt_intersect_rays_filtered(const rt_accel* as, const rt_ray* rays, rt_hit* hits, uint32_t num_rays, int mode,
                               uint32_t num_primitives, const rt_hit_filter* filter, uint64_t* counters, void* stream);
int rt_ray_hits_count_filtered(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                               uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, void* stream);
int rt_ray_hits_collect_filtered(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, const rt_hit_filter* filter,
                                 const uint64_t* offsets, rt_hit* hits, uint32_t* counts, uint64_t* counters, uint32_t* status,
                                 void* stream);
int rt_ray_first_hits_filtered(const rt_accel* as, const rt_ray* rays, uint32_t num_rays, uint32_t k,
                               const rt_hit_filter* filter, rt_hit* out, uint64_t* counters, uint32_t* status, void* stream);

/* ---- hit filters and instance masks for the instanced ray query (no reference counterpart).  rt_hit_filter cannot serve a scene
 * of placed copies: its skip_id is a bare primitive_id, and the same id exists in every copy of a BLAS; its facing is decided on
 * the stored object-space corners, so a mirrored instance shows the caller the wrong side; and its masks are per triangle, so a
 * masked instance would still be entered, its BLAS walked and its candidates rejected one by one.  This block is the filter of
 * the two-level query: an instance visibility mask asked at the TLAS leaf (DXR's InstanceMask, OptiX's visibility mask: shadow
 * casters only, no self-shadowing of one model, a per-layer ray) -- the one filter that makes a ray cheaper, because the whole
 * BLAS descent is saved --, face culling by the WORLD-space facing, and a per-ray (instance, primitive) pair to skip.
 *
 * rt_intersect_rays_instanced_filtered: every argument other than `filter` keeps the type and meaning it has in
 * rt_intersect_rays_instanced, and all of that call's rules carry over unchanged: rays, records, modes, the NaN and empty-window
 * rule, the ONE 64-entry stack of both levels, the rule for when an instance is never entered, the world ray reloaded on exit,
 * the counters.  rt_instance_hit_filter is a HOST struct holding device pointers, like rt_hit_filter; it is read during the call
 * and need not outlive it.
 *   flags: RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT (the hit-filter block's bits); both together are legal.
 *   ray_mask: the mask of every ray when per_ray is null.
 *   per_instance: optional DEVICE rt_instance_filter[num_instance_filters], indexed by the instance index (a TLAS leaf's
 *     primitive_id_0, the value reported in instance_ids): the instance's mask and its RT_INSTANCE_FILTER_* flags.  A null
 *     per_instance is an absent array whatever num_instance_filters says; the array may be shorter than num_instances.
 *   per_ray: optional DEVICE rt_instance_ray_filter[num_rays], indexed by the ray's index i: the ray's own mask and the
 *     (skip_instance, skip_id) pair it skips.  One 16-byte load per ray.
 *   pad: 0 (not read); rt_instance_ray_filter.pad: not read.
 * The call adds two rules.
 * 1. Instance rule, asked at the TLAS leaf when the traversal is about to enter instance `id` (id < num_instances), BEFORE the
 *    instance record is read:
 *      rm = per_ray[i].mask, or ray_mask when per_ray is null;
 *      im = per_instance[id].mask when per_instance is non-null and id < num_instance_filters (one 8-byte load that also
 *           brings the instance's flags), else im = 0xFFFFFFFF and nothing is read;
 *      the instance is entered only if (im & rm) != 0 -- and, as before, only if its record's flags are zero, its blas <
 *      num_blas and the table entry's count is 1 .. 7.
 *    An instance that is not entered is treated exactly like a flagged one: the lane advances in the TLAS; the instance
 *    contributes no box test, no leaf visit and no candidate, and neither its record nor its rt_accel is read.
 * 2. Candidate rule, asked at the leaf test's acceptance point inside the entered instance `id`.  A candidate is a triangle
 *    A = (v0, v1, v2) or B = (v2, v1, v3) of a BLAS leaf record that rt_intersect_rays_instanced's leaf test accepts
 *    (Moller-Trumbore on the STORED corners with the object-space ray, against the current [tmin, tmax]), with the determinant
 *    a = e1 . (dir' x e2) exactly as that test computes it in float32 (the hit-filter block's `a`, in object space), and the
 *    record's primitive_id.  With W = the record's float32 world_to_object, rows w0, w1, w2:
 *      det  = (w0.x*(w1.y*w2.z - w1.z*w2.y) - w0.y*(w1.x*w2.z - w1.z*w2.x)) + w0.z*(w1.x*w2.y - w1.y*w2.x), every product,
 *             difference and sum rounded to float32 in the order written (no fused multiply-add); it is computed only when
 *             a cull bit is set;
 *      flip = (det < 0) XOR (per_instance[id].flags & RT_INSTANCE_FILTER_FLIP_FACING); a NaN det counts as not mirrored.  A
 *             mirroring object_to_world (negative determinant, and so a negative det) reverses the winding the world sees;
 *      world-facing = a when flip is false, -a when it is true (the sign of a is unchanged by a non-mirroring affine map:
 *             a = -dir . n scales by the determinant);
 *    the candidate is KEPT iff all three hold:
 *      a. not (RT_FILTER_CULL_BACK and world-facing < 0), unless the instance has RT_INSTANCE_FILTER_CULL_DISABLE;
 *      b. not (RT_FILTER_CULL_FRONT and world-facing > 0), unless the instance has RT_INSTANCE_FILTER_CULL_DISABLE;
 *      c. not (id == skip_instance and primitive_id == skip_id and skip_id != RT_MISS).  RT_MISS in either word is "none":
 *         skip_instance = RT_MISS matches no instance (id < num_instances), and skip_id = RT_MISS skips nothing whatever
 *         skip_instance is (no leaf record carries that primitive_id in a tree the builders make; the rule does not depend
 *         on it).  A null per_ray skips nothing.
 *    A NaN a is neither front nor back and is never culled.  Equivalently the kernel applies, to `a` itself, the call's cull
 *    bits with BACK and FRONT exchanged when flip is true and cleared under CULL_DISABLE, and skip_id only inside skip_instance.
 *    A rejected candidate is treated exactly as if the leaf test had rejected it: no window update, and an any-hit ray goes on.
 *    An instance without a per_instance record has flags 0.  An unknown bit in a device-side per_instance[].flags is ignored.
 * Contracts.
 *   filter == NULL forwards to rt_intersect_rays_instanced.
 *   A filter that keeps everything -- null arrays with ray_mask all ones and flags 0, or arrays of all-ones masks with zero flags
 *     and skip_instance = RT_MISS -- gives the unfiltered call's hits, instance_ids and all four counters, byte for byte.
 *   Any-hit hits iff closest-hit hits (no dropped push): both run one sequence of tests until the first kept candidate.
 *   One identity instance with no per_instance: the call equals rt_intersect_rays_filtered on the BLAS with the same flags,
 *     null prim_masks and per-ray records {mask, skip_id} for rays whose skip_instance is 0, on rays without -0 components.
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): all of rt_intersect_rays_instanced's; a flag bit
 * other than RT_FILTER_CULL_BACK / RT_FILTER_CULL_FRONT in filter->flags; per_instance not 8-byte aligned; per_ray not 16-byte
 * aligned.  num_instance_filters > 0 with a null per_instance is fine.  Asynchronous and hipGraph-capturable like the sibling.
 * Out of scope: there is no per-primitive mask in this call -- grouping is per instance.  The indexed form of this call is
 * rt_intersect_rays_instanced_indexed with the same filter (the indexed-instanced block below).  The instanced all-hit and first-K queries take this same filter through entry points of their own
 * (the instanced set-filter block below). */
enum { RT_INSTANCE_FILTER_CULL_DISABLE = 1, RT_INSTANCE_FILTER_FLIP_FACING = 2 };
typedef struct rt_instance_filter {
    uint32_t mask;                        /* im of rule 1 */
    uint32_t flags;                       /* RT_INSTANCE_FILTER_*; other bits are ignored */
} rt_instance_filter;                     /* 8 bytes, per instance */
typedef struct rt_instance_ray_filter {
    uint32_t mask;                        /* rm of rule 1 */
    uint32_t skip_instance;               /* rule 2c; RT_MISS: nothing */
    uint32_t skip_id;                     /* rule 2c: the primitive_id skipped inside skip_instance */
    uint32_t pad;                         /* not read */
} rt_instance_ray_filter;                 /* 16 bytes, per ray */
typedef struct rt_instance_hit_filter {
    uint32_t flags;                       /* RT_FILTER_CULL_BACK | RT_FILTER_CULL_FRONT; any other bit: RT_ERR_INVALID_ARGUMENT */
    uint32_t ray_mask;                    /* the mask of every ray when per_ray is null */
    uint32_t num_instance_filters;        /* length of per_instance */
    uint32_t pad;                         /* 0, not read */
    const rt_instance_filter* per_instance;   /* optional DEVICE array, indexed by the instance index */
    const rt_instance_ray_filter* per_ray;    /* optional DEVICE array [num_rays], indexed by the ray's index */
} rt_instance_hit_filter;                 /* 32 bytes */
int rt_intersect_rays_instanced_filtered(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                         const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, rt_hit* hits,
                                         uint32_t* instance_ids, uint32_t num_rays, int mode, uint32_t num_primitives,
                                         const rt_instance_hit_filter* filter, uint64_t* counters, void* stream);

/* ---- instance filters for the instanced all-hit and first-K ray queries (no reference counterpart): the instanced set-filter
 * block.  The two set-valued queries of a placed scene need the filter above more than the closest-hit query does: a ray that
 * leaves a surface must skip the (instance, primitive) it stands on (depth peeling, layered transparency), visibility groups
 * are instance masks that save the whole BLAS descent, thickness and entry / exit pairing need the WORLD-space facing on
 * mirrored parts -- and a first-K row computed without the filter cannot be repaired afterwards: a rejected crossing that
 * entered the list has shrunk the bound and evicted a kept one.
 *
 * rt_ray_hits_count_instanced_filtered, rt_ray_hits_collect_instanced_filtered, rt_ray_first_hits_instanced_filtered: each is
 * its sibling's signature (rt_ray_hits_count_instanced, rt_ray_hits_collect_instanced, rt_ray_first_hits_instanced) with one
 * more argument, `filter`, before the outputs.  rt_instance_hit_filter, its flag bits, rt_instance_filter and
 * rt_instance_ray_filter are the instance-filter block's, unchanged; every other argument keeps the type and meaning it has in
 * the sibling, and all of the sibling's rules carry over.  filter == NULL forwards to the unfiltered sibling.
 *
 * Rules 1 and 2 of the instance-filter block apply word for word:
 * 1. Instance rule.  Asked at the TLAS leaf, for id < num_instances, BEFORE the instance record is read.  An instance that is
 *    not entered contributes no BLAS box test, no leaf visit and no candidate; neither its record nor its rt_accel is read.
 *    Its proxy's slab test in the TLAS is still counted.
 * 2. Candidate rule.  Asked at the leaf test's ONE acceptance point (after the t window test), with det in the header's
 *    operation order, the BACK / FRONT exchange under flip, CULL_DISABLE, and skip_id only inside skip_instance.  A rejected
 *    candidate is treated exactly as if Moller-Trumbore had rejected it.
 *
 * All-hit.  Let W be the unfiltered instanced all-hit row of the ray.  The filtered row is the multiset of the items of W whose
 * instance passes rule 1 and whose candidate passes rule 2.  The window never moves, so the row is again a function of the
 * bytes, the ray and the filter; count and collect are one traversal compiled twice and cannot disagree (under the same
 * filter).  Fixed-K mode, counts, RT_RAY_HITS_TRUNCATED, the one 64-entry stack and RT_RAY_HITS_STACK_OVERFLOW are the
 * sibling's.
 *
 * First-K.  The instanced first-K block with W read as the FILTERED all-hit row: Ws, E, T1 and the decided rays are defined on
 * it.  The bound b moves only on kept items: a rejected candidate never enters the list.  Key, list rule, padding, the gate
 * g(w), the order and the note that a popped TLAS entry is not re-tested are unchanged; a popped entry of a masked instance
 * fails rule 1 and the lane goes on in the TLAS.  Claims 1-4 hold on the filtered W (DESIGN section 31 has the proofs); claim 4
 * compares with rt_ray_hits_count_instanced_filtered under the same filter.
 *
 * Contracts.
 *   (a) Keep-all.  A filter that keeps everything -- null arrays with ray_mask all ones and flags 0, or arrays of all-ones
 *       masks with zero flags and skip_instance = RT_MISS -- gives the unfiltered sibling's offsets, counts, counters[0..1] and
 *       status byte for byte, and the same items in every row (all-hit) or the same bytes (first-K).
 *   (b) Composition.  The all-hit row is the union, over the instances rule 1 lets in, of rt_ray_hits_collect_filtered's row on
 *       the BLAS for the object ray under the effective single-tree filter (the cull bits rule 2 applies to `a`, skip_id inside
 *       skip_instance, null masks), each record tagged with the instance.
 *   (c) Closest hit.  The all-hit row holds the (instance, t, u, v) bits of rt_intersect_rays_instanced_filtered's closest-hit
 *       answer under the same filter; a miss there is an empty row and the other way round.  First-K with k = 1 on a decided
 *       ray gives a t at most that one.
 *   (d) Masks.  With masks that admit no instance every row is empty (all-hit) or all pads (first-K), counters[1] adds 0 and
 *       counters[0] adds exactly the TLAS slots examined.
 *   (e) One identity instance with no per_instance equals the single-tree filtered sibling (rt_ray_hits_collect_filtered /
 *       rt_ray_first_hits_filtered) with the same flags and per-ray records {mask, skip_id} for rays whose skip_instance is 0,
 *       on rays without -0 components, all instances 0.
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): all of the sibling's; a flag bit other than
 * RT_FILTER_CULL_BACK / RT_FILTER_CULL_FRONT in filter->flags; per_instance not 8-byte aligned; per_ray not 16-byte aligned.
 * num_instance_filters > 0 with a null per_instance is fine (an absent array).  Asynchronous and hipGraph-capturable like the
 * siblings.
 * Out of scope: per-primitive masks, instance motion, mixed / sphere BLASes, an indexed form, the host mirror and rt_cli. */
int rt_ray_hits_count_instanced_filtered(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                         const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                         const rt_instance_hit_filter* filter, uint64_t* offsets, void* scratch,
                                         uint64_t* counters, uint32_t* status, void* stream);
int rt_ray_hits_collect_instanced_filtered(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                           const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays,
                                           uint32_t num_rays, const rt_instance_hit_filter* filter, const uint64_t* offsets,
                                           rt_hit* hits, uint32_t* instance_ids, uint32_t* counts, uint64_t* counters,
                                           uint32_t* status, void* stream);
int rt_ray_first_hits_instanced_filtered(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                         const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                         uint32_t k, const rt_instance_hit_filter* filter, rt_hit* hits, uint32_t* instance_ids,
                                         uint64_t* counters, uint32_t* status, void* stream);

/* ---- indexed forms of the instanced and motion ray queries (no reference counterpart): the indexed-instanced block.
 * rt_sort_rays takes a TLAS as its tree, and secondary rays over a placed scene are the least coherent batches there are (the
 * lanes of one wave sit in different BLASes).  These four calls are their siblings through an index list, with exactly
 * rt_intersect_rays_indexed's contract, so a sorted order or a list of the rays still alive is traced without moving a
 * 32-byte ray record, a hit record or an instance id:
 *   rt_intersect_rays_instanced_indexed          sibling: rt_intersect_rays_instanced (filter == NULL) or
 *                                                rt_intersect_rays_instanced_filtered (any other filter) -- one entry point
 *                                                serves both, there is no separate filtered-indexed symbol
 *   rt_intersect_rays_instanced_motion_indexed   sibling: rt_intersect_rays_instanced_motion
 *   rt_intersect_rays_instanced_mixed_indexed    sibling: rt_intersect_rays_instanced_mixed (a null geom_table forwards to
 *                                                rt_intersect_rays_instanced_indexed as the sibling forwards to its own)
 *   rt_intersect_rays_motion_indexed             sibling: rt_intersect_rays_motion
 * The arguments are the sibling's in the sibling's order, with (order, num_indices) after num_rays and the output arrays
 * behind them, as in rt_intersect_rays_indexed.
 *   Index choice.  Lane j of the launch (j < num_indices, 64 consecutive j per wave) takes i = order[j].  If i >= num_rays
 *   (0xFFFFFFFF for instance) the lane does nothing.  The grid is sized by num_indices, which may exceed num_rays.
 *   Indexed by ray index.  Everything per ray goes by i, never by j: rays[i], times[i], filter->per_ray[i], hits[i],
 *   instance_ids[i], and the reload of the world ray when a lane leaves an instance.
 *   Written records.  For any index list each written hits[i] / instance_ids[i] equals the sibling's bytes (a ray's result
 *   does not depend on its wave neighbours; the kernel body after the choice of i is the sibling's).  Records whose index
 *   is not listed are not written, in neither array; a duplicated index writes the same bytes twice.
 *   Counters.  When order is a permutation counters[0] and [1] equal the sibling's; with the identity list all four do;
 *   [2] / [3] (wave steps) depend on the order: they measure its coherence.
 *   Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): all of the sibling's, plus a null order or one
 *   not 4-byte aligned.  num_indices = 0 (like num_rays = 0) runs nothing; errors win over both.
 *   Asynchronous: no host copy, no synchronisation, one launch -- hipGraph-capturable on one stream, behind rt_sort_rays.
 * Out of scope: indexed forms of the set-valued queries (all-hit and first-K, flat or instanced: their row / CSR layout by ray
 * index is a design of its own); a sort key that knows about instances (rt_sort_rays sees the TLAS root box only); the host
 * mirror and rt_cli. */
int rt_intersect_rays_instanced_indexed(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                        const rt_accel* blas_table, uint32_t num_blas, const rt_ray* rays, uint32_t num_rays,
                                        const uint32_t* order, uint32_t num_indices, rt_hit* hits, uint32_t* instance_ids,
                                        int mode, uint32_t num_primitives, const rt_instance_hit_filter* filter,
                                        uint64_t* counters, void* stream);
int rt_intersect_rays_instanced_motion_indexed(const rt_motion_accel* tlas, const rt_motion_instance_record* records,
                                               uint32_t num_instances, const rt_accel* blas_table, uint32_t num_blas,
                                               const rt_ray* rays, const float* times, uint32_t num_rays, const uint32_t* order,
                                               uint32_t num_indices, rt_hit* hits, uint32_t* instance_ids, int mode,
                                               uint64_t* counters, void* stream);
int rt_intersect_rays_instanced_mixed_indexed(const rt_accel* tlas, const rt_instance_record* records, uint32_t num_instances,
                                              const rt_accel* blas_table, const rt_geometry* geom_table, uint32_t num_blas,
                                              const rt_ray* rays, uint32_t num_rays, const uint32_t* order, uint32_t num_indices,
                                              rt_hit* hits, uint32_t* instance_ids, int mode, uint64_t* counters, void* stream);
int rt_intersect_rays_motion_indexed(const rt_motion_accel* as, const rt_ray* rays, const float* times, uint32_t num_rays,
                                     const uint32_t* order, uint32_t num_indices, rt_hit* hits, int mode, uint64_t* counters,
                                     void* stream);

/* ---- triangle-overlap queries (no reference counterpart).  For each caller triangle: WHICH triangles of the tree it cuts --
 * the narrow phase of mesh-against-mesh collision, self-intersection of a deforming mesh, interpenetration checks -- through
 * any tree rt_intersect_rays takes (runs of 1..7 slots; an empty tree, count = 0, is accepted and every set is empty).
 * Everything that is not the predicate is the range-query block's, WORD FOR WORD, with rt_tri_overlaps_count /
 * rt_tri_overlaps_collect / RT_TRI_* read for rt_range_count / rt_range_collect / RT_RANGE_*: the CSR contract (offsets[0 .. n]
 * uint64 and one id array, query i owns ids[offsets[i] .. offsets[i+1])); count's offsets, scratch
 * (rt_tri_overlaps_scratch_bytes = rt_range_scratch_bytes: one uint64 per 256 queries, 256-byte aligned, no initialisation) and
 * three launches; collect's segments, `counts` and RT_TRI_TRUNCATED; both call patterns ((a) everything: count, read
 * offsets[num_queries] back, allocate ids, collect with the same offsets; (b) a fixed K per query: offsets[i] = i * K, one
 * collect pass, min(counts[i], K) of each segment are valid); the 64-entry stack (a dropped push sets RT_TRI_STACK_OVERFLOW,
 * the result is then a subset, and both calls drop the same pushes); the counters ([0] += non-NONE slots examined, [1] += leaf
 * records visited, [2] / [3] not touched, the same in both calls); num_queries = 0 (count still writes offsets[0] = 0, collect
 * does nothing); the traversal order of the ids; no allocation, no host copy, no synchronisation (hipGraph-capturable).
 *
 * queries: an array of rt_triangle (36 bytes, 4-byte aligned), P = (p0, p1, p2).
 * Not traced (count 0, no tests counted): a query with a non-finite component among its nine.  Degenerate query triangles (a
 * point, a segment) ARE traced.
 *
 * The predicate cuts(P, Q).  Q = (q0, q1, q2): a caller triangle, its corners in the caller's order (pair leaves go back through
 * rt_triangle_pair.rotations, exactly as the sphere range query un-rotates them).  float32, every operation rounded on its own
 * (no fused multiply-add):
 *     cross(a, b) = (a.y*b.z - a.z*b.y,  a.z*b.x - a.x*b.z,  a.x*b.y - a.y*b.x)
 *     dot(a, b)   = (a.x*b.x + a.y*b.y) + a.z*b.z
 *     a - b       componentwise
 * cuts is true iff both hold:
 *   1. Vertex boxes.  The two triangles' vertex boxes overlap on every axis with closed comparisons: RT_RANGE_BOX's triangle
 *      test with [lo, hi] = the query's fminf / fmaxf box (tlo <= hi && thi >= lo; a NaN coordinate of Q is dropped by fminf /
 *      fmaxf; -0 equals +0).
 *   2. No separating axis among seventeen.  All corners relative to p0:
 *        P' = (0, p1 - p0, p2 - p0)                 Q' = (q0 - p0, q1 - p0, q2 - p0)
 *        e0 = p1 - p0, e1 = p2 - p1, e2 = p0 - p2   f0 = q1 - q0, f1 = q2 - q1, f2 = q0 - q2
 *        nP = cross(e0, e1)                         nQ = cross(f0, f1)
 *      Axes, in this order: nP; nQ; cross(e_i, f_j) for i = 0..2 (outer), j = 0..2 (inner); cross(nP, e_i) for i = 0..2;
 *      cross(nQ, f_j) for j = 0..2.
 *      On an axis a: sP_k = dot(a, P'_k), sQ_k = dot(a, Q'_k), k = 0..2 (sP_0 = dot(a, 0) is computed like the others);
 *      minP = fminf(fminf(sP_0, sP_1), sP_2), maxP = fmaxf(fmaxf(sP_0, sP_1), sP_2), and minQ / maxQ alike.
 *      The axis SEPARATES iff minP > maxQ || minQ > maxP.  Strict: touching does not separate.  A NaN makes both comparisons
 *      false: a NaN does not separate.
 *   The six in-plane axes make coplanar and coincident triangles come out right, where the nine edge crosses vanish.  A zero
 *   axis never separates (degenerate triangles).  Overflow gives inf or NaN and hence a match.  Accuracy: the projections are
 *   products of degree 4 in the coordinate differences, so differences beyond about 2^31 overflow float32; the result there is
 *   still deterministic and equal to this text, but it is not an accurate intersection test (as the closest-point block says of
 *   its own overflow).  The answer does not depend on the order the axes are evaluated in (a
 *   conjunction); the kernel leaves at the first separating axis.
 *
 * Slot test.  A non-NONE slot is skipped iff its box fails the closed overlap test against the query's vertex box (the
 * RT_RANGE_BOX slot test).  Condition 1 is part of the predicate and uses nothing but min, max and comparisons, so skipping loses
 * nothing.
 * Result: a SET -- no ordering promise and no tie rule.
 *   - exact (the brute-force set { k : cuts(P, tri[k]) } over the caller's triangles, each id once) on every tree whose slot
 *     boxes contain the vertex boxes below them: LBVH, pairs, hybrid, hybrid + pairs, SAH, SAH + pairs, and every refitted tree;
 *   - spatial-split trees (rt_run_sah_build with enable_splits): the leaf test is on the whole triangle, so every reported id
 *     is a true match; but an id appears once per REFERENCE that is reached (duplicates are possible), and a triangle is missed
 *     when every one of its clipped references lies outside the query's vertex box.  Refitting a split tree restores exactness
 *     up to the duplicates: refit writes unclipped boxes, but the references stay.
 *
 * flags: 0 or RT_TRI_SELF.  RT_TRI_SELF: the caller passes the triangles the tree was built over (after a refit: the moved
 * ones), and query i IS triangle i.  Candidate j is reported iff cuts holds and
 *   - j > i, and
 *   - no corner of j equals a corner of i: nine corner comparisons, two corners being equal when all three components are float
 *     == (as the pairing test compares corners: -0 == +0, a NaN equals nothing).
 * Every intersecting pair without a shared corner therefore appears once, in row min(i, j).  Without the flag nothing is
 * excluded: a query identical to a scene triangle matches that triangle.
 *
 * Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): a null as / queries / offsets / scratch (count) /
 * ids (collect), a tree with count > 0 and a null node or leaf pointer, count > 7, a flag bit other than RT_TRI_SELF, queries
 * not 4-byte, offsets not 8-byte, ids / counts / status not 4-byte, scratch not 256-byte aligned. */
enum { RT_TRI_SELF = 1 };
enum { RT_TRI_STACK_OVERFLOW = 1, RT_TRI_TRUNCATED = 2 };
size_t rt_tri_overlaps_scratch_bytes(uint32_t num_queries);
int rt_tri_overlaps_count(const rt_accel* as, const rt_triangle* queries, uint32_t num_queries, uint32_t flags,
                          uint64_t* offsets, void* scratch, uint64_t* counters, uint32_t* status, void* stream);
int rt_tri_overlaps_collect(const rt_accel* as, const rt_triangle* queries, uint32_t num_queries, uint32_t flags,
                            const uint64_t* offsets, uint32_t* ids, uint32_t* counts, uint64_t* counters,
                            uint32_t* status, void* stream);

/* ---- signed distance and occupancy (no reference counterpart).  For each caller point: how far is the nearest triangle, and is
 * the point INSIDE the closed mesh the tree was built over -- the two calls mesh-query libraries offer next to closest points
 * (SDF volumes for marching cubes, collision margins, voxelisation, point-in-solid tests), through any tree rt_intersect_rays
 * takes (runs of 1..7 slots; an empty tree, count = 0, is accepted: every query is a miss and outside).  One launch per call;
 * both halves of the result are defined by blocks above, so the result equals a composition of rt_closest_points and
 * rt_ray_hits_count bit for bit.
 *
 * Queries: rt_point_query records (p, dist2_max), with rt_closest_points's liveness rule: a query with a non-finite component
 * of p, a NaN dist2_max or a negative dist2_max is not traced by either call -- its output is {+inf, RT_MISS} / inside = 0 and no
 * tests are counted for it.  rt_occupancy uses dist2_max for this rule and for nothing else.
 *
 * Distance half (rt_signed_distance).  (dist2, primitive_id) is EXACTLY the pair rt_closest_points reports for the query: the
 * lexicographic minimum of (d2, id) over the triangles with d2 <= dist2_max, d2 the closest-point block's float32 routine
 * (Ericson, the clamp into the vertex box, the squared distance) on the caller's corners in the caller's order, the search
 * started from (dist2_max, RT_MISS), a slot or a popped entry skipped iff boxdist2 > best (never on equality), the same visiting
 * order (nearest surviving slot first, ties to the lower slot), the same restarts (below).  Hence the same exactness statement:
 * bit for bit the brute force on LBVH, pairs, hybrid, hybrid + pairs, SAH, SAH + pairs and every refitted tree; on spatial-split
 * trees dist2 is d2(p, tri[primitive_id]) bit for bit and sqrt(dist2) exceeds the brute-force minimum by at most 2^-20 * M.
 *   |sdist| = sqrtf(dist2), the correctly rounded float32 square root.  No query triangle within the radius: primitive_id =
 *   RT_MISS and |sdist| = +inf; the sign is computed all the same (a point deep inside with a small radius gives -inf).
 *   No weights are reported: a caller who wants the closest point itself calls rt_closest_points.
 *
 * Sign half (both calls).  Vote j < votes casts the ray (origin = p, tmin = 0, dir = D[j], tmax = +inf) and takes its crossing
 * count c_j = the length of the row the all-hit block defines for that ray: the same slot test (back >= front && front <= tmax
 * && back >= tmin on rt_trace's slab test, 1/dir computed once per vote by IEEE division), the same leaf test (rt_trace's
 * Moller-Trumbore on the stored corners, A = (v0, v1, v2), and B = (v2, v1, v3) iff v3 != v2 bit for bit), the window fixed for the
 * whole traversal.  As there, c_j is a function of the tree's bytes and the ray alone.
 *   inside = (number of j with c_j odd) * 2 > votes
 *   sdist  = inside ? -|sdist| : |sdist|, except that dist2 == 0 always gives +0 (a point on the surface has no side).
 * votes is 1 or 3 (RT_SDF_MAX_VOTES).  With votes = 3 a query whose first two votes agree does NOT cast the third: the majority
 * is already decided, so the result is the same -- but the counters below see two traversals for it, not three.
 * dirs: a HOST pointer to 3 * votes floats (D[j] = dirs[3j .. 3j+2]), copied into the kernel arguments at call time, or null for
 * the default directions
 *   D0 = ( 0.577f,  0.211f, 0.789f)
 *   D1 = (-0.683f,  0.619f, 0.387f)
 *   D2 = ( 0.259f, -0.857f, 0.446f)
 * -- not normalised (nothing here needs it), not axis-aligned, no two components of equal magnitude, so none of them runs along
 * the edges or diagonals of an axis-aligned lattice or box.  A caller direction with a zero or non-finite component is accepted
 * exactly as rt_ray_hits_count accepts it (1/0 = inf in the slab test); a NaN component makes that vote's ray dead: c_j = 0, even.
 *
 * What the sign means -- and where it means nothing:
 *   - only for a CLOSED mesh: there, every ray from a point crosses the surface an odd number of times iff the point is inside.
 *     For an open mesh the votes are still the parities defined above, but "inside" has no meaning;
 *   - only on trees where each triangle sits in one leaf: LBVH, pairs, hybrid, hybrid + pairs, SAH, SAH + pairs and their refits.
 *     On spatial-split trees (rt_run_sah_build with enable_splits) a triangle is counted once per reached REFERENCE, so the
 *     parity and the sign mean nothing there, and refit does not repair it (the references stay).  The distance half keeps the
 *     closest-point block's statement for split trees.  rt_accel carries no flag that says "split tree", so the library CANNOT
 *     refuse one: the caller must not ask a split tree for a sign;
 *   - Moller-Trumbore here is not watertight: a ray through a shared edge or corner can be counted zero or two times instead of
 *     once.  That is what the vote is for: three directions rarely graze edges for the same point.  With votes = 1 the caller
 *     gets the raw parity of one ray.
 *
 * Stack: 64 pending entries per query in either half, as in the blocks they come from; a push beyond them is dropped.  A
 * distance pass that dropped a push is run again from the root with the best so far, at most twice (rt_closest_points's rule).
 * RT_SDF_STACK_OVERFLOW is ORed into *status when the last distance pass of a query still dropped a push (its record is an
 * exact (d2, id) of a real triangle but may not be the nearest), or when any parity traversal of a query dropped a push (its
 * count is then a lower bound, so its parity -- and the sign -- is unknown).
 * counters: optional device uint64[4]: [0] += non-NONE slots examined, [1] += leaf records visited, both summed over every
 * traversal that actually ran (every distance pass, every vote that was cast); [2] / [3] are not touched.  One LDS reduction +
 * 2 device atomics per workgroup of 256 queries.  status: optional device uint32 the calls OR flags into (the caller clears it).
 * rt_signed_distance: out[i] for queries[i], i < num_queries, one 8-byte record; rt_occupancy: inside[i] = 0 or 1, one byte;
 * nothing is written at i >= num_queries.  Asynchronous (no allocation, no host copy, no synchronisation: hipGraph-capturable;
 * dirs is read on the host during the call).  num_queries = 0 with valid arguments: nothing runs.
 * Argument errors, returned before any GPU work and before the empty-batch return (RT_ERR_INVALID_ARGUMENT): a null as / queries /
 * out / inside, a tree with count > 0 and a null node or leaf pointer, count > 7, votes not 1 or 3, queries not 16-byte
 * aligned, out not 8-byte aligned, status not 4-byte aligned.
 *
 * rt_generate_grid_points: the lattice counterpart of rt_generate_camera_rays.  Point (i, j, k), i < dims[0], j < dims[1],
 * k < dims[2], is p = (origin[0] + (float)i * spacing[0], origin[1] + (float)j * spacing[1], origin[2] + (float)k * spacing[2])
 * -- float32, one multiplication and then one addition per component, each rounded on its own (no fused multiply-add) -- with
 * the given dist2_max.  origin, spacing, dims: HOST pointers read during the call.  Layouts:
 *   RT_GRID_ROW_MAJOR  dims[0]*dims[1]*dims[2] records; point (i, j, k) at index (k*dims[1] + j)*dims[0] + i
 *   RT_GRID_BRICKS     nbx*nby*nbz*64 records, nb = ceil(dims / 4) per axis; brick (bx, by, bz) has number (bz*nby + by)*nbx + bx
 *                      and holds its 64 points at brick*64 + lane, point (4*bx + lx, 4*by + ly, 4*bz + lz) with lane the 3-D
 *                      Morton code of the offset: lx = lane bits 0, 3, ly = bits 1, 4, lz = bits 2, 5 -- one wave of either
 *                      query gets one 4 x 4 x 4 brick.  Off-lattice lanes of edge bricks get {0, 0, 0, -1}: a negative radius,
 *                      so the query is not traced.
 * queries: 16-byte aligned device array of that many records.  Asynchronous, hipGraph-capturable.  A lattice with a zero
 * dimension: nothing runs.  Errors, before any GPU work: a null origin / spacing / dims / queries, queries not 16-byte aligned
 * or a bad layout (RT_ERR_INVALID_ARGUMENT); a record count that does not fit 32 bits (RT_ERR_TOO_LARGE). */
typedef struct rt_sdf_hit { float sdist; uint32_t primitive_id; } rt_sdf_hit;
#define RT_SDF_MAX_VOTES 3
enum { RT_SDF_STACK_OVERFLOW = 1 };
int rt_signed_distance(const rt_accel* as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes,
                       const float* dirs, rt_sdf_hit* out, uint64_t* counters, uint32_t* status, void* stream);
int rt_occupancy(const rt_accel* as, const rt_point_query* queries, uint32_t num_queries, uint32_t votes,
                 const float* dirs, uint8_t* inside, uint64_t* counters, uint32_t* status, void* stream);
enum { RT_GRID_ROW_MAJOR = 0, RT_GRID_BRICKS = 1 };
int rt_generate_grid_points(const float origin[3], const float spacing[3], const uint32_t dims[3], float dist2_max,
                            int layout, rt_point_query* queries, void* stream);

/* ---- deferred shading (no reference counterpart: the reference shades inside TraceRays, Tracer.cu:471-595).  The ray queries
 * give (t, primitive_id, u, v) records; these two calls turn records into rt_trace's frames:
 *   rt_generate_camera_rays -> rt_intersect_rays(closest) -> [rt_generate_shadow_rays -> rt_intersect_rays(any hit)] ->
 *   rt_shade_frame            (the bracketed pair for RT_RENDER_TEXTURE_LIT_SHADOWS only)
 *
 * rt_generate_shadow_rays writes shadow_rays[i] for i < num_rays at the index of its primary ray, so the row-major or tiled
 * layout carries over.  light: HOST float[3] (rt_scene.light).
 *   Hit (hits[i].primitive_id < num_triangles, and rays[i] alive: tmin <= tmax, no NaN in origin or direction).  float32, every
 *   operation rounded on its own (no fused multiply-add), IEEE division and square root:
 *     hp = origin + dir * t                          per component, t = hits[i].t
 *     l  = light - hp
 *     to_light = sqrtf((l.x*l.x + l.y*l.y) + l.z*l.z)
 *     linv = 1.0f / to_light
 *     shadow ray: origin = hp, dir = l * linv, tmin = 0.001f, tmax = to_light
 *   -- the expressions, in the order, that rt_trace's RT_RENDER_TEXTURE_LIT_SHADOWS sample compiles (a + b + c is (a + b) + c).
 *   Miss, or a dead primary ray: a dead ray, origin 0, dir 0, tmin 0, tmax -1.
 *   A shadow ray is occluded when rt_intersect_rays(..., RT_RAY_ANY_HIT) returns a hit for it.  rt_trace decides shadow with a
 *   closest-hit traversal; any hit accepts a triangle exactly where closest hit does, so the boolean is the same.
 *   One divergence: with the hit point at the light (to_light = 0: a NaN direction) or within 0.001 of it (tmin > tmax) the
 *   shadow ray is dead for the query, i.e. unshadowed, while rt_trace still runs its traversal there.
 *
 * rt_shade_frame: one RGBA8 pixel from the spp records of each pixel -- rt_trace's stratified sample order, its float sums
 * (sum += sample; sum / (float)spp), its float -> u8 conversion; row 0 first, pitch 4*w.  spp in {1, 4, 16}; layout and the
 * index of sample s of pixel (x, y) are rt_generate_camera_rays's (tiled: off-frame lanes of edge tiles are not read and write
 * nothing).  Inputs: scene (attributes, materials, textures, light and the three counts; scene->camera is NOT read), the
 * caller's triangles[num_triangles] (no tree), rays, hits, and shadow_hits (required for RT_RENDER_TEXTURE_LIT_SHADOWS --
 * only its primitive_id is read: < num_triangles = occluded -- and ignored otherwise).
 *   A record is a hit iff primitive_id < num_triangles.  Anything else (RT_MISS, garbage, the record of a dead ray) shades as
 *   rt_trace's miss, whatever its other fields hold.
 *   A hit is shaded as rt_trace shades it (Tracer.cu:506-593) from the ray rays[i] with tmax = hits[i].t, barycentrics
 *   (hits[i].u, hits[i].v), the triangle triangles[primitive_id] and attribute corners 0, 1, 2 in the caller's order
 *   (rotation 0), spread = 2.0f / w; material and texture indices are range-checked as in rt_trace.  RT_RENDER_DEPTH takes
 *   max_depth from the ray's own tmax (rt_generate_camera_rays sets it to camera->max_depth).
 *   Render types: RT_RENDER_DEPTH, MATERIAL_ID, LODS, DIFFUSE, TEXTURE, TEXTURE_LIT, TEXTURE_LIT_SHADOWS.  RT_RENDER_BOXTESTS
 *   and RT_RENDER_TRIANGLE_TESTS need per-ray test counts, which a record does not carry: RT_ERR_UNSUPPORTED, nothing runs.
 *   The frame is a function of the records and the caller's data only; it does not depend on which tree produced the hits.
 *   Every single-triangle leaf stores the caller's corners unrotated (refit notes above), split references included, so on
 *   every non-pair tree (LBVH, hybrid, SAH, SAH with splits) the pipeline's frame equals rt_trace's BYTE FOR BYTE.  On pair
 *   trees the records were computed on rotated corners and mapped back: the frame equals rt_trace's up to float32 rounding.
 * Both calls are asynchronous (no allocation, no host copy, no synchronisation: hipGraph-capturable).  num_rays = 0 / w*h = 0:
 * nothing runs.  Argument errors, returned before any GPU work (RT_ERR_INVALID_ARGUMENT): null pointers (scene, triangles,
 * rays, hits, rgba8, light, shadow_rays; attributes / materials / textures where rt_trace requires them), rays, hits,
 * shadow_rays or shadow_hits not 16-byte aligned, rgba8 or triangles not 4-byte aligned, a bad spp, layout or render_type,
 * RT_RENDER_TEXTURE_LIT_SHADOWS with a null shadow_hits. */
int rt_generate_shadow_rays(const rt_ray* rays, const rt_hit* hits, uint32_t num_rays, uint32_t num_triangles,
                            const float* light, rt_ray* shadow_rays, void* stream);
int rt_shade_frame(const rt_scene* scene, const rt_triangle* triangles, uint32_t num_triangles, const rt_ray* rays,
                   const rt_hit* hits, const rt_hit* shadow_hits, uint32_t w, uint32_t h, uint32_t spp, int layout,
                   int render_type, uint8_t* rgba8, void* stream);

/* ---- instanced deferred shading (no reference counterpart).  rt_shade_frame for the records of the INSTANCED ray queries: an
 * instanced record's primitive_id indexes a BLAS's own triangles in object space, so rt_shade_frame's one flat triangles[] /
 * attributes[] cannot serve it without flattening every instance on the host.  The chain:
 *   rt_generate_camera_rays -> rt_intersect_rays_instanced -> rt_generate_shadow_rays(num_triangles = RT_MISS) ->
 *   rt_intersect_rays_instanced(any hit) -> rt_shade_frame_instanced       (the middle pair for RT_RENDER_TEXTURE_LIT_SHADOWS only)
 * rt_generate_shadow_rays needs only the world ray and the world-space t, which the instanced query preserves: with
 * num_triangles = RT_MISS every record but a miss is a hit, which is right for instanced records.  The any-hit instanced query
 * gives the occlusion bit as an instance id.  The records of rt_intersect_rays_instanced_filtered and of
 * rt_intersect_rays_instanced_motion work unchanged; for instance motion the caller passes the rt_instance array and the
 * rt_prepare_instances records of the pose they want shaded.
 *
 * rt_shade_geometry (32 bytes; a DEVICE array parallel to the BLAS table, 16-byte aligned): what a hit in blas_table[b] is
 * shaded from -- the BLAS's CALLER triangles (object space, the build input, not its tree), one rt_attributes per triangle,
 * their count, and material_base, added to attributes[].material_id (several meshes, one concatenated material table).
 *
 * Sample i is a HIT iff, with k = instance_ids[i]: k < num_instances, records[k].flags == 0, b = records[k].blas < num_blas,
 * geometry[b].triangles and geometry[b].attributes are non-null, and p = hits[i].primitive_id < geometry[b].num_triangles.
 * Anything else (RT_MISS, garbage, the record of a dead ray) shades as rt_shade_frame's miss, whatever the other fields hold;
 * nothing is read through an index that failed its check.
 * A hit, with M = instances[k].object_to_world and W = records[k].world_to_object (float32, every operation rounded on its own):
 *   corner c of geometry[b].triangles[p]:  row r = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3]   (rt_prepare_instances's order)
 *   normal of corner c:                    n'_r = (W[0][r]*nx + W[1][r]*ny) + W[2][r]*nz             (the transpose of W's 3x3:
 *                                          the inverse-transpose of M, the normal matrix)
 *   flags & RT_SHADE_RENORMALIZE:          l2 = (n'x*n'x + n'y*n'y) + n'z*n'z; if l2 > 0 and finite, n'' = n' * (1.0f / sqrtf(l2));
 *                                          otherwise, and without the flag, n' is used as it is.  The lit shaders do not normalise
 *                                          the interpolated normal, so a scaled instance is lit wrongly without the flag; it is a
 *                                          flag because an identity instance must give rt_shade_frame's bytes
 *   uv:                                    unchanged
 *   material id:                           attributes[p].material_id + geometry[b].material_base (int32, wrapping); if
 *                                          instance_materials is non-null and instance_materials[k] >= 0, instance_materials[k];
 *                                          then rt_shade_frame's range checks (outside the table: material 0)
 *   then exactly rt_shade_frame's per-sample path: the ray rays[i] with tmax = hits[i].t, barycentrics (u, v), rotation 0,
 *   spread = 2.0f / w, the same render types (RT_RENDER_BOXTESTS / RT_RENDER_TRIANGLE_TESTS: RT_ERR_UNSUPPORTED), the same
 *   spp {1, 4, 16} accumulation, row-major / 8x8-tiled sample indexing and float -> u8 store.
 *   RT_RENDER_TEXTURE_LIT_SHADOWS: shadowed iff shadow_instance_ids[i] < num_instances.
 *   A MIRRORED instance (negative determinant) keeps its corner order, so the tangent frame's geometric normal (the cross
 *   product of the placed edges) flips against the placed shading normals -- as it does in the flattened scene.
 * Contract: the frame EQUALS rt_shade_frame's on the flattened scene -- the placed corners, the placed normals and the resolved
 * material ids as one triangle and one attribute array, hit records whose primitive_id is the flattened index -- byte for byte,
 * in every supported mode, layout and spp.  One identity instance without RT_SHADE_RENORMALIZE equals rt_shade_frame on the
 * BLAS's own arrays byte for byte, for data without -0 components (-0 + 0 = +0).
 * Out of scope: sphere BLASes of the mixed query (their table entry, with null pointers, shades as a miss); interpolated-pose
 * shading for instance motion; the host mirror; rt_cli.
 * Asynchronous (no allocation, no host copy, no synchronisation: hipGraph-capturable).  w*h = 0: nothing runs.  num_instances = 0
 * with null geometry / instances / records is legal: every pixel is a miss.  Argument errors, returned before any GPU work
 * (RT_ERR_INVALID_ARGUMENT): null pointers (scene, rays, hits, instance_ids, rgba8; geometry, instances, records when
 * num_instances > 0; materials / textures where rt_shade_frame requires them -- scene->attributes is NOT read), geometry,
 * instances, records, rays or hits not 16-byte aligned, instance_ids, shadow_instance_ids, instance_materials or rgba8 not
 * 4-byte aligned, a bad spp, layout or render_type, unknown flag bits, RT_RENDER_TEXTURE_LIT_SHADOWS with a null
 * shadow_instance_ids, num_instances > 0 with num_blas = 0. */
typedef struct rt_shade_geometry {      /* 32 bytes; DEVICE array parallel to the BLAS table */
    const rt_triangle*   triangles;     /* the BLAS's caller triangles (object space), not its tree */
    const rt_attributes* attributes;    /* one per triangle */
    uint32_t num_triangles;
    int32_t  material_base;             /* added to attributes[].material_id (one concatenated material table) */
    uint32_t pad[2];
} rt_shade_geometry;
enum { RT_SHADE_RENORMALIZE = 1 };
int rt_shade_frame_instanced(const rt_scene* scene, const rt_shade_geometry* geometry, uint32_t num_blas,
                             const rt_instance* instances, const rt_instance_record* records, uint32_t num_instances,
                             const int32_t* instance_materials, const rt_ray* rays, const rt_hit* hits,
                             const uint32_t* instance_ids, const uint32_t* shadow_instance_ids, uint32_t w, uint32_t h,
                             uint32_t spp, int layout, int render_type, uint32_t flags, uint8_t* rgba8, void* stream);

/* static string for a return code */
const char* rt_error_string(int code);

/* library / kernel configuration, for logs: e.g. "rt_amd gfx950 sort=8bit x4 tile=4096 ..." */
const char* rt_version_string(void);

#ifdef __cplusplus
}
#endif
#endif
