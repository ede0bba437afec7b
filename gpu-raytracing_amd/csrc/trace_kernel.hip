// trace_kernel.hip -- primary-ray generation, BVH traversal, intersection, shading, RGBA8 store.
//
// Replaces TraceRays / TraceRay / IntersectRayAabb / IntersectRayTriangle(Pair) / AmbientShader
// (Tracer.cu:187-200, 256-374, 376-469, 471-595).  Per-ray semantics -- and therefore the per-ray box /
// triangle test counts, which are OUTPUTS of the kBoxtests / kTriangleTests modes -- follow the
// reference exactly: children visited in slot order, a leaf hit is intersected before the next slot's
// box is compared against tmax, the nearest Box child is continued first (ties: larger child index),
// the others are pushed in encounter order, popped entries are not re-culled.
//
// Machine mapping for wave64 (what differs from the reference's one-thread-one-ray loop):
//   * one wave = one 8x8 pixel tile (Morton order inside the tile): the 64 rays walk the same upper
//     tree, their 64-byte sibling-pair loads hit the same lines (L1 hit rate 97 % on the bench scene);
//   * a sibling pair (2 x 32-byte slots, 64-byte aligned) is fetched with four 16-byte loads issued
//     together; front/back of BOTH boxes are computed at once (they do not depend on tmax), the
//     tmax/tmin comparisons are then applied in slot order;
//   * WAVE-LEVEL TWO-PHASE SCHEDULE: a leaf hit is rare per ray (about 1 in 70 steps) but almost
//     certain per 64-lane step, and the triangle test is the long divergent path.  A lane that needs a
//     leaf test parks (phase LEAF0 / LEAF1, keeping the second slot's front/back in registers) and the
//     wave keeps stepping boxes for the others; when parked lanes outnumber stepping lanes
//     (one __builtin_amdgcn_ballot_w64 pair per step) the wave runs ONE leaf phase for all of them.
//     Only the interleaving ACROSS lanes changes; each ray's own sequence of tests is untouched;
//   * HOLD AT POP (quad_hold, rt_traverse.hpp; the instantiations trace_quad_wait() names): the address path charges a quad
//     ONE request for a load only when its lanes carry one address, and the four rays of a 2 x 2 pixel quad visit nearly the
//     same pairs a step or more apart.  A lane that has just popped entry E from level s of its stack sits out the FIRST
//     box step of a vote while a quad-mate still holds E at level s of its own (the mate is deeper in the subtree both
//     took first); the rule is asked once per vote, the vote counts the lanes that will take that first step, and the
//     second step under the vote steps every lane in PH_STEP, held ones included.  A held lane keeps its phase; a mate
//     that pops E in the meantime steps on it with the held lane, one address, one request.  Again only the
//     interleaving across lanes changes.  Nobody waits for ever: see the comment at quad_hold;
//   * HOLD BY STACK DEPTH, BEFORE BOTH STEPS (quad_hold_sp, RT_TRACE_HOLD_FIRST / RT_TRACE_HOLD_SECOND = 1, rt_traverse.hpp; shipped in
//     the place of the entry test above, which is what both knobs at 0 build): the same rule without looking at the stack --
//     a lane that has just popped from level s < 16 sits a box step out while an unfinished quad-mate's sp is greater than s.
//     The mate is deeper, most often in the subtree both took first.  It is sp alone, already in a register: four quad-perm
//     DPP moves folded into a max and one compare, no ds_read_b128, no branch, no wait in front of the loads -- cheap enough
//     to ask before the SECOND step of a vote as well, where the entry test lost.  The second step's lane
//     mask is PH_STEP && exact_cur(cur) && !hold; a lane that sits out keeps PH_STEP_POP and pushes nothing, so the lean
//     margin stands.  The unfinished lane of a quad with the greatest sp never holds: every pass still steps a lane or runs
//     a leaf phase.  Measured on the headline: 43 % fewer L1 lookups, TA busy -12 %, 8 % more wave steps, +4.1 % with frames in
//     flight and +1.8 % one frame at a time (profiles/hold_second_bench.txt, hold_second_pmc.txt);
//   * TWO ARMS OF A VOTE (the same instantiations; kLeanMargin, rt_traverse.hpp): one more ballot per vote asks whether any
//     unfinished lane has more than kStackLds - 4 = 12 stack entries.  If none has, the vote is LEAN: every push and pop of
//     its two box steps, and of the leaf phase if the vote ends the box phase, is one ds_write / ds_read on the LDS column
//     behind a scalar branch -- a lane pushes at most four entries under a vote, so the column cannot overflow.  Otherwise
//     the vote is FULL: the same sites take the LDS / private / dropped ladders.  One stack, one sp; a wave may change arm
//     at every vote, a ray's sequence of tests is the same in both.  The bench scenes peak at 10 entries and run lean
//     throughout: 3.1 % fewer issued instructions per launch, +1.6 %;
//   * TWO FORMS OF A BOX STEP (the same instantiations; RT_TRACE_PAIR_STEP / pair_step_on, rt_traverse.hpp): the nearest
//     Box child is carried from step to step only inside a node of more than two slots -- advance() resets it at the end of
//     every other pair, so in an LBVH, a pairs tree or a hybrid tree every pair is entered without one.  One more ballot per
//     vote asks whether any unfinished lane carries a near or sits on anything but a pair below index 2^27 - 1 (exact_cur:
//     one compare on the packed word).  If none does, the vote is EXACT: both of its steps decide slot 0, slot 1, the one
//     possible push and the advance from values of the step alone -- no push site for slot 0, no compare against a carried
//     front, near_e / near_d written only where they outlive the step (a leaf in slot 1) -- and fetch the pair at scalar
//     base + (cur << 5) as a 32-bit lane offset, four loads off one register with no 64-bit arithmetic (the launch gets a
//     node pointer, not a node count: the vote establishes from the data that the offset fits).  A lane whose cur is not
//     exact after the first step -- a lone slot, a wider node, a pair beyond 4 GiB -- sits the second step out and makes the
//     next vote a general one.  Any other vote runs the general step.  One traversal state; a wave may change form at every
//     vote, a ray's sequence of tests is the same in both.  The forms stand one after the other in the loop, each behind its
//     own scalar branch, so that neither moves the lanes' state between registers.  The bench tree has only exact entries:
//     every vote the narrow rule ran narrow is exact, 98 - 99 % of them (profiles/exact_pair_model.txt), and no lane sits
//     out.  The pair-local tests: 7.8 % fewer issued instructions per launch, +3.6 %; the short address on top of them:
//     5.8 % fewer, +1.0 % at 1 spp, +6 % at 16 spp, where the four loads of a pair now issue together;
//   * a leaf (64 bytes) is fetched with four 16-byte loads issued together, the words no test reads included: left to
//     itself the compiler narrows them to seven smaller requests, and the address path charges per request;
//   * the traversal stack is a lane-interleaved LDS column addressed through an address_space(3)
//     pointer (ds_read/ds_write; conflict-free: bank = lane % 32 in both 32-lane halves); an entry is
//     one packed dword child:29|count:3; entries beyond the LDS depth spill to private memory;
//   * the reference's push-then-pop of the nearest child is kept in a register instead;
//   * 1/direction is computed once per ray (bit-identical to recomputing it per box: IEEE division);
//   * test counters are wave-reduced and added with ONE 64-bit atomic pair per wave (reference: one
//     atomic per ray, Tracer.cu:503);
//   * workgroups are dealt to XCDs round-robin by the hardware; the tile order is remapped so that an XCD
//     takes runs of 8 consecutive workgroups (256 x 8 pixels) spread over the whole frame: neighbouring
//     rays share an L2, and every XCD gets its share of the expensive parts of the image.
// Compiled with -ffp-contract=off: results are bit-identical to the C oracle.
#include <cstdio>
#include <cstdlib>

#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_math.h"
#include "rt_shade.hpp"      // the shading helpers (shared with shade.hip)
#include "rt_traverse.hpp"   // Ray, Hit, Trav, box_step, trace_ray, camera_ray (shared with ray_query.hip)

namespace rt {

// (the traversal constants kStackLds, kStackMax, kPrefetchMinPrims, kTraceWaves live in rt_traverse.hpp)
// Tuning build only (make TUNING=1 -> -DRT_TRACE_TUNING; never in the shipped library): render type 100 writes the raw
// u32 box-test count per pixel (tools/divergence_stats.py) and RT_TRACE_PARK="num,den" overrides the park threshold.
#ifdef RT_TRACE_TUNING
constexpr int kRenderDebugBoxCount = 100;
#else
constexpr int kRenderDebugBoxCount = -1;   // matches no render type: every use below folds away
#endif
// (the park threshold kParkNum / kParkDen: rt_traverse.hpp)
// A workgroup's four tiles: 4 x 1 (32 x 8 px, consecutive in row-major tile order).  (A 2 x 2 arrangement, 16 x 16 px, was
// measured no faster and retired: DESIGN section 5)


// ---- publication of the test counters (see the end of trace_kernel).  The caller's four counters are ONE 32-byte target
// for every workgroup of a frame, and same-address device atomics queue at the memory side at ~18 ns each: 8,100
// workgroups = 0.15 ms behind which a sparse frame waits (camera B of the bench: 2,690 instead of 3,330 Mrays/s serial).
// So a launch borrows one of kCtrSlots slots of module-static device memory: workgroup b adds its sums into row b mod
// kCtrSub of the slot (16 queues instead of one) and takes a ticket on that row; the last ticket of a row takes a ticket on the
// slot; the last of those folds the 16 rows into the caller's counters and leaves the slot zeroed (nobody waits; the
// "last arriver continues" hand-off of lbvh_levels.hip).  Slots are handed out round-robin by launch_trace: two launches
// share one only if more than kCtrSlots launches with counters are in flight at once.
constexpr uint32_t kCtrSlots = 256, kCtrSub = 16;
struct alignas(64) CtrSlot {
    // one 64-byte line per row: [box, tri, box-phase steps, leaf-phase steps, the row's tickets, pad x 3] -- the ticket lives
    // in its row's line: sixteen tickets in ONE line would queue exactly like the single target this replaces
    unsigned long long part[kCtrSub][8];
    unsigned long long top, pad[7];
};
__device__ CtrSlot g_ctr[kCtrSlots];

struct TraceParams {
    const rt_node* nodes;
    const rt_triangle_pair* leaves;
    const rt_attributes* attributes;
    const rt_material* materials;
    const rt_texture* textures;
    const rt_camera* camera;
    float light[3];
    uint32_t root, count, num_materials, num_textures;
    uint8_t* rgba8;
    uint32_t w, h, y0, y1, spp;
    unsigned long long* counters;
    uint32_t tiles_x, num_tiles;
    // interleaved strips (rt_trace_strips): strip_tiles > 0 tile rows per strip; tile row t of the launch is row
    // (t % strip_tiles) of strip  strip_first + (t / strip_tiles) * strip_stride  and is stored at tile row t (compactly)
    uint32_t strip_tiles, strip_first, strip_stride;
    int park_num, park_den;
    uint32_t ctr_slot;   // counters != null: this launch's slot of g_ctr
};


// (the device shading helpers -- colour conversion, texture sampling, ComputeLOD, TangentMatrix, Bump2Normal -- live in
// rt_shade.hpp, shared with shade.hip.  shade_sample below keeps its own text of the shaders after the hit: routing it through
// rt_shade.hpp's shade_unlit / shade_lit changed the instruction order and spill counts of modes 3 and 5-8)

// Which instantiations can hold at pop (rt_traverse.hpp quad_hold): RT_TRACE_QUAD_WAIT = 1 the 64-VGPR ones (kDepth / kBoxtests /
// kTriangleTests) of cache-resident scenes, 2 the shaded ones as well (both traversals of kTextureLitShadows), 0 none.  The
// PF instantiations wait for L2 misses, not for the address path, and keep the plain loop.  Each such instantiation exists
// with and without the rule (trace_kernel's QW) and launch_trace picks by tree: see there.  How each was decided: DESIGN section 5.
constexpr bool trace_quad_wait(int render, bool pf)
{
    return !pf && (RT_TRACE_QUAD_WAIT >= 2 || (RT_TRACE_QUAD_WAIT == 1 && (render <= 2 || render == kRenderDebugBoxCount)));
}

// one sample of one pixel -> float colour 0..255 per channel + alpha (TraceRays body, Tracer.cu:482-593).
// Every lane of the wave calls this (inactive lanes trace nothing) because trace_ray votes with ballots; the shadow
// ray of kTextureLitShadows is a second wave-level traversal over the lanes that hit something.
template <int RENDER, bool PF, bool QW>
__device__ __forceinline__ void shade_sample(const TraceParams& p, const rt_camera& cam, uint32_t x, uint32_t y,
                                             float ox, float oy, Trav& t, bool active, uint32_t& box_acc,
                                             uint32_t& tri_acc, uint32_t* steps, float& R, float& G, float& B, float& A)
{
    const float max_depth = cam.max_depth;
    Ray r;
    camera_ray(cam, p.w, p.h, x, y, ox, oy, r);
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    Hit h = {0u, 0u, 0.f, 0.f};
    const bool hit = trace_ray<PF, false, QW>(p, r, h, t, active, steps);
    const uint32_t box_tests = t.box_tests, tri_tests = t.tri_tests;
    box_acc += box_tests;
    tri_acc += tri_tests;
    const float depth = hit ? r.tmax : 0.0f;
    R = G = B = 0;
    A = 255.0f;

    if (RENDER == RT_RENDER_DEPTH) {
        R = G = B = fminf(1.0f, depth / max_depth) * 255;
        return;
    }
    if (RENDER == RT_RENDER_BOXTESTS) {
        G = B = fminf(box_tests / 180.0f, 1.0f) * 255;
        return;
    }
    if (RENDER == kRenderDebugBoxCount) {  // tuning aid: R carries the raw count (bit pattern), see trace_kernel
        R = __uint_as_float(box_tests);
        return;
    }
    if (RENDER == RT_RENDER_TRIANGLE_TESTS) {
        const float g = fminf(tri_tests / 32.0f, 1.0f);
        R = g * 100; G = g * 255; B = g * 100;
        return;
    }
    // ---- modes that look at the surface.  The reference fetches attributes / material before testing `hit`
    // (Tracer.cu:506-509: primitive 0 on a miss); only kLODs depends on that (magenta unless textured AND hit).
    const bool lit = active && hit;
    const bool fetch = active && (hit || RENDER == RT_RENDER_LODS);
    rt_material mat = {};
    Surface s = {};
    int material_id = 0;
    if (fetch) {
        // RotateAttributes (Tracer.cu:57-82)
        const rt_triangle_pair* pair = p.leaves + (h.tri_id >> 1);
        const bool second = h.tri_id & 1;
        const uint32_t rot = second ? pair->rotations[1] : pair->rotations[0];
        const rt_attributes* at = p.attributes + h.primitive_id;
        const int i0 = rot == 1 ? 2 : (rot == 2 ? 1 : 0);
        const int i1 = rot == 1 ? 0 : (rot == 2 ? 2 : 1);
        const int i2 = rot == 1 ? 1 : (rot == 2 ? 0 : 2);
        material_id = at->material_id;
        // indices from scene data are range-checked (the reference is not: FileIO.cpp:191 gives faces before the first
        // usemtl material_id -1): an id outside the table shades as material 0, a texture index outside the texture
        // table reads as -1 (untextured)
        mat = p.materials[(uint32_t)material_id < p.num_materials ? (uint32_t)material_id : 0u];
        if ((uint32_t)mat.texture >= p.num_textures) mat.texture = -1;
        if ((uint32_t)mat.bump >= p.num_textures) mat.bump = -1;
        if ((uint32_t)mat.disp >= p.num_textures) mat.disp = -1;
        const rt_float3 n0 = at->normal[i0], n1 = at->normal[i1], n2 = at->normal[i2];
        s.n[0] = v3(n0.x, n0.y, n0.z); s.n[1] = v3(n1.x, n1.y, n1.z); s.n[2] = v3(n2.x, n2.y, n2.z);
        if (render_uses_surface(RENDER)) {
            s.uv[0][0] = at->uv[i0][0]; s.uv[0][1] = at->uv[i0][1];
            s.uv[1][0] = at->uv[i1][0]; s.uv[1][1] = at->uv[i1][1];
            s.uv[2][0] = at->uv[i2][0]; s.uv[2][1] = at->uv[i2][1];
            const rt_float3 a = second ? pair->v2 : pair->v0, b = pair->v1, c = second ? pair->v3 : pair->v2;
            s.tri[0] = v3(a.x, a.y, a.z); s.tri[1] = v3(b.x, b.y, b.z); s.tri[2] = v3(c.x, c.y, c.z);
        }
    }
    const float spread = 2.0f / p.w;
    if (RENDER == RT_RENDER_LODS) {                       // Tracer.cu:543-556
        if (!active) return;
        if (mat.texture != -1 && hit) {
            const float lod = compute_lod(r, h, spread, s, p.textures[mat.texture]);
            R = G = B = A = (float)(((uint32_t)((int)lod * 20)) & 255u);
        } else {
            R = 255; G = 0; B = 255;
        }
        return;
    }
    if (RENDER == RT_RENDER_MATERIAL_ID) {
        if (lit) hsv_to_rgb255((float)material_id / p.num_materials, 1.0f, 1.0f, R, G, B);
        return;
    }
    if (RENDER == RT_RENDER_TEXTURE) {                    // Tracer.cu:557-578
        if (!lit) return;
        if (mat.texture != -1) {
            const rt_texture& tex = p.textures[mat.texture];
            const float lod = compute_lod(r, h, spread, s, tex);
            const U8x4 c = trilinear_sample(tex, interp_uv(s, h.bu, h.bv), lod);
            R = (float)c.c[0]; G = (float)c.c[1]; B = (float)c.c[2]; A = (float)c.c[3];
        } else {
            R = mat.diffuse.x * 255; G = mat.diffuse.y * 255; B = mat.diffuse.z * 255;
        }
        return;
    }
    // ---- AmbientShader (Tracer.cu:376-469): kDiffuse (no textures), kTextureLit (textures + bump), kTextureLitShadows
    constexpr bool use_textures = RENDER == RT_RENDER_TEXTURE_LIT || RENDER == RT_RENDER_TEXTURE_LIT_SHADOWS;
    constexpr bool use_bump = use_textures;
    constexpr bool use_shadows = RENDER == RT_RENDER_TEXTURE_LIT_SHADOWS;
    const float hx = r.ox + r.dx * r.tmax, hy = r.oy + r.dy * r.tmax, hz = r.oz + r.dz * r.tmax;
    float lx = p.light[0] - hx, ly = p.light[1] - hy, lz = p.light[2] - hz;
    const float to_light = sqrtf(lx * lx + ly * ly + lz * lz);      // length(light_pos - hit_pos) (:455)
    const float linv = 1.0f / to_light;
    lx *= linv; ly *= linv; lz *= linv;
    bool shadowed = false;
    if (use_shadows) {                                    // (:447-462) a second traversal, wave-wide
        Ray sr;
        sr.ox = hx; sr.oy = hy; sr.oz = hz;
        sr.dx = lx; sr.dy = ly; sr.dz = lz;
        sr.ix = 1.0f / lx; sr.iy = 1.0f / ly; sr.iz = 1.0f / lz;
        sr.tmin = 0.001f;
        sr.tmax = to_light;
        Hit sh = {0u, 0u, 0.f, 0.f};
        shadowed = trace_ray<PF, false, QW>(p, sr, sh, t, lit, steps);   // its test counts are not reported (shadow_stats, :451)
    }
    if (!lit) return;
    const float w0 = 1 - h.bu - h.bv;
    V3 n = vadd(vadd(vscale(s.n[0], w0), vscale(s.n[1], h.bu)), vscale(s.n[2], h.bv));   // InterpolateNormals (:50-56)
    if (use_bump && mat.disp != -1) {                     // displacement map read as a normal map (:388-403)
        const rt_texture& disp = p.textures[mat.disp];
        const float lod = compute_lod(r, h, spread, s, disp);
        V3 tbn[3];
        tangent_matrix(s, tbn);
        const U8x4 smp = trilinear_sample(disp, interp_uv(s, h.bu, h.bv), lod);
        n = v3((float)smp.c[0] / 255.0f, (float)smp.c[1] / 255.0f, (float)smp.c[2] / 255.0f);
        n = vnormalize(v3(n.x * 2.0f - 1.0f, n.y * 2.0f - 1.0f, n.z * 2.0f - 1.0f));
        n = vnormalize(v3(vdot(tbn[0], n), vdot(tbn[1], n), vdot(tbn[2], n)));
    } else if (use_bump && mat.bump != -1) {              // (:405-415)
        const rt_texture& bump = p.textures[mat.bump];
        const float lod = compute_lod(r, h, spread, s, bump);
        V3 tbn[3];
        tangent_matrix(s, tbn);
        n = bump2normal(bump, tbn, interp_uv(s, h.bu, h.bv), lod);
    }
    const float nx = n.x, ny = n.y, nz = n.z;
    const float lcx = 1.0f, lcy = 0.9f, lcz = 0.8f;
    float dterm = 1.0f * fmaxf(nx * lx + ny * ly + nz * lz, 0.0f);
    // reflect(-l, n) = -l - 2.0f * n * dot(n, -l)   (helper_math.h:1435-1438)
    const float nlx = -lx, nly = -ly, nlz = -lz;
    const float ndl = nx * nlx + ny * nly + nz * nlz;
    const float rx = nlx - (nx * 2.0f) * ndl, ry = nly - (ny * 2.0f) * ndl, rz = nlz - (nz * 2.0f) * ndl;
    // pow(max(dot(-dir, refl), 0.0), Ns): double max, double pow, narrowed by operator*(float, float3)
    const double sb = fmax((double)((-r.dx) * rx + (-r.dy) * ry + (-r.dz) * rz), 0.0);
    float sp = (float)(1.0f * rt_pow_d(sb, (double)mat.specular_exp));   // pow: rt_math.h
    float odx = mat.diffuse.x, ody = mat.diffuse.y, odz = mat.diffuse.z;
    if (use_textures && mat.texture != -1) {              // (:432-445): BilinearSample(tex, uv, (int)lod)
        const rt_texture& tex = p.textures[mat.texture];
        const float lod = compute_lod(r, h, spread, s, tex);
        const U8x4 smp = bilinear_sample(tex, interp_uv(s, h.bu, h.bv), (int)lod);
        odx = (float)smp.c[0] / 255; ody = (float)smp.c[1] / 255; odz = (float)smp.c[2] / 255;
    }
    float dfx = lcx * dterm, dfy = lcy * dterm, dfz = lcz * dterm;
    float spx = lcx * sp, spy = lcy * sp, spz = lcz * sp;
    if (shadowed) { dfx = dfy = dfz = 0.0f; spx = spy = spz = 0.0f; }
    const float cr = (dfx * odx + (lcx * 0.2f) * mat.ambient.x) + spx * mat.specular.x;
    const float cg = (dfy * ody + (lcy * 0.2f) * mat.ambient.y) + spy * mat.specular.y;
    const float cb = (dfz * odz + (lcz * 0.2f) * mat.ambient.z) + spz * mat.specular.z;
    R = clampf(cr, 0.0f, 1.0f) * 255;
    G = clampf(cg, 0.0f, 1.0f) * 255;
    B = clampf(cb, 0.0f, 1.0f) * 255;
}

// PF (pair prefetch): for trees that do not fit the caches.  On the 10M-triangle scene (1.28 GB of nodes + leaves, 5 x the
// Infinity Cache; L2 hit 94 %) a wave waits for L2 misses, not for the address path: issuing the NEXT pair's loads right
// after advance() -- one more pair in flight per lane across the wave's vote -- at 96 VGPRs / 5 waves per SIMD is +8 % serial,
// +16 % with frames in flight on camera A, +6 / +14 % on camera B; on the cache-resident 1M tree the same kernel is 25 % SLOWER
// (five waves instead of eight feed the address path), at 4.5M -7 % / +6 %; at 64 - 80 VGPRs the sixteen extra registers
// spill and it is 2 - 5 x slower everywhere (profiles/r04_trace_10m_experiments.txt).  launch_trace picks it by scene size.
template <int RENDER, bool PF, bool QW = false>
// kDepth / kBoxtests / kTriangleTests end in a one-line colour conversion: they fit 64 VGPRs (8 waves per SIMD); the
// shading of the other render types would spill there, they keep 72 VGPRs (7 waves) (RT_TRACE_LEAN_EXTRA: rt_traverse.hpp)
__global__ __launch_bounds__(kTraceWaves * 64, PF ? RT_TRACE_PF_WAVES : ((RENDER <= 2 || RENDER == kRenderDebugBoxCount) ? RT_TRACE_MIN_WAVES + RT_TRACE_LEAN_EXTRA : RT_TRACE_MIN_WAVES))
void trace_kernel(TraceParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t stack_lds[kTraceWaves][kStackLds][64];   // (aligned: quad_hold reads a quad's four columns of a level as 16 bytes)
    __shared__ unsigned long long csum[4];   // the workgroup's test counters (see the end of the kernel)
    __shared__ uint32_t carrive;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p.counters) {                         // (kernel argument: the same for every thread)
        if (threadIdx.x < 4) csum[threadIdx.x] = 0ull;
        if (threadIdx.x == 4) carrive = 0u;
        __syncthreads();
    }

    // XCD-aware remap (xcd_chunk_block, rt_traverse.hpp): an XCD takes runs of 8 consecutive workgroups = 8 x 4 tiles
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint32_t tile = vb * kTraceWaves + wave;
    const uint32_t tx = tile % p.tiles_x, ty = tile / p.tiles_x;

    // lane -> pixel inside the 8x8 tile, Morton order
    const uint32_t lx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4);
    const uint32_t ly = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4);
    const uint32_t x = tx * 8 + lx;
    uint32_t y = p.y0 + ty * 8 + ly, out_y = y;      // row band: rendered in place
    if (p.strip_tiles) {                            // interleaved strips: rendered compactly
        const uint32_t strip = p.strip_first + (ty / p.strip_tiles) * p.strip_stride;
        y = (strip * p.strip_tiles + ty % p.strip_tiles) * 8 + ly;
        out_y = ty * 8 + ly;
    }
    const bool active = tile < p.num_tiles && x < p.w && y < p.y1;

    const rt_camera cam = *p.camera;
    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t box_acc = 0, tri_acc = 0;
    uint32_t steps[2] = {0u, 0u};
    float R, G, B, A;
    if (p.spp <= 1) {
        shade_sample<RENDER, PF, QW>(p, cam, x, y, 0.5f, 0.5f, t, active, box_acc, tri_acc, steps, R, G, B, A);
    } else {
        float ar = 0, ag = 0, ab = 0, aa = 0;
        const uint32_t side = p.spp == 4 ? 2u : 4u;   // stratified side x side sub-pixel grid (2 x 2 or 4 x 4)
        for (uint32_t s = 0; s < p.spp; s++) {
            const float ox = ((float)(s % side) + 0.5f) / (float)side, oy = ((float)((s / side) % side) + 0.5f) / (float)side;
            shade_sample<RENDER, PF, QW>(p, cam, x, y, ox, oy, t, active, box_acc, tri_acc, steps, R, G, B, A);
            ar += R; ag += G; ab += B; aa += A;
        }
        R = ar / (float)p.spp; G = ag / (float)p.spp; B = ab / (float)p.spp; A = aa / (float)p.spp;
    }
    if (active) {
        uint32_t px = sat_u8(R) | (sat_u8(G) << 8) | (sat_u8(B) << 16) | (sat_u8(A) << 24);
        if (RENDER == kRenderDebugBoxCount) px = __float_as_uint(R);
        reinterpret_cast<uint32_t*>(p.rgba8)[(size_t)out_y * p.w + x] = px;
    }
    if (p.counters) {
        // The workgroup's waves add into LDS, and the LAST wave to finish (an LDS arrival count: no barrier, nobody waits)
        // publishes the four sums (round 2 issued four device atomics per wave on the caller's counters: 130 k queued
        // same-address atomics = 1.4 ms per 1080p frame).
        const uint32_t bsum = wave_sum_u32(box_acc), tsum = wave_sum_u32(tri_acc);  // <= 64 * 2^26: no overflow per wave
        uint32_t last = 0;
        if (lane == 0) {
            atomicAdd(&csum[0], (unsigned long long)bsum);
            atomicAdd(&csum[1], (unsigned long long)tsum);
            atomicAdd(&csum[2], (unsigned long long)steps[0]);  // wave-level box-phase steps (profiling)
            atomicAdd(&csum[3], (unsigned long long)steps[1]);  // wave-level leaf-phase steps
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            last = atomicAdd(&carrive, 1u) == (uint32_t)kTraceWaves - 1u ? 1u : 0u;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        if (__builtin_amdgcn_readfirstlane((int)last)) {   // the workgroup's last wave: publish (see g_ctr above)
            CtrSlot& S = g_ctr[p.ctr_slot];
            const uint32_t sub = blockIdx.x % kCtrSub;
            if (lane < 4) {
                const unsigned long long v = *(volatile unsigned long long*)&csum[lane];
                // a RETURNING atomic: its value coming back means the add has been performed at the memory side, so the
                // ticket below cannot overtake it
                const unsigned long long old = v ? __hip_atomic_fetch_add(&S.part[sub][lane], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                asm volatile("" ::"v"((uint32_t)old), "v"((uint32_t)(old >> 32)) : "memory");
            }
            uint32_t fin = 0;
            if (lane == 0) {
                const uint32_t members = (gridDim.x - sub + kCtrSub - 1) / kCtrSub;
                if (__hip_atomic_fetch_add(&S.part[sub][4], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == members) {
                    const uint32_t rows = min(gridDim.x, kCtrSub);
                    fin = __hip_atomic_fetch_add(&S.top, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull == rows ? 1u : 0u;
                }
            }
            if (__builtin_amdgcn_readfirstlane((int)fin)) {
                // every workgroup of the launch has added its sums: fold the rows (lane = row * 4 + counter), hand them to the
                // caller, leave the slot zeroed for its next user
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                unsigned long long* cell = &S.part[lane >> 2][lane & 3];
                unsigned long long v = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(cell, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane < (int)kCtrSub) __hip_atomic_store(&S.part[lane][4], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane == 0) __hip_atomic_store(&S.top, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int off = 4; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
                if (lane < 4 && v) atomicAdd(&p.counters[lane], v);
            }
        }
    }
}

hipError_t launch_trace(const TraceLaunch& t, hipStream_t st)
{
    if (t.y1 <= t.y0 || t.w == 0) return hipSuccess;
    TraceParams p;
    p.nodes = t.as.nodes;
    p.leaves = t.as.triangles;
    p.attributes = t.scene.attributes;
    p.materials = t.scene.materials;
    p.textures = t.scene.textures;
    p.camera = t.scene.camera;
    p.light[0] = t.scene.light[0]; p.light[1] = t.scene.light[1]; p.light[2] = t.scene.light[2];
    p.root = t.as.root;
    p.count = t.as.count;
    p.num_materials = t.scene.num_materials;
    p.num_textures = t.scene.textures ? t.scene.num_textures : 0;
    p.rgba8 = t.rgba8;
    p.w = t.w; p.h = t.h; p.y0 = t.y0; p.y1 = t.y1; p.spp = t.spp;
    p.counters = reinterpret_cast<unsigned long long*>(t.counters);
    static std::atomic<uint32_t> ctr_seq{0};
    p.ctr_slot = t.counters ? ctr_seq.fetch_add(1u, std::memory_order_relaxed) % kCtrSlots : 0u;
    p.tiles_x = (t.w + 7) / 8;
    uint32_t tiles_y = (t.y1 - t.y0 + 7) / 8;
    p.strip_tiles = t.strip_rows / 8;
    p.strip_first = t.strip_first;
    p.strip_stride = t.strip_stride;
    if (p.strip_tiles) {   // this launch's strips: first, first + stride, ... < ceil(h / strip_rows)
        const uint32_t nstrips = (t.h + t.strip_rows - 1) / t.strip_rows;
        if (t.strip_first >= nstrips) return hipSuccess;
        tiles_y = ((nstrips - t.strip_first + t.strip_stride - 1) / t.strip_stride) * p.strip_tiles;
    }
    p.num_tiles = p.tiles_x * tiles_y;
    p.park_num = kParkNum;
    p.park_den = kParkDen;
#ifdef RT_TRACE_TUNING
    static const int* park = [] {
        static int v[2] = {kParkNum, kParkDen};
        if (const char* e = getenv("RT_TRACE_PARK")) {
            int a = 0, b = 0;
            if (sscanf(e, "%d,%d", &a, &b) == 2 && a > 0 && b > 0) { v[0] = a; v[1] = b; }
        }
        return v;
    }();
    p.park_num = park[0];
    p.park_den = park[1];
#endif
    const uint32_t blocks = (p.num_tiles + kTraceWaves - 1) / kTraceWaves;
    const dim3 grid(blocks), block(kTraceWaves * 64);
    // scene size (DeviceScene::num_attributes, filled by the caller as main.cu:166 does; 0 = unknown): a tree of kPrefetchMinPrims
    // primitives is 1 GB of nodes + leaves, four times the Infinity Cache
    const bool pf = t.scene.num_attributes >= kPrefetchMinPrims;
    // Hold at pop by tree: a tree entered through a root PAIR (the bottom-up builders: LBVH, pairs, hybrid) takes the
    // instantiation with the rule; one entered through a single root slot (the SAH builder's, whose traversals are a quarter
    // as long and leaf-heavy) keeps the plain loop -- with the rule it ties with frames in flight and loses 1.1 % one frame
    // at a time (profiles/quad_wait_bench.txt).  Both loops do the same tests: the choice is about time only.
    const bool qw = t.as.count >= 2;
#define RT_TRACE_CASE(R) case R: \
        if (pf) trace_kernel<R, true><<<grid, block, 0, st>>>(p); \
        else if (trace_quad_wait(R, false) && qw) trace_kernel<R, false, trace_quad_wait(R, false)><<<grid, block, 0, st>>>(p); \
        else trace_kernel<R, false><<<grid, block, 0, st>>>(p); \
        break;
    switch (t.render_type) {
    RT_TRACE_CASE(RT_RENDER_DEPTH)
    RT_TRACE_CASE(RT_RENDER_BOXTESTS)
    RT_TRACE_CASE(RT_RENDER_TRIANGLE_TESTS)
    RT_TRACE_CASE(RT_RENDER_MATERIAL_ID)
    RT_TRACE_CASE(RT_RENDER_DIFFUSE)
    RT_TRACE_CASE(RT_RENDER_LODS)
    RT_TRACE_CASE(RT_RENDER_TEXTURE)
    RT_TRACE_CASE(RT_RENDER_TEXTURE_LIT)
    RT_TRACE_CASE(RT_RENDER_TEXTURE_LIT_SHADOWS)
#ifdef RT_TRACE_TUNING
    case kRenderDebugBoxCount: trace_kernel<kRenderDebugBoxCount, false><<<grid, block, 0, st>>>(p); break;
#endif
    default: return hipErrorInvalidValue;
    }
#undef RT_TRACE_CASE
    return hipGetLastError();
}

}  // namespace rt
