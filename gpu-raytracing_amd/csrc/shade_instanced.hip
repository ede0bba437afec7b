// shade_instanced.hip -- deferred shading of INSTANCED hit records (rt_shade_frame_instanced; semantics: rt_abi.h, instanced
// deferred-shading block).
//
// rt_intersect_rays_instanced and its siblings give (t, primitive_id, u, v) in the BLAS's own object space plus an instance
// id.  shade.hip's shaders take their input by value in a Surface, so the instanced shader is "gather, transform, then the
// same shaders": the frame is, byte for byte, the one rt_shade_frame renders on the flattened scene.
//
// shade_instanced_kernel<RENDER, TILED>: one thread per pixel, a loop over the spp samples, shade_kernel's pixel -> sample
// mapping (restated here: shade.hip's code object does not change).  Per sample:
//   ray                 two 16-byte loads
//   hit record          one 16-byte load
//   instance id         4 bytes (+ 4 bytes of the shadow instance id in mode 8)
//   instance record     the last 16 bytes (blas, flags) always; the three matrix rows only in the lit instantiations, whose
//                       normals go through their transpose
//   geometry entry      two 16-byte loads (pointers; count and material base)
//   object_to_world     three 16-byte loads, only where corners are read (render_uses_surface)
//   attributes          material id; normals (lit), uv (surface); then the shaders of rt_shade.hpp, untouched
// RT_RENDER_DEPTH and RT_RENDER_MATERIAL_ID touch neither matrix.  Record and geometry loads are per lane: a tile sees few
// instances, so they are mostly wave-coherent and served by one or two cache lines; there is no wave-uniform fast path.
// All addresses are 64-bit.  Compiled with -ffp-contract=off: every operation below is rounded on its own.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_shade.hpp"

namespace rt {

static_assert(sizeof(rt_shade_geometry) == 32 && offsetof(rt_shade_geometry, triangles) == 0 &&
              offsetof(rt_shade_geometry, attributes) == 8 && offsetof(rt_shade_geometry, num_triangles) == 16 &&
              offsetof(rt_shade_geometry, material_base) == 20, "rt_shade_geometry: two 16-byte halves");
static_assert(sizeof(rt_instance) == 64 && sizeof(rt_instance_record) == 64 && offsetof(rt_instance_record, blas) == 48 &&
              offsetof(rt_instance_record, flags) == 52, "instance and record: three 16-byte matrix rows, then blas / flags");

struct ShadeInstancedParams {
    const rt_material* materials;
    const rt_texture* textures;
    const uint4* geometry;             // rt_shade_geometry = two uint4: (triangles, attributes), (count, base, pad, pad)
    const float4* instances;           // rt_instance = four float4: object_to_world rows, (blas, pad)
    const float4* records;             // rt_instance_record = four float4: world_to_object rows, (blas, flags, spare)
    const int32_t* instance_materials; // optional per-instance material override (>= 0)
    const float4* rays;
    const float4* hits;
    const uint32_t* instance_ids;
    const uint32_t* shadow_instance_ids;   // mode 8: < num_instances = occluded
    float light[3];
    uint32_t num_blas, num_instances, num_materials, num_textures;
    uint32_t renormalize;
    uint32_t* rgba8;
    uint32_t w, h, spp, tiles_x;
};

// rows ((m0*x + m1*y) + m2*z) + m3 of object_to_world: rt_prepare_instances's order
__device__ __forceinline__ V3 place_corner(const float4& r0, const float4& r1, const float4& r2, const rt_float3& c)
{
    return v3(((r0.x * c.x + r0.y * c.y) + r0.z * c.z) + r0.w, ((r1.x * c.x + r1.y * c.y) + r1.z * c.z) + r1.w,
              ((r2.x * c.x + r2.y * c.y) + r2.z * c.z) + r2.w);
}

// the transpose of world_to_object's 3x3 applied to a normal: n'_r = (W[0][r]*nx + W[1][r]*ny) + W[2][r]*nz, then
// vnormalize's order under RT_SHADE_RENORMALIZE where the squared length is positive and finite
__device__ __forceinline__ V3 place_normal(const float4& w0, const float4& w1, const float4& w2, const rt_float3& n,
                                           bool renormalize)
{
    V3 o = v3((w0.x * n.x + w1.x * n.y) + w2.x * n.z, (w0.y * n.x + w1.y * n.y) + w2.y * n.z,
              (w0.z * n.x + w1.z * n.y) + w2.z * n.z);
    if (renormalize) {
        const float l2 = (o.x * o.x + o.y * o.y) + o.z * o.z;
        if (l2 > 0.0f && l2 < __builtin_inff()) o = vscale(o, 1.0f / sqrtf(l2));
    }
    return o;
}

// one sample: shade.hip's shade_record with the triangle, its attributes and its material id found through the instance
template <int RENDER>
__device__ __forceinline__ void shade_record_instanced(const ShadeInstancedParams& p, uint64_t i, float& R, float& G, float& B,
                                                       float& A)
{
    const float4 ra = p.rays[2 * i], rb = p.rays[2 * i + 1], hr = p.hits[i];
    const uint32_t k = p.instance_ids[i];
    const uint32_t prim = __float_as_uint(hr.y);
    // hit: a live instance (k in range, record unflagged, blas in range), a table entry with both arrays, an id inside it.
    // Nothing is read through an index before that index has been checked.
    bool hit = k < p.num_instances;
    const rt_triangle* triangles = nullptr;
    const rt_attributes* attributes = nullptr;
    int material_base = 0;
    if (hit) {
        const float4 tail = p.records[4 * (uint64_t)k + 3];
        const uint32_t blas = __float_as_uint(tail.x), flags = __float_as_uint(tail.y);
        hit = flags == 0u && blas < p.num_blas;
        if (hit) {
            const uint4 g0 = p.geometry[2 * (uint64_t)blas], g1 = p.geometry[2 * (uint64_t)blas + 1];
            triangles = reinterpret_cast<const rt_triangle*>((uint64_t)g0.x | ((uint64_t)g0.y << 32));
            attributes = reinterpret_cast<const rt_attributes*>((uint64_t)g0.z | ((uint64_t)g0.w << 32));
            material_base = (int)g1.y;
            hit = triangles != nullptr && attributes != nullptr && prim < g1.x;
        }
    }
    R = G = B = 0;
    A = 255.0f;
    if (RENDER == RT_RENDER_DEPTH) {
        if (hit) R = G = B = fminf(1.0f, hr.x / rb.w) * 255;
        return;
    }
    if (!hit) {
        if (RENDER == RT_RENDER_LODS) { R = 255; G = 0; B = 255; }
        return;
    }
    Ray r;
    r.ox = ra.x; r.oy = ra.y; r.oz = ra.z; r.tmin = ra.w;
    r.dx = rb.x; r.dy = rb.y; r.dz = rb.z; r.tmax = hr.x;
    r.ix = r.iy = r.iz = 0.0f;   // (the shaders do not read them)
    Hit h;
    h.primitive_id = prim; h.tri_id = 0u; h.bu = hr.z; h.bv = hr.w;

    const rt_attributes* at = attributes + prim;
    int material_id = (int)((uint32_t)at->material_id + (uint32_t)material_base);
    if (p.instance_materials) {
        const int over = p.instance_materials[k];
        if (over >= 0) material_id = over;
    }
    rt_material mat;
    fetch_material(p, material_id, mat);
    Surface s = {};
    if (render_is_lit(RENDER)) {
        const float4 w0 = p.records[4 * (uint64_t)k], w1 = p.records[4 * (uint64_t)k + 1], w2 = p.records[4 * (uint64_t)k + 2];
        const bool renorm = p.renormalize != 0u;
        s.n[0] = place_normal(w0, w1, w2, at->normal[0], renorm);
        s.n[1] = place_normal(w0, w1, w2, at->normal[1], renorm);
        s.n[2] = place_normal(w0, w1, w2, at->normal[2], renorm);
    }
    if (render_uses_surface(RENDER)) {
        s.uv[0][0] = at->uv[0][0]; s.uv[0][1] = at->uv[0][1];
        s.uv[1][0] = at->uv[1][0]; s.uv[1][1] = at->uv[1][1];
        s.uv[2][0] = at->uv[2][0]; s.uv[2][1] = at->uv[2][1];
        const float4 m0 = p.instances[4 * (uint64_t)k], m1 = p.instances[4 * (uint64_t)k + 1], m2 = p.instances[4 * (uint64_t)k + 2];
        const rt_triangle* tri = triangles + prim;
        s.tri[0] = place_corner(m0, m1, m2, tri->v0);
        s.tri[1] = place_corner(m0, m1, m2, tri->v1);
        s.tri[2] = place_corner(m0, m1, m2, tri->v2);
    }
    const float spread = 2.0f / p.w;
    if (shade_unlit<RENDER>(p, r, h, spread, mat, s, material_id, true, true, true, R, G, B, A)) return;
    float hx, hy, hz, lx, ly, lz, to_light;
    light_vector(p, r, hx, hy, hz, lx, ly, lz, to_light);
    bool shadowed = false;
    if (RENDER == RT_RENDER_TEXTURE_LIT_SHADOWS) shadowed = p.shadow_instance_ids[i] < p.num_instances;
    shade_lit<RENDER>(p, r, h, spread, mat, s, lx, ly, lz, shadowed, R, G, B);
}

// Launch bounds: shade_kernel's floors (shade.hip, shade_min_waves): 8 waves per SIMD for the colour-only render types, 4 for
// RT_RENDER_DIFFUSE, 2 for the textured ones.  DESIGN section 28 has the resource table.
constexpr int shade_instanced_min_waves(int render)
{
    return render == RT_RENDER_DEPTH || render == RT_RENDER_MATERIAL_ID ? 8 : (render == RT_RENDER_DIFFUSE ? 4 : 2);
}

template <int RENDER, bool TILED>
__global__ __launch_bounds__(256, shade_instanced_min_waves(RENDER))
void shade_instanced_kernel(ShadeInstancedParams p)
{
    // shade_kernel's mapping: pixel position j = tile * 64 + lane (lane = Morton position in the 8 x 8 tile), or y * w + x
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t x, y;
    uint64_t base, stride;                                        // ray of sample s: base + s * stride
    if (TILED) {
        const uint32_t lane = (uint32_t)(j & 63u);
        const uint64_t tile = j >> 6;
        const uint32_t lx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4);
        const uint32_t ly = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4);
        x = (uint32_t)(tile % p.tiles_x) * 8 + lx;
        const uint64_t ty = tile / p.tiles_x;
        if (ty * 8 + ly >= p.h) return;
        y = (uint32_t)ty * 8 + ly;
        base = tile * p.spp * 64u + lane;
        stride = 64u;
    } else {
        if (j >= (uint64_t)p.w * p.h) return;
        x = (uint32_t)(j % p.w);
        y = (uint32_t)(j / p.w);
        base = j * p.spp;
        stride = 1u;
    }
    if (x >= p.w) return;
    float R, G, B, A;
    if (p.spp <= 1) {
        shade_record_instanced<RENDER>(p, base, R, G, B, A);
    } else {
        float ar = 0, ag = 0, ab = 0, aa = 0;
        for (uint32_t s = 0; s < p.spp; s++) {
            shade_record_instanced<RENDER>(p, base + s * stride, R, G, B, A);
            ar += R; ag += G; ab += B; aa += A;
        }
        R = ar / (float)p.spp; G = ag / (float)p.spp; B = ab / (float)p.spp; A = aa / (float)p.spp;
    }
    p.rgba8[(size_t)y * p.w + x] = sat_u8(R) | (sat_u8(G) << 8) | (sat_u8(B) << 16) | (sat_u8(A) << 24);
}

hipError_t launch_shade_frame_instanced(const ShadeInstancedLaunch& t, hipStream_t st)
{
    ShadeInstancedParams p;
    p.materials = t.scene.materials;
    p.textures = t.scene.textures;
    p.geometry = reinterpret_cast<const uint4*>(t.geometry);
    p.instances = reinterpret_cast<const float4*>(t.instances);
    p.records = reinterpret_cast<const float4*>(t.records);
    p.instance_materials = t.instance_materials;
    p.rays = reinterpret_cast<const float4*>(t.rays);
    p.hits = reinterpret_cast<const float4*>(t.hits);
    p.instance_ids = t.instance_ids;
    p.shadow_instance_ids = t.shadow_instance_ids;
    p.light[0] = t.scene.light[0]; p.light[1] = t.scene.light[1]; p.light[2] = t.scene.light[2];
    p.num_blas = t.num_blas;
    p.num_instances = t.num_instances;   // 0: the three arrays may be null, every record is a miss and none is read
    p.num_materials = t.scene.num_materials;
    p.num_textures = t.scene.textures ? t.scene.num_textures : 0;
    p.renormalize = (t.flags & RT_SHADE_RENORMALIZE) ? 1u : 0u;
    p.rgba8 = reinterpret_cast<uint32_t*>(t.rgba8);
    p.w = t.w; p.h = t.h; p.spp = t.spp;
    p.tiles_x = (t.w + 7) / 8;
    const uint64_t tiles_y = (t.h + 7) / 8;
    const uint64_t positions = t.tiled ? (uint64_t)p.tiles_x * tiles_y * 64u : (uint64_t)t.w * t.h;
    const uint64_t blocks = (positions + 255) / 256;
    if (blocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks), block(256);
#define RT_SHADE_CASE(R) case R: if (t.tiled) shade_instanced_kernel<R, true><<<grid, block, 0, st>>>(p); else shade_instanced_kernel<R, false><<<grid, block, 0, st>>>(p); break;
    switch (t.render_type) {
    RT_SHADE_CASE(RT_RENDER_DEPTH)
    RT_SHADE_CASE(RT_RENDER_MATERIAL_ID)
    RT_SHADE_CASE(RT_RENDER_LODS)
    RT_SHADE_CASE(RT_RENDER_DIFFUSE)
    RT_SHADE_CASE(RT_RENDER_TEXTURE)
    RT_SHADE_CASE(RT_RENDER_TEXTURE_LIT)
    RT_SHADE_CASE(RT_RENDER_TEXTURE_LIT_SHADOWS)
    default: return hipErrorInvalidValue;
    }
#undef RT_SHADE_CASE
    return hipGetLastError();
}

}  // namespace rt
