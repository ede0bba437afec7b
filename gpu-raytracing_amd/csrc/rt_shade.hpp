// rt_shade.hpp -- the device shading code: colour conversion, texture sampling, ComputeLOD, TangentMatrix, Bump2Normal
// and the shaders of the surface render types once the hit is known (Tracer.cu:15-185, 202-254, 376-469, 506-593).
//
// Shared by trace_kernel.hip (rt_trace: traversal and shading in one kernel) and shade.hip (rt_shade_frame: shading from
// stored hit records), as rt_traverse.hpp is shared by the tracer and the ray queries.
//   * The helpers (hsv_to_rgb255 ... bump2normal, Surface, sat_u8) are used by both kernels; moving them here left every
//     trace_kernel<RENDER, PF> instantiation's gfx950 code unchanged.
//   * The part of a sample after the hit is split where rt_trace runs its shadow traversal, so that the shadow decision is
//     an INPUT:
//       shade_unlit<RENDER>   kLODs, kMaterialId, kTexture (returns true: the sample is done)
//       light_vector          hit point, unit vector to the light and its distance = the shadow ray
//       shade_lit<RENDER>     AmbientShader for kDiffuse, kTextureLit, kTextureLitShadows
//     shade.hip uses these three.  trace_kernel.hip's shade_sample keeps its own text of the same statements: called
//     through these functions its modes 3 and 5-8 compiled to other code (instruction order, spill counts), and the
//     headline benchmark rests on that kernel.  The two texts are held together by tests/test_gpu_shade_frame.py, which
//     compares the frames of the two kernels byte for byte.  Change one, change the other.
// `P` is the kernel's parameter block; the shaders read p.materials, p.textures, p.light, p.num_materials and
// p.num_textures of it.  Everything is __forceinline__.  Compiled with -ffp-contract=off, every operation rounded on its own.
#pragma once

#include "rt_device.hpp"
#include "rt_math.h"
#include "rt_traverse.hpp"   // Ray, Hit

namespace rt {

__device__ __forceinline__ float clampf(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }

// Tracer.cu:15-41 (float rgb 0..255 before the uchar truncation)
__device__ __forceinline__ void hsv_to_rgb255(float h, float s, float v, float& R, float& G, float& B)
{
    h = clampf(h, 0.f, 1.f) * 360.0f;
    s = clampf(s, 0.f, 1.f);
    v = clampf(v, 0.f, 1.f);
    const float c = s * v;
    const float x = c * (1 - fabsf(((int)h % 120) / 60.0f - 1));
    const float m = v - c;
    float r, g, b;
    if (h >= 0 && h < 60) { r = c; g = x; b = 0; }
    else if (h >= 60 && h < 120) { r = x; g = c; b = 0; }
    else if (h >= 120 && h < 180) { r = 0; g = c; b = x; }
    else if (h >= 180 && h < 240) { r = 0; g = x; b = c; }
    else if (h >= 240 && h < 300) { r = x; g = 0; b = c; }
    else { r = c; g = 0; b = x; }
    R = (r + m) * 255; G = (g + m) * 255; B = (b + m) * 255;
}

// ---------------------------------------------------------------------------------------------
// float -> unsigned char as CUDA converts it (cvt.rzi.u8.f32: NaN -> 0, saturating); bilinear weights at a texture
// border leave [0, 255]
__device__ __forceinline__ uint32_t sat_u8(float v) { return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (uint32_t)v); }
struct F2 { float x, y; };
struct U8x4 { uint32_t c[4]; };
__device__ __forceinline__ float fracf1(float v) { return v - floorf(v); }   // helper_math.h:1367

// Sample(Texture&, int2, lod) (Tracer.cu:103-108)
__device__ __forceinline__ void tex_fetch(const rt_texture& t, int x, int y, int lod, float out[4])
{
    const int sx = t.size_x[lod], sy = t.size_y[lod];
    x = max(0, min(x, sx - 1));
    y = max(0, min(y, sy - 1));
    const uint32_t w = t.mips[lod][(size_t)y * sx + x];
    out[0] = (float)(w & 255u); out[1] = (float)((w >> 8) & 255u); out[2] = (float)((w >> 16) & 255u); out[3] = (float)(w >> 24);
}
// BilinearSample (Tracer.cu:122-140)
__device__ __forceinline__ U8x4 bilinear_sample(const rt_texture& t, F2 uv, int lod)
{
    float cx = fracf1(uv.x) * (float)t.size_x[lod] - 0.5f;
    float cy = fracf1(uv.y) * (float)t.size_y[lod] - 0.5f;
    cy = (float)t.size_y[lod] - cy;
    const int ix = (int)cx, iy = (int)cy;
    const float dx = cx - (float)ix, dy = cy - (float)iy;
    const float w0 = (1.0f - dx) * dy, w1 = dx * dy, w2 = (1.0f - dx) * (1.0f - dy), w3 = dx * (1.0f - dy);
    float s0[4], s1[4], s2[4], s3[4];
    tex_fetch(t, ix, iy, lod, s0);
    tex_fetch(t, ix + 1, iy, lod, s1);
    tex_fetch(t, ix, iy - 1, lod, s2);
    tex_fetch(t, ix + 1, iy - 1, lod, s3);
    U8x4 o;
#pragma unroll
    for (int c = 0; c < 4; c++) o.c[c] = sat_u8(((s0[c] * w0 + s1[c] * w1) + s2[c] * w2) + s3[c] * w3);
    return o;
}
// TrilinearSample (Tracer.cu:142-155)
__device__ __forceinline__ U8x4 trilinear_sample(const rt_texture& t, F2 uv, float lod)
{
    uint32_t min_lod = (uint32_t)floorf(lod), max_lod = min_lod + 1;
    min_lod = min(min_lod, t.max_lod);
    max_lod = min(max_lod, t.max_lod);
    const U8x4 a = bilinear_sample(t, uv, (int)min_lod), b = bilinear_sample(t, uv, (int)max_lod);
    const float frac = fracf1(lod);
    U8x4 o;
#pragma unroll
    for (int c = 0; c < 4; c++) o.c[c] = sat_u8((float)a.c[c] * (1.0f - frac) + (float)b.c[c] * frac);
    return o;
}
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 vscale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float vdot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 vcross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 vnormalize(V3 v) { return vscale(v, 1.0f / sqrtf(vdot(v, v))); }

struct Surface {   // what the textured shaders need about the hit
    V3 tri[3];
    float uv[3][2];
    V3 n[3];
};
__device__ __forceinline__ F2 interp_uv(const Surface& s, float bu, float bv)   // InterpolateUVs (Tracer.cu:43-48)
{
    const float w0 = 1 - bu - bv;
    return {(s.uv[0][0] * w0 + s.uv[1][0] * bu) + s.uv[2][0] * bv, (s.uv[0][1] * w0 + s.uv[1][1] * bu) + s.uv[2][1] * bv};
}
// ComputeLOD (Tracer.cu:237-254) with RayTriangleGradients (:202-235) inlined
__device__ __forceinline__ float compute_lod(const Ray& r, const Hit& h, float spread, const Surface& s, const rt_texture& tex)
{
    const V3 o = v3(r.ox, r.oy, r.oz), d = v3(r.dx, r.dy, r.dz);
    const V3 edge1 = vsub(s.tri[1], s.tri[0]), edge2 = vsub(s.tri[2], s.tri[0]);
    const V3 sv = vsub(o, s.tri[0]);
    const V3 q = vcross(sv, edge1);
    const V3 x = vscale(vscale(vnormalize(vcross(d, v3(0, 1, 0))), r.tmax), spread);
    const V3 y = vscale(vscale(vnormalize(vcross(d, x)), r.tmax), spread);
    const V3 hit_point = vadd(o, vscale(d, r.tmax));
    const V3 dirx = vnormalize(vsub(vadd(hit_point, x), o)), diry = vnormalize(vsub(vadd(hit_point, y), o));
    const V3 h0 = vcross(dirx, edge2);
    const float f0 = 1.0f / vdot(edge1, h0);
    const float bu0 = f0 * vdot(sv, h0), bv0 = f0 * vdot(dirx, q);
    const V3 h1 = vcross(diry, edge2);
    const float f1 = 1.0f / vdot(edge1, h1);
    const float bu1 = f1 * vdot(sv, h1), bv1 = f1 * vdot(diry, q);
    const F2 uvs = interp_uv(s, h.bu, h.bv), ux = interp_uv(s, bu0, bv0), uy = interp_uv(s, bu1, bv1);
    const float sx = (float)tex.size_x[0], sy = (float)tex.size_y[0];
    const float dxx = fabsf(ux.x - uvs.x) * sx, dxy = fabsf(ux.y - uvs.y) * sy;
    const float dyx = fabsf(uy.x - uvs.x) * sx, dyy = fabsf(uy.y - uvs.y) * sy;
    const float max_change = fmaxf(sqrtf(dxx * dxx + dxy * dxy), sqrtf(dyx * dyx + dyy * dyy));
    return fmaxf(0.0f, fminf(rt_log2f(max_change), (float)tex.max_lod));   // log2f: rt_math.h (bit-identical to the oracle)
}
// TangentMatrix (Tracer.cu:84-101)
__device__ __forceinline__ void tangent_matrix(const Surface& s, V3 rows[3])
{
    const V3 e1 = vsub(s.tri[1], s.tri[0]), e2 = vsub(s.tri[2], s.tri[0]);
    const float d1x = s.uv[1][0] - s.uv[0][0], d1y = s.uv[1][1] - s.uv[0][1];
    const float d2x = s.uv[2][0] - s.uv[0][0], d2y = s.uv[2][1] - s.uv[0][1];
    const float f = 1.0f / (d1x * d2y - d1y * d2x);
    const V3 normal = vnormalize(vcross(e1, e2));
    const V3 tangent = vnormalize(vscale(vsub(vscale(e1, d2y), vscale(e2, d1y)), f));
    const V3 bitangent = vnormalize(vscale(vsub(vscale(e2, d1x), vscale(e1, d2x)), f));
    rows[0] = v3(tangent.x, bitangent.x, normal.x);
    rows[1] = v3(tangent.y, bitangent.y, normal.y);
    rows[2] = v3(tangent.z, bitangent.z, normal.z);
}
// Bump2Normal (Tracer.cu:157-185)
__device__ __forceinline__ V3 bump2normal(const rt_texture& tex, const V3 tbn[3], F2 uv, float lod)
{
    const float texel_step = rt_exp2f(lod);   // powf(2.0f, lod): rt_math.h
    const float stx = texel_step / (float)tex.size_x[0], sty = texel_step / (float)tex.size_y[0];
    const U8x4 a = trilinear_sample(tex, F2{uv.x - stx * 0.5f, uv.y - sty * 0.5f}, lod);
    const U8x4 b = trilinear_sample(tex, F2{uv.x + stx * 0.5f, uv.y + 0.0f}, lod);
    const U8x4 c = trilinear_sample(tex, F2{uv.x + 0.0f, uv.y + sty * 0.5f}, lod);
    const float gx = (float)b.c[0] - (float)a.c[0], gy = (float)c.c[0] - (float)a.c[0];
    const float d = 4.0f;
    V3 n = vnormalize(vcross(v3(1, 0, d * gx / (texel_step * 256.0f)), v3(0, 1, d * gy / (texel_step * 256.0f))));
    n = v3(vdot(tbn[0], n), vdot(tbn[1], n), vdot(tbn[2], n));
    return vnormalize(n);
}

constexpr bool render_is_lit(int r) { return r == RT_RENDER_DIFFUSE || r == RT_RENDER_TEXTURE_LIT || r == RT_RENDER_TEXTURE_LIT_SHADOWS; }
constexpr bool render_uses_surface(int r) { return r == RT_RENDER_LODS || r == RT_RENDER_TEXTURE || r == RT_RENDER_TEXTURE_LIT || r == RT_RENDER_TEXTURE_LIT_SHADOWS; }

// Material of a hit (Tracer.cu:506-509).  Indices from scene data are range-checked (the reference is not: FileIO.cpp:191
// gives faces before the first usemtl material_id -1): an id outside the table shades as material 0, a texture index outside
// the texture table reads as -1 (untextured)
template <class P>
__device__ __forceinline__ void fetch_material(const P& p, int material_id, rt_material& mat)
{
    mat = p.materials[(uint32_t)material_id < p.num_materials ? (uint32_t)material_id : 0u];
    if ((uint32_t)mat.texture >= p.num_textures) mat.texture = -1;
    if ((uint32_t)mat.bump >= p.num_textures) mat.bump = -1;
    if ((uint32_t)mat.disp >= p.num_textures) mat.disp = -1;
}

// The render types that need no light: kLODs (Tracer.cu:543-556), kMaterialId, kTexture (:557-578).  r.tmax = the hit
// distance, (h.bu, h.bv) the weights of corners 1 and 2 of s.tri; `fetched` = mat / s hold the hit's data (kLODs: the caller
// may fetch primitive 0 on a miss, as the reference does -- the colour does not depend on it).  Returns true when RENDER is
// one of the three: R, G, B, A are final (they come in as the miss colour 0, 0, 0, 255).  lit = active && hit.
template <int RENDER, class P>
__device__ __forceinline__ bool shade_unlit(const P& p, const Ray& r, const Hit& h, float spread, const rt_material& mat,
                                            const Surface& s, int material_id, bool active, bool hit, bool lit, float& R,
                                            float& G, float& B, float& A)
{
    if (RENDER == RT_RENDER_LODS) {                       // Tracer.cu:543-556
        if (!active) return true;
        if (mat.texture != -1 && hit) {
            const float lod = compute_lod(r, h, spread, s, p.textures[mat.texture]);
            R = G = B = A = (float)(((uint32_t)((int)lod * 20)) & 255u);
        } else {
            R = 255; G = 0; B = 255;
        }
        return true;
    }
    if (RENDER == RT_RENDER_MATERIAL_ID) {
        if (lit) hsv_to_rgb255((float)material_id / p.num_materials, 1.0f, 1.0f, R, G, B);
        return true;
    }
    if (RENDER == RT_RENDER_TEXTURE) {                    // Tracer.cu:557-578
        if (!lit) return true;
        if (mat.texture != -1) {
            const rt_texture& tex = p.textures[mat.texture];
            const float lod = compute_lod(r, h, spread, s, tex);
            const U8x4 c = trilinear_sample(tex, interp_uv(s, h.bu, h.bv), lod);
            R = (float)c.c[0]; G = (float)c.c[1]; B = (float)c.c[2]; A = (float)c.c[3];
        } else {
            R = mat.diffuse.x * 255; G = mat.diffuse.y * 255; B = mat.diffuse.z * 255;
        }
        return true;
    }
    return false;
}

// Hit point, unit vector to the light and the light's distance (Tracer.cu:447-455): origin, direction and tmax of the
// shadow ray.  Expression order: ((lx*lx + ly*ly) + lz*lz), 1 / sqrtf, then three products -- rt_generate_shadow_rays
// restates it.
template <class P>
__device__ __forceinline__ void light_vector(const P& p, const Ray& r, float& hx, float& hy, float& hz, float& lx, float& ly,
                                             float& lz, float& to_light)
{
    hx = r.ox + r.dx * r.tmax; hy = r.oy + r.dy * r.tmax; hz = r.oz + r.dz * r.tmax;
    lx = p.light[0] - hx; ly = p.light[1] - hy; lz = p.light[2] - hz;
    to_light = sqrtf(lx * lx + ly * ly + lz * lz);      // length(light_pos - hit_pos) (:455)
    const float linv = 1.0f / to_light;
    lx *= linv; ly *= linv; lz *= linv;
}

// AmbientShader (Tracer.cu:376-469) of a hit: kDiffuse (no textures), kTextureLit (textures + bump), kTextureLitShadows
// (the same with `shadowed` from a shadow ray: rt_trace's second traversal, or the caller's any-hit record)
template <int RENDER, class P>
__device__ __forceinline__ void shade_lit(const P& p, const Ray& r, const Hit& h, float spread, const rt_material& mat,
                                          const Surface& s, float lx, float ly, float lz, bool shadowed, float& R, float& G,
                                          float& B)
{
    constexpr bool use_textures = RENDER == RT_RENDER_TEXTURE_LIT || RENDER == RT_RENDER_TEXTURE_LIT_SHADOWS;
    constexpr bool use_bump = use_textures;
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

}  // namespace rt
