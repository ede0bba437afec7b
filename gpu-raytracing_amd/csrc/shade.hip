// shade.hip -- deferred shading: frames from ray-query hit records (rt_generate_shadow_rays, rt_shade_frame).
//
// rt_trace shades inside its traversal kernel: the shaded instantiations carry the traversal state and the shader at once
// and spill (trace_kernel<7, false>: 195 spilled VGPRs).  Here the two halves are separate launches that meet in memory:
//   rt_generate_camera_rays -> rt_intersect_rays -> [rt_generate_shadow_rays -> rt_intersect_rays(any hit)] -> rt_shade_frame
// The traversal runs in its lean form (64 VGPRs, 8 waves per SIMD) and the shader below has no stack and no LDS.
//
// shadow_rays_kernel: one thread per ray.  The ray is the one trace_kernel's kTextureLitShadows sample builds from its hit
// (light_vector, rt_shade.hpp -- the same function), written at the index of its primary ray.
// shade_kernel<RENDER, TILED>: one thread per pixel, a loop over the spp samples in trace_kernel's order and with its
// accumulation.  Per sample: two 16-byte loads for the ray, one for the hit record, 4 bytes of the shadow record (mode 8),
// then the caller's triangle (rotation 0: triangles[primitive_id], attribute corners 0, 1, 2) and the shaders of
// rt_shade.hpp.  TILED: a wave is one 8 x 8 tile (lane = Morton position) and reads one sample of it per iteration, 2 KB of
// consecutive rays; off-frame lanes of edge tiles leave at once.  Row-major: 64 consecutive pixels of the frame per wave.
// All addresses are 64-bit.  A record is a hit iff primitive_id < num_triangles; its other fields are not looked at otherwise.
// Compiled with -ffp-contract=off: per sample bit-identical to trace_kernel given the same hit.
#include "rt_device.hpp"
#include "rt_launch.hpp"
#include "rt_shade.hpp"

namespace rt {

struct ShadeParams {
    const rt_attributes* attributes;
    const rt_material* materials;
    const rt_texture* textures;
    const rt_triangle* triangles;
    const float4* rays;          // rt_ray = two float4: (origin, tmin), (dir, tmax)
    const float4* hits;          // rt_hit = one float4: (t, primitive_id bits, u, v)
    const rt_hit* shadow_hits;   // mode 8: primitive_id < num_triangles = occluded
    float light[3];
    uint32_t num_triangles, num_materials, num_textures;
    uint32_t* rgba8;
    uint32_t w, h, spp, tiles_x;
};

// one sample: ray i with its records -> float colour 0..255 per channel + alpha (shade_sample of trace_kernel.hip after
// trace_ray, with rotation 0)
template <int RENDER>
__device__ __forceinline__ void shade_record(const ShadeParams& p, uint64_t i, float& R, float& G, float& B, float& A)
{
    const float4 ra = p.rays[2 * i], rb = p.rays[2 * i + 1], hr = p.hits[i];
    const uint32_t prim = __float_as_uint(hr.y);
    const bool hit = prim < p.num_triangles;
    R = G = B = 0;
    A = 255.0f;
    if (RENDER == RT_RENDER_DEPTH) {
        // max_depth is the generated ray's tmax (rt_generate_camera_rays: tmax = camera->max_depth)
        if (hit) R = G = B = fminf(1.0f, hr.x / rb.w) * 255;
        return;
    }
    if (!hit) {
        if (RENDER == RT_RENDER_LODS) { R = 255; G = 0; B = 255; }   // (Tracer.cu:543-556: magenta unless textured AND hit)
        return;
    }
    Ray r;
    r.ox = ra.x; r.oy = ra.y; r.oz = ra.z; r.tmin = ra.w;
    r.dx = rb.x; r.dy = rb.y; r.dz = rb.z; r.tmax = hr.x;
    r.ix = r.iy = r.iz = 0.0f;   // (the shaders do not read them)
    Hit h;
    h.primitive_id = prim; h.tri_id = 0u; h.bu = hr.z; h.bv = hr.w;

    const rt_attributes* at = p.attributes + prim;
    const int material_id = at->material_id;
    rt_material mat;
    fetch_material(p, material_id, mat);
    Surface s = {};
    const rt_float3 n0 = at->normal[0], n1 = at->normal[1], n2 = at->normal[2];
    s.n[0] = v3(n0.x, n0.y, n0.z); s.n[1] = v3(n1.x, n1.y, n1.z); s.n[2] = v3(n2.x, n2.y, n2.z);
    if (render_uses_surface(RENDER)) {
        s.uv[0][0] = at->uv[0][0]; s.uv[0][1] = at->uv[0][1];
        s.uv[1][0] = at->uv[1][0]; s.uv[1][1] = at->uv[1][1];
        s.uv[2][0] = at->uv[2][0]; s.uv[2][1] = at->uv[2][1];
        const rt_triangle* tri = p.triangles + prim;
        const rt_float3 a = tri->v0, b = tri->v1, c = tri->v2;
        s.tri[0] = v3(a.x, a.y, a.z); s.tri[1] = v3(b.x, b.y, b.z); s.tri[2] = v3(c.x, c.y, c.z);
    }
    const float spread = 2.0f / p.w;
    if (shade_unlit<RENDER>(p, r, h, spread, mat, s, material_id, true, true, true, R, G, B, A)) return;
    float hx, hy, hz, lx, ly, lz, to_light;
    light_vector(p, r, hx, hy, hz, lx, ly, lz, to_light);
    bool shadowed = false;
    if (RENDER == RT_RENDER_TEXTURE_LIT_SHADOWS) shadowed = p.shadow_hits[i].primitive_id < p.num_triangles;
    shade_lit<RENDER>(p, r, h, spread, mat, s, lx, ly, lz, shadowed, R, G, B);
}

// Launch bounds: a 256-thread workgroup, and a floor of waves per SIMD under which the instantiation has no scratch
// (DESIGN section 12 has the table): the colour-only render types keep 8 waves, the textured ones get the registers they ask for
constexpr int shade_min_waves(int render)
{
    return render == RT_RENDER_DEPTH || render == RT_RENDER_MATERIAL_ID ? 8 : (render == RT_RENDER_DIFFUSE ? 4 : 2);
}

template <int RENDER, bool TILED>
__global__ __launch_bounds__(256, shade_min_waves(RENDER))
void shade_kernel(ShadeParams p)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;   // pixel position: tile * 64 + lane, or y * w + x
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
        shade_record<RENDER>(p, base, R, G, B, A);
    } else {
        float ar = 0, ag = 0, ab = 0, aa = 0;
        for (uint32_t s = 0; s < p.spp; s++) {
            shade_record<RENDER>(p, base + s * stride, R, G, B, A);
            ar += R; ag += G; ab += B; aa += A;
        }
        R = ar / (float)p.spp; G = ag / (float)p.spp; B = ab / (float)p.spp; A = aa / (float)p.spp;
    }
    p.rgba8[(size_t)y * p.w + x] = sat_u8(R) | (sat_u8(G) << 8) | (sat_u8(B) << 16) | (sat_u8(A) << 24);
}

// rt_generate_shadow_rays: one thread per ray (see rt_abi.h for the recipe)
struct LightPos { float light[3]; };
__global__ __launch_bounds__(256) void shadow_rays_kernel(const float4* rays, const float4* hits, uint32_t num_rays,
                                                          uint32_t num_triangles, LightPos light, float4* shadow_rays)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= num_rays) return;
    const float4 ra = rays[2 * i], rb = rays[2 * i + 1], hr = hits[i];
    // a dead primary ray (rt_intersect_rays's rule) has no hit point, whatever its record says
    const bool nan_ray = __builtin_isnan(ra.x) | __builtin_isnan(ra.y) | __builtin_isnan(ra.z) | __builtin_isnan(rb.x) |
                         __builtin_isnan(rb.y) | __builtin_isnan(rb.z);
    const bool live = ra.w <= rb.w && !nan_ray;
    float4 o = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, -1.f};
    if (live && __float_as_uint(hr.y) < num_triangles) {
        Ray r;
        r.ox = ra.x; r.oy = ra.y; r.oz = ra.z; r.dx = rb.x; r.dy = rb.y; r.dz = rb.z; r.tmax = hr.x;
        float hx, hy, hz, dx, dy, dz, to_light;
        light_vector(light, r, hx, hy, hz, dx, dy, dz, to_light);
        o = float4{hx, hy, hz, 0.001f};
        d = float4{dx, dy, dz, to_light};
    }
    shadow_rays[2 * i] = o;
    shadow_rays[2 * i + 1] = d;
}

hipError_t launch_shadow_rays(const rt_ray* rays, const rt_hit* hits, uint32_t num_rays, uint32_t num_triangles,
                              const float light[3], rt_ray* shadow_rays, hipStream_t st)
{
    const uint32_t blocks = (uint32_t)(((uint64_t)num_rays + 255) / 256);
    shadow_rays_kernel<<<dim3(blocks), dim3(256), 0, st>>>(reinterpret_cast<const float4*>(rays),
                                                          reinterpret_cast<const float4*>(hits), num_rays, num_triangles,
                                                          LightPos{{light[0], light[1], light[2]}},
                                                          reinterpret_cast<float4*>(shadow_rays));
    return hipGetLastError();
}

hipError_t launch_shade_frame(const ShadeLaunch& t, hipStream_t st)
{
    ShadeParams p;
    p.attributes = t.scene.attributes;
    p.materials = t.scene.materials;
    p.textures = t.scene.textures;
    p.triangles = t.triangles;
    p.rays = reinterpret_cast<const float4*>(t.rays);
    p.hits = reinterpret_cast<const float4*>(t.hits);
    p.shadow_hits = t.shadow_hits;
    p.light[0] = t.scene.light[0]; p.light[1] = t.scene.light[1]; p.light[2] = t.scene.light[2];
    p.num_triangles = t.num_triangles;
    p.num_materials = t.scene.num_materials;
    p.num_textures = t.scene.textures ? t.scene.num_textures : 0;
    p.rgba8 = reinterpret_cast<uint32_t*>(t.rgba8);
    p.w = t.w; p.h = t.h; p.spp = t.spp;
    p.tiles_x = (t.w + 7) / 8;
    const uint64_t tiles_y = (t.h + 7) / 8;
    const uint64_t positions = t.tiled ? (uint64_t)p.tiles_x * tiles_y * 64u : (uint64_t)t.w * t.h;
    const uint64_t blocks = (positions + 255) / 256;
    if (blocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks), block(256);
#define RT_SHADE_CASE(R) case R: if (t.tiled) shade_kernel<R, true><<<grid, block, 0, st>>>(p); else shade_kernel<R, false><<<grid, block, 0, st>>>(p); break;
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
