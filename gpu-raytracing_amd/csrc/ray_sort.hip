// ray_sort.hip -- rt_sort_rays: a coherence order for a caller's ray batch (semantics and the exact key recipe: rt_abi.h,
// "ray sorting"; the measured key layouts: DESIGN section 11).
//
// Three steps on the caller's stream, a fixed number of launches for a given num_rays:
//   1. ray_sort_init_kernel, one wave: the tree's box = ordered min / max over the non-NONE slots of the root run (at most 7
//      slots, read as prepare_instances_kernel reads a BLAS's box) into the scratch header, num_live = 0;
//   2. ray_key_kernel, one thread per ray: two 16-byte loads, the box from the header through uniform loads, one key store
//      straight into the array the sort reads first (no index is stored: the sort's first pass takes the values as the
//      identity); live rays are counted by a wave ballot, one LDS add per wave and one device atomic per workgroup of
//      4096 rays (one workgroup per 256 rays queued 8,100 same-address atomics behind a 1080p batch: 94 us for the launch);
//   3. launch_radix_sort on 30-bit keys (radix_sort.hip, unchanged): `order` is its value array.
// Compiled with -ffp-contract=off: every float operation of the key is the documented one (tests/ray_sort_ref.py restates
// it in numpy, bit for bit).
#include "rt_device.hpp"
#include "rt_launch.hpp"

namespace rt {

namespace {

constexpr uint32_t kRayKeyBits = RT_RAY_KEY_BITS;           // what the sort is told: three 10-bit passes up to kSort3PassMaxTiles tiles
constexpr uint32_t kRayDeadKey = RT_RAY_KEY_DEAD;     // a dead ray's whole key: after every live ray, in index order

constexpr uint32_t kRaysPerKeyBlock = 4096;     // rays per workgroup of the key kernel (16 rounds of 256)

struct RaySortHeader {      // the first 256 bytes of the scratch
    float lo[4], hi[4];     // the box (w unused, 0)
    uint32_t num_live;
    uint32_t pad[55];
};
static_assert(sizeof(RaySortHeader) == 256, "ray sort scratch header");

// bits of v (< 1024) moved to positions 0, 3, 6, ...
__device__ __forceinline__ uint32_t spread3(uint32_t v)
{
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton3(uint32_t x, uint32_t y, uint32_t z)
{
    return (spread3(x) << 2) | (spread3(y) << 1) | spread3(z);
}

// cell of a scaled coordinate q among `cells` (a power of two): truncation inside (0, cells - 1), the border cells outside,
// cell 0 for a NaN.  Selects only.
__device__ __forceinline__ uint32_t cell_of(float q, uint32_t cells)
{
    uint32_t c = 0u;
    if (q > 0.0f) c = q >= (float)(cells - 1u) ? cells - 1u : (uint32_t)(int)q;
    return c;
}

// The key of a live ray.  OB origin bits and DB direction bits per axis.
template <uint32_t OB, uint32_t DB>
__device__ __forceinline__ void ray_cells(const float4& a, const float4& b, const RaySortHeader* __restrict__ hd, uint32_t* oc,
                                          uint32_t* dc)
{
    constexpr uint32_t OC = 1u << OB, DC = 1u << DB;
    const float o[3] = {a.x, a.y, a.z}, d[3] = {b.x, b.y, b.z};
    float m = fabsf(d[0]);
    if (fabsf(d[1]) > m) m = fabsf(d[1]);
    if (fabsf(d[2]) > m) m = fabsf(d[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float e = hd->hi[k] - hd->lo[k];
        oc[k] = cell_of(((o[k] - hd->lo[k]) / e) * (float)OC, OC);
        dc[k] = DB ? cell_of((d[k] / m) * (float)(DC / 2u) + (float)(DC / 2u), DC) : 0u;
    }
}

// shipped layout: 7 origin bits per axis, Morton-interleaved, above 2 direction bits per axis, Morton-interleaved (27 bits)
__device__ __forceinline__ uint32_t ray_key(const float4& a, const float4& b, const RaySortHeader* __restrict__ hd)
{
    uint32_t oc[3], dc[3];
    ray_cells<7, 2>(a, b, hd, oc, dc);
    return (morton3(oc[0], oc[1], oc[2]) << 6) | morton3(dc[0], dc[1], dc[2]);
}

#ifdef RT_EXP_RAY_KEYS
// experiment arms (make librt_amd_exp.so EXPFLAGS=-DRT_EXP_RAY_KEYS, layout picked per launch by the RT_RAY_KEY environment
// variable; tools/ray_sort_bench.py --layouts): the layouts DESIGN section 11 compares.  Not in the shipped library.
__device__ __forceinline__ uint32_t ray_key_exp(int layout, const float4& a, const float4& b, const RaySortHeader* __restrict__ hd)
{
    uint32_t oc[3], dc[3];
    switch (layout) {
    case 1: {   // octant first: the direction signs on top, then the origin, then the finer direction bit
        ray_cells<7, 2>(a, b, hd, oc, dc);
        const uint32_t md = morton3(dc[0], dc[1], dc[2]);
        return ((md >> 3) << 24) | (morton3(oc[0], oc[1], oc[2]) << 3) | (md & 7u);
    }
    case 2:     // 6 origin bits and 3 direction bits per axis
        ray_cells<6, 3>(a, b, hd, oc, dc);
        return (morton3(oc[0], oc[1], oc[2]) << 9) | morton3(dc[0], dc[1], dc[2]);
    case 3:     // origin only, 9 bits per axis
        ray_cells<9, 0>(a, b, hd, oc, dc);
        return morton3(oc[0], oc[1], oc[2]);
    case 4:     // direction major: 2 direction bits per axis above 7 origin bits per axis
        ray_cells<7, 2>(a, b, hd, oc, dc);
        return (morton3(dc[0], dc[1], dc[2]) << 21) | morton3(oc[0], oc[1], oc[2]);
    case 5:     // 8 origin bits and 1 direction bit (the sign) per axis
        ray_cells<8, 1>(a, b, hd, oc, dc);
        return (morton3(oc[0], oc[1], oc[2]) << 3) | morton3(dc[0], dc[1], dc[2]);
    default: return ray_key(a, b, hd);
    }
}
#endif

__global__ __launch_bounds__(64) void ray_sort_init_kernel(const rt_node* nodes, uint32_t root, uint32_t count, RaySortHeader* hd)
{
    if (threadIdx.x != 0) return;
    int lo_i[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi_i[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    bool any = false;
    for (uint32_t s = 0; s < count; s++) {
        const rt_node nd = nodes[(root & kIndexMask) + s];
        if ((nd.w28 >> 29) == RT_CHILD_NONE) continue;
        any = true;
        const float mn[3] = {nd.min.x, nd.min.y, nd.min.z}, mx[3] = {nd.max.x, nd.max.y, nd.max.z};
        for (int k = 0; k < 3; k++) {
            lo_i[k] = min(lo_i[k], float_to_ordered_int(mn[k]));
            hi_i[k] = max(hi_i[k], float_to_ordered_int(mx[k]));
        }
    }
    for (int k = 0; k < 3; k++) {   // an empty tree or a run of NONE slots: the box is the point 0
        hd->lo[k] = any ? ordered_int_to_float(lo_i[k]) : 0.0f;
        hd->hi[k] = any ? ordered_int_to_float(hi_i[k]) : 0.0f;
    }
    hd->lo[3] = hd->hi[3] = 0.0f;
    hd->num_live = 0u;
}

__global__ __launch_bounds__(256) void ray_key_kernel(const float4* __restrict__ rays, uint32_t num_rays,
                                                      const RaySortHeader* __restrict__ hd, uint32_t* __restrict__ num_live,
                                                      uint32_t* __restrict__ keys, int layout)
{
    __shared__ uint32_t live_sum;
    if (threadIdx.x == 0) live_sum = 0u;
    __syncthreads();
    uint32_t n_live = 0u;   // wave-uniform
    // kRaysPerKeyBlock rays per workgroup, 256 consecutive rays per round: few workgroups, so few same-address atomics
    for (uint32_t round = 0; round < kRaysPerKeyBlock / 256u; round++) {
        const uint32_t i = blockIdx.x * kRaysPerKeyBlock + round * 256u + threadIdx.x;   // (num_rays <= 0x3FFFFFFF: no wrap)
        const bool in_range = i < num_rays;
        float4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, -1.f};
        if (in_range) { a = rays[2 * (uint64_t)i]; b = rays[2 * (uint64_t)i + 1]; }
        // rt_intersect_rays's rule, word for word (ray_query.hip)
        const bool nan_ray = __builtin_isnan(a.x) | __builtin_isnan(a.y) | __builtin_isnan(a.z) | __builtin_isnan(b.x) |
                             __builtin_isnan(b.y) | __builtin_isnan(b.z);
        const bool live = in_range && a.w <= b.w && !nan_ray;
        uint32_t key = kRayDeadKey;
        if (live) {
#ifdef RT_EXP_RAY_KEYS
            key = ray_key_exp(layout, a, b, hd);
#else
            key = ray_key(a, b, hd);
#endif
        }
        if (in_range) keys[i] = key;
        n_live += (uint32_t)__popcll(__ballot(live));
    }
    if ((threadIdx.x & 63u) == 0u && n_live) atomicAdd(&live_sum, n_live);
    __syncthreads();
    if (threadIdx.x == 0 && live_sum) atomicAdd(num_live, live_sum);
}

}  // namespace

static inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

RaySortLayout ray_sort_layout(uint32_t num_rays)
{
    RaySortLayout L;
    const size_t nn = num_rays ? num_rays : 1;
    size_t off = 0;
    L.box = off;
    L.num_live = off + offsetof(RaySortHeader, num_live);
    off += sizeof(RaySortHeader);
    L.keys = off;       off = align256(off + nn * 4);
    L.tmp_keys = off;   off = align256(off + nn * 4);
    L.tmp_values = off; off = align256(off + nn * 4);
    L.sort = off;       off = align256(off + sort_scratch_layout(num_rays).total);
    L.total = off;
    return L;
}

hipError_t launch_sort_rays(const rt_accel& as, const rt_ray* rays, uint32_t num_rays, uint32_t* order, void* scratch,
                            hipStream_t st)
{
    const RaySortLayout L = ray_sort_layout(num_rays);
    char* s = static_cast<char*>(scratch);
    RaySortHeader* hd = reinterpret_cast<RaySortHeader*>(s + L.box);
    uint32_t* keys = reinterpret_cast<uint32_t*>(s + L.keys);
    uint32_t* tmpk = reinterpret_cast<uint32_t*>(s + L.tmp_keys);
    uint32_t* tmpv = reinterpret_cast<uint32_t*>(s + L.tmp_values);
    int layout = 0;
#ifdef RT_EXP_RAY_KEYS
    if (const char* e = getenv("RT_RAY_KEY")) layout = atoi(e);
#endif
    ray_sort_init_kernel<<<1, 64, 0, st>>>(as.nodes, as.root, as.count, hd);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // three passes read their input from the temporaries, four from keys / order: the result is in keys / order either way
    const bool three = sort_three_passes(sort_num_tiles(num_rays));
    ray_key_kernel<<<(num_rays + kRaysPerKeyBlock - 1u) / kRaysPerKeyBlock, 256, 0, st>>>(reinterpret_cast<const float4*>(rays), num_rays, hd,
                                                             &hd->num_live, three ? tmpk : keys, layout);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // ident0: the unsorted values are the ray indices 0 .. num_rays - 1, which the first pass makes up itself
    return launch_radix_sort(keys, order, tmpk, tmpv, num_rays, s + L.sort, st, nullptr, kRayKeyBits, false, true);
}

}  // namespace rt
