// ref_kernels_driver.cpp -- TEST INFRASTRUCTURE: runs the reference's own LBVH kernels and its tracer on the CPU.
// It #includes BottomUpBuilder.cu and Tracer.cu from the reference tree where they lie (nothing is copied or edited);
// ref_cuda_host.h, force-included ahead of this file, stands in for the CUDA built-ins they use.  Each entry point
// emulates one launch by looping over blockIdx / threadIdx and calling the __global__ function as the reference wrote
// it.  Built into oracle/_ref by oracle/Makefile; only tests/ load it (oracle/oracle_py.py: ref_build_lbvh, ref_trace).
//
// What is and is not emulated:
// - GenerateMortonCodes, GenerateHierarchy, GenerateTriangles: one thread per item, no cross-thread traffic; any
//   order is the reference's result.
// - GenerateMortonCodesPairs claims leaf slots with atomicAdd, so on a GPU the leaf order is the order in which the
//   threads arrive.  Here the threads run one after another in gid order: slot = running sum of the leaf counts of
//   the candidates before it.  That is one of the orders a GPU can produce; callers compare the leaf *multiset*.
// - GenerateAABBs climbs the tree by last-arrival locks.  It runs serially: a serial run is a valid interleaving of that
//   protocol (the first thread to reach a parent stops, the second one carries on with both children's boxes ready),
//   and it does not lean on how a host compiler orders volatile accesses between threads.
// - The radix sort (RadixSort.cu) is block-cooperative and is not emulated: callers sort (key, value) stably, which
//   is its contract.
// - TraceRays: blockDim = (w,1,1), gridDim = (1,h,1), so w and h are exact for any frame size; rows run on up to 16
//   host threads.  Each TraceRays thread owns its stack and its pixel; the box-test counter goes through atomicAdd.
#include <omp.h>

#include <algorithm>
#include <new>
#include <vector>

#include "BottomUpBuilder.cu"
#include "Tracer.cu"

thread_local uint3 threadIdx;
thread_local uint3 blockIdx;
thread_local dim3 blockDim;
thread_local dim3 gridDim;
thread_local void (*ref_atomic_add_observer)(const void*) = nullptr;

namespace {

constexpr unsigned kBlock = 256;

template <class F> void launch_1d(unsigned threads, F&& kernel)
{
    blockDim = dim3(kBlock, 1, 1);
    gridDim = dim3((threads + kBlock - 1) / kBlock, 1, 1);
    for (unsigned b = 0; b < gridDim.x; ++b) {
        for (unsigned t = 0; t < kBlock; ++t) {
            blockIdx = make_uint3(b, 0, 0);
            threadIdx = make_uint3(t, 0, 0);
            kernel();
        }
    }
}

// the oracle's POD views of the scene (oracle/rt_oracle.h: ora_material, ora_texture)
struct PodMaterial {
    float ambient[3], diffuse[3], specular[3];
    float specular_exp;
    int32_t texture, bump, disp;
};
struct PodTexture {
    const uint32_t* mips[NUM_LODS];
    int32_t size_x[NUM_LODS], size_y[NUM_LODS];
    uint32_t max_lod, pad;
};

thread_local unsigned* tri_tests_slot = nullptr;

void read_tri_tests(const void* operand)   // operand = &stats.box_tests, the first member of TraceRays' TraceStats
{
    const TraceStats* stats = reinterpret_cast<const TraceStats*>(static_cast<const unsigned*>(operand));
    *tri_tests_slot = stats->tri_tests;
}

}  // namespace

extern "C" {

static_assert(sizeof(Node) == 32 && sizeof(TrianglePair) == 64 && sizeof(Camera) == 64 && sizeof(Attributes) == 72,
              "the reference's PODs must match the oracle's layouts");

// GenerateMortonCodes: tris = n x 9 floats, aabb = the scene box as ordered ints (min xyz, max xyz)
void ref_morton(const float* tris, unsigned n, const int32_t* aabb, unsigned* codes, unsigned* values)
{
    launch_1d(n, [&] {
        GenerateMortonCodes(codes, values, (float3*)tris, (AABB*)aabb, n);
    });
}

// GenerateMortonCodesPairs, threads in gid order (see the top of the file).  codes / values: n entries.  Returns the
// number of leaves.
unsigned ref_morton_pairs(const float* tris, unsigned n, const int32_t* aabb, unsigned* codes, unsigned* values)
{
    unsigned num_leaves = 0;
    launch_1d((n + 1) / 2, [&] {
        GenerateMortonCodesPairs(codes, values, (float3*)tris, (AABB*)aabb, &num_leaves, n);
    });
    return num_leaves;
}

// GenerateHierarchy over n sorted codes: nodes = 2*(n-1) slots, zeroed by the caller; leaf_indices = n entries
void ref_hierarchy(unsigned* codes, unsigned n, void* nodes, unsigned* leaf_indices)
{
    launch_1d(n, [&] {
        GenerateHierarchy((volatile Node*)nodes, leaf_indices, codes, nullptr, (int)n);
    });
}

// GenerateTriangles.  tris must hold n + 1 triangles: the kernel reads the triangle after every leaf's first one,
// also for the last single leaf.
void ref_triangles(unsigned* sorted_indices, const float* tris, void* leaves, unsigned n)
{
    launch_1d(n, [&] {
        GenerateTriangles(sorted_indices, (float3*)tris, (TrianglePair*)leaves, n);
    });
}

// GenerateAABBs with zeroed locks, serially.  nodes: the hierarchy from ref_hierarchy.
void ref_aabbs(void* nodes, unsigned* leaf_indices, unsigned* sorted_indices, void* leaves, unsigned n)
{
    std::vector<unsigned> locks(std::max(n, 1u), 0u);
    launch_1d(n, [&] {
        GenerateAABBs((volatile Node*)nodes, leaf_indices, sorted_indices, locks.data(), (TrianglePair*)leaves, n);
    });
}

// TraceRays over a w x h frame.  attributes: the reference's Attributes records (72 B, same layout as the oracle's);
// materials / textures: the oracle's POD views, converted here.  out_rgba: w*h*4 bytes.  out_tests[0] = the kernel's
// box-test counter, out_tests[1] = the sum of its per-ray triangle-test counts.
void ref_trace(const void* leaves, const void* nodes, unsigned root, unsigned count, const void* camera,
               const void* attributes, unsigned num_attributes, const void* materials, unsigned num_materials,
               const void* textures, unsigned num_textures, const float* light, int w, int h, int render_type,
               uint8_t* out_rgba, unsigned long long* out_tests)
{
    // Material declares a destructor the reference defines elsewhere: the records live in raw storage and are not
    // destroyed (their names are empty, so they own no memory).
    const PodMaterial* pm = static_cast<const PodMaterial*>(materials);
    void* mat_store = ::operator new(sizeof(Material) * std::max(num_materials, 1u));
    Material* mats = static_cast<Material*>(mat_store);
    for (unsigned i = 0; i < num_materials; ++i) {
        Material* m = new (&mats[i]) Material(std::string());
        m->ambient = make_float3(pm[i].ambient[0], pm[i].ambient[1], pm[i].ambient[2]);
        m->diffuse = make_float3(pm[i].diffuse[0], pm[i].diffuse[1], pm[i].diffuse[2]);
        m->specular = make_float3(pm[i].specular[0], pm[i].specular[1], pm[i].specular[2]);
        m->specular_exp = pm[i].specular_exp;
        m->texture = pm[i].texture;
        m->bump = pm[i].bump;
        m->disp = pm[i].disp;
    }
    const PodTexture* pt = static_cast<const PodTexture*>(textures);
    std::vector<Texture> texs;
    texs.reserve(num_textures);
    for (unsigned i = 0; i < num_textures; ++i) {
        texs.emplace_back(std::string());
        Texture& t = texs.back();
        for (unsigned l = 0; l < NUM_LODS; ++l) {
            t.gpu_mips[l] = l <= pt[i].max_lod ? (uchar4*)pt[i].mips[l] : nullptr;
            t.sizes[l] = l <= pt[i].max_lod ? make_int2(pt[i].size_x[l], pt[i].size_y[l]) : make_int2(0, 0);
        }
        t.max_lod = pt[i].max_lod;
    }

    DeviceAccelerationStructure as;
    as.triangles = (TrianglePair*)leaves;
    as.nodes = (Node*)nodes;
    as.root = root;
    as.count = count;
    DeviceScene scene;
    scene.attributes = (Attributes*)attributes;
    scene.materials = mats;
    scene.textures = texs.empty() ? nullptr : texs.data();
    scene.camera = (Camera*)camera;
    scene.light = make_float3(light[0], light[1], light[2]);
    scene.num_attributes = num_attributes;
    scene.num_materials = num_materials;
    scene.num_textures = num_textures;

    RefSurface surface = {(uchar4*)out_rgba, w};
    const cudaSurfaceObject_t image = (cudaSurfaceObject_t)(uintptr_t)&surface;
    uint32_t box_tests = 0;
    std::vector<unsigned> tri_tests((size_t)w * h, 0u);

#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min(16, std::max(1, omp_get_max_threads())))
    for (int y = 0; y < h; ++y) {
        blockDim = dim3(w, 1, 1);
        gridDim = dim3(1, h, 1);
        blockIdx = make_uint3(0, y, 0);
        ref_atomic_add_observer = read_tri_tests;
        for (int x = 0; x < w; ++x) {
            threadIdx = make_uint3(x, 0, 0);
            tri_tests_slot = &tri_tests[(size_t)y * w + x];
            TraceRays(as, scene, &box_tests, (RenderType)render_type, image);
        }
        ref_atomic_add_observer = nullptr;
    }

    unsigned long long tri_sum = 0;
    for (unsigned t : tri_tests) tri_sum += t;
    out_tests[0] = box_tests;
    out_tests[1] = tri_sum;
    ::operator delete(mat_store);
}

}  // extern "C"
