// csr_scan.hip -- the second and third launch of every CSR count call (rt_range_count, rt_ray_hits_count,
// rt_tri_overlaps_count): the count kernel has left workgroup-local exclusive prefixes in offsets[0..n) and one total per
// workgroup of kCsrBlock queries in the scratch (rt_csr.hpp); csr_scan_kernel (one workgroup, 64-bit through three limbs)
// turns the totals into exclusive prefixes and writes offsets[n]; csr_add_kernel adds each workgroup's prefix to its offsets.
// Nothing is read back.
#include "rt_csr.hpp"
#include "rt_launch.hpp"

namespace rt {

namespace {

// in-place exclusive scan of the workgroups' totals (one workgroup; a total is below 2^40, three limbs carry 2^63);
// *total = their sum = offsets[n]
__global__ __launch_bounds__(1024) void csr_scan_kernel(uint64_t* __restrict__ block_sums, uint32_t nblocks,
                                                        uint64_t* __restrict__ total)
{
    __shared__ uint32_t ws[20];
    uint64_t running = 0;
    for (uint32_t c = 0; c < nblocks; c += 1024) {
        const uint32_t i = c + threadIdx.x;
        const uint64_t v = i < nblocks ? block_sums[i] : 0ull;
        uint64_t chunk;
        const uint64_t ex = block_excl_scan_u64<1024, 3>(v, ws, &chunk);
        if (i < nblocks) block_sums[i] = running + ex;
        running += chunk;
    }
    if (threadIdx.x == 0) *total = running;
}

// offsets[i] += the prefix of its workgroup
__global__ __launch_bounds__(256) void csr_add_kernel(uint64_t* __restrict__ offsets, const uint64_t* __restrict__ block_sums,
                                                      uint32_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) offsets[i] += block_sums[i / kCsrBlock];
}

}  // namespace

hipError_t launch_csr_offsets(uint64_t* offsets, uint64_t* block_sums, uint32_t n, hipStream_t st)
{
    const uint32_t blocks = csr_blocks(n);
    // (n = 0 still launches the scan's one workgroup: offsets[0] = 0)
    csr_scan_kernel<<<1, 1024, 0, st>>>(block_sums, blocks, offsets + n);
    if (blocks) csr_add_kernel<<<(uint32_t)(((uint64_t)n + 255) / 256), 256, 0, st>>>(offsets, block_sums, n);
    return hipGetLastError();
}

}  // namespace rt
