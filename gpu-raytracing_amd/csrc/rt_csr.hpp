// rt_csr.hpp -- what the set-valued queries share: range_query.hip, ray_hits_query.hip and tri_overlap_query.hip answer in CSR
// (offsets[0..n] by a 64-bit device scan of the per-query counts, then rows written per query segment).  Here: the geometry
// of their common kernel frame (kCsrBlock queries per workgroup, kCsrStackLds stack entries per lane in LDS, one 8-byte total
// per workgroup in the count call's scratch), the 64-bit workgroup scan, the segment prologue of the collect kernels and the
// epilogue.
// The scan over the workgroups' totals and the add pass are csr_scan.hip's (launch_csr_offsets, rt_launch.hpp).
// csr_finish is the frame's epilogue for range_query.hip and tri_overlap_query.hip; ray_hits_query.hip keeps its own, and the
// stack, the box step and the two-phase loop stay written out in each kernel: moved into functions here they compiled to
// other code (DESIGN section 17 has the comparison, file by file and piece by piece).
#pragma once

#include "rt_device.hpp"
#include "rt_traverse.hpp"

namespace rt {

constexpr uint32_t kCsrBlock = kTraceWaves * 64;   // queries per workgroup = offsets per block sum
constexpr int kCsrStackLds = 16;       // LDS-resident stack entries per lane: 16 x 4 B x 256 lanes = 16 KB per workgroup

inline uint32_t csr_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + kCsrBlock - 1) / kCsrBlock); }
// the count call's scratch: one uint64 per workgroup (at least one), 256-byte aligned
inline size_t csr_scratch_bytes(uint32_t n)
{
    const size_t blocks = csr_blocks(n);
    return ((blocks ? blocks : 1) * sizeof(uint64_t) + 255) / 256 * 256;
}

// exclusive scan of one 64-bit value per thread through block_excl_scan_u32, LIMBS limbs of 21 bits: a limb's block sum stays
// below 2^31 for NT <= 1024, so the 32-bit scans are exact and the result is exact for values below 2^(21 LIMBS).
// All NT threads must call it (rt_device.hpp: full waves).
template <int NT, int LIMBS>
__device__ __forceinline__ uint64_t block_excl_scan_u64(uint64_t v, uint32_t* ws, uint64_t* total)
{
    uint64_t r = 0, t = 0;
#pragma unroll
    for (int l = 0; l < LIMBS; l++) {
        uint32_t tl;
        const uint32_t e = block_excl_scan_u32<NT>((uint32_t)(v >> (21 * l)) & 0x1FFFFFu, ws, &tl);
        r += (uint64_t)e << (21 * l);
        t += (uint64_t)tl << (21 * l);
    }
    *total = t;
    return r;
}

// collect: query i's segment [out, out + room) of `rows`, room = offsets[i+1] - offsets[i] clamped into 0 .. 2^32 - 1
template <class T>
__device__ __forceinline__ T* csr_segment(const uint64_t* offsets, T* rows, uint64_t i, uint32_t& room)
{
    const uint64_t o0 = offsets[i], o1 = offsets[i + 1];
    const uint64_t d = o1 > o0 ? o1 - o0 : 0ull;
    room = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
    return rows + o0;
}

// the epilogue of a kernel of the frame, its text moved here verbatim.  COLLECT: counts[i] and the truncation flag; else the
// workgroup's exclusive scan of the counts (a count is below 2^32: two 21-bit limbs; lanes past the batch add 0) into
// offsets[i] and the workgroup's total into block_sums[vb].  Then the status word through ballots (one atomicOr per wave that
// has something to say) and the exact counters through csum (zeroed by threads 0 and 1 at the kernel's start).  Every thread
// of the workgroup must call it.  ws and csum are the kernel's __shared__ arrays.
template <bool COLLECT, uint32_t F_OVERFLOW, uint32_t F_TRUNCATED>
__device__ __forceinline__ void csr_finish(bool in_range, uint64_t i, uint32_t vb, int lane, bool overflow, uint32_t found,
                                           uint32_t room, uint32_t box_tests, uint32_t tri_tests, uint64_t* offsets,
                                           uint64_t* block_sums, uint32_t* counts, uint32_t* status,
                                           unsigned long long* counters, uint32_t* ws, unsigned long long* csum)
{
    uint32_t flags = overflow ? F_OVERFLOW : 0u;
    if (COLLECT) {
        if (in_range && counts) counts[i] = found;
        if (found > room) flags |= F_TRUNCATED;
    } else {
        uint64_t total;
        const uint64_t ex = block_excl_scan_u64<kTraceWaves * 64, 2>(found, ws, &total);
        if (in_range) offsets[i] = ex;
        if (threadIdx.x == 0) block_sums[vb] = total;
    }
    if (status) {
        const bool any_over = __builtin_amdgcn_ballot_w64((flags & F_OVERFLOW) != 0) != 0;
        const bool any_trunc = __builtin_amdgcn_ballot_w64((flags & F_TRUNCATED) != 0) != 0;
        const uint32_t wf = (any_over ? F_OVERFLOW : 0u) | (any_trunc ? F_TRUNCATED : 0u);
        if (wf && lane == 0) atomicOr(status, wf);
    }
    if (counters) {
        const uint32_t bsum = wave_sum_u32(box_tests), tsum = wave_sum_u32(tri_tests);
        __syncthreads();                      // csum's zeroes
        if (lane == 0) {
            atomicAdd(&csum[0], (unsigned long long)bsum);
            atomicAdd(&csum[1], (unsigned long long)tsum);
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const unsigned long long v = csum[threadIdx.x];
            if (v) atomicAdd(&counters[threadIdx.x], v);
        }
    }
}

}  // namespace rt
