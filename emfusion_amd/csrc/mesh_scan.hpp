// mesh_scan.hpp -- the exclusive scan of 0/1 flags that mesh_weld.hip and mesh_components.hip rank by: per-workgroup
// sums (block_scan1), one workgroup that scans the sums in place (scan_sums), then block_scan1 again for the ranks.
// No library scan, no atomics: a rank is a pure function of the flags.
#pragma once

#include <hip/hip_runtime.h>

namespace emf_hip {

constexpr int kScanBlock = 256;  // threads of the flag / rank kernels
constexpr int kSumsBlock = 1024; // threads of the one workgroup that scans the sums

// the workgroup's sum of v (all lanes get it) and this lane's exclusive prefix
__device__ __forceinline__ unsigned block_scan1(unsigned v, unsigned& total, unsigned* lds /* [kScanBlock / 64] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kScanBlock / 64; ++w) {
        const unsigned t = lds[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();
    return before + inc - v;
}

// one workgroup of kSumsBlock threads: sums[b] := sum of sums[0 .. b), sums[nblocks] := the total
__device__ __forceinline__ void scan_sums(unsigned* sums, unsigned nblocks, unsigned* lds /* [16] */, unsigned* carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) *carry = 0u;
    __syncthreads();
    for (unsigned start = 0; start < nblocks; start += kSumsBlock) {
        const unsigned i = start + threadIdx.x;
        const unsigned v = i < nblocks ? sums[i] : 0u;
        unsigned inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == 63) lds[wave] = inc;
        __syncthreads();
        unsigned before = *carry, total = 0u;
        for (int w = 0; w < kSumsBlock / 64; ++w) {
            const unsigned t = lds[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < nblocks) sums[i] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) *carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[nblocks] = *carry;
}

}  // namespace emf_hip
