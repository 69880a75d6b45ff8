// wave_ops.hpp -- the integer building blocks the kernel files share: the scan and the reduction of a
// wave, the exclusive scan of a workgroup, the one workgroup that scans per-workgroup sums in place, and the scan over
// the runs of equal keys of a wave that lets one lane per run issue the atomic.  Integers only (unsigned, int,
// unsigned long long, uint2): every result is a pure function of the inputs.  The float reductions of the tracking,
// life-cycle and colour kernels are not here: their addition order is part of parity with the oracle.
// Workgroups are one-dimensional and whole waves of 64: the lane is threadIdx.x & 63, the wave threadIdx.x >> 6.
#pragma once

#include <hip/hip_runtime.h>

namespace emf_hip {

constexpr int kScanBlock = 256;   // threads of the flag / rank kernels
constexpr int kSumsBlock = 1024;  // threads of the one workgroup that scans the sums

struct OpAdd {
    template <typename T>
    __device__ __forceinline__ static T apply(T a, T b) { return a + b; }
};
struct OpMin {
    template <typename T>
    __device__ __forceinline__ static T apply(T a, T b) { return min(a, b); }
};
struct OpMax {
    template <typename T>
    __device__ __forceinline__ static T apply(T a, T b) { return max(a, b); }
};
struct OpOr {
    template <typename T>
    __device__ __forceinline__ static T apply(T a, T b) { return a | b; }
};

// uint2 adds and subtracts by component (HIP's vector operators); only the shuffles need an overload
template <typename T>
__device__ __forceinline__ T shfl_up(T v, int o) { return __shfl_up(v, o); }
__device__ __forceinline__ uint2 shfl_up(uint2 v, int o) { return make_uint2(__shfl_up(v.x, o), __shfl_up(v.y, o)); }
template <typename T>
__device__ __forceinline__ T shfl_xor(T v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ uint2 shfl_xor(uint2 v, int o) { return make_uint2(__shfl_xor(v.x, o), __shfl_xor(v.y, o)); }

// the sum of v over the lanes of the wave that are not above this one
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

// v, through a DPP move with the identity lane pattern: a value the compiler cannot look through, so a product that
// went through here is no product to -ffp-contract=fast any more (DESIGN.md 5.26 "CONTRACTION").  For the kernels whose
// bytes must not depend on contraction: every product that feeds a sum goes through mul_rounded.
__device__ __forceinline__ float rounded(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xE4 /* quad_perm 0, 1, 2, 3 */, 0xf, 0xf, false));
}
__device__ __forceinline__ float mul_rounded(float a, float b) { return rounded(__fmul_rn(a, b)); }
// (1 - f) * c0 + f * c1 with g = 1 - f: two products, one sum
__device__ __forceinline__ float lerp_rounded(float g, float f, float c0, float c1) {
    return __fadd_rn(mul_rounded(g, c0), mul_rounded(f, c1));
}

// Op over the 64 lanes of the wave, in every lane
template <typename Op, typename T>
__device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::apply(v, shfl_xor(v, o));
    return v;
}

// the sum of v over a workgroup of NW waves (all lanes get it) and this lane's exclusive prefix; lds may be used again
// when it returns
template <int NW, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T& total, T* lds /* [NW] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_inclusive_scan(v);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    T before{};
    total = T{};
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const T t = lds[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();
    return before + inc - v;
}

// One workgroup of kSumsBlock threads: sums[i] := sum of sums[lo .. i) for i in [lo, hi), in chunks of kSumsBlock with
// the carry in a register of every lane.  Returns the sum of sums[lo .. hi) as it was, in every lane, and writes
// nothing past hi - 1: where the total goes is the caller's matter.
template <typename T>
__device__ __forceinline__ T scan_sums(T* sums, unsigned lo, unsigned hi, T* lds /* [kSumsBlock / 64] */) {
    T carry{};
    for (unsigned start = lo; start < hi; start += kSumsBlock) {
        const unsigned i = start + threadIdx.x;
        T total;
        const T mine = block_exclusive_scan<kSumsBlock / 64>(i < hi ? sums[i] : T{}, total, lds);
        if (i < hi) sums[i] = carry + mine;
        carry += total;
    }
    return carry;
}

// ---- runs: neighbouring lanes of a wave that share a key ----------------------------------------------------------
// run_scan combines over the lanes of this lane's run that are not above it, in log steps: a lane takes the value o
// lanes below when that lane has the same run number, and concludes that every lane between has it too.  That holds
//   * where run numbers do not recur within the wave: take them from run_id, or use a key that ascends with the lane
//     (voxel_rays.hip: i / group); or
//   * where a number may recur (A, B, A) but Op is idempotent and the value is bound for the key itself, so that what
//     the far A contributes wrongly is what it issues rightly anyway (ground_map.hip: OR into the word that is the key).
// A sum over keys that can come back (planes.hip) needs run_id.  Every lane of the wave must be present at all three:
// a lane with nothing to add brings a key of its own (-1) and the identity, and tests run_is_last before it leaves.

// the number of the run this lane lies in, counted from lane 0 of the wave: unlike keys, run numbers ascend
__device__ __forceinline__ int run_id(int key, int lane) {
    const int below = __shfl_up(key, 1);
    const unsigned long long heads = __ballot(lane == 0 || below != key);
    return __popcll(heads & (~0ull >> (63 - lane)));
}

template <typename Op, typename T>
__device__ __forceinline__ T run_scan(T v, int lane, int run) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T below = shfl_up(v, o);
        const int belowRun = __shfl_up(run, o);
        if (lane >= o && belowRun == run) v = Op::apply(v, below);
    }
    return v;
}

// is this the last lane of its run: the one whose run_scan value covers the run and that issues the atomic
__device__ __forceinline__ bool run_is_last(int run, int lane) {
    const int above = __shfl_down(run, 1);
    return lane == 63 || above != run;
}

}  // namespace emf_hip
