/*
 * Stand-in for <cuda_runtime.h>: lets g++ compile the reference's CUDA kernel text as host C++.
 * TEST INFRASTRUCTURE ONLY (see oracle/build_ref.py).  Our own text; holds nothing of the reference.
 *
 * A "kernel launch" is ref_launch(): every block and every thread of the grid runs in a fixed
 * order on the calling thread.  That is only valid for kernels without shared memory, atomics or
 * inter-thread ordering; build_ref.py checks the compiled text for those words.
 *
 * Semantics that silently change results, and how they are pinned here:
 *   __float2int_rn   round-half-to-even (nearbyintf under the default rounding mode)
 *   abs(float)       must pick the float overload: <cmath>/<cstdlib> before <math.h>/<stdlib.h>
 *                    pull std::abs(float) into the global namespace (ref_abi.cpp asserts it)
 *   min(float,float) fminf, max(int,int) the integer maximum: CUDA's global overloads
 */
#pragma once
#include <cmath>
#include <cstdlib>
#include <math.h>
#include <stdlib.h>
#include <cassert>
#include <cstddef>
#include <cstring>

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct ushort2 { unsigned short x, y; };
struct uchar3 { unsigned char x, y, z; };
struct uint3 { unsigned x, y, z; };
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};

#define __global__
#define __device__
#define __host__
#define __inline__ inline

inline float2 make_float2(float a, float b) { return {a, b}; }
inline float3 make_float3(float a, float b, float c) { return {a, b, c}; }
inline int2 make_int2(int a, int b) { return {a, b}; }
inline int3 make_int3(int a, int b, int c) { return {a, b, c}; }
inline uchar3 make_uchar3(unsigned char a, unsigned char b, unsigned char c) { return {a, b, c}; }

extern thread_local uint3 threadIdx, blockIdx;
extern thread_local dim3 blockDim, gridDim;

typedef void* cudaStream_t;
inline int cudaDeviceSynchronize() { return 0; }

inline int __float2int_rn(float f) { return (int)nearbyintf(f); }
inline float min(float a, float b) { return fminf(a, b); }
inline int max(int a, int b) { return a > b ? a : b; }

/* kernel<<<grid, block, ...>>>(args) is rewritten to ref_launch(grid, block, kernel, args) */
template <class... P, class... A>
void ref_launch(dim3 g, dim3 b, void (*k)(P...), A&&... a) {
    assert(g.z == 1 && b.z == 1);
    gridDim = g;
    blockDim = b;
    for (unsigned by = 0; by < g.y; ++by)
        for (unsigned bx = 0; bx < g.x; ++bx)
            for (unsigned ty = 0; ty < b.y; ++ty)
                for (unsigned tx = 0; tx < b.x; ++tx) {
                    blockIdx = {bx, by, 0};
                    threadIdx = {tx, ty, 0};
                    k(a...);
                }
}
