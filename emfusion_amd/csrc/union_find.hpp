// union_find.hpp -- the lock-free union-find that mesh_components.hip (over welded vertex indices) and
// motion_masks.hip (over linear pixel indices) label connected components with.
//
// parent[x] <= x always, a root is its own parent.  find walks to the root and halves the path it walks with
// atomicMin -- parent[x] only ever decreases, and only to an ancestor; unite hooks the larger root under the
// smaller with a CAS and, on failure, goes on from what the CAS saw.  Every step of every loop moves to a
// strictly smaller index, so each loop is bounded by construction and no lane waits for another lane's progress
// (no lock, no spin-wait: a wave runs in lock-step).  The root of a tree is its minimum index, whatever order
// the hooks ran in.  All atomics are ordinary global atomics on vector memory.
#pragma once

#include <hip/hip_runtime.h>

namespace emf_hip {

__device__ __forceinline__ unsigned load_parent(const unsigned* parent, unsigned x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above x at the time of the walk.  Every step goes to a strictly smaller index (parent[y] < y for a
// non-root), so the loop ends after at most x steps; nodes on the way are pointed at their grandparent.
__device__ __forceinline__ unsigned find_root(unsigned* parent, unsigned x) {
    unsigned p = load_parent(parent, x);
    while (p < x) {
        const unsigned gp = load_parent(parent, p);
        if (gp < p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

// Joins the trees of a and b.  Each round either ends or goes on from indices of which one is strictly smaller than
// before (a failed CAS saw a parent below the root it tried to hook), so the rounds are bounded by a + b.
__device__ __forceinline__ void unite(unsigned* parent, unsigned a, unsigned b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
        const unsigned seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        a = seen;  // hi was hooked meanwhile: seen < hi
        b = lo;
    }
}

}  // namespace emf_hip
