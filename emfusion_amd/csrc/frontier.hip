// frontier.hip -- exploration frontiers: the free voxels of a box of class bytes that touch unknown space, their
// 26-connected clusters and one record per cluster (include/emf_hip.h "Frontiers").
//
// Linear index i = (z * ny + y) * nx + x < 2^31.  The label volume is the union-find's parent array: a frontier voxel
// holds an index <= its own, every other voxel the sentinel -1, which is never followed and never changes.
//   k_fr_flags    one wave per row.  The free and unknown bits of 64 voxels are two __ballots; the x neighbours are
//                 the unknown ballot shifted by one with a carry from the chunk before and the chunk after, y +- 1 and
//                 z +- 1 the unknown ballots of four other rows (those inside the box).  labels[i] = i at a frontier
//                 voxel (after the clearance gate d2[i] >= min_d2), -1 elsewhere; frontier voxels counted per wave.
//   k_fr_hook     per frontier voxel: unite with the frontier voxels among its 13 neighbours of smaller linear index
//                 (dz = -1: nine, dz = 0 and dy = -1: three, x - 1) -- every pair of the 26-neighbourhood once.
//                 union_find.hpp as it is: lock-free, every step to a strictly smaller index.
//   k_fr_flatten  labels[i] := root of i, the minimum index of the cluster whatever order the hooks ran in
//   k_fr_count    roots (labels[i] == i), summed per workgroup, one atomicAdd per workgroup that has any
//   k_fr_rootsums roots per workgroup of 256 voxels -> bsums;  k_fr_scan: their exclusive scan (wave_ops.hpp)
//   k_fr_roots    roots[rank] = i in index order, placed by scan; clears the slot's statistics
//   k_fr_stats    one wave per row, 16 rows per workgroup.  A RUN is a maximal stretch of consecutive lanes with the
//                 same label: same y and z, consecutive x, so its count, sums and box follow from its first x and
//                 its length.  While the chunks of a row hold one label the wave keeps one pending part (popcount, one
//                 wave reduction for the sum of x); the workgroup's waves merge their parts by label through LDS, and
//                 one lane per label finds the cluster's slot by binary search of the label in the sorted roots and
//                 adds count and the three u64 sums, atomicMin / atomicMax for the box where the part moves it.  A
//                 chunk with several labels adds its runs one by one.
//   k_fr_rep      one wave per row.  The first lane of a run finds the slot and computes the rounded centroid from the
//                 finished sums (three 64-bit divisions per run, not per voxel) and hands both to the run's lanes,
//                 each of which offers its key (dist^2 << 31 | i) to a 64-bit atomicMin -- only where it is below
//                 the key it reads.
//   k_fr_keepsums kept flags (count >= min_voxels) per workgroup of 256 slots -> csums;  k_fr_scan again
//   k_fr_emit     kept slots write their record at their rank (label order: the slots are sorted by label) while the
//                 rank is below capacity; thread 0 writes the kept total
// Integer atomics on vector memory only: no result depends on the order of workgroups.  No index leaves its array: a
// neighbour is tested against the box before it is read, a slot is used only where roots[slot] == label with
// slot < min(n_clusters, roots found), a record's rank is below capacity.
#include "common.hpp"
#include "wave_ops.hpp"
#include "union_find.hpp"

#include <climits>

namespace emf_hip {
namespace {

constexpr int kFrBlock = kScanBlock;
constexpr unsigned kNone = 0xffffffffu;  // -1: no frontier voxel

static_assert(sizeof(emf_frontier_cluster_t) == 72, "emf_frontier_cluster_t is mirrored by emfusion_amd/_lib.py");

struct FrArgs {
    unsigned long long* sums;  // 3 per slot
    unsigned long long* key;   // per slot
    unsigned* roots;           // per slot, ascending
    unsigned* count;           // per slot
    int* box;                  // 6 per slot: lo x y z, hi x y z
    unsigned* bsums;           // blocks + 1
    unsigned* csums;           // cblocks + 1
    unsigned n, nc, blocks, cblocks;
    int nx, ny, nz;
};

inline size_t place(FrArgs& a, const int32_t size[3], unsigned nc, void* scratch) {
    const size_t n = static_cast<size_t>(size[0]) * size[1] * static_cast<size_t>(size[2]);
    a.nx = size[0];
    a.ny = size[1];
    a.nz = size[2];
    a.n = static_cast<unsigned>(n);
    a.nc = nc;
    a.blocks = ceil_div(n, kFrBlock);
    a.cblocks = ceil_div(nc, kFrBlock);
    ScratchArena s{static_cast<char*>(scratch), 0};
    a.sums = s.take<unsigned long long>(3 * static_cast<size_t>(nc));
    a.key = s.take<unsigned long long>(nc);
    a.roots = s.take<unsigned>(nc);
    a.count = s.take<unsigned>(nc);
    a.box = s.take<int>(6 * static_cast<size_t>(nc));
    a.bsums = s.take<unsigned>(a.blocks + 1);
    a.csums = s.take<unsigned>(a.cblocks + 1);
    return s.off;
}

// the free and the unknown bits of chunk k of a row (bit l: voxel 64 k + l; nothing past the row's end)
__device__ __forceinline__ void row_bits(const uint8_t* __restrict__ c, int nx, int k, int lane, unsigned long long& fr,
                                         unsigned long long& un) {
    const int x = 64 * k + lane;
    const unsigned v = x < nx ? c[x] : 255u;
    fr = __ballot(v == EMF_OCC_FREE);
    un = __ballot(v == EMF_OCC_UNKNOWN);
}

__device__ __forceinline__ unsigned long long unknown_bits(const uint8_t* __restrict__ c, int nx, int k, int lane) {
    const int x = 64 * k + lane;
    return __ballot(x < nx && c[x] == EMF_OCC_UNKNOWN);
}

__global__ __launch_bounds__(256) void k_fr_flags(const uint8_t* __restrict__ classes, const int* __restrict__ d2,
                                                  int minD2, unsigned* __restrict__ labels, unsigned* voxels, int nx,
                                                  int ny, int nz) {
    const int lane = threadIdx.x & 63;
    const size_t rows = static_cast<size_t>(ny) * nz;
    const size_t row = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);  // z * ny + y
    if (row >= rows) return;  // whole waves leave
    const int z = static_cast<int>(row / ny), y = static_cast<int>(row - static_cast<size_t>(z) * ny);
    const size_t base = row * nx, plane = static_cast<size_t>(nx) * ny;
    const uint8_t* c = classes + base;
    const bool ym = y > 0, yp = y + 1 < ny, zm = z > 0, zp = z + 1 < nz;  // wave-uniform
    const int chunks = (nx + 63) >> 6;
    unsigned long long uPrev = 0ull, fCur, uCur;
    row_bits(c, nx, 0, lane, fCur, uCur);
    unsigned found = 0u;
    for (int k = 0; k < chunks; ++k) {
        unsigned long long fNext = 0ull, uNext = 0ull;
        if (k + 1 < chunks) row_bits(c, nx, k + 1, lane, fNext, uNext);
        unsigned long long nb = (uCur << 1) | (uPrev >> 63) | (uCur >> 1) | (uNext << 63);
        if (ym) nb |= unknown_bits(c - nx, nx, k, lane);
        if (yp) nb |= unknown_bits(c + nx, nx, k, lane);
        if (zm) nb |= unknown_bits(c - plane, nx, k, lane);
        if (zp) nb |= unknown_bits(c + plane, nx, k, lane);
        const int x = 64 * k + lane;
        bool front = ((fCur & nb) >> lane) & 1ull;  // never set past the row's end: fCur is not
        if (front && d2 != nullptr && minD2 > 0) front = d2[base + x] >= minD2;
        if (x < nx) labels[base + x] = front ? static_cast<unsigned>(base + x) : kNone;
        found += static_cast<unsigned>(__popcll(__ballot(front)));
        uPrev = uCur;
        uCur = uNext;
        fCur = fNext;
    }
    if (lane == 0 && found) atomicAdd(voxels, found);
}

__global__ __launch_bounds__(kFrBlock) void k_fr_hook(unsigned* labels, int nx, int ny, int nz) {
    const unsigned n = static_cast<unsigned>(nx) * ny * nz;
    const unsigned i = blockIdx.x * kFrBlock + threadIdx.x;
    if (i >= n || load_parent(labels, i) == kNone) return;
    const unsigned plane = static_cast<unsigned>(nx) * ny;
    const int z = static_cast<int>(i / plane), r = static_cast<int>(i - z * plane), y = r / nx, x = r - y * nx;
#pragma unroll
    for (int k = 0; k < 13; ++k) {  // (dz, dy, dx) in index order below (0, 0, 0)
        const int dz = k < 9 ? -1 : 0, dy = k < 9 ? k / 3 - 1 : (k < 12 ? -1 : 0), dx = k < 12 ? k % 3 - 1 : -1;
        const int qx = x + dx, qy = y + dy, qz = z + dz;
        if (qx < 0 || qx >= nx || qy < 0 || qy >= ny || qz < 0) continue;
        const unsigned j = (static_cast<unsigned>(qz) * ny + qy) * nx + qx;
        if (load_parent(labels, j) != kNone) unite(labels, i, j);
    }
}

__global__ __launch_bounds__(kFrBlock) void k_fr_flatten(unsigned* labels, unsigned n) {
    const unsigned i = blockIdx.x * kFrBlock + threadIdx.x;
    if (i >= n || load_parent(labels, i) == kNone) return;
    const unsigned r = find_root(labels, i);
    atomicMin(labels + i, r);  // (a halving step of another lane may still be under way: the minimum wins)
}

__device__ __forceinline__ unsigned root_flag(const unsigned* labels, unsigned n, unsigned i) {
    return i < n && labels[i] == i ? 1u : 0u;
}

__global__ __launch_bounds__(kFrBlock) void k_fr_count(const unsigned* __restrict__ labels, unsigned n,
                                                       unsigned* clusters) {
    __shared__ unsigned lds[kFrBlock / 64];
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(root_flag(labels, n, blockIdx.x * kFrBlock + threadIdx.x), total, lds);
    if (threadIdx.x == 0 && total) atomicAdd(clusters, total);
}

__global__ __launch_bounds__(kFrBlock) void k_fr_rootsums(const FrArgs a, const unsigned* __restrict__ labels) {
    __shared__ unsigned lds[kFrBlock / 64];
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(root_flag(labels, a.n, blockIdx.x * kFrBlock + threadIdx.x), total, lds);
    if (threadIdx.x == 0) a.bsums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSumsBlock) void k_fr_scan(unsigned* sums, unsigned nblocks) {
    __shared__ unsigned lds[kSumsBlock / 64];
    const unsigned total = scan_sums(sums, 0u, nblocks, lds);
    if (threadIdx.x == 0) sums[nblocks] = total;
}

__global__ __launch_bounds__(kFrBlock) void k_fr_roots(const FrArgs a, const unsigned* __restrict__ labels) {
    __shared__ unsigned lds[kFrBlock / 64];
    const unsigned i = blockIdx.x * kFrBlock + threadIdx.x;
    const unsigned flag = root_flag(labels, a.n, i);
    unsigned total;
    const unsigned rank = a.bsums[blockIdx.x] + block_exclusive_scan<kScanBlock / 64>(flag, total, lds);
    if (!flag || rank >= a.nc) return;
    a.roots[rank] = i;
    a.count[rank] = 0u;
    a.key[rank] = ~0ull;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        a.sums[3 * static_cast<size_t>(rank) + j] = 0ull;
        a.box[6 * static_cast<size_t>(rank) + j] = INT_MAX;
        a.box[6 * static_cast<size_t>(rank) + 3 + j] = -1;
    }
}

// the slot of the cluster labelled `label` among the first nc sorted roots, or kNone
__device__ __forceinline__ unsigned slot_of(const unsigned* __restrict__ roots, unsigned nc, unsigned label) {
    unsigned lo = 0u, hi = nc;  // roots[lo] <= label < roots[hi] once lo's holds
    while (hi - lo > 1u) {
        const unsigned mid = (lo + hi) >> 1;
        if (roots[mid] <= label) lo = mid;
        else hi = mid;
    }
    return nc != 0u && roots[lo] == label ? lo : kNone;
}

// atomicMin / atomicMax of a bound that only ever moves one way: a value that does not move what is there now never will
__device__ __forceinline__ void lower(int* p, int v) {
    if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, v);
}
__device__ __forceinline__ void raise(int* p, int v) {
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}

// one part of a cluster's statistics: count voxels with coordinate sums sx, sy, sz inside [x0, x1] x [y0, y1] x [z0, z1]
__device__ __forceinline__ void add_part(const FrArgs& a, unsigned nc, unsigned label, unsigned count,
                                         unsigned long long sx, unsigned long long sy, unsigned long long sz, int x0,
                                         int x1, int y0, int y1, int z0, int z1) {
    const unsigned slot = slot_of(a.roots, nc, label);
    if (slot == kNone) return;
    const size_t s = slot;
    atomicAdd(a.count + s, count);
    atomicAdd(a.sums + 3 * s, sx);
    atomicAdd(a.sums + 3 * s + 1, sy);
    atomicAdd(a.sums + 3 * s + 2, sz);
    lower(a.box + 6 * s, x0);
    lower(a.box + 6 * s + 1, y0);
    lower(a.box + 6 * s + 2, z0);
    raise(a.box + 6 * s + 3, x1);
    raise(a.box + 6 * s + 4, y1);
    raise(a.box + 6 * s + 5, z1);
}

constexpr int kStatRows = 16;  // rows, one wave each, of a workgroup of k_fr_stats

// Statistics.  On a real scene nearly every frontier voxel belongs to one giant cluster, and a set of atomics per run
// would serialise on its slot.  A wave keeps ONE pending part while the chunks of its row hold one label each and the
// same one (wave-uniform: count by popcount, sum of x by one wave reduction); a chunk with several labels adds its runs
// one by one, as does a pending part another label displaces.  At the row's end the workgroup's waves merge their
// pending parts by label through LDS: one set of atomics per label and workgroup of 16 rows.
__global__ __launch_bounds__(64 * kStatRows) void k_fr_stats(const FrArgs a, const unsigned* __restrict__ labels) {
    __shared__ unsigned sLabel[kStatRows], sCount[kStatRows], sSx[kStatRows];
    __shared__ int sX0[kStatRows], sX1[kStatRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t rows = static_cast<size_t>(a.ny) * a.nz;
    const size_t row0 = static_cast<size_t>(blockIdx.x) * kStatRows, row = row0 + wave;
    const unsigned nc = min(a.nc, a.bsums[a.blocks]);  // the slots k_fr_roots did fill
    unsigned pLabel = kNone, pCount = 0u, pSx = 0u;  // the pending part: wave-uniform
    int pX0 = INT_MAX, pX1 = -1;
    if (row < rows) {  // wave-uniform
        const int z = static_cast<int>(row / a.ny), y = static_cast<int>(row - static_cast<size_t>(z) * a.ny);
        const unsigned base = static_cast<unsigned>(row * a.nx);
        const int chunks = (a.nx + 63) >> 6;
        for (int k = 0; k < chunks; ++k) {
            const int x = 64 * k + lane;
            const unsigned label = x < a.nx ? labels[base + x] : kNone;
            const bool live = label != kNone;
            const unsigned long long liveMask = __ballot(live);
            if (liveMask == 0ull) continue;  // wave-uniform
            const int firstLane = __ffsll(static_cast<long long>(liveMask)) - 1;
            const unsigned first = __shfl(label, firstLane);
            const bool uniform = __all(!live || label == first);
            if (pLabel != kNone && (!uniform || first != pLabel)) {  // displaced
                if (lane == 0)
                    add_part(a, nc, pLabel, pCount, pSx, static_cast<unsigned long long>(pCount) * y,
                             static_cast<unsigned long long>(pCount) * z, pX0, pX1, y, y, z, z);
                pLabel = kNone;
                pCount = pSx = 0u;
                pX0 = INT_MAX;
                pX1 = -1;
            }
            if (uniform) {
                unsigned sum = live ? static_cast<unsigned>(x) : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
                pLabel = first;
                pCount += static_cast<unsigned>(__popcll(liveMask));
                pSx += sum;
                pX0 = min(pX0, 64 * k + firstLane);
                pX1 = max(pX1, 64 * k + 63 - __clzll(static_cast<long long>(liveMask)));
            } else {  // run by run: consecutive x, so count, sum and box follow from the first x and the length
                const unsigned before = __shfl_up(label, 1);
                const bool cont = live && lane > 0 && before == label;  // goes on the run of the lane before
                const unsigned long long contMask = __ballot(cont);
                if (live && !cont) {
                    const unsigned long long after = lane == 63 ? 0ull : contMask >> (lane + 1);
                    const unsigned len = 1u + static_cast<unsigned>(__ffsll(static_cast<long long>(~after)) - 1);
                    add_part(a, nc, label, len, static_cast<unsigned long long>(len) * x + len * (len - 1u) / 2u,
                             static_cast<unsigned long long>(len) * y, static_cast<unsigned long long>(len) * z, x,
                             x + static_cast<int>(len) - 1, y, y, z, z);
                }
            }
        }
    }
    if (lane == 0) {
        sLabel[wave] = pLabel;
        sCount[wave] = pCount;
        sSx[wave] = pSx;
        sX0[wave] = pX0;
        sX1[wave] = pX1;
    }
    __syncthreads();
    if (lane != 0 || pLabel == kNone) return;
    for (int u = 0; u < wave; ++u)
        if (sLabel[u] == pLabel) return;  // an earlier wave adds this label for the workgroup
    unsigned count = 0u;
    unsigned long long sx = 0ull, sy = 0ull, sz = 0ull;
    int x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1, z0 = INT_MAX, z1 = -1;
    for (int u = wave; u < kStatRows; ++u) {
        if (sLabel[u] != pLabel) continue;
        const size_t r = row0 + u;  // < rows: the wave had a part
        const int z = static_cast<int>(r / a.ny), y = static_cast<int>(r - static_cast<size_t>(z) * a.ny);
        count += sCount[u];
        sx += sSx[u];
        sy += static_cast<unsigned long long>(sCount[u]) * y;
        sz += static_cast<unsigned long long>(sCount[u]) * z;
        x0 = min(x0, sX0[u]);
        x1 = max(x1, sX1[u]);
        y0 = min(y0, y);
        y1 = max(y1, y);
        z0 = min(z0, z);
        z1 = max(z1, z);
    }
    add_part(a, nc, pLabel, count, sx, sy, sz, x0, x1, y0, y1, z0, z1);
}

// Representative.  One wave per row; the first lane of a run finds the slot and computes the rounded centroid from the
// finished sums (three 64-bit divisions per run, not per voxel) and hands both to the run's lanes.
__global__ __launch_bounds__(256) void k_fr_rep(const FrArgs a, const unsigned* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const size_t rows = static_cast<size_t>(a.ny) * a.nz;
    const size_t row = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // whole waves leave
    const int z = static_cast<int>(row / a.ny), y = static_cast<int>(row - static_cast<size_t>(z) * a.ny);
    const unsigned base = static_cast<unsigned>(row * a.nx);
    const unsigned nc = min(a.nc, a.bsums[a.blocks]);  // the slots k_fr_roots did fill
    const int chunks = (a.nx + 63) >> 6;
    for (int k = 0; k < chunks; ++k) {
        const int x = 64 * k + lane;
        const unsigned label = x < a.nx ? labels[base + x] : kNone;
        const bool live = label != kNone;
        const unsigned before = __shfl_up(label, 1);
        const bool cont = live && lane > 0 && before == label;  // goes on the run of the lane before
        const unsigned long long headMask = __ballot(live && !cont);
        if (headMask == 0ull) continue;  // wave-uniform
        unsigned slot = kNone;
        int cx = 0, cy = 0, cz = 0;
        if (live && !cont) {
            slot = slot_of(a.roots, nc, label);
            if (slot != kNone) {
                const size_t s = slot;
                const unsigned long long cnt = a.count[s];
                if (cnt != 0ull) {  // (always: this run is part of it)
                    cx = static_cast<int>((2ull * a.sums[3 * s] + cnt) / (2ull * cnt));
                    cy = static_cast<int>((2ull * a.sums[3 * s + 1] + cnt) / (2ull * cnt));
                    cz = static_cast<int>((2ull * a.sums[3 * s + 2] + cnt) / (2ull * cnt));
                }
            }
        }
        // the first lane of this lane's run: the highest head at or below it
        const unsigned long long below = headMask & (~0ull >> (63 - lane));
        const int head = below ? 63 - __clzll(static_cast<long long>(below)) : 0;
        slot = __shfl(slot, head);
        cx = __shfl(cx, head);
        cy = __shfl(cy, head);
        cz = __shfl(cz, head);
        if (live && slot != kNone) {
            const int dx = x - cx, dy = y - cy, dz = z - cz;
            const unsigned long long key = (static_cast<unsigned long long>(dx * dx + dy * dy + dz * dz) << 31) | (base + x);
            // the key only ever decreases: one that is not below what is there now can never win
            if (key < __hip_atomic_load(a.key + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(a.key + slot, key);
        }
    }
}

__device__ __forceinline__ unsigned keep_flag(const FrArgs& a, unsigned nc, unsigned s, unsigned minVoxels) {
    return s < nc && a.count[s] >= minVoxels ? 1u : 0u;
}

__global__ __launch_bounds__(kFrBlock) void k_fr_keepsums(const FrArgs a, unsigned minVoxels) {
    __shared__ unsigned lds[kFrBlock / 64];
    const unsigned nc = min(a.nc, a.bsums[a.blocks]);
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(keep_flag(a, nc, blockIdx.x * kFrBlock + threadIdx.x, minVoxels), total, lds);
    if (threadIdx.x == 0) a.csums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kFrBlock) void k_fr_emit(const FrArgs a, unsigned minVoxels,
                                                      emf_frontier_cluster_t* __restrict__ records, unsigned capacity,
                                                      unsigned* kept) {
    __shared__ unsigned lds[kFrBlock / 64];
    const unsigned nc = min(a.nc, a.bsums[a.blocks]);
    const unsigned s = blockIdx.x * kFrBlock + threadIdx.x;
    const unsigned flag = keep_flag(a, nc, s, minVoxels);
    unsigned total;
    const unsigned rank = a.csums[blockIdx.x] + block_exclusive_scan<kScanBlock / 64>(flag, total, lds);
    if (s == 0u) *kept = a.csums[a.cblocks];
    if (!flag || rank >= capacity) return;
    emf_frontier_cluster_t r;
    r.label = static_cast<int32_t>(a.roots[s]);
    r.count = static_cast<int32_t>(a.count[s]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        r.lo[j] = a.box[6 * static_cast<size_t>(s) + j];
        r.hi[j] = a.box[6 * static_cast<size_t>(s) + 3 + j];
        r.sum[j] = a.sums[3 * static_cast<size_t>(s) + j];
    }
    const unsigned lin = static_cast<unsigned>(a.key[s] & 0x7fffffffull), plane = static_cast<unsigned>(a.nx) * a.ny;
    const unsigned rem = lin % plane;
    r.rep[0] = static_cast<int32_t>(rem % a.nx);
    r.rep[1] = static_cast<int32_t>(rem / a.nx);
    r.rep[2] = static_cast<int32_t>(lin / plane);
    r.reserved = 0;
    records[rank] = r;
}

int check_size(const int32_t size[3], const char* what) {
    if (!size) return fail(EMF_E_ARG, "%s: size is NULL", what);
    for (int i = 0; i < 3; ++i) {
        if (size[i] < 1) return fail(EMF_E_ARG, "%s: box axis %d has %d voxels", what, i, size[i]);
        if (size[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "%s: box axis %d has %d voxels, above %d", what, i, size[i], EMF_DF_MAX_AXIS);
    }
    const unsigned long long voxels = static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]);
    if (voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "%s: a box of %llu voxels, above 2^31 - 1", what, voxels);
    return EMF_OK;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_frontierLabel(const uint8_t* classes, const int32_t size[3], const int32_t* d2, int32_t min_d2,
                          int32_t* labels, uint32_t* counters, emf_stream_t stream) {
    if (!classes || !labels || !counters) return fail(EMF_E_ARG, "frontierLabel: classes, labels or counters is NULL");
    EMF_TRY(check_size(size, "frontierLabel"));
    if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(d2) | reinterpret_cast<uintptr_t>(counters)) & 3u)
        return fail(EMF_E_ARG, "frontierLabel: misaligned arrays");
    const int nx = size[0], ny = size[1], nz = size[2];
    const size_t rows = static_cast<size_t>(ny) * nz;
    const unsigned n = static_cast<unsigned>(rows * nx), blocks = ceil_div(n, kFrBlock);
    const hipStream_t s = as_stream(stream);
    unsigned* parent = reinterpret_cast<unsigned*>(labels);
    EMF_TRY(memset_async(counters, 0, 3 * sizeof(uint32_t), stream, "frontierLabel"));
    hipLaunchKernelGGL(k_fr_flags, dim3(ceil_div(rows, 4)), dim3(256), 0, s, classes, d2, min_d2, parent,
                       counters + EMF_FRONTIER_VOXELS, nx, ny, nz);
    hipLaunchKernelGGL(k_fr_hook, dim3(blocks), dim3(kFrBlock), 0, s, parent, nx, ny, nz);
    hipLaunchKernelGGL(k_fr_flatten, dim3(blocks), dim3(kFrBlock), 0, s, parent, n);
    hipLaunchKernelGGL(k_fr_count, dim3(blocks), dim3(kFrBlock), 0, s, parent, n, counters + EMF_FRONTIER_CLUSTERS);
    return launch_status("frontierLabel");
}

size_t emf_hip_frontierScratchBytes(const int32_t size[3], uint32_t n_clusters) {
    if (!size) return 0;
    for (int i = 0; i < 3; ++i)
        if (size[i] < 1 || size[i] > EMF_DF_MAX_AXIS) return 0;
    if (static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]) > 0x7fffffffull) return 0;
    FrArgs a;
    char origin[16];
    (void)origin;
    return place(a, size, n_clusters, origin);  // only the offsets are used
}

int emf_hip_frontierClusters(const int32_t* labels, const int32_t size[3], int32_t min_voxels, uint32_t n_clusters,
                             void* scratch_dev, emf_frontier_cluster_t* records, int32_t capacity, uint32_t* counters,
                             emf_stream_t stream) {
    if (!labels || !counters) return fail(EMF_E_ARG, "frontierClusters: labels or counters is NULL");
    EMF_TRY(check_size(size, "frontierClusters"));
    if (min_voxels < 1) return fail(EMF_E_ARG, "frontierClusters: min_voxels %d", min_voxels);
    if (capacity < 0) return fail(EMF_E_ARG, "frontierClusters: capacity %d", capacity);
    if (capacity > 0 && !records) return fail(EMF_E_ARG, "frontierClusters: records is NULL with capacity %d", capacity);
    const unsigned long long voxels = static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]);
    if (n_clusters > voxels) return fail(EMF_E_ARG, "frontierClusters: %u clusters in %llu voxels", n_clusters, voxels);
    if (n_clusters && !scratch_dev) return fail(EMF_E_ARG, "frontierClusters: scratch is NULL");
    if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(counters)) & 3u ||
        (reinterpret_cast<uintptr_t>(scratch_dev) & 15u) || (reinterpret_cast<uintptr_t>(records) & 7u))
        return fail(EMF_E_ARG, "frontierClusters: misaligned arrays");
    const hipStream_t s = as_stream(stream);
    if (n_clusters == 0) return memset_async(counters + EMF_FRONTIER_KEPT, 0, sizeof(uint32_t), stream, "frontierClusters");
    FrArgs a;
    place(a, size, n_clusters, scratch_dev);
    const unsigned* parent = reinterpret_cast<const unsigned*>(labels);
    const size_t rows = static_cast<size_t>(size[1]) * size[2];
    const unsigned minVoxels = static_cast<unsigned>(min_voxels);
    hipLaunchKernelGGL(k_fr_rootsums, dim3(a.blocks), dim3(kFrBlock), 0, s, a, parent);
    hipLaunchKernelGGL(k_fr_scan, dim3(1), dim3(kSumsBlock), 0, s, a.bsums, a.blocks);
    hipLaunchKernelGGL(k_fr_roots, dim3(a.blocks), dim3(kFrBlock), 0, s, a, parent);
    hipLaunchKernelGGL(k_fr_stats, dim3(ceil_div(rows, kStatRows)), dim3(64 * kStatRows), 0, s, a, parent);
    hipLaunchKernelGGL(k_fr_rep, dim3(ceil_div(rows, 4)), dim3(256), 0, s, a, parent);
    hipLaunchKernelGGL(k_fr_keepsums, dim3(a.cblocks), dim3(kFrBlock), 0, s, a, minVoxels);
    hipLaunchKernelGGL(k_fr_scan, dim3(1), dim3(kSumsBlock), 0, s, a.csums, a.cblocks);
    hipLaunchKernelGGL(k_fr_emit, dim3(a.cblocks), dim3(kFrBlock), 0, s, a, minVoxels, records,
                       static_cast<unsigned>(capacity), counters + EMF_FRONTIER_KEPT);
    return launch_status("frontierClusters");
}

}  // extern "C"
