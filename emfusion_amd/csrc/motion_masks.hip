// motion_masks.hip -- instance proposals from geometry: connected regions of pixels measured in front of the
// background's own raycast (include/emf_hip.h "Motion masks").
//
// Everything is per-frame image work over n = w * h pixels, linear index i = y * w + x.  The scratch is
//   [m: f32 x n][parent: u32 x n][area: u32 x n][roots: u32 x n][candA: u8 x n][candB: u8 x n]
//   [sums: u32 x (blocks + 1)]
//   k_mm_candidates  m[i] = |p|, cand[i], parent[i] = i, area[i] = 0                       (stage 1 + the labels' init)
//   k_mm_erode       one 3 x 3 erosion pass candA <-> candB through a 32 x 8 LDS tile with a one-pixel halo; what
//                    lies outside the image loads as 0, lanes outside it store nothing           (stage 2, x erode)
//   k_mm_hook        per candidate pixel: unite with its right and its lower neighbour if that is a candidate
//                    and the ray lengths differ by no more than `continuity` (union_find.hpp)          (stage 3)
//   k_mm_flatten     parent[i] := root of i.  A root is the minimum index of its tree
//   k_mm_count       area[root] += 1 per candidate: a wave whose live lanes share one root adds its lane count
//                    once, the workgroup's uniform waves are merged through LDS (as k_cc_count)        (stage 4)
//   k_mm_flags       roots with area >= min_pixels, summed per workgroup
//   k_mm_scan        one workgroup: the exclusive scan of the sums (wave_ops.hpp)
//   k_mm_compact     roots[rank] = i for every such root: index order, placed by scan, never by atomics
//   k_mm_select      one workgroup: max_masks rounds of "the largest key (area << 32 | ~label) below the last one"
//                    over the compacted roots; writes count and info (boxes empty)
//   k_mm_emit        labels, the mask planes (all max_masks of them, so unused planes come back zero) and the
//                    boxes: min / max in LDS per workgroup, then one global atomic per touched corner   (stage 5)
// No index leaves [0, n): the neighbours of the hook are tested against w and h, the tile's halo against the image,
// ranks are below the scanned total <= n, and a proposal's rank is below max_masks <= EMF_MOTION_MAX_MASKS.
#include "common.hpp"
#include "wave_ops.hpp"
#include "union_find.hpp"

#include <climits>

namespace emf_hip {
namespace {

constexpr int kMmBlock = kScanBlock;
constexpr int kTileW = 32, kTileH = 8;  // kTileW * kTileH == kMmBlock
static_assert(kTileW * kTileH == kMmBlock, "one lane per tile pixel");

struct MmArgs {
    float* m;
    unsigned* parent;
    unsigned* area;
    unsigned* roots;
    uint8_t* candA;
    uint8_t* candB;
    unsigned* sums;  // blocks + 1
    unsigned n, blocks;
    int w, h;
};

inline size_t place(MmArgs& a, int w, int h, void* scratch) {
    const size_t n = static_cast<size_t>(w) * static_cast<size_t>(h);
    a.w = w;
    a.h = h;
    a.n = static_cast<unsigned>(n);
    a.blocks = ceil_div(n, kMmBlock);
    ScratchArena s{static_cast<char*>(scratch), 0};
    a.m = s.take<float>(n);
    a.parent = s.take<unsigned>(n);
    a.area = s.take<unsigned>(n);
    a.roots = s.take<unsigned>(n);
    a.candA = s.take<uint8_t>(n);
    a.candB = s.take<uint8_t>(n);
    a.sums = s.take<unsigned>(a.blocks + 1);
    return s.off;
}

__global__ __launch_bounds__(kMmBlock) void k_mm_candidates(const MmArgs a, const float* __restrict__ points,
                                                            const float* __restrict__ bg, float band) {
    const unsigned i = blockIdx.x * kMmBlock + threadIdx.x;
    if (i >= a.n) return;
    const float* p = points + 3 * static_cast<size_t>(i);
    const float m = norm(v3(p[0], p[1], p[2]));
    const float b = bg[i];
    a.m[i] = m;
    a.candA[i] = (p[2] > 0.f && b > 0.f && b - m > band) ? 1 : 0;
    a.parent[i] = i;
    a.area[i] = 0u;
}

__global__ __launch_bounds__(kMmBlock) void k_mm_erode(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int w,
                                                       int h) {
    __shared__ uint8_t tile[kTileH + 2][kTileW + 2];
    const int x0 = static_cast<int>(blockIdx.x) * kTileW, y0 = static_cast<int>(blockIdx.y) * kTileH;
    for (int k = threadIdx.x; k < (kTileH + 2) * (kTileW + 2); k += kMmBlock) {
        const int ty = k / (kTileW + 2), tx = k - ty * (kTileW + 2);
        const int gx = x0 + tx - 1, gy = y0 + ty - 1;
        const bool inside = gx >= 0 && gx < w && gy >= 0 && gy < h;
        tile[ty][tx] = inside ? in[static_cast<size_t>(gy) * w + gx] : 0;
    }
    __syncthreads();
    const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) return;
    unsigned all = 1u;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) all &= tile[ty + dy][tx + dx];
    out[static_cast<size_t>(y) * w + x] = static_cast<uint8_t>(all);
}

__device__ __forceinline__ bool joins(float ma, float mb, float continuity) { return fabsf(ma - mb) <= continuity; }

__global__ __launch_bounds__(kMmBlock) void k_mm_hook(const MmArgs a, const uint8_t* __restrict__ cand, float continuity) {
    const unsigned i = blockIdx.x * kMmBlock + threadIdx.x;
    if (i >= a.n || !cand[i]) return;
    const unsigned w = static_cast<unsigned>(a.w);
    const unsigned x = i % w, y = i / w;
    const float m = a.m[i];
    if (x + 1 < w && cand[i + 1] && joins(m, a.m[i + 1], continuity)) unite(a.parent, i, i + 1);
    if (y + 1 < static_cast<unsigned>(a.h) && cand[i + w] && joins(m, a.m[i + w], continuity)) unite(a.parent, i, i + w);
}

__global__ __launch_bounds__(kMmBlock) void k_mm_flatten(const MmArgs a, const uint8_t* __restrict__ cand) {
    const unsigned i = blockIdx.x * kMmBlock + threadIdx.x;
    if (i >= a.n || !cand[i]) return;
    const unsigned r = find_root(a.parent, i);
    atomicMin(a.parent + i, r);  // (a halving step of another lane may still be under way: the minimum wins)
}

// One large region would serialise one add per pixel on one address.  A wave whose live lanes share a root adds
// once; the workgroup's uniform waves are merged in LDS.
__global__ __launch_bounds__(kMmBlock) void k_mm_count(const MmArgs a, const uint8_t* __restrict__ cand) {
    __shared__ unsigned wroot[kMmBlock / 64], wcount[kMmBlock / 64];
    const unsigned i = blockIdx.x * kMmBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = i < a.n && cand[i];
    const unsigned root = live ? a.parent[i] : 0u;
    const unsigned long long mask = __ballot(live);
    unsigned uroot = 0u, ucount = 0u;
    if (mask) {
        const unsigned first = __shfl(root, __ffsll(static_cast<long long>(mask)) - 1);
        if (__all(!live || root == first)) {
            uroot = first;
            ucount = static_cast<unsigned>(__popcll(mask));
        } else if (live) {
            atomicAdd(a.area + root, 1u);
        }
    }
    if (lane == 0) {
        wroot[wave] = uroot;
        wcount[wave] = ucount;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kMmBlock / 64; ++w) {
            unsigned c = wcount[w];
            if (c == 0u) continue;
            for (int u = w + 1; u < kMmBlock / 64; ++u)
                if (wcount[u] && wroot[u] == wroot[w]) {
                    c += wcount[u];
                    wcount[u] = 0u;
                }
            atomicAdd(a.area + wroot[w], c);
        }
    }
}

// a root of at least minPixels pixels
__device__ __forceinline__ unsigned root_flag(const MmArgs& a, const uint8_t* cand, unsigned i, unsigned minPixels) {
    if (i >= a.n || !cand[i] || a.parent[i] != i) return 0u;
    return a.area[i] >= minPixels ? 1u : 0u;
}

__global__ __launch_bounds__(kMmBlock) void k_mm_flags(const MmArgs a, const uint8_t* __restrict__ cand,
                                                       unsigned minPixels) {
    __shared__ unsigned lds[kMmBlock / 64];
    const unsigned i = blockIdx.x * kMmBlock + threadIdx.x;
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(root_flag(a, cand, i, minPixels), total, lds);
    if (threadIdx.x == 0) a.sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSumsBlock) void k_mm_scan(const MmArgs a) {
    __shared__ unsigned lds[kSumsBlock / 64];
    const unsigned total = scan_sums(a.sums, 0u, a.blocks, lds);
    if (threadIdx.x == 0) a.sums[a.blocks] = total;
}

__global__ __launch_bounds__(kMmBlock) void k_mm_compact(const MmArgs a, const uint8_t* __restrict__ cand,
                                                         unsigned minPixels) {
    __shared__ unsigned lds[kMmBlock / 64];
    const unsigned i = blockIdx.x * kMmBlock + threadIdx.x;
    const unsigned f = root_flag(a, cand, i, minPixels);
    unsigned total;
    const unsigned mine = block_exclusive_scan<kScanBlock / 64>(f, total, lds);
    if (f) a.roots[a.sums[blockIdx.x] + mine] = i;  // < sums[blocks] <= n
}

__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor(static_cast<unsigned>(v >> 32), o);
        const unsigned lo = __shfl_xor(static_cast<unsigned>(v), o);
        const unsigned long long other = static_cast<unsigned long long>(hi) << 32 | lo;
        v = other > v ? other : v;
    }
    return v;
}

// One workgroup.  Keys are distinct (the labels are), so round r's winner is the largest key strictly below round
// r - 1's: no marking, no dependence on the order of anything.  A key is never 0 (area >= 1).
__global__ __launch_bounds__(kSumsBlock) void k_mm_select(const MmArgs a, int maxMasks, emf_motion_info_t* info,
                                                          int32_t* count) {
    __shared__ unsigned long long wbest[kSumsBlock / 64];
    __shared__ unsigned long long winner;
    const unsigned k = a.sums[a.blocks];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long prev = ~0ull;
    int found = 0;
    for (int r = 0; r < maxMasks; ++r) {
        unsigned long long best = 0ull;
        for (unsigned j = threadIdx.x; j < k; j += kSumsBlock) {
            const unsigned root = a.roots[j];
            const unsigned long long key = static_cast<unsigned long long>(a.area[root]) << 32 | static_cast<unsigned>(~root);
            if (key < prev && key > best) best = key;
        }
        best = wave_max64(best);
        if (lane == 0) wbest[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long v = 0ull;
            for (int w = 0; w < kSumsBlock / 64; ++w) v = wbest[w] > v ? wbest[w] : v;
            winner = v;
            emf_motion_info_t e{0, 0, 0, 0, 0, 0};
            if (v) {
                e.label = static_cast<int32_t>(~static_cast<unsigned>(v));
                e.area = static_cast<int32_t>(v >> 32);
                e.x0 = e.y0 = INT_MAX;
                e.x1 = e.y1 = -1;
            }
            info[r] = e;
        }
        __syncthreads();
        prev = winner;
        if (prev == 0ull) {  // no component left: the remaining entries are zeroed, no round can find one
            if (threadIdx.x == 0)
                for (int q = r + 1; q < maxMasks; ++q) info[q] = emf_motion_info_t{0, 0, 0, 0, 0, 0};
            break;
        }
        ++found;
    }
    if (threadIdx.x == 0) *count = found;
}

__global__ __launch_bounds__(kMmBlock) void k_mm_emit(const MmArgs a, const uint8_t* __restrict__ cand, int maxMasks,
                                                      emf_motion_info_t* info, const int32_t* __restrict__ count,
                                                      int32_t* __restrict__ labels, uint8_t* __restrict__ masks) {
    __shared__ int sel[EMF_MOTION_MAX_MASKS];
    __shared__ int box[EMF_MOTION_MAX_MASKS][4];
    const int found = *count;  // <= maxMasks <= EMF_MOTION_MAX_MASKS
    if (threadIdx.x < EMF_MOTION_MAX_MASKS) {
        const int r = threadIdx.x;
        sel[r] = r < found ? info[r].label : -1;
        box[r][0] = box[r][1] = INT_MAX;
        box[r][2] = box[r][3] = -1;
    }
    __syncthreads();
    const unsigned i = blockIdx.x * kMmBlock + threadIdx.x;
    int rank = -1;
    if (i < a.n) {
        if (cand[i]) {
            const int root = static_cast<int>(a.parent[i]);
            for (int r = 0; r < found; ++r)
                if (sel[r] == root) rank = r;
        }
        labels[i] = rank;
        for (int r = 0; r < maxMasks; ++r) masks[static_cast<size_t>(r) * a.n + i] = r == rank ? 1 : 0;
        if (rank >= 0) {
            const int x = static_cast<int>(i % static_cast<unsigned>(a.w)), y = static_cast<int>(i / static_cast<unsigned>(a.w));
            atomicMin(&box[rank][0], x);
            atomicMin(&box[rank][1], y);
            atomicMax(&box[rank][2], x);
            atomicMax(&box[rank][3], y);
        }
    }
    __syncthreads();
    if (threadIdx.x < static_cast<unsigned>(found) && box[threadIdx.x][2] >= 0) {
        emf_motion_info_t* e = info + threadIdx.x;
        atomicMin(&e->x0, box[threadIdx.x][0]);
        atomicMin(&e->y0, box[threadIdx.x][1]);
        atomicMax(&e->x1, box[threadIdx.x][2]);
        atomicMax(&e->y1, box[threadIdx.x][3]);
    }
}

bool sizes_ok(int w, int h, int maxMasks) {
    return w >= 1 && h >= 1 && static_cast<unsigned long long>(w) * static_cast<unsigned long long>(h) <= (1ull << 30) &&
           maxMasks >= 1 && maxMasks <= EMF_MOTION_MAX_MASKS;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

size_t emf_hip_motionMasksScratchBytes(int w, int h, int max_masks) {
    if (!sizes_ok(w, h, max_masks)) return 0;
    MmArgs a;
    char origin[16];
    (void)origin;
    return place(a, w, h, origin);  // only the offsets are used
}

int emf_hip_motionMasks(const float* points, const float* bg_raylengths, int w, int h, const emf_motion_params_t* params,
                        void* scratch_dev, int32_t* labels, uint8_t* masks, emf_motion_info_t* info, int32_t* count,
                        emf_stream_t stream) {
    if (!points || !bg_raylengths || !params || !scratch_dev || !labels || !masks || !info || !count)
        return fail(EMF_E_ARG, "motionMasks: %s is NULL",
                    !points ? "points" : !bg_raylengths ? "bg_raylengths" : !params ? "params" : !scratch_dev ? "scratch_dev"
                    : !labels ? "labels" : !masks ? "masks" : !info ? "info" : "count");
    const emf_motion_params_t p = *params;
    if (p.max_masks < 1 || p.max_masks > EMF_MOTION_MAX_MASKS)
        return fail(EMF_E_ARG, "motionMasks: max_masks %d (1 .. %d)", p.max_masks, EMF_MOTION_MAX_MASKS);
    if (!sizes_ok(w, h, p.max_masks)) return fail(EMF_E_ARG, "motionMasks: %d x %d pixels (at least 1 x 1, at most 2^30)", w, h);
    if (p.erode < 0 || p.erode > 3) return fail(EMF_E_ARG, "motionMasks: erode %d (0 .. 3)", p.erode);
    if (p.min_pixels < 0) return fail(EMF_E_ARG, "motionMasks: min_pixels %d (>= 0)", p.min_pixels);
    if (!(p.band >= 0.f) || !(p.continuity >= 0.f))
        return fail(EMF_E_ARG, "motionMasks: band %g / continuity %g (both >= 0)", static_cast<double>(p.band),
                    static_cast<double>(p.continuity));
    MmArgs a;
    place(a, w, h, scratch_dev);
    const hipStream_t s = as_stream(stream);
    const dim3 block(kMmBlock), grid(a.blocks);
    hipLaunchKernelGGL(k_mm_candidates, grid, block, 0, s, a, points, bg_raylengths, p.band);
    const uint8_t* cand = a.candA;
    for (int e = 0; e < p.erode; ++e) {
        uint8_t* out = cand == a.candA ? a.candB : a.candA;
        hipLaunchKernelGGL(k_mm_erode, dim3(ceil_div(w, kTileW), ceil_div(h, kTileH)), block, 0, s, cand, out, w, h);
        cand = out;
    }
    const unsigned minPixels = static_cast<unsigned>(p.min_pixels);
    hipLaunchKernelGGL(k_mm_hook, grid, block, 0, s, a, cand, p.continuity);
    hipLaunchKernelGGL(k_mm_flatten, grid, block, 0, s, a, cand);
    hipLaunchKernelGGL(k_mm_count, grid, block, 0, s, a, cand);
    hipLaunchKernelGGL(k_mm_flags, grid, block, 0, s, a, cand, minPixels);
    hipLaunchKernelGGL(k_mm_scan, dim3(1), dim3(kSumsBlock), 0, s, a);
    hipLaunchKernelGGL(k_mm_compact, grid, block, 0, s, a, cand, minPixels);
    hipLaunchKernelGGL(k_mm_select, dim3(1), dim3(kSumsBlock), 0, s, a, p.max_masks, info, count);
    hipLaunchKernelGGL(k_mm_emit, grid, block, 0, s, a, cand, p.max_masks, info, count, labels, masks);
    return launch_status("motionMasks");
}

}  // extern "C"
