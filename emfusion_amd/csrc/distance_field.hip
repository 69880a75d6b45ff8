// distance_field.hip -- occupancy classes of a box of a scene and the exact Euclidean distance transform over them
// (include/emf_hip.h "Distance field").
//
//   k_occ_classes  one wave per row of the box; a lane classifies four consecutive voxels from two 16-byte loads
//                  (rows that are 16-byte aligned in both arrays) or voxel by voxel, and stores four class bytes as
//                  one word where the destination allows.  Single float comparisons: FREE / OCCUPIED / UNKNOWN.
//   k_occ_stamp    blockIdx.y selects one of up to EMF_MAX_BATCH objects (passed by value), blockIdx.x a 64 x 4 x 1
//                  piece of that object's sub-box of the background lattice; one voxel per lane: background voxel ->
//                  object voxel (nearest, ties to even) -> one byte store of OCCUPIED where the object is solid.  All
//                  stores write the same value: no atomics, no dependence on order.
//   k_df_rows      pass x.  One wave per row: the site bits of 64 voxels are one __ballot, lane k keeps the ballot of
//                  chunk k (a row has at most 32 chunks), and the nearest site to the left and to the right of every
//                  voxel comes from bit scans on the chunk's mask, carried across chunks through the first / last
//                  site of the nearest non-empty chunk on either side.  No LDS; classes read once, dx^2 written once.
//   k_df_lines     passes y and z.  One workgroup per BUNDLE: the whole line length x C neighbouring columns (lanes
//                  along x, so every global row is coalesced), staged in LDS as int32 before anything is written --
//                  the pass runs in place.  Output i of a column scans outward, min over line[i +- d] + d^2, and
//                  stops as soon as d * d >= best: nothing farther can win, so the minimum is exact (with a cap, best
//                  starts at cap^2 + 1 at the latest: what lies beyond ends as "far" anyway).  A lane reads
//                  line[i +- d] at its own column: with C = 64 or 32 the 32 lanes that share an LDS cycle sit in 32
//                  different banks however they diverge in d.
//   nearest site    the NEAREST instantiations of the two kernels also carry the linear index of the
//                  winning site: pass x writes it next to dx^2 (on dl == dr the left site), passes y and z find the
//                  winning line element j -- the scan runs while d * d <= best and takes the lower side on equality, so
//                  every pass breaks ties toward the smaller coordinate, which is the smallest linear index overall --
//                  and copy index_in[column, j] from global memory into a second index buffer: the indices ping-pong
//                  between `nearest` and a scratch array, no pass reads an index array it writes, and LDS holds d2 only.
//   k_df_query     one lane per point: a gather of class, d2 and nearest site at box voxels.
// Integer arithmetic throughout (the metres output is one correctly rounded square root and one product per voxel).
#include "common.hpp"

#include <algorithm>
#include <cmath>

namespace emf_hip {
namespace {

constexpr int kFar = EMF_DF_FAR;
constexpr int kBig = 0x40000000;  // "no site" inside the LDS lines: kBig + d^2 never overflows (d <= 2047)
constexpr size_t kMaxBundleBytes = 128u << 10;  // of the CU's 160 KiB

static_assert(sizeof(emf_occ_object_t) == 112, "emf_occ_object_t is mirrored by emfusion_amd/_lib.py");

struct ClassArgs {
    const float* tsdf;
    const float* weights;
    uint8_t* out;
    I3 n, lo, size;
};

__device__ __forceinline__ unsigned occ_class(float t, float w) {
    return w > 0.f ? (t > 0.f ? EMF_OCC_FREE : EMF_OCC_OCCUPIED) : EMF_OCC_UNKNOWN;
}

__global__ __launch_bounds__(256) void k_occ_classes(const ClassArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const size_t row = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);  // z * size.y + y of the box
    if (row >= static_cast<size_t>(a.size.y) * a.size.z) return;
    const int z = static_cast<int>(row / a.size.y), y = static_cast<int>(row - static_cast<size_t>(z) * a.size.y);
    const size_t src = (static_cast<size_t>(a.lo.z + z) * a.n.y + (a.lo.y + y)) * a.n.x + a.lo.x;
    const float* __restrict__ t = a.tsdf + src;
    const float* __restrict__ w = a.weights + src;
    uint8_t* __restrict__ o = a.out + row * a.size.x;
    const bool vec = ((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(w)) & 15u) == 0;  // wave-uniform
    const bool word = (reinterpret_cast<uintptr_t>(o) & 3u) == 0;
    for (int x = 4 * static_cast<int>(lane); x < a.size.x; x += 256) {
        if (vec && x + 4 <= a.size.x) {
            const float4 tv = *reinterpret_cast<const float4*>(t + x), wv = *reinterpret_cast<const float4*>(w + x);
            const unsigned c0 = occ_class(tv.x, wv.x), c1 = occ_class(tv.y, wv.y), c2 = occ_class(tv.z, wv.z),
                           c3 = occ_class(tv.w, wv.w);
            if (word) {
                *reinterpret_cast<unsigned*>(o + x) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
            } else {
                o[x] = static_cast<uint8_t>(c0);
                o[x + 1] = static_cast<uint8_t>(c1);
                o[x + 2] = static_cast<uint8_t>(c2);
                o[x + 3] = static_cast<uint8_t>(c3);
            }
        } else {
            const int end = min(x + 4, a.size.x);
            for (int e = x; e < end; ++e) o[e] = static_cast<uint8_t>(occ_class(t[e], w[e]));
        }
    }
}

struct StampArgs {
    uint8_t* classes;
    I3 boxLo, boxSize;
    V3 half;  // of the background
    float voxel;
    emf_occ_object_t obj[EMF_MAX_BATCH];  // lo / size already clipped to the box
};

constexpr int kStampX = 64, kStampY = 4;

__global__ __launch_bounds__(kStampX * kStampY) void k_occ_stamp(const StampArgs a) {
    const emf_occ_object_t& o = a.obj[blockIdx.y];
    if (o.size[0] <= 0 || o.size[1] <= 0 || o.size[2] <= 0) return;
    const unsigned tx = (o.size[0] + kStampX - 1) / kStampX, ty = (o.size[1] + kStampY - 1) / kStampY;
    const unsigned b = blockIdx.x;  // block-uniform decode of the piece
    if (b >= tx * ty * static_cast<unsigned>(o.size[2])) return;
    const unsigned bz = b / (tx * ty), r = b - bz * tx * ty, by = r / tx, bx = r - by * tx;
    const int lx = bx * kStampX + (threadIdx.x & 63u), ly = by * kStampY + (threadIdx.x >> 6);
    if (lx >= o.size[0] || ly >= o.size[1]) return;
    const int x = o.lo[0] + lx, y = o.lo[1] + ly, z = o.lo[2] + static_cast<int>(bz);
    const V3 pb = v3((static_cast<float>(x) - a.half.x) * a.voxel, (static_cast<float>(y) - a.half.y) * a.voxel,
                     (static_cast<float>(z) - a.half.z) * a.voxel);
    const M33 R{{o.R[0], o.R[1], o.R[2]}, {o.R[3], o.R[4], o.R[5]}, {o.R[6], o.R[7], o.R[8]}};
    const V3 po = mul(R, pb) + v3(o.t[0], o.t[1], o.t[2]);
    const I3 n{o.res[0], o.res[1], o.res[2]};
    const V3 q = to_voxel(po, o.voxelSize, half_extent(n));
    if (!(q.x == q.x) || !(q.y == q.y) || !(q.z == q.z)) return;  // NaN: outside
    const int ix = __float2int_rn(q.x), iy = __float2int_rn(q.y), iz = __float2int_rn(q.z);  // saturating
    if (ix < 0 || ix >= n.x || iy < 0 || iy >= n.y || iz < 0 || iz >= n.z) return;
    const size_t i = (static_cast<size_t>(iz) * n.y + iy) * n.x + ix;
    if (!(o.weights[i] > 0.f)) return;
    if (o.fgVolMask && o.fgVolMask[i] == 0) return;
    if (o.tsdf[i] > 0.f) return;
    a.classes[(static_cast<size_t>(z - a.boxLo.z) * a.boxSize.y + (y - a.boxLo.y)) * a.boxSize.x + (x - a.boxLo.x)] =
        EMF_OCC_OCCUPIED;
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
    const unsigned lo = __shfl(static_cast<unsigned>(v), src), hi = __shfl(static_cast<unsigned>(v >> 32), src);
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// Pass x: d2 = (distance along the row to the nearest site of the row)^2, kFar for a row without a site.
// NEAREST: also idx = the linear index of that site (the left one where both sides are equally far), -1 without one.
template <bool NEAREST>
__global__ __launch_bounds__(256) void k_df_rows(const uint8_t* __restrict__ classes, int* __restrict__ d2,
                                                 int* __restrict__ idx, int nx, size_t rows, unsigned siteMask) {
    const int lane = threadIdx.x & 63;
    const size_t row = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // whole waves leave
    const uint8_t* c = classes + row * nx;
    int* o = d2 + row * nx;
    const int chunks = (nx + 63) >> 6;  // <= 32: lane k keeps chunk k
    unsigned long long mine = 0ull;
    for (int k = 0; k < chunks; ++k) {
        const int x = 64 * k + lane;
        bool site = false;
        if (x < nx) {
            const unsigned v = c[x];
            site = v < 3u && ((siteMask >> v) & 1u) != 0u;
        }
        const unsigned long long m = __ballot(site);
        if (lane == k) mine = m;
    }
    const int first = mine ? 64 * lane + __ffsll(static_cast<long long>(mine)) - 1 : -1;
    const int last = mine ? 64 * lane + 63 - __clzll(static_cast<long long>(mine)) : -1;
    const unsigned long long nonEmpty = __ballot(mine != 0ull);
    for (int k = 0; k < chunks; ++k) {  // k and everything derived from it alone is wave-uniform
        const unsigned long long m = shfl64(mine, k);
        const unsigned long long below = nonEmpty & ((1ull << k) - 1ull), above = nonEmpty & ~((2ull << k) - 1ull);
        const int prevLast = __shfl(last, below ? 63 - __clzll(static_cast<long long>(below)) : 0);
        const int nextFirst = __shfl(first, above ? __ffsll(static_cast<long long>(above)) - 1 : 0);
        const int x = 64 * k + lane;
        const unsigned long long ml = m & (~0ull >> (63 - lane)), mr = m & (~0ull << lane);
        int dl = -1, dr = -1;
        if (ml) dl = lane - (63 - __clzll(static_cast<long long>(ml)));
        else if (below) dl = x - prevLast;
        if (mr) dr = __ffsll(static_cast<long long>(mr)) - 1 - lane;
        else if (above) dr = nextFirst - x;
        const int d = dl < 0 ? dr : (dr < 0 ? dl : min(dl, dr));
        if (x < nx) o[x] = d < 0 ? kFar : d * d;
        if (NEAREST) {
            const int site = dl >= 0 && (dr < 0 || dl <= dr) ? x - dl : (dr >= 0 ? x + dr : -1);
            if (x < nx) idx[row * nx + x] = site < 0 ? EMF_DF_NONE : static_cast<int>(row * nx) + site;
        }
    }
}

// Passes y and z, in place.  Line element i of column x of bundle row blockIdx.y lives at
// d2[blockIdx.y * outerStride + i * lineStride + x]; C (a power of two) columns per workgroup.
// NEAREST: idxOut[v] = idxIn at the winning line element of v's column, -1 where d2 ends as kFar; idxIn != idxOut.
template <bool FINAL, bool NEAREST>
__global__ __launch_bounds__(1024) void k_df_lines(int* __restrict__ d2, float* __restrict__ metres,
                                                   const int* __restrict__ idxIn, int* __restrict__ idxOut, int n, int nx,
                                                   size_t lineStride, size_t outerStride, int logC, int cap2,
                                                   float voxel) {
    extern __shared__ int line[];
    const int C = 1 << logC;
    const int col = threadIdx.x & (C - 1), slot = threadIdx.x >> logC, slots = blockDim.x >> logC;
    const int x = blockIdx.x * C + col;
    const bool live = x < nx;
    const size_t base = static_cast<size_t>(blockIdx.y) * outerStride + x;
    for (int i = slot; i < n; i += slots) {
        const int v = live ? d2[base + i * lineStride] : kFar;
        line[(i << logC) + col] = v == kFar ? kBig : v;
    }
    __syncthreads();  // the bundle is staged whole: from here on its global copy may be overwritten
    if (!live) return;
    // With a cap, a distance above it ends as kFar whatever it is, and a distance within it is made of per-axis parts
    // within it: every pass may stop at cap^2 + 1, which keeps the scans short in wide free space.
    const int bound = cap2 > 0 ? cap2 + 1 : kBig;
    for (int i = slot; i < n; i += slots) {
        int best = min(line[(i << logC) + col], bound);
        int j = i;  // the winning line element (NEAREST)
        if (NEAREST) {
            // an element at distance exactly d with d * d == best ties the best so far: the scan goes on while
            // d * d <= best.  Every lo is below, every hi above all elements seen before it: lo wins on equality.
            for (int d = 1; d * d <= best; ++d) {
                const int lo = i - d, hi = i + d;
                if (lo < 0 && hi >= n) break;
                if (lo >= 0) {
                    const int v = line[(lo << logC) + col] + d * d;
                    if (v <= best) {
                        best = v;
                        j = lo;
                    }
                }
                if (hi < n) {
                    const int v = line[(hi << logC) + col] + d * d;
                    if (v < best) {
                        best = v;
                        j = hi;
                    }
                }
            }
        } else {
            for (int d = 1; d * d < best; ++d) {
                const int lo = i - d, hi = i + d;
                if (lo < 0 && hi >= n) break;
                if (lo >= 0) best = min(best, line[(lo << logC) + col] + d * d);
                if (hi < n) best = min(best, line[(hi << logC) + col] + d * d);
            }
        }
        const int out = best >= bound ? kFar : best;
        const size_t at = base + i * lineStride;
        if (NEAREST) idxOut[at] = out == kFar ? EMF_DF_NONE : idxIn[base + j * lineStride];
        if (FINAL) {
            if (metres) metres[at] = out == kFar ? __builtin_inff() : sqrtf(static_cast<float>(out)) * voxel;
        }
        d2[at] = out;
    }
}

int check_box_size(const int32_t size[3], const char* what) {
    for (int i = 0; i < 3; ++i) {
        if (size[i] < 1) return fail(EMF_E_ARG, "%s: box axis %d has %d voxels", what, i, size[i]);
        if (size[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "%s: box axis %d has %d voxels, above %d", what, i, size[i], EMF_DF_MAX_AXIS);
    }
    const unsigned long long voxels = static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]);
    if (voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "%s: a box of %llu voxels, above 2^31 - 1", what, voxels);
    return EMF_OK;
}

int check_box(const int32_t res[3], const int32_t lo[3], const int32_t size[3], const char* what) {
    if (!res || !lo || !size) return fail(EMF_E_ARG, "%s: res, box_lo or box_size is NULL", what);
    EMF_TRY(check_box_size(size, what));
    for (int i = 0; i < 3; ++i)
        if (res[i] < 1 || lo[i] < 0 || lo[i] > res[i] - size[i])
            return fail(EMF_E_ARG, "%s: the box [%d, %d + %d) leaves the volume's axis %d of %d voxels", what, lo[i], lo[i],
                        size[i], i, res[i]);
    const unsigned long long n = static_cast<unsigned long long>(res[0]) * res[1] * static_cast<unsigned long long>(res[2]);
    if (n > (1ull << 36)) return fail(EMF_E_LIMIT, "%s: volume of %llu voxels exceeds 2^36", what, n);
    return EMF_OK;
}

template <bool FINAL, bool NEAREST>
int launch_lines(int32_t* d2, float* metres, const int32_t* idxIn, int32_t* idxOut, int n, int nx, size_t lineStride,
                 size_t outerStride, int outer, int cap2, float voxel, hipStream_t stream) {
    // C = 64 up to 512 voxels per line, narrower so that a bundle stays within kMaxBundleBytes: 16 at 2048
    const int logC = n <= 512 ? 6 : (n <= 1024 ? 5 : 4);
    const int C = 1 << logC, perWave = 64 >> logC;  // lines of the bundle a wave covers at once
    int slots = std::min(std::max((n + 3) / 4, 1), 1024 / C);
    slots = std::min((slots + perWave - 1) / perWave * perWave, 1024 / C);  // whole waves
    const size_t lds = static_cast<size_t>(n) * C * sizeof(int);
    if (lds > kMaxBundleBytes) return fail(EMF_E_LIMIT, "distanceTransform: a line of %d voxels does not fit a bundle", n);
    if (lds > (48u << 10)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_df_lines<FINAL, NEAREST>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(static_cast<int>(e), "distanceTransform: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
        }
    }
    hipLaunchKernelGGL((k_df_lines<FINAL, NEAREST>), dim3(ceil_div(nx, C), outer), dim3(C * slots), lds, stream, d2, metres,
                       idxIn, idxOut, n, nx, lineStride, outerStride, logC, cap2, voxel);
    return launch_status("distanceTransform");
}

int check_transform(const char* what, const uint8_t* classes, const int32_t size[3], uint32_t site_mask, int32_t cap,
                    const int32_t* d2, const float* metres, float voxel_size) {
    if (!classes || !d2 || !size) return fail(EMF_E_ARG, "%s: classes, d2 or size is NULL", what);
    EMF_TRY(check_box_size(size, what));
    if (site_mask < 1u || site_mask > 7u) return fail(EMF_E_ARG, "%s: site_mask %u outside 1 .. 7", what, site_mask);
    if (cap < 0) return fail(EMF_E_ARG, "%s: cap %d", what, cap);
    if (metres && !(voxel_size > 0.f)) return fail(EMF_E_ARG, "%s: voxel_size %g", what, static_cast<double>(voxel_size));
    if ((reinterpret_cast<uintptr_t>(d2) | reinterpret_cast<uintptr_t>(metres)) & 3u)
        return fail(EMF_E_ARG, "%s: misaligned arrays", what);
    return EMF_OK;
}

// the three passes; NEAREST: the indices go x -> nearest, y -> scratch, z -> nearest
template <bool NEAREST>
int run_transform(const uint8_t* classes, const int32_t size[3], uint32_t site_mask, int32_t cap, int32_t* d2, float* metres,
                  int32_t* nearest, int32_t* scratch, float voxel_size, hipStream_t stream) {
    const int nx = size[0], ny = size[1], nz = size[2];
    // the largest distance of a box is below 3 * 2047^2: a cap at or above 4096 voxels caps nothing
    const int cap2 = cap > 0 && cap < 4096 ? cap * cap : 0;
    const size_t rows = static_cast<size_t>(ny) * nz, plane = static_cast<size_t>(nx) * ny;
    hipLaunchKernelGGL(k_df_rows<NEAREST>, dim3(ceil_div(rows, 4)), dim3(256), 0, stream, classes, d2, nearest, nx, rows,
                       site_mask);
    EMF_TRY(launch_status("distanceTransform"));
    EMF_TRY((launch_lines<false, NEAREST>(d2, nullptr, nearest, scratch, ny, nx, static_cast<size_t>(nx), plane, nz, cap2, 0.f,
                                          stream)));
    return launch_lines<true, NEAREST>(d2, metres, scratch, nearest, nz, nx, plane, static_cast<size_t>(nx), ny, cap2,
                                       voxel_size, stream);
}

struct QueryArgs {
    const uint8_t* classes;
    const int* d2;
    const int* nearest;
    const int* voxels;
    uint8_t* outClass;
    int* outD2;
    int* outNearest;
    I3 size;
    int n;
};

// one lane per point: plain loads and stores; a voxel outside the box reads as class 255, kFar, no site
__global__ __launch_bounds__(256) void k_df_query(const QueryArgs a) {
    const int i = static_cast<int>(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.n) return;
    const int x = a.voxels[3 * static_cast<size_t>(i)], y = a.voxels[3 * static_cast<size_t>(i) + 1],
              z = a.voxels[3 * static_cast<size_t>(i) + 2];
    const bool inside = x >= 0 && x < a.size.x && y >= 0 && y < a.size.y && z >= 0 && z < a.size.z;
    const size_t at = inside ? (static_cast<size_t>(z) * a.size.y + y) * a.size.x + x : 0;
    if (a.outClass) a.outClass[i] = inside ? a.classes[at] : static_cast<uint8_t>(255);
    if (a.outD2) a.outD2[i] = inside ? a.d2[at] : kFar;
    if (a.outNearest) a.outNearest[i] = inside ? a.nearest[at] : EMF_DF_NONE;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_occupancyClasses(const float* tsdf, const float* weights, const int32_t res[3], const int32_t box_lo[3],
                             const int32_t box_size[3], uint8_t* classes, emf_stream_t stream) {
    if (!tsdf || !weights || !classes) return fail(EMF_E_ARG, "occupancyClasses: tsdf, weights or classes is NULL");
    EMF_TRY(check_box(res, box_lo, box_size, "occupancyClasses"));
    if ((reinterpret_cast<uintptr_t>(tsdf) | reinterpret_cast<uintptr_t>(weights)) & 3u)
        return fail(EMF_E_ARG, "occupancyClasses: misaligned arrays");
    ClassArgs a{tsdf, weights, classes, i3_from(res), i3_from(box_lo), i3_from(box_size)};
    const size_t rows = static_cast<size_t>(box_size[1]) * box_size[2];
    hipLaunchKernelGGL(k_occ_classes, dim3(ceil_div(rows, 4)), dim3(256), 0, as_stream(stream), a);
    return launch_status("occupancyClasses");
}

int emf_hip_occupancyObjectBox(emf_occ_object_t* object, const int32_t res[3], float voxel_size) {
    if (!object || !res) return fail(EMF_E_ARG, "occupancyObjectBox: object or res is NULL");
    if (res[0] < 1 || res[1] < 1 || res[2] < 1 || object->res[0] < 1 || object->res[1] < 1 || object->res[2] < 1 ||
        !(voxel_size > 0.f) || !(object->voxelSize > 0.f))
        return fail(EMF_E_ARG, "occupancyObjectBox: a resolution below 1 or a voxel size that is not positive");
    for (int i = 0; i < 3; ++i) {  // the fall-back: everywhere
        object->lo[i] = 0;
        object->size[i] = res[i];
    }
    const float* Rf = object->R;
    double R[9], inv[9];
    for (int i = 0; i < 9; ++i) R[i] = Rf[i];
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!std::isfinite(det) || std::fabs(det) < 1e-12) return EMF_OK;
    inv[0] = (R[4] * R[8] - R[5] * R[7]) / det;
    inv[1] = (R[2] * R[7] - R[1] * R[8]) / det;
    inv[2] = (R[1] * R[5] - R[2] * R[4]) / det;
    inv[3] = (R[5] * R[6] - R[3] * R[8]) / det;
    inv[4] = (R[0] * R[8] - R[2] * R[6]) / det;
    inv[5] = (R[2] * R[3] - R[0] * R[5]) / det;
    inv[6] = (R[3] * R[7] - R[4] * R[6]) / det;
    inv[7] = (R[1] * R[6] - R[0] * R[7]) / det;
    inv[8] = (R[0] * R[4] - R[1] * R[3]) / det;
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    for (int k = 0; k < 8; ++k) {
        double po[3];  // a corner of the cube of object positions that round into the resolution
        for (int i = 0; i < 3; ++i) {
            const double q = ((k >> i) & 1) ? object->res[i] - 0.5 : -0.5;
            po[i] = (q - (object->res[i] - 1) / 2.0) * object->voxelSize - object->t[i];
        }
        for (int i = 0; i < 3; ++i) {
            const double pb = inv[3 * i] * po[0] + inv[3 * i + 1] * po[1] + inv[3 * i + 2] * po[2];
            const double v = pb / voxel_size + (res[i] - 1) / 2.0;
            if (!std::isfinite(v)) return EMF_OK;
            mn[i] = std::min(mn[i], v);
            mx[i] = std::max(mx[i], v);
        }
    }
    for (int i = 0; i < 3; ++i) {  // one voxel of margin: far above the float rounding of the forward map
        const double lo = std::max(std::floor(mn[i]) - 1.0, 0.0), hi = std::min(std::ceil(mx[i]) + 1.0, res[i] - 1.0);
        object->lo[i] = hi < lo ? 0 : static_cast<int32_t>(lo);
        object->size[i] = hi < lo ? 0 : static_cast<int32_t>(hi - lo) + 1;
    }
    return EMF_OK;
}

int emf_hip_occupancyStampObjects(uint8_t* classes, const int32_t res[3], float voxel_size, const int32_t box_lo[3],
                                  const int32_t box_size[3], const emf_occ_object_t* objects, int32_t n,
                                  emf_stream_t stream) {
    if (!classes) return fail(EMF_E_ARG, "occupancyStampObjects: classes is NULL");
    EMF_TRY(check_box(res, box_lo, box_size, "occupancyStampObjects"));
    if (!(voxel_size > 0.f)) return fail(EMF_E_ARG, "occupancyStampObjects: voxel_size %g", static_cast<double>(voxel_size));
    if (n < 0 || (n > 0 && !objects)) return fail(EMF_E_ARG, "occupancyStampObjects: %d objects, list %p", n, static_cast<const void*>(objects));
    for (int k = 0; k < n; ++k) {  // everything is checked before the first launch
        const emf_occ_object_t& o = objects[k];
        if (!o.tsdf || !o.weights) return fail(EMF_E_ARG, "occupancyStampObjects: object %d has a NULL volume", k);
        if (o.res[0] < 1 || o.res[1] < 1 || o.res[2] < 1 || !(o.voxelSize > 0.f))
            return fail(EMF_E_ARG, "occupancyStampObjects: object %d: resolution %d x %d x %d, voxel size %g", k, o.res[0],
                        o.res[1], o.res[2], static_cast<double>(o.voxelSize));
        if (static_cast<unsigned long long>(o.res[0]) * o.res[1] * static_cast<unsigned long long>(o.res[2]) > (1ull << 36))
            return fail(EMF_E_LIMIT, "occupancyStampObjects: object %d exceeds 2^36 voxels", k);
    }
    for (int first = 0; first < n; first += EMF_MAX_BATCH) {
        const int count = std::min<int>(EMF_MAX_BATCH, n - first);
        StampArgs a{};
        a.classes = classes;
        a.boxLo = i3_from(box_lo);
        a.boxSize = i3_from(box_size);
        a.half = half_extent(i3_from(res));
        a.voxel = voxel_size;
        unsigned blocks = 0;
        for (int k = 0; k < count; ++k) {
            emf_occ_object_t& o = a.obj[k];
            o = objects[first + k];
            for (int i = 0; i < 3; ++i) {  // the sub-box clipped to the box (64-bit: any lo / size is harmless)
                const long long lo = std::max<long long>(o.lo[i], box_lo[i]);
                const long long hi = std::min<long long>(static_cast<long long>(o.lo[i]) + std::max(o.size[i], 0),
                                                         static_cast<long long>(box_lo[i]) + box_size[i]);
                o.lo[i] = static_cast<int32_t>(lo);
                o.size[i] = hi > lo ? static_cast<int32_t>(hi - lo) : 0;
            }
            if (o.size[0] > 0 && o.size[1] > 0 && o.size[2] > 0)  // <= 32 * 512 * 2048 pieces
                blocks = std::max(blocks, ceil_div(o.size[0], kStampX) * ceil_div(o.size[1], kStampY) * static_cast<unsigned>(o.size[2]));
        }
        if (blocks == 0) continue;
        hipLaunchKernelGGL(k_occ_stamp, dim3(blocks, count), dim3(kStampX * kStampY), 0, as_stream(stream), a);
        EMF_TRY(launch_status("occupancyStampObjects"));
    }
    return EMF_OK;
}

int emf_hip_distanceTransform(const uint8_t* classes, const int32_t size[3], uint32_t site_mask, int32_t cap, int32_t* d2,
                              float* metres, float voxel_size, emf_stream_t stream) {
    EMF_TRY(check_transform("distanceTransform", classes, size, site_mask, cap, d2, metres, voxel_size));
    return run_transform<false>(classes, size, site_mask, cap, d2, metres, nullptr, nullptr, voxel_size, as_stream(stream));
}

size_t emf_hip_nearestSiteScratchBytes(const int32_t size[3]) {
    if (!size) return 0;
    unsigned long long voxels = 1;
    for (int i = 0; i < 3; ++i) {
        if (size[i] < 1 || size[i] > EMF_DF_MAX_AXIS) return 0;
        voxels *= static_cast<unsigned long long>(size[i]);
    }
    return voxels > 0x7fffffffull ? 0 : static_cast<size_t>(voxels) * sizeof(int32_t);
}

int emf_hip_distanceTransformNearest(const uint8_t* classes, const int32_t size[3], uint32_t site_mask, int32_t cap,
                                     int32_t* d2, float* metres, int32_t* nearest, void* scratch, float voxel_size,
                                     emf_stream_t stream) {
    EMF_TRY(check_transform("distanceTransformNearest", classes, size, site_mask, cap, d2, metres, voxel_size));
    if (!nearest || !scratch) return fail(EMF_E_ARG, "distanceTransformNearest: nearest or scratch is NULL");
    if ((reinterpret_cast<uintptr_t>(nearest) | reinterpret_cast<uintptr_t>(scratch)) & 3u)
        return fail(EMF_E_ARG, "distanceTransformNearest: misaligned arrays");
    if (nearest == scratch || nearest == d2 || scratch == d2)
        return fail(EMF_E_ARG, "distanceTransformNearest: d2, nearest and scratch must be three arrays");
    return run_transform<true>(classes, size, site_mask, cap, d2, metres, nearest, static_cast<int32_t*>(scratch), voxel_size,
                               as_stream(stream));
}

int emf_hip_distanceQuery(const uint8_t* classes, const int32_t* d2, const int32_t* nearest, const int32_t size[3],
                          const int32_t* voxels, int32_t n, uint8_t* out_class, int32_t* out_d2, int32_t* out_nearest,
                          emf_stream_t stream) {
    if (!size) return fail(EMF_E_ARG, "distanceQuery: size is NULL");
    EMF_TRY(check_box_size(size, "distanceQuery"));
    if (n < 0 || (n > 0 && !voxels)) return fail(EMF_E_ARG, "distanceQuery: %d points, list %p", n, static_cast<const void*>(voxels));
    if ((classes == nullptr) != (out_class == nullptr) || (d2 == nullptr) != (out_d2 == nullptr) ||
        (nearest == nullptr) != (out_nearest == nullptr))
        return fail(EMF_E_ARG, "distanceQuery: an input array and its output go together");
    if ((reinterpret_cast<uintptr_t>(d2) | reinterpret_cast<uintptr_t>(nearest) | reinterpret_cast<uintptr_t>(voxels) |
         reinterpret_cast<uintptr_t>(out_d2) | reinterpret_cast<uintptr_t>(out_nearest)) & 3u)
        return fail(EMF_E_ARG, "distanceQuery: misaligned arrays");
    if (n == 0 || (!classes && !d2 && !nearest)) return EMF_OK;
    const QueryArgs a{classes, d2, nearest, voxels, out_class, out_d2, out_nearest, i3_from(size), n};
    hipLaunchKernelGGL(k_df_query, dim3(ceil_div(n, 256)), dim3(256), 0, as_stream(stream), a);
    return launch_status("distanceQuery");
}

}  // extern "C"
