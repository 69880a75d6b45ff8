// object_shape.hip -- object shapes: the integer moments of the observed solid band of every model of a table, and its
// extents along given axes (include/emf_hip.h "Object shapes").
//
// A launch covers the slots [first, first + n) of a model table: model m owns a contiguous range of workgroups, one per
// 32 x 8 x 8 tile of its volume (the tile of the unseen-tile map); the ranges travel in the kernel arguments, the
// volumes' pointers in the device table.
//   k_shape_moments  256 lanes = 8 quads along x, 8 rows, 4 planes; two steps cover the tile's 8 planes.  A lane takes
//                    four consecutive voxels from two 16-byte loads where its address is 16-byte aligned in both arrays
//                    (a row whose first voxel is, as in k_occ_classes) and voxel by voxel elsewhere; the mask bytes
//                    come as one word or byte by byte.  Only a solid voxel gathers its six face neighbours -- the band
//                    is thin, so these are gathers behind a branch, no LDS halo.  Per-lane sums are u32 (8 voxels of at
//                    most 2047^2), the wave's too (512 voxels: below 2^32); the four waves meet in LDS, the workgroup's
//                    total is u64 and goes to the model's record with one integer atomic per non-zero quantity.  A wave
//                    that observed nothing skips its shuffles.
//   k_shape_extents  the same walk; a solid voxel computes e_k in single float32 operations (the _rn intrinsics: never
//                    contracted, whatever the build) and keeps the minimum and maximum of their order-preserving u32
//                    keys; wave shuffles, LDS, one atomicMin / atomicMax per workgroup and quantity.
//   k_shape_init / k_shape_finish  one lane per record: the neutral records before the pass, keys -> f32 bits after it.
// A workgroup whose tile the model's unseen-tile map marks "every weight is 0" leaves at once: it holds no solid and no
// observed voxel.  Integer atomics only: the records do not depend on the order of waves or workgroups.
#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {
namespace {

constexpr int kShBlock = 256;
constexpr int kShTileX = 32, kShTileY = 8, kShTileZ = 8;  // the tile of emf_model_t.unseenTiles
constexpr int kShSums = 13;

static_assert(sizeof(emf_shape_moments_t) == 128, "emf_shape_moments_t is mirrored by emfusion_amd/_lib.py");
static_assert(sizeof(emf_shape_axes_t) == 48 && sizeof(emf_shape_extents_t) == 24, "mirrored by emfusion_amd/_lib.py");

struct ShapeArgs {
    const emf_model_t* models;  // slot `first` of the table
    emf_shape_moments_t* moments;
    const emf_shape_axes_t* frames;
    emf_shape_extents_t* extents;  // u32 keys between k_shape_init and k_shape_finish
    unsigned n;
    unsigned start[EMF_MAX_MODELS + 1];  // model m: workgroups [start[m], start[m + 1])
};
static_assert(sizeof(ShapeArgs) <= 4096, "ShapeArgs travels in the kernel arguments");

// the model whose range [start[m], start[m + 1]) holds x (block-uniform)
__device__ __forceinline__ unsigned model_of(const unsigned* start, unsigned n, unsigned x) {
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (x >= start[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned float_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ unsigned key_bits(unsigned k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// The tile of a workgroup and the model it belongs to; false: nothing to do (block-uniform).
struct Tile {
    const float* tsdf;
    const float* weights;
    const uint8_t* mask;
    I3 n;
    int x0, y, z0;  // this lane's quad, row and first plane
    unsigned m;
};

__device__ __forceinline__ bool tile_of(const ShapeArgs& a, Tile& t) {
    t.m = model_of(a.start, a.n, blockIdx.x);
    const emf_model_t& md = a.models[t.m];
    t.n = I3{md.res[0], md.res[1], md.res[2]};
    const unsigned ntx = (t.n.x + kShTileX - 1) / kShTileX, nty = (t.n.y + kShTileY - 1) / kShTileY;
    const unsigned b = blockIdx.x - a.start[t.m];
    if (md.unseenTiles != nullptr && md.unseenTiles[b] != 0) return false;  // the map's index is this tile order
    const unsigned tz = b / (ntx * nty), r = b - tz * ntx * nty, ty = r / ntx, tx = r - ty * ntx;
    t.tsdf = md.tsdf;
    t.weights = md.weights;
    t.mask = md.fgVolMask;
    t.x0 = static_cast<int>(tx) * kShTileX + 4 * static_cast<int>(threadIdx.x & 7u);
    t.y = static_cast<int>(ty) * kShTileY + static_cast<int>((threadIdx.x >> 3) & 7u);
    t.z0 = static_cast<int>(tz) * kShTileZ + static_cast<int>(threadIdx.x >> 6);
    return true;
}

// Up to four consecutive voxels of a row from x0 on: their values and, per voxel, bit e of `solid` and `observed`.
struct Quad {
    unsigned solid, observed;
    int count;
};

__device__ __forceinline__ Quad load_quad(const Tile& t, size_t i, int count) {
    float tv[4] = {1.f, 1.f, 1.f, 1.f}, wv[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned fg = 0x01010101u;
    const float* tp = t.tsdf + i;
    const float* wp = t.weights + i;
    if (count == 4 && ((reinterpret_cast<uintptr_t>(tp) | reinterpret_cast<uintptr_t>(wp)) & 15u) == 0) {
        const float4 a = *reinterpret_cast<const float4*>(tp), b = *reinterpret_cast<const float4*>(wp);
        tv[0] = a.x, tv[1] = a.y, tv[2] = a.z, tv[3] = a.w;
        wv[0] = b.x, wv[1] = b.y, wv[2] = b.z, wv[3] = b.w;
        if (t.mask != nullptr) {
            const uint8_t* mp = t.mask + i;
            if ((reinterpret_cast<uintptr_t>(mp) & 3u) == 0)
                fg = *reinterpret_cast<const unsigned*>(mp);
            else
                fg = mp[0] | (mp[1] << 8) | (mp[2] << 16) | (static_cast<unsigned>(mp[3]) << 24);
        }
    } else {
        fg = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < count) {
                tv[e] = tp[e];
                wv[e] = wp[e];
                fg |= (t.mask == nullptr || t.mask[i + e] != 0 ? 1u : 0u) << (8 * e);
            }
    }
    Quad q{0u, 0u, count};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool obs = e < count && wv[e] > 0.f;
        const bool sol = obs && ((fg >> (8 * e)) & 0xffu) != 0u && !(tv[e] > 0.f);
        q.observed |= (obs ? 1u : 0u) << e;
        q.solid |= (sol ? 1u : 0u) << e;
    }
    return q;
}

// the kind of a face neighbour inside the volume: 1 for FREE, 1 << 16 for UNKNOWN, 0 for neither (a lane meets at most
// 48 neighbours: the two counts share a word)
__device__ __forceinline__ unsigned face_kind(const Tile& t, size_t j) {
    if (!(t.weights[j] > 0.f)) return 1u << 16;
    return t.tsdf[j] > 0.f ? 1u : 0u;
}

__global__ __launch_bounds__(kShBlock) void k_shape_moments(const ShapeArgs a) {
    __shared__ unsigned sums[kShBlock / 64][kShSums];
    __shared__ int bounds[kShBlock / 64][6];
    Tile t;
    if (!tile_of(a, t)) return;  // block-uniform: no lane reaches the barrier
    // solid, observed, x, y, z, xx, yy, zz, xy, xz, yz, free faces, unknown faces: the order of the record
    unsigned cs = 0u, co = 0u, sx = 0u, sy1 = 0u, sz1 = 0u, sxx = 0u, syy = 0u, szz = 0u, sxy = 0u, sxz = 0u, syz = 0u, faces = 0u;
    int lox = t.n.x, loy = t.n.y, loz = t.n.z, hix = -1, hiy = -1, hiz = -1;
    const size_t sy = static_cast<size_t>(t.n.x), sz = sy * t.n.y;
    const int count = min(4, t.n.x - t.x0);
    if (count > 0 && t.y < t.n.y) {
#pragma unroll
        for (int step = 0; step < 2; ++step) {
            const int z = t.z0 + 4 * step;
            if (z < t.n.z) {
                const size_t i = static_cast<size_t>(z) * sz + static_cast<size_t>(t.y) * sy + t.x0;
                const Quad q = load_quad(t, i, count);
                co += __popc(q.observed);
                if (q.solid != 0u) {
                    const unsigned uy = t.y, uz = z;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if ((q.solid >> e) & 1u) {
                            const int x = t.x0 + e;
                            const unsigned ux = x;
                            const size_t v = i + e;
                            cs += 1u;
                            sx += ux, sy1 += uy, sz1 += uz;
                            sxx += ux * ux, syy += uy * uy, szz += uz * uz;
                            sxy += ux * uy, sxz += ux * uz, syz += uy * uz;
                            lox = min(lox, x), hix = max(hix, x);
                            if (x > 0) faces += face_kind(t, v - 1);
                            if (x + 1 < t.n.x) faces += face_kind(t, v + 1);
                            if (t.y > 0) faces += face_kind(t, v - sy);
                            if (t.y + 1 < t.n.y) faces += face_kind(t, v + sy);
                            if (z > 0) faces += face_kind(t, v - sz);
                            if (z + 1 < t.n.z) faces += face_kind(t, v + sz);
                        }
                    }
                    loy = min(loy, t.y), hiy = max(hiy, t.y);
                    loz = min(loz, z), hiz = max(hiz, z);
                }
            }
        }
    }
    unsigned acc[kShSums] = {cs, co, sx, sy1, sz1, sxx, syy, szz, sxy, sxz, syz, faces & 0xffffu, faces >> 16};
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (__ballot(acc[1] != 0u) != 0ull) {  // wave-uniform
#pragma unroll
        for (int k = 0; k < kShSums; ++k) acc[k] = wave_reduce<OpAdd>(acc[k]);
        lox = wave_reduce<OpMin>(lox), loy = wave_reduce<OpMin>(loy), loz = wave_reduce<OpMin>(loz);
        hix = wave_reduce<OpMax>(hix), hiy = wave_reduce<OpMax>(hiy), hiz = wave_reduce<OpMax>(hiz);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kShSums; ++k) sums[wave][k] = acc[k];
        bounds[wave][0] = lox, bounds[wave][1] = loy, bounds[wave][2] = loz;
        bounds[wave][3] = hix, bounds[wave][4] = hiy, bounds[wave][5] = hiz;
    }
    __syncthreads();
    emf_shape_moments_t* out = a.moments + t.m;
    const unsigned k = threadIdx.x;
    if (k < kShSums) {  // the record's first 13 words are its sums, in this order
        unsigned long long total = 0ull;
#pragma unroll
        for (int w = 0; w < kShBlock / 64; ++w) total += sums[w][k];
        if (total) atomicAdd(reinterpret_cast<unsigned long long*>(out) + k, total);
    } else if (k < kShSums + 6) {
        const unsigned solid = sums[0][0] + sums[1][0] + sums[2][0] + sums[3][0];  // at most 2048
        if (solid) {
            const int j = static_cast<int>(k) - kShSums;
            int v = bounds[0][j];
            if (j < 3) {
                for (int w = 1; w < kShBlock / 64; ++w) v = min(v, bounds[w][j]);
                atomicMin(&out->lo[j], v);
            } else {
                for (int w = 1; w < kShBlock / 64; ++w) v = max(v, bounds[w][j]);
                atomicMax(&out->hi[j - 3], v);
            }
        }
    }
}

__global__ __launch_bounds__(kShBlock) void k_shape_extents(const ShapeArgs a) {
    __shared__ unsigned keys[kShBlock / 64][6];
    __shared__ unsigned any[kShBlock / 64];
    Tile t;
    if (!tile_of(a, t)) return;  // block-uniform
    const emf_shape_axes_t& f = a.frames[t.m];
    unsigned lo0 = 0xffffffffu, lo1 = 0xffffffffu, lo2 = 0xffffffffu, hi0 = 0u, hi1 = 0u, hi2 = 0u, solid = 0u;
    const size_t sy = static_cast<size_t>(t.n.x), sz = sy * t.n.y;
    const int count = min(4, t.n.x - t.x0);
    if (count > 0 && t.y < t.n.y) {
        const float p1 = __fsub_rn(static_cast<float>(t.y), f.c[1]);
#pragma unroll
        for (int step = 0; step < 2; ++step) {
            const int z = t.z0 + 4 * step;
            if (z >= t.n.z) continue;
            const size_t i = static_cast<size_t>(z) * sz + static_cast<size_t>(t.y) * sy + t.x0;
            const Quad q = load_quad(t, i, count);
            if (q.solid == 0u) continue;
            solid |= q.solid;
            const float p2 = __fsub_rn(static_cast<float>(z), f.c[2]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!((q.solid >> e) & 1u)) continue;
                const float p0 = __fsub_rn(static_cast<float>(t.x0 + e), f.c[0]);
                const float e0 = __fadd_rn(__fadd_rn(__fmul_rn(f.A[0], p0), __fmul_rn(f.A[1], p1)), __fmul_rn(f.A[2], p2));
                const float e1 = __fadd_rn(__fadd_rn(__fmul_rn(f.A[3], p0), __fmul_rn(f.A[4], p1)), __fmul_rn(f.A[5], p2));
                const float e2 = __fadd_rn(__fadd_rn(__fmul_rn(f.A[6], p0), __fmul_rn(f.A[7], p1)), __fmul_rn(f.A[8], p2));
                const unsigned k0 = float_key(e0), k1 = float_key(e1), k2 = float_key(e2);
                lo0 = min(lo0, k0), hi0 = max(hi0, k0);
                lo1 = min(lo1, k1), hi1 = max(hi1, k1);
                lo2 = min(lo2, k2), hi2 = max(hi2, k2);
            }
        }
    }
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool waveSolid = __ballot(solid != 0u) != 0ull;  // wave-uniform
    if (waveSolid) {
        lo0 = wave_reduce<OpMin>(lo0), lo1 = wave_reduce<OpMin>(lo1), lo2 = wave_reduce<OpMin>(lo2);
        hi0 = wave_reduce<OpMax>(hi0), hi1 = wave_reduce<OpMax>(hi1), hi2 = wave_reduce<OpMax>(hi2);
    }
    if (lane == 0) {
        keys[wave][0] = lo0, keys[wave][1] = lo1, keys[wave][2] = lo2;
        keys[wave][3] = hi0, keys[wave][4] = hi1, keys[wave][5] = hi2;
        any[wave] = waveSolid ? 1u : 0u;
    }
    __syncthreads();
    const unsigned k = threadIdx.x;
    if (k < 6 && (any[0] | any[1] | any[2] | any[3]) != 0u) {
        unsigned* out = reinterpret_cast<unsigned*>(a.extents + t.m);  // lo[3] then hi[3]
        unsigned v = keys[0][k];
        if (k < 3) {
            for (int w = 1; w < kShBlock / 64; ++w) v = min(v, keys[w][k]);
            atomicMin(out + k, v);
        } else {
            for (int w = 1; w < kShBlock / 64; ++w) v = max(v, keys[w][k]);
            atomicMax(out + k, v);
        }
    }
}

// one lane per record: the neutral records
__global__ __launch_bounds__(256) void k_shape_init(const ShapeArgs a) {
    const unsigned m = blockIdx.x * 256u + threadIdx.x;
    if (m >= a.n) return;
    if (a.moments != nullptr) {
        emf_shape_moments_t r{};
        for (int j = 0; j < 3; ++j) {
            r.lo[j] = a.models[m].res[j];
            r.hi[j] = -1;
        }
        a.moments[m] = r;
    }
    if (a.extents != nullptr) {
        unsigned* e = reinterpret_cast<unsigned*>(a.extents + m);
        for (int j = 0; j < 3; ++j) {
            e[j] = 0xff800000u;      // the key of +inf
            e[3 + j] = 0x007fffffu;  // the key of -inf
        }
    }
}

// one lane per record: keys -> the bits of the floats
__global__ __launch_bounds__(256) void k_shape_finish(const ShapeArgs a) {
    const unsigned m = blockIdx.x * 256u + threadIdx.x;
    if (m >= a.n) return;
    unsigned* e = reinterpret_cast<unsigned*>(a.extents + m);
    for (int j = 0; j < 6; ++j) e[j] = key_bits(e[j]);
}

// the checks both entries share and the workgroup ranges; nothing is enqueued
int plan(ShapeArgs& a, const char* who, const emf_model_t* models_dev, const int32_t* res_host, int32_t first, int32_t n) {
    if (!models_dev || !res_host) return fail(EMF_E_ARG, "%s: the model table or its resolutions are NULL", who);
    if (n <= 0 || first < 0 || first > EMF_MAX_MODELS || n > EMF_MAX_MODELS - first)
        return fail(EMF_E_ARG, "%s: slots [%d, %d + %d) of a table of %d", who, first, first, n, EMF_MAX_MODELS);
    if (reinterpret_cast<uintptr_t>(models_dev) & 7u) return fail(EMF_E_ARG, "%s: a misaligned model table", who);
    unsigned long long blocks = 0;
    for (int m = 0; m < n; ++m) {
        const int32_t* r = res_host + 3 * m;
        for (int i = 0; i < 3; ++i) {
            if (r[i] < 1) return fail(EMF_E_ARG, "%s: model %d has %d voxels on axis %d", who, first + m, r[i], i);
            if (r[i] > EMF_DF_MAX_AXIS)
                return fail(EMF_E_LIMIT, "%s: model %d has %d voxels on axis %d, above %d", who, first + m, r[i], i, EMF_DF_MAX_AXIS);
        }
        const unsigned long long voxels = static_cast<unsigned long long>(r[0]) * r[1] * static_cast<unsigned long long>(r[2]);
        if (voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "%s: model %d has %llu voxels, above 2^31 - 1", who, first + m, voxels);
        a.start[m] = static_cast<unsigned>(blocks);
        blocks += static_cast<unsigned long long>((r[0] + kShTileX - 1) / kShTileX) * ((r[1] + kShTileY - 1) / kShTileY) *
                  ((r[2] + kShTileZ - 1) / kShTileZ);
        if (blocks > 0xffffffull) return fail(EMF_E_LIMIT, "%s: more than 2^24 - 1 tiles in one launch", who);
    }
    for (int m = n; m <= EMF_MAX_MODELS; ++m) a.start[m] = static_cast<unsigned>(blocks);
    a.models = models_dev + first;
    a.n = static_cast<unsigned>(n);
    return EMF_OK;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_shapeMoments(const emf_model_t* models_dev, const int32_t* res_host, int32_t first, int32_t n,
                         emf_shape_moments_t* moments_dev, emf_stream_t stream) {
    ShapeArgs a{};
    EMF_TRY(plan(a, "shapeMoments", models_dev, res_host, first, n));
    if (!moments_dev) return fail(EMF_E_ARG, "shapeMoments: the records are NULL");
    if (reinterpret_cast<uintptr_t>(moments_dev) & 7u) return fail(EMF_E_ARG, "shapeMoments: misaligned records");
    a.moments = moments_dev;
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_shape_init, dim3(ceil_div(a.n, 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_shape_moments, dim3(a.start[a.n]), dim3(kShBlock), 0, s, a);
    return launch_status("shapeMoments");
}

int emf_hip_shapeExtents(const emf_model_t* models_dev, const int32_t* res_host, int32_t first, int32_t n,
                         const emf_shape_axes_t* frames_dev, emf_shape_extents_t* extents_dev, emf_stream_t stream) {
    ShapeArgs a{};
    EMF_TRY(plan(a, "shapeExtents", models_dev, res_host, first, n));
    if (!frames_dev || !extents_dev) return fail(EMF_E_ARG, "shapeExtents: the frames or the records are NULL");
    if ((reinterpret_cast<uintptr_t>(frames_dev) | reinterpret_cast<uintptr_t>(extents_dev)) & 3u)
        return fail(EMF_E_ARG, "shapeExtents: misaligned frames or records");
    a.frames = frames_dev;
    a.extents = extents_dev;
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_shape_init, dim3(ceil_div(a.n, 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_shape_extents, dim3(a.start[a.n]), dim3(kShBlock), 0, s, a);
    hipLaunchKernelGGL(k_shape_finish, dim3(ceil_div(a.n, 256)), dim3(256), 0, s, a);
    return launch_status("shapeExtents");
}

}  // extern "C"
