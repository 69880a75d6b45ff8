// volume_roll.hip -- shift a volume by whole voxels from one copy into another (include/emf_hip.h "Rolling a
// volume").
//
// dst(v) = src(v + shift) inside the source, 0 elsewhere, for the tsdf, the weights and -- when given -- the
// u16 x 4 colour volume, all in one launch.  Words are moved, never interpreted: -0.0f and NaN patterns survive.
//   k_roll_tiles   shift and resolution are multiples of the 32 x 8 x 8 integration tile: one workgroup per
//                  DESTINATION tile, the tile coordinate is the block index (no division anywhere), a lane moves
//                  four consecutive voxels of a row with 16-byte accesses (two per array, four for the colour),
//                  every load of a lane issued before its first store.  A tile whose source lies outside the volume is
//                  written as zeros without a load.  Thread 0 moves the tile's three map entries (positive sign,
//                  negative sign, unseen) or writes "no sign, unseen": a whole-tile move maps tiles onto tiles, so
//                  the moved entries are what a rebuild from the shifted values computes.
//   k_roll_voxels  anything else: one voxel per lane on a 3-d grid (no division either), 4-byte accesses (8 for
//                  the colour).  The maps are not written: the caller rebuilds them.
// A pure HBM stream: every source byte inside the overlap is read once, every destination byte written once.
#include "device_core.hpp"

#include <algorithm>

namespace emf_hip {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct RollArgs {
    const unsigned* sT;
    const unsigned* sW;
    const uint16_t* sC;  // nullptr: no colour
    unsigned* dT;
    unsigned* dW;
    uint16_t* dC;
    const uint8_t* sSign;  // nullptr: the maps are not moved
    const uint8_t* sUnseen;
    uint8_t* dSign;
    uint8_t* dUnseen;
    I3 n;      // voxels
    I3 shift;  // k_roll_tiles: in TILES; k_roll_voxels: in voxels
};

__global__ __launch_bounds__(256) void k_roll_tiles(const RollArgs a) {
    const int ntx = a.n.x / kTileX, nty = a.n.y / kTileY, ntz = a.n.z / kTileZ;
    const int tx = blockIdx.x, ty = blockIdx.y, tz = blockIdx.z;
    const int sx = tx + a.shift.x, sy = ty + a.shift.y, sz = tz + a.shift.z;  // source tile (wave-uniform)
    const bool inside = sx >= 0 && sx < ntx && sy >= 0 && sy < nty && sz >= 0 && sz < ntz;
    const int xg = threadIdx.x & 7, yy = (threadIdx.x >> 3) & 7, zs = threadIdx.x >> 6;
    const size_t nx = static_cast<size_t>(a.n.x), ny = static_cast<size_t>(a.n.y);
    // voxel index of this lane's four voxels in plane zs of the tile; the second plane is 4 * ny * nx further
    const size_t d0 = (static_cast<size_t>(tz * kTileZ + zs) * ny + (ty * kTileY + yy)) * nx + (tx * kTileX + 4 * xg);
    const size_t plane4 = 4 * ny * nx;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 t0 = zero, t1 = zero, w0 = zero, w1 = zero, c00 = zero, c01 = zero, c10 = zero, c11 = zero;
    if (inside) {
        const size_t s0 = (static_cast<size_t>(sz * kTileZ + zs) * ny + (sy * kTileY + yy)) * nx + (sx * kTileX + 4 * xg);
        t0 = *reinterpret_cast<const u32x4*>(a.sT + s0);
        t1 = *reinterpret_cast<const u32x4*>(a.sT + s0 + plane4);
        w0 = *reinterpret_cast<const u32x4*>(a.sW + s0);
        w1 = *reinterpret_cast<const u32x4*>(a.sW + s0 + plane4);
        if (a.sC) {  // 4 voxels x 8 bytes
            c00 = *reinterpret_cast<const u32x4*>(a.sC + 4 * s0);
            c01 = *reinterpret_cast<const u32x4*>(a.sC + 4 * s0 + 8);
            c10 = *reinterpret_cast<const u32x4*>(a.sC + 4 * (s0 + plane4));
            c11 = *reinterpret_cast<const u32x4*>(a.sC + 4 * (s0 + plane4) + 8);
        }
    }
    *reinterpret_cast<u32x4*>(a.dT + d0) = t0;
    *reinterpret_cast<u32x4*>(a.dT + d0 + plane4) = t1;
    *reinterpret_cast<u32x4*>(a.dW + d0) = w0;
    *reinterpret_cast<u32x4*>(a.dW + d0 + plane4) = w1;
    if (a.dC) {
        *reinterpret_cast<u32x4*>(a.dC + 4 * d0) = c00;
        *reinterpret_cast<u32x4*>(a.dC + 4 * d0 + 8) = c01;
        *reinterpret_cast<u32x4*>(a.dC + 4 * (d0 + plane4)) = c10;
        *reinterpret_cast<u32x4*>(a.dC + 4 * (d0 + plane4) + 8) = c11;
    }
    if (threadIdx.x == 0 && a.dSign) {
        const size_t tiles = static_cast<size_t>(ntx) * nty * ntz;
        const size_t dt = (static_cast<size_t>(tz) * nty + ty) * ntx + tx;
        uint8_t pos = 0, neg = 0, unseen = 1;  // an all-zero tile: no sign, unseen
        if (inside) {
            const size_t st = (static_cast<size_t>(sz) * nty + sy) * ntx + sx;
            pos = a.sSign[st];
            neg = a.sSign[tiles + st];
            unseen = a.sUnseen[st];
        }
        a.dSign[dt] = pos;
        a.dSign[tiles + dt] = neg;
        a.dUnseen[dt] = unseen;
    }
}

constexpr int kRollX = 64, kRollY = 4;

__global__ __launch_bounds__(kRollX * kRollY) void k_roll_voxels(const RollArgs a) {
    const int x = blockIdx.x * kRollX + threadIdx.x, y = blockIdx.y * kRollY + threadIdx.y, z = blockIdx.z;
    if (x >= a.n.x || y >= a.n.y) return;
    const int sx = x + a.shift.x, sy = y + a.shift.y, sz = z + a.shift.z;
    const bool inside = sx >= 0 && sx < a.n.x && sy >= 0 && sy < a.n.y && sz >= 0 && sz < a.n.z;
    const size_t nx = static_cast<size_t>(a.n.x), ny = static_cast<size_t>(a.n.y);
    const size_t d = (static_cast<size_t>(z) * ny + y) * nx + x;
    unsigned t = 0u, w = 0u;
    u32x2 c = {0u, 0u};
    if (inside) {
        const size_t s = (static_cast<size_t>(sz) * ny + sy) * nx + sx;
        t = a.sT[s];
        w = a.sW[s];
        if (a.sC) c = *reinterpret_cast<const u32x2*>(a.sC + 4 * s);
    }
    a.dT[d] = t;
    a.dW[d] = w;
    if (a.dC) *reinterpret_cast<u32x2*>(a.dC + 4 * d) = c;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_rollVolumeIsTiled(const int32_t res[3], const int32_t shift[3]) {
    if (!res || !shift) return 0;
    const int tile[3] = {kTileX, kTileY, kTileZ};
    for (int i = 0; i < 3; ++i)
        if (res[i] < 1 || res[i] % tile[i] != 0 || shift[i] % tile[i] != 0) return 0;
    return 1;
}

int emf_hip_rollVolume(const float* srcTsdf, const float* srcWeights, const uint16_t* srcColor, const uint8_t* srcSignMaps,
                       const uint8_t* srcUnseenTiles, float* dstTsdf, float* dstWeights, uint16_t* dstColor,
                       uint8_t* dstSignMaps, uint8_t* dstUnseenTiles, const int32_t res[3], const int32_t shift[3],
                       emf_stream_t stream) {
    EMF_REQUIRE_PTR(srcTsdf);
    EMF_REQUIRE_PTR(srcWeights);
    EMF_REQUIRE_PTR(dstTsdf);
    EMF_REQUIRE_PTR(dstWeights);
    EMF_REQUIRE_PTR(shift);
    EMF_TRY(check_res(res));
    if ((srcColor == nullptr) != (dstColor == nullptr))
        return fail(EMF_E_ARG, "rollVolume: a colour volume on one side only");
    const int maps = (srcSignMaps != nullptr) + (srcUnseenTiles != nullptr) + (dstSignMaps != nullptr) + (dstUnseenTiles != nullptr);
    if (maps != 0 && maps != 4) return fail(EMF_E_ARG, "rollVolume: the four map pointers go together");
    const size_t voxels = static_cast<size_t>(res[0]) * res[1] * static_cast<size_t>(res[2]);
    const void* srcs[3] = {srcTsdf, srcWeights, srcColor};
    const void* dsts[3] = {dstTsdf, dstWeights, dstColor};
    const size_t bytes[3] = {voxels * 4, voxels * 4, voxels * 8};
    for (int d = 0; d < 3; ++d)
        for (int s = 0; s < 3; ++s)
            if (dsts[d] && srcs[s] && overlap(dsts[d], bytes[d], srcs[s], bytes[s]))
                return fail(EMF_E_ARG, "rollVolume: a destination array overlaps a source array (the roll is out of place)");
    for (int d = 0; d < 3; ++d)
        for (int e = d + 1; e < 3; ++e)
            if (dsts[d] && dsts[e] && overlap(dsts[d], bytes[d], dsts[e], bytes[e]))
                return fail(EMF_E_ARG, "rollVolume: two destination arrays overlap");
    RollArgs a{};
    a.sT = reinterpret_cast<const unsigned*>(srcTsdf);
    a.sW = reinterpret_cast<const unsigned*>(srcWeights);
    a.sC = srcColor;
    a.dT = reinterpret_cast<unsigned*>(dstTsdf);
    a.dW = reinterpret_cast<unsigned*>(dstWeights);
    a.dC = dstColor;
    a.n = i3_from(res);
    if (emf_hip_rollVolumeIsTiled(res, shift)) {
        for (int k = 0; k < 3; ++k)
            if (!aligned16(srcs[k]) || !aligned16(dsts[k]))
                return fail(EMF_E_ARG, "rollVolume: the arrays of a tile-granular roll must be 16-byte aligned");
        const int ntx = res[0] / kTileX, nty = res[1] / kTileY, ntz = res[2] / kTileZ;
        if (nty > 65535 || ntz > 65535) return fail(EMF_E_LIMIT, "rollVolume: volume too large");
        if (maps) {
            const size_t tiles = static_cast<size_t>(ntx) * nty * ntz;
            if (overlap(dstSignMaps, 2 * tiles, srcSignMaps, 2 * tiles) || overlap(dstUnseenTiles, tiles, srcUnseenTiles, tiles) ||
                overlap(dstSignMaps, 2 * tiles, dstUnseenTiles, tiles))
                return fail(EMF_E_ARG, "rollVolume: the destination maps overlap the source maps or each other");
            a.sSign = srcSignMaps;
            a.sUnseen = srcUnseenTiles;
            a.dSign = dstSignMaps;
            a.dUnseen = dstUnseenTiles;
        }
        // in tiles, clamped: any shift of a whole extent or more empties the volume (and keeps sums inside int)
        a.shift = I3{std::clamp(shift[0] / kTileX, -ntx, ntx), std::clamp(shift[1] / kTileY, -nty, nty),
                     std::clamp(shift[2] / kTileZ, -ntz, ntz)};
        hipLaunchKernelGGL(k_roll_tiles, dim3(ntx, nty, ntz), dim3(256), 0, as_stream(stream), a);
        return launch_status("rollVolume");
    }
    if ((srcColor && ((reinterpret_cast<uintptr_t>(srcColor) | reinterpret_cast<uintptr_t>(dstColor)) & 7u)) ||
        ((reinterpret_cast<uintptr_t>(srcTsdf) | reinterpret_cast<uintptr_t>(srcWeights) | reinterpret_cast<uintptr_t>(dstTsdf) |
          reinterpret_cast<uintptr_t>(dstWeights)) & 3u))
        return fail(EMF_E_ARG, "rollVolume: misaligned arrays");
    if (ceil_div(res[1], kRollY) > 65535u || res[2] > 65535) return fail(EMF_E_LIMIT, "rollVolume: volume too large");
    a.shift = I3{std::clamp(shift[0], -res[0], res[0]), std::clamp(shift[1], -res[1], res[1]), std::clamp(shift[2], -res[2], res[2])};
    hipLaunchKernelGGL(k_roll_voxels, dim3(ceil_div(res[0], kRollX), ceil_div(res[1], kRollY), res[2]), dim3(kRollX, kRollY), 0,
                       as_stream(stream), a);
    return launch_status("rollVolume");
}

}  // extern "C"
