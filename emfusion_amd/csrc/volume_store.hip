// volume_store.hip -- whole integration tiles out of a volume and back into one (include/emf_hip.h "Storing and
// restoring tiles").
//
// A tile is 32 x 8 x 8 voxels: 8 KiB of tsdf, 8 KiB of weights, 16 KiB of u16 x 4 colour.  Words are moved and
// compared as BITS, never interpreted; each array of a tile gets a packed-buffer class of its own:
//   class 0  every word 0                               -> nothing stored
//   class 1  every element equals one non-zero element  -> that element (a u32; the 8-byte voxel for colour)
//   class 2  anything else                              -> the array's bytes, in tile order, in an arena
//   k_spill_classify  one workgroup of 256 lanes per tile of a box, the lane layout of k_roll_tiles: a lane holds
//                     four consecutive voxels of a row in two z planes, 16-byte loads, every load issued before the
//                     first compare; the verdict is __syncthreads_and against lane 0's first element
//   k_spill_sums      arena units (8 KiB) per workgroup of 256 candidates
//   k_spill_scan      one workgroup: exclusive scan of the sums in place, the total behind them (wave_ops.hpp)
//   k_spill_place     lits[c][k] = the arena unit of candidate c's array k.  Placement is by scan, not by atomics:
//                     candidate order, tsdf / weights / colour within a candidate, on every run
//   k_spill_gather    one workgroup per tile again: the literal arrays -> arena, tile order (z, y, x; x fastest)
//   k_fill_tiles      one workgroup per LISTED tile: every word of the tile from zero, the repeated element or the
//                     arena; thread 0 writes the tile's sign / unseen entries from the values just written
// Every byte offset is 64-bit.  A pure HBM stream: classify reads each byte once, gather re-reads the literals.
#include "device_core.hpp"
#include "wave_ops.hpp"

namespace emf_hip {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kUnitWords = 2048;  // one arena unit: 8 KiB, a tile's tsdf or weights; its colour is two

struct SpillArgs {
    const unsigned* sT;
    const unsigned* sW;
    const uint16_t* sC;  // nullptr: no colour
    I3 n;                // voxels
    I3 lo;               // the box's first tile
    uint8_t* cls;        // [ncand][3]
    unsigned* words;     // [ncand][4]
    const unsigned* lits;  // [ncand][3] (gather)
    unsigned* arena;
    unsigned long long arenaUnits;
};

// word index of this lane's four voxels in the tile's first plane group; the second is 4 * ny * nx further
__device__ __forceinline__ size_t lane_voxel(const I3& n, int tx, int ty, int tz) {
    const int xg = threadIdx.x & 7, yy = (threadIdx.x >> 3) & 7, zs = threadIdx.x >> 6;
    return (static_cast<size_t>(tz * kTileZ + zs) * n.y + (ty * kTileY + yy)) * static_cast<size_t>(n.x) + (tx * kTileX + 4 * xg);
}

__device__ __forceinline__ bool all_are(const u32x4 v, unsigned f) { return v.x == f && v.y == f && v.z == f && v.w == f; }
__device__ __forceinline__ bool pairs_are(const u32x4 v, unsigned f0, unsigned f1) {
    return v.x == f0 && v.y == f1 && v.z == f0 && v.w == f1;
}

__global__ __launch_bounds__(256) void k_spill_classify(const SpillArgs a) {
    __shared__ unsigned first[4];
    const int tx = a.lo.x + blockIdx.x, ty = a.lo.y + blockIdx.y, tz = a.lo.z + blockIdx.z;
    const size_t c = (static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const size_t s0 = lane_voxel(a.n, tx, ty, tz);
    const size_t plane4 = 4 * static_cast<size_t>(a.n.y) * a.n.x;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 c00 = zero, c01 = zero, c10 = zero, c11 = zero;
    const u32x4 t0 = *reinterpret_cast<const u32x4*>(a.sT + s0);
    const u32x4 t1 = *reinterpret_cast<const u32x4*>(a.sT + s0 + plane4);
    const u32x4 w0 = *reinterpret_cast<const u32x4*>(a.sW + s0);
    const u32x4 w1 = *reinterpret_cast<const u32x4*>(a.sW + s0 + plane4);
    if (a.sC) {  // 4 voxels x 8 bytes
        c00 = *reinterpret_cast<const u32x4*>(a.sC + 4 * s0);
        c01 = *reinterpret_cast<const u32x4*>(a.sC + 4 * s0 + 8);
        c10 = *reinterpret_cast<const u32x4*>(a.sC + 4 * (s0 + plane4));
        c11 = *reinterpret_cast<const u32x4*>(a.sC + 4 * (s0 + plane4) + 8);
    }
    if (threadIdx.x == 0) {  // lane 0 holds the tile's first voxel
        first[0] = t0.x;
        first[1] = w0.x;
        first[2] = c00.x;
        first[3] = c00.y;
    }
    __syncthreads();
    const unsigned fT = first[0], fW = first[1], fC0 = first[2], fC1 = first[3];
    const int sameT = __syncthreads_and(all_are(t0, fT) && all_are(t1, fT));
    const int sameW = __syncthreads_and(all_are(w0, fW) && all_are(w1, fW));
    const int sameC = __syncthreads_and(pairs_are(c00, fC0, fC1) && pairs_are(c01, fC0, fC1) && pairs_are(c10, fC0, fC1) &&
                                        pairs_are(c11, fC0, fC1));
    if (threadIdx.x == 0) {
        a.cls[3 * c + 0] = sameT ? (fT == 0u ? 0 : 1) : 2;
        a.cls[3 * c + 1] = sameW ? (fW == 0u ? 0 : 1) : 2;
        a.cls[3 * c + 2] = sameC ? ((fC0 | fC1) == 0u ? 0 : 1) : 2;
        *reinterpret_cast<u32x4*>(a.words + 4 * c) = u32x4{fT, fW, fC0, fC1};
    }
}

// arena units of candidate i: 1 per literal tsdf / weights, 2 per literal colour
__device__ __forceinline__ unsigned units_of(const uint8_t* cls, unsigned i, unsigned ncand) {
    if (i >= ncand) return 0u;
    const uint8_t* c = cls + 3 * static_cast<size_t>(i);
    return (c[0] == 2 ? 1u : 0u) + (c[1] == 2 ? 1u : 0u) + (c[2] == 2 ? 2u : 0u);
}

__global__ __launch_bounds__(kScanBlock) void k_spill_sums(const uint8_t* cls, unsigned ncand, unsigned* sums) {
    __shared__ unsigned lds[kScanBlock / 64];
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(units_of(cls, blockIdx.x * kScanBlock + threadIdx.x, ncand), total, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSumsBlock) void k_spill_scan(unsigned* sums, unsigned nblocks, unsigned* totals) {
    __shared__ unsigned lds[kSumsBlock / 64];
    const unsigned total = scan_sums(sums, 0u, nblocks, lds);
    if (threadIdx.x == 0) sums[nblocks] = totals[0] = total;
}

__global__ __launch_bounds__(kScanBlock) void k_spill_place(const uint8_t* cls, unsigned ncand, const unsigned* sums,
                                                            unsigned* lits) {
    __shared__ unsigned lds[kScanBlock / 64];
    const unsigned i = blockIdx.x * kScanBlock + threadIdx.x;
    unsigned total;
    unsigned at = sums[blockIdx.x] + block_exclusive_scan<kScanBlock / 64>(units_of(cls, i, ncand), total, lds);
    if (i >= ncand) return;
    const uint8_t* c = cls + 3 * static_cast<size_t>(i);
    unsigned* l = lits + 3 * static_cast<size_t>(i);
    l[0] = c[0] == 2 ? at : 0u;
    at += c[0] == 2 ? 1u : 0u;
    l[1] = c[1] == 2 ? at : 0u;
    at += c[1] == 2 ? 1u : 0u;
    l[2] = c[2] == 2 ? at : 0u;
}

// the literal of `units` units at `unit` lies inside the arena
__device__ __forceinline__ bool in_arena(unsigned unit, unsigned units, unsigned long long arenaUnits) {
    return static_cast<unsigned long long>(unit) + units <= arenaUnits;
}

__global__ __launch_bounds__(256) void k_spill_gather(const SpillArgs a) {
    const int tx = a.lo.x + blockIdx.x, ty = a.lo.y + blockIdx.y, tz = a.lo.z + blockIdx.z;
    const size_t c = (static_cast<size_t>(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    // (workgroup-uniform) a literal that would not fit is left out, never written past the arena
    const unsigned lT = a.lits[3 * c + 0], lW = a.lits[3 * c + 1], lC = a.lits[3 * c + 2];
    const bool doT = a.cls[3 * c + 0] == 2 && in_arena(lT, 1, a.arenaUnits);
    const bool doW = a.cls[3 * c + 1] == 2 && in_arena(lW, 1, a.arenaUnits);
    const bool doC = a.sC && a.cls[3 * c + 2] == 2 && in_arena(lC, 2, a.arenaUnits);
    if (!doT && !doW && !doC) return;
    const size_t s0 = lane_voxel(a.n, tx, ty, tz);
    const size_t plane4 = 4 * static_cast<size_t>(a.n.y) * a.n.x;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 t0 = zero, t1 = zero, w0 = zero, w1 = zero, c00 = zero, c01 = zero, c10 = zero, c11 = zero;
    if (doT) {
        t0 = *reinterpret_cast<const u32x4*>(a.sT + s0);
        t1 = *reinterpret_cast<const u32x4*>(a.sT + s0 + plane4);
    }
    if (doW) {
        w0 = *reinterpret_cast<const u32x4*>(a.sW + s0);
        w1 = *reinterpret_cast<const u32x4*>(a.sW + s0 + plane4);
    }
    if (doC) {
        c00 = *reinterpret_cast<const u32x4*>(a.sC + 4 * s0);
        c01 = *reinterpret_cast<const u32x4*>(a.sC + 4 * s0 + 8);
        c10 = *reinterpret_cast<const u32x4*>(a.sC + 4 * (s0 + plane4));
        c11 = *reinterpret_cast<const u32x4*>(a.sC + 4 * (s0 + plane4) + 8);
    }
    // tile order: word (z * 8 + y) * 32 + x of the tile; this lane's first voxel is 4 * threadIdx.x, its second
    // plane group 1024 voxels further
    const size_t v = 4 * static_cast<size_t>(threadIdx.x);
    if (doT) {
        unsigned* d = a.arena + static_cast<size_t>(lT) * kUnitWords;
        *reinterpret_cast<u32x4*>(d + v) = t0;
        *reinterpret_cast<u32x4*>(d + v + 1024) = t1;
    }
    if (doW) {
        unsigned* d = a.arena + static_cast<size_t>(lW) * kUnitWords;
        *reinterpret_cast<u32x4*>(d + v) = w0;
        *reinterpret_cast<u32x4*>(d + v + 1024) = w1;
    }
    if (doC) {  // two words per voxel
        unsigned* d = a.arena + static_cast<size_t>(lC) * kUnitWords;
        *reinterpret_cast<u32x4*>(d + 2 * v) = c00;
        *reinterpret_cast<u32x4*>(d + 2 * v + 4) = c01;
        *reinterpret_cast<u32x4*>(d + 2 * (v + 1024)) = c10;
        *reinterpret_cast<u32x4*>(d + 2 * (v + 1024) + 4) = c11;
    }
}

struct FillArgs {
    unsigned* dT;
    unsigned* dW;
    uint16_t* dC;      // nullptr: no colour
    uint8_t* dSign;    // nullptr: the maps are not written
    uint8_t* dUnseen;
    I3 n;              // voxels
    const int32_t* coords;  // [ntiles][3]
    const uint8_t* cls;     // [ntiles][3]
    const unsigned* words;  // [ntiles][4]
    const unsigned* lits;   // [ntiles][3]
    const unsigned* arena;
    unsigned long long arenaUnits;
};

__device__ __forceinline__ bool any_positive(const u32x4 v) {
    return __uint_as_float(v.x) > 0.f || __uint_as_float(v.y) > 0.f || __uint_as_float(v.z) > 0.f || __uint_as_float(v.w) > 0.f;
}
__device__ __forceinline__ bool any_negative(const u32x4 v) {
    return __uint_as_float(v.x) < 0.f || __uint_as_float(v.y) < 0.f || __uint_as_float(v.z) < 0.f || __uint_as_float(v.w) < 0.f;
}
// as k_unseen_tiles: a weight that is not 0 or a tsdf that is not finite
__device__ __forceinline__ bool any_seen(const u32x4 t, const u32x4 w) {
    bool seen = false;
    seen = seen || !(__uint_as_float(w.x) == 0.f) || !(fabsf(__uint_as_float(t.x)) <= 3.0e38f);
    seen = seen || !(__uint_as_float(w.y) == 0.f) || !(fabsf(__uint_as_float(t.y)) <= 3.0e38f);
    seen = seen || !(__uint_as_float(w.z) == 0.f) || !(fabsf(__uint_as_float(t.z)) <= 3.0e38f);
    seen = seen || !(__uint_as_float(w.w) == 0.f) || !(fabsf(__uint_as_float(t.w)) <= 3.0e38f);
    return seen;
}

__global__ __launch_bounds__(256) void k_fill_tiles(const FillArgs a) {
    const size_t i = blockIdx.x;
    const int ntx = a.n.x / kTileX, nty = a.n.y / kTileY, ntz = a.n.z / kTileZ;
    const int tx = a.coords[3 * i + 0], ty = a.coords[3 * i + 1], tz = a.coords[3 * i + 2];
    // (workgroup-uniform) whatever the list holds, nothing outside the volume or the arena is touched
    if (tx < 0 || tx >= ntx || ty < 0 || ty >= nty || tz < 0 || tz >= ntz) return;
    const unsigned kT = a.cls[3 * i + 0], kW = a.cls[3 * i + 1], kC = a.dC ? a.cls[3 * i + 2] : 0u;
    if (kT > 2u || kW > 2u || kC > 2u) return;
    const unsigned lT = a.lits[3 * i + 0], lW = a.lits[3 * i + 1], lC = a.lits[3 * i + 2];
    if ((kT == 2u && !in_arena(lT, 1, a.arenaUnits)) || (kW == 2u && !in_arena(lW, 1, a.arenaUnits)) ||
        (kC == 2u && !in_arena(lC, 2, a.arenaUnits)))
        return;
    const unsigned eT = kT == 1u ? a.words[4 * i + 0] : 0u, eW = kW == 1u ? a.words[4 * i + 1] : 0u;
    const unsigned eC0 = kC == 1u ? a.words[4 * i + 2] : 0u, eC1 = kC == 1u ? a.words[4 * i + 3] : 0u;
    u32x4 t0 = {eT, eT, eT, eT}, t1 = t0, w0 = {eW, eW, eW, eW}, w1 = w0;
    u32x4 c00 = {eC0, eC1, eC0, eC1}, c01 = c00, c10 = c00, c11 = c00;
    const size_t v = 4 * static_cast<size_t>(threadIdx.x);
    if (kT == 2u) {
        const unsigned* s = a.arena + static_cast<size_t>(lT) * kUnitWords;
        t0 = *reinterpret_cast<const u32x4*>(s + v);
        t1 = *reinterpret_cast<const u32x4*>(s + v + 1024);
    }
    if (kW == 2u) {
        const unsigned* s = a.arena + static_cast<size_t>(lW) * kUnitWords;
        w0 = *reinterpret_cast<const u32x4*>(s + v);
        w1 = *reinterpret_cast<const u32x4*>(s + v + 1024);
    }
    if (kC == 2u) {
        const unsigned* s = a.arena + static_cast<size_t>(lC) * kUnitWords;
        c00 = *reinterpret_cast<const u32x4*>(s + 2 * v);
        c01 = *reinterpret_cast<const u32x4*>(s + 2 * v + 4);
        c10 = *reinterpret_cast<const u32x4*>(s + 2 * (v + 1024));
        c11 = *reinterpret_cast<const u32x4*>(s + 2 * (v + 1024) + 4);
    }
    const size_t d0 = lane_voxel(a.n, tx, ty, tz);
    const size_t plane4 = 4 * static_cast<size_t>(a.n.y) * a.n.x;
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
    if (!a.dSign) return;  // (uniform)
    // what k_sign_maps / k_unseen_tiles compute from the values just written
    const int pos = __syncthreads_or(any_positive(t0) || any_positive(t1));
    const int neg = __syncthreads_or(any_negative(t0) || any_negative(t1));
    const int seen = __syncthreads_or(any_seen(t0, w0) || any_seen(t1, w1));
    if (threadIdx.x == 0) {
        const size_t tiles = static_cast<size_t>(ntx) * nty * ntz;
        const size_t dt = (static_cast<size_t>(tz) * nty + ty) * ntx + tx;
        a.dSign[dt] = pos ? 1 : 0;
        a.dSign[tiles + dt] = neg ? 1 : 0;
        a.dUnseen[dt] = seen ? 0 : 1;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_tiled(const int32_t res[3], const char* what) {
    EMF_TRY(check_res(res));
    if (res[0] % kTileX != 0 || res[1] % kTileY != 0 || res[2] % kTileZ != 0)
        return fail(EMF_E_ARG, "%s: resolution %d x %d x %d is not a multiple of the tile (32, 8, 8)", what, res[0], res[1], res[2]);
    return EMF_OK;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

size_t emf_hip_spillScratchBytes(uint64_t ntiles) {
    if (ntiles > (1ull << 30)) return 0;
    return sizeof(unsigned) * (static_cast<size_t>(ceil_div(ntiles, kScanBlock)) + 1);
}

int emf_hip_spillTiles(const float* tsdf, const float* weights, const uint16_t* color, const int32_t res[3],
                       const int32_t box_lo[3], const int32_t box_size[3], void* scratch_dev, uint8_t* classes,
                       uint32_t* words, uint32_t* lits, uint32_t* totals, void* arena, uint64_t arena_units,
                       emf_stream_t stream) {
    EMF_REQUIRE_PTR(tsdf);
    EMF_REQUIRE_PTR(weights);
    EMF_REQUIRE_PTR(box_lo);
    EMF_REQUIRE_PTR(box_size);
    EMF_REQUIRE_PTR(scratch_dev);
    EMF_REQUIRE_PTR(totals);
    EMF_TRY(check_tiled(res, "spillTiles"));
    if (!aligned16(tsdf) || !aligned16(weights) || !aligned16(color) || !aligned16(arena) || !aligned16(words))
        return fail(EMF_E_ARG, "spillTiles: the volume arrays, words and the arena must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(scratch_dev) & 3u) != 0 || (reinterpret_cast<uintptr_t>(lits) & 3u) != 0)
        return fail(EMF_E_ARG, "spillTiles: scratch_dev or lits is misaligned");
    const int nt[3] = {res[0] / kTileX, res[1] / kTileY, res[2] / kTileZ};
    for (int i = 0; i < 3; ++i)
        if (box_lo[i] < 0 || box_size[i] < 0 || box_lo[i] > nt[i] || box_size[i] > nt[i] - box_lo[i])
            return fail(EMF_E_ARG, "spillTiles: box [%d, %d + %d) on axis %d lies outside the volume's %d tiles", box_lo[i],
                        box_lo[i], box_size[i], i, nt[i]);
    const uint64_t ncand64 = static_cast<uint64_t>(box_size[0]) * box_size[1] * static_cast<uint64_t>(box_size[2]);
    if (ncand64 > (1ull << 30) || box_size[1] > 65535 || box_size[2] > 65535) return fail(EMF_E_LIMIT, "spillTiles: box too large");
    const unsigned ncand = static_cast<unsigned>(ncand64);
    if (arena && arena_units < ncand64 * (color ? 4u : 2u))
        return fail(EMF_E_LIMIT, "spillTiles: an arena of %llu units for a box whose worst case is %llu (spill it in several calls)",
                    (unsigned long long)arena_units, (unsigned long long)(ncand64 * (color ? 4u : 2u)));
    unsigned* sums = static_cast<unsigned*>(scratch_dev);
    const unsigned nblocks = ceil_div(ncand, kScanBlock);
    SpillArgs a{};
    if (ncand) {
        EMF_REQUIRE_PTR(classes);
        EMF_REQUIRE_PTR(words);
        EMF_REQUIRE_PTR(lits);
        a.sT = reinterpret_cast<const unsigned*>(tsdf);
        a.sW = reinterpret_cast<const unsigned*>(weights);
        a.sC = color;
        a.n = i3_from(res);
        a.lo = i3_from(box_lo);
        a.cls = classes;
        a.words = words;
        a.lits = lits;
        a.arena = static_cast<unsigned*>(arena);
        a.arenaUnits = arena_units;
        const dim3 grid(box_size[0], box_size[1], box_size[2]);
        hipLaunchKernelGGL(k_spill_classify, grid, dim3(256), 0, as_stream(stream), a);
        hipLaunchKernelGGL(k_spill_sums, dim3(nblocks), dim3(kScanBlock), 0, as_stream(stream), classes, ncand, sums);
    }
    hipLaunchKernelGGL(k_spill_scan, dim3(1), dim3(kSumsBlock), 0, as_stream(stream), sums, nblocks, totals);
    if (ncand) {
        hipLaunchKernelGGL(k_spill_place, dim3(nblocks), dim3(kScanBlock), 0, as_stream(stream), classes, ncand,
                           static_cast<const unsigned*>(sums), lits);
        if (arena)
            hipLaunchKernelGGL(k_spill_gather, dim3(box_size[0], box_size[1], box_size[2]), dim3(256), 0, as_stream(stream), a);
    }
    return launch_status("spillTiles");
}

int emf_hip_fillTiles(float* tsdf, float* weights, uint16_t* color, uint8_t* signMaps, uint8_t* unseenTiles,
                      const int32_t res[3], const int32_t* coords, const uint8_t* classes, const uint8_t* classes_host,
                      const uint32_t* words, const uint32_t* lits, const void* arena, uint64_t arena_units, uint32_t n,
                      emf_stream_t stream) {
    EMF_REQUIRE_PTR(tsdf);
    EMF_REQUIRE_PTR(weights);
    EMF_TRY(check_tiled(res, "fillTiles"));
    if ((signMaps == nullptr) != (unseenTiles == nullptr))
        return fail(EMF_E_ARG, "fillTiles: the sign maps and the unseen-tile map go together");
    if (!aligned16(tsdf) || !aligned16(weights) || !aligned16(color) || !aligned16(arena))
        return fail(EMF_E_ARG, "fillTiles: the volume arrays and the arena must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(coords) & 3u) != 0 || (reinterpret_cast<uintptr_t>(words) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(lits) & 3u) != 0)
        return fail(EMF_E_ARG, "fillTiles: coords, words or lits is misaligned");
    if (res[1] / kTileY > 65535 || res[2] / kTileZ > 65535 || n > (1u << 30)) return fail(EMF_E_LIMIT, "fillTiles: too large");
    if (n == 0) return EMF_OK;
    EMF_REQUIRE_PTR(coords);
    EMF_REQUIRE_PTR(classes);
    EMF_REQUIRE_PTR(classes_host);
    EMF_REQUIRE_PTR(words);
    EMF_REQUIRE_PTR(lits);
    bool literal = false;
    for (size_t i = 0; i < 3 * static_cast<size_t>(n); ++i) {
        if (classes_host[i] > 2) return fail(EMF_E_ARG, "fillTiles: class %u of tile %zu (0, 1 or 2)", classes_host[i], i / 3);
        literal = literal || classes_host[i] == 2;
    }
    if (literal && (arena == nullptr || arena_units == 0)) return fail(EMF_E_NULL, "fillTiles: literal tiles without an arena");
    FillArgs a{};
    a.dT = reinterpret_cast<unsigned*>(tsdf);
    a.dW = reinterpret_cast<unsigned*>(weights);
    a.dC = color;
    a.dSign = signMaps;
    a.dUnseen = unseenTiles;
    a.n = i3_from(res);
    a.coords = coords;
    a.cls = classes;
    a.words = words;
    a.lits = lits;
    a.arena = static_cast<const unsigned*>(arena);
    a.arenaUnits = arena ? arena_units : 0;
    hipLaunchKernelGGL(k_fill_tiles, dim3(n), dim3(256), 0, as_stream(stream), a);
    return launch_status("fillTiles");
}

}  // extern "C"
