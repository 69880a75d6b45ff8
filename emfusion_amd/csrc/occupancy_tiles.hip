// occupancy_tiles.hip -- occupancy classes of a box of the LATTICE from a sparse set of integration tiles
// (include/emf_hip.h "Occupancy of a set of tiles"): emf_hip_occupancyClasses of the dense volume that
// holds exactly the listed tiles and is unobserved everywhere else, without that volume ever existing.
//
//   k_occ_tiles  one workgroup of 256 lanes per tile-aligned cell (32 x 8 x 8) the box overlaps.  Wave 0 finds the
//                cell's tile in the table, which is sorted in (z, y, x) -- a search that probes 64 entries per step, at
//                most three steps instead of a binary search's seventeen --, and lane 0 resolves its tsdf and
//                weights into a base and two strides each (a literal: rows 32, planes 256 apart in the arena; in place:
//                the volume's own strides) -- 72 bytes of LDS, the only LDS there is.  A cell without a tile, or with
//                one the device has to skip, is UNKNOWN; a tile whose two arrays are all zero or one repeated word
//                has one class, decided once.  Otherwise a lane reads four consecutive voxels of both arrays by one
//                16-byte load each, twice (z and z + 4), and classifies them with the three comparisons of
//                k_occ_classes.  Four class bytes go out as one 32-bit store where all four lie inside the box and
//                the destination is 4-byte aligned, byte by byte otherwise.
// Every byte of the box is written exactly once by a plain store: no atomics, no dependence on workgroup order.
#include "tile_table.hpp"

namespace emf_hip {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kOccTilesBlock = 256;

struct OccTilesArgs {
    const emf_mesh_tile_t* tiles;
    unsigned n;
    const unsigned* arena;
    unsigned long long arenaUnits;
    const unsigned* vT;  // the dense volume of class 3
    const unsigned* vW;
    const void* vC;      // only asked whether it is there: a tile is skipped as a whole (the mesher's rule)
    unsigned long long volElems, row, plane;
    uint8_t* out;
    I3 lo, size;         // the box, lattice voxels
    I3 cell0, cells;     // the lattice tile coordinate of the first cell, and how many there are
};

// The tile of a cell as the lanes read it.  uniform: both arrays are all zero or one word, the class is cls.
struct Resolved {
    const unsigned* base[2];
    unsigned long long row[2], plane[2];
    unsigned w[2];
    unsigned vec[2];  // the array is read from base (class 2, 3); else every voxel is w
    unsigned uniform, cls;
};

__device__ __forceinline__ unsigned occ_class(float t, float w) {
    return w > 0.f ? (t > 0.f ? EMF_OCC_FREE : EMF_OCC_OCCUPIED) : EMF_OCC_UNKNOWN;
}

// array k of an entry can be read (mesh_tiles.hip array_ok): its literal inside the arena, its in-place tile inside
// the volume
__device__ __forceinline__ bool array_ok(const OccTilesArgs& a, unsigned c, unsigned long long at, int k) {
    const unsigned long long units = k == 2 ? 2ull : 1ull;
    const bool literal = at <= a.arenaUnits && a.arenaUnits - at >= units;
    const void* v = k == 0 ? static_cast<const void*>(a.vT) : (k == 1 ? static_cast<const void*>(a.vW) : a.vC);
    const unsigned long long span = 7ull * a.plane + 7ull * a.row + 32ull;
    const bool inplace = v != nullptr && (at & 3ull) == 0ull && at <= a.volElems && a.volElems - at >= span;
    return c <= 1u || (c == 2u && literal) || (c == 3u && inplace);
}

// Wave 0, all 64 lanes: the index of the first entry not before (cz, cy, cx).  A 64-ary search: every step probes 64
// evenly spaced entries at once and a ballot counts those before the key, so a table of 2^17 entries takes three
// dependent loads where a binary search takes seventeen -- the search is the latency every workgroup starts with.
__device__ __forceinline__ unsigned first_not_before(const OccTilesArgs& a, int cx, int cy, int cz) {
    const unsigned lane = threadIdx.x & 63u;
    unsigned lo = 0, hi = a.n;
    while (lo < hi) {  // (wave-uniform)
        const unsigned step = (hi - lo + 63u) / 64u;
        const unsigned at = lo + lane * step;  // below 2^17 + 63 * 2^11
        bool before = false;
        if (at < hi) {
            const emf_mesh_tile_t& e = a.tiles[at];
            const int ex = e.coord[0], ey = e.coord[1], ez = e.coord[2];
            before = ez != cz ? ez < cz : (ey != cy ? ey < cy : ex < cx);
        }
        const unsigned c = static_cast<unsigned>(__popcll(__ballot(before)));  // a prefix of the probes: the table is sorted
        if (c == 0u) break;                                                    // the first probe is entry lo
        const unsigned upper = lo + c * step;
        lo = lo + (c - 1u) * step + 1u;
        hi = upper < hi ? upper : hi;
    }
    return lo;
}

// lane 0: entry `lo` resolved if it is the tile at lattice tile (cx, cy, cz); an absent or skipped tile is uniform UNKNOWN
__device__ __forceinline__ void resolve(const OccTilesArgs& a, unsigned lo, int cx, int cy, int cz, Resolved* out) {
    Resolved r{};
    r.uniform = 1u;
    r.cls = EMF_OCC_UNKNOWN;
    bool ok = lo < a.n;
    if (ok) {
        const emf_mesh_tile_t& e = a.tiles[lo];
        ok = e.coord[0] == cx && e.coord[1] == cy && e.coord[2] == cz;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) ok = ok & array_ok(a, e.cls[k], e.at[k], k);
        }
        if (ok) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const unsigned c = e.cls[k];
                const unsigned long long at = e.at[k];
                const unsigned* vol = k == 0 ? a.vT : a.vW;
                r.vec[k] = c >= 2u ? 1u : 0u;
                r.w[k] = c == 1u ? e.words[k] : 0u;
                r.base[k] = c == 2u ? a.arena + at * kUnitWords : vol + at;  // (read only when vec[k])
                r.row[k] = c == 2u ? static_cast<unsigned long long>(kTX) : a.row;
                r.plane[k] = c == 2u ? static_cast<unsigned long long>(kTX * kTY) : a.plane;
            }
            r.uniform = (r.vec[0] | r.vec[1]) == 0u ? 1u : 0u;
            r.cls = occ_class(__uint_as_float(r.w[0]), __uint_as_float(r.w[1]));
        }
    }
    *out = r;
}

__global__ __launch_bounds__(kOccTilesBlock) void k_occ_tiles(const OccTilesArgs a) {
    __shared__ Resolved sTile;
    // (workgroup-uniform) the cell
    const unsigned b = blockIdx.x;
    const unsigned perZ = static_cast<unsigned>(a.cells.x) * static_cast<unsigned>(a.cells.y);
    const unsigned bz = b / perZ, r = b - bz * perZ, by = r / static_cast<unsigned>(a.cells.x),
                   bx = r - by * static_cast<unsigned>(a.cells.x);
    if (bz >= static_cast<unsigned>(a.cells.z)) return;
    const int cx = a.cell0.x + static_cast<int>(bx), cy = a.cell0.y + static_cast<int>(by), cz = a.cell0.z + static_cast<int>(bz);
    if (threadIdx.x < 64) {  // (the whole of wave 0)
        const unsigned found = first_not_before(a, cx, cy, cz);
        if (threadIdx.x == 0) resolve(a, found, cx, cy, cz, &sTile);
    }
    __syncthreads();
    const Resolved& t = sTile;

    // this lane's four voxels of a row: x = 4 (lane & 7) .., y = lane >> 3 & 7, z = (lane >> 6) + 4 g
    const int lx = 4 * (threadIdx.x & 7), ly = (threadIdx.x >> 3) & 7;
    const int bxv = cx * kTX + lx - a.lo.x, byv = cy * kTY + ly - a.lo.y;  // box coordinates
    if (byv < 0 || byv >= a.size.y) return;
    // which of the four lie inside the box on x
    unsigned inx = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) inx |= (bxv + i >= 0 && bxv + i < a.size.x) ? 1u << i : 0u;
    if (inx == 0u) return;
    const bool vec0 = t.vec[0] != 0u, vec1 = t.vec[1] != 0u, uniform = t.uniform != 0u;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int lz = static_cast<int>(threadIdx.x >> 6) + 4 * g;
        const int bzv = cz * kTZ + lz - a.lo.z;
        if (bzv < 0 || bzv >= a.size.z) continue;
        unsigned c0, c1, c2, c3;
        if (uniform) {
            c0 = c1 = c2 = c3 = t.cls;
        } else {
            u32x4 tv = {t.w[0], t.w[0], t.w[0], t.w[0]}, wv = {t.w[1], t.w[1], t.w[1], t.w[1]};
            if (vec0)
                tv = *reinterpret_cast<const u32x4*>(t.base[0] + (static_cast<unsigned long long>(lz) * t.plane[0] +
                                                                  static_cast<unsigned long long>(ly) * t.row[0] + lx));
            if (vec1)
                wv = *reinterpret_cast<const u32x4*>(t.base[1] + (static_cast<unsigned long long>(lz) * t.plane[1] +
                                                                  static_cast<unsigned long long>(ly) * t.row[1] + lx));
            c0 = occ_class(__uint_as_float(tv.x), __uint_as_float(wv.x));
            c1 = occ_class(__uint_as_float(tv.y), __uint_as_float(wv.y));
            c2 = occ_class(__uint_as_float(tv.z), __uint_as_float(wv.z));
            c3 = occ_class(__uint_as_float(tv.w), __uint_as_float(wv.w));
        }
        // the row of the box; bxv may be negative here, the pointer is formed only where a byte is stored
        const long long at = (static_cast<long long>(bzv) * a.size.y + byv) * static_cast<long long>(a.size.x) + bxv;
        if (inx == 15u && ((reinterpret_cast<uintptr_t>(a.out) + static_cast<unsigned long long>(at)) & 3u) == 0u) {
            *reinterpret_cast<unsigned*>(a.out + at) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
        } else {
            if (inx & 1u) a.out[at] = static_cast<uint8_t>(c0);
            if (inx & 2u) a.out[at + 1] = static_cast<uint8_t>(c1);
            if (inx & 4u) a.out[at + 2] = static_cast<uint8_t>(c2);
            if (inx & 8u) a.out[at + 3] = static_cast<uint8_t>(c3);
        }
    }
}

int floor_div(int v, int d) { return v >= 0 ? v / d : -((-v + d - 1) / d); }

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_occupancyTiles(const emf_mesh_tile_t* tiles_dev, const emf_mesh_tile_t* tiles_host, uint32_t n,
                           const emf_mesh_tiles_source_t* source, const int32_t box_lo[3], const int32_t box_size[3],
                           uint8_t* classes, emf_stream_t stream) {
    const char* what = "occupancyTiles";
    if (n > kMaxTiles) return fail(EMF_E_LIMIT, "%s: %u tiles (at most %u per table)", what, n, kMaxTiles);
    EMF_REQUIRE_PTR(source);
    if (n) {
        EMF_REQUIRE_PTR(tiles_dev);
        EMF_REQUIRE_PTR(tiles_host);
    }
    if ((reinterpret_cast<uintptr_t>(tiles_dev) & 7u) != 0) return fail(EMF_E_ARG, "%s: tiles_dev is misaligned", what);
    EMF_TRY(check_tiles_source(source, what));
    for (uint32_t i = 0; i < n; ++i) EMF_TRY(check_tile_entry(tiles_host, i, source, what));
    // the box: the limits of emf_hip_occupancyClasses, on the lattice
    if (!box_lo || !box_size || !classes) return fail(EMF_E_ARG, "%s: box_lo, box_size or classes is NULL", what);
    const long long lim = 1ll << kLatticeBits;
    unsigned long long voxels = 1;
    for (int i = 0; i < 3; ++i) {
        if (box_size[i] < 1) return fail(EMF_E_ARG, "%s: box axis %d has %d voxels", what, i, box_size[i]);
        if (box_size[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "%s: box axis %d has %d voxels, above %d", what, i, box_size[i], EMF_DF_MAX_AXIS);
        if (box_lo[i] < -lim || static_cast<long long>(box_lo[i]) + box_size[i] > lim)
            return fail(EMF_E_LIMIT, "%s: the box [%d, %d + %d) leaves the lattice on axis %d (within +-2^%d)", what, box_lo[i],
                        box_lo[i], box_size[i], i, kLatticeBits);
        voxels *= static_cast<unsigned long long>(box_size[i]);
    }
    if (voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "%s: a box of %llu voxels, above 2^31 - 1", what, voxels);

    OccTilesArgs a{};
    a.tiles = tiles_dev;
    a.n = n;
    a.arena = static_cast<const unsigned*>(source->arena);
    a.arenaUnits = source->arena ? source->arena_units : 0;
    a.vT = reinterpret_cast<const unsigned*>(source->tsdf);
    a.vW = reinterpret_cast<const unsigned*>(source->weights);
    a.vC = source->color;
    a.volElems = source->tsdf ? source->volume_elements : 0;
    a.row = source->row_stride;
    a.plane = source->plane_stride;
    a.out = classes;
    a.lo = i3_from(box_lo);
    a.size = i3_from(box_size);
    const int ext[3] = {kTX, kTY, kTZ};
    int first[3], count[3];
    for (int i = 0; i < 3; ++i) {
        first[i] = floor_div(box_lo[i], ext[i]);
        count[i] = floor_div(box_lo[i] + box_size[i] - 1, ext[i]) - first[i] + 1;
    }
    a.cell0 = I3{first[0], first[1], first[2]};
    a.cells = I3{count[0], count[1], count[2]};
    // at most 65 x 257 x 257 cells: a one-dimensional grid
    const unsigned blocks = static_cast<unsigned>(count[0]) * static_cast<unsigned>(count[1]) * static_cast<unsigned>(count[2]);
    hipLaunchKernelGGL(k_occ_tiles, dim3(blocks), dim3(kOccTilesBlock), 0, as_stream(stream), a);
    return launch_status(what);
}

}  // extern "C"
