// tile_table.hpp -- what the passes over a table of emf_mesh_tile_t share (include/emf_hip.h "Meshing a set of tiles"):
// the tile's extent, the limits of a table, and the refusals the host can make from tiles_host and the source before
// anything is launched.  mesh_tiles.hip and occupancy_tiles.hip answer a malformed table with the same codes.
#pragma once

#include "common.hpp"

namespace emf_hip {

constexpr int kTX = 32, kTY = 8, kTZ = 8;  // the integration tile (device_core.hpp kTileX / Y / Z)
constexpr unsigned kUnitWords = 2048;      // one arena unit: 8 KiB
constexpr unsigned kMaxTiles = 1u << 17;   // 2^17 x 24576 vertices stays below 2^32
constexpr int kLatticeBits = 19;           // lattice voxel coordinates in [-2^19, 2^19)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the arena and the dense volume of class 3, as far as the host sees them
inline int check_tiles_source(const emf_mesh_tiles_source_t* source, const char* what) {
    if (!aligned16(source->arena)) return fail(EMF_E_ARG, "%s: the arena must be 16-byte aligned", what);
    if (!aligned16(source->tsdf) || !aligned16(source->weights) || !aligned16(source->color))
        return fail(EMF_E_ARG, "%s: the volume arrays must be 16-byte aligned", what);
    if ((source->weights != nullptr || source->color != nullptr) && source->tsdf == nullptr)
        return fail(EMF_E_NULL, "%s: a weight or colour volume without its tsdf", what);
    if (source->tsdf != nullptr) {
        if (source->weights == nullptr) return fail(EMF_E_NULL, "%s: source->weights is NULL", what);
        if ((source->row_stride & 3u) != 0 || (source->plane_stride & 3u) != 0)
            return fail(EMF_E_ARG, "%s: the volume's strides must be multiples of 4 voxels", what);
        if (source->row_stride > (1ull << 40) || source->plane_stride > (1ull << 40) || source->volume_elements > (1ull << 48))
            return fail(EMF_E_LIMIT, "%s: volume too large", what);
    }
    return EMF_OK;
}

// entry i of the table as the host sees it: its classes, its lattice coordinate, its place after entry i - 1
inline int check_tile_entry(const emf_mesh_tile_t* th, uint32_t i, const emf_mesh_tiles_source_t* source, const char* what) {
    const long long lim = 1ll << kLatticeBits;
    const int ext[3] = {kTX, kTY, kTZ};
    const emf_mesh_tile_t& e = th[i];
    for (int k = 0; k < 3; ++k) {
        if (e.cls[k] > 3) return fail(EMF_E_ARG, "%s: class %u of tile %u (0 .. 3)", what, e.cls[k], i);
        if (e.cls[k] == 2 && (source->arena == nullptr || source->arena_units == 0))
            return fail(EMF_E_NULL, "%s: literal tiles without an arena", what);
        if (e.cls[k] == 3 && (k == 2 ? source->color == nullptr : source->tsdf == nullptr))
            return fail(EMF_E_NULL, "%s: in-place tiles without a volume", what);
        const long long lo = static_cast<long long>(e.coord[k]) * ext[k];
        if (lo < -lim || lo + ext[k] > lim)
            return fail(EMF_E_LIMIT, "%s: tile %u at lattice voxel %lld on axis %d (within +-2^%d)", what, i, lo, k, kLatticeBits);
    }
    if (i > 0) {
        const emf_mesh_tile_t& p = th[i - 1];
        const bool after = e.coord[2] != p.coord[2] ? e.coord[2] > p.coord[2]
                           : (e.coord[1] != p.coord[1] ? e.coord[1] > p.coord[1] : e.coord[0] > p.coord[0]);
        if (!after) return fail(EMF_E_ARG, "%s: tile %u is not after tile %u in (z, y, x) order", what, i, i - 1);
    }
    return EMF_OK;
}

}  // namespace emf_hip
