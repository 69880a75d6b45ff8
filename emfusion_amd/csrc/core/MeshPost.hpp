// MeshPost.hpp -- what every mesher here does with its soup on the device: weld by grid edge, label / filter by
// component, cluster by cell (include/emf_hip.h "Welded meshes", "Mesh components", "Simplified meshes"), and bring to
// the host only what is left, cut into one Mesh per model.  One chain for one model (TSDF::finishMesh: fresh object,
// null stream) and for a table of models (EMFusion::extractMeshes: one persistent object on the main stream).
#pragma once

#include <cstdint>
#include <vector>

#include "emf_hip.h"
#include "types.hpp"

namespace emf {

// ---- pure host bookkeeping (no HIP call) ---------------------------------------------------------------------------

/** Model k's part of the arrays of a table of meshes: vertices [v0, v0 + vc), triangles [t0, t0 + tc). */
struct MeshSlice {
    size_t v0, vc, t0, tc;
};

/** Offsets of arrays laid one behind the other in one allocation, each 16-byte aligned (ScratchArena of
 *  csrc/common.hpp, for the host): take() them in order, allocate `off` bytes, then add the offsets to the block. */
struct Carve {
    size_t off = 0;
    template <typename T>
    size_t take(size_t count) {
        const size_t at = off;
        off += (sizeof(T) * count + 15) & ~static_cast<size_t>(15);
        return at;
    }
};

/** Slices of what a count entry left.  counts: 2 n (vertices, triangles); bases: 2 (n + 1) interleaved, or nullptr for
 *  the one-model entries, which start at 0. */
inline std::vector<MeshSlice> slicesOf(int n, const uint64_t* bases, const uint32_t* counts) {
    std::vector<MeshSlice> s(n);
    for (int k = 0; k < n; ++k)
        s[k] = MeshSlice{bases ? static_cast<size_t>(bases[2 * k]) : 0, counts[2 * k],
                         bases ? static_cast<size_t>(bases[2 * k + 1]) : 0, counts[2 * k + 1]};
    return s;
}

/** Slices of the welded table: the weld compacts the vertices (welded bases n + 1 or nullptr for one model, welded
 *  counts n) and rewrites the triangles where they lie (soup bases 2 (n + 1) interleaved, or nullptr: nt from 0). */
inline std::vector<MeshSlice> slicesOfWeld(int n, const uint64_t* weldedBases, const uint32_t* weldedCounts,
                                           const uint64_t* soupBases, uint64_t nt) {
    std::vector<MeshSlice> s(n);
    for (int k = 0; k < n; ++k)
        s[k] = MeshSlice{weldedBases ? static_cast<size_t>(weldedBases[k]) : 0, weldedCounts[k],
                         soupBases ? static_cast<size_t>(soupBases[2 * k + 1]) : 0,
                         soupBases ? static_cast<size_t>(soupBases[2 * k + 3] - soupBases[2 * k + 1]) : static_cast<size_t>(nt)};
    return s;
}

/** The bases of a table of nv vertices and nt triangles in the layout the entries take: triBases 2 (n + 1) interleaved
 *  (vertex base, triangle base), vertexBases n + 1. */
inline void basesOf(const std::vector<MeshSlice>& slices, uint64_t nv, uint64_t nt, std::vector<uint64_t>& triBases,
                    std::vector<uint64_t>& vertexBases) {
    const size_t n = slices.size();
    triBases.assign(2 * (n + 1), 0);
    vertexBases.assign(n + 1, 0);
    for (size_t k = 0; k < n; ++k) {
        vertexBases[k] = triBases[2 * k] = slices[k].v0;
        triBases[2 * k + 1] = slices[k].t0;
    }
    vertexBases[n] = triBases[2 * n] = nv;
    triBases[2 * n + 1] = nt;
}

// ---- the chain -----------------------------------------------------------------------------------------------------

/** An indexed mesh, or a table of them, on the device.  Not owned. */
struct DeviceMesh {
    const float* v = nullptr;
    const float* n = nullptr;
    const int32_t* t = nullptr;
    const uint8_t* c = nullptr;  // or nullptr: no colours
    uint64_t nv = 0, nt = 0;
};

class MeshPost {
public:
    /** The soup as the emit entries wrote it, nv > 0.  t is rewritten in place by the weld. */
    struct Soup {
        const float* v;
        const float* n;
        int32_t* t;
        const uint8_t* c;      // or nullptr
        const uint64_t* keys;  // one grid-edge key per vertex
        uint64_t nv, nt;
    };
    /** The models the soup is made of.  basesDev / bases: 2 (n + 1) interleaved soup bases as emf_hip_meshCountBatched
     *  writes them, on the device and on the host; both nullptr (n == 1): one model from 0, the one-model entries. */
    struct Table {
        int n;
        const uint64_t* basesDev;
        const uint64_t* bases;
    };
    /** What to run behind the weld.  perModel: n filters (minTriangles, largestOnly, simplifyCell), read when `filter`
     *  or `simplify`.  components: the welded mesh's labels and sizes (one model only). */
    struct Request {
        bool filter = false, simplify = false;
        const MeshFilter* perModel = nullptr;
        MeshComponents* components = nullptr;
    };
    /** What is left, in buffers of this object (valid until the next run).  filterStats: n entries when the filter
     *  ran; simplifyStats: n entries when simplification was asked for. */
    struct Result {
        DeviceMesh mesh;
        std::vector<MeshSlice> slices;
        std::vector<MeshFilterStats> filterStats;
        std::vector<MeshSimplifyStats> simplifyStats;
    };

    /** weld -> label / filter -> simplify, enqueued on `s`.  The host waits where it needs a size: in each stage's
     *  Status call.  who: the caller's name in what is thrown. */
    Result run(const Stream& s, const Soup& soup, const Table& table, const Request& req, const char* who);

    /** The arrays of `m` to the host in one set of copies on `s` and one wait, cut into out[k] by slices[k]. */
    void download(const Stream& s, const DeviceMesh& m, const std::vector<MeshSlice>& slices, Mesh* out);

private:
    DeviceBuffer weldScratch, weldArena;          // welded counts / bases and the weld's scratch; the welded arrays
    DeviceBuffer filterScratch, filterArena;      // the filter's counts + scratch; its kept arrays
    DeviceBuffer simplifyScratch, simplifyArena;  // the simplification's bases, counts + scratch; its arrays
    DeviceBuffer labels, sizes;                   // Request::components
    PinnedBuffer stage;                           // download's staging (grown when needed)
};

}  // namespace emf
