// mesh_components.hip -- connected components of the welded mesh and the component filter (include/emf_hip.h
// "Mesh components").
//
// Works on the welded index buffer and the soup / welded bases mesh_weld.hip leaves behind; it never sees a volume.
// Two welded vertices are connected when a triangle has both -- by INDEX: vertices of different grid edges that
// coincide at a voxel corner stay distinct, as the weld keeps them.  A vertex's label is the smallest model-local
// welded index of its component, a component's size its number of triangles.
//
// The scratch is linear in welded vertices plus triangles, under 13 bytes per vertex + 5 per triangle + 6 KiB:
//   [parent: u32 x nv][size: u32 x nv][vexcl: u32 x nv][texcl: u32 x nt][vsums: u32 x (vblocks + 1)]
//   [tsums: u32 x (tblocks + 1)][best: u64 x MAX][components: u32 x MAX][kept components: u32 x MAX][flag]
//   k_cc_init     parent[i] = i, size[i] = 0
//   k_cc_hook     per triangle: unite(a, b), unite(a, c) in a lock-free union-find over GLOBAL welded indices with
//                 parent[x] <= x always: find both roots, CAS the larger root's parent from itself to the smaller
//                 root; on failure go on from what the CAS saw.  Every step of every loop moves to a strictly
//                 smaller index, so each loop is bounded by construction and no lane waits for another lane's
//                 progress (no lock, no spin-wait: a wave runs in lock-step).  find halves the path it walks with
//                 atomicMin -- parent[x] only ever decreases, and only to an ancestor.
//   k_cc_flatten  parent[i] := root of i.  A root is the minimum index of its tree, whatever order the hooks ran in.
//   k_cc_count    size[root] += 1 per triangle: a wave whose triangles share one root adds its lane count once, the
//                 workgroup's waves are merged through LDS, lanes of a mixed wave add for themselves
//   k_cc_labels   labels[i] = root - the model's welded base, sizes[i] = size[root]   (optional outputs)
//   k_cc_select   per root: atomicMax(best[model], size << 32 | ~label) -- the largest component, ties to the
//                 smaller label
//   k_cc_flags    keep flags of vertex i and triangle i, summed per workgroup; roots count the model's components
//   k_sums_scan   two workgroups: the exclusive scans of the two sums arrays (mesh_table.hpp)
//   k_cc_rank     vexcl[i], texcl[i] = kept vertices / triangles before i; per-model kept counts and bases are the
//                 ranks at the models' bases
//   k_cc_emit     kept vertices copy position, normal and colour to their rank; kept triangles are rewritten
// A triangle index outside its model's welded range is never dereferenced: the triangle joins nothing, counts
// nowhere, is dropped by the filter, and raises `flag` (emf_hip_meshComponentsStatus -> EMF_E_ARG).
// All atomics are ordinary global atomics on vector memory; every output is a pure function of the index buffer.
#include "mesh_table.hpp"
#include "union_find.hpp"

namespace emf_hip {
namespace {

constexpr int kCcBlock = kScanBlock;

struct CcArgs : Compaction {
    unsigned* parent;
    unsigned* size;
    unsigned long long* best;  // EMF_MAX_MODELS
    unsigned* ncomp;           // EMF_MAX_MODELS
    unsigned* nkept;           // EMF_MAX_MODELS
    unsigned* flag;
};

inline size_t place(CcArgs& a, unsigned long long nv, unsigned long long nt, void* scratch) {
    a.nv = static_cast<unsigned>(nv);
    a.nt = static_cast<unsigned>(nt);
    a.vblocks = ceil_div(nv, kCcBlock);
    a.tblocks = ceil_div(nt, kCcBlock);
    ScratchArena s{static_cast<char*>(scratch), 0};
    a.parent = s.take<unsigned>(nv);
    a.size = s.take<unsigned>(nv);
    a.vexcl = s.take<unsigned>(nv);
    a.texcl = s.take<unsigned>(nt);
    a.vsums = s.take<unsigned>(a.vblocks + 1);
    a.tsums = s.take<unsigned>(a.tblocks + 1);
    a.best = s.take<unsigned long long>(EMF_MAX_MODELS);
    a.ncomp = s.take<unsigned>(EMF_MAX_MODELS);
    a.nkept = s.take<unsigned>(EMF_MAX_MODELS);
    a.flag = s.take<unsigned>(4);
    return s.off;
}

// each model's criteria, by value: the host arrays need not outlive the call
struct CcCriteria {
    unsigned minTriangles[EMF_MAX_MODELS];
    unsigned char largestOnly[EMF_MAX_MODELS];
};

// (find_root / unite: union_find.hpp, shared with motion_masks.hip)

__global__ __launch_bounds__(kCcBlock) void k_cc_init(const CcArgs a) {
    const unsigned i = blockIdx.x * kCcBlock + threadIdx.x;
    if (i < a.nv) {
        a.parent[i] = i;
        a.size[i] = 0u;
    }
}

__global__ __launch_bounds__(kCcBlock) void k_cc_hook(const CcArgs a, const MeshTable md, const int32_t* tris) {
    const unsigned t = blockIdx.x * kCcBlock + threadIdx.x;
    if (t >= a.nt) return;
    unsigned g[3];
    if (!corners(a.nv, range_of_triangle(a.nv, md, t), tris, t, g)) {
        atomicOr(a.flag, 1u);
        return;
    }
    unite(a.parent, g[0], g[1]);
    unite(a.parent, g[0], g[2]);
}

__global__ __launch_bounds__(kCcBlock) void k_cc_flatten(const CcArgs a) {
    const unsigned i = blockIdx.x * kCcBlock + threadIdx.x;
    if (i >= a.nv) return;
    const unsigned r = find_root(a.parent, i);
    atomicMin(a.parent + i, r);  // (a halving step of another lane may still be under way: the minimum wins)
}

// On a real mesh nearly every triangle belongs to one giant component, and one add per triangle would serialise on
// one address.  A wave whose live lanes share a root adds once; the workgroup's uniform waves are merged in LDS.
__global__ __launch_bounds__(kCcBlock) void k_cc_count(const CcArgs a, const MeshTable md, const int32_t* tris) {
    __shared__ unsigned wroot[kCcBlock / 64], wcount[kCcBlock / 64];
    const unsigned t = blockIdx.x * kCcBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned root = 0u;
    bool live = false;
    if (t < a.nt) {
        unsigned g[3];
        if (corners(a.nv, range_of_triangle(a.nv, md, t), tris, t, g)) {
            root = a.parent[g[0]];
            live = true;
        }
    }
    const unsigned long long mask = __ballot(live);
    unsigned uroot = 0u, ucount = 0u;
    if (mask) {
        const unsigned first = __shfl(root, __ffsll(static_cast<long long>(mask)) - 1);
        if (__all(!live || root == first)) {
            uroot = first;
            ucount = static_cast<unsigned>(__popcll(mask));
        } else if (live) {
            atomicAdd(a.size + root, 1u);
        }
    }
    if (lane == 0) {
        wroot[wave] = uroot;
        wcount[wave] = ucount;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kCcBlock / 64; ++w) {
            unsigned c = wcount[w];
            if (c == 0u) continue;
            for (int u = w + 1; u < kCcBlock / 64; ++u)
                if (wcount[u] && wroot[u] == wroot[w]) {
                    c += wcount[u];
                    wcount[u] = 0u;
                }
            atomicAdd(a.size + wroot[w], c);
        }
    }
}

__global__ __launch_bounds__(kCcBlock) void k_cc_labels(const CcArgs a, const MeshTable md, int32_t* labels,
                                                        uint32_t* sizes) {
    const unsigned i = blockIdx.x * kCcBlock + threadIdx.x;
    if (i >= a.nv) return;
    const unsigned r = a.parent[i];
    if (labels) labels[i] = static_cast<int32_t>(r - range_of_vertex(a.nv, md, i).lo);
    if (sizes) sizes[i] = a.size[r];
}

__device__ __forceinline__ unsigned long long pack_best(unsigned size, unsigned label) {
    return static_cast<unsigned long long>(size) << 32 | static_cast<unsigned>(~label);
}

__global__ __launch_bounds__(kCcBlock) void k_cc_select(const CcArgs a, const MeshTable md) {
    const unsigned i = blockIdx.x * kCcBlock + threadIdx.x;
    if (i >= a.nv || a.parent[i] != i) return;
    const Range r = range_of_vertex(a.nv, md, i);
    atomicMax(a.best + r.model, pack_best(a.size[i], i - r.lo));
}

// is the component rooted at `root` (of a model whose welded vertices start at r.lo) kept?
__device__ __forceinline__ bool kept(const CcArgs& a, const CcCriteria& c, const Range& r, unsigned root) {
    const unsigned size = a.size[root];
    if (c.minTriangles[r.model] > 1u && size < c.minTriangles[r.model]) return false;
    return !c.largestOnly[r.model] || a.best[r.model] == pack_best(size, root - r.lo);
}

__device__ __forceinline__ unsigned vertex_flag(const CcArgs& a, const MeshTable& md, const CcCriteria& c, unsigned i) {
    if (i >= a.nv) return 0u;
    return kept(a, c, range_of_vertex(a.nv, md, i), a.parent[i]) ? 1u : 0u;
}

__device__ __forceinline__ unsigned triangle_flag(const CcArgs& a, const MeshTable& md, const CcCriteria& c,
                                                  const int32_t* tris, unsigned t) {
    if (t >= a.nt) return 0u;
    const Range r = range_of_triangle(a.nv, md, t);
    unsigned g[3];
    if (!corners(a.nv, r, tris, t, g)) return 0u;
    return kept(a, c, r, a.parent[g[0]]) ? 1u : 0u;
}

__global__ __launch_bounds__(kCcBlock) void k_cc_flags(const CcArgs a, const MeshTable md, const CcCriteria c,
                                                       const int32_t* tris) {
    __shared__ unsigned lds[kCcBlock / 64];
    const unsigned i = blockIdx.x * kCcBlock + threadIdx.x;
    const unsigned vf = vertex_flag(a, md, c, i);
    if (i < a.nv && a.parent[i] == i) {  // a root: one component of its model
        const unsigned m = range_of_vertex(a.nv, md, i).model;
        atomicAdd(a.ncomp + m, 1u);
        if (vf) atomicAdd(a.nkept + m, 1u);
    }
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(vf, total, lds);
    if (threadIdx.x == 0 && blockIdx.x < a.vblocks) a.vsums[blockIdx.x] = total;
    block_exclusive_scan<kScanBlock / 64>(triangle_flag(a, md, c, tris, i), total, lds);
    if (threadIdx.x == 0 && blockIdx.x < a.tblocks) a.tsums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCcBlock) void k_cc_rank(const CcArgs a, const MeshTable md, const CcCriteria c,
                                                      const int32_t* tris) {
    __shared__ unsigned lds[kCcBlock / 64];
    const unsigned i = blockIdx.x * kCcBlock + threadIdx.x;
    unsigned total;
    const unsigned vmine = block_exclusive_scan<kScanBlock / 64>(vertex_flag(a, md, c, i), total, lds);
    if (i < a.nv) a.vexcl[i] = a.vsums[blockIdx.x] + vmine;
    const unsigned tmine = block_exclusive_scan<kScanBlock / 64>(triangle_flag(a, md, c, tris, i), total, lds);
    if (i < a.nt) a.texcl[i] = a.tsums[blockIdx.x] + tmine;
}

struct CcCounts {
    uint32_t* keptCounts;           // 2 n: vertices, triangles
    unsigned long long* keptBases;  // 2 (n + 1) interleaved or nullptr
    uint32_t* components;           // n or nullptr
    uint32_t* keptComponents;       // n or nullptr
};

// per model: a model's kept vertices and triangles lie in its own ranges, so its kept ranges start at the ranks of
// its bases
__global__ __launch_bounds__(kCcBlock) void k_cc_bases(const CcArgs a, const MeshTable md, const CcCounts out) {
    const unsigned i = blockIdx.x * kCcBlock + threadIdx.x;
    if (i > md.n) return;
    kept_ranges(a, md, i, out.keptCounts, out.keptBases);
    if (i < md.n) {
        if (out.components) out.components[i] = a.ncomp[i];
        if (out.keptComponents) out.keptComponents[i] = a.nkept[i];
    }
}

__global__ __launch_bounds__(kCcBlock) void k_cc_emit(const CcArgs a, const MeshTable md, const MeshArrays e) {
    const unsigned i = blockIdx.x * kCcBlock + threadIdx.x;
    if (i < a.nv) {
        const unsigned r = a.vexcl[i];
        if (a.vrank_at(static_cast<unsigned long long>(i) + 1) != r) copy_vertex(e, i, r);  // kept: the rank steps behind it
    }
    rewrite_triangle(a, md, e, i, [&](unsigned g) { return a.vexcl[g]; });
}

int cc_label(const int32_t* tris, uint64_t nv, uint64_t nt, const uint64_t* soupBases, const uint64_t* weldedBases, int n,
             void* scratch, int32_t* labels, uint32_t* sizes, emf_stream_t stream, const char* what) {
    EMF_TRY(check_sizes(nv, nt, n, "welded ", what));
    EMF_REQUIRE_PTR(scratch);
    if (nt) EMF_REQUIRE_PTR(tris);
    EMF_TRY(check_no_orphans(nv, nt, what));
    CcArgs a;
    place(a, nv, nt, scratch);
    EMF_TRY(memset_async(a.flag, 0, sizeof(unsigned), stream, what));
    if (nv == 0) return EMF_OK;  // nothing to label, no launch
    const MeshTable md = mesh_table(soupBases, weldedBases, n);
    const dim3 block(kCcBlock);
    hipLaunchKernelGGL(k_cc_init, dim3(a.vblocks), block, 0, as_stream(stream), a);
    if (nt) {
        hipLaunchKernelGGL(k_cc_hook, dim3(a.tblocks), block, 0, as_stream(stream), a, md, tris);
        hipLaunchKernelGGL(k_cc_flatten, dim3(a.vblocks), block, 0, as_stream(stream), a);
        hipLaunchKernelGGL(k_cc_count, dim3(a.tblocks), block, 0, as_stream(stream), a, md, tris);
    }
    if (labels || sizes) hipLaunchKernelGGL(k_cc_labels, dim3(a.vblocks), block, 0, as_stream(stream), a, md, labels, sizes);
    return launch_status(what);
}

int cc_filter_count(const int32_t* tris, uint64_t nv, uint64_t nt, const uint64_t* soupBases, const uint64_t* weldedBases,
                    int n, void* scratch, const uint32_t* minTriangles, const uint8_t* largestOnly, uint32_t* keptCounts,
                    uint64_t* keptBases, uint32_t* components, uint32_t* keptComponents, emf_stream_t stream,
                    const char* what) {
    EMF_TRY(check_sizes(nv, nt, n, "welded ", what));
    EMF_REQUIRE_PTR(scratch);
    EMF_REQUIRE_PTR(keptCounts);
    if (nt) EMF_REQUIRE_PTR(tris);
    EMF_TRY(check_no_orphans(nv, nt, what));
    if (nv == 0) {  // empty meshes: zero counts, zero bases, no launch
        EMF_TRY(memset_async(keptCounts, 0, sizeof(uint32_t) * 2 * n, stream, what));
        if (keptBases) EMF_TRY(memset_async(keptBases, 0, sizeof(uint64_t) * 2 * (n + 1), stream, what));
        if (components) EMF_TRY(memset_async(components, 0, sizeof(uint32_t) * n, stream, what));
        if (keptComponents) EMF_TRY(memset_async(keptComponents, 0, sizeof(uint32_t) * n, stream, what));
        return EMF_OK;
    }
    CcArgs a;
    place(a, nv, nt, scratch);
    CcCriteria c;
    for (int k = 0; k < EMF_MAX_MODELS; ++k) {
        c.minTriangles[k] = k < n && minTriangles ? minTriangles[k] : 0u;
        c.largestOnly[k] = k < n && largestOnly && largestOnly[k] ? 1 : 0;
    }
    // best, components and kept components are contiguous
    EMF_TRY(memset_async(a.best, 0, reinterpret_cast<char*>(a.flag) - reinterpret_cast<char*>(a.best), stream, what));
    const MeshTable md = mesh_table(soupBases, weldedBases, n);
    const CcCounts out{keptCounts, reinterpret_cast<unsigned long long*>(keptBases), components, keptComponents};
    const dim3 block(kCcBlock), items(items_blocks(a));
    hipLaunchKernelGGL(k_cc_select, dim3(a.vblocks), block, 0, as_stream(stream), a, md);
    hipLaunchKernelGGL(k_cc_flags, items, block, 0, as_stream(stream), a, md, c, tris);
    hipLaunchKernelGGL(k_sums_scan, dim3(2), dim3(kSumsBlock), 0, as_stream(stream),
                       SumsArrays{a.vsums, a.tsums, nullptr, a.vblocks, a.tblocks, 0u});
    hipLaunchKernelGGL(k_cc_rank, items, block, 0, as_stream(stream), a, md, c, tris);
    hipLaunchKernelGGL(k_cc_bases, dim3(ceil_div(n + 1, kCcBlock)), block, 0, as_stream(stream), a, md, out);
    return launch_status(what);
}

int cc_emit(const void* scratch, uint64_t nv, uint64_t nt, const uint64_t* soupBases, const uint64_t* weldedBases, int n,
            const MeshArrays& e, emf_stream_t stream, const char* what) {
    EMF_TRY(check_sizes(nv, nt, n, "welded ", what));
    EMF_TRY(check_no_orphans(nv, nt, what));
    if (nv == 0) return EMF_OK;
    EMF_TRY(check_emit_arrays(scratch, e, nt, what));
    EMF_TRY(check_emit_pairs(e, false, nt, "kept", "welded mesh's", what));
    CcArgs a;
    place(a, nv, nt, const_cast<void*>(scratch));
    hipLaunchKernelGGL(k_cc_emit, dim3(items_blocks(a)), dim3(kCcBlock), 0, as_stream(stream), a,
                       mesh_table(soupBases, weldedBases, n), e);
    return launch_status(what);
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

// The bound include/emf_hip.h declares: under 13 bytes per welded vertex + 5 per triangle + 6 KiB.
size_t emf_hip_meshComponentsScratchBytes(uint64_t weldedVertices, uint64_t triangles) {
    if (weldedVertices > (1ull << 30) || triangles >= (1ull << 31)) return 0;
    CcArgs a;
    char origin[16];
    (void)origin;
    return place(a, weldedVertices, triangles, origin);  // only the offsets are used
}

int emf_hip_meshComponentsLabel(const int32_t* triangles, uint64_t weldedVertices, uint64_t nTriangles, void* cc_scratch_dev,
                                int32_t* labels, uint32_t* sizes, emf_stream_t stream) {
    return cc_label(triangles, weldedVertices, nTriangles, nullptr, nullptr, 1, cc_scratch_dev, labels, sizes, stream,
                    "meshComponentsLabel");
}

int emf_hip_meshComponentsLabelBatched(const int32_t* triangles, uint64_t weldedVertices, uint64_t nTriangles,
                                       const uint64_t* soup_bases_dev, const uint64_t* welded_bases_dev, int n,
                                       void* cc_scratch_dev, int32_t* labels, uint32_t* sizes, emf_stream_t stream) {
    EMF_REQUIRE_PTR(soup_bases_dev);
    EMF_REQUIRE_PTR(welded_bases_dev);
    return cc_label(triangles, weldedVertices, nTriangles, soup_bases_dev, welded_bases_dev, n, cc_scratch_dev, labels,
                    sizes, stream, "meshComponentsLabelBatched");
}

int emf_hip_meshComponentsFilterCount(const int32_t* triangles, uint64_t weldedVertices, uint64_t nTriangles,
                                      void* cc_scratch_dev, const uint32_t* min_triangles, const uint8_t* largest_only,
                                      uint32_t* kept_counts, uint32_t* components, uint32_t* kept_components,
                                      emf_stream_t stream) {
    return cc_filter_count(triangles, weldedVertices, nTriangles, nullptr, nullptr, 1, cc_scratch_dev, min_triangles,
                           largest_only, kept_counts, nullptr, components, kept_components, stream,
                           "meshComponentsFilterCount");
}

int emf_hip_meshComponentsFilterCountBatched(const int32_t* triangles, uint64_t weldedVertices, uint64_t nTriangles,
                                             const uint64_t* soup_bases_dev, const uint64_t* welded_bases_dev, int n,
                                             void* cc_scratch_dev, const uint32_t* min_triangles,
                                             const uint8_t* largest_only, uint32_t* kept_counts, uint64_t* kept_bases,
                                             uint32_t* components, uint32_t* kept_components, emf_stream_t stream) {
    EMF_REQUIRE_PTR(soup_bases_dev);
    EMF_REQUIRE_PTR(welded_bases_dev);
    return cc_filter_count(triangles, weldedVertices, nTriangles, soup_bases_dev, welded_bases_dev, n, cc_scratch_dev,
                           min_triangles, largest_only, kept_counts, kept_bases, components, kept_components, stream,
                           "meshComponentsFilterCountBatched");
}

int emf_hip_meshComponentsStatus(const void* cc_scratch_dev, uint64_t weldedVertices, uint64_t nTriangles,
                                 emf_stream_t stream) {
    EMF_REQUIRE_PTR(cc_scratch_dev);
    EMF_TRY(check_sizes(weldedVertices, nTriangles, 1, "welded ", "meshComponentsStatus"));
    CcArgs a;
    place(a, weldedVertices, nTriangles, const_cast<void*>(cc_scratch_dev));
    unsigned flag;
    EMF_TRY(read_flag(a.flag, flag, stream, "meshComponentsStatus"));
    if (flag) return fail(EMF_E_ARG, "meshComponents: a triangle index lies outside its model's welded vertices");
    return EMF_OK;
}

int emf_hip_meshComponentsEmit(const void* cc_scratch_dev, uint64_t weldedVertices, uint64_t nTriangles,
                               const float* vertices, const float* normals, const uint8_t* colors,
                               const int32_t* triangles, float* kept_vertices, float* kept_normals, uint8_t* kept_colors,
                               int32_t* kept_triangles, emf_stream_t stream) {
    return cc_emit(cc_scratch_dev, weldedVertices, nTriangles, nullptr, nullptr, 1,
                   MeshArrays{vertices, normals, colors, triangles, kept_vertices, kept_normals, kept_colors, kept_triangles},
                   stream, "meshComponentsEmit");
}

int emf_hip_meshComponentsEmitBatched(const void* cc_scratch_dev, uint64_t weldedVertices, uint64_t nTriangles,
                                      const uint64_t* soup_bases_dev, const uint64_t* welded_bases_dev, int n,
                                      const float* vertices, const float* normals, const uint8_t* colors,
                                      const int32_t* triangles, float* kept_vertices, float* kept_normals,
                                      uint8_t* kept_colors, int32_t* kept_triangles, emf_stream_t stream) {
    EMF_REQUIRE_PTR(soup_bases_dev);
    EMF_REQUIRE_PTR(welded_bases_dev);
    return cc_emit(cc_scratch_dev, weldedVertices, nTriangles, soup_bases_dev, welded_bases_dev, n,
                   MeshArrays{vertices, normals, colors, triangles, kept_vertices, kept_normals, kept_colors, kept_triangles},
                   stream, "meshComponentsEmitBatched");
}

}  // extern "C"
