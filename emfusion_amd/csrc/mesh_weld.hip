// mesh_weld.hip -- welding the marching-cubes soup by grid edge (include/emf_hip.h "Welded meshes").
//
// meshing.hip emits the reference's triangle soup: every cube its own copy of every vertex it touches, so a
// vertex of a closed surface is stored four times and no two triangles share an index.  Adjacent cubes
// interpolate the same grid edge in opposite directions (edge 0 runs 0 -> 1, edge 2 runs 2 -> 3), so the copies
// differ in their float bits in a few percent of the cases and welding by position is a tolerance guess.  The
// extractor knows the grid edge: k_mesh_keys (meshing.hip) writes it per soup vertex as a u64 key, and this
// file welds on the keys alone -- it never sees a volume.
//
// Everything here is sized by the SOUP.  A per-voxel owner map would be the obvious alternative (three edges per
// voxel -> one slot each), but the surface touches a vanishing share of the voxels: the reference's own
// per-cube buffers are 9 bytes per voxel, 1.2 GB for the 512^3 background, and the counting pass of meshing.hip
// exists to avoid exactly that.  The scratch is under 57 bytes per soup vertex (plus 1 KiB) instead:
//   [table keys: u64 x cap][table first: u32 x cap][remap: u32 x nv][excl: u32 x nv][sums: u32 x (blocks + 1)][flag]
// with cap the smallest power of two >= 2 nv.
//   k_weld_insert  per soup vertex: claim the key's slot of the open-addressing table (64-bit atomicCAS, linear
//                  probing bounded by cap -- a table that is too small raises `flag` instead of spinning), then
//                  atomicMin the soup index into it; remap[i] := the slot
//   k_weld_flags   first[i] = (table first[remap[i]] == i), summed per workgroup -> sums[b]
//   k_sums_scan    one workgroup: exclusive scan of sums in place, the total behind them (mesh_table.hpp)
//   k_weld_rank    excl[i] = firsts before i = the welded index of i if i is a first
//   k_weld_remap   remap[i] := excl[first of i's key]; the models' welded bases are excl at their soup bases
//   k_weld_emit    firsts (remap[i] == excl[i]) copy position, normal and colour to their rank; triangles are
//                  rewritten through remap, minus the model's welded base
// Which slot a key lands in depends on the order the lanes arrive; the MINIMUM soup index per key, hence every
// output, does not.  All atomics are ordinary global atomics on vector memory.
#include "mesh_table.hpp"

namespace emf_hip {
namespace {

constexpr int kWeldBlock = kScanBlock;

struct WeldArgs {
    unsigned long long* tkeys;
    unsigned* tfirst;
    unsigned* remap;
    unsigned* excl;
    unsigned* sums;  // nblocks + 1
    unsigned* flag;
    unsigned nv, cap, nblocks;
};

inline size_t place(WeldArgs& a, unsigned long long nv, void* scratch) {
    a.nv = static_cast<unsigned>(nv);
    a.cap = capacity_for(nv);
    a.nblocks = ceil_div(nv, kWeldBlock);
    ScratchArena s{static_cast<char*>(scratch), 0};
    a.tkeys = s.take<unsigned long long>(a.cap);
    a.tfirst = s.take<unsigned>(a.cap);
    a.remap = s.take<unsigned>(nv);
    a.excl = s.take<unsigned>(nv);
    a.sums = s.take<unsigned>(a.nblocks + 1);
    a.flag = s.take<unsigned>(4);
    return s.off;
}

__global__ __launch_bounds__(kWeldBlock) void k_weld_insert(const WeldArgs a, const unsigned long long* keys) {
    const unsigned i = blockIdx.x * kWeldBlock + threadIdx.x;
    if (i >= a.nv) return;
    const unsigned h = claim_slot(a.tkeys, a.tfirst, a.cap, keys[i], i);
    // (no slot: 0 is a valid one, the later passes stay inside the table whatever they compute)
    a.remap[i] = h != kNoSlot ? h : 0u;
    if (h == kNoSlot) atomicOr(a.flag, 1u);
}

__device__ __forceinline__ unsigned is_first(const WeldArgs& a, unsigned i) {
    return i < a.nv && a.tfirst[a.remap[i]] == i ? 1u : 0u;
}

__global__ __launch_bounds__(kWeldBlock) void k_weld_flags(const WeldArgs a) {
    __shared__ unsigned lds[kWeldBlock / 64];
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(is_first(a, blockIdx.x * kWeldBlock + threadIdx.x), total, lds);
    if (threadIdx.x == 0) a.sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kWeldBlock) void k_weld_rank(const WeldArgs a) {
    __shared__ unsigned lds[kWeldBlock / 64];
    const unsigned i = blockIdx.x * kWeldBlock + threadIdx.x;
    unsigned total;
    const unsigned mine = block_exclusive_scan<kScanBlock / 64>(is_first(a, i), total, lds);
    if (i < a.nv) a.excl[i] = a.sums[blockIdx.x] + mine;
}

// per-model soup bases (device, 2 (n + 1) u64 as emf_hip_meshCountBatched writes them) or, for one model, none
struct WeldModels {
    const unsigned long long* soupBases;  // nullptr: one model from 0
    unsigned n;
    unsigned* weldedCounts;               // n
    unsigned long long* weldedBases;      // n + 1 or nullptr
};

// firsts before soup vertex b (b == nv: all of them)
__device__ __forceinline__ unsigned first_rank(const WeldArgs& a, unsigned long long b) {
    return rank_at(a.excl, a.sums, a.nv, a.nblocks, b);
}

__global__ __launch_bounds__(kWeldBlock) void k_weld_remap(const WeldArgs a, const WeldModels md) {
    const unsigned i = blockIdx.x * kWeldBlock + threadIdx.x;
    if (i < a.nv) {  // own element only: in place.  (No first: only behind a raised flag -- stay inside the arrays.)
        const unsigned f = a.tfirst[a.remap[i]];
        a.remap[i] = f < a.nv ? a.excl[f] : 0u;
    }
    if (i <= md.n) {  // (EMF_MAX_MODELS + 1 <= the grid's first two workgroups; nv > 0 here)
        // a model's keys carry its slot, so its firsts lie in its own soup range: its welded range starts at the
        // rank of its soup base
        const unsigned long long lo = md.soupBases ? md.soupBases[2 * i] : (i == 0 ? 0ull : a.nv);
        const unsigned rlo = first_rank(a, lo);
        if (md.weldedBases) md.weldedBases[i] = rlo;
        if (i < md.n) {
            const unsigned long long hi = md.soupBases ? md.soupBases[2 * (i + 1)] : a.nv;
            md.weldedCounts[i] = first_rank(a, hi) - rlo;
        }
    }
}

// soup vertex -> welded vertex, soup triangle -> welded triangle.  md: the soup bases and the welded bases; e: the
// soup and the welded arrays (kt may be t)
__global__ __launch_bounds__(kWeldBlock) void k_weld_emit(const WeldArgs a, const MeshTable md, unsigned long long ntris,
                                                          const MeshArrays e) {
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kWeldBlock + threadIdx.x;
    if (i < a.nv) {
        const unsigned r = a.remap[i];
        if (r == a.excl[i]) copy_vertex(e, i, r);  // a first: a later copy's excl is at least its first's + 1
    }
    if (i < ntris) {
        unsigned long long sb = 0, wb = 0;
        if (md.triBases) {
            const unsigned m = model_of(md.triBases + 1, 2, md.n, i);
            sb = md.triBases[2 * m];
            wb = md.vertexBases[m];
        }
        const int32_t* ti = e.t + 4 * i;
        const int32_t i0 = ti[1], i1 = ti[2], i2 = ti[3];  // read before written: kt may be t
        int32_t* to = e.kt + 4 * i;
        to[0] = 3;
        // (an index outside the soup -- not something the emit kernels write -- becomes -1 instead of a wild read)
        auto welded = [&](int32_t s) {
            const unsigned long long g = sb + static_cast<unsigned>(s);
            return g < a.nv ? static_cast<int32_t>(a.remap[g] - wb) : -1;
        };
        to[1] = welded(i0);
        to[2] = welded(i1);
        to[3] = welded(i2);
    }
}

int weld_count(const uint64_t* keys, uint64_t nv, const uint64_t* soupBases, int n, void* scratch,
               uint32_t* counts, uint64_t* bases, emf_stream_t stream, const char* what) {
    EMF_TRY(check_sizes(nv, 0, n, "soup ", what));
    EMF_REQUIRE_PTR(counts);
    EMF_REQUIRE_PTR(scratch);
    if (nv) EMF_REQUIRE_PTR(keys);  // (nothing is enqueued for rejected arguments)
    WeldArgs a;
    place(a, nv, scratch);
    EMF_TRY(memset_async(a.flag, 0, sizeof(unsigned), stream, what));
    if (nv == 0) {  // an empty soup: zero counts, zero bases, no launch
        EMF_TRY(memset_async(counts, 0, sizeof(uint32_t) * n, stream, what));
        if (bases) EMF_TRY(memset_async(bases, 0, sizeof(uint64_t) * (n + 1), stream, what));
        return EMF_OK;
    }
    // keys and first indices are contiguous: all bits set = empty slot, no first yet
    EMF_TRY(memset_async(a.tkeys, 0xff, reinterpret_cast<char*>(a.remap) - reinterpret_cast<char*>(a.tkeys), stream, what));
    const dim3 grid(a.nblocks), block(kWeldBlock);
    const WeldModels md{reinterpret_cast<const unsigned long long*>(soupBases), static_cast<unsigned>(n), counts,
                        reinterpret_cast<unsigned long long*>(bases)};
    hipLaunchKernelGGL(k_weld_insert, grid, block, 0, as_stream(stream), a,
                       reinterpret_cast<const unsigned long long*>(keys));
    hipLaunchKernelGGL(k_weld_flags, grid, block, 0, as_stream(stream), a);
    hipLaunchKernelGGL(k_sums_scan, dim3(1), dim3(kSumsBlock), 0, as_stream(stream),
                       SumsArrays{a.sums, nullptr, nullptr, a.nblocks, 0u, 0u});
    hipLaunchKernelGGL(k_weld_rank, grid, block, 0, as_stream(stream), a);
    // the per-model part needs n + 1 <= 257 threads: two workgroups at least
    hipLaunchKernelGGL(k_weld_remap, dim3(a.nblocks < 2u ? 2u : a.nblocks), block, 0, as_stream(stream), a, md);
    return launch_status(what);
}

int weld_emit(const void* scratch, uint64_t nv, uint64_t nt, const uint64_t* soupBases, const uint64_t* weldedBases,
              int n, const MeshArrays& e, emf_stream_t stream, const char* what) {
    EMF_TRY(check_sizes(nv, nt, n, "soup ", what));
    EMF_TRY(check_no_orphans(nv, nt, what));
    if (nv == 0) return EMF_OK;
    EMF_TRY(check_emit_arrays(scratch, e, nt, what));
    EMF_TRY(check_emit_pairs(e, true, nt, "welded", "soup's", what));
    WeldArgs a;
    place(a, nv, const_cast<void*>(scratch));
    const uint64_t items = nv > nt ? nv : nt;
    hipLaunchKernelGGL(k_weld_emit, dim3(ceil_div(items, kWeldBlock)), dim3(kWeldBlock), 0, as_stream(stream), a,
                       mesh_table(soupBases, weldedBases, n), nt, e);
    return launch_status(what);
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

size_t emf_hip_meshWeldScratchBytes(uint64_t soupVertices) {
    if (soupVertices > (1ull << 30)) return 0;  // the table's capacity stays in 32 bits
    WeldArgs a;
    char origin[16];
    (void)origin;
    return place(a, soupVertices, origin);  // only the offsets are used
}

int emf_hip_meshWeldCount(const uint64_t* keys, uint64_t soupVertices, void* weld_scratch_dev, uint32_t* welded_count,
                          emf_stream_t stream) {
    return weld_count(keys, soupVertices, nullptr, 1, weld_scratch_dev, welded_count, nullptr, stream, "meshWeldCount");
}

int emf_hip_meshWeldCountBatched(const uint64_t* keys, uint64_t soupVertices, const uint64_t* soup_bases_dev, int n,
                                 void* weld_scratch_dev, uint32_t* welded_counts, uint64_t* welded_bases,
                                 emf_stream_t stream) {
    EMF_REQUIRE_PTR(soup_bases_dev);
    return weld_count(keys, soupVertices, soup_bases_dev, n, weld_scratch_dev, welded_counts, welded_bases, stream,
                      "meshWeldCountBatched");
}

int emf_hip_meshWeldStatus(const void* weld_scratch_dev, uint64_t soupVertices, emf_stream_t stream) {
    EMF_REQUIRE_PTR(weld_scratch_dev);
    EMF_TRY(check_sizes(soupVertices, 0, 1, "soup ", "meshWeldStatus"));
    WeldArgs a;
    place(a, soupVertices, const_cast<void*>(weld_scratch_dev));
    unsigned flag;
    EMF_TRY(read_flag(a.flag, flag, stream, "meshWeldStatus"));
    if (flag)
        return fail(EMF_E_LIMIT, "meshWeld: the table for %llu soup vertices overflowed (scratch of another size?)",
                    (unsigned long long)soupVertices);
    return EMF_OK;
}

int emf_hip_meshWeldEmit(const void* weld_scratch_dev, uint64_t soupVertices, uint64_t soupTriangles,
                         const float* vertices, const float* normals, const uint8_t* colors, const int32_t* triangles,
                         float* welded_vertices, float* welded_normals, uint8_t* welded_colors,
                         int32_t* welded_triangles, emf_stream_t stream) {
    return weld_emit(weld_scratch_dev, soupVertices, soupTriangles, nullptr, nullptr, 1,
                     MeshArrays{vertices, normals, colors, triangles, welded_vertices, welded_normals, welded_colors,
                                welded_triangles},
                     stream, "meshWeldEmit");
}

int emf_hip_meshWeldEmitBatched(const void* weld_scratch_dev, uint64_t soupVertices, uint64_t soupTriangles,
                                const uint64_t* soup_bases_dev, const uint64_t* welded_bases_dev, int n,
                                const float* vertices, const float* normals, const uint8_t* colors,
                                const int32_t* triangles, float* welded_vertices, float* welded_normals,
                                uint8_t* welded_colors, int32_t* welded_triangles, emf_stream_t stream) {
    EMF_REQUIRE_PTR(soup_bases_dev);
    EMF_REQUIRE_PTR(welded_bases_dev);
    return weld_emit(weld_scratch_dev, soupVertices, soupTriangles, soup_bases_dev, welded_bases_dev, n,
                     MeshArrays{vertices, normals, colors, triangles, welded_vertices, welded_normals, welded_colors,
                                welded_triangles},
                     stream, "meshWeldEmitBatched");
}

}  // extern "C"
