// mesh_simplify.hip -- vertex clustering of the welded mesh (include/emf_hip.h "Simplified meshes").
//
// Works on an indexed mesh (or a table of them) as mesh_weld.hip / mesh_components.hip leave it; it never sees a
// volume.  All vertices of a model that fall into one cubic cell become one vertex, triangles are re-indexed, the
// collapsed ones dropped, and so are the clusters no kept triangle references.
//
// A cluster is known by its FIRST member: the smallest global vertex index that carries its key.  Everything a
// cluster owns -- its accumulators, its "referenced" mark, its rank -- sits at that index, so no array is sized by
// the number of clusters and nothing has to be read back between the passes.  The scratch is linear in vertices
// plus triangles, under 137 bytes per vertex + 5 per triangle + 8 KiB:
//   [table keys: u64 x cap][table first: u32 x cap][rep: u32 x nv][count: u32 x nv][ref: u32 x nv]
//   [sums: i64 x 9 nv (position, normal, colour)][vexcl: u32 x nv][texcl: u32 x nt]
//   [csums: u32 x (vblocks + 1)][vsums: u32 x (vblocks + 1)][tsums: u32 x (tblocks + 1)][flag]
// with cap the smallest power of two >= 2 nv.
//   k_sp_insert      per vertex: the cell in double (no reciprocal), the 64-bit key, then the weld's insert: claim the
//                    key's slot (64-bit atomicCAS, linear probing bounded by cap), atomicMin the vertex index into
//                    it; rep[i] := the slot.  A vertex of a pass-through model (cell <= 0) or one the definition
//                    refuses is its own cluster (rep[i] := none); a refusal raises `flag`
//   k_sp_accumulate  rep[i] := the first member of i's cluster; count and the nine integer sums are added at that
//                    index.  Welded vertices arrive in spatial runs, so a wave first sums every run of lanes that
//                    share a first (a segmented shuffle reduction) and only the run's head lane issues the ten
//                    atomics: a coarse cell costs nv / 64 adds per accumulator instead of nv
//   k_sp_mark        per triangle: corners -> firsts; kept if the three differ (always, in a pass-through model);
//                    the kept flag goes to texcl, ref[first] := 1 for its three clusters (every lane stores the same
//                    1).  Per vertex of a pass-through model: ref[i] := 1
//   k_sp_flags       three flags summed per workgroup: "is a first" (the clusters met), "is a referenced first" (the
//                    kept vertices), "kept triangle"
//   k_sums_scan      three workgroups: the exclusive scans of the three sums arrays (mesh_table.hpp)
//   k_sp_rank        vexcl[i], texcl[i] = kept vertices / triangles before i
//   k_sp_bases       per model: kept counts, kept bases and the clusters met, all ranks at the models' bases
//   k_sp_emit        a kept first writes its cluster's vertex at its rank (its own bits if it is alone, the integer
//                    means otherwise); a kept triangle is rewritten through vexcl[first of corner]
// Why atomics and not store-then-sum-per-destination: the traffic is 80 bytes per vertex -- 10 MB for the 123 k
// vertices of the benchmark scene, 80 MB for a million -- so even far below the chip's atomic rate the pass stays
// well under a millisecond, while the other form needs a count per cluster, a third scan, a scatter of 80-byte
// records and a reducer whose time is set by the fullest cell.  The adds are 64-bit INTEGER adds, which commute:
// the sums, hence every output, are the same whatever order they arrive in.  No float atomics.
// Which slot a key lands in depends on the order the lanes arrive; the MINIMUM index per key does not.  All atomics
// are ordinary global atomics on vector memory; every loop is bounded by construction; nothing waits on another lane.
#include "mesh_table.hpp"

namespace emf_hip {
namespace {

constexpr int kSpBlock = kScanBlock;
constexpr unsigned kNone = kNoSlot;  // rep[i] after the insert: no slot, the vertex is its own cluster
constexpr unsigned kFlagLimit = 1u, kFlagArg = 2u;

struct SpArgs : Compaction {
    unsigned long long* tkeys;
    unsigned* tfirst;
    unsigned* rep;
    unsigned* count;
    unsigned* ref;
    long long* sums;  // 9 per vertex: position x y z, normal x y z, colour r g b
    unsigned* csums;  // vblocks + 1: firsts (Compaction's vsums: referenced firsts, tsums: kept triangles)
    unsigned* flag;
    unsigned cap;
};

inline size_t place(SpArgs& a, unsigned long long nv, unsigned long long nt, void* scratch) {
    a.nv = static_cast<unsigned>(nv);
    a.nt = static_cast<unsigned>(nt);
    a.cap = capacity_for(nv);
    a.vblocks = ceil_div(nv, kSpBlock);
    a.tblocks = ceil_div(nt, kSpBlock);
    ScratchArena s{static_cast<char*>(scratch), 0};
    a.tkeys = s.take<unsigned long long>(a.cap);
    a.tfirst = s.take<unsigned>(a.cap);
    a.rep = s.take<unsigned>(nv);
    a.count = s.take<unsigned>(nv);
    a.ref = s.take<unsigned>(nv);
    a.sums = s.take<long long>(9 * nv);
    a.vexcl = s.take<unsigned>(nv);
    a.texcl = s.take<unsigned>(nt);
    a.csums = s.take<unsigned>(a.vblocks + 1);
    a.vsums = s.take<unsigned>(a.vblocks + 1);
    a.tsums = s.take<unsigned>(a.tblocks + 1);
    a.flag = s.take<unsigned>(4);
    return s.off;
}

// each model's cell and the origin, by value: the host arrays need not outlive the call
struct SpCells {
    float cell[EMF_MAX_MODELS];
    float origin[3];
};

// the cluster key of position p in model `slot`, or false where the definition refuses the vertex
__device__ __forceinline__ bool cluster_key(const float* p, const SpCells& c, unsigned slot, unsigned long long& key) {
    key = static_cast<unsigned long long>(slot) << 48;
    const double cell = static_cast<double>(c.cell[slot]);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float x = p[j];
        const double q = floor((static_cast<double>(x) - static_cast<double>(c.origin[j])) / cell);
        // (a NaN or infinite x fails the first comparison, a NaN or infinite q the second)
        const bool in = fabsf(x) < 1024.0f && q >= -32768.0 && q < 32768.0;
        ok = ok && in;
        key |= static_cast<unsigned long long>(in ? static_cast<long long>(q) + 32768 : 0) << (16 * j);
    }
    return ok;
}

__global__ __launch_bounds__(kSpBlock) void k_sp_insert(const SpArgs a, const MeshTable md, const SpCells c,
                                                        const float* verts) {
    const unsigned i = blockIdx.x * kSpBlock + threadIdx.x;
    if (i >= a.nv) return;
    const unsigned slot = range_of_vertex(a.nv, md, i).model;
    a.rep[i] = kNone;
    if (!(c.cell[slot] > 0.0f)) return;  // a pass-through model: every vertex its own cluster
    unsigned long long key;
    if (!cluster_key(verts + 3 * static_cast<size_t>(i), c, slot, key)) {
        atomicOr(a.flag, kFlagLimit);
        return;
    }
    const unsigned h = claim_slot(a.tkeys, a.tfirst, a.cap, key, i);
    if (h == kNoSlot) atomicOr(a.flag, kFlagLimit);  // the table cannot hold the keys
    else a.rep[i] = h;
}

// Q20 of a coordinate with |p| < 2^10: exact in double, |q| <= 2^30
__device__ __forceinline__ long long q20(float p) { return llrint(ldexp(static_cast<double>(p), 20)); }

// a normal component that is not finite or has |n| >= 2^10 counts as 0
__device__ __forceinline__ long long q20_normal(float n) { return fabsf(n) < 1024.0f ? q20(n) : 0ll; }

__device__ __forceinline__ long long shfl_down64(long long v, int o) {
    const int lo = __shfl_down(static_cast<int>(v), o);
    const int hi = __shfl_down(static_cast<int>(v >> 32), o);
    return static_cast<long long>(static_cast<unsigned long long>(static_cast<unsigned>(hi)) << 32 |
                                  static_cast<unsigned>(lo));
}

__global__ __launch_bounds__(kSpBlock) void k_sp_accumulate(const SpArgs a, const float* verts, const float* norms,
                                                            const uint8_t* cols) {
    const unsigned i = blockIdx.x * kSpBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned first = kNone;  // lanes past the end: a run of their own that adds nothing
    long long s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned cnt = 0u;
    if (i < a.nv) {
        const unsigned h = a.rep[i];
        const unsigned f = h == kNone ? i : a.tfirst[h];
        first = f < a.nv ? f : i;  // (the table only holds indices below nv: stay inside the arrays whatever it says)
        a.rep[i] = first;
        cnt = 1u;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float p = verts[3 * static_cast<size_t>(i) + j];
            s[j] = fabsf(p) < 1024.0f ? q20(p) : 0ll;  // (a refused coordinate: the flag is up already)
            s[3 + j] = q20_normal(norms[3 * static_cast<size_t>(i) + j]);
            s[6 + j] = cols ? static_cast<long long>(cols[3 * static_cast<size_t>(i) + j]) : 0ll;
        }
    }
    // runs of consecutive lanes with one first: the head of a run collects the run's sums
    const unsigned before = __shfl_up(first, 1);
    const bool head = lane == 0 || before != first;
    const unsigned long long heads = __ballot(head);
    if (heads != ~0ull) {  // (a wave of 64 runs of one lane has nothing to collect)
        const unsigned long long later = (heads >> lane) >> 1;
        const int last = later ? lane + __ffsll(static_cast<long long>(later)) - 1 : 63;  // the run's last lane
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const bool take = lane + o <= last;
            const unsigned oc = __shfl_down(cnt, o);
            if (take) cnt += oc;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const long long os = shfl_down64(s[j], o);
                if (take) s[j] += os;
            }
        }
    }
    if (!head || first == kNone) return;
    atomicAdd(a.count + first, cnt);
    const int nsum = cols ? 9 : 6;
    for (int j = 0; j < nsum; ++j)
        atomicAdd(reinterpret_cast<unsigned long long*>(a.sums + 9 * static_cast<size_t>(first) + j),
                  static_cast<unsigned long long>(s[j]));
}

__device__ __forceinline__ bool is_first(const SpArgs& a, unsigned i) { return i < a.nv && a.rep[i] == i; }

__global__ __launch_bounds__(kSpBlock) void k_sp_mark(const SpArgs a, const MeshTable md, const SpCells c,
                                                      const int32_t* tris) {
    const unsigned i = blockIdx.x * kSpBlock + threadIdx.x;
    if (i < a.nv && !(c.cell[range_of_vertex(a.nv, md, i).model] > 0.0f)) a.ref[i] = 1u;  // pass-through: all kept
    if (i >= a.nt) return;
    const Range r = range_of_triangle(a.nv, md, i);
    unsigned g[3];
    unsigned keep = 0u;
    if (!corners(a.nv, r, tris, i, g)) {
        atomicOr(a.flag, kFlagArg);
    } else {
        const unsigned f0 = a.rep[g[0]], f1 = a.rep[g[1]], f2 = a.rep[g[2]];
        if (!(c.cell[r.model] > 0.0f) || (f0 != f1 && f1 != f2 && f0 != f2)) {
            keep = 1u;
            a.ref[f0] = 1u;
            a.ref[f1] = 1u;
            a.ref[f2] = 1u;
        }
    }
    a.texcl[i] = keep;
}

__device__ __forceinline__ unsigned vertex_flag(const SpArgs& a, unsigned i) {
    return is_first(a, i) && a.ref[i] ? 1u : 0u;
}

__global__ __launch_bounds__(kSpBlock) void k_sp_flags(const SpArgs a) {
    __shared__ unsigned lds[kSpBlock / 64];
    const unsigned i = blockIdx.x * kSpBlock + threadIdx.x;
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(is_first(a, i) ? 1u : 0u, total, lds);
    if (threadIdx.x == 0 && blockIdx.x < a.vblocks) a.csums[blockIdx.x] = total;
    block_exclusive_scan<kScanBlock / 64>(vertex_flag(a, i), total, lds);
    if (threadIdx.x == 0 && blockIdx.x < a.vblocks) a.vsums[blockIdx.x] = total;
    block_exclusive_scan<kScanBlock / 64>(i < a.nt ? a.texcl[i] : 0u, total, lds);
    if (threadIdx.x == 0 && blockIdx.x < a.tblocks) a.tsums[blockIdx.x] = total;
}

// texcl[i] holds triangle i's kept flag on entry and its rank on exit: each lane reads and writes its own element
__global__ __launch_bounds__(kSpBlock) void k_sp_rank(const SpArgs a) {
    __shared__ unsigned lds[kSpBlock / 64];
    const unsigned i = blockIdx.x * kSpBlock + threadIdx.x;
    unsigned total;
    const unsigned vmine = block_exclusive_scan<kScanBlock / 64>(vertex_flag(a, i), total, lds);
    if (i < a.nv) a.vexcl[i] = a.vsums[blockIdx.x] + vmine;
    const unsigned tmine = block_exclusive_scan<kScanBlock / 64>(i < a.nt ? a.texcl[i] : 0u, total, lds);
    if (i < a.nt) a.texcl[i] = a.tsums[blockIdx.x] + tmine;
}

// clusters before vertex b: the scanned sum of b's workgroup and at most kSpBlock - 1 flags behind it
__device__ __forceinline__ unsigned crank_at(const SpArgs& a, unsigned long long b) {
    if (b >= a.nv) return a.csums[a.vblocks];
    const unsigned blk = static_cast<unsigned>(b) / kSpBlock;
    unsigned r = a.csums[blk];
    for (unsigned i = blk * kSpBlock; i < b; ++i) r += is_first(a, i) ? 1u : 0u;
    return r;
}

struct SpCounts {
    uint32_t* keptCounts;           // 2 n: vertices, triangles
    unsigned long long* keptBases;  // 2 (n + 1) interleaved or nullptr
    uint32_t* clusters;             // n or nullptr
};

// per model: a model's clusters, kept vertices and kept triangles lie in its own ranges, so its kept ranges start
// at the ranks of its bases
__global__ __launch_bounds__(kSpBlock) void k_sp_bases(const SpArgs a, const MeshTable md, const SpCounts out) {
    const unsigned i = blockIdx.x * kSpBlock + threadIdx.x;
    if (i > md.n) return;
    kept_ranges(a, md, i, out.keptCounts, out.keptBases);
    if (i < md.n && out.clusters)
        out.clusters[i] = crank_at(a, vertex_base(a.nv, md, i + 1)) - crank_at(a, vertex_base(a.nv, md, i));
}

// the mean of `count` Q20 values whose sum is `sum`
__device__ __forceinline__ float mean_q20(long long sum, unsigned count) {
    return static_cast<float>((static_cast<double>(sum) / static_cast<double>(count)) * 0x1p-20);
}

__global__ __launch_bounds__(kSpBlock) void k_sp_emit(const SpArgs a, const MeshTable md, const MeshArrays e) {
    const unsigned i = blockIdx.x * kSpBlock + threadIdx.x;
    if (i < a.nv) {
        const unsigned r = a.vexcl[i];
        if (a.vrank_at(static_cast<unsigned long long>(i) + 1) != r) {  // a kept first: the rank steps behind it
            const unsigned count = a.count[i];
            const long long* s = a.sums + 9 * static_cast<size_t>(i);
            if (count <= 1u) {  // alone: its own bits
                copy_vertex(e, i, r);
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    e.kv[3 * static_cast<size_t>(r) + j] = mean_q20(s[j], count);
                    e.kn[3 * static_cast<size_t>(r) + j] = mean_q20(s[3 + j], count);
                }
                if (e.c) {
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        e.kc[3 * static_cast<size_t>(r) + j] = static_cast<uint8_t>(
                            (2ull * static_cast<unsigned long long>(s[6 + j]) + count) / (2ull * count));
                }
            }
        }
    }
    rewrite_triangle(a, md, e, i, [&](unsigned g) { return a.vexcl[a.rep[g]]; });
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

// The bound include/emf_hip.h declares: under 137 bytes per vertex + 5 per triangle + 8 KiB.
size_t emf_hip_meshSimplifyScratchBytes(uint64_t vertices, uint64_t triangles) {
    if (vertices > (1ull << 30) || triangles >= (1ull << 31)) return 0;
    SpArgs a;
    char origin[16];
    (void)origin;
    return place(a, vertices, triangles, origin);  // only the offsets are used
}

int emf_hip_meshSimplifyCount(const float* vertices, const float* normals, const uint8_t* colors,
                              const int32_t* triangles, uint64_t nVertices, uint64_t nTriangles,
                              const uint64_t* tri_bases_dev, const uint64_t* vertex_bases_dev, int n, const float* cells,
                              const float origin[3], void* simplify_scratch_dev, uint32_t* kept_counts,
                              uint64_t* kept_bases, uint32_t* clusters, emf_stream_t stream) {
    const char* what = "meshSimplifyCount";
    EMF_TRY(check_sizes(nVertices, nTriangles, n, "", what));
    EMF_TRY(check_no_orphans(nVertices, nTriangles, what));
    EMF_REQUIRE_PTR(simplify_scratch_dev);
    EMF_REQUIRE_PTR(kept_counts);
    EMF_REQUIRE_PTR(cells);
    if ((tri_bases_dev == nullptr) != (vertex_bases_dev == nullptr))
        return fail(EMF_E_NULL, "%s: tri_bases_dev and vertex_bases_dev go together", what);
    if (!tri_bases_dev && n != 1) return fail(EMF_E_ARG, "%s: %d models need their bases", what, n);
    if (nVertices) {
        EMF_REQUIRE_PTR(vertices);
        EMF_REQUIRE_PTR(normals);
    }
    if (nTriangles) EMF_REQUIRE_PTR(triangles);
    SpCells c;
    for (int k = 0; k < EMF_MAX_MODELS; ++k) c.cell[k] = k < n ? cells[k] : 0.0f;
    for (int j = 0; j < 3; ++j) c.origin[j] = origin ? origin[j] : 0.0f;
    for (int k = 0; k < n; ++k)
        if (c.cell[k] != c.cell[k] || c.cell[k] > 3.0e38f) return fail(EMF_E_ARG, "%s: cell %d is not finite", what, k);
    for (int j = 0; j < 3; ++j)
        if (!(c.origin[j] >= -3.0e38f && c.origin[j] <= 3.0e38f)) return fail(EMF_E_ARG, "%s: the origin is not finite", what);
    SpArgs a;
    place(a, nVertices, nTriangles, simplify_scratch_dev);
    EMF_TRY(memset_async(a.flag, 0, sizeof(unsigned), stream, what));
    if (nVertices == 0) {  // empty meshes: zero counts, zero bases, no launch
        EMF_TRY(memset_async(kept_counts, 0, sizeof(uint32_t) * 2 * n, stream, what));
        if (kept_bases) EMF_TRY(memset_async(kept_bases, 0, sizeof(uint64_t) * 2 * (n + 1), stream, what));
        if (clusters) EMF_TRY(memset_async(clusters, 0, sizeof(uint32_t) * n, stream, what));
        return EMF_OK;
    }
    // keys and first indices are contiguous: all bits set = empty slot, no first yet; so are the counts, the marks
    // and the sums: zero
    EMF_TRY(memset_async(a.tkeys, 0xff, reinterpret_cast<char*>(a.rep) - reinterpret_cast<char*>(a.tkeys), stream, what));
    EMF_TRY(memset_async(a.count, 0, reinterpret_cast<char*>(a.vexcl) - reinterpret_cast<char*>(a.count), stream, what));
    const MeshTable md = mesh_table(tri_bases_dev, vertex_bases_dev, n);
    const SpCounts out{kept_counts, reinterpret_cast<unsigned long long*>(kept_bases), clusters};
    const dim3 block(kSpBlock), vgrid(a.vblocks), items(items_blocks(a));
    hipLaunchKernelGGL(k_sp_insert, vgrid, block, 0, as_stream(stream), a, md, c, vertices);
    hipLaunchKernelGGL(k_sp_accumulate, vgrid, block, 0, as_stream(stream), a, vertices, normals, colors);
    hipLaunchKernelGGL(k_sp_mark, items, block, 0, as_stream(stream), a, md, c, triangles);
    hipLaunchKernelGGL(k_sp_flags, items, block, 0, as_stream(stream), a);
    hipLaunchKernelGGL(k_sums_scan, dim3(3), dim3(kSumsBlock), 0, as_stream(stream),
                       SumsArrays{a.csums, a.vsums, a.tsums, a.vblocks, a.vblocks, a.tblocks});
    hipLaunchKernelGGL(k_sp_rank, items, block, 0, as_stream(stream), a);
    hipLaunchKernelGGL(k_sp_bases, dim3(ceil_div(n + 1, kSpBlock)), block, 0, as_stream(stream), a, md, out);
    return launch_status(what);
}

int emf_hip_meshSimplifyStatus(const void* simplify_scratch_dev, uint64_t nVertices, uint64_t nTriangles,
                               emf_stream_t stream) {
    EMF_REQUIRE_PTR(simplify_scratch_dev);
    EMF_TRY(check_sizes(nVertices, nTriangles, 1, "", "meshSimplifyStatus"));
    EMF_TRY(check_no_orphans(nVertices, nTriangles, "meshSimplifyStatus"));
    SpArgs a;
    place(a, nVertices, nTriangles, const_cast<void*>(simplify_scratch_dev));
    unsigned flag;
    EMF_TRY(read_flag(a.flag, flag, stream, "meshSimplifyStatus"));
    if (flag & kFlagLimit)
        return fail(EMF_E_LIMIT, "meshSimplify: a vertex is not finite, lies 2^10 m or more from zero or in a cell outside "
                                 "[-2^15, 2^15), or the table overflowed (scratch of another size?)");
    if (flag & kFlagArg) return fail(EMF_E_ARG, "meshSimplify: a triangle index lies outside its model's vertices");
    return EMF_OK;
}

int emf_hip_meshSimplifyEmit(const void* simplify_scratch_dev, uint64_t nVertices, uint64_t nTriangles,
                             const uint64_t* tri_bases_dev, const uint64_t* vertex_bases_dev, int n, const float* vertices,
                             const float* normals, const uint8_t* colors, const int32_t* triangles, float* kept_vertices,
                             float* kept_normals, uint8_t* kept_colors, int32_t* kept_triangles, emf_stream_t stream) {
    const char* what = "meshSimplifyEmit";
    EMF_TRY(check_sizes(nVertices, nTriangles, n, "", what));
    EMF_TRY(check_no_orphans(nVertices, nTriangles, what));
    if (nVertices == 0) return EMF_OK;
    const MeshArrays e{vertices, normals, colors, triangles, kept_vertices, kept_normals, kept_colors, kept_triangles};
    EMF_TRY(check_emit_arrays(simplify_scratch_dev, e, nTriangles, what));
    if ((tri_bases_dev == nullptr) != (vertex_bases_dev == nullptr))
        return fail(EMF_E_NULL, "%s: tri_bases_dev and vertex_bases_dev go together", what);
    if (!tri_bases_dev && n != 1) return fail(EMF_E_ARG, "%s: %d models need their bases", what, n);
    EMF_TRY(check_emit_pairs(e, false, nTriangles, "kept", "input mesh's", what));
    SpArgs a;
    place(a, nVertices, nTriangles, const_cast<void*>(simplify_scratch_dev));
    hipLaunchKernelGGL(k_sp_emit, dim3(items_blocks(a)), dim3(kSpBlock), 0, as_stream(stream), a,
                       mesh_table(tri_bases_dev, vertex_bases_dev, n), e);
    return launch_status(what);
}

}  // extern "C"
