// mesh_table.hpp -- what the mesh post-passes share (mesh_weld.hip, mesh_components.hip, mesh_simplify.hip; DESIGN.md
// 5.18c): the table of indexed meshes a launch works on, the open-addressing key table, the compaction of kept
// vertices and triangles by rank, and the host-side checks of the entries.  mesh_core.hpp is about marching-cubes
// geometry; nothing here sees a volume.  Nothing here branches on which pass calls it.
#pragma once

#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {

// ---- table and range ----------------------------------------------------------------------------------------------

// the models of a table launch (device arrays in the layout meshCountBatched, the weld and the filter leave) or, for
// one model, none: both null, the model's vertices are [0, nv) and its triangles [0, nt)
struct MeshTable {
    const unsigned long long* triBases;     // 2 (n + 1) interleaved: the triangle bases are the odd entries
    const unsigned long long* vertexBases;  // n + 1
    unsigned n;
};

inline MeshTable mesh_table(const uint64_t* triBases, const uint64_t* vertexBases, int n) {
    return MeshTable{reinterpret_cast<const unsigned long long*>(triBases),
                     reinterpret_cast<const unsigned long long*>(vertexBases), static_cast<unsigned>(n)};
}

// the last model whose base is <= x (empty models share a base with their successor: the one that holds x wins)
__device__ __forceinline__ unsigned model_of(const unsigned long long* bases, unsigned stride, unsigned n,
                                             unsigned long long x) {
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (x >= bases[stride * mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct Range {
    unsigned model, lo, hi;  // the model's vertices are [lo, hi)
};

__device__ __forceinline__ Range range_of_model(const MeshTable& md, unsigned m) {
    return Range{m, static_cast<unsigned>(md.vertexBases[m]), static_cast<unsigned>(md.vertexBases[m + 1])};
}

__device__ __forceinline__ Range range_of_vertex(unsigned nv, const MeshTable& md, unsigned g) {
    if (!md.vertexBases) return Range{0u, 0u, nv};
    return range_of_model(md, model_of(md.vertexBases, 1, md.n, g));
}

__device__ __forceinline__ Range range_of_triangle(unsigned nv, const MeshTable& md, unsigned t) {
    if (!md.vertexBases) return Range{0u, 0u, nv};
    return range_of_model(md, model_of(md.triBases + 1, 2, md.n, t));
}

// model i's first vertex / triangle, i in [0, n]: i == n gives the ends
__device__ __forceinline__ unsigned long long vertex_base(unsigned nv, const MeshTable& md, unsigned i) {
    return md.vertexBases ? md.vertexBases[i] : (i == 0 ? 0ull : nv);
}
__device__ __forceinline__ unsigned long long triangle_base(unsigned nt, const MeshTable& md, unsigned i) {
    return md.vertexBases ? md.triBases[2 * i + 1] : (i == 0 ? 0ull : nt);
}

// the global indices of triangle t's corners; false (and nothing to dereference) if one lies outside its model's
// vertex range or past the nv vertices the scratch was laid out for
__device__ __forceinline__ bool corners(unsigned nv, const Range& r, const int32_t* tris, unsigned t, unsigned g[3]) {
    const int32_t* ti = tris + 4 * static_cast<size_t>(t);
    const unsigned hi = r.hi < nv ? r.hi : nv;
    bool ok = r.lo <= hi;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const unsigned long long x = static_cast<unsigned long long>(r.lo) + static_cast<unsigned>(ti[1 + j]);
        ok = ok && ti[1 + j] >= 0 && x < hi;
        g[j] = static_cast<unsigned>(x);
    }
    return ok;
}

// ---- key table ----------------------------------------------------------------------------------------------------
// 64-bit keys in an open-addressing table of `cap` slots; tfirst[slot] is the smallest index that carries the slot's
// key.  Which slot a key lands in depends on the order the lanes arrive; the minimum index per key does not.

constexpr unsigned long long kEmptyKey = ~0ull;  // no edge or cluster key has all bits set (slot < 256 sits at bit 48)
constexpr unsigned kNoSlot = ~0u;

// the table's capacity for nv keys: a power of two >= 2 nv (load factor <= 1/2)
inline unsigned capacity_for(unsigned long long nv) {
    unsigned long long cap = 64;
    while (cap < 2 * nv) cap <<= 1;
    return static_cast<unsigned>(cap);
}

// splitmix64's finaliser: neighbouring keys (edges 3 apart, adjacent cells) must not land in neighbouring slots
__device__ __forceinline__ unsigned hash_slot(unsigned long long k, unsigned mask) {
    k ^= k >> 30;
    k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27;
    k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return static_cast<unsigned>(k) & mask;
}

// Claim the key's slot (64-bit atomicCAS, linear probing bounded by cap) and atomicMin index i into it.  Returns the
// slot, or kNoSlot when the table cannot hold the key: a table that is too small is the caller's flag, not a spin.
__device__ __forceinline__ unsigned claim_slot(unsigned long long* tkeys, unsigned* tfirst, unsigned cap,
                                               unsigned long long key, unsigned i) {
    const unsigned mask = cap - 1u;
    unsigned h = hash_slot(key, mask);
    for (unsigned probe = 0; probe < cap; ++probe) {
        const unsigned long long seen = atomicCAS(tkeys + h, kEmptyKey, key);
        if (seen == kEmptyKey || seen == key) {
            atomicMin(tfirst + h, i);
            return h;
        }
        h = (h + 1u) & mask;
    }
    return kNoSlot;
}

// ---- compaction ---------------------------------------------------------------------------------------------------

// flags before element b of `count` (b past the end: all of them): excl as the rank kernels write it, sums scanned
// with the total behind its `blocks` entries
__device__ __forceinline__ unsigned rank_at(const unsigned* excl, const unsigned* sums, unsigned count, unsigned blocks,
                                            unsigned long long b) {
    return b < count ? excl[b] : sums[blocks];
}

// the ranks of the kept vertices and triangles of a filtering pass: the part of its scratch the shared code reads
struct Compaction {
    unsigned* vexcl;
    unsigned* texcl;
    unsigned* vsums;  // vblocks + 1
    unsigned* tsums;  // tblocks + 1
    unsigned nv, nt, vblocks, tblocks;
    // kept vertices before vertex b / kept triangles before triangle b
    __device__ __forceinline__ unsigned vrank_at(unsigned long long b) const { return rank_at(vexcl, vsums, nv, vblocks, b); }
    __device__ __forceinline__ unsigned trank_at(unsigned long long b) const { return rank_at(texcl, tsums, nt, tblocks, b); }
};

// the grid of a kernel whose thread i handles vertex i and triangle i
inline unsigned items_blocks(const Compaction& a) { return a.vblocks > a.tblocks ? a.vblocks : a.tblocks; }

// Thread i <= n of a bases kernel.  A model's kept vertices and triangles lie in its own ranges, so its kept ranges
// start at the ranks of its bases: keptBases (2 (n + 1) interleaved, or nullptr) and keptCounts (2 n).
__device__ __forceinline__ void kept_ranges(const Compaction& a, const MeshTable& md, unsigned i, uint32_t* keptCounts,
                                            unsigned long long* keptBases) {
    const unsigned rv = a.vrank_at(vertex_base(a.nv, md, i)), rt = a.trank_at(triangle_base(a.nt, md, i));
    if (keptBases) {
        keptBases[2 * i] = rv;
        keptBases[2 * i + 1] = rt;
    }
    if (i < md.n) {
        keptCounts[2 * i] = a.vrank_at(vertex_base(a.nv, md, i + 1)) - rv;
        keptCounts[2 * i + 1] = a.trank_at(triangle_base(a.nt, md, i + 1)) - rt;
    }
}

// the arrays of a mesh going in and of the mesh coming out (colours: both or neither)
struct MeshArrays {
    const float* v;
    const float* nrm;
    const uint8_t* c;
    const int32_t* t;
    float* kv;
    float* kn;
    uint8_t* kc;
    int32_t* kt;
};

// vertex `from` of the input becomes vertex `to` of the output: position, normal and colour, bit for bit
__device__ __forceinline__ void copy_vertex(const MeshArrays& e, size_t from, size_t to) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        e.kv[3 * to + j] = e.v[3 * from + j];
        e.kn[3 * to + j] = e.nrm[3 * from + j];
    }
    if (e.c) {
#pragma unroll
        for (int j = 0; j < 3; ++j) e.kc[3 * to + j] = e.c[3 * from + j];
    }
}

// Triangle i, if kept, goes to its rank with its corners rewritten to model-local kept indices; keptVertex(g) is the
// global kept index of the vertex that stands for global vertex g.
template <typename KeptVertex>
__device__ __forceinline__ void rewrite_triangle(const Compaction& a, const MeshTable& md, const MeshArrays& e, unsigned i,
                                                 KeptVertex keptVertex) {
    if (i >= a.nt) return;
    const unsigned r = a.texcl[i];
    if (a.trank_at(static_cast<unsigned long long>(i) + 1) == r) return;  // kept: the rank steps behind it
    const Range m = range_of_triangle(a.nv, md, i);
    unsigned g[3];
    if (!corners(a.nv, m, e.t, i, g)) return;  // (a kept triangle lies inside its model's range)
    const unsigned base = a.vrank_at(m.lo);
    int32_t* to = e.kt + 4 * static_cast<size_t>(r);
    to[0] = 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) to[1 + j] = static_cast<int32_t>(keptVertex(g[j]) - base);
}

// up to three arrays of per-workgroup sums, each with room for its total behind its n entries
struct SumsArrays {
    unsigned* sums0;
    unsigned* sums1;
    unsigned* sums2;
    unsigned n0, n1, n2;
};

// one workgroup per array (the grid is the number of arrays): sums[b] := sum of sums[0 .. b), sums[n] := the total
static __global__ __launch_bounds__(kSumsBlock) void k_sums_scan(const SumsArrays a) {
    __shared__ unsigned lds[kSumsBlock / 64];
    unsigned* sums = blockIdx.x == 0 ? a.sums0 : (blockIdx.x == 1 ? a.sums1 : a.sums2);
    const unsigned n = blockIdx.x == 0 ? a.n0 : (blockIdx.x == 1 ? a.n1 : a.n2);
    const unsigned total = scan_sums(sums, 0u, n, lds);
    if (threadIdx.x == 0) sums[n] = total;
}

// ---- the host side of the entries ---------------------------------------------------------------------------------

// the sizes every entry refuses first; noun: what the vertices are in the caller's message ("soup", "welded", "")
inline int check_sizes(unsigned long long nv, unsigned long long nt, int n, const char* noun, const char* what) {
    if (nv > (1ull << 30)) return fail(EMF_E_LIMIT, "%s: %llu %svertices (at most 2^30)", what, nv, noun);
    if (nt >= (1ull << 31)) return fail(EMF_E_LIMIT, "%s: %llu triangles (below 2^31)", what, nt);
    if (n < 1 || n > EMF_MAX_MODELS) return fail(EMF_E_LIMIT, "%s: %d models (1 .. %d per launch)", what, n, EMF_MAX_MODELS);
    return EMF_OK;
}

inline int check_no_orphans(unsigned long long nv, unsigned long long nt, const char* what) {
    if (nv == 0 && nt != 0) return fail(EMF_E_ARG, "%s: %llu triangles over no vertex", what, nt);
    return EMF_OK;
}

// the arrays an emit entry needs once there are vertices (scratch: the pass's own)
inline int check_emit_arrays(const void* scratch, const MeshArrays& e, unsigned long long nt, const char* what) {
    const void* need[] = {scratch, e.v, e.nrm, e.kv, e.kn, nt ? e.t : scratch, nt ? e.kt : scratch};
    const char* names[] = {"the scratch", "vertices", "normals", "the output vertices", "the output normals", "triangles",
                           "the output triangles"};
    for (int k = 0; k < 7; ++k)
        if (!need[k]) return fail(EMF_E_NULL, "%s: %s is NULL", what, names[k]);
    return EMF_OK;
}

// colours come in and go out together, and no output array is its input (triangles: only where the pass cannot
// rewrite in place); out / in name the two meshes in the messages
inline int check_emit_pairs(const MeshArrays& e, bool trianglesInPlace, unsigned long long nt, const char* out,
                            const char* in, const char* what) {
    if ((e.c == nullptr) != (e.kc == nullptr)) return fail(EMF_E_NULL, "%s: colors and %s_colors go together", what, out);
    if (e.kv == e.v || e.kn == e.nrm || (e.c && e.kc == e.c) || (!trianglesInPlace && nt && e.kt == e.t))
        return fail(EMF_E_ARG, "%s: the %s arrays must not alias the %s", what, out, in);
    return EMF_OK;
}

// a Status entry's read-back of the pass's flag word: waits for the stream
inline int read_flag(const unsigned* flagDev, unsigned& flag, emf_stream_t stream, const char* what) {
    flag = 0;
    hipError_t e = hipMemcpyAsync(&flag, flagDev, sizeof(flag), hipMemcpyDeviceToHost, as_stream(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return static_cast<int>(e);
    }
    return EMF_OK;
}

}  // namespace emf_hip
