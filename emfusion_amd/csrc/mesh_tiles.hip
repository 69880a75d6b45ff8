// mesh_tiles.hip -- marching cubes over a sparse SET of integration tiles on one integer lattice (include/emf_hip.h
// "Meshing a set of tiles"): the mesh of the dense volume that holds exactly the listed tiles and is
// unobserved everywhere else, without that volume ever existing.
//
// A tile is 32 x 8 x 8 voxels and comes in one of four representations per array (all zero, one repeated element, a
// literal in an arena, in place in a dense volume); the table is sorted and every entry names its 7 neighbours on
// the + side, so no kernel searches.  One workgroup of 256 lanes per listed tile, in every pass:
//   stage     the tile's tsdf with its +2 halo (34 x 10 x 10 floats; +1 where no normal is made) and "weight > 0" with
//             the +1 halo (33 x 9 x 9 bytes) go to LDS once.  The tile's own 2048 voxels come by 16-byte loads (a
//             literal, or rows of the dense volume); the halo, 1352 voxels of up to 7 neighbours of whatever class,
//             by scalar loads.  A neighbour that is not listed reads as tsdf 0, weight 0.
//   classify  lane l owns the cubes anchored at (l & 31, l >> 5, j), j = 0 .. 7: cube j * 256 + l of the tile's
//             (z, y, x) order; rows of 34 floats keep the 32 lanes of a half-wave on 32 different banks.
//   k_tiles<kCount>  per (j, wave) the packed (vertices | triangles << 16) sum, per tile their total -> vertBase[t],
//             triBase[t].  A tile owns at most 24576 vertices and 10240 triangles: 16 + 16 bits.
//   k_tiles_scan     one workgroup: both arrays become their exclusive scans, entry n the totals (wave_ops.hpp)
//   k_tiles<kEmit / kColors / kKeys>  a tile without surface returns before it stages anything; the others classify
//             again, scan inside the workgroup (wave shuffles + 32 LDS words) and write where the canonical order
//             puts them: tiles in table order, cubes in (z, y, x) order, vertices in edge-bit order.
// No atomics, no scratch memory, no device hash table.  What the table says is believed only as far as it can be
// checked: an entry whose literal leaves the arena or whose in-place tile leaves the volume, and a neighbour index
// that does not name the tile at the neighbouring coordinate, count as "not listed" and are never dereferenced.
#include "mesh_core.hpp"
#include "tile_table.hpp"
#include "wave_ops.hpp"

#include "mc_tables.h"

namespace emf_hip {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTilesBlock = 256;
constexpr int kVX = kTX + 1, kVY = kTY + 1, kVZ = kTZ + 1;  // the "weight > 0" image: +1 halo

static_assert(sizeof(emf_mesh_tile_t) == 88, "emf_mesh_tile_t layout is mirrored in _lib.py");
static_assert(sizeof(emf_mesh_tiles_source_t) == 64, "emf_mesh_tiles_source_t layout is mirrored in _lib.py");

enum Mode { kCount, kEmit, kColors, kKeys };

struct TilesArgs {
    const emf_mesh_tile_t* tiles;
    unsigned n;
    const unsigned* arena;
    unsigned long long arenaUnits;
    const unsigned* vT;  // the dense volume of class 3
    const unsigned* vW;
    const ushort4* vC;
    unsigned long long volElems, row, plane;
    unsigned* vertBase;  // [n + 1]: per-tile totals, after k_tiles_scan their exclusive scan and the total
    unsigned* triBase;   // [n + 1]
    unsigned* cubes;     // [n]: surface cubes the tile owns (written by the count, never scanned)
    emf_mesh_counts_t* counts;
    V3 half;
    float voxelSize;
    float* vertices;
    float* normals;
    int32_t* triangles;
    uint8_t* colors;
    unsigned long long* keys;
};

// What a workgroup keeps of the tile itself (k = 0) and of its 7 neighbours: k = dx | dy << 1 | dz << 2.  A literal and
// an in-place array are the same thing to the readers: a base and two strides (32 and 256 voxels in the arena).
struct Ent {
    int idx;  // -1: not listed, or skipped
    unsigned cls[3];
    unsigned w[4];
    const unsigned* base[3];  // class 2 and 3: the array's first voxel of this tile
    unsigned long long row[3], plane[3];
};

// array k of entry e can be read: its literal lies inside the arena, its in-place tile inside the volume.  Plain
// boolean arithmetic, no early return: every lane evaluates everything.
__device__ __forceinline__ bool array_ok(const TilesArgs& a, unsigned c, unsigned long long at, int k) {
    const unsigned long long units = k == 2 ? 2ull : 1ull;
    const bool literal = at <= a.arenaUnits && a.arenaUnits - at >= units;
    const void* v = k == 0 ? static_cast<const void*>(a.vT) : (k == 1 ? static_cast<const void*>(a.vW) : static_cast<const void*>(a.vC));
    // the tile's last voxel: 7 planes, 7 rows and 31 voxels further (the strides are bounded by the host)
    const unsigned long long span = 7ull * a.plane + 7ull * a.row + 32ull;
    const bool inplace = v != nullptr && (at & 3ull) == 0ull && at <= a.volElems && a.volElems - at >= span;
    return c <= 1u || (c == 2u && literal) || (c == 3u && inplace);
}

__device__ __forceinline__ void load_ents(const TilesArgs& a, unsigned t, Ent* ents) {
    const int k = threadIdx.x;
    if (k >= 8) return;
    const emf_mesh_tile_t* self = a.tiles + t;
    const int named = k == 0 ? static_cast<int>(t) : self->nbr[k > 0 ? k - 1 : 0];
    const bool listed = named >= 0 && static_cast<unsigned>(named) < a.n;
    const emf_mesh_tile_t* e = a.tiles + (listed ? static_cast<unsigned>(named) : t);  // always a readable entry
    Ent en;
    bool ok = listed;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const unsigned c = e->cls[i];
        const unsigned long long at = e->at[i];
        const unsigned step = (static_cast<unsigned>(k) >> i) & 1u;
        ok = ok & (static_cast<unsigned>(e->coord[i]) == static_cast<unsigned>(self->coord[i]) + step);
        ok = ok & array_ok(a, c, at, i);
        const unsigned long long words = i == 2 ? 2ull : 1ull;  // per voxel
        const unsigned* vol = i == 0 ? a.vT : (i == 1 ? a.vW : reinterpret_cast<const unsigned*>(a.vC));
        en.cls[i] = c;
        en.base[i] = c == 2u ? a.arena + at * kUnitWords : vol + at * words;  // (read only when ok and c >= 2)
        en.row[i] = c == 2u ? static_cast<unsigned long long>(kTX) : a.row;
        en.plane[i] = c == 2u ? static_cast<unsigned long long>(kTX * kTY) : a.plane;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) en.w[i] = e->words[i];
    en.idx = ok ? named : -1;
    ents[k] = en;
}

// voxel (lx, ly, lz) of array k of the tile behind `en`, in voxels from en.base[k]
__device__ __forceinline__ unsigned long long voxel_at(const Ent& en, int k, int lx, int ly, int lz) {
    return static_cast<unsigned long long>(lz) * en.plane[k] + static_cast<unsigned long long>(ly) * en.row[k] +
           static_cast<unsigned long long>(lx);
}

// word of array k (0 tsdf, 1 weights) of voxel (lx, ly, lz) of the tile behind `en`
__device__ __forceinline__ unsigned tile_word(const Ent& en, int k, int lx, int ly, int lz) {
    unsigned r = en.cls[k] == 1u ? en.w[k] : 0u;
    if (en.idx >= 0 && en.cls[k] >= 2u) r = en.base[k][voxel_at(en, k, lx, ly, lz)];
    return en.idx >= 0 ? r : 0u;
}

__device__ __forceinline__ ushort4 tile_colour(const Ent& en, int lx, int ly, int lz) {
    const bool one = en.idx >= 0 && en.cls[2] == 1u;
    ushort4 r = make_ushort4(one ? en.w[2] & 0xffffu : 0u, one ? en.w[2] >> 16 : 0u, one ? en.w[3] & 0xffffu : 0u,
                             one ? en.w[3] >> 16 : 0u);
    if (en.idx >= 0 && en.cls[2] >= 2u) r = reinterpret_cast<const ushort4*>(en.base[2])[voxel_at(en, 2, lx, ly, lz)];
    return r;
}

// this lane's four voxels (x = 4 (lane & 7) .., y = lane >> 3 & 7, z = (lane >> 6) + 4 g) of the tile's own array k
__device__ __forceinline__ u32x4 own_words(const Ent& en, int k, int g) {
    const int lx = 4 * (threadIdx.x & 7), ly = (threadIdx.x >> 3) & 7, lz = (threadIdx.x >> 6) + 4 * g;
    const unsigned w = en.cls[k] == 1u ? en.w[k] : 0u;
    u32x4 r = {w, w, w, w};
    if (en.cls[k] >= 2u) r = *reinterpret_cast<const u32x4*>(en.base[k] + voxel_at(en, k, lx, ly, lz));
    return r;
}

// tsdf with a halo of kH voxels and "weight > 0" with a halo of 1 -> LDS.  All lanes call together, after load_ents.
template <int kH>
__device__ __forceinline__ void stage(const TilesArgs& a, const Ent* ents, float* sT, uint8_t* sV) {
    constexpr int SX = kTX + kH, SY = kTY + kH, SZ = kTZ + kH;
    const Ent& self = ents[0];
    {  // the tile's own voxels
        const int lx = 4 * (threadIdx.x & 7), ly = (threadIdx.x >> 3) & 7;
        u32x4 t[2], w[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            t[g] = own_words(self, 0, g);
            w[g] = own_words(self, 1, g);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int lz = (threadIdx.x >> 6) + 4 * g;
            float* dT = sT + (lz * SY + ly) * SX + lx;
            uint8_t* dV = sV + (lz * kVY + ly) * kVX + lx;
            dT[0] = __uint_as_float(t[g].x);
            dT[1] = __uint_as_float(t[g].y);
            dT[2] = __uint_as_float(t[g].z);
            dT[3] = __uint_as_float(t[g].w);
            dV[0] = __uint_as_float(w[g].x) > 0.f;
            dV[1] = __uint_as_float(w[g].y) > 0.f;
            dV[2] = __uint_as_float(w[g].z) > 0.f;
            dV[3] = __uint_as_float(w[g].w) > 0.f;
        }
    }
    // the halo: what lies at x >= 32, y >= 8 or z >= 8 belongs to neighbour (x >= 32) | (y >= 8) << 1 | (z >= 8) << 2
    for (int i = threadIdx.x; i < SX * SY * SZ; i += kTilesBlock) {
        const int x = i % SX, r = i / SX, y = r % SY, z = r / SY;
        const int k = (x >= kTX ? 1 : 0) | (y >= kTY ? 2 : 0) | (z >= kTZ ? 4 : 0);
        if (k == 0) continue;
        const int lx = x & (kTX - 1), ly = y & (kTY - 1), lz = z & (kTZ - 1);
        const Ent& en = ents[k];
        sT[i] = __uint_as_float(tile_word(en, 0, lx, ly, lz));
        if (x < kVX && y < kVY && z < kVZ) sV[(z * kVY + y) * kVX + x] = __uint_as_float(tile_word(en, 1, lx, ly, lz)) > 0.f;
    }
    __syncthreads();
}

// class of the cube anchored at (x, y, z) of the tile: 0 when a corner is unobserved or there is no surface
template <int kH>
__device__ __forceinline__ unsigned cube_class(const float* sT, const uint8_t* sV, int x, int y, int z) {
    constexpr int SX = kTX + kH, SY = kTY + kH;
    bool valid = true;
    unsigned cls = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int dx, dy, dz;
        cube_corner(i, dx, dy, dz);
        valid = valid && sV[((z + dz) * kVY + y + dy) * kVX + x + dx] != 0;
        cls |= (sT[((z + dz) * SY + y + dy) * SX + x + dx] < 0.f ? 1u : 0u) << i;
    }
    return (!valid || cls == 255u) ? 0u : cls;
}

__device__ __forceinline__ unsigned triangles_of(unsigned cls) {
    unsigned n = 0;
    while (n < 5 && emf_mc_tri_table[cls][3 * n] >= 0) ++n;
    return n;
}

// vertices | triangles << 16 of a cube
__device__ __forceinline__ unsigned packed_counts(unsigned cls) {
    return cls ? static_cast<unsigned>(__popc(active_edges(cls))) | (triangles_of(cls) << 16) : 0u;
}

// Per (plane j, wave) the packed sum -> sTot[j * 4 + wave]; then their exclusive scan in place and the tile's total in
// sTot[32].  Fields cannot carry: a wave holds at most 768 vertices and 320 triangles, a tile 24576 and 10240.
template <int kH>
__device__ __forceinline__ void tile_totals(const float* sT, const uint8_t* sV, unsigned* sTot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = threadIdx.x & (kTX - 1), y = threadIdx.x >> 5;
    unsigned cubes = 0;  // (wave-uniform) surface cubes of this wave
#pragma unroll 1
    for (int j = 0; j < kTZ; ++j) {
        unsigned p = packed_counts(cube_class<kH>(sT, sV, x, y, j));
        const unsigned long long surface = __ballot(p != 0u);
        cubes += static_cast<unsigned>(__popcll(surface));
        if (surface != 0ull) p = wave_reduce<OpAdd>(p);  // wave-uniform: most waves hold no surface
        if (lane == 0) sTot[j * 4 + wave] = p;
    }
    if (lane == 0) sTot[33 + wave] = cubes;
    __syncthreads();
    if (threadIdx.x < 64) {
        const unsigned v = threadIdx.x < 32 ? sTot[threadIdx.x] : 0u;
        const unsigned inc = wave_inclusive_scan(v);
        if (threadIdx.x < 32) sTot[threadIdx.x] = inc - v;
        if (threadIdx.x == 31) sTot[32] = inc;
    }
    __syncthreads();
}

struct CubeOut {
    int x, y, z;         // the anchor inside the tile
    unsigned cls, edges, ntris;
    unsigned vb, tb;     // global first vertex / triangle of the cube
};

template <int kH>
__device__ __forceinline__ void emit_cube(const TilesArgs& a, const float* sT, const int lat[3], const CubeOut& q) {
    constexpr int SX = kTX + kH, SY = kTY + kH, SZ = kTZ + kH;
    static_assert(kH >= 2, "a corner's forward differences read one voxel beyond the +1 halo");
    (void)SZ;
    int offsets[12];
    unsigned k = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        offsets[e] = 0;
        if (!((q.edges >> e) & 1u)) continue;
        V3 p[2], g[2];
        float val[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int dx, dy, dz;
            cube_corner(emf_mc_edge_corner[e][s], dx, dy, dz);
            const int cx = q.x + dx, cy = q.y + dy, cz = q.z + dz;
            const int idx = (cz * SY + cy) * SX + cx;
            val[s] = sT[idx];
            p[s] = v3((static_cast<float>(lat[0] + cx) - a.half.x) * a.voxelSize,
                      (static_cast<float>(lat[1] + cy) - a.half.y) * a.voxelSize,
                      (static_cast<float>(lat[2] + cz) - a.half.z) * a.voxelSize);
            // what kernel_computeTSDFGrads stores away from the last planes; the next voxel is in the halo
            g[s] = v3(sT[idx + 1] - val[s], sT[idx + SX] - val[s], sT[idx + SX * SY] - val[s]);
        }
        const V3 pv = vertex_interp(p[0], p[1], val[0], val[1]);
        const V3 nv = vertex_interp(g[0], g[1], val[0], val[1]);  // not normalised: Q19
        float* vo = a.vertices + 3 * static_cast<size_t>(q.vb + k);
        float* no = a.normals + 3 * static_cast<size_t>(q.vb + k);
        vo[0] = pv.x;
        vo[1] = pv.y;
        vo[2] = pv.z;
        no[0] = nv.x;
        no[1] = nv.y;
        no[2] = nv.z;
        offsets[e] = static_cast<int>(k++);
    }
    for (unsigned t = 0; t < q.ntris; ++t) {
        int32_t* to = a.triangles + 4 * static_cast<size_t>(q.tb + t);
        to[0] = 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = emf_mc_tri_table[q.cls][3 * t + j];
            int o = 0;  // offsets[e] without a dynamically indexed register array
#pragma unroll
            for (int i = 0; i < 12; ++i) o = e == i ? offsets[i] : o;
            to[1 + j] = static_cast<int32_t>(q.vb + static_cast<unsigned>(o));  // global
        }
    }
}

template <int kH>
__device__ __forceinline__ void color_cube(const TilesArgs& a, const float* sT, const Ent* ents, const CubeOut& q) {
    constexpr int SX = kTX + kH, SY = kTY + kH;
    unsigned k = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!((q.edges >> e) & 1u)) continue;
        float val[2];
        ushort4 c[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int dx, dy, dz;
            cube_corner(emf_mc_edge_corner[e][s], dx, dy, dz);
            const int cx = q.x + dx, cy = q.y + dy, cz = q.z + dz;
            val[s] = sT[(cz * SY + cy) * SX + cx];
            const int nb = (cx >= kTX ? 1 : 0) | (cy >= kTY ? 2 : 0) | (cz >= kTZ ? 4 : 0);
            c[s] = tile_colour(ents[nb], cx & (kTX - 1), cy & (kTY - 1), cz & (kTZ - 1));
        }
        edge_colour(c[0], c[1], val[0], val[1], a.colors + 3 * static_cast<size_t>(q.vb + k));
        ++k;
    }
}

__device__ __forceinline__ void key_cube(const TilesArgs& a, const int lat[3], const CubeOut& q) {
    constexpr long long kBias = 1ll << kLatticeBits;
    unsigned k = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!((q.edges >> e) & 1u)) continue;
        int ax, ay, az, bx, by, bz;
        cube_corner(emf_mc_edge_corner[e][0], ax, ay, az);
        cube_corner(emf_mc_edge_corner[e][1], bx, by, bz);
        const int lx = ax < bx ? ax : bx, ly = ay < by ? ay : by, lz = az < bz ? az : bz;  // the lower voxel
        const unsigned axis = ax != bx ? 0u : (ay != by ? 1u : 2u);
        const unsigned long long X = static_cast<unsigned long long>(lat[0] + q.x + lx + kBias);
        const unsigned long long Y = static_cast<unsigned long long>(lat[1] + q.y + ly + kBias);
        const unsigned long long Z = static_cast<unsigned long long>(lat[2] + q.z + lz + kBias);
        a.keys[q.vb + k] = 3ull * ((Z << 40) | (Y << 20) | X) + axis;
        ++k;
    }
}

template <int kMode>
__global__ __launch_bounds__(kTilesBlock) void k_tiles(const TilesArgs a) {
    constexpr int kH = kMode == kEmit ? 2 : 1;
    constexpr int SX = kTX + kH, SY = kTY + kH, SZ = kTZ + kH;
    __shared__ float sT[SX * SY * SZ];
    __shared__ uint8_t sV[(kVX * kVY * kVZ + 3) & ~3];
    __shared__ Ent ents[8];
    __shared__ unsigned sTot[37];  // 32 (plane, wave) sums, their total, surface cubes per wave
    const unsigned t = blockIdx.x;
    if (t >= a.n) return;
    // (workgroup-uniform) a tile without surface costs the later passes two loads
    if (kMode != kCount && a.vertBase[t + 1] == a.vertBase[t]) return;
    load_ents(a, t, ents);
    __syncthreads();
    if (ents[0].idx < 0) {  // (uniform) a skipped tile owns nothing
        if (kMode == kCount && threadIdx.x == 0) {
            a.vertBase[t] = 0u;
            a.triBase[t] = 0u;
            a.cubes[t] = 0u;
        }
        return;
    }
    stage<kH>(a, ents, sT, sV);
    tile_totals<kH>(sT, sV, sTot);
    if (kMode == kCount) {
        if (threadIdx.x == 0) {
            a.vertBase[t] = sTot[32] & 0xffffu;
            a.triBase[t] = sTot[32] >> 16;
            a.cubes[t] = sTot[33] + sTot[34] + sTot[35] + sTot[36];
        }
        return;
    }
    const int wave = threadIdx.x >> 6;
    const emf_mesh_tile_t& self = a.tiles[t];
    const int lat[3] = {static_cast<int>(static_cast<unsigned>(self.coord[0]) * kTX),
                        static_cast<int>(static_cast<unsigned>(self.coord[1]) * kTY),
                        static_cast<int>(static_cast<unsigned>(self.coord[2]) * kTZ)};
    const unsigned vb = a.vertBase[t], tb = a.triBase[t];
    CubeOut q;
    q.x = threadIdx.x & (kTX - 1);
    q.y = threadIdx.x >> 5;
#pragma unroll 1
    for (int j = 0; j < kTZ; ++j) {
        q.z = j;
        q.cls = cube_class<kH>(sT, sV, q.x, q.y, j);
        const unsigned p = packed_counts(q.cls);
        if (__ballot(p != 0u) == 0ull) continue;  // wave-uniform
        const unsigned inc = wave_inclusive_scan(p);
        if (!q.cls) continue;
        const unsigned before = sTot[j * 4 + wave] + inc - p;
        q.edges = active_edges(q.cls);
        q.ntris = p >> 16;
        q.vb = vb + (before & 0xffffu);
        q.tb = tb + (before >> 16);
        if constexpr (kMode == kEmit) emit_cube<kH>(a, sT, lat, q);
        if constexpr (kMode == kColors) color_cube<kH>(a, sT, ents, q);
        if constexpr (kMode == kKeys) key_cube(a, lat, q);
    }
}

// both per-tile arrays become their exclusive scans, entry n the totals
__global__ __launch_bounds__(kSumsBlock) void k_tiles_scan(unsigned* vertBase, unsigned* triBase, unsigned n,
                                                           emf_mesh_counts_t* counts) {
    __shared__ unsigned lds[kSumsBlock / 64];
    const unsigned vertices = scan_sums(vertBase, 0u, n, lds);
    const unsigned triangles = scan_sums(triBase, 0u, n, lds);
    if (threadIdx.x == 0) {
        counts->vertices = vertBase[n] = vertices;
        counts->triangles = triBase[n] = triangles;
    }
}

// what every entry checks of its arguments, and the kernels' view of them
int prepare(TilesArgs& a, const emf_mesh_tile_t* tiles_dev, uint32_t n, const emf_mesh_tiles_source_t* source,
            const void* scratch_dev, const char* what) {
    if (n > kMaxTiles) return fail(EMF_E_LIMIT, "%s: %u tiles (at most %u per table)", what, n, kMaxTiles);
    EMF_REQUIRE_PTR(source);
    EMF_REQUIRE_PTR(scratch_dev);
    if (n) EMF_REQUIRE_PTR(tiles_dev);
    if ((reinterpret_cast<uintptr_t>(tiles_dev) & 7u) != 0 || (reinterpret_cast<uintptr_t>(scratch_dev) & 3u) != 0)
        return fail(EMF_E_ARG, "%s: tiles_dev or scratch_dev is misaligned", what);
    EMF_TRY(check_tiles_source(source, what));
    a = TilesArgs{};
    a.tiles = tiles_dev;
    a.n = n;
    a.arena = static_cast<const unsigned*>(source->arena);
    a.arenaUnits = source->arena ? source->arena_units : 0;
    a.vT = reinterpret_cast<const unsigned*>(source->tsdf);
    a.vW = reinterpret_cast<const unsigned*>(source->weights);
    a.vC = reinterpret_cast<const ushort4*>(source->color);
    a.volElems = source->tsdf ? source->volume_elements : 0;
    a.row = source->row_stride;
    a.plane = source->plane_stride;
    a.vertBase = static_cast<unsigned*>(const_cast<void*>(scratch_dev));
    a.triBase = a.vertBase + (static_cast<size_t>(n) + 1);
    a.cubes = a.triBase + (static_cast<size_t>(n) + 1);
    return EMF_OK;
}

// the table as the host sees it
int check_table(const emf_mesh_tile_t* th, uint32_t n, const emf_mesh_tiles_source_t* source) {
    for (uint32_t i = 0; i < n; ++i) {
        EMF_TRY(check_tile_entry(th, i, source, "meshTilesCount"));
        const emf_mesh_tile_t& e = th[i];
        for (int k = 1; k < 8; ++k) {
            const int32_t j = e.nbr[k - 1];
            if (j < -1 || (j >= 0 && static_cast<uint32_t>(j) >= n))
                return fail(EMF_E_ARG, "meshTilesCount: neighbour %d of tile %u is %d (-1 or below %u)", k, i, j, n);
            if (j >= 0 && (th[j].coord[0] != e.coord[0] + (k & 1) || th[j].coord[1] != e.coord[1] + ((k >> 1) & 1) ||
                           th[j].coord[2] != e.coord[2] + ((k >> 2) & 1)))
                return fail(EMF_E_ARG, "meshTilesCount: neighbour %d of tile %u names a tile at another coordinate", k, i);
        }
    }
    return EMF_OK;
}

template <int kMode>
int launch(const TilesArgs& a, emf_stream_t stream, const char* what) {
    if (a.n == 0) return EMF_OK;
    hipLaunchKernelGGL(k_tiles<kMode>, dim3(a.n), dim3(kTilesBlock), 0, as_stream(stream), a);
    return launch_status(what);
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

size_t emf_hip_meshTilesScratchBytes(uint32_t n) {
    if (n > kMaxTiles) return 0;
    return sizeof(unsigned) * (3 * static_cast<size_t>(n) + 2);
}

int emf_hip_meshTilesCount(const emf_mesh_tile_t* tiles_dev, const emf_mesh_tile_t* tiles_host, uint32_t n,
                           const emf_mesh_tiles_source_t* source, void* scratch_dev, emf_mesh_counts_t* counts_dev,
                           emf_stream_t stream) {
    TilesArgs a;
    EMF_TRY(prepare(a, tiles_dev, n, source, scratch_dev, "meshTilesCount"));
    EMF_REQUIRE_PTR(counts_dev);
    if (n) EMF_REQUIRE_PTR(tiles_host);
    EMF_TRY(check_table(tiles_host, n, source));
    a.counts = counts_dev;
    if (n) {
        hipLaunchKernelGGL(k_tiles<kCount>, dim3(n), dim3(kTilesBlock), 0, as_stream(stream), a);
        EMF_TRY(launch_status("meshTilesCount"));
    }
    hipLaunchKernelGGL(k_tiles_scan, dim3(1), dim3(kSumsBlock), 0, as_stream(stream), a.vertBase, a.triBase, n, counts_dev);
    return launch_status("meshTilesCount");
}

int emf_hip_meshTilesEmit(const emf_mesh_tile_t* tiles_dev, uint32_t n, const emf_mesh_tiles_source_t* source,
                          const float half[3], float voxelSize, const void* scratch_dev, float* vertices, float* normals,
                          int32_t* triangles, emf_stream_t stream) {
    TilesArgs a;
    EMF_TRY(prepare(a, tiles_dev, n, source, scratch_dev, "meshTilesEmit"));
    EMF_REQUIRE_PTR(half);
    if (!(voxelSize > 0.f)) return fail(EMF_E_ARG, "meshTilesEmit: voxelSize %g", static_cast<double>(voxelSize));
    if (n) {
        EMF_REQUIRE_PTR(vertices);
        EMF_REQUIRE_PTR(normals);
        EMF_REQUIRE_PTR(triangles);
    }
    a.half = v3_from(half);
    a.voxelSize = voxelSize;
    a.vertices = vertices;
    a.normals = normals;
    a.triangles = triangles;
    return launch<kEmit>(a, stream, "meshTilesEmit");
}

int emf_hip_meshTilesColors(const emf_mesh_tile_t* tiles_dev, uint32_t n, const emf_mesh_tiles_source_t* source,
                            const void* scratch_dev, uint8_t* colors, emf_stream_t stream) {
    TilesArgs a;
    EMF_TRY(prepare(a, tiles_dev, n, source, scratch_dev, "meshTilesColors"));
    if (n) EMF_REQUIRE_PTR(colors);
    a.colors = colors;
    return launch<kColors>(a, stream, "meshTilesColors");
}

int emf_hip_meshTilesEdgeKeys(const emf_mesh_tile_t* tiles_dev, uint32_t n, const emf_mesh_tiles_source_t* source,
                              const void* scratch_dev, uint64_t* keys, emf_stream_t stream) {
    TilesArgs a;
    EMF_TRY(prepare(a, tiles_dev, n, source, scratch_dev, "meshTilesEdgeKeys"));
    if (n) EMF_REQUIRE_PTR(keys);
    a.keys = reinterpret_cast<unsigned long long*>(keys);
    return launch<kKeys>(a, stream, "meshTilesEdgeKeys");
}

}  // extern "C"
