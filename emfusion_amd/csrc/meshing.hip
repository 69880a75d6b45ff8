// meshing.hip -- marching cubes over a TSDF volume: the mesh that
// TSDF::getMesh / ObjTSDF::getMesh hand to the PLY writer (reference TSDF.cu:855-1152,
// TSDF.cpp:356-373, ObjTSDF.cpp:247-268).
//
// The reference classifies every cube into three N^3-sized buffers (class u8, vertex count i32,
// triangle count i32 -- 9 bytes per voxel, 1.2 GB for the 512^3 background), sums them, runs two
// device-wide thrust::exclusive_scan passes over them and reads them back in the emit kernel.
// Here nothing per cube is stored.  The cube anchored at voxel (x, y, z) is visited in voxel order
// (= the reference's buffer order with empty slots where x, y or z is the last index) in chunks of
// 252 positions -- 4 waves of 63 cubes; lane 63 only lends its voxel to lane 62 -- and only per-chunk
// numbers go through memory (9 bytes per chunk):
//   k_mesh_count  a workgroup classifies 32 chunks (8 for small volumes).  A lane loads ITS voxel of the four rows
//                 (y, z), (y+1, z), (y, z+1), (y+1, z+1) -- 8 coalesced loads instead of 16
//                 gathers -- and the "observed" and "negative" predicates become 64-bit wave masks
//                 (a v_cmp each); the x+1 neighbour is the mask shifted by one, so which cubes are
//                 complete and which hold a sign change is a handful of SCALAR and / or / shift
//                 instructions per wave.  Only lanes with surface (rare) build their class.  Per
//                 chunk the packed (vertices, triangles) total -> chunkTot[g], per workgroup their
//                 sum -> blockSums[b], and the ids of the chunks that hold surface -> list[]
//   k_mesh_scan   one workgroup: exclusive scan of blockSums in place (wave_ops.hpp; 17 k pairs at 512^3), totals
//   k_mesh_emit   a fixed grid walks list[]: classify the chunk again, scan inside the workgroup (wave
//                 shuffles + LDS) on top of blockSums[g / 8] + the chunk totals before it, and write
//                 vertices, normals and triangles where the reference puts them
//   k_mesh_colors / k_mesh_keys  the emit's walk over list[] once more each (the same chunk_slot, hence the same vertex
//                 slots): u8 x 3 vertex colours from a colour volume; the u64 grid-edge key per vertex that
//                 mesh_weld.hip welds by (opt-in, the soup above is what it was)
// A launch covers a TABLE of volumes (emf_hip_mesh*Batched; the level-1 entries are its one-volume case): model m
// owns a contiguous range of counting workgroups (its own chunks-per-workgroup choice and XCD banding inside it),
// of per-workgroup sums and of chunks; the scan restarts at every model and yields its counts and 64-bit bases in
// the concatenated outputs, so model m's slice is exactly the mesh of that volume alone.  The ranges travel in the
// kernel arguments (MeshArgs), the volumes' pointers in the device model table.
// Each volume is streamed once (count) plus its surface chunks once more (emit; a workgroup per
// chunk that returns when its total is 0 measured 0.57 ms at 512^3 for launching 0.5 M workgroups
// alone).  Counting workgroups are mapped so that each XCD walks a contiguous eighth of the volume
// (its own z-slabs stay in its L2).
// The output is element-for-element the reference's: cubes in (z, y, x) order, a cube's vertices
// in edge-bit order, triangles as (3, i0, i1, i2) in table order.  Normals are the interpolated RAW
// gradients: the reference's `ns[i] /= norm(ns[i])` and `normals[..] /= norm(..)` call an
// operator/= that takes its left side by const reference and returns the quotient (common.cuh:170-173),
// so nothing is normalised (quirk Q19).
#include "mesh_core.hpp"
#include "wave_ops.hpp"

#include "mc_tables.h"

namespace emf_hip {
namespace {

constexpr int kMcBlock = 256;
constexpr int kMcWaveCubes = 63;                               // positions per wave (lanes 0..62)
constexpr int kMcChunk = kMcWaveCubes * (kMcBlock / 64);       // 252 positions per chunk
// chunks per counting workgroup: 32 for large volumes (the one-workgroup scan over the per-workgroup
// sums shrinks: 0.52 -> 0.455 ms count + scan at 512^3), 8 for small ones (a 128^3 object would
// otherwise be 260 workgroups of 32 serial steps: 0.020 -> 0.055 ms)
constexpr int kMcChunksLarge = 32, kMcChunksSmall = 8;
constexpr size_t kMcLargeVoxels = size_t(1) << 24;
__host__ __device__ inline int chunks_for(size_t nvox) { return nvox >= kMcLargeVoxels ? kMcChunksLarge : kMcChunksSmall; }
constexpr unsigned kXcds = 8;

// Workgroups are dealt round-robin to the 8 XCDs, each with its own 4 MiB L2.  A cube needs the
// planes z and z + 1, so every plane is read twice, one plane's worth of workgroups apart -- 2 MiB of
// tsdf + weights per 512^2 plane, which does not survive in an L2 that streams the whole plane.
// Each XCD therefore takes the same BAND of every plane (an eighth of its rows) and walks z: the data
// it has to keep between the two uses is an eighth of a plane.  `wpp` = workgroups per plane.
__device__ __forceinline__ unsigned logical_block(unsigned block, unsigned nblocks, unsigned wpp) {
    const unsigned band = (wpp + kXcds - 1) / kXcds;
    const unsigned k = block % kXcds, i = block / kXcds;  // (a model's range starts at a multiple of kXcds)
    const unsigned col = k * band + i % band;
    const unsigned b = (i / band) * wpp + col;
    return col < wpp ? b : nblocks;  // nblocks = nothing to do
}

// One launch = a table of n volumes.  Per model m (host-computed, see plan()): counting workgroups
// [launchStart[m], launchStart[m + 1]) of the grid, per-workgroup sums blockSums[blockBase[m] ..] and chunks
// chunkTot[chunkBase[m] ..]; chunk ids in list[] are global (chunkBase[m] + the model's own chunk index).
struct MeshArgs {
    const emf_model_t* models;  // device table (tsdf, weights, grads, fgVolMask, res, voxelSize), or nullptr:
    MeshSource one;             // the single volume of a level-1 call (kTable = false), with
    const float* oneGrads;      // its N^3 x 3 gradient volume or nullptr (forward differences on the fly)
    uint2* blockSums;    // per counting workgroup (vertices, triangles); after k_mesh_scan their exclusive scan per model
    unsigned* chunkTot;  // per chunk: vertices | triangles << 16 (at most 3072 and 1280)
    unsigned* list;      // ids of the chunks with a non-zero total, in no particular order
    unsigned* listCount;
    unsigned long long* bases;  // 2 per model: its first vertex / triangle in the concatenated outputs
    emf_mesh_counts_t* counts;  // n, written by k_mesh_scan
    unsigned long long* basesOut;  // 2 (n + 1) or nullptr: a copy of `bases` plus the totals
    float* vertices;
    float* normals;
    int32_t* triangles;
    unsigned n;
    unsigned launchStart[EMF_MAX_MODELS + 1];
    unsigned blockBase[EMF_MAX_MODELS + 1];
    unsigned chunkBase[EMF_MAX_MODELS + 1];
};
static_assert(sizeof(MeshArgs) <= 4096, "MeshArgs travels in the kernel arguments");

// the model whose range [start[m], start[m + 1]) holds x (wave-uniform; no step at all for one model)
__device__ __forceinline__ unsigned model_of(const unsigned* start, unsigned n, unsigned x) {
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (x >= start[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// kTable: the volumes come from the device table (level 3), else from the arguments (level 1).  Both are
// instances of the same kernels; one kernel choosing at run time held the volume's pointers in VGPRs (count:
// 68 -> 90, emit: 74 -> 93 VGPRs, 7 -> 5 waves per SIMD).
template <bool kTable>
__device__ __forceinline__ MeshSource source_of(const MeshArgs& a, unsigned m, const float*& grads) {
    if constexpr (!kTable) {
        grads = a.oneGrads;
        return a.one;
    }
    const emf_model_t& md = a.models[m];
    grads = md.grads;
    return MeshSource{md.tsdf, md.weights, md.fgVolMask, I3{md.res[0], md.res[1], md.res[2]}, md.voxelSize};
}

struct Cube {
    int x, y, z;
    size_t base;
    unsigned cls;  // 0 when the cube is masked out or carries no surface
};

// Voxel coordinates of a linear position.  Dividing is done once per workgroup (wave-uniform
// values); chunks, waves and lanes are reached from there by carrying -- two 64-bit divisions per
// cube were most of the first counting kernel's time.
struct Origin {
    unsigned x, y, z;
};

__device__ __forceinline__ Origin origin_of(const I3& n, size_t p) {
    const unsigned nx = n.x, ny = n.y;
    const size_t r = p / nx;
    return Origin{static_cast<unsigned>(p - r * nx), static_cast<unsigned>(r % ny), static_cast<unsigned>(r / ny)};
}

__device__ __forceinline__ Origin advanced(const I3& n, Origin o, unsigned by) {
    const unsigned nx = n.x, ny = n.y;
    o.x += by;
    while (o.x >= nx) {  // at most once per wave when Nx >= 64
        o.x -= nx;
        ++o.y;
    }
    while (o.y >= ny) {
        o.y -= ny;
        ++o.z;
    }
    return o;
}

// the cube anchored at voxel `o` (emit pass: its 16 corner values are gathered by the lane itself)
__device__ __forceinline__ Cube classify(const MeshSource& s, const Origin& o, bool inRange) {
    Cube q{0, 0, 0, 0, 0u};
    const I3 n = s.n;
    if (!inRange || o.x + 1 >= static_cast<unsigned>(n.x) || o.y + 1 >= static_cast<unsigned>(n.y) ||
        o.z + 1 >= static_cast<unsigned>(n.z))
        return q;
    q.x = static_cast<int>(o.x);
    q.y = static_cast<int>(o.y);
    q.z = static_cast<int>(o.z);
    const size_t sy = static_cast<size_t>(n.x), sz = sy * n.y;
    q.base = static_cast<size_t>(q.z) * sz + static_cast<size_t>(q.y) * sy + q.x;
    bool valid = true;  // kernel_classifyCubes: all 8 corners observed (and foreground)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int dx, dy, dz;
        cube_corner(i, dx, dy, dz);
        const size_t idx = q.base + dx + dy * sy + dz * sz;
        valid = valid && s.weights[idx] > 0.f && (!s.fg || s.fg[idx] != 0);
    }
    if (!valid) return q;
    unsigned cls = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int dx, dy, dz;
        cube_corner(i, dx, dy, dz);
        cls |= (s.tsdf[q.base + dx + dy * sy + dz * sz] < 0.f ? 1u : 0u) << i;
    }
    q.cls = cls == 255u ? 0u : cls;
    return q;
}

// The same decision for the 63 cubes of a wave at once (count pass).  `ow` / `pw`: coordinates and
// linear position of the wave's first voxel (wave-uniform); lane l holds voxel pw + l.  Returns the
// lane's class (0: no surface here); all lanes of the wave call together.
__device__ __forceinline__ unsigned classify_wave(const MeshSource& s, const Origin& ow, size_t pw, size_t nvox,
                                                  int lane) {
    const I3 n = s.n;
    const unsigned nx = n.x, ny = n.y, nz = n.z;
    const size_t sy = static_cast<size_t>(nx), sz = sy * ny;
    unsigned x = ow.x + lane, y = ow.y, z = ow.z;
    if (nx >= 64u) {  // a wave wraps at most once
        if (x >= nx) {
            x -= nx;
            ++y;
        }
        if (y >= ny) {
            y -= ny;
            ++z;
        }
    } else {
        while (x >= nx) {
            x -= nx;
            ++y;
        }
        while (y >= ny) {
            y -= ny;
            ++z;
        }
    }
    const bool in = pw + lane < nvox;
    const bool rowY = in && y + 1 < ny, rowZ = in && z + 1 < nz;
    const bool row[4] = {in, rowY, rowZ, rowY && rowZ};
    const size_t rowOff[4] = {0, sy, sz, sy + sz};
    float w[4], t[4];
    unsigned char g[4];
    if (pw + 64 + sy + sz <= nvox) {
        // every address of the wave lies inside the arrays (all but the last plane): scalar row bases,
        // the lane index as the only per-lane part of the address.  A row that does not exist for a
        // lane (y + 1 == Ny, z + 1 == Nz) yields a neighbouring row's values; V masks them out.
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            w[r] = (s.weights + pw + rowOff[r])[lane];
            t[r] = (s.tsdf + pw + rowOff[r])[lane];
            g[r] = s.fg ? (s.fg + pw + rowOff[r])[lane] : 1;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // clamped addresses, still unconditional loads
            const size_t q = row[r] ? pw + lane + rowOff[r] : 0;
            w[r] = s.weights[q];
            t[r] = s.tsdf[q];
            g[r] = s.fg ? s.fg[q] : 1;
        }
    }
    unsigned long long V[4], N[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        V[r] = __ballot(row[r] && w[r] > 0.f && g[r] != 0);
        N[r] = __ballot(t[r] < 0.f);  // only read where V says the cube is complete
    }
    // lanes 0..62 whose x + 1 exists; the rows' existence is already in V
    unsigned long long complete = __ballot(x + 1 < nx) & 0x7fffffffffffffffull;
    unsigned long long all = ~0ull, any = 0ull;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        complete &= V[r] & (V[r] >> 1);
        all &= N[r] & (N[r] >> 1);
        any |= N[r] | (N[r] >> 1);
    }
    const unsigned long long surface = complete & any & ~all;  // both signs among the 8 corners
    if (surface == 0ull) return 0u;  // wave-uniform: the common case
    if (!((surface >> lane) & 1ull)) return 0u;
    auto bit = [&](unsigned long long m, int d) { return static_cast<unsigned>((m >> (lane + d)) & 1ull); };
    // corners 0:(0,0,0) 1:(1,0,0) 2:(1,0,1) 3:(0,0,1) 4:(0,1,0) 5:(1,1,0) 6:(1,1,1) 7:(0,1,1); rows (dy, dz):
    // N[0] = (0,0), N[1] = (1,0), N[2] = (0,1), N[3] = (1,1)
    return bit(N[0], 0) | bit(N[0], 1) << 1 | bit(N[2], 1) << 2 | bit(N[2], 0) << 3 | bit(N[1], 0) << 4 |
           bit(N[1], 1) << 5 | bit(N[3], 1) << 6 | bit(N[3], 0) << 7;
}

__device__ __forceinline__ unsigned triangles_of(unsigned cls) {
    unsigned n = 0;
    while (n < 5 && emf_mc_tri_table[cls][3 * n] >= 0) ++n;
    return n;
}

// the counting work of one workgroup: logical workgroup b of a volume with kMcChunks chunks per workgroup
template <int kMcChunks>
__device__ __forceinline__ void count_chunks(const MeshArgs& a, const MeshSource& src, unsigned b,
                                             unsigned blockBase, unsigned chunkBase,
                                             unsigned (*lds)[kMcChunksLarge]) {
    constexpr int kMcSpan = kMcChunk * kMcChunks;
    const I3 n = src.n;
    const size_t nvox = static_cast<size_t>(n.x) * n.y * n.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned p[kMcChunks];
    size_t pw = static_cast<size_t>(b) * kMcSpan + static_cast<size_t>(wave) * kMcWaveCubes;  // this wave, chunk 0
    Origin o = origin_of(n, pw);
#pragma unroll
    for (int c = 0; c < kMcChunks; ++c) {
        const unsigned cls = classify_wave(src, o, pw, nvox, lane);
        p[c] = cls ? __popc(active_edges(cls)) | (triangles_of(cls) << 16) : 0u;
        pw += kMcChunk;
        o = advanced(n, o, kMcChunk);
    }
#pragma unroll
    for (int c = 0; c < kMcChunks; ++c) {
        if (__ballot(p[c] != 0u) != 0ull) {  // wave-uniform: most waves hold no surface
#pragma unroll
            for (int o2 = 32; o2 > 0; o2 >>= 1) p[c] += __shfl_xor(p[c], o2);  // fields cannot carry: <= 756, 315 per wave
        }
        if (lane == 0) lds[wave][c] = p[c];
    }
    __syncthreads();
    if (threadIdx.x < kMcChunks) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < kMcBlock / 64; ++w) t += lds[w][threadIdx.x];
        const unsigned g = chunkBase + b * kMcChunks + threadIdx.x;
        a.chunkTot[g] = t;
        if (t) a.list[atomicAdd(a.listCount, 1u)] = g;
        uint2 sum = make_uint2(t & 0xffffu, t >> 16);
#pragma unroll
        for (int o2 = 1; o2 < kMcChunks; o2 <<= 1) {
            sum.x += __shfl_xor(sum.x, o2);
            sum.y += __shfl_xor(sum.y, o2);
        }
        if (threadIdx.x == 0) a.blockSums[blockBase + b] = sum;
    }
}

template <bool kTable>
__global__ __launch_bounds__(kMcBlock) void k_mesh_count(const MeshArgs a) {
    __shared__ unsigned lds[kMcBlock / 64][kMcChunksLarge];
    const unsigned m = kTable ? model_of(a.launchStart, a.n, blockIdx.x) : 0u;
    const unsigned blockBase = a.blockBase[m], nblocks = a.blockBase[m + 1] - blockBase;
    const float* grads;
    const MeshSource src = source_of<kTable>(a, m, grads);
    const size_t nvox = static_cast<size_t>(src.n.x) * src.n.y * src.n.z;
    const unsigned chunks = static_cast<unsigned>(chunks_for(nvox));
    const size_t plane = static_cast<size_t>(src.n.x) * src.n.y, span = static_cast<size_t>(kMcChunk) * chunks;
    const unsigned wpp = plane >= span ? static_cast<unsigned>(plane / span) : 1u;  // counting workgroups per z plane
    const unsigned b = logical_block(blockIdx.x - a.launchStart[m], nblocks, wpp);
    if (b >= nblocks) return;
    if (chunks == static_cast<unsigned>(kMcChunksLarge))
        count_chunks<kMcChunksLarge>(a, src, b, blockBase, a.chunkBase[m], lds);
    else
        count_chunks<kMcChunksSmall>(a, src, b, blockBase, a.chunkBase[m], lds);
}

// one workgroup walks each model's per-workgroup sums in chunks of 1024 (a 512^3 volume has 17 k of them), the
// total restarting at every model; the models' totals become their counts and, summed in 64 bits, their bases
__global__ __launch_bounds__(kSumsBlock) void k_mesh_scan(const MeshArgs a) {
    __shared__ uint2 lds[kSumsBlock / 64];
    unsigned long long vbase = 0, tbase = 0;
    for (unsigned m = 0; m < a.n; ++m) {
        const uint2 total = scan_sums(a.blockSums, a.blockBase[m], a.blockBase[m + 1], lds);
        if (threadIdx.x == 0) {
            a.counts[m].vertices = total.x;
            a.counts[m].triangles = total.y;
            a.bases[2 * m] = vbase;
            a.bases[2 * m + 1] = tbase;
            if (a.basesOut) {
                a.basesOut[2 * m] = vbase;
                a.basesOut[2 * m + 1] = tbase;
            }
            vbase += total.x;
            tbase += total.y;
        }
    }
    if (threadIdx.x == 0 && a.basesOut) {
        a.basesOut[2 * a.n] = vbase;
        a.basesOut[2 * a.n + 1] = tbase;
    }
}

// where one model's mesh goes: its slice of the concatenated outputs
struct MeshOut {
    MeshSource src;
    const float* grads;
    float* vertices;
    float* normals;
    int32_t* triangles;
};

// gradient of the corner voxel: the gradient volume if there is one, else what
// kernel_computeTSDFGrads would have stored there (forward differences, zero on the last planes)
__device__ __forceinline__ V3 corner_gradient(const MeshOut& a, size_t idx, int x, int y, int z) {
    if (a.grads) return v3(a.grads[3 * idx], a.grads[3 * idx + 1], a.grads[3 * idx + 2]);
    const I3 n = a.src.n;
    if (x >= n.x - 1 || y >= n.y - 1 || z >= n.z - 1) return v3(0.f, 0.f, 0.f);
    const size_t sy = static_cast<size_t>(n.x), sz = sy * n.y;
    const float t = a.src.tsdf[idx];
    return v3(a.src.tsdf[idx + 1] - t, a.src.tsdf[idx + sy] - t, a.src.tsdf[idx + sz] - t);
}

__device__ __forceinline__ void emit_cube(const MeshOut& a, const Cube& q, unsigned edges, unsigned ntris,
                                          unsigned vertBase, unsigned triBase);

// One entry of the list of surface chunks as the lanes of a workgroup see it: the model, its volume, the lane's cube
// and where the cube's vertices and triangles go in the model's slice.  The emit kernel and the colour kernel both
// walk the list through this, so a vertex has the same slot in both.  All lanes of the workgroup call it together.
struct ChunkSlot {
    unsigned m;          // model
    MeshSource src;
    const float* grads;
    Cube q;              // q.cls == 0: nothing to write for this lane
    unsigned edges, ntris;
    unsigned vertBase, triBase;  // model-local first vertex / triangle of the lane's cube
};

template <bool kTable>
__device__ __forceinline__ ChunkSlot chunk_slot(const MeshArgs& a, unsigned i, uint2* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ChunkSlot s;
    const unsigned gg = a.list[i];
    s.m = kTable ? model_of(a.chunkBase, a.n, gg) : 0u;
    s.src = source_of<kTable>(a, s.m, s.grads);
    const I3 n = s.src.n;
    const size_t nvox = static_cast<size_t>(n.x) * n.y * n.z;
    const unsigned chunks = static_cast<unsigned>(chunks_for(nvox));
    const unsigned* tot = a.chunkTot + a.chunkBase[s.m];
    const unsigned g = gg - a.chunkBase[s.m];  // the model's own chunk index
    const unsigned first = g & ~(chunks - 1u);
    uint2 base = a.blockSums[a.blockBase[s.m] + g / chunks];
    for (unsigned c = first; c < g; ++c) {
        const unsigned t = tot[c];
        base.x += t & 0xffffu;
        base.y += t >> 16;
    }
    const size_t p = static_cast<size_t>(g) * kMcChunk + static_cast<size_t>(wave) * kMcWaveCubes + lane;
    s.q = classify(s.src, origin_of(n, p), lane < kMcWaveCubes && p < nvox);
    s.edges = s.q.cls ? active_edges(s.q.cls) : 0u;
    uint2 v = make_uint2(0u, 0u);
    if (s.q.cls) v = make_uint2(__popc(s.edges), triangles_of(s.q.cls));
    uint2 total;
    const uint2 mine = block_exclusive_scan<kMcBlock / 64>(v, total, lds);
    s.ntris = v.y;
    s.vertBase = base.x + mine.x;
    s.triBase = base.y + mine.y;
    return s;
}

// 6 waves per SIMD like the one-volume kernel before the table (74 VGPRs); uncapped the slice offsets take the
// argument form to 81 = 5 waves
template <bool kTable>
__global__ __launch_bounds__(kMcBlock) __attribute__((amdgpu_waves_per_eu(6))) void k_mesh_emit(const MeshArgs a) {
    __shared__ uint2 lds[kMcBlock / 64];
    const unsigned todo = *a.listCount;
    for (unsigned i = blockIdx.x; i < todo; i += gridDim.x) {
        const ChunkSlot s = chunk_slot<kTable>(a, i, lds);
        MeshOut out;
        out.src = s.src;
        out.grads = s.grads;
        const unsigned long long vb = a.bases[2 * s.m], tb = a.bases[2 * s.m + 1];
        out.vertices = a.vertices + 3 * vb;
        out.normals = a.normals + 3 * vb;
        out.triangles = a.triangles + 4 * tb;
        // (3, i0, i1, i2) per triangle
        if (s.q.cls) emit_cube(out, s.q, s.edges, s.ntris, s.vertBase, 4u * s.triBase);
    }
}

__device__ __forceinline__ void emit_cube(const MeshOut& a, const Cube& q, unsigned edges, unsigned ntris,
                                          unsigned vertBase, unsigned triBase) {
    const I3 n = a.src.n;
    const size_t sy = static_cast<size_t>(n.x), sz = sy * n.y;
    const V3 half = half_extent(n);
    int offsets[12];
    unsigned k = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        offsets[e] = 0;
        if (!((edges >> e) & 1u)) continue;
        V3 p[2], g[2];
        float val[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int dx, dy, dz;
            cube_corner(emf_mc_edge_corner[e][s], dx, dy, dz);
            const size_t idx = q.base + dx + dy * sy + dz * sz;
            val[s] = a.src.tsdf[idx];
            // ( x + 1 - ( volSize.x - 1 ) / 2.f ) * voxelSize  (TSDF.cu:945-968)
            p[s] = v3((static_cast<float>(q.x + dx) - half.x) * a.src.voxelSize,
                      (static_cast<float>(q.y + dy) - half.y) * a.src.voxelSize,
                      (static_cast<float>(q.z + dz) - half.z) * a.src.voxelSize);
            g[s] = corner_gradient(a, idx, q.x + dx, q.y + dy, q.z + dz);
        }
        const V3 pv = vertex_interp(p[0], p[1], val[0], val[1]);
        const V3 nv = vertex_interp(g[0], g[1], val[0], val[1]);  // not normalised: Q19
        float* vo = a.vertices + 3 * static_cast<size_t>(vertBase + k);
        float* no = a.normals + 3 * static_cast<size_t>(vertBase + k);
        vo[0] = pv.x;
        vo[1] = pv.y;
        vo[2] = pv.z;
        no[0] = nv.x;
        no[1] = nv.y;
        no[2] = nv.z;
        offsets[e] = static_cast<int>(k++);
    }
    for (unsigned t = 0; t < ntris; ++t) {
        int32_t* to = a.triangles + triBase + 4 * t;
        to[0] = 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = emf_mc_tri_table[q.cls][3 * t + j];
            int o = 0;  // offsets[e] without a dynamically indexed register array
#pragma unroll
            for (int i = 0; i < 12; ++i) o = e == i ? offsets[i] : o;
            to[1 + j] = static_cast<int32_t>(vertBase) + o;  // model-local: the slice is the volume's own mesh
        }
    }
}

// ---- vertex colours (new behaviour: include/emf_hip.h "Per-voxel colour") ------------------------------------
// The emit kernel's walk over the list of surface chunks once more (chunk_slot: the same function, hence the same
// vertex slots), writing u8 x 3 per vertex from a colour volume instead of position and normal.  A pass of
// its own so that the emit kernels stay what they are; it costs the surface chunks' corner gathers a second time.
struct MeshColorArgs {
    const uint16_t* one;           // colour volume of a level-1 call
    uint16_t* const* table;        // device array parallel to the model table (level 3); NULL entry: black
    uint8_t* colors;               // 3 per vertex, concatenated like the vertices
};

__device__ __forceinline__ void color_cube(const MeshSource& src, const ushort4* vol, const Cube& q, unsigned edges,
                                           unsigned vertBase, uint8_t* colors) {
    const I3 n = src.n;
    const size_t sy = static_cast<size_t>(n.x), sz = sy * n.y;
    unsigned k = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!((edges >> e) & 1u)) continue;
        float val[2];
        ushort4 c[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int dx, dy, dz;
            cube_corner(emf_mc_edge_corner[e][s], dx, dy, dz);
            const size_t idx = q.base + dx + dy * sy + dz * sz;
            val[s] = src.tsdf[idx];
            c[s] = vol ? vol[idx] : make_ushort4(0, 0, 0, 0);
        }
        edge_colour(c[0], c[1], val[0], val[1], colors + 3 * static_cast<size_t>(vertBase + k));
        ++k;
    }
}

template <bool kTable>
__global__ __launch_bounds__(kMcBlock) void k_mesh_colors(const MeshArgs a, const MeshColorArgs ca) {
    __shared__ uint2 lds[kMcBlock / 64];
    const unsigned todo = *a.listCount;
    for (unsigned i = blockIdx.x; i < todo; i += gridDim.x) {
        const ChunkSlot s = chunk_slot<kTable>(a, i, lds);
        const ushort4* vol = reinterpret_cast<const ushort4*>(kTable ? ca.table[s.m] : ca.one);
        if (s.q.cls) color_cube(s.src, vol, s.q, s.edges, s.vertBase, ca.colors + 3 * a.bases[2 * s.m]);
    }
}

// ---- edge keys (new behaviour: include/emf_hip.h "Welded meshes"; the welding itself is mesh_weld.hip) ----------
// The walk over the list of surface chunks a third time (chunk_slot again: the same vertex slots), writing per soup
// vertex the u64 key of the grid edge it lies on: slot << 48 | 3 * linear(lower voxel) + axis.  The cube and the
// edge bits are in registers here and the corner offsets are compile-time constants: no voxel is read beyond what
// chunk_slot's classification reads.
constexpr int kMeshKeySlotShift = 48;  // 3 * voxels of one volume stays below 2^41 (plan(): chunk ids in 31 bits)

__device__ __forceinline__ void key_cube(const MeshSource& src, unsigned m, const Cube& q, unsigned edges,
                                         unsigned vertBase, unsigned long long* keys) {
    const I3 n = src.n;
    const size_t sy = static_cast<size_t>(n.x), sz = sy * n.y;
    unsigned k = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!((edges >> e) & 1u)) continue;
        int ax, ay, az, bx, by, bz;
        cube_corner(emf_mc_edge_corner[e][0], ax, ay, az);
        cube_corner(emf_mc_edge_corner[e][1], bx, by, bz);
        const int lx = ax < bx ? ax : bx, ly = ay < by ? ay : by, lz = az < bz ? az : bz;  // the lower voxel
        const int axis = ax != bx ? 0 : (ay != by ? 1 : 2);
        const unsigned long long lin = q.base + lx + ly * sy + lz * sz;
        keys[vertBase + k] = (static_cast<unsigned long long>(m) << kMeshKeySlotShift) | (3ull * lin + axis);
        ++k;
    }
}

template <bool kTable>
__global__ __launch_bounds__(kMcBlock) void k_mesh_keys(const MeshArgs a, unsigned long long* keys) {
    __shared__ uint2 lds[kMcBlock / 64];
    const unsigned todo = *a.listCount;
    for (unsigned i = blockIdx.x; i < todo; i += gridDim.x) {
        const ChunkSlot s = chunk_slot<kTable>(a, i, lds);
        if (s.q.cls) key_cube(s.src, s.m, s.q, s.edges, s.vertBase, keys + a.bases[2 * s.m]);
    }
}

// grid of one volume's counting pass: 8 XCDs x ceil(wpp / 8) columns x planes (see logical_block)
unsigned launch_blocks(unsigned nblocks, unsigned wpp) {
    const unsigned band = (wpp + kXcds - 1) / kXcds, rows = (nblocks + wpp - 1) / wpp;
    return kXcds * band * rows;
}

// The ranges of a table of n volumes (res: 3 per model) and the scratch they need:
//   [bases: 2n u64][blockSums: uint2 per counting workgroup][chunkTot, list: u32 per chunk][listCount][pad]
int plan(MeshArgs& a, const int32_t* res, int n, size_t& scratchBytes) {
    EMF_REQUIRE_PTR(res);
    if (n < 1 || n > EMF_MAX_MODELS)
        return fail(EMF_E_LIMIT, "mesh: %d models (1 .. %d per launch)", n, EMF_MAX_MODELS);
    unsigned long long grid = 0, blocks = 0, chunks = 0;
    for (int m = 0; m < n; ++m) {
        EMF_TRY(check_res(res + 3 * m));
        const size_t nvox = static_cast<size_t>(res[3 * m]) * res[3 * m + 1] * res[3 * m + 2];
        const unsigned per = static_cast<unsigned>(chunks_for(nvox));
        const size_t span = static_cast<size_t>(kMcChunk) * per;
        const unsigned long long nb = (nvox + span - 1) / span;
        const size_t plane = static_cast<size_t>(res[3 * m]) * res[3 * m + 1];
        const unsigned wpp = static_cast<unsigned>(plane >= span ? plane / span : 1);
        a.launchStart[m] = static_cast<unsigned>(grid);
        a.blockBase[m] = static_cast<unsigned>(blocks);
        a.chunkBase[m] = static_cast<unsigned>(chunks);
        // the XCD banding pads a model's grid to whole bands: at most 8 wpp workgroups more than it has
        grid += launch_blocks(static_cast<unsigned>(nb), wpp);
        blocks += nb;
        chunks += nb * per;
        if (chunks > 0x7ffffff0ull || grid > 0xffffffull)  // chunk ids in 32 bits, 256-lane workgroups in one grid
            return fail(EMF_E_LIMIT, "mesh: %d volumes of %llu chunks exceed one launch", m + 1, chunks);
    }
    a.launchStart[n] = static_cast<unsigned>(grid);
    a.blockBase[n] = static_cast<unsigned>(blocks);
    a.chunkBase[n] = static_cast<unsigned>(chunks);
    a.n = static_cast<unsigned>(n);
    scratchBytes = 16 * static_cast<size_t>(n) + blocks * sizeof(uint2) + 2 * chunks * sizeof(unsigned) + 16;
    return EMF_OK;
}

void place(MeshArgs& a, void* scratch) {
    a.bases = static_cast<unsigned long long*>(scratch);
    a.blockSums = reinterpret_cast<uint2*>(a.bases + 2 * a.n);
    a.chunkTot = reinterpret_cast<unsigned*>(a.blockSums + a.blockBase[a.n]);
    a.list = a.chunkTot + a.chunkBase[a.n];
    a.listCount = a.list + a.chunkBase[a.n];
}

int launch_count(MeshArgs& a, emf_stream_t stream, const char* what) {
    const hipError_t e = hipMemsetAsync(a.listCount, 0, sizeof(unsigned), as_stream(stream));
    if (e != hipSuccess) {
        set_error("%s: memset: %s", what, hipGetErrorString(e));
        return static_cast<int>(e);
    }
    if (a.models)
        hipLaunchKernelGGL(k_mesh_count<true>, dim3(a.launchStart[a.n]), dim3(kMcBlock), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(k_mesh_count<false>, dim3(a.launchStart[a.n]), dim3(kMcBlock), 0, as_stream(stream), a);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kSumsBlock), 0, as_stream(stream), a);
    return launch_status(what);
}

int launch_emit(MeshArgs& a, emf_stream_t stream, const char* what) {
    const unsigned nchunks = a.chunkBase[a.n];  // fixed grid over the list of surface chunks
    const dim3 grid(nchunks < 4096u ? nchunks : 4096u);
    if (a.models)
        hipLaunchKernelGGL(k_mesh_emit<true>, grid, dim3(kMcBlock), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(k_mesh_emit<false>, grid, dim3(kMcBlock), 0, as_stream(stream), a);
    return launch_status(what);
}

// the level-1 form: a one-volume table whose volume travels in the arguments
int single(MeshArgs& a, const float* tsdf, const float* weights, const uint8_t* fg, const float* grads,
           const int32_t res[3], float voxelSize, void* scratch) {
    EMF_REQUIRE_PTR(tsdf);
    EMF_REQUIRE_PTR(weights);
    EMF_REQUIRE_PTR(scratch);
    EMF_TRY(check_res(res));
    size_t bytes = 0;
    a = MeshArgs{};
    EMF_TRY(plan(a, res, 1, bytes));
    a.one = MeshSource{tsdf, weights, fg, i3_from(res), voxelSize};
    a.oneGrads = grads;
    place(a, scratch);
    return EMF_OK;
}

int table(MeshArgs& a, const emf_model_t* models, const int32_t* res, int n, void* scratch) {
    EMF_REQUIRE_PTR(models);
    size_t bytes = 0;
    a = MeshArgs{};
    EMF_TRY(plan(a, res, n, bytes));
    EMF_REQUIRE_PTR(scratch);
    a.models = models;
    place(a, scratch);
    return EMF_OK;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

size_t emf_hip_meshScratchBytes(const int32_t res[3]) { return emf_hip_meshScratchBytesBatched(res, 1); }

size_t emf_hip_meshScratchBytesBatched(const int32_t* res_host, int n) {
    if (!res_host || n < 1 || n > EMF_MAX_MODELS) return 0;
    for (int m = 0; m < n; ++m)
        if (res_host[3 * m] < 2 || res_host[3 * m + 1] < 2 || res_host[3 * m + 2] < 2) return 0;
    MeshArgs a;
    size_t bytes = 0;
    return plan(a, res_host, n, bytes) == EMF_OK ? bytes : 0;
}

int emf_hip_meshCount(const float* tsdf, const float* weights, const uint8_t* fgVolMask,
                      const int32_t res[3], void* scratch_dev, emf_mesh_counts_t* counts_dev,
                      emf_stream_t stream) {
    MeshArgs a;
    EMF_TRY(single(a, tsdf, weights, fgVolMask, nullptr, res, 1.f, scratch_dev));
    EMF_REQUIRE_PTR(counts_dev);
    a.counts = counts_dev;
    return launch_count(a, stream, "meshCount");
}

int emf_hip_meshEmit(const float* tsdf, const float* grads, const float* weights,
                     const uint8_t* fgVolMask, const int32_t res[3], float voxelSize,
                     const void* scratch_dev, float* vertices, float* normals, int32_t* triangles,
                     emf_stream_t stream) {
    MeshArgs a;
    EMF_TRY(single(a, tsdf, weights, fgVolMask, grads, res, voxelSize, const_cast<void*>(scratch_dev)));
    EMF_REQUIRE_PTR(vertices);
    EMF_REQUIRE_PTR(normals);
    EMF_REQUIRE_PTR(triangles);
    a.vertices = vertices;
    a.normals = normals;
    a.triangles = triangles;
    return launch_emit(a, stream, "meshEmit");
}

int emf_hip_meshCountBatched(const emf_model_t* models_dev, const int32_t* res_host, int n, void* scratch_dev,
                             emf_mesh_counts_t* counts_dev, uint64_t* bases_dev, emf_stream_t stream) {
    MeshArgs a;
    EMF_TRY(table(a, models_dev, res_host, n, scratch_dev));
    EMF_REQUIRE_PTR(counts_dev);
    a.counts = counts_dev;
    a.basesOut = reinterpret_cast<unsigned long long*>(bases_dev);
    return launch_count(a, stream, "meshCountBatched");
}

int emf_hip_meshEmitBatched(const emf_model_t* models_dev, const int32_t* res_host, int n, const void* scratch_dev,
                            float* vertices, float* normals, int32_t* triangles, emf_stream_t stream) {
    MeshArgs a;
    EMF_TRY(table(a, models_dev, res_host, n, const_cast<void*>(scratch_dev)));
    EMF_REQUIRE_PTR(vertices);
    EMF_REQUIRE_PTR(normals);
    EMF_REQUIRE_PTR(triangles);
    a.vertices = vertices;
    a.normals = normals;
    a.triangles = triangles;
    return launch_emit(a, stream, "meshEmitBatched");
}

int emf_hip_meshColors(const float* tsdf, const float* weights, const uint8_t* fgVolMask, const uint16_t* color,
                       const int32_t res[3], const void* scratch_dev, uint8_t* colors, emf_stream_t stream) {
    MeshArgs a;
    EMF_TRY(single(a, tsdf, weights, fgVolMask, nullptr, res, 1.f, const_cast<void*>(scratch_dev)));
    EMF_REQUIRE_PTR(color);
    EMF_REQUIRE_PTR(colors);
    const MeshColorArgs ca{color, nullptr, colors};
    const unsigned nchunks = a.chunkBase[a.n];
    hipLaunchKernelGGL(k_mesh_colors<false>, dim3(nchunks < 4096u ? nchunks : 4096u), dim3(kMcBlock), 0,
                       as_stream(stream), a, ca);
    return launch_status("meshColors");
}

int emf_hip_meshColorsBatched(const emf_model_t* models_dev, uint16_t* const* colors_dev, const int32_t* res_host, int n,
                              const void* scratch_dev, uint8_t* colors, emf_stream_t stream) {
    MeshArgs a;
    EMF_TRY(table(a, models_dev, res_host, n, const_cast<void*>(scratch_dev)));
    EMF_REQUIRE_PTR(colors_dev);
    EMF_REQUIRE_PTR(colors);
    const MeshColorArgs ca{nullptr, colors_dev, colors};
    const unsigned nchunks = a.chunkBase[a.n];
    hipLaunchKernelGGL(k_mesh_colors<true>, dim3(nchunks < 4096u ? nchunks : 4096u), dim3(kMcBlock), 0,
                       as_stream(stream), a, ca);
    return launch_status("meshColorsBatched");
}

int emf_hip_meshEdgeKeys(const float* tsdf, const float* weights, const uint8_t* fgVolMask, const int32_t res[3],
                         const void* scratch_dev, uint64_t* keys, emf_stream_t stream) {
    MeshArgs a;
    EMF_TRY(single(a, tsdf, weights, fgVolMask, nullptr, res, 1.f, const_cast<void*>(scratch_dev)));
    EMF_REQUIRE_PTR(keys);
    const unsigned nchunks = a.chunkBase[a.n];
    hipLaunchKernelGGL(k_mesh_keys<false>, dim3(nchunks < 4096u ? nchunks : 4096u), dim3(kMcBlock), 0,
                       as_stream(stream), a, reinterpret_cast<unsigned long long*>(keys));
    return launch_status("meshEdgeKeys");
}

int emf_hip_meshEdgeKeysBatched(const emf_model_t* models_dev, const int32_t* res_host, int n, const void* scratch_dev,
                                uint64_t* keys, emf_stream_t stream) {
    MeshArgs a;
    EMF_TRY(table(a, models_dev, res_host, n, const_cast<void*>(scratch_dev)));
    EMF_REQUIRE_PTR(keys);
    const unsigned nchunks = a.chunkBase[a.n];
    hipLaunchKernelGGL(k_mesh_keys<true>, dim3(nchunks < 4096u ? nchunks : 4096u), dim3(kMcBlock), 0,
                       as_stream(stream), a, reinterpret_cast<unsigned long long*>(keys));
    return launch_status("meshEdgeKeysBatched");
}

}  // extern "C"
