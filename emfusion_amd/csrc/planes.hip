// planes.hip -- planes: the surface voxels of a box of a volume with their TSDF gradients, the votes of those gradients
// for a direction and for an offset along given directions, and the assignment of every surface voxel to one of a list
// of planes with the integer moments of each plane's members (include/emf_hip.h "Planes").
//
//   k_pl_surface<false>  one workgroup of 256 lanes per 32 x 8 x 8 tile anchored at the box origin.  tsdf and weights of
//                        the tile with a one-voxel halo (34 x 10 x 10, taken from the VOLUME, weight 0 outside it) are
//                        staged in LDS: the 32 voxels of a row as eight 16-byte loads where the row's first voxel is
//                        16-byte aligned in both arrays, voxel by voxel elsewhere, the two halo columns voxel by voxel.
//                        A lane owns 8 consecutive voxels of a row, so lane order is the tile's (z, y, x) order.  The
//                        workgroup's count of records goes to the tile's u32, the two totals to the counters with one
//                        integer atomic each.  A workgroup whose voxels all lie in tiles the volume's unseen-tile map
//                        marks "every weight is 0" writes a count of 0 and leaves before it stages anything.
//   k_pl_scan            one workgroup: the tiles' counts -> exclusive offsets in place (scan_sums of wave_ops.hpp), records
//                        written -> counters[2].
//   k_pl_surface<true>   the same walk; a tile without a record or wholly past the capacity leaves at once; the rank of a
//                        record is the tile's offset plus the workgroup scan of the lanes' counts.  One 16-byte store per
//                        record.  No atomic decides a position.
//   k_pl_directions      a workgroup takes 8192 consecutive records into a cube-map histogram in LDS (6 K^2 u32, at most
//                        23064 bytes) and adds the non-zero bins to the global one.
//   k_pl_offsets         one lane per record; per direction the destination slot, then run_scan (wave_ops.hpp) over the
//                        wave's runs of equal destinations and one atomic per run (records are spatially ordered: runs are
//                        long).  Over run numbers (run_id), since a destination can come back in a wave.
//   k_pl_assign          one lane per record; the label, then the ten sums and six bounds per run of equal labels.
// Stage 4, patches: the connected surfaces of every plane, without a dense volume.
//   k_pp_init            parent[i] = i for a record with a label, -1 for one without (the patch array is the union-find)
//   k_pp_hook            one lane per member: the 13 (reach 1) or 62 (reach 2) voxels that precede its own in (z, y, x)
//                        order; each one inside the box is looked up by a binary search of its tile-order key among the
//                        records' own keys, and a record found there with the same label is united (union_find.hpp)
//   k_pp_flatten         patch[i] := root of i, the smallest record index of the patch; members and roots counted
//   k_pp_rootsums / k_pp_scan / k_pp_roots   roots ranked by scan in record order; roots[rank] = i, the slot initialised
//   k_pp_stats           one lane per record; ten sums, six bounds and four extent keys per run of equal PATCH in a wave
//                        (run_id: a patch can come back), the slot by binary search of the root, then one atomic each
//   k_pp_keepsums / k_pp_scan / k_pp_emit    slots of at least min_count members written in id order, placed by scan
// Every float step is a single float32 operation through the _rn intrinsics, never contracted whatever the build; integer
// atomics only: every output is a pure function of the inputs.  No scratch memory, no float atomics, no inline assembly.
#include <cfloat>

#include "common.hpp"
#include "wave_ops.hpp"
#include "union_find.hpp"

namespace emf_hip {
namespace {

constexpr int kPlBlock = 256;
constexpr int kPlTX = 32, kPlTY = 8, kPlTZ = 8;       // the tile, and the tile of the unseen-tile map
constexpr int kPlHX = kPlTX + 2, kPlHY = kPlTY + 2, kPlHZ = kPlTZ + 2;
constexpr int kPlRowTasks = 10;                       // eight quads and the two halo voxels of a staged row
constexpr unsigned kPlChunk = 8192;                   // records per workgroup of k_pl_directions
constexpr unsigned long long kPlMaxTiles = 0xffffffull;

static_assert(sizeof(emf_plane_voxel_t) == 16 && sizeof(emf_plane_moments_t) == 104, "mirrored by emfusion_amd/_lib.py");
static_assert(6 * EMF_PLANE_MAX_K * EMF_PLANE_MAX_K * sizeof(unsigned) <= 24 * 1024, "the direction histogram lives in LDS");

struct SurfArgs {
    const float* tsdf;
    const float* weights;
    const uint8_t* unseen;  // or NULL
    emf_plane_voxel_t* records;
    unsigned* tiles;  // count: the tiles' counts; emit: their exclusive offsets
    unsigned* counters;
    I3 res, lo, size;
    unsigned ntx, nty, ntiles;
    unsigned capacity;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }

template <bool EMIT>
__global__ __launch_bounds__(kPlBlock) void k_pl_surface(const SurfArgs a) {
    __shared__ float st[kPlHZ][kPlHY][kPlHX];
    __shared__ float sw[kPlHZ][kPlHY][kPlHX];
    __shared__ unsigned scanLds[kPlBlock / 64];
    const unsigned b = blockIdx.x;
    const unsigned tz = b / (a.ntx * a.nty), r = b - tz * a.ntx * a.nty, ty = r / a.ntx, tx = r - ty * a.ntx;
    const int bx0 = static_cast<int>(tx) * kPlTX, by0 = static_cast<int>(ty) * kPlTY, bz0 = static_cast<int>(tz) * kPlTZ;
    const int ex = min(kPlTX, a.size.x - bx0), ey = min(kPlTY, a.size.y - by0), ez = min(kPlTZ, a.size.z - bz0);
    const int vx0 = a.lo.x + bx0, vy0 = a.lo.y + by0, vz0 = a.lo.z + bz0;  // volume coordinates of the tile's origin
    unsigned base = 0u;
    if (EMIT) {  // block-uniform
        base = a.tiles[b];
        const unsigned next = b + 1u < a.ntiles ? a.tiles[b + 1u] : a.counters[1];
        if (next == base || base >= a.capacity) return;
    } else if (a.unseen != nullptr) {  // block-uniform: the map's tiles are anchored at the volume's origin
        const unsigned mtx = (a.res.x + kPlTX - 1) / kPlTX, mty = (a.res.y + kPlTY - 1) / kPlTY;
        bool seen = false;
        for (int mz = vz0 / kPlTZ; mz <= (vz0 + ez - 1) / kPlTZ; ++mz)
            for (int my = vy0 / kPlTY; my <= (vy0 + ey - 1) / kPlTY; ++my)
                for (int mx = vx0 / kPlTX; mx <= (vx0 + ex - 1) / kPlTX; ++mx)
                    seen = seen || a.unseen[(static_cast<size_t>(mz) * mty + my) * mtx + mx] == 0;
        if (!seen) {
            if (threadIdx.x == 0) a.tiles[b] = 0u;
            return;
        }
    }
    // stage: row (ly, lz) of the halo box is the volume row (vy0 + ly - 1, vz0 + lz - 1); what lies outside the volume
    // has weight 0, which makes it neither free nor observed
    const long long sy = a.res.x, sz = sy * a.res.y;
    for (int t = threadIdx.x; t < kPlHZ * kPlHY * kPlRowTasks; t += kPlBlock) {
        const int row = t / kPlRowTasks, q = t - row * kPlRowTasks;
        const int lz = row / kPlHY, ly = row - lz * kPlHY;
        const int vy = vy0 + ly - 1, vz = vz0 + lz - 1;
        const bool rowIn = vy >= 0 && vy < a.res.y && vz >= 0 && vz < a.res.z;
        const int lx = q < 8 ? 1 + 4 * q : (q == 8 ? 0 : kPlHX - 1);
        const int vx = vx0 + lx - 1, count = q < 8 ? 4 : 1;
        float tv[4] = {0.f, 0.f, 0.f, 0.f}, wv[4] = {0.f, 0.f, 0.f, 0.f};
        if (rowIn) {
            const long long i = static_cast<long long>(vz) * sz + static_cast<long long>(vy) * sy + vx;  // used only where inside
            const float* tp = a.tsdf + i;
            const float* wp = a.weights + i;
            if (count == 4 && vx + 3 < a.res.x &&
                ((reinterpret_cast<uintptr_t>(tp) | reinterpret_cast<uintptr_t>(wp)) & 15u) == 0) {
                const float4 p = *reinterpret_cast<const float4*>(tp), w = *reinterpret_cast<const float4*>(wp);
                tv[0] = p.x, tv[1] = p.y, tv[2] = p.z, tv[3] = p.w;
                wv[0] = w.x, wv[1] = w.y, wv[2] = w.z, wv[3] = w.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < count && vx + e >= 0 && vx + e < a.res.x) {
                        tv[e] = tp[e];
                        wv[e] = wp[e];
                    }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < count) {
                st[lz][ly][lx + e] = tv[e];
                sw[lz][ly][lx + e] = wv[e];
            }
    }
    __syncthreads();
    // a lane's 8 voxels: x0 .. x0 + 7 of row (y, z); bit e of the masks is voxel x0 + e
    const int x0 = 8 * static_cast<int>(threadIdx.x & 3u), y = static_cast<int>((threadIdx.x >> 2) & 7u),
              z = static_cast<int>(threadIdx.x >> 5);
    unsigned surf = 0u, norm = 0u;
    if (y < ey && z < ez) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int x = x0 + e;
            if (x >= ex) continue;
            const int cx = x + 1, cy = y + 1, cz = z + 1;
            if (!(sw[cz][cy][cx] > 0.f) || st[cz][cy][cx] > 0.f) continue;  // not solid
            const float wxm = sw[cz][cy][cx - 1], wxp = sw[cz][cy][cx + 1], wym = sw[cz][cy - 1][cx], wyp = sw[cz][cy + 1][cx],
                        wzm = sw[cz - 1][cy][cx], wzp = sw[cz + 1][cy][cx];
            const float txm = st[cz][cy][cx - 1], txp = st[cz][cy][cx + 1], tym = st[cz][cy - 1][cx], typ = st[cz][cy + 1][cx],
                        tzm = st[cz - 1][cy][cx], tzp = st[cz + 1][cy][cx];
            const bool anyFree = (wxm > 0.f && txm > 0.f) || (wxp > 0.f && txp > 0.f) || (wym > 0.f && tym > 0.f) ||
                                 (wyp > 0.f && typ > 0.f) || (wzm > 0.f && tzm > 0.f) || (wzp > 0.f && tzp > 0.f);
            if (!anyFree) continue;
            surf |= 1u << e;
            if (!(wxm > 0.f && wxp > 0.f && wym > 0.f && wyp > 0.f && wzm > 0.f && wzp > 0.f)) continue;
            const float g0 = __fsub_rn(txp, txm), g1 = __fsub_rn(typ, tym), g2 = __fsub_rn(tzp, tzm);
            if (!(finite_f(g0) && finite_f(g1) && finite_f(g2))) continue;
            if (g0 == 0.f && g1 == 0.f && g2 == 0.f) continue;
            norm |= 1u << e;
        }
    }
    const unsigned counts = __popc(norm) | (__popc(surf) << 16);  // both at most 2048 over the workgroup
    unsigned total;
    const unsigned before = block_exclusive_scan<kPlBlock / 64>(counts, total, scanLds);
    if (!EMIT) {
        if (threadIdx.x == 0) {
            a.tiles[b] = total & 0xffffu;
            if (total >> 16) atomicAdd(&a.counters[0], total >> 16);
            if (total & 0xffffu) atomicAdd(&a.counters[1], total & 0xffffu);
        }
        return;
    }
    unsigned pos = base + (before & 0xffffu);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (!((norm >> e) & 1u)) continue;
        if (pos < a.capacity) {
            const int cx = x0 + e + 1, cy = y + 1, cz = z + 1;
            const float g0 = __fsub_rn(st[cz][cy][cx + 1], st[cz][cy][cx - 1]);
            const float g1 = __fsub_rn(st[cz][cy + 1][cx], st[cz][cy - 1][cx]);
            const float g2 = __fsub_rn(st[cz + 1][cy][cx], st[cz - 1][cy][cx]);
            const int index = ((bz0 + z) * a.size.y + (by0 + y)) * a.size.x + (bx0 + x0 + e);
            *reinterpret_cast<float4*>(a.records + pos) = make_float4(__int_as_float(index), g0, g1, g2);
        }
        ++pos;
    }
}

// one workgroup: tiles[b] := sum of tiles[0 .. b); counters[2] := min(total, capacity), counters[3] := 0
__global__ __launch_bounds__(kSumsBlock) void k_pl_scan(unsigned* tiles, unsigned ntiles, unsigned* counters, unsigned capacity) {
    __shared__ unsigned lds[kSumsBlock / 64];
    const unsigned total = scan_sums(tiles, 0u, ntiles, lds);
    if (threadIdx.x == 0) {
        counters[2] = min(total, capacity);
        counters[3] = 0u;
    }
}

__global__ __launch_bounds__(256) void k_pl_zero(unsigned* words, unsigned n) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) words[i] = 0u;
}

// ---- votes ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ emf_plane_voxel_t load_record(const emf_plane_voxel_t* records, unsigned i) {
    const float4 v = *reinterpret_cast<const float4*>(records + i);
    emf_plane_voxel_t r;
    r.index = __float_as_int(v.x);
    r.g[0] = v.y, r.g[1] = v.z, r.g[2] = v.w;
    return r;
}

struct DirArgs {
    const emf_plane_voxel_t* records;
    const unsigned* counters;
    unsigned capacity;
    int K;
    float halfK;
    unsigned* bins;
};

__device__ __forceinline__ int cube_cell(float u, int K, float halfK) {
    const int c = static_cast<int>(floorf(__fmul_rn(__fadd_rn(u, 1.f), halfK)));  // u in [-1, 1]: 0 .. K
    return min(c, K - 1);
}

__global__ __launch_bounds__(kPlBlock) void k_pl_directions(const DirArgs a) {
    __shared__ unsigned h[6 * EMF_PLANE_MAX_K * EMF_PLANE_MAX_K];
    const unsigned n = min(a.counters[2], a.capacity);
    const unsigned first = blockIdx.x * kPlChunk;
    if (first >= n) return;  // block-uniform
    const unsigned nb = 6u * a.K * a.K;
    for (unsigned i = threadIdx.x; i < nb; i += kPlBlock) h[i] = 0u;
    __syncthreads();
    const unsigned end = min(n - first, kPlChunk) + first;
    for (unsigned i = first + threadIdx.x; i < end; i += kPlBlock) {
        const emf_plane_voxel_t r = load_record(a.records, i);
        const float a0 = fabsf(r.g[0]), a1 = fabsf(r.g[1]), a2 = fabsf(r.g[2]);
        if (!(finite_f(a0) && finite_f(a1) && finite_f(a2))) continue;
        int m = 0;
        float am = a0;
        if (a1 > am) m = 1, am = a1;
        if (a2 > am) m = 2, am = a2;
        if (!(am > 0.f)) continue;
        const float gm = m == 0 ? r.g[0] : (m == 1 ? r.g[1] : r.g[2]);
        const float gu = m == 0 ? r.g[1] : (m == 1 ? r.g[2] : r.g[0]);
        const float gv = m == 0 ? r.g[2] : (m == 1 ? r.g[0] : r.g[1]);
        const int face = 2 * m + (gm < 0.f ? 1 : 0);
        const int iu = cube_cell(__fdiv_rn(gu, am), a.K, a.halfK), iv = cube_cell(__fdiv_rn(gv, am), a.K, a.halfK);
        atomicAdd(&h[(face * a.K + iv) * a.K + iu], 1u);
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < nb; i += kPlBlock) {
        const unsigned v = h[i];
        if (v) atomicAdd(&a.bins[i], v);
    }
}

struct OffArgs {
    const emf_plane_voxel_t* records;
    const unsigned* counters;
    unsigned capacity;
    int bx, by;
    int D, S;
    float cos2, invBin;
    float n[3 * EMF_PLANE_MAX_DIRS];
    float shift[EMF_PLANE_MAX_DIRS];
    unsigned* hist;
};

__device__ __forceinline__ float dot3(float n0, float n1, float n2, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(n0, x), __fmul_rn(n1, y)), __fmul_rn(n2, z));
}

// a > 0 && a * a >= cos2 * gg, as computed; a NaN aligns with nothing
__device__ __forceinline__ bool is_aligned(float a, float gg, float cos2) {
    return a > 0.f && __fmul_rn(a, a) >= __fmul_rn(cos2, gg);
}

__global__ __launch_bounds__(kPlBlock) void k_pl_offsets(const OffArgs a) {
    const unsigned n = min(a.counters[2], a.capacity);
    if (blockIdx.x * static_cast<unsigned>(kPlBlock) >= n) return;  // block-uniform
    const unsigned i = blockIdx.x * kPlBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = i < n;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, x = 0.f, y = 0.f, z = 0.f;
    if (live) {
        const emf_plane_voxel_t r = load_record(a.records, i);
        g0 = r.g[0], g1 = r.g[1], g2 = r.g[2];
        const int row = r.index / a.bx;
        x = static_cast<float>(r.index - row * a.bx);
        z = static_cast<float>(row / a.by);
        y = static_cast<float>(row - (row / a.by) * a.by);
    }
    const float gg = dot3(g0, g1, g2, g0, g1, g2);
    // every lane of the wave is here: a lane without a vote has destination -1 and adds nothing
    for (int k = 0; k < a.D; ++k) {
        const float n0 = a.n[3 * k], n1 = a.n[3 * k + 1], n2 = a.n[3 * k + 2];
        int dest = -1;
        if (live && is_aligned(dot3(n0, n1, n2, g0, g1, g2), gg, a.cos2)) {
            const float s = floorf(__fadd_rn(__fmul_rn(dot3(n0, n1, n2, x, y, z), a.invBin), a.shift[k]));
            if (s >= 0.f && s < static_cast<float>(a.S)) dest = k * a.S + static_cast<int>(s);
        }
        const int run = run_id(dest, lane);
        const unsigned votes = run_scan<OpAdd>(dest >= 0 ? 1u : 0u, lane, run);
        if (run_is_last(run, lane) && dest >= 0) atomicAdd(&a.hist[dest], votes);
    }
}

struct AssignArgs {
    const emf_plane_voxel_t* records;
    const unsigned* counters;
    unsigned capacity;
    int bx, by, bz;
    int P;
    float cos2, band;
    float planes[4 * EMF_PLANE_MAX_PLANES];  // n0, n1, n2, d
    int16_t* labels;
    emf_plane_moments_t* moments;
};
static_assert(sizeof(AssignArgs) <= 4096, "AssignArgs travels in the kernel arguments");

__global__ __launch_bounds__(256) void k_pl_assign_init(emf_plane_moments_t* moments, int P, int bx, int by, int bz) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P) return;
    emf_plane_moments_t m{};
    m.lo[0] = bx, m.lo[1] = by, m.lo[2] = bz;
    m.hi[0] = m.hi[1] = m.hi[2] = -1;
    moments[k] = m;
}

__global__ __launch_bounds__(kPlBlock) void k_pl_assign(const AssignArgs a) {
    const unsigned n = min(a.counters[2], a.capacity);
    if (blockIdx.x * static_cast<unsigned>(kPlBlock) >= n) return;  // block-uniform
    const unsigned i = blockIdx.x * kPlBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = i < n;
    int label = -1, ix = 0, iy = 0, iz = 0;
    if (live) {
        const emf_plane_voxel_t r = load_record(a.records, i);
        const int row = r.index / a.bx;
        ix = r.index - row * a.bx;
        iz = row / a.by;
        iy = row - iz * a.by;
        const float x = static_cast<float>(ix), y = static_cast<float>(iy), z = static_cast<float>(iz);
        const float gg = dot3(r.g[0], r.g[1], r.g[2], r.g[0], r.g[1], r.g[2]);
        float best = 0.f;
        for (int k = 0; k < a.P; ++k) {
            const float n0 = a.planes[4 * k], n1 = a.planes[4 * k + 1], n2 = a.planes[4 * k + 2];
            if (!is_aligned(dot3(n0, n1, n2, r.g[0], r.g[1], r.g[2]), gg, a.cos2)) continue;
            const float e = fabsf(__fsub_rn(dot3(n0, n1, n2, x, y, z), a.planes[4 * k + 3]));
            if (e <= a.band && (label < 0 || e < best)) label = k, best = e;
        }
        a.labels[i] = static_cast<int16_t>(label);
    }
    if (__ballot(label >= 0) == 0ull) return;  // wave-uniform
    // count, x, y, z, xx, yy, zz, xy, xz, yz of the run's lanes that are not above this one: at most 64 * 2047^2 < 2^32
    const unsigned ux = ix, uy = iy, uz = iz, in = label >= 0 ? 1u : 0u;
    unsigned s[10] = {in, ux, uy, uz, ux * ux, uy * uy, uz * uz, ux * uy, ux * uz, uy * uz};
    int lo[3] = {ix, iy, iz}, hi[3] = {ix, iy, iz};
    const int run = run_id(label, lane);
#pragma unroll
    for (int q = 0; q < 10; ++q) s[q] = run_scan<OpAdd>(s[q], lane, run);
#pragma unroll
    for (int j = 0; j < 3; ++j) lo[j] = run_scan<OpMin>(lo[j], lane, run), hi[j] = run_scan<OpMax>(hi[j], lane, run);
    if (!run_is_last(run, lane) || label < 0) return;  // not the last lane of a run of members
    emf_plane_moments_t* m = a.moments + label;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(m);  // count, sum[3], sum2[6]: the record's first ten words
#pragma unroll
    for (int q = 0; q < 10; ++q)
        if (s[q]) atomicAdd(w + q, static_cast<unsigned long long>(s[q]));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        atomicMin(&m->lo[j], lo[j]);
        atomicMax(&m->hi[j], hi[j]);
    }
}

// ---- stage 4: patches -----------------------------------------------------------------------------------------------
// The patch array is the union-find's parent array over RECORD indices (union_find.hpp): a member holds an index <= its
// own, every other record the sentinel -1, which is never followed and never changes.  There is no dense volume: the
// record of a neighbouring voxel is found by binary search of that voxel's tile-order key among the records' own keys.

constexpr unsigned kPpNone = 0xffffffffu;

static_assert(sizeof(emf_plane_patch_t) == 128, "mirrored by emfusion_amd/_lib.py");

struct PatchBox {
    int bx, by, bz;
    unsigned ntx, nty, voxels;
};

// tile(v) * 2048 + within(v): strictly increasing along stage 1's order; at most 2^22 tiles, so below 2^33
__device__ __forceinline__ unsigned long long voxel_key(const PatchBox& b, int x, int y, int z) {
    const unsigned tile = (static_cast<unsigned>(z >> 3) * b.nty + static_cast<unsigned>(y >> 3)) * b.ntx + static_cast<unsigned>(x >> 5);
    const unsigned within = (static_cast<unsigned>(z & 7) << 8) | (static_cast<unsigned>(y & 7) << 5) | static_cast<unsigned>(x & 31);
    return (static_cast<unsigned long long>(tile) << 11) | within;
}

// the box voxel of a linear index; false for an index outside the box, which then has no voxel
__device__ __forceinline__ bool index_voxel(const PatchBox& b, int index, int& x, int& y, int& z) {
    if (index < 0 || static_cast<unsigned>(index) >= b.voxels) return false;
    const int row = index / b.bx;
    x = index - row * b.bx;
    z = row / b.by;
    y = row - z * b.by;
    return true;
}

// the key of record i; ~0 (the key of no voxel) where its index lies outside the box
__device__ __forceinline__ unsigned long long record_key(const emf_plane_voxel_t* __restrict__ records, const PatchBox& b, unsigned i) {
    int x, y, z;
    return index_voxel(b, records[i].index, x, y, z) ? voxel_key(b, x, y, z) : ~0ull;
}

// the record whose key is `key` among the first n (> 0), or kPpNone.  Bounded by n whatever the records hold.
__device__ __forceinline__ unsigned record_of(const emf_plane_voxel_t* __restrict__ records, const PatchBox& b, unsigned n,
                                              unsigned long long key) {
    unsigned lo = 0u, hi = n;  // key(lo) <= key < key(hi) once lo's holds
    while (hi - lo > 1u) {
        const unsigned mid = (lo + hi) >> 1;
        if (record_key(records, b, mid) <= key) lo = mid;
        else hi = mid;
    }
    return record_key(records, b, lo) == key ? lo : kPpNone;
}

struct PatchLabelArgs {
    const emf_plane_voxel_t* records;
    const int16_t* labels;
    const unsigned* counters;
    unsigned capacity;
    PatchBox box;
    int reach;
    unsigned* parent;         // the patch array
    unsigned* patchCounters;  // EMF_PATCH_*
};

__global__ __launch_bounds__(kPlBlock) void k_pp_init(const PatchLabelArgs a) {
    const unsigned n = min(a.counters[2], a.capacity);
    const unsigned i = blockIdx.x * kPlBlock + threadIdx.x;
    if (i < n) a.parent[i] = a.labels[i] >= 0 ? i : kPpNone;
}

// per member: unite with the members of the same label among the voxels that precede its own in (z, y, x) order and lie
// within `reach` of it -- every pair of the (2 reach + 1)^3 neighbourhood once: 13 offsets at reach 1, 62 at reach 2
__global__ __launch_bounds__(kPlBlock) void k_pp_hook(const PatchLabelArgs a) {
    const unsigned n = min(a.counters[2], a.capacity);
    const unsigned i = blockIdx.x * kPlBlock + threadIdx.x;
    if (i >= n) return;
    const int label = a.labels[i];
    int x, y, z;
    if (label < 0 || !index_voxel(a.box, a.records[i].index, x, y, z)) return;
    const int R = a.reach;
    for (int dz = -R; dz <= 0; ++dz) {
        const int qz = z + dz;
        if (qz < 0) continue;
        for (int dy = -R; dy <= (dz < 0 ? R : 0); ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= a.box.by) continue;
            for (int dx = -R; dx <= (dz < 0 || dy < 0 ? R : -1); ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= a.box.bx) continue;
                const unsigned j = record_of(a.records, a.box, n, voxel_key(a.box, qx, qy, qz));
                if (j != kPpNone && a.labels[j] == label) unite(a.parent, i, j);
            }
        }
    }
}

// patch[i] := root of i, the smallest record index of the patch whatever order the hooks ran in; members and roots counted
__global__ __launch_bounds__(kPlBlock) void k_pp_flatten(const PatchLabelArgs a) {
    __shared__ unsigned lds[kPlBlock / 64];
    const unsigned n = min(a.counters[2], a.capacity);
    if (blockIdx.x * static_cast<unsigned>(kPlBlock) >= n) return;  // block-uniform
    const unsigned i = blockIdx.x * kPlBlock + threadIdx.x;
    unsigned flags = 0u;  // member | root << 16: both at most 256 over the workgroup
    if (i < n && load_parent(a.parent, i) != kPpNone) {
        const unsigned r = find_root(a.parent, i);
        atomicMin(a.parent + i, r);  // (a halving step of another lane may still be under way: the minimum wins)
        flags = 1u | (r == i ? 1u << 16 : 0u);
    }
    unsigned total;
    block_exclusive_scan<kPlBlock / 64>(flags, total, lds);
    if (threadIdx.x == 0) {
        if (total & 0xffffu) atomicAdd(&a.patchCounters[EMF_PATCH_MEMBERS], total & 0xffffu);
        if (total >> 16) atomicAdd(&a.patchCounters[EMF_PATCH_PATCHES], total >> 16);
    }
}

struct PatchArgs {
    const emf_plane_voxel_t* records;
    const int16_t* labels;
    const unsigned* patch;
    const unsigned* counters;
    unsigned capacity;
    PatchBox box;
    int P;
    unsigned long long minCount;
    emf_plane_patch_t* slots;  // per slot; the four floats hold their u32 keys until k_pp_emit
    unsigned* roots;           // per slot, ascending
    unsigned* bsums;           // blocks + 1
    unsigned* csums;           // cblocks + 1
    unsigned nc, blocks, cblocks;
    emf_plane_patch_t* out;
    unsigned capacityOut;
    unsigned* kept;
    float axes[6 * EMF_PLANE_MAX_PLANES];  // u0, u1, u2, v0, v1, v2 per plane
};
static_assert(sizeof(PatchArgs) <= 4096, "PatchArgs travels in the kernel arguments");

inline size_t place(PatchArgs& a, unsigned capacity, unsigned nPatches, void* scratch) {
    a.nc = min(nPatches, capacity);
    a.blocks = ceil_div(capacity, kPlBlock);
    a.cblocks = ceil_div(a.nc, kPlBlock);
    ScratchArena s{static_cast<char*>(scratch), 0};
    a.slots = s.take<emf_plane_patch_t>(a.nc);
    a.roots = s.take<unsigned>(a.nc);
    a.bsums = s.take<unsigned>(static_cast<size_t>(a.blocks) + 1);
    a.csums = s.take<unsigned>(static_cast<size_t>(a.cblocks) + 1);
    return s.off;
}

__device__ __forceinline__ unsigned pp_root_flag(const PatchArgs& a, unsigned n, unsigned i) {
    return i < n && a.patch[i] == i ? 1u : 0u;
}

__global__ __launch_bounds__(kPlBlock) void k_pp_rootsums(const PatchArgs a) {
    __shared__ unsigned lds[kPlBlock / 64];
    const unsigned n = min(a.counters[2], a.capacity);
    if (blockIdx.x * static_cast<unsigned>(kPlBlock) >= n) return;  // block-uniform; k_pp_scan stops at n as well
    unsigned total;
    block_exclusive_scan<kPlBlock / 64>(pp_root_flag(a, n, blockIdx.x * kPlBlock + threadIdx.x), total, lds);
    if (threadIdx.x == 0) a.bsums[blockIdx.x] = total;
}

// one workgroup: the exclusive scan of the sums of the workgroups that hold records (of all `count` sums where counters
// is NULL); the total goes behind the last sum
__global__ __launch_bounds__(kSumsBlock) void k_pp_scan(unsigned* sums, unsigned count, const unsigned* counters, unsigned capacity) {
    __shared__ unsigned lds[kSumsBlock / 64];
    const unsigned used = counters ? (min(counters[2], capacity) + kPlBlock - 1u) / kPlBlock : count;
    const unsigned total = scan_sums(sums, 0u, used, lds);
    if (threadIdx.x == 0) sums[count] = total;
}

__global__ __launch_bounds__(kPlBlock) void k_pp_roots(const PatchArgs a) {
    __shared__ unsigned lds[kPlBlock / 64];
    const unsigned n = min(a.counters[2], a.capacity);
    if (blockIdx.x * static_cast<unsigned>(kPlBlock) >= n) return;  // block-uniform
    const unsigned i = blockIdx.x * kPlBlock + threadIdx.x;
    const unsigned flag = pp_root_flag(a, n, i);
    unsigned total;
    const unsigned rank = a.bsums[blockIdx.x] + block_exclusive_scan<kPlBlock / 64>(flag, total, lds);
    if (!flag || rank >= a.nc) return;
    a.roots[rank] = i;
    emf_plane_patch_t s{};
    s.id = static_cast<int32_t>(i);
    s.plane = a.labels[i];
    s.lo[0] = a.box.bx, s.lo[1] = a.box.by, s.lo[2] = a.box.bz;
    s.hi[0] = s.hi[1] = s.hi[2] = -1;
    s.ulo = s.vlo = __uint_as_float(0xff800000u);  // the key of +inf
    s.uhi = s.vhi = __uint_as_float(0x007fffffu);  // the key of -inf
    a.slots[rank] = s;
}

// v, through a DPP move with the identity lane pattern: a value the compiler cannot look through.  A build with
// -ffp-contract=fast fuses a product into a neighbouring sum whatever a pragma or an _rn intrinsic says; a product
// that went through here is no product to it any more.
__device__ __forceinline__ float pp_rounded(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xE4 /* quad_perm 0, 1, 2, 3 */, 0xf, 0xf, false));
}

// (a0 * x + a1 * y) + a2 * z as five single float32 operations, whatever the build
__device__ __forceinline__ float pp_extent(float a0, float a1, float a2, float x, float y, float z) {
    const float p0 = pp_rounded(__fmul_rn(a0, x)), p1 = pp_rounded(__fmul_rn(a1, y)), p2 = pp_rounded(__fmul_rn(a2, z));
    return __fadd_rn(__fadd_rn(p0, p1), p2);
}

// the order-preserving map of the f32 bits to u32 that emf_hip_shapeExtents documents, and back
__device__ __forceinline__ unsigned pp_float_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ unsigned pp_key_bits(unsigned k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// the slot of the patch `id` among the first nc sorted roots, or kPpNone
__device__ __forceinline__ unsigned pp_slot_of(const unsigned* __restrict__ roots, unsigned nc, unsigned id) {
    unsigned lo = 0u, hi = nc;
    while (hi - lo > 1u) {
        const unsigned mid = (lo + hi) >> 1;
        if (roots[mid] <= id) lo = mid;
        else hi = mid;
    }
    return nc != 0u && roots[lo] == id ? lo : kPpNone;
}

// one lane per record; the ten sums, six bounds and four extent keys per run of equal patches in a wave, then one
// integer atomic per quantity and run.  Over run numbers (run_id): a patch can come back within a wave.
__global__ __launch_bounds__(kPlBlock) void k_pp_stats(const PatchArgs a) {
    const unsigned n = min(a.counters[2], a.capacity);
    if (blockIdx.x * static_cast<unsigned>(kPlBlock) >= n) return;  // block-uniform
    const unsigned i = blockIdx.x * kPlBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int id = -1, ix = 0, iy = 0, iz = 0;
    unsigned k[4] = {0xffffffffu, 0u, 0xffffffffu, 0u};  // ulo, uhi, vlo, vhi: neutral
    if (i < n) {
        id = static_cast<int>(a.patch[i]);  // below 2^31 - 1: the capacity is
        if (id >= 0) {
            if (!index_voxel(a.box, a.records[i].index, ix, iy, iz)) ix = iy = iz = 0;
            const int plane = a.labels[i];
            if (plane >= 0 && plane < a.P) {
                const float x = static_cast<float>(ix), y = static_cast<float>(iy), z = static_cast<float>(iz);
                const float* ax = a.axes + 6 * plane;
                k[0] = k[1] = pp_float_key(pp_extent(ax[0], ax[1], ax[2], x, y, z));
                k[2] = k[3] = pp_float_key(pp_extent(ax[3], ax[4], ax[5], x, y, z));
            }
        }
    }
    if (__ballot(id >= 0) == 0ull) return;  // wave-uniform
    // count, x, y, z, xx, yy, zz, xy, xz, yz of the run's lanes that are not above this one: at most 64 * 2047^2 < 2^32;
    // a patch's totals stay below 2^31 * 2047^2 < 2^53
    const unsigned ux = ix, uy = iy, uz = iz, in = id >= 0 ? 1u : 0u;
    unsigned s[10] = {in, ux, uy, uz, ux * ux, uy * uy, uz * uz, ux * uy, ux * uz, uy * uz};
    int lo[3] = {ix, iy, iz}, hi[3] = {ix, iy, iz};
    const int run = run_id(id, lane);
#pragma unroll
    for (int q = 0; q < 10; ++q) s[q] = run_scan<OpAdd>(s[q], lane, run);
#pragma unroll
    for (int j = 0; j < 3; ++j) lo[j] = run_scan<OpMin>(lo[j], lane, run), hi[j] = run_scan<OpMax>(hi[j], lane, run);
    k[0] = run_scan<OpMin>(k[0], lane, run), k[1] = run_scan<OpMax>(k[1], lane, run);
    k[2] = run_scan<OpMin>(k[2], lane, run), k[3] = run_scan<OpMax>(k[3], lane, run);
    if (!run_is_last(run, lane) || id < 0) return;  // not the last lane of a run of members
    const unsigned slot = pp_slot_of(a.roots, min(a.nc, a.bsums[a.blocks]), static_cast<unsigned>(id));
    if (slot == kPpNone) return;  // a patch beyond n_patches
    emf_plane_patch_t* m = a.slots + slot;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(m) + 1;  // count, sum[3], sum2[6] behind id and plane
#pragma unroll
    for (int q = 0; q < 10; ++q)
        if (s[q]) atomicAdd(w + q, static_cast<unsigned long long>(s[q]));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        atomicMin(&m->lo[j], lo[j]);
        atomicMax(&m->hi[j], hi[j]);
    }
    unsigned* e = reinterpret_cast<unsigned*>(&m->ulo);
    atomicMin(e, k[0]);
    atomicMax(e + 1, k[1]);
    atomicMin(e + 2, k[2]);
    atomicMax(e + 3, k[3]);
}

__device__ __forceinline__ unsigned pp_keep_flag(const PatchArgs& a, unsigned nc, unsigned s) {
    return s < nc && a.slots[s].count >= a.minCount ? 1u : 0u;
}

__global__ __launch_bounds__(kPlBlock) void k_pp_keepsums(const PatchArgs a) {
    __shared__ unsigned lds[kPlBlock / 64];
    const unsigned nc = min(a.nc, a.bsums[a.blocks]);  // the slots k_pp_roots did fill
    unsigned total;
    block_exclusive_scan<kPlBlock / 64>(pp_keep_flag(a, nc, blockIdx.x * kPlBlock + threadIdx.x), total, lds);
    if (threadIdx.x == 0) a.csums[blockIdx.x] = total;
}

// kept slots write their record at their rank (id order: the slots are sorted by id) while the rank is below the
// capacity; the keys become the bits of the floats; thread 0 writes the kept total
__global__ __launch_bounds__(kPlBlock) void k_pp_emit(const PatchArgs a) {
    __shared__ unsigned lds[kPlBlock / 64];
    const unsigned nc = min(a.nc, a.bsums[a.blocks]);
    const unsigned s = blockIdx.x * kPlBlock + threadIdx.x;
    const unsigned flag = pp_keep_flag(a, nc, s);
    unsigned total;
    const unsigned rank = a.csums[blockIdx.x] + block_exclusive_scan<kPlBlock / 64>(flag, total, lds);
    if (s == 0u) *a.kept = a.csums[a.cblocks];
    if (!flag || rank >= a.capacityOut) return;
    emf_plane_patch_t r = a.slots[s];
    r.ulo = __uint_as_float(pp_key_bits(__float_as_uint(r.ulo)));
    r.uhi = __uint_as_float(pp_key_bits(__float_as_uint(r.uhi)));
    r.vlo = __uint_as_float(pp_key_bits(__float_as_uint(r.vlo)));
    r.vhi = __uint_as_float(pp_key_bits(__float_as_uint(r.vhi)));
    a.out[rank] = r;
}

// ---- host: the checks; nothing is enqueued by them --------------------------------------------------------------

int check_size(const int32_t size[3], const char* who) {
    if (!size) return fail(EMF_E_ARG, "%s: box_size is NULL", who);
    for (int i = 0; i < 3; ++i) {
        if (size[i] < 1) return fail(EMF_E_ARG, "%s: box axis %d has %d voxels", who, i, size[i]);
        if (size[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "%s: box axis %d has %d voxels, above %d", who, i, size[i], EMF_DF_MAX_AXIS);
    }
    const unsigned long long voxels = static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]);
    if (voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "%s: a box of %llu voxels, above 2^31 - 1", who, voxels);
    return EMF_OK;
}

unsigned long long tiles_of(const int32_t size[3]) {
    return static_cast<unsigned long long>((size[0] + kPlTX - 1) / kPlTX) * ((size[1] + kPlTY - 1) / kPlTY) *
           ((size[2] + kPlTZ - 1) / kPlTZ);
}

PatchBox patch_box(const int32_t size[3]) {  // of a size check_size has passed
    PatchBox b;
    b.bx = size[0], b.by = size[1], b.bz = size[2];
    b.ntx = (size[0] + kPlTX - 1) / kPlTX, b.nty = (size[1] + kPlTY - 1) / kPlTY;
    b.voxels = static_cast<unsigned>(size[0]) * size[1] * static_cast<unsigned>(size[2]);
    return b;
}

// the record list of the entries that read one
int check_records(const char* who, const emf_plane_voxel_t* records, const uint32_t* counters, uint32_t capacity) {
    if (!records || !counters) return fail(EMF_E_ARG, "%s: the records or the counters are NULL", who);
    if ((reinterpret_cast<uintptr_t>(records) & 15u) || (reinterpret_cast<uintptr_t>(counters) & 3u))
        return fail(EMF_E_ARG, "%s: misaligned records or counters", who);
    if (capacity < 1u) return fail(EMF_E_ARG, "%s: a capacity of 0 records", who);
    if (capacity > 0x7fffffffu) return fail(EMF_E_LIMIT, "%s: a capacity of %u records, above 2^31 - 1", who, capacity);
    return EMF_OK;
}

int check_gate(const char* who, float cos2) {
    if (!(cos2 >= 0.f && cos2 <= 1.f)) return fail(EMF_E_ARG, "%s: cos2 %g outside 0 .. 1", who, static_cast<double>(cos2));
    return EMF_OK;
}

void zero(unsigned* words, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_pl_zero, dim3(ceil_div(n, 256)), dim3(256), 0, s, words, static_cast<unsigned>(n));
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

size_t emf_hip_planeSurfaceScratchBytes(const int32_t box_size[3]) {
    if (!box_size) return 0;
    for (int i = 0; i < 3; ++i)
        if (box_size[i] < 1 || box_size[i] > EMF_DF_MAX_AXIS) return 0;
    const unsigned long long tiles = tiles_of(box_size);
    return tiles > kPlMaxTiles ? 0 : static_cast<size_t>(tiles) * sizeof(uint32_t);
}

int emf_hip_planeSurface(const float* tsdf, const float* weights, const int32_t res[3], const int32_t box_lo[3],
                         const int32_t box_size[3], const uint8_t* unseenTiles, emf_plane_voxel_t* records, uint32_t capacity,
                         uint32_t* counters, void* scratch, emf_stream_t stream) {
    if (!tsdf || !weights || !counters || !scratch) return fail(EMF_E_ARG, "planeSurface: tsdf, weights, counters or scratch is NULL");
    if (!res || !box_lo) return fail(EMF_E_ARG, "planeSurface: res or box_lo is NULL");
    EMF_TRY(check_size(box_size, "planeSurface"));
    for (int i = 0; i < 3; ++i)
        if (res[i] < 1 || box_lo[i] < 0 || box_lo[i] > res[i] - box_size[i])
            return fail(EMF_E_ARG, "planeSurface: the box [%d, %d + %d) leaves the volume's axis %d of %d voxels", box_lo[i],
                        box_lo[i], box_size[i], i, res[i]);
    const unsigned long long voxels = static_cast<unsigned long long>(res[0]) * res[1] * static_cast<unsigned long long>(res[2]);
    if (voxels > (1ull << 36)) return fail(EMF_E_LIMIT, "planeSurface: volume of %llu voxels exceeds 2^36", voxels);
    const unsigned long long tiles = tiles_of(box_size);
    if (tiles > kPlMaxTiles) return fail(EMF_E_LIMIT, "planeSurface: more than 2^24 - 1 tiles");
    if (capacity > 0u && !records) return fail(EMF_E_ARG, "planeSurface: a capacity of %u records and no records", capacity);
    if (capacity > 0x7fffffffu) return fail(EMF_E_LIMIT, "planeSurface: a capacity of %u records, above 2^31 - 1", capacity);
    if (((reinterpret_cast<uintptr_t>(tsdf) | reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(counters) |
          reinterpret_cast<uintptr_t>(scratch)) & 3u) || (reinterpret_cast<uintptr_t>(records) & 15u))
        return fail(EMF_E_ARG, "planeSurface: misaligned arrays");
    SurfArgs a{};
    a.tsdf = tsdf, a.weights = weights, a.unseen = unseenTiles, a.records = records;
    a.tiles = static_cast<unsigned*>(scratch), a.counters = counters;
    a.res = i3_from(res), a.lo = i3_from(box_lo), a.size = i3_from(box_size);
    a.ntx = (box_size[0] + kPlTX - 1) / kPlTX, a.nty = (box_size[1] + kPlTY - 1) / kPlTY;
    a.ntiles = static_cast<unsigned>(tiles);
    a.capacity = capacity;
    const hipStream_t s = as_stream(stream);
    zero(counters, 4, s);
    hipLaunchKernelGGL(k_pl_surface<false>, dim3(a.ntiles), dim3(kPlBlock), 0, s, a);
    hipLaunchKernelGGL(k_pl_scan, dim3(1), dim3(kSumsBlock), 0, s, a.tiles, a.ntiles, counters, capacity);
    if (capacity > 0u) hipLaunchKernelGGL(k_pl_surface<true>, dim3(a.ntiles), dim3(kPlBlock), 0, s, a);
    return launch_status("planeSurface");
}

int emf_hip_planeDirections(const emf_plane_voxel_t* records, const uint32_t* counters, uint32_t capacity, int32_t K,
                            uint32_t* bins, emf_stream_t stream) {
    EMF_TRY(check_records("planeDirections", records, counters, capacity));
    if (K < 1) return fail(EMF_E_ARG, "planeDirections: %d cells per face side", K);
    if (K > EMF_PLANE_MAX_K) return fail(EMF_E_LIMIT, "planeDirections: %d cells per face side, above %d", K, EMF_PLANE_MAX_K);
    if (!bins || (reinterpret_cast<uintptr_t>(bins) & 3u)) return fail(EMF_E_ARG, "planeDirections: the bins are NULL or misaligned");
    const DirArgs a{records, counters, capacity, K, static_cast<float>(K) / 2.f, bins};
    const hipStream_t s = as_stream(stream);
    zero(bins, 6u * K * K, s);
    hipLaunchKernelGGL(k_pl_directions, dim3(ceil_div(capacity, kPlChunk)), dim3(kPlBlock), 0, s, a);
    return launch_status("planeDirections");
}

int emf_hip_planeOffsets(const emf_plane_voxel_t* records, const uint32_t* counters, uint32_t capacity,
                         const int32_t box_size[3], const float* dirs_host, const float* shift_host, int32_t D, float cos2,
                         float inv_bin, int32_t S, uint32_t* hist, emf_stream_t stream) {
    EMF_TRY(check_records("planeOffsets", records, counters, capacity));
    EMF_TRY(check_size(box_size, "planeOffsets"));
    if (!dirs_host || !shift_host) return fail(EMF_E_ARG, "planeOffsets: the directions or the shifts are NULL");
    if (D < 1 || S < 1) return fail(EMF_E_ARG, "planeOffsets: %d directions of %d slots", D, S);
    if (D > EMF_PLANE_MAX_DIRS) return fail(EMF_E_LIMIT, "planeOffsets: %d directions, above %d", D, EMF_PLANE_MAX_DIRS);
    if (S > EMF_PLANE_MAX_SLOTS) return fail(EMF_E_LIMIT, "planeOffsets: %d slots, above %d", S, EMF_PLANE_MAX_SLOTS);
    EMF_TRY(check_gate("planeOffsets", cos2));
    if (!hist || (reinterpret_cast<uintptr_t>(hist) & 3u)) return fail(EMF_E_ARG, "planeOffsets: the histogram is NULL or misaligned");
    OffArgs a{};
    a.records = records, a.counters = counters, a.capacity = capacity;
    a.bx = box_size[0], a.by = box_size[1];
    a.D = D, a.S = S, a.cos2 = cos2, a.invBin = inv_bin;
    std::memcpy(a.n, dirs_host, sizeof(float) * 3 * D);
    std::memcpy(a.shift, shift_host, sizeof(float) * D);
    a.hist = hist;
    const hipStream_t s = as_stream(stream);
    zero(hist, static_cast<size_t>(D) * S, s);
    hipLaunchKernelGGL(k_pl_offsets, dim3(ceil_div(capacity, kPlBlock)), dim3(kPlBlock), 0, s, a);
    return launch_status("planeOffsets");
}

int emf_hip_planeAssign(const emf_plane_voxel_t* records, const uint32_t* counters, uint32_t capacity,
                        const int32_t box_size[3], const float* planes_host, int32_t P, float cos2, float band,
                        int16_t* labels, emf_plane_moments_t* moments, emf_stream_t stream) {
    EMF_TRY(check_records("planeAssign", records, counters, capacity));
    EMF_TRY(check_size(box_size, "planeAssign"));
    if (!planes_host) return fail(EMF_E_ARG, "planeAssign: the planes are NULL");
    if (P < 1) return fail(EMF_E_ARG, "planeAssign: %d planes", P);
    if (P > EMF_PLANE_MAX_PLANES) return fail(EMF_E_LIMIT, "planeAssign: %d planes, above %d", P, EMF_PLANE_MAX_PLANES);
    EMF_TRY(check_gate("planeAssign", cos2));
    if (!(band >= 0.f)) return fail(EMF_E_ARG, "planeAssign: a band of %g voxels", static_cast<double>(band));
    if (!labels || !moments) return fail(EMF_E_ARG, "planeAssign: the labels or the moments are NULL");
    if ((reinterpret_cast<uintptr_t>(labels) & 1u) || (reinterpret_cast<uintptr_t>(moments) & 7u))
        return fail(EMF_E_ARG, "planeAssign: misaligned labels or moments");
    AssignArgs a{};
    a.records = records, a.counters = counters, a.capacity = capacity;
    a.bx = box_size[0], a.by = box_size[1], a.bz = box_size[2];
    a.P = P, a.cos2 = cos2, a.band = band;
    std::memcpy(a.planes, planes_host, sizeof(float) * 4 * P);
    a.labels = labels, a.moments = moments;
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_pl_assign_init, dim3(1), dim3(256), 0, s, moments, P, a.bx, a.by, a.bz);
    hipLaunchKernelGGL(k_pl_assign, dim3(ceil_div(capacity, kPlBlock)), dim3(kPlBlock), 0, s, a);
    return launch_status("planeAssign");
}

int emf_hip_planePatchLabel(const emf_plane_voxel_t* records, const int16_t* labels, const uint32_t* counters, uint32_t capacity,
                            const int32_t box_size[3], int32_t reach, int32_t* patch, uint32_t* patch_counters,
                            emf_stream_t stream) {
    EMF_TRY(check_records("planePatchLabel", records, counters, capacity));
    EMF_TRY(check_size(box_size, "planePatchLabel"));
    if (reach < 1) return fail(EMF_E_ARG, "planePatchLabel: a reach of %d voxels", reach);
    if (reach > EMF_PLANE_MAX_REACH) return fail(EMF_E_LIMIT, "planePatchLabel: a reach of %d voxels, above %d", reach, EMF_PLANE_MAX_REACH);
    if (!labels || !patch || !patch_counters) return fail(EMF_E_ARG, "planePatchLabel: the labels, the patches or their counters are NULL");
    if ((reinterpret_cast<uintptr_t>(labels) & 1u) || ((reinterpret_cast<uintptr_t>(patch) | reinterpret_cast<uintptr_t>(patch_counters)) & 3u))
        return fail(EMF_E_ARG, "planePatchLabel: misaligned labels, patches or counters");
    PatchLabelArgs a{};
    a.records = records, a.labels = labels, a.counters = counters, a.capacity = capacity;
    a.box = patch_box(box_size);
    a.reach = reach;
    a.parent = reinterpret_cast<unsigned*>(patch), a.patchCounters = patch_counters;
    const hipStream_t s = as_stream(stream);
    const dim3 grid(ceil_div(capacity, kPlBlock)), block(kPlBlock);
    zero(patch_counters, 3, s);
    hipLaunchKernelGGL(k_pp_init, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_pp_hook, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_pp_flatten, grid, block, 0, s, a);
    return launch_status("planePatchLabel");
}

size_t emf_hip_planePatchScratchBytes(uint32_t capacity, uint32_t n_patches) {
    if (capacity < 1u || capacity > 0x7fffffffu) return 0;
    PatchArgs a;
    char origin[16];
    return place(a, capacity, n_patches, origin);  // only the offsets are used
}

int emf_hip_planePatches(const emf_plane_voxel_t* records, const int16_t* labels, const int32_t* patch, const uint32_t* counters,
                         uint32_t capacity, const int32_t box_size[3], const float* axes_host, int32_t P, int64_t min_count,
                         uint32_t n_patches, void* scratch, emf_plane_patch_t* out, int32_t capacity_patches,
                         uint32_t* patch_counters, emf_stream_t stream) {
    EMF_TRY(check_records("planePatches", records, counters, capacity));
    EMF_TRY(check_size(box_size, "planePatches"));
    if (!labels || !patch || !patch_counters) return fail(EMF_E_ARG, "planePatches: the labels, the patches or their counters are NULL");
    if (!axes_host) return fail(EMF_E_ARG, "planePatches: the axes are NULL");
    if (P < 1) return fail(EMF_E_ARG, "planePatches: %d planes", P);
    if (P > EMF_PLANE_MAX_PLANES) return fail(EMF_E_LIMIT, "planePatches: %d planes, above %d", P, EMF_PLANE_MAX_PLANES);
    if (min_count < 1) return fail(EMF_E_ARG, "planePatches: a min_count of %lld members", static_cast<long long>(min_count));
    if (capacity_patches < 0) return fail(EMF_E_ARG, "planePatches: a capacity of %d patches", capacity_patches);
    if (capacity_patches > 0 && !out) return fail(EMF_E_ARG, "planePatches: a capacity of %d patches and no patches", capacity_patches);
    if (n_patches && !scratch) return fail(EMF_E_ARG, "planePatches: scratch is NULL");
    if ((reinterpret_cast<uintptr_t>(labels) & 1u) || ((reinterpret_cast<uintptr_t>(patch) | reinterpret_cast<uintptr_t>(patch_counters)) & 3u) ||
        (reinterpret_cast<uintptr_t>(scratch) & 15u) || (reinterpret_cast<uintptr_t>(out) & 7u))
        return fail(EMF_E_ARG, "planePatches: misaligned arrays");
    const hipStream_t s = as_stream(stream);
    if (n_patches == 0u) {
        zero(patch_counters + EMF_PATCH_KEPT, 1, s);
        return launch_status("planePatches");
    }
    PatchArgs a{};
    place(a, capacity, n_patches, scratch);
    a.records = records, a.labels = labels, a.patch = reinterpret_cast<const unsigned*>(patch), a.counters = counters;
    a.capacity = capacity;
    a.box = patch_box(box_size);
    a.P = P;
    a.minCount = static_cast<unsigned long long>(min_count);
    a.out = out, a.capacityOut = static_cast<unsigned>(capacity_patches), a.kept = patch_counters + EMF_PATCH_KEPT;
    std::memcpy(a.axes, axes_host, sizeof(float) * 6 * P);
    const dim3 grid(a.blocks), cgrid(a.cblocks), block(kPlBlock);
    hipLaunchKernelGGL(k_pp_rootsums, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_pp_scan, dim3(1), dim3(kSumsBlock), 0, s, a.bsums, a.blocks, counters, capacity);
    hipLaunchKernelGGL(k_pp_roots, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_pp_stats, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_pp_keepsums, cgrid, block, 0, s, a);
    hipLaunchKernelGGL(k_pp_scan, dim3(1), dim3(kSumsBlock), 0, s, a.csums, a.cblocks, static_cast<const unsigned*>(nullptr), 0u);
    hipLaunchKernelGGL(k_pp_emit, cgrid, block, 0, s, a);
    return launch_status("planePatches");
}

}  // extern "C"
