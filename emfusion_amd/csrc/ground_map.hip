// ground_map.hip -- ground map: a box of class bytes projected along "up" onto ground cells with a bit column of height
// bins per cell, the floor / headroom record of every column and the 2-D classes (include/emf_hip.h "Ground map",
// DESIGN.md 5.24).
//   k_ground_columns  the streaming pass.  One workgroup of 128 lanes per 32 x 8 x 8 tile of the box: a lane takes sixteen
//                     consecutive class bytes of a row with one 16-byte load where the row is aligned, byte by byte on
//                     ragged rows.  A wave none of whose bytes is FREE or OCCUPIED leaves at once.  A lane walks its
//                     sixteen voxels in x order and keeps the bits of the destination word it is in (occ and fre); when
//                     the word changes, the finished one is flushed.  A flush is a wave matter: consecutive lanes with
//                     the same destination word OR their bits (run_scan of wave_ops.hpp) and the last lane of the run issues
//                     the atomics, so with up along x a whole row is one atomic and with up along z a pair of rows
//                     shares theirs.  The flush steps are skipped while no lane of the wave has a word to flush.
//   k_ground_cells    one lane per cell: both columns in registers (at most four words each), walked from the top bin
//                     down with the count of FREE slots directly above; words without an OCC bit go by in one step.
//   k_ground_classes  one lane per cell, plain loads of the eight neighbours' floors.
// Integer atomics only (64-bit OR): the planes do not depend on the order of lanes, waves or workgroups.
#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {
namespace {

constexpr int kGmBlock = 128;
constexpr int kGmTileX = 32, kGmTileY = 8, kGmTileZ = 8;
constexpr unsigned kGmUnknown4 = 0x02020202u;  // four EMF_OCC_UNKNOWN bytes

static_assert(sizeof(emf_ground_frame_t) == 60 && sizeof(emf_ground_cell_t) == 8, "mirrored by emfusion_amd/_lib.py");
static_assert(EMF_OCC_FREE == 0 && EMF_OCC_OCCUPIED == 1 && EMF_OCC_UNKNOWN == 2, "k_ground_columns tests c <= 1");

struct ColumnArgs {
    const uint8_t* classes;
    unsigned long long* occ;
    unsigned long long* fre;
    emf_ground_frame_t f;
    int nx, ny, nz;
    int words;
};

// does one of the four bytes of w have no bit above bit 0 (the exact "has a zero byte" test on the upper seven bits)
__device__ __forceinline__ bool any_known(unsigned w) {
    const unsigned v = w & 0xfefefefeu;
    return ((v - 0x01010101u) & ~v & 0x80808080u) != 0u;
}

// Every lane of the wave is here.  dest < 0: nothing to flush (such lanes form runs that issue nothing).
// The destination itself is the run number: it can come back within a wave, but OR is idempotent and the bits go to the
// word that is the key (wave_ops.hpp), so no run_id and no ballot for it in the seventeen flushes of a lane.
__device__ __forceinline__ void flush(const ColumnArgs& a, int lane, int dest, unsigned long long o, unsigned long long f) {
    if (__ballot(dest >= 0) == 0ull) return;  // wave-uniform
    o = run_scan<OpOr>(o, lane, dest);
    f = run_scan<OpOr>(f, lane, dest);
    if (!run_is_last(dest, lane) || dest < 0) return;
    if (o) atomicOr(a.occ + dest, o);
    if (f) atomicOr(a.fre + dest, f);
}

__global__ __launch_bounds__(kGmBlock) void k_ground_columns(const ColumnArgs a) {
    const int t = threadIdx.x, lane = t & 63;
    const int x0 = static_cast<int>(blockIdx.x) * kGmTileX + 16 * (t & 1);
    const int y = static_cast<int>(blockIdx.y) * kGmTileY + ((t >> 1) & 7);
    const int z = static_cast<int>(blockIdx.z) * kGmTileZ + (t >> 4);
    const int count = (y < a.ny && z < a.nz) ? min(16, a.nx - x0) : 0;  // may be negative: no voxel
    unsigned w0 = kGmUnknown4, w1 = kGmUnknown4, w2 = kGmUnknown4, w3 = kGmUnknown4;
    if (count > 0) {
        const uint8_t* p = a.classes + ((static_cast<size_t>(z) * a.ny + y) * a.nx + x0);
        if (count == 16 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            const uint4 q = *reinterpret_cast<const uint4*>(p);
            w0 = q.x, w1 = q.y, w2 = q.z, w3 = q.w;
        } else {
            unsigned long long lo = 0x0202020202020202ull, hi = lo;  // bytes past the row stay UNKNOWN
            for (int e = 0; e < count; ++e) {
                const unsigned long long b = p[e];
                const int s = 8 * (e & 7);
                if (e < 8) lo = (lo & ~(0xffull << s)) | (b << s);
                else hi = (hi & ~(0xffull << s)) | (b << s);
            }
            w0 = static_cast<unsigned>(lo), w1 = static_cast<unsigned>(lo >> 32);
            w2 = static_cast<unsigned>(hi), w3 = static_cast<unsigned>(hi >> 32);
        }
    }
    // a byte is known (FREE or OCCUPIED) iff it is <= 1, that is iff its upper seven bits are a zero byte
    if (__ballot(any_known(w0) || any_known(w1) || any_known(w2) || any_known(w3)) == 0ull)
        return;  // wave-uniform; the kernel has no barrier

    const float W = static_cast<float>(a.f.map[0]), H = static_cast<float>(a.f.map[1]), B = static_cast<float>(a.f.bins);
    const float fy = static_cast<float>(y), fz = static_cast<float>(z);
    const float* G = a.f.G;
    const float uy = __fmul_rn(G[1], fy), uz = __fmul_rn(G[2], fz);
    const float vy = __fmul_rn(G[5], fy), vz = __fmul_rn(G[6], fz);
    const float hy = __fmul_rn(G[9], fy), hz = __fmul_rn(G[10], fz);
    int cur = -1;  // the destination word this lane is in
    unsigned long long curOcc = 0ull, curFre = 0ull;
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
        const unsigned c = w0 & 0xffu;
        w0 = (w0 >> 8) | (w1 << 24), w1 = (w1 >> 8) | (w2 << 24), w2 = (w2 >> 8) | (w3 << 24), w3 = (w3 >> 8) | (kGmUnknown4 << 24);
        int dest = -1;
        unsigned long long bit = 0ull;
        if (c <= 1u) {
            const float fx = static_cast<float>(x0 + e);
            const float qu = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(G[0], fx), uy), uz), G[3]);
            const float qv = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(G[4], fx), vy), vz), G[7]);
            const float qh = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(G[8], fx), hy), hz), G[11]);
            const float iu = floorf(qu), iv = floorf(qv), ih = floorf(qh);
            if (iu >= 0.f && iu < W && iv >= 0.f && iv < H && ih >= 0.f && ih < B) {
                const int b = static_cast<int>(ih);
                dest = (static_cast<int>(iv) * a.f.map[0] + static_cast<int>(iu)) * a.words + (b >> 6);
                bit = 1ull << (b & 63);
            }
        }
        const bool leave = dest >= 0 && cur >= 0 && dest != cur;
        flush(a, lane, leave ? cur : -1, curOcc, curFre);
        if (leave) curOcc = 0ull, curFre = 0ull;
        if (dest >= 0) {
            cur = dest;
            if (c == EMF_OCC_OCCUPIED) curOcc |= bit;
            else curFre |= bit;
        }
    }
    flush(a, lane, cur, curOcc, curFre);
}

__global__ __launch_bounds__(256) void k_ground_zero(unsigned long long* a, unsigned long long* b, size_t n) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i < n) {
        a[i] = 0ull;
        b[i] = 0ull;
    }
}

__global__ __launch_bounds__(256) void k_ground_cells(const unsigned long long* __restrict__ occ,
                                                      const unsigned long long* __restrict__ fre, int cellsN, int bins,
                                                      int words, int robot, emf_ground_cell_t* __restrict__ cells) {
    const int c = static_cast<int>(blockIdx.x) * 256 + threadIdx.x;
    if (c >= cellsN) return;
    unsigned long long o[4] = {0ull, 0ull, 0ull, 0ull}, f[4] = {0ull, 0ull, 0ull, 0ull};
    const size_t base = static_cast<size_t>(c) * words;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < words) {
            o[w] = occ[base + w];
            f[w] = fre[base + w] & ~o[w];  // FREE: the occ bit clear and the fre bit set
        }
    int floorLevel = -1, top = -1, clear = 0, levels = 0;
    int above = 0;  // consecutive FREE slots directly above the slot in hand
#pragma unroll
    for (int w = 3; w >= 0; --w) {
        if (w >= words) continue;
        const int nb = min(64, bins - 64 * w);  // bits of this word that are slots
        const unsigned long long ow = o[w], fw = f[w];
        if (ow == 0ull) {  // no level in this word: only the run of FREE slots moves
            const unsigned long long full = nb == 64 ? ~0ull : (1ull << nb) - 1ull;
            above = fw == full ? above + nb : __ffsll(static_cast<unsigned long long>(~fw)) - 1;
            continue;
        }
        for (int b = nb - 1; b >= 0; --b) {
            const int k = 64 * w + b;
            if ((ow >> b) & 1ull) {
                if (top < 0) top = k;
                if (above >= robot) {
                    ++levels;
                    floorLevel = k;  // walking down: the last one is the lowest
                    clear = above;
                }
                above = 0;
            } else {
                above = ((fw >> b) & 1ull) ? above + 1 : 0;
            }
        }
    }
    emf_ground_cell_t r;
    r.floor = static_cast<int16_t>(floorLevel);
    r.top = static_cast<int16_t>(top);
    r.clear = static_cast<int16_t>(clear);
    r.levels = static_cast<int16_t>(levels);
    cells[c] = r;
}

__global__ __launch_bounds__(256) void k_ground_classes(const emf_ground_cell_t* __restrict__ cells, int W, int H, int maxStep,
                                                        uint8_t* __restrict__ out) {
    const int c = static_cast<int>(blockIdx.x) * 256 + threadIdx.x;
    if (c >= W * H) return;
    const int v = c / W, u = c - v * W;
    const emf_ground_cell_t me = cells[c];
    unsigned cls;
    if (me.floor < 0) {
        cls = me.top >= 0 ? EMF_OCC_OCCUPIED : EMF_OCC_UNKNOWN;
    } else {
        cls = EMF_OCC_FREE;
        for (int dv = -1; dv <= 1; ++dv)
            for (int du = -1; du <= 1; ++du) {
                const int nu = u + du, nv = v + dv;
                if ((du == 0 && dv == 0) || nu < 0 || nu >= W || nv < 0 || nv >= H) continue;
                const int fn = cells[nv * W + nu].floor;
                if (fn >= 0 && abs(static_cast<int>(me.floor) - fn) > maxStep) cls = EMF_OCC_OCCUPIED;
            }
    }
    out[c] = static_cast<uint8_t>(cls);
}

int check_map(const char* who, const int32_t map[2]) {
    if (!map) return fail(EMF_E_ARG, "%s: map is NULL", who);
    for (int i = 0; i < 2; ++i) {
        if (map[i] < 1) return fail(EMF_E_ARG, "%s: the map has %d cells on axis %d", who, map[i], i);
        if (map[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "%s: the map has %d cells on axis %d, above %d", who, map[i], i, EMF_DF_MAX_AXIS);
    }
    return EMF_OK;
}

int check_bins(const char* who, int32_t bins) {
    if (bins < 1) return fail(EMF_E_ARG, "%s: %d height bins", who, bins);
    if (bins > EMF_GROUND_MAX_BINS) return fail(EMF_E_LIMIT, "%s: %d height bins, above %d", who, bins, EMF_GROUND_MAX_BINS);
    return EMF_OK;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_groundColumns(const uint8_t* classes_dev, const int32_t size[3], emf_ground_frame_t frame, uint64_t* occ_dev,
                          uint64_t* fre_dev, emf_stream_t stream) {
    if (!classes_dev || !size || !occ_dev || !fre_dev) return fail(EMF_E_ARG, "groundColumns: a NULL pointer");
    for (int i = 0; i < 3; ++i) {
        if (size[i] < 1) return fail(EMF_E_ARG, "groundColumns: box axis %d has %d voxels", i, size[i]);
        if (size[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "groundColumns: box axis %d has %d voxels, above %d", i, size[i], EMF_DF_MAX_AXIS);
    }
    const unsigned long long voxels = static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]);
    if (voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "groundColumns: a box of %llu voxels, above 2^31 - 1", voxels);
    EMF_TRY(check_map("groundColumns", frame.map));
    EMF_TRY(check_bins("groundColumns", frame.bins));
    if ((reinterpret_cast<uintptr_t>(occ_dev) | reinterpret_cast<uintptr_t>(fre_dev)) & 7u)
        return fail(EMF_E_ARG, "groundColumns: a misaligned plane");
    if (occ_dev == fre_dev) return fail(EMF_E_ARG, "groundColumns: occ and fre are the same plane");
    ColumnArgs a{};
    a.classes = classes_dev;
    a.occ = reinterpret_cast<unsigned long long*>(occ_dev);
    a.fre = reinterpret_cast<unsigned long long*>(fre_dev);
    a.f = frame;
    a.nx = size[0], a.ny = size[1], a.nz = size[2];
    a.words = (frame.bins + 63) / 64;
    const size_t n = static_cast<size_t>(frame.map[0]) * frame.map[1] * a.words;  // at most 2^24
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ground_zero, dim3(ceil_div(n, 256)), dim3(256), 0, s, a.occ, a.fre, n);
    hipLaunchKernelGGL(k_ground_columns,
                       dim3(ceil_div(a.nx, kGmTileX), ceil_div(a.ny, kGmTileY), ceil_div(a.nz, kGmTileZ)), dim3(kGmBlock),
                       0, s, a);
    return launch_status("groundColumns");
}

int emf_hip_groundCells(const uint64_t* occ_dev, const uint64_t* fre_dev, const int32_t map[2], int32_t bins,
                        int32_t robot_bins, emf_ground_cell_t* cells_dev, emf_stream_t stream) {
    if (!occ_dev || !fre_dev || !cells_dev) return fail(EMF_E_ARG, "groundCells: a NULL pointer");
    EMF_TRY(check_map("groundCells", map));
    EMF_TRY(check_bins("groundCells", bins));
    if (robot_bins < 1) return fail(EMF_E_ARG, "groundCells: a robot of %d bins", robot_bins);
    if ((reinterpret_cast<uintptr_t>(occ_dev) | reinterpret_cast<uintptr_t>(fre_dev)) & 7u)
        return fail(EMF_E_ARG, "groundCells: a misaligned plane");
    if (reinterpret_cast<uintptr_t>(cells_dev) & 1u) return fail(EMF_E_ARG, "groundCells: misaligned records");
    const int n = map[0] * map[1];
    hipLaunchKernelGGL(k_ground_cells, dim3(ceil_div(n, 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const unsigned long long*>(occ_dev), reinterpret_cast<const unsigned long long*>(fre_dev), n,
                       bins, (bins + 63) / 64, robot_bins, cells_dev);
    return launch_status("groundCells");
}

int emf_hip_groundClasses(const emf_ground_cell_t* cells_dev, const int32_t map[2], int32_t max_step,
                          uint8_t* classes2d_dev, emf_stream_t stream) {
    if (!cells_dev || !classes2d_dev) return fail(EMF_E_ARG, "groundClasses: a NULL pointer");
    EMF_TRY(check_map("groundClasses", map));
    if (max_step < 0) return fail(EMF_E_ARG, "groundClasses: a step of %d bins", max_step);
    if (reinterpret_cast<uintptr_t>(cells_dev) & 1u) return fail(EMF_E_ARG, "groundClasses: misaligned records");
    hipLaunchKernelGGL(k_ground_classes, dim3(ceil_div(static_cast<size_t>(map[0]) * map[1], 256)), dim3(256), 0,
                       as_stream(stream), cells_dev, map[0], map[1], max_step, classes2d_dev);
    return launch_status("groundClasses");
}

}  // extern "C"
