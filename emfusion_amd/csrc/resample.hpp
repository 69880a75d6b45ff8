// resample.hpp -- the one resampler of the passes that carry a dense volume through a rigid pose onto another lattice
// (include/emf_hip.h "Object contacts", "Absorbing a volume" and "Lifting a volume"; contacts.hip and
// volume_transfer.hip).  On the device: the tile walk, the sample point, what the source holds there (rs_source: the
// pad-1 outside rule, the unseen-tile byte, the corner gathers, the blend, the mask byte at the nearest voxel), and the
// record epilogue (RsBounds, rs_add64, rs_init_record), and for the passes that carry colour with the band the colour
// entry as one 8-byte word and its exact integer blend (rs_color_*).  On the host: the argument checks, the kernel
// arguments and the launch of a pass over a box of the destination.  Every float step is one float32 operation: the _rn intrinsics, and
// every product that feeds a sum goes through mul_rounded / lerp_rounded of wave_ops.hpp, so that a build with
// -ffp-contract=fast has no product left to fuse.
#pragma once

#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {

constexpr int kRsBlock = 256;
constexpr int kRsTileX = 32, kRsTileY = 8, kRsTileZ = 8;  // the tile of emf_model_t.unseenTiles

// What a pass over a box of the destination is handed.  The source is only read; a pass that reads one byte volume of
// the other party alone (k_lf_release: the claimant's mask) leaves srcTsdf, srcWeights and srcUnseen NULL.
template <typename Record>
struct ResampleArgs {
    float* dstTsdf;
    float* dstWeights;
    const float* srcTsdf;
    const float* srcWeights;
    const uint8_t* srcMask;    // or NULL
    const uint8_t* srcUnseen;  // or NULL
    Record* record;
    I3 nd, ns;                 // resolutions
    I3 lo, hi;                 // the box [lo, hi) of the destination
    I3 t0;                     // the first tile of the box, in tiles
    unsigned ntx, nty;         // tiles of the box along x and y
    float voxD, voxS, ratio, maxWeight;
    float R[9], t[3];          // source frame <- destination frame
};

// What the colour variant of a pass is handed on top: the destination's colour volume (uint16_t[4] per voxel, an entry
// = one 8-byte word), the source's (or NULL: every source entry is (0, 0, 0, 0); a release has none), the colour
// record and the weight cap in 8.8 fixed point.  The plain kernels keep ResampleArgs: their arguments do not change.
template <typename Record>
struct ResampleColorArgs : ResampleArgs<Record> {
    uint2* dstColor;
    const uint2* srcColor;
    emf_color_moved_t* colorRecord;
    unsigned capq;
};

// ---- device --------------------------------------------------------------------------------------------------------

// One workgroup per tile of the box, 256 lanes = 32 along x, 8 rows: a lane's column and the z planes [z0, z1) of its
// tile that lie in the box.
struct RsLane {
    int x, y, z0, z1;
    bool mine;  // the column lies in the box
};

__device__ __forceinline__ RsLane rs_lane(const I3& t0, unsigned ntx, unsigned nty, const I3& lo, const I3& hi) {
    const unsigned b = blockIdx.x;
    const unsigned tz = b / (ntx * nty), r = b - tz * ntx * nty, ty = r / ntx, tx = r - ty * ntx;
    RsLane l;
    l.x = (t0.x + static_cast<int>(tx)) * kRsTileX + static_cast<int>(threadIdx.x & 31u);
    l.y = (t0.y + static_cast<int>(ty)) * kRsTileY + static_cast<int>(threadIdx.x >> 5);
    const int zt = (t0.z + static_cast<int>(tz)) * kRsTileZ;
    l.z0 = max(zt, lo.z), l.z1 = min(zt + kRsTileZ, hi.z);
    l.mine = l.x >= lo.x && l.x < hi.x && l.y >= lo.y && l.y < hi.y;
    return l;
}

// p_d_j = (float(v_j) - half_d_j) * voxelSize_d
__device__ __forceinline__ float rs_pd(int v, int n, float vox) {
    return __fmul_rn(__fsub_rn(static_cast<float>(v), static_cast<float>(n - 1) / 2.f), vox);
}

// the first two products of every pose row, summed left to right: what a column keeps over its z planes
struct RsRows {
    float r0, r1, r2;
};

__device__ __forceinline__ RsRows rs_rows(const float* R, float pdx, float pdy) {
    return RsRows{__fadd_rn(mul_rounded(R[0], pdx), mul_rounded(R[1], pdy)), __fadd_rn(mul_rounded(R[3], pdx), mul_rounded(R[4], pdy)),
                  __fadd_rn(mul_rounded(R[6], pdx), mul_rounded(R[7], pdy))};
}

// A volume as its sampler sees it: the arrays (mask and unseen-tile map or NULL), the resolution and what follows from it.
struct RsVolume {
    const float* tsdf;
    const float* weights;
    const uint8_t* mask;
    const uint8_t* unseen;
    I3 n;
    size_t by, bz;       // strides of y and z
    unsigned stx, sty;   // tiles of the unseen-tile map along x and y
    V3 half, fn;
};

__device__ __forceinline__ RsVolume rs_volume(const float* tsdf, const float* weights, const uint8_t* mask, const uint8_t* unseen,
                                              const I3& n) {
    const size_t by = static_cast<size_t>(n.x);
    return RsVolume{tsdf, weights, mask, unseen, n, by, by * n.y, static_cast<unsigned>(n.x + kRsTileX - 1) / kRsTileX,
                    static_cast<unsigned>(n.y + kRsTileY - 1) / kRsTileY, half_extent(n),
                    V3{static_cast<float>(n.x), static_cast<float>(n.y), static_cast<float>(n.z)}};
}

// q_i = (((R_i0 * p_d_0 + R_i1 * p_d_1) + R_i2 * p_d_2) + t_i) / voxelSize_s + half_s_i
__device__ __forceinline__ V3 rs_sample(const RsRows& rows, const float* R, const float* t, float pdz, float voxS, const V3& halfS) {
    const float psx = __fadd_rn(__fadd_rn(rows.r0, mul_rounded(R[2], pdz)), t[0]);
    const float psy = __fadd_rn(__fadd_rn(rows.r1, mul_rounded(R[5], pdz)), t[1]);
    const float psz = __fadd_rn(__fadd_rn(rows.r2, mul_rounded(R[8], pdz)), t[2]);
    return V3{__fadd_rn(__fdiv_rn(psx, voxS), halfS.x), __fadd_rn(__fdiv_rn(psy, voxS), halfS.y), __fadd_rn(__fdiv_rn(psz, voxS), halfS.z)};
}

// the pad-1 rule of outside(), a NaN first: all eight corners of an inside cell lie in the volume of fn voxels
__device__ __forceinline__ bool rs_outside(const V3& q, const V3& fn) {
    return !(q.x == q.x) || !(q.y == q.y) || !(q.z == q.z) || q.x < 0.f || __fadd_rn(q.x, 1.f) >= fn.x || q.y < 0.f ||
           __fadd_rn(q.y, 1.f) >= fn.y || q.z < 0.f || __fadd_rn(q.z, 1.f) >= fn.z;
}

// the eight corners of the cell at c, x fastest: 8 independent loads
__device__ __forceinline__ void rs_gather(const float* __restrict__ p, size_t c, size_t by, size_t bz, float (&o)[8]) {
    o[0] = p[c], o[1] = p[c + 1], o[2] = p[c + by], o[3] = p[c + by + 1];
    o[4] = p[c + bz], o[5] = p[c + bz + 1], o[6] = p[c + bz + by], o[7] = p[c + bz + by + 1];
}

__device__ __forceinline__ bool rs_all_seen(const float (&w)[8]) {
    return w[0] > 0.f && w[1] > 0.f && w[2] > 0.f && w[3] > 0.f && w[4] > 0.f && w[5] > 0.f && w[6] > 0.f && w[7] > 0.f;
}

// all eight are > 0, none is NaN: the minimum does not depend on the order
__device__ __forceinline__ float rs_min8(const float (&w)[8]) {
    return fminf(fminf(fminf(w[0], w[1]), fminf(w[2], w[3])), fminf(fminf(w[4], w[5]), fminf(w[6], w[7])));
}

// blend8 of common.hpp, its products made opaque: x pairs, then y, then z
__device__ __forceinline__ float rs_blend(float fx, float fy, float fz, const float (&t)[8]) {
    const float gx = __fsub_rn(1.f, fx), gy = __fsub_rn(1.f, fy), gz = __fsub_rn(1.f, fz);
    const float a0 = lerp_rounded(gx, fx, t[0], t[1]), a1 = lerp_rounded(gx, fx, t[2], t[3]), a2 = lerp_rounded(gx, fx, t[4], t[5]),
                a3 = lerp_rounded(gx, fx, t[6], t[7]);
    const float b0 = lerp_rounded(gy, fy, a0, a1), b1 = lerp_rounded(gy, fy, a2, a3);
    return lerp_rounded(gz, fz, b0, b1);
}

// the voxel nearest to q, ties to even: inside the volume by the outside rule
__device__ __forceinline__ size_t rs_nearest(const V3& q, int ny, size_t by) {
    const int rx = __float2int_rn(q.x), ry = __float2int_rn(q.y), rz = __float2int_rn(q.z);
    return (static_cast<size_t>(rz) * ny + ry) * by + rx;
}

// corner 0 of q's cell in a tile whose every weight is 0, by the unseen-tile map if there is one: its weight is not > 0,
// the cell is UNKNOWN unread
__device__ __forceinline__ bool rs_unseen(const RsVolume& v, const V3& q) {
    const unsigned lx = static_cast<unsigned>(static_cast<int>(q.x)), ly = static_cast<unsigned>(static_cast<int>(q.y)),
                   lz = static_cast<unsigned>(static_cast<int>(q.z));
    return v.unseen != nullptr && v.unseen[(lz / kRsTileZ * v.sty + ly / kRsTileY) * v.stx + lx / kRsTileX] != 0;
}

// the cell of an inside q: the gathers of w, then of t, the blend s; false where a corner is unseen or s is NaN
__device__ __forceinline__ bool rs_cell(const RsVolume& v, const V3& q, float& s, float (&w)[8]) {
    const int lx = static_cast<int>(q.x), ly = static_cast<int>(q.y), lz = static_cast<int>(q.z);
    const size_t c = (static_cast<size_t>(lz) * v.n.y + ly) * v.by + lx;
    float t[8];
    rs_gather(v.weights, c, v.by, v.bz, w);
    rs_gather(v.tsdf, c, v.by, v.bz, t);
    s = rs_blend(__fsub_rn(q.x, static_cast<float>(lx)), __fsub_rn(q.y, static_cast<float>(ly)), __fsub_rn(q.z, static_cast<float>(lz)), t);
    return rs_all_seen(w) && s == s;
}

// the mask byte, if there is a mask, at the voxel nearest to an inside q is 0
__device__ __forceinline__ bool rs_masked(const RsVolume& v, const V3& q) {
    return v.mask != nullptr && v.mask[rs_nearest(q, v.n.y, v.by)] == 0;
}

// What the source holds at q, in the one fixed order: the outside rule; the unseen-tile byte; the cell; the mask byte.
// A VALUE comes with the blended s and the eight corner weights w.
enum class RsClass { Outside, Unknown, Masked, Value };

__device__ __forceinline__ RsClass rs_source(const RsVolume& v, const V3& q, float& s, float (&w)[8]) {
    if (rs_outside(q, v.fn)) return RsClass::Outside;
    if (rs_unseen(v, q) || !rs_cell(v, q, s, w)) return RsClass::Unknown;
    return rs_masked(v, q) ? RsClass::Masked : RsClass::Value;
}

// The record epilogue.  The bounds of the voxels a lane kept, neutral at (n, -1); a wave reduces them only where any()
// says that some lane kept one, and lane 0 alone commits them: six integer atomics.
struct RsBounds {
    int lox, loy, loz, hix, hiy, hiz;

    __device__ __forceinline__ explicit RsBounds(const I3& n) : lox(n.x), loy(n.y), loz(n.z), hix(-1), hiy(-1), hiz(-1) {}
    __device__ __forceinline__ void include(int x, int y, int z) {
        lox = min(lox, x), hix = max(hix, x);
        loy = min(loy, y), hiy = max(hiy, y);
        loz = min(loz, z), hiz = max(hiz, z);
    }
    __device__ __forceinline__ bool any() const { return __ballot(hix >= 0) != 0ull; }  // wave-uniform
    __device__ __forceinline__ void reduce() {
        lox = wave_reduce<OpMin>(lox), loy = wave_reduce<OpMin>(loy), loz = wave_reduce<OpMin>(loz);
        hix = wave_reduce<OpMax>(hix), hiy = wave_reduce<OpMax>(hiy), hiz = wave_reduce<OpMax>(hiz);
    }
    template <typename Record>
    __device__ __forceinline__ void commit(Record* out) const {
        atomicMin(&out->lo[0], lox), atomicMin(&out->lo[1], loy), atomicMin(&out->lo[2], loz);
        atomicMax(&out->hi[0], hix), atomicMax(&out->hi[1], hiy), atomicMax(&out->hi[2], hiz);
    }
};

// ---- colour entries (include/emf_hip.h "Per-voxel colour"): R | G << 16 in .x, B | Wc << 16 in .y, all integer ----

__device__ __forceinline__ unsigned rs_color_weight(const uint2& e) { return e.y >> 16; }

// the source entry at the voxel nearest to an inside q (the addressing of MASKED); without a source colour volume (0, 0, 0, 0)
__device__ __forceinline__ uint2 rs_color_source(const uint2* __restrict__ color, const V3& q, int ny, size_t by) {
    return color != nullptr ? color[rs_nearest(q, ny, by)] : make_uint2(0u, 0u);
}

// (de * dc + sw * sc + (de + sw) / 2) / (de + sw), floor, exact for every u16 input with de + sw > 0.  The two products
// fit 32 bits each, their sum does not: each is divided on its own and the remainders, below den each, are divided with
// the half -- three 32-bit divisions by one divisor instead of one 64-bit division.
__device__ __forceinline__ unsigned rs_color_blend(unsigned de, unsigned dc, unsigned sw, unsigned sc, unsigned den) {
    const unsigned a = de * dc, b = sw * sc;
    return a / den + b / den + (a % den + b % den + den / 2u) / den;
}

// D blended with the COLOURED source entry S under the destination weight de (0 for a FRESH voxel): a copy of Sc then
__device__ __forceinline__ uint2 rs_color_fuse(const uint2& D, const uint2& S, unsigned de, unsigned capq) {
    const unsigned sw = rs_color_weight(S), den = de + sw;
    const unsigned r = rs_color_blend(de, D.x & 0xffffu, sw, S.x & 0xffffu, den);
    const unsigned g = rs_color_blend(de, D.x >> 16, sw, S.x >> 16, den);
    const unsigned b = rs_color_blend(de, D.y & 0xffffu, sw, S.y & 0xffffu, den);
    return make_uint2(r | g << 16, b | min(den, capq) << 16);
}

// a count of the record: an atomic only where there is something to add
__device__ __forceinline__ void rs_add64(uint64_t* q, unsigned long long v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(q), v);
}

// the neutral record: no count, the bounds at (n, -1)
template <typename Record>
__device__ __forceinline__ Record rs_neutral(const I3& nd) {
    Record r{};
    r.lo[0] = nd.x, r.lo[1] = nd.y, r.lo[2] = nd.z;
    r.hi[0] = r.hi[1] = r.hi[2] = -1;
    return r;
}

// one lane: the neutral record before a pass
template <typename Record>
__global__ void rs_init_record(Record* record, I3 nd) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    *record = rs_neutral<Record>(nd);
}

// one lane: both neutral records before a colour pass
template <typename Record>
__global__ void rs_init_records(Record* record, I3 nd, emf_color_moved_t* colorRecord) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    *record = rs_neutral<Record>(nd);
    *colorRecord = emf_color_moved_t{0u, 0u};
}

// ---- host ----------------------------------------------------------------------------------------------------------

inline bool rs_positive_finite(float v) { return v > 0.f && std::isfinite(v); }

// [p, p + bytes) and [q, q + qbytes) share a byte
inline bool rs_overlap(const void* p, size_t bytes, const void* q, size_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qbytes && b < a + bytes;
}

inline int rs_check_volume(const char* who, const int32_t* res, const char* which, unsigned long long* voxels) {
    for (int i = 0; i < 3; ++i) {
        if (res[i] < 1) return fail(EMF_E_ARG, "%s: the %s has %d voxels on axis %d", who, which, res[i], i);
        if (res[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "%s: the %s has %d voxels on axis %d, above %d", who, which, res[i], i, EMF_DF_MAX_AXIS);
    }
    *voxels = static_cast<unsigned long long>(res[0]) * res[1] * static_cast<unsigned long long>(res[2]);
    if (*voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "%s: the %s has %llu voxels, above 2^31 - 1", who, which, *voxels);
    return EMF_OK;
}

inline int rs_check_box(const char* who, const int32_t* box_lo, const int32_t* box_size, const int32_t* dst_res, bool* empty) {
    *empty = false;
    for (int i = 0; i < 3; ++i) {
        if (box_lo[i] < 0 || box_size[i] < 0 || box_lo[i] > dst_res[i] || box_size[i] > dst_res[i] - box_lo[i])
            return fail(EMF_E_ARG, "%s: the box [%d, %d + %d) leaves the destination's %d voxels on axis %d", who, box_lo[i], box_lo[i],
                        box_size[i], dst_res[i], i);
        *empty |= box_size[i] == 0;
    }
    return EMF_OK;
}

// The tiles of a non-empty box: [lo, hi), the first tile and the tiles along x and y; returns the number of tiles, at
// most 64 * 256 * 256 = 2^22 in a volume of EMF_DF_MAX_AXIS per axis.
inline unsigned rs_tiles(const int32_t* box_lo, const int32_t* box_size, I3* lo, I3* hi, I3* t0, unsigned* ntx, unsigned* nty) {
    *lo = I3{box_lo[0], box_lo[1], box_lo[2]};
    *hi = I3{box_lo[0] + box_size[0], box_lo[1] + box_size[1], box_lo[2] + box_size[2]};
    *t0 = I3{lo->x / kRsTileX, lo->y / kRsTileY, lo->z / kRsTileZ};
    *ntx = static_cast<unsigned>((hi->x - 1) / kRsTileX - t0->x + 1);
    *nty = static_cast<unsigned>((hi->y - 1) / kRsTileY - t0->y + 1);
    const unsigned ntz = static_cast<unsigned>((hi->z - 1) / kRsTileZ - t0->z + 1);
    return *ntx * *nty * ntz;
}

// The first checks of a pass, before any resolution is read: the destination, the pose, the box and the record are there
// and aligned.
inline int rs_check_destination(const char* who, const float* dst_tsdf, const float* dst_weights, const int32_t* dst_res, const float* R,
                                const float* t, const int32_t* box_lo, const int32_t* box_size, const void* record_dev) {
    if (!dst_tsdf || !dst_weights || !dst_res) return fail(EMF_E_ARG, "%s: the destination or its resolution is NULL", who);
    if (!R || !t || !box_lo || !box_size || !record_dev) return fail(EMF_E_ARG, "%s: the pose, the box or the record is NULL", who);
    if ((reinterpret_cast<uintptr_t>(dst_tsdf) | reinterpret_cast<uintptr_t>(dst_weights)) & 3u)
        return fail(EMF_E_ARG, "%s: a misaligned volume", who);
    if (reinterpret_cast<uintptr_t>(record_dev) & 7u) return fail(EMF_E_ARG, "%s: a misaligned record", who);
    return EMF_OK;
}

// The checks of a pass once both resolutions hold: the voxel sizes; the destination's two arrays, the record and the
// other party's arrays (others[k] of otherBytes[k] bytes, or NULL) share no byte but among the others; the box.  Fills
// the destination, the box, the pose and the record of the arguments; *tiles is 0 for an empty box.
template <typename Record>
inline int rs_check_layout(const char* who, ResampleArgs<Record>* a, unsigned* tiles, float* dst_tsdf, float* dst_weights,
                           const int32_t* dst_res, unsigned long long dst_voxels, float dst_voxel_size, const char* other,
                           const int32_t* other_res, float other_voxel_size, const void* const* others, const size_t* otherBytes,
                           int nOthers, const float* R, const float* t, const int32_t* box_lo, const int32_t* box_size,
                           Record* record_dev) {
    if (!rs_positive_finite(dst_voxel_size) || !rs_positive_finite(other_voxel_size))
        return fail(EMF_E_ARG, "%s: voxel sizes %g and %g", who, static_cast<double>(dst_voxel_size), static_cast<double>(other_voxel_size));
    const size_t dBytes = static_cast<size_t>(dst_voxels) * sizeof(float);
    if (rs_overlap(dst_tsdf, dBytes, dst_weights, dBytes)) return fail(EMF_E_ARG, "%s: the destination's tsdf and weights overlap", who);
    for (int k = 0; k < nOthers; ++k) {
        if (others[k] == nullptr) continue;
        if (rs_overlap(dst_tsdf, dBytes, others[k], otherBytes[k]) || rs_overlap(dst_weights, dBytes, others[k], otherBytes[k]))
            return fail(EMF_E_ARG, "%s: the destination overlaps the %s", who, other);
        if (rs_overlap(record_dev, sizeof(Record), others[k], otherBytes[k])) return fail(EMF_E_ARG, "%s: the record overlaps the %s", who, other);
    }
    if (rs_overlap(record_dev, sizeof(Record), dst_tsdf, dBytes) || rs_overlap(record_dev, sizeof(Record), dst_weights, dBytes))
        return fail(EMF_E_ARG, "%s: the record overlaps the destination", who);
    bool empty = false;
    EMF_TRY(rs_check_box(who, box_lo, box_size, dst_res, &empty));
    a->dstTsdf = dst_tsdf, a->dstWeights = dst_weights, a->record = record_dev;
    a->nd = I3{dst_res[0], dst_res[1], dst_res[2]};
    a->ns = I3{other_res[0], other_res[1], other_res[2]};
    *tiles = empty ? 0u : rs_tiles(box_lo, box_size, &a->lo, &a->hi, &a->t0, &a->ntx, &a->nty);
    a->voxD = dst_voxel_size, a->voxS = other_voxel_size;
    for (int i = 0; i < 9; ++i) a->R[i] = R[i];
    for (int i = 0; i < 3; ++i) a->t[i] = t[i];
    return EMF_OK;
}

// Every check of a pass that resamples a whole source (tsdf, weights, optional mask and unseen-tile map) into a
// destination with a band of its own, and the arguments of its kernel.
template <typename Record>
inline int rs_check_transfer(const char* who, ResampleArgs<Record>* a, unsigned* tiles, float* dst_tsdf, float* dst_weights,
                             const int32_t* dst_res, float dst_voxel_size, float dst_truncdist, float max_weight,
                             const emf_absorb_source_t* source, const float* R, const float* t, const int32_t* box_lo,
                             const int32_t* box_size, Record* record_dev) {
    if (!source || !source->tsdf || !source->weights) return fail(EMF_E_ARG, "%s: the source or one of its volumes is NULL", who);
    EMF_TRY(rs_check_destination(who, dst_tsdf, dst_weights, dst_res, R, t, box_lo, box_size, record_dev));
    if ((reinterpret_cast<uintptr_t>(source->tsdf) | reinterpret_cast<uintptr_t>(source->weights)) & 3u)
        return fail(EMF_E_ARG, "%s: a misaligned volume", who);
    unsigned long long nDst = 0, nSrc = 0;
    EMF_TRY(rs_check_volume(who, dst_res, "destination", &nDst));
    EMF_TRY(rs_check_volume(who, source->res, "source", &nSrc));
    if (!rs_positive_finite(dst_truncdist) || !rs_positive_finite(source->truncdist))
        return fail(EMF_E_ARG, "%s: truncation distances %g and %g", who, static_cast<double>(dst_truncdist),
                    static_cast<double>(source->truncdist));
    if (!rs_positive_finite(max_weight)) return fail(EMF_E_ARG, "%s: maxWeight %g", who, static_cast<double>(max_weight));
    const float ratio = source->truncdist / dst_truncdist;  // one float32 division
    if (!rs_positive_finite(ratio))
        return fail(EMF_E_ARG, "%s: the ratio of the truncation distances %g / %g is no positive finite float", who,
                    static_cast<double>(source->truncdist), static_cast<double>(dst_truncdist));
    // the arrays: two of the destination, up to four of the source; the destination's share no byte with any other
    const size_t sBytes = static_cast<size_t>(nSrc) * sizeof(float);
    const void* others[4] = {source->tsdf, source->weights, source->fgVolMask, source->unseenTiles};
    const size_t otherBytes[4] = {sBytes, sBytes, static_cast<size_t>(nSrc), emf_hip_unseenTileBytes(source->res)};
    EMF_TRY(rs_check_layout(who, a, tiles, dst_tsdf, dst_weights, dst_res, nDst, dst_voxel_size, "source", source->res, source->voxelSize,
                            others, otherBytes, 4, R, t, box_lo, box_size, record_dev));
    a->srcTsdf = source->tsdf, a->srcWeights = source->weights, a->srcMask = source->fgVolMask, a->srcUnseen = source->unseenTiles;
    a->ratio = ratio, a->maxWeight = max_weight;
    return EMF_OK;
}

// The weight cap of a colour pass in 8.8 fixed point, from the destination's maxWeight (finite and > 0).
inline unsigned rs_color_cap(float max_weight) {
    if (max_weight * 256.f >= 65535.f) return 65535u;
    return static_cast<unsigned>(std::max(std::lrintf(max_weight * 256.f), 1l));
}

// The checks a colour pass adds once its sibling's have passed and `a` holds the resolutions: the destination's colour
// volume and the colour record are there, 8-byte aligned (the source's colour volume too, where there is one) and share
// no byte with each other or with any other array of the call.  others / otherBytes: the other party's arrays as the
// sibling's check saw them (NULL entries skipped).  Fills the colour part of the arguments but the cap.
template <typename Record>
inline int rs_check_color(const char* who, ResampleColorArgs<Record>* a, uint16_t* dst_color, const uint16_t* src_color,
                          emf_color_moved_t* color_record_dev, const void* const* others, const size_t* otherBytes, int nOthers) {
    if (!dst_color) return fail(EMF_E_ARG, "%s: the destination's colour volume is NULL (the plain entry takes none)", who);
    if (!color_record_dev) return fail(EMF_E_ARG, "%s: the colour record is NULL", who);
    if ((reinterpret_cast<uintptr_t>(dst_color) | reinterpret_cast<uintptr_t>(src_color) | reinterpret_cast<uintptr_t>(color_record_dev)) & 7u)
        return fail(EMF_E_ARG, "%s: a misaligned colour volume or colour record", who);
    const size_t nDst = static_cast<size_t>(a->nd.x) * a->nd.y * a->nd.z, nSrc = static_cast<size_t>(a->ns.x) * a->ns.y * a->ns.z;
    // everything else the call names: the destination's two arrays, the record, the other party's arrays, its colour
    const void* all[12] = {a->dstTsdf, a->dstWeights, a->record, src_color};
    size_t allBytes[12] = {nDst * sizeof(float), nDst * sizeof(float), sizeof(Record), nSrc * 8u};
    int n = 4;
    for (int k = 0; k < nOthers && n < 12; ++k) all[n] = others[k], allBytes[n++] = otherBytes[k];
    for (int k = 0; k < n; ++k) {
        if (all[k] == nullptr) continue;
        if (rs_overlap(dst_color, nDst * 8u, all[k], allBytes[k]))
            return fail(EMF_E_ARG, "%s: the destination's colour volume overlaps another array of the call", who);
        if (rs_overlap(color_record_dev, sizeof(emf_color_moved_t), all[k], allBytes[k]))
            return fail(EMF_E_ARG, "%s: the colour record overlaps another array of the call", who);
    }
    if (rs_overlap(color_record_dev, sizeof(emf_color_moved_t), dst_color, nDst * 8u))
        return fail(EMF_E_ARG, "%s: the colour record overlaps the destination's colour volume", who);
    a->dstColor = reinterpret_cast<uint2*>(dst_color), a->srcColor = reinterpret_cast<const uint2*>(src_color);
    a->colorRecord = color_record_dev, a->capq = 0u;
    return EMF_OK;
}

// The neutral record, then -- unless the box is empty -- the pass, one workgroup per tile.  Everything that refuses a
// call has happened before.
template <typename Record>
inline int rs_launch(const char* who, void (*pass)(ResampleArgs<Record>), const ResampleArgs<Record>& a, unsigned tiles, emf_stream_t stream) {
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(rs_init_record<Record>, dim3(1), dim3(64), 0, s, a.record, a.nd);
    if (tiles != 0u) hipLaunchKernelGGL(pass, dim3(tiles), dim3(kRsBlock), 0, s, a);
    return launch_status(who);
}

// The same for a colour pass: both neutral records in the one init launch.
template <typename Record>
inline int rs_launch(const char* who, void (*pass)(ResampleColorArgs<Record>), const ResampleColorArgs<Record>& a, unsigned tiles,
                     emf_stream_t stream) {
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(rs_init_records<Record>, dim3(1), dim3(64), 0, s, a.record, a.nd, a.colorRecord);
    if (tiles != 0u) hipLaunchKernelGGL(pass, dim3(tiles), dim3(kRsBlock), 0, s, a);
    return launch_status(who);
}

}  // namespace emf_hip
