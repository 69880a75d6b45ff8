// resample.hpp -- what the passes that carry one dense volume through a rigid pose onto another lattice share
// (include/emf_hip.h "Absorbing a volume" and "Lifting a volume"; absorb.hip and lift.hip): the tile walk, the sample
// point, the pad-1 outside rule, the corner gathers, the blend and the nearest voxel on the device; the argument checks
// and the tile grid on the host.  Every float step is one float32 operation: the _rn intrinsics, and every product that
// feeds a sum goes through mul_rounded / lerp_rounded of wave_ops.hpp, so that a build with -ffp-contract=fast has no
// product left to fuse.
#pragma once

#include <cmath>

#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {

constexpr int kRsBlock = 256;
constexpr int kRsTileX = 32, kRsTileY = 8, kRsTileZ = 8;  // the tile of emf_model_t.unseenTiles

// ---- device --------------------------------------------------------------------------------------------------------

// One workgroup per tile of the box, 256 lanes = 32 along x, 8 rows (the layout of k_ct_probe): a lane's column and the
// z planes [z0, z1) of its tile that lie in the box.
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

// q_i = (((R_i0 * p_d_0 + R_i1 * p_d_1) + R_i2 * p_d_2) + t_i) / voxelSize_s + half_s_i
__device__ __forceinline__ V3 rs_sample(const RsRows& rows, const float* R, const float* t, float pdz, float voxS, const V3& halfS) {
    const float psx = __fadd_rn(__fadd_rn(rows.r0, mul_rounded(R[2], pdz)), t[0]);
    const float psy = __fadd_rn(__fadd_rn(rows.r1, mul_rounded(R[5], pdz)), t[1]);
    const float psz = __fadd_rn(__fadd_rn(rows.r2, mul_rounded(R[8], pdz)), t[2]);
    return V3{__fadd_rn(__fdiv_rn(psx, voxS), halfS.x), __fadd_rn(__fdiv_rn(psy, voxS), halfS.y), __fadd_rn(__fdiv_rn(psz, voxS), halfS.z)};
}

// the pad-1 rule of outside(), a NaN first: all eight corners of an inside cell lie in the volume of fn voxels
__device__ __forceinline__ bool rs_outside(const V3& q, float fnx, float fny, float fnz) {
    return !(q.x == q.x) || !(q.y == q.y) || !(q.z == q.z) || q.x < 0.f || __fadd_rn(q.x, 1.f) >= fnx || q.y < 0.f ||
           __fadd_rn(q.y, 1.f) >= fny || q.z < 0.f || __fadd_rn(q.z, 1.f) >= fnz;
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

}  // namespace emf_hip
