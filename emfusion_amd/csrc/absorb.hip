// absorb.hip -- absorbing a volume: the signed-distance band of a SOURCE volume, resampled through a rigid pose into a
// DESTINATION volume and fused there by the destination's running average (include/emf_hip.h "Absorbing a volume",
// DESIGN.md 5.29).
//   k_ab_absorb  one workgroup per 32 x 8 x 8 tile of the DESTINATION that meets the box, 256 lanes = 32 along x, 8 rows
//                (the layout of k_ct_probe); a lane walks the tile's z planes.  The x and y parts of the three pose rows
//                are hoisted out of the z loop.  A wave whose lanes all lie outside the box leaves.  Per voxel: the
//                sample point in the source, the outside rule, 8 + 8 dependent gathers, the mask byte, the band rule,
//                the fusion; a destination voxel reads and writes only itself, so the pass is in place.  Only the words
//                whose bits change are stored.  Per wave: wave_reduce of what is not zero anywhere in the wave, then
//                one integer atomic per non-zero quantity from lane 0.  No LDS, no barrier.
//   k_ab_init    one lane: the neutral record before the pass.
// Every float step is one float32 operation: the _rn intrinsics, and every product that feeds a sum goes through an
// identity DPP move (mul_rounded of wave_ops.hpp, as in contacts.hip), so that a build with -ffp-contract=fast has no
// product left to fuse.  Integer atomics only: the record does not depend on the order of lanes, waves or workgroups.
#include <cmath>

#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {
namespace {

constexpr int kAbBlock = 256;
constexpr int kAbTileX = 32, kAbTileY = 8, kAbTileZ = 8;  // the tile of emf_model_t.unseenTiles

static_assert(sizeof(emf_absorb_t) == 88 && sizeof(emf_absorb_source_t) == 56, "mirrored by emfusion_amd/_lib.py");

struct AbsorbArgs {
    float* dstTsdf;
    float* dstWeights;
    const float* srcTsdf;
    const float* srcWeights;
    const uint8_t* srcMask;    // or NULL
    const uint8_t* srcUnseen;  // or NULL
    emf_absorb_t* record;
    I3 nd, ns;                 // resolutions
    I3 lo, hi;                 // the box [lo, hi) of the destination
    I3 t0;                     // the first tile of the box, in tiles
    unsigned ntx, nty;         // tiles of the box along x and y
    float voxD, voxS, ratio, maxWeight;
    float R[9], t[3];          // source frame <- destination frame
};

__global__ __launch_bounds__(kAbBlock) void k_ab_absorb(const AbsorbArgs a) {
    const unsigned b = blockIdx.x;
    const unsigned tz = b / (a.ntx * a.nty), r = b - tz * a.ntx * a.nty, ty = r / a.ntx, tx = r - ty * a.ntx;
    const int x = (a.t0.x + static_cast<int>(tx)) * kAbTileX + static_cast<int>(threadIdx.x & 31u);
    const int y = (a.t0.y + static_cast<int>(ty)) * kAbTileY + static_cast<int>(threadIdx.x >> 5);
    const int zt = (a.t0.z + static_cast<int>(tz)) * kAbTileZ;
    const int z0 = max(zt, a.lo.z), z1 = min(zt + kAbTileZ, a.hi.z);
    const bool mine = x >= a.lo.x && x < a.hi.x && y >= a.lo.y && y < a.hi.y;
    if (__ballot(mine) == 0ull) return;  // wave-uniform; the kernel has no barrier

    const I3 nd = a.nd, ns = a.ns;
    const size_t dy = static_cast<size_t>(nd.x), dz = dy * nd.y;
    const size_t by = static_cast<size_t>(ns.x), bz = by * ns.y;
    const float* __restrict__ tb = a.srcTsdf;
    const float* __restrict__ wb = a.srcWeights;
    const uint8_t* __restrict__ fb = a.srcMask;
    const uint8_t* __restrict__ ub = a.srcUnseen;
    const unsigned stx = static_cast<unsigned>(ns.x + kAbTileX - 1) / kAbTileX, sty = static_cast<unsigned>(ns.y + kAbTileY - 1) / kAbTileY;
    const V3 halfS = half_extent(ns);
    const float fnx = static_cast<float>(ns.x), fny = static_cast<float>(ns.y), fnz = static_cast<float>(ns.z);
    const float pdx = __fmul_rn(__fsub_rn(static_cast<float>(x), static_cast<float>(nd.x - 1) / 2.f), a.voxD);
    const float pdy = __fmul_rn(__fsub_rn(static_cast<float>(y), static_cast<float>(nd.y - 1) / 2.f), a.voxD);
    const float halfDz = static_cast<float>(nd.z - 1) / 2.f;
    // the first two products of every row, summed left to right
    const float r0 = __fadd_rn(mul_rounded(a.R[0], pdx), mul_rounded(a.R[1], pdy));
    const float r1 = __fadd_rn(mul_rounded(a.R[3], pdx), mul_rounded(a.R[4], pdy));
    const float r2 = __fadd_rn(mul_rounded(a.R[6], pdx), mul_rounded(a.R[7], pdy));

    unsigned cOut = 0u, cUnk = 0u, cMask = 0u, cSat = 0u, cFused = 0u, cFresh = 0u, cSolid = 0u;
    int lox = nd.x, loy = nd.y, loz = nd.z, hix = -1, hiy = -1, hiz = -1;

    if (mine) {
        for (int z = z0; z < z1; ++z) {
            const float pdz = __fmul_rn(__fsub_rn(static_cast<float>(z), halfDz), a.voxD);
            const float psx = __fadd_rn(__fadd_rn(r0, mul_rounded(a.R[2], pdz)), a.t[0]);
            const float psy = __fadd_rn(__fadd_rn(r1, mul_rounded(a.R[5], pdz)), a.t[1]);
            const float psz = __fadd_rn(__fadd_rn(r2, mul_rounded(a.R[8], pdz)), a.t[2]);
            const float qx = __fadd_rn(__fdiv_rn(psx, a.voxS), halfS.x);
            const float qy = __fadd_rn(__fdiv_rn(psy, a.voxS), halfS.y);
            const float qz = __fadd_rn(__fdiv_rn(psz, a.voxS), halfS.z);
            // the pad-1 rule of outside(), a NaN first: all eight corners of an inside cell lie in the source
            if (!(qx == qx) || !(qy == qy) || !(qz == qz) || qx < 0.f || __fadd_rn(qx, 1.f) >= fnx || qy < 0.f ||
                __fadd_rn(qy, 1.f) >= fny || qz < 0.f || __fadd_rn(qz, 1.f) >= fnz) {
                cOut += 1u;
                continue;
            }
            const int lx = static_cast<int>(qx), ly = static_cast<int>(qy), lz = static_cast<int>(qz);
            // corner 0 in a tile whose every weight is 0: its weight is not > 0, the cell is UNKNOWN unread
            if (ub != nullptr && ub[(static_cast<unsigned>(lz) / kAbTileZ * sty + static_cast<unsigned>(ly) / kAbTileY) * stx +
                                    static_cast<unsigned>(lx) / kAbTileX] != 0) {
                cUnk += 1u;
                continue;
            }
            const float fx = __fsub_rn(qx, static_cast<float>(lx)), fy = __fsub_rn(qy, static_cast<float>(ly)),
                        fz = __fsub_rn(qz, static_cast<float>(lz));
            const size_t c = (static_cast<size_t>(lz) * ns.y + ly) * by + lx;
            const float w0 = wb[c], w1 = wb[c + 1], w2 = wb[c + by], w3 = wb[c + by + 1], w4 = wb[c + bz], w5 = wb[c + bz + 1],
                        w6 = wb[c + bz + by], w7 = wb[c + bz + by + 1];
            const float t0 = tb[c], t1 = tb[c + 1], t2 = tb[c + by], t3 = tb[c + by + 1], t4 = tb[c + bz], t5 = tb[c + bz + 1],
                        t6 = tb[c + bz + by], t7 = tb[c + bz + by + 1];
            const bool seen = w0 > 0.f && w1 > 0.f && w2 > 0.f && w3 > 0.f && w4 > 0.f && w5 > 0.f && w6 > 0.f && w7 > 0.f;
            // blend8 of common.hpp, its products made opaque: x pairs, then y, then z
            const float gx = __fsub_rn(1.f, fx), gy = __fsub_rn(1.f, fy), gz = __fsub_rn(1.f, fz);
            const float a0 = lerp_rounded(gx, fx, t0, t1), a1 = lerp_rounded(gx, fx, t2, t3), a2 = lerp_rounded(gx, fx, t4, t5),
                        a3 = lerp_rounded(gx, fx, t6, t7);
            const float b0 = lerp_rounded(gy, fy, a0, a1), b1 = lerp_rounded(gy, fy, a2, a3);
            const float s = lerp_rounded(gz, fz, b0, b1);
            if (!seen || !(s == s)) {
                cUnk += 1u;
                continue;
            }
            if (fb != nullptr) {  // the voxel nearest to q, ties to even: inside the source by the rule above
                const int rx = __float2int_rn(qx), ry = __float2int_rn(qy), rz = __float2int_rn(qz);
                if (fb[(static_cast<size_t>(rz) * ns.y + ry) * by + rx] == 0) {
                    cMask += 1u;
                    continue;
                }
            }
            if (!(fabsf(s) < 1.f)) {  // "at least one source truncation away": no value the destination can fuse
                cSat += 1u;
                continue;
            }
            const float u = fminf(fmaxf(__fmul_rn(s, a.ratio), -1.f), 1.f);
            // all eight are > 0, none is NaN: the minimum does not depend on the order
            const float wo = fminf(fminf(fminf(w0, w1), fminf(w2, w3)), fminf(fminf(w4, w5), fminf(w6, w7)));
            const size_t v = static_cast<size_t>(z) * dz + static_cast<size_t>(y) * dy + x;
            const float pw = a.dstWeights[v], pt = a.dstTsdf[v];
            float nt, nw;
            if (!(pw > 0.f)) {  // a select: whatever an unseen voxel holds goes nowhere
                nt = u;
                nw = fminf(wo, a.maxWeight);
                cFresh += 1u;
            } else {
                nt = __fdiv_rn(__fadd_rn(mul_rounded(pw, pt), mul_rounded(wo, u)), __fadd_rn(pw, wo));
                nw = fminf(__fadd_rn(pw, wo), a.maxWeight);
            }
            cFused += 1u;
            if (!(nt > 0.f)) cSolid += 1u;
            lox = min(lox, x), hix = max(hix, x);
            loy = min(loy, y), hiy = max(hiy, y);
            loz = min(loz, z), hiz = max(hiz, z);
            if (__float_as_uint(nt) != __float_as_uint(pt)) a.dstTsdf[v] = nt;
            if (__float_as_uint(nw) != __float_as_uint(pw)) a.dstWeights[v] = nw;
        }
    }

    // a lane holds at most 8 voxels, a wave 512: every wave sum fits 32 bits
    const unsigned lane = threadIdx.x & 63u;
    cOut = wave_reduce<OpAdd>(cOut), cUnk = wave_reduce<OpAdd>(cUnk), cMask = wave_reduce<OpAdd>(cMask);
    cSat = wave_reduce<OpAdd>(cSat);
    const bool anyFused = __ballot(cFused != 0u) != 0ull;  // wave-uniform
    if (anyFused) {
        cFused = wave_reduce<OpAdd>(cFused), cFresh = wave_reduce<OpAdd>(cFresh), cSolid = wave_reduce<OpAdd>(cSolid);
        lox = wave_reduce<OpMin>(lox), loy = wave_reduce<OpMin>(loy), loz = wave_reduce<OpMin>(loz);
        hix = wave_reduce<OpMax>(hix), hiy = wave_reduce<OpMax>(hiy), hiz = wave_reduce<OpMax>(hiz);
    }
    if (lane == 0u) {
        emf_absorb_t* out = a.record;
        auto add = [](uint64_t* q, unsigned long long v) {
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(q), v);
        };
        add(&out->visited, static_cast<unsigned long long>(cOut) + cUnk + cMask + cSat + (anyFused ? cFused : 0u));
        add(&out->outside, cOut), add(&out->unknown, cUnk), add(&out->masked, cMask), add(&out->saturated, cSat);
        if (anyFused) {
            add(&out->fused, cFused), add(&out->fresh, cFresh), add(&out->solid, cSolid);
            atomicMin(&out->lo[0], lox), atomicMin(&out->lo[1], loy), atomicMin(&out->lo[2], loz);
            atomicMax(&out->hi[0], hix), atomicMax(&out->hi[1], hiy), atomicMax(&out->hi[2], hiz);
        }
    }
}

// one lane: the neutral record
__global__ void k_ab_init(emf_absorb_t* record, I3 nd) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    emf_absorb_t r{};
    r.lo[0] = nd.x, r.lo[1] = nd.y, r.lo[2] = nd.z;
    r.hi[0] = r.hi[1] = r.hi[2] = -1;
    *record = r;
}

bool positive_finite(float v) { return v > 0.f && std::isfinite(v); }

// [p, p + bytes) and [q, q + qbytes) share a byte
bool overlap(const void* p, size_t bytes, const void* q, size_t qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qbytes && b < a + bytes;
}

int check_volume(const int32_t* res, const char* which, unsigned long long* voxels) {
    for (int i = 0; i < 3; ++i) {
        if (res[i] < 1) return fail(EMF_E_ARG, "absorbVolume: the %s has %d voxels on axis %d", which, res[i], i);
        if (res[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "absorbVolume: the %s has %d voxels on axis %d, above %d", which, res[i], i, EMF_DF_MAX_AXIS);
    }
    *voxels = static_cast<unsigned long long>(res[0]) * res[1] * static_cast<unsigned long long>(res[2]);
    if (*voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "absorbVolume: the %s has %llu voxels, above 2^31 - 1", which, *voxels);
    return EMF_OK;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_absorbVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size, float dst_truncdist,
                         float max_weight, const emf_absorb_source_t* source, const float R[9], const float t[3],
                         const int32_t box_lo[3], const int32_t box_size[3], emf_absorb_t* record_dev, emf_stream_t stream) {
    if (!dst_tsdf || !dst_weights || !dst_res) return fail(EMF_E_ARG, "absorbVolume: the destination or its resolution is NULL");
    if (!source || !source->tsdf || !source->weights) return fail(EMF_E_ARG, "absorbVolume: the source or one of its volumes is NULL");
    if (!R || !t || !box_lo || !box_size || !record_dev) return fail(EMF_E_ARG, "absorbVolume: the pose, the box or the record is NULL");
    if ((reinterpret_cast<uintptr_t>(dst_tsdf) | reinterpret_cast<uintptr_t>(dst_weights) | reinterpret_cast<uintptr_t>(source->tsdf) |
         reinterpret_cast<uintptr_t>(source->weights)) & 3u)
        return fail(EMF_E_ARG, "absorbVolume: a misaligned volume");
    if (reinterpret_cast<uintptr_t>(record_dev) & 7u) return fail(EMF_E_ARG, "absorbVolume: a misaligned record");
    unsigned long long nDst = 0, nSrc = 0;
    EMF_TRY(check_volume(dst_res, "destination", &nDst));
    EMF_TRY(check_volume(source->res, "source", &nSrc));
    if (!positive_finite(dst_voxel_size) || !positive_finite(source->voxelSize))
        return fail(EMF_E_ARG, "absorbVolume: voxel sizes %g and %g", static_cast<double>(dst_voxel_size), static_cast<double>(source->voxelSize));
    if (!positive_finite(dst_truncdist) || !positive_finite(source->truncdist))
        return fail(EMF_E_ARG, "absorbVolume: truncation distances %g and %g", static_cast<double>(dst_truncdist),
                    static_cast<double>(source->truncdist));
    if (!positive_finite(max_weight)) return fail(EMF_E_ARG, "absorbVolume: maxWeight %g", static_cast<double>(max_weight));
    const float ratio = source->truncdist / dst_truncdist;  // one float32 division
    if (!positive_finite(ratio))
        return fail(EMF_E_ARG, "absorbVolume: the ratio of the truncation distances %g / %g is no positive finite float",
                    static_cast<double>(source->truncdist), static_cast<double>(dst_truncdist));
    // the arrays: two of the destination, up to four of the source; the destination's share no byte with any other
    const size_t dBytes = static_cast<size_t>(nDst) * sizeof(float), sBytes = static_cast<size_t>(nSrc) * sizeof(float);
    const void* others[4] = {source->tsdf, source->weights, source->fgVolMask, source->unseenTiles};
    const size_t otherBytes[4] = {sBytes, sBytes, static_cast<size_t>(nSrc), emf_hip_unseenTileBytes(source->res)};
    if (overlap(dst_tsdf, dBytes, dst_weights, dBytes)) return fail(EMF_E_ARG, "absorbVolume: the destination's tsdf and weights overlap");
    for (int k = 0; k < 4; ++k) {
        if (others[k] == nullptr) continue;
        if (overlap(dst_tsdf, dBytes, others[k], otherBytes[k]) || overlap(dst_weights, dBytes, others[k], otherBytes[k]))
            return fail(EMF_E_ARG, "absorbVolume: the destination overlaps the source (dst == src is no absorption)");
        if (overlap(record_dev, sizeof(emf_absorb_t), others[k], otherBytes[k]))
            return fail(EMF_E_ARG, "absorbVolume: the record overlaps the source");
    }
    if (overlap(record_dev, sizeof(emf_absorb_t), dst_tsdf, dBytes) || overlap(record_dev, sizeof(emf_absorb_t), dst_weights, dBytes))
        return fail(EMF_E_ARG, "absorbVolume: the record overlaps the destination");
    bool empty = false;
    for (int i = 0; i < 3; ++i) {
        if (box_lo[i] < 0 || box_size[i] < 0 || box_lo[i] > dst_res[i] || box_size[i] > dst_res[i] - box_lo[i])
            return fail(EMF_E_ARG, "absorbVolume: the box [%d, %d + %d) leaves the destination's %d voxels on axis %d", box_lo[i],
                        box_lo[i], box_size[i], dst_res[i], i);
        empty |= box_size[i] == 0;
    }
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ab_init, dim3(1), dim3(64), 0, s, record_dev, I3{dst_res[0], dst_res[1], dst_res[2]});
    if (empty) return launch_status("absorbVolume");
    AbsorbArgs a{};
    a.dstTsdf = dst_tsdf, a.dstWeights = dst_weights;
    a.srcTsdf = source->tsdf, a.srcWeights = source->weights, a.srcMask = source->fgVolMask, a.srcUnseen = source->unseenTiles;
    a.record = record_dev;
    a.nd = I3{dst_res[0], dst_res[1], dst_res[2]};
    a.ns = I3{source->res[0], source->res[1], source->res[2]};
    a.lo = I3{box_lo[0], box_lo[1], box_lo[2]};
    a.hi = I3{box_lo[0] + box_size[0], box_lo[1] + box_size[1], box_lo[2] + box_size[2]};
    a.t0 = I3{a.lo.x / kAbTileX, a.lo.y / kAbTileY, a.lo.z / kAbTileZ};
    a.ntx = static_cast<unsigned>((a.hi.x - 1) / kAbTileX - a.t0.x + 1);
    a.nty = static_cast<unsigned>((a.hi.y - 1) / kAbTileY - a.t0.y + 1);
    const unsigned ntz = static_cast<unsigned>((a.hi.z - 1) / kAbTileZ - a.t0.z + 1);
    a.voxD = dst_voxel_size, a.voxS = source->voxelSize, a.ratio = ratio, a.maxWeight = max_weight;
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t[i];
    // at most 64 * 256 * 256 = 2^22 tiles in a volume of EMF_DF_MAX_AXIS per axis
    hipLaunchKernelGGL(k_ab_absorb, dim3(a.ntx * a.nty * ntz), dim3(kAbBlock), 0, s, a);
    return launch_status("absorbVolume");
}

}  // extern "C"
