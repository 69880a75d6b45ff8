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
// The tile walk, the sample point, the outside rule, the gathers and the blend stand in resample.hpp, shared with lift.hip.
#include "resample.hpp"

namespace emf_hip {
namespace {

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

__global__ __launch_bounds__(kRsBlock) void k_ab_absorb(const AbsorbArgs a) {
    const RsLane ln = rs_lane(a.t0, a.ntx, a.nty, a.lo, a.hi);
    const int x = ln.x, y = ln.y;
    if (__ballot(ln.mine) == 0ull) return;  // wave-uniform; the kernel has no barrier

    const I3 nd = a.nd, ns = a.ns;
    const size_t dy = static_cast<size_t>(nd.x), dz = dy * nd.y;
    const size_t by = static_cast<size_t>(ns.x), bz = by * ns.y;
    const float* __restrict__ tb = a.srcTsdf;
    const float* __restrict__ wb = a.srcWeights;
    const uint8_t* __restrict__ fb = a.srcMask;
    const uint8_t* __restrict__ ub = a.srcUnseen;
    const unsigned stx = static_cast<unsigned>(ns.x + kRsTileX - 1) / kRsTileX, sty = static_cast<unsigned>(ns.y + kRsTileY - 1) / kRsTileY;
    const V3 halfS = half_extent(ns);
    const float fnx = static_cast<float>(ns.x), fny = static_cast<float>(ns.y), fnz = static_cast<float>(ns.z);
    const RsRows rows = rs_rows(a.R, rs_pd(x, nd.x, a.voxD), rs_pd(y, nd.y, a.voxD));

    unsigned cOut = 0u, cUnk = 0u, cMask = 0u, cSat = 0u, cFused = 0u, cFresh = 0u, cSolid = 0u;
    int lox = nd.x, loy = nd.y, loz = nd.z, hix = -1, hiy = -1, hiz = -1;

    if (ln.mine) {
        for (int z = ln.z0; z < ln.z1; ++z) {
            const V3 q = rs_sample(rows, a.R, a.t, rs_pd(z, nd.z, a.voxD), a.voxS, halfS);
            if (rs_outside(q, fnx, fny, fnz)) {
                cOut += 1u;
                continue;
            }
            const int lx = static_cast<int>(q.x), ly = static_cast<int>(q.y), lz = static_cast<int>(q.z);
            // corner 0 in a tile whose every weight is 0: its weight is not > 0, the cell is UNKNOWN unread
            if (ub != nullptr && ub[(static_cast<unsigned>(lz) / kRsTileZ * sty + static_cast<unsigned>(ly) / kRsTileY) * stx +
                                    static_cast<unsigned>(lx) / kRsTileX] != 0) {
                cUnk += 1u;
                continue;
            }
            const size_t c = (static_cast<size_t>(lz) * ns.y + ly) * by + lx;
            float w[8], t[8];
            rs_gather(wb, c, by, bz, w);
            rs_gather(tb, c, by, bz, t);
            const float s = rs_blend(__fsub_rn(q.x, static_cast<float>(lx)), __fsub_rn(q.y, static_cast<float>(ly)),
                                     __fsub_rn(q.z, static_cast<float>(lz)), t);
            if (!rs_all_seen(w) || !(s == s)) {
                cUnk += 1u;
                continue;
            }
            if (fb != nullptr && fb[rs_nearest(q, ns.y, by)] == 0) {
                cMask += 1u;
                continue;
            }
            if (!(fabsf(s) < 1.f)) {  // "at least one source truncation away": no value the destination can fuse
                cSat += 1u;
                continue;
            }
            const float u = fminf(fmaxf(__fmul_rn(s, a.ratio), -1.f), 1.f);
            const float wo = rs_min8(w);
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
    EMF_TRY(rs_check_volume("absorbVolume", dst_res, "destination", &nDst));
    EMF_TRY(rs_check_volume("absorbVolume", source->res, "source", &nSrc));
    if (!rs_positive_finite(dst_voxel_size) || !rs_positive_finite(source->voxelSize))
        return fail(EMF_E_ARG, "absorbVolume: voxel sizes %g and %g", static_cast<double>(dst_voxel_size), static_cast<double>(source->voxelSize));
    if (!rs_positive_finite(dst_truncdist) || !rs_positive_finite(source->truncdist))
        return fail(EMF_E_ARG, "absorbVolume: truncation distances %g and %g", static_cast<double>(dst_truncdist),
                    static_cast<double>(source->truncdist));
    if (!rs_positive_finite(max_weight)) return fail(EMF_E_ARG, "absorbVolume: maxWeight %g", static_cast<double>(max_weight));
    const float ratio = source->truncdist / dst_truncdist;  // one float32 division
    if (!rs_positive_finite(ratio))
        return fail(EMF_E_ARG, "absorbVolume: the ratio of the truncation distances %g / %g is no positive finite float",
                    static_cast<double>(source->truncdist), static_cast<double>(dst_truncdist));
    // the arrays: two of the destination, up to four of the source; the destination's share no byte with any other
    const size_t dBytes = static_cast<size_t>(nDst) * sizeof(float), sBytes = static_cast<size_t>(nSrc) * sizeof(float);
    const void* others[4] = {source->tsdf, source->weights, source->fgVolMask, source->unseenTiles};
    const size_t otherBytes[4] = {sBytes, sBytes, static_cast<size_t>(nSrc), emf_hip_unseenTileBytes(source->res)};
    if (rs_overlap(dst_tsdf, dBytes, dst_weights, dBytes)) return fail(EMF_E_ARG, "absorbVolume: the destination's tsdf and weights overlap");
    for (int k = 0; k < 4; ++k) {
        if (others[k] == nullptr) continue;
        if (rs_overlap(dst_tsdf, dBytes, others[k], otherBytes[k]) || rs_overlap(dst_weights, dBytes, others[k], otherBytes[k]))
            return fail(EMF_E_ARG, "absorbVolume: the destination overlaps the source (dst == src is no absorption)");
        if (rs_overlap(record_dev, sizeof(emf_absorb_t), others[k], otherBytes[k]))
            return fail(EMF_E_ARG, "absorbVolume: the record overlaps the source");
    }
    if (rs_overlap(record_dev, sizeof(emf_absorb_t), dst_tsdf, dBytes) || rs_overlap(record_dev, sizeof(emf_absorb_t), dst_weights, dBytes))
        return fail(EMF_E_ARG, "absorbVolume: the record overlaps the destination");
    bool empty = false;
    EMF_TRY(rs_check_box("absorbVolume", box_lo, box_size, dst_res, &empty));
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ab_init, dim3(1), dim3(64), 0, s, record_dev, I3{dst_res[0], dst_res[1], dst_res[2]});
    if (empty) return launch_status("absorbVolume");
    AbsorbArgs a{};
    a.dstTsdf = dst_tsdf, a.dstWeights = dst_weights;
    a.srcTsdf = source->tsdf, a.srcWeights = source->weights, a.srcMask = source->fgVolMask, a.srcUnseen = source->unseenTiles;
    a.record = record_dev;
    a.nd = I3{dst_res[0], dst_res[1], dst_res[2]};
    a.ns = I3{source->res[0], source->res[1], source->res[2]};
    const unsigned tiles = rs_tiles(box_lo, box_size, &a.lo, &a.hi, &a.t0, &a.ntx, &a.nty);
    a.voxD = dst_voxel_size, a.voxS = source->voxelSize, a.ratio = ratio, a.maxWeight = max_weight;
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t[i];
    hipLaunchKernelGGL(k_ab_absorb, dim3(tiles), dim3(kRsBlock), 0, s, a);
    return launch_status("absorbVolume");
}

}  // extern "C"
