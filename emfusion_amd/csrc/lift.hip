// lift.hip -- lifting a volume out of another (include/emf_hip.h "Lifting a volume"): the two passes that
// hand geometry from the background to a new object, on the conventions of absorb.hip and the shared resample.hpp.
//   k_lf_seed     the DESTINATION takes the source's band only where it has no observation of its own.  One workgroup per
//                 32 x 8 x 8 destination tile that meets the box, 256 lanes = 32 along x, 8 rows; a lane walks the tile's
//                 z planes with the x and y parts of the pose rows hoisted.  Per voxel: its own weight first -- KEPT is
//                 decided before anything of the source is read -- then the sample point, the outside rule, 8 + 8
//                 gathers, the mask byte, the band rule on the source's and on the destination's scale.
//   k_lf_release  the DESTINATION gives up the band voxels that a claimant holds.  The same walk; per voxel its own weight
//                 and tsdf first -- EMPTY and FREE cost 8 bytes and no transform -- then the sample point, the outside
//                 rule and the claimant's mask byte at the nearest voxel.
//   k_lf_init_*   one lane: the neutral record before the pass.
// A destination voxel reads and writes only itself: both passes are in place.  Only the words whose bits change are
// stored.  Per wave: wave_reduce of what is not zero anywhere in the wave, then one integer atomic per non-zero quantity
// from lane 0.  No float atomics, no LDS, no barrier.
#include "resample.hpp"

namespace emf_hip {
namespace {

static_assert(sizeof(emf_seed_t) == 88 && sizeof(emf_release_t) == 80, "mirrored by emfusion_amd/_lib.py");

struct SeedArgs {
    float* dstTsdf;
    float* dstWeights;
    const float* srcTsdf;
    const float* srcWeights;
    const uint8_t* srcMask;    // or NULL
    const uint8_t* srcUnseen;  // or NULL
    emf_seed_t* record;
    I3 nd, ns;                 // resolutions
    I3 lo, hi;                 // the box [lo, hi) of the destination
    I3 t0;                     // the first tile of the box, in tiles
    unsigned ntx, nty;         // tiles of the box along x and y
    float voxD, voxS, ratio, maxWeight;
    float R[9], t[3];          // source frame <- destination frame
};

struct ReleaseArgs {
    float* dstTsdf;
    float* dstWeights;
    const uint8_t* claim;      // or NULL: everything inside the claimant's cube
    emf_release_t* record;
    I3 nd, nc;
    I3 lo, hi;
    I3 t0;
    unsigned ntx, nty;
    float voxD, voxC;
    float R[9], t[3];          // claimant frame <- destination frame
};

__device__ __forceinline__ void add64(uint64_t* q, unsigned long long v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(q), v);
}

__global__ __launch_bounds__(kRsBlock) void k_lf_seed(const SeedArgs a) {
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

    unsigned cKept = 0u, cOut = 0u, cUnk = 0u, cMask = 0u, cSat = 0u, cSeed = 0u, cSolid = 0u;
    int lox = nd.x, loy = nd.y, loz = nd.z, hix = -1, hiy = -1, hiz = -1;

    if (ln.mine) {
        for (int z = ln.z0; z < ln.z1; ++z) {
            const size_t v = static_cast<size_t>(z) * dz + static_cast<size_t>(y) * dy + x;
            const float pw = a.dstWeights[v];
            if (pw > 0.f) {  // its own observation stands: nothing of the source is read
                cKept += 1u;
                continue;
            }
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
            const float u = __fmul_rn(s, a.ratio);
            if (!(fabsf(s) < 1.f) || !(fabsf(u) < 1.f)) {  // outside the source's band or the destination's own
                cSat += 1u;
                continue;
            }
            const float nw = fminf(rs_min8(w), a.maxWeight);
            const float pt = a.dstTsdf[v];
            cSeed += 1u;
            if (!(u > 0.f)) cSolid += 1u;
            lox = min(lox, x), hix = max(hix, x);
            loy = min(loy, y), hiy = max(hiy, y);
            loz = min(loz, z), hiz = max(hiz, z);
            if (__float_as_uint(u) != __float_as_uint(pt)) a.dstTsdf[v] = u;
            if (__float_as_uint(nw) != __float_as_uint(pw)) a.dstWeights[v] = nw;
        }
    }

    // a lane holds at most 8 voxels, a wave 512: every wave sum fits 32 bits
    const unsigned lane = threadIdx.x & 63u;
    cKept = wave_reduce<OpAdd>(cKept), cOut = wave_reduce<OpAdd>(cOut), cUnk = wave_reduce<OpAdd>(cUnk);
    cMask = wave_reduce<OpAdd>(cMask), cSat = wave_reduce<OpAdd>(cSat);
    const bool anySeed = __ballot(cSeed != 0u) != 0ull;  // wave-uniform
    if (anySeed) {
        cSeed = wave_reduce<OpAdd>(cSeed), cSolid = wave_reduce<OpAdd>(cSolid);
        lox = wave_reduce<OpMin>(lox), loy = wave_reduce<OpMin>(loy), loz = wave_reduce<OpMin>(loz);
        hix = wave_reduce<OpMax>(hix), hiy = wave_reduce<OpMax>(hiy), hiz = wave_reduce<OpMax>(hiz);
    }
    if (lane == 0u) {
        emf_seed_t* out = a.record;
        add64(&out->visited, static_cast<unsigned long long>(cKept) + cOut + cUnk + cMask + cSat + (anySeed ? cSeed : 0u));
        add64(&out->kept, cKept), add64(&out->outside, cOut), add64(&out->unknown, cUnk), add64(&out->masked, cMask);
        add64(&out->saturated, cSat);
        if (anySeed) {
            add64(&out->seeded, cSeed), add64(&out->solid, cSolid);
            atomicMin(&out->lo[0], lox), atomicMin(&out->lo[1], loy), atomicMin(&out->lo[2], loz);
            atomicMax(&out->hi[0], hix), atomicMax(&out->hi[1], hiy), atomicMax(&out->hi[2], hiz);
        }
    }
}

__global__ __launch_bounds__(kRsBlock) void k_lf_release(const ReleaseArgs a) {
    const RsLane ln = rs_lane(a.t0, a.ntx, a.nty, a.lo, a.hi);
    const int x = ln.x, y = ln.y;
    if (__ballot(ln.mine) == 0ull) return;  // wave-uniform; the kernel has no barrier

    const I3 nd = a.nd, nc = a.nc;
    const size_t dy = static_cast<size_t>(nd.x), dz = dy * nd.y;
    const size_t by = static_cast<size_t>(nc.x);
    const uint8_t* __restrict__ cb = a.claim;
    const V3 halfC = half_extent(nc);
    const float fnx = static_cast<float>(nc.x), fny = static_cast<float>(nc.y), fnz = static_cast<float>(nc.z);
    const RsRows rows = rs_rows(a.R, rs_pd(x, nd.x, a.voxD), rs_pd(y, nd.y, a.voxD));

    unsigned cEmpty = 0u, cFree = 0u, cOut = 0u, cUncl = 0u, cRel = 0u, cSolid = 0u;
    int lox = nd.x, loy = nd.y, loz = nd.z, hix = -1, hiy = -1, hiz = -1;

    if (ln.mine) {
        for (int z = ln.z0; z < ln.z1; ++z) {
            const size_t v = static_cast<size_t>(z) * dz + static_cast<size_t>(y) * dy + x;
            const float pw = a.dstWeights[v], pt = a.dstTsdf[v];
            if (!(pw > 0.f)) {
                cEmpty += 1u;
                continue;
            }
            if (!(fabsf(pt) < 1.f)) {  // free space and NaN stay: only the band is released
                cFree += 1u;
                continue;
            }
            const V3 q = rs_sample(rows, a.R, a.t, rs_pd(z, nd.z, a.voxD), a.voxC, halfC);
            if (rs_outside(q, fnx, fny, fnz)) {
                cOut += 1u;
                continue;
            }
            if (cb != nullptr && cb[rs_nearest(q, nc.y, by)] == 0) {
                cUncl += 1u;
                continue;
            }
            cRel += 1u;
            if (!(pt > 0.f)) cSolid += 1u;
            lox = min(lox, x), hix = max(hix, x);
            loy = min(loy, y), hiy = max(hiy, y);
            loz = min(loz, z), hiz = max(hiz, z);
            // what TSDF::reset leaves in an unseen voxel; pw > 0, so its word always changes
            if (__float_as_uint(pt) != 0u) a.dstTsdf[v] = 0.f;
            a.dstWeights[v] = 0.f;
        }
    }

    const unsigned lane = threadIdx.x & 63u;
    cEmpty = wave_reduce<OpAdd>(cEmpty), cFree = wave_reduce<OpAdd>(cFree), cOut = wave_reduce<OpAdd>(cOut);
    cUncl = wave_reduce<OpAdd>(cUncl);
    const bool anyRel = __ballot(cRel != 0u) != 0ull;  // wave-uniform
    if (anyRel) {
        cRel = wave_reduce<OpAdd>(cRel), cSolid = wave_reduce<OpAdd>(cSolid);
        lox = wave_reduce<OpMin>(lox), loy = wave_reduce<OpMin>(loy), loz = wave_reduce<OpMin>(loz);
        hix = wave_reduce<OpMax>(hix), hiy = wave_reduce<OpMax>(hiy), hiz = wave_reduce<OpMax>(hiz);
    }
    if (lane == 0u) {
        emf_release_t* out = a.record;
        add64(&out->visited, static_cast<unsigned long long>(cEmpty) + cFree + cOut + cUncl + (anyRel ? cRel : 0u));
        add64(&out->empty, cEmpty), add64(&out->free_space, cFree), add64(&out->outside, cOut), add64(&out->unclaimed, cUncl);
        if (anyRel) {
            add64(&out->released, cRel), add64(&out->solid, cSolid);
            atomicMin(&out->lo[0], lox), atomicMin(&out->lo[1], loy), atomicMin(&out->lo[2], loz);
            atomicMax(&out->hi[0], hix), atomicMax(&out->hi[1], hiy), atomicMax(&out->hi[2], hiz);
        }
    }
}

// one lane: the neutral record
template <typename Record>
__global__ void k_lf_init(Record* record, I3 nd) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Record r{};
    r.lo[0] = nd.x, r.lo[1] = nd.y, r.lo[2] = nd.z;
    r.hi[0] = r.hi[1] = r.hi[2] = -1;
    *record = r;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_seedVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size, float dst_truncdist,
                       float max_weight, const emf_absorb_source_t* source, const float R[9], const float t[3],
                       const int32_t box_lo[3], const int32_t box_size[3], emf_seed_t* record_dev, emf_stream_t stream) {
    if (!dst_tsdf || !dst_weights || !dst_res) return fail(EMF_E_ARG, "seedVolume: the destination or its resolution is NULL");
    if (!source || !source->tsdf || !source->weights) return fail(EMF_E_ARG, "seedVolume: the source or one of its volumes is NULL");
    if (!R || !t || !box_lo || !box_size || !record_dev) return fail(EMF_E_ARG, "seedVolume: the pose, the box or the record is NULL");
    if ((reinterpret_cast<uintptr_t>(dst_tsdf) | reinterpret_cast<uintptr_t>(dst_weights) | reinterpret_cast<uintptr_t>(source->tsdf) |
         reinterpret_cast<uintptr_t>(source->weights)) & 3u)
        return fail(EMF_E_ARG, "seedVolume: a misaligned volume");
    if (reinterpret_cast<uintptr_t>(record_dev) & 7u) return fail(EMF_E_ARG, "seedVolume: a misaligned record");
    unsigned long long nDst = 0, nSrc = 0;
    EMF_TRY(rs_check_volume("seedVolume", dst_res, "destination", &nDst));
    EMF_TRY(rs_check_volume("seedVolume", source->res, "source", &nSrc));
    if (!rs_positive_finite(dst_voxel_size) || !rs_positive_finite(source->voxelSize))
        return fail(EMF_E_ARG, "seedVolume: voxel sizes %g and %g", static_cast<double>(dst_voxel_size), static_cast<double>(source->voxelSize));
    if (!rs_positive_finite(dst_truncdist) || !rs_positive_finite(source->truncdist))
        return fail(EMF_E_ARG, "seedVolume: truncation distances %g and %g", static_cast<double>(dst_truncdist),
                    static_cast<double>(source->truncdist));
    if (!rs_positive_finite(max_weight)) return fail(EMF_E_ARG, "seedVolume: maxWeight %g", static_cast<double>(max_weight));
    const float ratio = source->truncdist / dst_truncdist;  // one float32 division
    if (!rs_positive_finite(ratio))
        return fail(EMF_E_ARG, "seedVolume: the ratio of the truncation distances %g / %g is no positive finite float",
                    static_cast<double>(source->truncdist), static_cast<double>(dst_truncdist));
    // the arrays: two of the destination, up to four of the source; the destination's share no byte with any other
    const size_t dBytes = static_cast<size_t>(nDst) * sizeof(float), sBytes = static_cast<size_t>(nSrc) * sizeof(float);
    const void* others[4] = {source->tsdf, source->weights, source->fgVolMask, source->unseenTiles};
    const size_t otherBytes[4] = {sBytes, sBytes, static_cast<size_t>(nSrc), emf_hip_unseenTileBytes(source->res)};
    if (rs_overlap(dst_tsdf, dBytes, dst_weights, dBytes)) return fail(EMF_E_ARG, "seedVolume: the destination's tsdf and weights overlap");
    for (int k = 0; k < 4; ++k) {
        if (others[k] == nullptr) continue;
        if (rs_overlap(dst_tsdf, dBytes, others[k], otherBytes[k]) || rs_overlap(dst_weights, dBytes, others[k], otherBytes[k]))
            return fail(EMF_E_ARG, "seedVolume: the destination overlaps the source");
        if (rs_overlap(record_dev, sizeof(emf_seed_t), others[k], otherBytes[k])) return fail(EMF_E_ARG, "seedVolume: the record overlaps the source");
    }
    if (rs_overlap(record_dev, sizeof(emf_seed_t), dst_tsdf, dBytes) || rs_overlap(record_dev, sizeof(emf_seed_t), dst_weights, dBytes))
        return fail(EMF_E_ARG, "seedVolume: the record overlaps the destination");
    bool empty = false;
    EMF_TRY(rs_check_box("seedVolume", box_lo, box_size, dst_res, &empty));
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_lf_init<emf_seed_t>, dim3(1), dim3(64), 0, s, record_dev, I3{dst_res[0], dst_res[1], dst_res[2]});
    if (empty) return launch_status("seedVolume");
    SeedArgs a{};
    a.dstTsdf = dst_tsdf, a.dstWeights = dst_weights;
    a.srcTsdf = source->tsdf, a.srcWeights = source->weights, a.srcMask = source->fgVolMask, a.srcUnseen = source->unseenTiles;
    a.record = record_dev;
    a.nd = I3{dst_res[0], dst_res[1], dst_res[2]};
    a.ns = I3{source->res[0], source->res[1], source->res[2]};
    const unsigned tiles = rs_tiles(box_lo, box_size, &a.lo, &a.hi, &a.t0, &a.ntx, &a.nty);
    a.voxD = dst_voxel_size, a.voxS = source->voxelSize, a.ratio = ratio, a.maxWeight = max_weight;
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t[i];
    hipLaunchKernelGGL(k_lf_seed, dim3(tiles), dim3(kRsBlock), 0, s, a);
    return launch_status("seedVolume");
}

int emf_hip_releaseVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size,
                          const uint8_t* claim_mask, const int32_t claim_res[3], float claim_voxel_size, const float R[9],
                          const float t[3], const int32_t box_lo[3], const int32_t box_size[3], emf_release_t* record_dev,
                          emf_stream_t stream) {
    if (!dst_tsdf || !dst_weights || !dst_res) return fail(EMF_E_ARG, "releaseVolume: the destination or its resolution is NULL");
    if (!claim_res) return fail(EMF_E_ARG, "releaseVolume: the claimant's resolution is NULL");
    if (!R || !t || !box_lo || !box_size || !record_dev) return fail(EMF_E_ARG, "releaseVolume: the pose, the box or the record is NULL");
    if ((reinterpret_cast<uintptr_t>(dst_tsdf) | reinterpret_cast<uintptr_t>(dst_weights)) & 3u)
        return fail(EMF_E_ARG, "releaseVolume: a misaligned volume");
    if (reinterpret_cast<uintptr_t>(record_dev) & 7u) return fail(EMF_E_ARG, "releaseVolume: a misaligned record");
    unsigned long long nDst = 0, nClaim = 0;
    EMF_TRY(rs_check_volume("releaseVolume", dst_res, "destination", &nDst));
    EMF_TRY(rs_check_volume("releaseVolume", claim_res, "claimant", &nClaim));
    if (!rs_positive_finite(dst_voxel_size) || !rs_positive_finite(claim_voxel_size))
        return fail(EMF_E_ARG, "releaseVolume: voxel sizes %g and %g", static_cast<double>(dst_voxel_size), static_cast<double>(claim_voxel_size));
    const size_t dBytes = static_cast<size_t>(nDst) * sizeof(float), cBytes = static_cast<size_t>(nClaim);
    if (rs_overlap(dst_tsdf, dBytes, dst_weights, dBytes)) return fail(EMF_E_ARG, "releaseVolume: the destination's tsdf and weights overlap");
    if (claim_mask != nullptr) {
        if (rs_overlap(dst_tsdf, dBytes, claim_mask, cBytes) || rs_overlap(dst_weights, dBytes, claim_mask, cBytes))
            return fail(EMF_E_ARG, "releaseVolume: the destination overlaps the claimant's mask");
        if (rs_overlap(record_dev, sizeof(emf_release_t), claim_mask, cBytes))
            return fail(EMF_E_ARG, "releaseVolume: the record overlaps the claimant's mask");
    }
    if (rs_overlap(record_dev, sizeof(emf_release_t), dst_tsdf, dBytes) || rs_overlap(record_dev, sizeof(emf_release_t), dst_weights, dBytes))
        return fail(EMF_E_ARG, "releaseVolume: the record overlaps the destination");
    bool empty = false;
    EMF_TRY(rs_check_box("releaseVolume", box_lo, box_size, dst_res, &empty));
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_lf_init<emf_release_t>, dim3(1), dim3(64), 0, s, record_dev, I3{dst_res[0], dst_res[1], dst_res[2]});
    if (empty) return launch_status("releaseVolume");
    ReleaseArgs a{};
    a.dstTsdf = dst_tsdf, a.dstWeights = dst_weights, a.claim = claim_mask, a.record = record_dev;
    a.nd = I3{dst_res[0], dst_res[1], dst_res[2]};
    a.nc = I3{claim_res[0], claim_res[1], claim_res[2]};
    const unsigned tiles = rs_tiles(box_lo, box_size, &a.lo, &a.hi, &a.t0, &a.ntx, &a.nty);
    a.voxD = dst_voxel_size, a.voxC = claim_voxel_size;
    for (int i = 0; i < 9; ++i) a.R[i] = R[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t[i];
    hipLaunchKernelGGL(k_lf_release, dim3(tiles), dim3(kRsBlock), 0, s, a);
    return launch_status("releaseVolume");
}

}  // extern "C"
