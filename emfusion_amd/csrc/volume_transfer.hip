// volume_transfer.hip -- the passes that hand the signed-distance band of one volume to another through a rigid pose, in
// place in the DESTINATION (include/emf_hip.h "Absorbing a volume", "Lifting a volume" and "Merging a volume", DESIGN.md
// 5.29, 5.30 and 5.32).
//   k_ab_absorb   the band of the SOURCE, fused into the destination by the destination's running average.
//   k_mg_merge    the same into an object: the (fg, bg) counts of a fused voxel follow the band (MergePolicy).
//   k_lf_seed     the destination takes the source's band only where it has no observation of its own.
//   k_lf_release  the destination gives up the band voxels that a claimant holds.
// One workgroup per 32 x 8 x 8 destination tile that meets the box, 256 lanes = 32 along x, 8 rows; a lane walks the tile's
// z planes with the x and y parts of the three pose rows hoisted.  A wave whose lanes all lie outside the box leaves.
// Absorb, merge and seed are one walk (rs_transfer) under three policies resolved at compile time: per voxel what the policy asks
// of the destination first, then the sample point and what the source holds there (rs_source of resample.hpp: the
// outside rule, 8 + 8 dependent gathers, the mask byte), then the policy's band rule and store.  The release reads its
// own weight and tsdf first -- EMPTY and FREE cost 8 bytes and no transform -- then the sample point, the outside rule
// and the claimant's mask byte at the nearest voxel.  A destination voxel reads and writes only itself: the passes are in
// place.  Only the words whose bits change are stored.  Per wave: wave_reduce of what is not zero anywhere in the wave,
// then one integer atomic per non-zero quantity from lane 0; the record does not depend on the order of lanes, waves or
// workgroups.  No float atomics, no LDS, no barrier.  Every float step is one float32 operation (resample.hpp).
// Each kernel has a COLOUR variant (k_ab_absorb_color, k_lf_seed_color, k_lf_release<true>), the same walk with a template flag resolved at compile
// time: on the FUSED / SEEDED / RELEASED path alone the voxel's colour entry -- one 8-byte word -- follows the band, from
// the source's entry at the nearest voxel, in exact integer arithmetic, and two more counts go into a second record.
#include <type_traits>

#include "resample.hpp"

namespace emf_hip {
namespace {

static_assert(sizeof(emf_absorb_t) == 88 && sizeof(emf_absorb_source_t) == 56, "mirrored by emfusion_amd/_lib.py");
static_assert(sizeof(emf_seed_t) == 88 && sizeof(emf_release_t) == 80, "mirrored by emfusion_amd/_lib.py");
static_assert(sizeof(emf_color_moved_t) == 16 && sizeof(uint2) == 4 * sizeof(uint16_t), "mirrored by emfusion_amd/_lib.py");
static_assert(sizeof(emf_merge_counts_t) == 16 && sizeof(float2) == 2 * sizeof(float), "mirrored by emfusion_amd/_lib.py");

// the arguments of a pass: with colour, the colour volumes, the colour record and the cap behind the plain ones
template <typename Record, bool Color>
using TransferArgs = std::conditional_t<Color, ResampleColorArgs<Record>, ResampleArgs<Record>>;

// the colour counts of a lane and their way into the colour record; empty without colour
template <bool Color>
struct ColorCounts {
    __device__ __forceinline__ void reduce() {}
    template <typename Args>
    __device__ __forceinline__ void commit(const Args&) const {}
};

template <>
struct ColorCounts<true> {
    unsigned cCol = 0u, cUncol = 0u;
    __device__ __forceinline__ void reduce() { cCol = wave_reduce<OpAdd>(cCol), cUncol = wave_reduce<OpAdd>(cUncol); }
    template <typename Args>
    __device__ __forceinline__ void commit(const Args& a) const {
        rs_add64(&a.colorRecord->colored, cCol), rs_add64(&a.colorRecord->uncolored, cUncol);
    }
};

// A policy of rs_transfer holds a lane's counts beyond outside / unknown / masked and says
//   wants(a, v)       what the destination voxel v decides before anything of the source is read: false = done;
//   take(a, v, q, s, w)  what becomes of a VALUE s at the sample point q with the corner weights w: true = the voxel was
//                     written and counts for the bounds; with colour, the voxel's colour entry follows here;
//   reduce(any)       the wave sums of its counts (those of the written voxels only where `any` lane wrote one);
//   commit(a, any)    lane 0: its counts into the record(s); returns how many voxels they stand for.

template <bool Color>
struct AbsorbPolicy {
    using Record = emf_absorb_t;
    using Args = TransferArgs<Record, Color>;
    unsigned cSat = 0u, cFused = 0u, cFresh = 0u, cSolid = 0u;
    ColorCounts<Color> color;

    __device__ __forceinline__ bool wants(const Args&, size_t) { return true; }
    __device__ __forceinline__ bool take(const Args& a, size_t v, const V3& q, float s, const float (&w)[8]) {
        return take(a, v, q, s, w, [](bool) {});
    }
    // between(fresh): what a policy built on this one does to a FUSED voxel once its band is written, before its colour
    // follows; fresh: the voxel had no observation of its own
    template <typename Between>
    __device__ __forceinline__ bool take(const Args& a, size_t v, const V3& q, float s, const float (&w)[8], Between between) {
        if (!(fabsf(s) < 1.f)) {  // "at least one source truncation away": no value the destination can fuse
            cSat += 1u;
            return false;
        }
        const float u = fminf(fmaxf(__fmul_rn(s, a.ratio), -1.f), 1.f);
        const float wo = rs_min8(w);
        const float pw = a.dstWeights[v], pt = a.dstTsdf[v];
        float nt, nw;
        const bool fresh = !(pw > 0.f);
        if (fresh) {  // a select: whatever an unseen voxel holds goes nowhere
            nt = u;
            nw = fminf(wo, a.maxWeight);
            cFresh += 1u;
        } else {
            nt = __fdiv_rn(__fadd_rn(mul_rounded(pw, pt), mul_rounded(wo, u)), __fadd_rn(pw, wo));
            nw = fminf(__fadd_rn(pw, wo), a.maxWeight);
        }
        cFused += 1u;
        if (!(nt > 0.f)) cSolid += 1u;
        if (__float_as_uint(nt) != __float_as_uint(pt)) a.dstTsdf[v] = nt;
        if (__float_as_uint(nw) != __float_as_uint(pw)) a.dstWeights[v] = nw;
        between(fresh);
        if constexpr (Color) {
            const uint2 S = rs_color_source(a.srcColor, q, a.ns.y, static_cast<size_t>(a.ns.x));
            if (rs_color_weight(S) == 0u) {  // UNCOLOURED: an unobserved voxel's entry is not evidence, any other stays
                color.cUncol += 1u;
                if (fresh) a.dstColor[v] = make_uint2(0u, 0u);
            } else {  // COLOURED: the entry is read once, as one word, before anything of it is written
                color.cCol += 1u;
                const uint2 D = a.dstColor[v];
                const uint2 N = rs_color_fuse(D, S, fresh ? 0u : rs_color_weight(D), a.capq);
                if (N.x != D.x || N.y != D.y) a.dstColor[v] = N;
            }
        }
        return true;
    }
    __device__ __forceinline__ void reduce(bool any) {
        cSat = wave_reduce<OpAdd>(cSat);
        if (any) cFused = wave_reduce<OpAdd>(cFused), cFresh = wave_reduce<OpAdd>(cFresh), cSolid = wave_reduce<OpAdd>(cSolid), color.reduce();
    }
    __device__ __forceinline__ unsigned long long commit(const Args& a, bool any) const {
        Record* out = a.record;
        rs_add64(&out->saturated, cSat);
        if (any) rs_add64(&out->fused, cFused), rs_add64(&out->fresh, cFresh), rs_add64(&out->solid, cSolid), color.commit(a);
        return static_cast<unsigned long long>(cSat) + (any ? cFused : 0u);
    }
};

template <bool Color>
struct SeedPolicy {
    using Record = emf_seed_t;
    using Args = TransferArgs<Record, Color>;
    unsigned cKept = 0u, cSat = 0u, cSeed = 0u, cSolid = 0u;
    float pw = 0.f;  // the voxel's own weight
    ColorCounts<Color> color;

    __device__ __forceinline__ bool wants(const Args& a, size_t v) {
        pw = a.dstWeights[v];
        if (pw > 0.f) cKept += 1u;  // its own observation stands: nothing of the source is read
        return !(pw > 0.f);
    }
    __device__ __forceinline__ bool take(const Args& a, size_t v, const V3& q, float s, const float (&w)[8]) {
        const float u = __fmul_rn(s, a.ratio);
        if (!(fabsf(s) < 1.f) || !(fabsf(u) < 1.f)) {  // outside the source's band or the destination's own
            cSat += 1u;
            return false;
        }
        const float nw = fminf(rs_min8(w), a.maxWeight);
        const float pt = a.dstTsdf[v];
        cSeed += 1u;
        if (!(u > 0.f)) cSolid += 1u;
        if (__float_as_uint(u) != __float_as_uint(pt)) a.dstTsdf[v] = u;
        if (__float_as_uint(nw) != __float_as_uint(pw)) a.dstWeights[v] = nw;
        if constexpr (Color) {  // the voxel had no observation: its entry is the source's, capped, or none; not read
            const uint2 S = rs_color_source(a.srcColor, q, a.ns.y, static_cast<size_t>(a.ns.x));
            const unsigned sw = rs_color_weight(S);
            if (sw == 0u) {
                color.cUncol += 1u;
                a.dstColor[v] = make_uint2(0u, 0u);
            } else {
                color.cCol += 1u;
                a.dstColor[v] = make_uint2(S.x, (S.y & 0xffffu) | min(sw, a.capq) << 16);
            }
        }
        return true;
    }
    __device__ __forceinline__ void reduce(bool any) {
        cKept = wave_reduce<OpAdd>(cKept), cSat = wave_reduce<OpAdd>(cSat);
        if (any) cSeed = wave_reduce<OpAdd>(cSeed), cSolid = wave_reduce<OpAdd>(cSolid), color.reduce();
    }
    __device__ __forceinline__ unsigned long long commit(const Args& a, bool any) const {
        Record* out = a.record;
        rs_add64(&out->kept, cKept), rs_add64(&out->saturated, cSat);
        if (any) rs_add64(&out->seeded, cSeed), rs_add64(&out->solid, cSolid), color.commit(a);
        return static_cast<unsigned long long>(cKept) + cSat + (any ? cSeed : 0u);
    }
};

// What a merge is handed on top of an absorption: the (fg, bg) count pairs of both volumes, a pair = one 8-byte word, and
// the record of the pairs that came out as foreground.
template <bool Color>
struct MergeArgs : TransferArgs<emf_absorb_t, Color> {
    float2* dstFgbg;
    const float2* srcFgbg;
    emf_merge_counts_t* counts;
};

// The destination is an object: the absorption's band rule, unchanged, and on the FUSED path alone the voxel's count
// pair follows the band -- the source's pair at the nearest voxel replaces that of a FRESH voxel and is added to any
// other, one float32 sum per count.
template <bool Color>
struct MergePolicy {
    using Record = emf_absorb_t;
    using Args = MergeArgs<Color>;
    AbsorbPolicy<Color> band;
    unsigned cFg = 0u, cGained = 0u;

    __device__ __forceinline__ bool wants(const Args&, size_t) { return true; }
    __device__ __forceinline__ bool take(const Args& a, size_t v, const V3& q, float s, const float (&w)[8]) {
        return band.take(a, v, q, s, w, [&](bool fresh) {
            const float2 S = a.srcFgbg[rs_nearest(q, a.ns.y, static_cast<size_t>(a.ns.x))];
            const float2 D = a.dstFgbg[v];  // read once, as one word, before anything of it is written
            const float2 N = fresh ? S : make_float2(__fadd_rn(D.x, S.x), __fadd_rn(D.y, S.y));
            if (N.x > N.y) {
                cFg += 1u;
                if (fresh || !(D.x > D.y)) cGained += 1u;
            }
            if (__float_as_uint(N.x) != __float_as_uint(D.x) || __float_as_uint(N.y) != __float_as_uint(D.y)) a.dstFgbg[v] = N;
        });
    }
    __device__ __forceinline__ void reduce(bool any) {
        band.reduce(any);
        if (any) cFg = wave_reduce<OpAdd>(cFg), cGained = wave_reduce<OpAdd>(cGained);
    }
    __device__ __forceinline__ unsigned long long commit(const Args& a, bool any) const {
        if (any) rs_add64(&a.counts->foreground, cFg), rs_add64(&a.counts->gained, cGained);
        return band.commit(a, any);
    }
};

template <typename Policy>
__device__ __forceinline__ void rs_transfer(const typename Policy::Args& a) {
    const RsLane ln = rs_lane(a.t0, a.ntx, a.nty, a.lo, a.hi);
    const int x = ln.x, y = ln.y;
    if (__ballot(ln.mine) == 0ull) return;  // wave-uniform; the kernel has no barrier

    const I3 nd = a.nd;
    const size_t dy = static_cast<size_t>(nd.x), dz = dy * nd.y;
    const RsVolume src = rs_volume(a.srcTsdf, a.srcWeights, a.srcMask, a.srcUnseen, a.ns);
    const RsRows rows = rs_rows(a.R, rs_pd(x, nd.x, a.voxD), rs_pd(y, nd.y, a.voxD));

    Policy p;
    unsigned cOut = 0u, cUnk = 0u, cMask = 0u;
    RsBounds written(nd);

    if (ln.mine) {
        for (int z = ln.z0; z < ln.z1; ++z) {
            const size_t v = static_cast<size_t>(z) * dz + static_cast<size_t>(y) * dy + x;
            if (!p.wants(a, v)) continue;
            float s, w[8];
            const V3 q = rs_sample(rows, a.R, a.t, rs_pd(z, nd.z, a.voxD), a.voxS, src.half);
            switch (rs_source(src, q, s, w)) {
                case RsClass::Outside: cOut += 1u; break;
                case RsClass::Unknown: cUnk += 1u; break;
                case RsClass::Masked: cMask += 1u; break;
                case RsClass::Value:
                    if (p.take(a, v, q, s, w)) written.include(x, y, z);
            }
        }
    }

    // a lane holds at most 8 voxels, a wave 512: every wave sum fits 32 bits
    cOut = wave_reduce<OpAdd>(cOut), cUnk = wave_reduce<OpAdd>(cUnk), cMask = wave_reduce<OpAdd>(cMask);
    const bool any = written.any();
    p.reduce(any);
    if (any) written.reduce();
    if ((threadIdx.x & 63u) == 0u) {
        typename Policy::Record* out = a.record;
        rs_add64(&out->visited, static_cast<unsigned long long>(cOut) + cUnk + cMask + p.commit(a, any));
        rs_add64(&out->outside, cOut), rs_add64(&out->unknown, cUnk), rs_add64(&out->masked, cMask);
        if (any) written.commit(out);
    }
}

__global__ __launch_bounds__(kRsBlock) void k_ab_absorb(const ResampleArgs<emf_absorb_t> a) { rs_transfer<AbsorbPolicy<false>>(a); }

// Left alone the colour variants of the walk come out at 72 and 69 VGPRs, 7 waves per SIMD; held to the plain kernels' 8
// waves they allocate 60 and 63 like them, without scratch (as k_render_view and k_ct_probe are held).
__global__ __launch_bounds__(kRsBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_ab_absorb_color(
    const ResampleColorArgs<emf_absorb_t> a) {
    rs_transfer<AbsorbPolicy<true>>(a);
}

__global__ __launch_bounds__(kRsBlock) void k_lf_seed(const ResampleArgs<emf_seed_t> a) { rs_transfer<SeedPolicy<false>>(a); }

__global__ __launch_bounds__(kRsBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_lf_seed_color(
    const ResampleColorArgs<emf_seed_t> a) {
    rs_transfer<SeedPolicy<true>>(a);
}

// The merge carries one more gather and one more 8-byte word per fused voxel than the absorption; both variants are held
// to the absorption's 8 waves per SIMD, without scratch.
__global__ __launch_bounds__(kRsBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_mg_merge(const MergeArgs<false> a) {
    rs_transfer<MergePolicy<false>>(a);
}

__global__ __launch_bounds__(kRsBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_mg_merge_color(const MergeArgs<true> a) {
    rs_transfer<MergePolicy<true>>(a);
}

// one lane: the neutral records before a merge, the colour record among them where there is one
template <bool Color>
__global__ void k_mg_init(emf_absorb_t* record, I3 nd, emf_merge_counts_t* counts, emf_color_moved_t* colorRecord) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    *record = rs_neutral<emf_absorb_t>(nd);
    *counts = emf_merge_counts_t{0u, 0u};
    if constexpr (Color) *colorRecord = emf_color_moved_t{0u, 0u};
}

// the source is the claimant: its mask (or NULL: everything inside its cube), its resolution and voxel size
template <bool Color>
__global__ __launch_bounds__(kRsBlock) void k_lf_release(const TransferArgs<emf_release_t, Color> a) {
    const RsLane ln = rs_lane(a.t0, a.ntx, a.nty, a.lo, a.hi);
    const int x = ln.x, y = ln.y;
    if (__ballot(ln.mine) == 0ull) return;  // wave-uniform; the kernel has no barrier

    const I3 nd = a.nd;
    const size_t dy = static_cast<size_t>(nd.x), dz = dy * nd.y;
    const RsVolume claim = rs_volume(nullptr, nullptr, a.srcMask, nullptr, a.ns);
    const RsRows rows = rs_rows(a.R, rs_pd(x, nd.x, a.voxD), rs_pd(y, nd.y, a.voxD));

    unsigned cEmpty = 0u, cFree = 0u, cOut = 0u, cUncl = 0u, cRel = 0u, cSolid = 0u;
    ColorCounts<Color> color;
    RsBounds released(nd);

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
            const V3 q = rs_sample(rows, a.R, a.t, rs_pd(z, nd.z, a.voxD), a.voxS, claim.half);
            if (rs_outside(q, claim.fn)) {
                cOut += 1u;
                continue;
            }
            if (rs_masked(claim, q)) {
                cUncl += 1u;
                continue;
            }
            cRel += 1u;
            if (!(pt > 0.f)) cSolid += 1u;
            released.include(x, y, z);
            // what TSDF::reset leaves in an unseen voxel; pw > 0, so its word always changes
            if (__float_as_uint(pt) != 0u) a.dstTsdf[v] = 0.f;
            a.dstWeights[v] = 0.f;
            if constexpr (Color) {  // and no colour: COLOURED counts the entries that held something
                const uint2 D = a.dstColor[v];
                if ((D.x | D.y) != 0u) {
                    color.cCol += 1u;
                    a.dstColor[v] = make_uint2(0u, 0u);
                } else {
                    color.cUncol += 1u;
                }
            }
        }
    }

    cEmpty = wave_reduce<OpAdd>(cEmpty), cFree = wave_reduce<OpAdd>(cFree), cOut = wave_reduce<OpAdd>(cOut);
    cUncl = wave_reduce<OpAdd>(cUncl);
    const bool any = released.any();
    if (any) {
        cRel = wave_reduce<OpAdd>(cRel), cSolid = wave_reduce<OpAdd>(cSolid);
        color.reduce();
        released.reduce();
    }
    if ((threadIdx.x & 63u) == 0u) {
        emf_release_t* out = a.record;
        rs_add64(&out->visited, static_cast<unsigned long long>(cEmpty) + cFree + cOut + cUncl + (any ? cRel : 0u));
        rs_add64(&out->empty, cEmpty), rs_add64(&out->free_space, cFree), rs_add64(&out->outside, cOut), rs_add64(&out->unclaimed, cUncl);
        if (any) {
            rs_add64(&out->released, cRel), rs_add64(&out->solid, cSolid);
            color.commit(a);
            released.commit(out);
        }
    }
}


// absorbVolumeColor and seedVolumeColor: every check of the sibling, then those of the colour arguments, then the launch
template <typename Record>
int transfer_color(const char* who, void (*pass)(ResampleColorArgs<Record>), float* dst_tsdf, float* dst_weights, uint16_t* dst_color,
                   const int32_t* dst_res, float dst_voxel_size, float dst_truncdist, float max_weight, const emf_absorb_source_t* source,
                   const uint16_t* src_color, const float* R, const float* t, const int32_t* box_lo, const int32_t* box_size,
                   Record* record_dev, emf_color_moved_t* color_record_dev, emf_stream_t stream) {
    ResampleColorArgs<Record> a{};
    unsigned tiles = 0;
    EMF_TRY(rs_check_transfer(who, static_cast<ResampleArgs<Record>*>(&a), &tiles, dst_tsdf, dst_weights, dst_res, dst_voxel_size,
                              dst_truncdist, max_weight, source, R, t, box_lo, box_size, record_dev));
    const size_t nSrc = static_cast<size_t>(a.ns.x) * a.ns.y * a.ns.z;
    const void* others[4] = {source->tsdf, source->weights, source->fgVolMask, source->unseenTiles};
    const size_t otherBytes[4] = {nSrc * sizeof(float), nSrc * sizeof(float), nSrc, emf_hip_unseenTileBytes(source->res)};
    EMF_TRY(rs_check_color(who, &a, dst_color, src_color, color_record_dev, others, otherBytes, 4));
    a.capq = rs_color_cap(max_weight);
    return rs_launch(who, pass, a, tiles, stream);
}

// every check of the release but those of the colour arguments; fills the arguments
int check_release(const char* who, ResampleArgs<emf_release_t>* a, unsigned* tiles, float* dst_tsdf, float* dst_weights,
                  const int32_t* dst_res, float dst_voxel_size, const uint8_t* claim_mask, const int32_t* claim_res, float claim_voxel_size,
                  const float* R, const float* t, const int32_t* box_lo, const int32_t* box_size, emf_release_t* record_dev) {
    EMF_TRY(rs_check_destination(who, dst_tsdf, dst_weights, dst_res, R, t, box_lo, box_size, record_dev));
    if (!claim_res) return fail(EMF_E_ARG, "%s: the claimant's resolution is NULL", who);
    unsigned long long nDst = 0, nClaim = 0;
    EMF_TRY(rs_check_volume(who, dst_res, "destination", &nDst));
    EMF_TRY(rs_check_volume(who, claim_res, "claimant", &nClaim));
    const void* others[1] = {claim_mask};
    const size_t otherBytes[1] = {static_cast<size_t>(nClaim)};
    EMF_TRY(rs_check_layout(who, a, tiles, dst_tsdf, dst_weights, dst_res, nDst, dst_voxel_size, "claimant's mask", claim_res,
                            claim_voxel_size, others, otherBytes, 1, R, t, box_lo, box_size, record_dev));
    a->srcMask = claim_mask;
    return EMF_OK;
}

// mergeVolume and mergeVolumeColor: the source's mask is there; every check of absorbVolume; with colour those of the
// colour arguments, the count arrays among the other arrays of the call; then the count arrays and their record -- there,
// 8-byte aligned, and no array the call writes shares a byte with any other array of the call -- then the launch.
template <bool Color>
int merge_volume(const char* who, void (*pass)(MergeArgs<Color>), float* dst_tsdf, float* dst_weights, float* dst_fgbg, uint16_t* dst_color,
                 const int32_t* dst_res, float dst_voxel_size, float dst_truncdist, float max_weight, const emf_absorb_source_t* source,
                 const float* src_fgbg, const uint16_t* src_color, const float* R, const float* t, const int32_t* box_lo,
                 const int32_t* box_size, emf_absorb_t* record_dev, emf_merge_counts_t* counts_dev, emf_color_moved_t* color_record_dev,
                 emf_stream_t stream) {
    MergeArgs<Color> a{};
    unsigned tiles = 0;
    if (source && !source->fgVolMask)
        return fail(EMF_E_ARG, "%s: the source has no fgVolMask (what the source itself calls background is no evidence)", who);
    EMF_TRY(rs_check_transfer(who, static_cast<ResampleArgs<emf_absorb_t>*>(&a), &tiles, dst_tsdf, dst_weights, dst_res, dst_voxel_size,
                              dst_truncdist, max_weight, source, R, t, box_lo, box_size, record_dev));
    if (!dst_fgbg || !src_fgbg || !counts_dev) return fail(EMF_E_ARG, "%s: a count volume or the count record is NULL", who);
    if ((reinterpret_cast<uintptr_t>(dst_fgbg) | reinterpret_cast<uintptr_t>(src_fgbg) | reinterpret_cast<uintptr_t>(counts_dev)) & 7u)
        return fail(EMF_E_ARG, "%s: a misaligned count volume or count record", who);
    const size_t nDst = static_cast<size_t>(a.nd.x) * a.nd.y * a.nd.z, nSrc = static_cast<size_t>(a.ns.x) * a.ns.y * a.ns.z;
    // the first five are written, the rest only read
    const void* all[11] = {dst_tsdf, dst_weights, record_dev, dst_fgbg, counts_dev, source->tsdf, source->weights, source->fgVolMask,
                           source->unseenTiles, src_fgbg, Color ? src_color : nullptr};
    const size_t allBytes[11] = {nDst * sizeof(float), nDst * sizeof(float), sizeof(emf_absorb_t), nDst * 8u, sizeof(emf_merge_counts_t),
                                 nSrc * sizeof(float), nSrc * sizeof(float), nSrc, emf_hip_unseenTileBytes(source->res), nSrc * 8u,
                                 Color ? nSrc * 8u : 0u};
    for (int w = 0; w < 5; ++w)
        for (int k = w + 1; k < 11; ++k)
            if (all[k] != nullptr && rs_overlap(all[w], allBytes[w], all[k], allBytes[k]))
                return fail(EMF_E_ARG, "%s: an array the call writes overlaps another array of the call", who);
    emf_color_moved_t* colorRecord = nullptr;
    if constexpr (Color) {
        EMF_TRY(rs_check_color(who, &a, dst_color, src_color, color_record_dev, all + 3, allBytes + 3, 7));
        a.capq = rs_color_cap(max_weight);
        colorRecord = color_record_dev;
    }
    a.dstFgbg = reinterpret_cast<float2*>(dst_fgbg), a.srcFgbg = reinterpret_cast<const float2*>(src_fgbg), a.counts = counts_dev;
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_mg_init<Color>, dim3(1), dim3(64), 0, s, a.record, a.nd, a.counts, colorRecord);
    if (tiles != 0u) hipLaunchKernelGGL(pass, dim3(tiles), dim3(kRsBlock), 0, s, a);
    return launch_status(who);
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_absorbVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size, float dst_truncdist,
                         float max_weight, const emf_absorb_source_t* source, const float R[9], const float t[3],
                         const int32_t box_lo[3], const int32_t box_size[3], emf_absorb_t* record_dev, emf_stream_t stream) {
    ResampleArgs<emf_absorb_t> a{};
    unsigned tiles = 0;
    EMF_TRY(rs_check_transfer("absorbVolume", &a, &tiles, dst_tsdf, dst_weights, dst_res, dst_voxel_size, dst_truncdist, max_weight, source,
                              R, t, box_lo, box_size, record_dev));
    return rs_launch("absorbVolume", k_ab_absorb, a, tiles, stream);
}

int emf_hip_absorbVolumeColor(float* dst_tsdf, float* dst_weights, uint16_t* dst_color, const int32_t dst_res[3], float dst_voxel_size,
                              float dst_truncdist, float max_weight, const emf_absorb_source_t* source, const uint16_t* src_color,
                              const float R[9], const float t[3], const int32_t box_lo[3], const int32_t box_size[3],
                              emf_absorb_t* record_dev, emf_color_moved_t* color_record_dev, emf_stream_t stream) {
    return transfer_color("absorbVolumeColor", k_ab_absorb_color, dst_tsdf, dst_weights, dst_color, dst_res, dst_voxel_size, dst_truncdist,
                          max_weight, source, src_color, R, t, box_lo, box_size, record_dev, color_record_dev, stream);
}

int emf_hip_seedVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size, float dst_truncdist,
                       float max_weight, const emf_absorb_source_t* source, const float R[9], const float t[3],
                       const int32_t box_lo[3], const int32_t box_size[3], emf_seed_t* record_dev, emf_stream_t stream) {
    ResampleArgs<emf_seed_t> a{};
    unsigned tiles = 0;
    EMF_TRY(rs_check_transfer("seedVolume", &a, &tiles, dst_tsdf, dst_weights, dst_res, dst_voxel_size, dst_truncdist, max_weight, source, R,
                              t, box_lo, box_size, record_dev));
    return rs_launch("seedVolume", k_lf_seed, a, tiles, stream);
}

int emf_hip_seedVolumeColor(float* dst_tsdf, float* dst_weights, uint16_t* dst_color, const int32_t dst_res[3], float dst_voxel_size,
                            float dst_truncdist, float max_weight, const emf_absorb_source_t* source, const uint16_t* src_color,
                            const float R[9], const float t[3], const int32_t box_lo[3], const int32_t box_size[3],
                            emf_seed_t* record_dev, emf_color_moved_t* color_record_dev, emf_stream_t stream) {
    return transfer_color("seedVolumeColor", k_lf_seed_color, dst_tsdf, dst_weights, dst_color, dst_res, dst_voxel_size, dst_truncdist,
                          max_weight, source, src_color, R, t, box_lo, box_size, record_dev, color_record_dev, stream);
}

int emf_hip_releaseVolume(float* dst_tsdf, float* dst_weights, const int32_t dst_res[3], float dst_voxel_size,
                          const uint8_t* claim_mask, const int32_t claim_res[3], float claim_voxel_size, const float R[9],
                          const float t[3], const int32_t box_lo[3], const int32_t box_size[3], emf_release_t* record_dev,
                          emf_stream_t stream) {
    ResampleArgs<emf_release_t> a{};
    unsigned tiles = 0;
    EMF_TRY(check_release("releaseVolume", &a, &tiles, dst_tsdf, dst_weights, dst_res, dst_voxel_size, claim_mask, claim_res,
                          claim_voxel_size, R, t, box_lo, box_size, record_dev));
    return rs_launch("releaseVolume", k_lf_release<false>, a, tiles, stream);
}

int emf_hip_releaseVolumeColor(float* dst_tsdf, float* dst_weights, uint16_t* dst_color, const int32_t dst_res[3], float dst_voxel_size,
                               const uint8_t* claim_mask, const int32_t claim_res[3], float claim_voxel_size, const float R[9],
                               const float t[3], const int32_t box_lo[3], const int32_t box_size[3], emf_release_t* record_dev,
                               emf_color_moved_t* color_record_dev, emf_stream_t stream) {
    ResampleColorArgs<emf_release_t> a{};
    unsigned tiles = 0;
    EMF_TRY(check_release("releaseVolumeColor", &a, &tiles, dst_tsdf, dst_weights, dst_res, dst_voxel_size, claim_mask, claim_res,
                          claim_voxel_size, R, t, box_lo, box_size, record_dev));
    const void* others[1] = {claim_mask};
    const size_t otherBytes[1] = {static_cast<size_t>(a.ns.x) * a.ns.y * a.ns.z};
    EMF_TRY(rs_check_color("releaseVolumeColor", &a, dst_color, nullptr, color_record_dev, others, otherBytes, 1));
    return rs_launch("releaseVolumeColor", k_lf_release<true>, a, tiles, stream);
}

int emf_hip_mergeVolume(float* dst_tsdf, float* dst_weights, float* dst_fgbg, const int32_t dst_res[3], float dst_voxel_size,
                        float dst_truncdist, float max_weight, const emf_absorb_source_t* source, const float* src_fgbg, const float R[9],
                        const float t[3], const int32_t box_lo[3], const int32_t box_size[3], emf_absorb_t* record_dev,
                        emf_merge_counts_t* counts_dev, emf_stream_t stream) {
    return merge_volume<false>("mergeVolume", k_mg_merge, dst_tsdf, dst_weights, dst_fgbg, nullptr, dst_res, dst_voxel_size, dst_truncdist,
                               max_weight, source, src_fgbg, nullptr, R, t, box_lo, box_size, record_dev, counts_dev, nullptr, stream);
}

int emf_hip_mergeVolumeColor(float* dst_tsdf, float* dst_weights, float* dst_fgbg, uint16_t* dst_color, const int32_t dst_res[3],
                             float dst_voxel_size, float dst_truncdist, float max_weight, const emf_absorb_source_t* source,
                             const float* src_fgbg, const uint16_t* src_color, const float R[9], const float t[3], const int32_t box_lo[3],
                             const int32_t box_size[3], emf_absorb_t* record_dev, emf_merge_counts_t* counts_dev,
                             emf_color_moved_t* color_record_dev, emf_stream_t stream) {
    return merge_volume<true>("mergeVolumeColor", k_mg_merge_color, dst_tsdf, dst_weights, dst_fgbg, dst_color, dst_res, dst_voxel_size,
                              dst_truncdist, max_weight, source, src_fgbg, src_color, R, t, box_lo, box_size, record_dev, counts_dev,
                              color_record_dev, stream);
}

}  // extern "C"
