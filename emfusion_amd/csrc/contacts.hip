// contacts.hip -- object contacts: clearance and penetration between the models of a table, read from their signed-
// distance volumes (include/emf_hip.h "Object contacts").
//
// An ordered pair is (probe a, field b).  Every surface voxel of a is taken through the pair's pose into b's volume and
// b's tsdf is sampled there trilinearly; the pair's record counts what became of the surface voxels and reduces the
// TOUCHING ones to a centroid, a box and a summed normal.
//   k_ct_probe   one workgroup per 32 x 8 x 8 tile of a PROBE (the tile of the unseen-tile map), 256 lanes = 32 along x,
//                8 rows; a lane walks the tile's 8 planes and makes the surface test ONCE per voxel (a solid voxel
//                gathers its six face neighbours behind a branch, as k_shape_moments does), keeping one bit per plane.
//                A wave without a surface voxel leaves.  Then the wave loops over the pairs that name this probe -- the
//                host passes, per probe, the first and the last index of the pair list at which it occurs, so a list
//                grouped by probe is walked without a miss and any other order gives the same bytes -- and each lane
//                samples the field at its surface voxels (rs_source of resample.hpp, the sampler of volume_transfer.hip
//                too): 8 + 8 dependent gathers per voxel inside the field.  The
//                pair and the field's table entry are wave-uniform (scalar loads).  Per pair and wave: wave_reduce
//                of what is not zero anywhere in the wave, then one integer atomic per non-zero quantity from lane
//                0.  A wave in which no lane sampled issues only its outside / unknown / masked counts (and their sum).
//                No LDS, no barrier.  94 to 103 VGPRs depending on how the sampler is spelled: the kernel asks for the
//                5 waves per SIMD it has always had (95 VGPRs, no scratch).
//   k_ct_init / k_ct_finish  one lane per record: the neutral records before the pass, the key of min_s -> f32 bits
//                after it.
// Every float step is one float32 operation: the _rn intrinsics, and every product that feeds a sum goes through an
// identity DPP move (mul_rounded of wave_ops.hpp), so that a build with -ffp-contract=fast has no product left to fuse (DESIGN.md 5.26
// "CONTRACTION").  Integer atomics only: the records do not depend on the order of lanes, waves or workgroups.
#include "resample.hpp"

namespace emf_hip {
namespace {

constexpr unsigned kCtKeyInf = 0xff800000u;  // the key of +inf

static_assert(sizeof(emf_contact_t) == 144 && sizeof(emf_contact_pair_t) == 64, "mirrored by emfusion_amd/_lib.py");
static_assert(EMF_MAX_MODELS <= 256 && EMF_CONTACT_MAX_PAIRS <= 65535, "ContactArgs keeps slots and pair indices in 16 bits");

struct ContactArgs {
    const emf_model_t* models;
    const emf_contact_pair_t* pairs;
    emf_contact_t* records;
    unsigned nModels, nPairs, nProbes;
    unsigned start[EMF_MAX_MODELS + 1];   // probe p: workgroups [start[p], start[p + 1])
    unsigned short slot[EMF_MAX_MODELS];  // probe p: its slot of the table
    unsigned short first[EMF_MAX_MODELS], last[EMF_MAX_MODELS];  // ... and the pairs [first, last] that may name it
};
static_assert(sizeof(ContactArgs) <= 4096, "ContactArgs travels in the kernel arguments");

// the probe whose range [start[p], start[p + 1]) holds x (block-uniform)
__device__ __forceinline__ unsigned probe_of(const unsigned* start, unsigned n, unsigned x) {
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (x >= start[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned ct_float_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ unsigned ct_key_bits(unsigned k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

__device__ __forceinline__ bool ct_finite(float v) { return fabsf(v) < __uint_as_float(0x7f800000u); }  // false for NaN

__global__ __launch_bounds__(kRsBlock) __attribute__((amdgpu_waves_per_eu(5))) void k_ct_probe(const ContactArgs a) {
    const unsigned p = probe_of(a.start, a.nProbes, blockIdx.x);
    const unsigned sa = a.slot[p];
    const emf_model_t& ma = a.models[sa];
    const I3 n{ma.res[0], ma.res[1], ma.res[2]};
    const unsigned ntx = (n.x + kRsTileX - 1) / kRsTileX, nty = (n.y + kRsTileY - 1) / kRsTileY;
    const unsigned b = blockIdx.x - a.start[p];
    if (ma.unseenTiles != nullptr && ma.unseenTiles[b] != 0) return;  // every weight is 0: no solid, no surface voxel
    const unsigned tz = b / (ntx * nty), r = b - tz * ntx * nty, ty = r / ntx, tx = r - ty * ntx;
    const int x = static_cast<int>(tx) * kRsTileX + static_cast<int>(threadIdx.x & 31u);
    const int y = static_cast<int>(ty) * kRsTileY + static_cast<int>(threadIdx.x >> 5);
    const int z0 = static_cast<int>(tz) * kRsTileZ;
    const float* __restrict__ ta = ma.tsdf;
    const float* __restrict__ wa = ma.weights;
    const uint8_t* __restrict__ fa = ma.fgVolMask;
    const size_t sy = static_cast<size_t>(n.x), sz = sy * n.y;

    // the surface test, once per voxel: bit k of surf is plane z0 + k
    unsigned surf = 0u;
    if (x < n.x && y < n.y) {
#pragma unroll
        for (int k = 0; k < kRsTileZ; ++k) {
            const int z = z0 + k;
            if (z >= n.z) break;
            const size_t v = static_cast<size_t>(z) * sz + static_cast<size_t>(y) * sy + x;
            if (!(wa[v] > 0.f) || (fa != nullptr && fa[v] == 0) || ta[v] > 0.f) continue;  // not solid
            bool free = false;
            if (x > 0) free |= wa[v - 1] > 0.f && ta[v - 1] > 0.f;
            if (x + 1 < n.x) free |= wa[v + 1] > 0.f && ta[v + 1] > 0.f;
            if (y > 0) free |= wa[v - sy] > 0.f && ta[v - sy] > 0.f;
            if (y + 1 < n.y) free |= wa[v + sy] > 0.f && ta[v + sy] > 0.f;
            if (z > 0) free |= wa[v - sz] > 0.f && ta[v - sz] > 0.f;
            if (z + 1 < n.z) free |= wa[v + sz] > 0.f && ta[v + sz] > 0.f;
            surf |= (free ? 1u : 0u) << k;
        }
    }
    if (__ballot(surf != 0u) == 0ull) return;  // wave-uniform; the kernel has no barrier

    const unsigned lane = threadIdx.x & 63u;
    const float voxA = ma.voxelSize;
    const float pax = rs_pd(x, n.x, voxA), pay = rs_pd(y, n.y, voxA);

    for (unsigned k = a.first[p]; k <= a.last[p]; ++k) {
        const emf_contact_pair_t& pr = a.pairs[k];  // wave-uniform
        if (static_cast<unsigned>(pr.a) != sa) continue;
        const unsigned sb = static_cast<unsigned>(pr.b);
        if (sb >= a.nModels || sb == sa) continue;  // refused on the host; never followed here
        const emf_model_t& mb = a.models[sb];
        // the field: its unseen-tile map is not consulted, a cell in an unseen tile reads UNKNOWN by its weights
        const RsVolume field = rs_volume(mb.tsdf, mb.weights, mb.fgVolMask, nullptr, I3{mb.res[0], mb.res[1], mb.res[2]});
        const float voxB = mb.voxelSize, touch = pr.touch;
        const RsRows rows = rs_rows(pr.R, pax, pay);

        unsigned cOut = 0u, cUnk = 0u, cMask = 0u, cSam = 0u, cIn = 0u, cTouch = 0u, cNorm = 0u;
        unsigned sx = 0u, sy1 = 0u, sz1 = 0u, key = 0xffffffffu;
        int g0 = 0, g1 = 0, g2 = 0;
        RsBounds touching(n);

        for (unsigned bits = surf; bits != 0u; bits &= bits - 1u) {
            const int z = z0 + (__ffs(bits) - 1);
            float s, w[8];
            switch (rs_source(field, rs_sample(rows, pr.R, pr.t, rs_pd(z, n.z, voxA), voxB, field.half), s, w)) {
                case RsClass::Outside: cOut += 1u; continue;
                case RsClass::Unknown: cUnk += 1u; continue;
                case RsClass::Masked: cMask += 1u; continue;
                case RsClass::Value: break;
            }
            cSam += 1u;
            key = min(key, ct_float_key(s));
            if (s < 0.f) cIn += 1u;
            if (!(s <= touch)) continue;
            cTouch += 1u;
            sx += static_cast<unsigned>(x), sy1 += static_cast<unsigned>(y), sz1 += static_cast<unsigned>(z);
            touching.include(x, y, z);
            if (x > 0 && x + 1 < n.x && y > 0 && y + 1 < n.y && z > 0 && z + 1 < n.z) {
                const size_t v = static_cast<size_t>(z) * sz + static_cast<size_t>(y) * sy + x;
                if (wa[v - 1] > 0.f && wa[v + 1] > 0.f && wa[v - sy] > 0.f && wa[v + sy] > 0.f && wa[v - sz] > 0.f &&
                    wa[v + sz] > 0.f) {
                    const float d0 = __fsub_rn(ta[v + 1], ta[v - 1]), d1 = __fsub_rn(ta[v + sy], ta[v - sy]),
                                d2 = __fsub_rn(ta[v + sz], ta[v - sz]);
                    if (ct_finite(d0) && ct_finite(d1) && ct_finite(d2)) {
                        cNorm += 1u;
                        g0 += __float2int_rn(fminf(fmaxf(__fmul_rn(d0, 4096.f), -8192.f), 8192.f));
                        g1 += __float2int_rn(fminf(fmaxf(__fmul_rn(d1, 4096.f), -8192.f), 8192.f));
                        g2 += __float2int_rn(fminf(fmaxf(__fmul_rn(d2, 4096.f), -8192.f), 8192.f));
                    }
                }
            }
        }

        // a lane holds at most 8 voxels, a wave 512: every wave sum fits 32 bits (512 * 2047, 512 * 8192)
        cOut = wave_reduce<OpAdd>(cOut), cUnk = wave_reduce<OpAdd>(cUnk), cMask = wave_reduce<OpAdd>(cMask);
        const bool anySampled = __ballot(cSam != 0u) != 0ull, anyTouch = touching.any();  // wave-uniform
        if (anySampled) {
            cSam = wave_reduce<OpAdd>(cSam), cIn = wave_reduce<OpAdd>(cIn);
            key = wave_reduce<OpMin>(key);
        }
        if (anyTouch) {
            cTouch = wave_reduce<OpAdd>(cTouch), cNorm = wave_reduce<OpAdd>(cNorm);
            sx = wave_reduce<OpAdd>(sx), sy1 = wave_reduce<OpAdd>(sy1), sz1 = wave_reduce<OpAdd>(sz1);
            g0 = wave_reduce<OpAdd>(g0), g1 = wave_reduce<OpAdd>(g1), g2 = wave_reduce<OpAdd>(g2);
            touching.reduce();
        }
        if (lane == 0u) {
            emf_contact_t* out = a.records + k;
            rs_add64(&out->surface, static_cast<unsigned long long>(cOut) + cUnk + cMask + cSam);  // the wave has a surface voxel
            rs_add64(&out->outside, cOut), rs_add64(&out->unknown, cUnk), rs_add64(&out->masked, cMask);
            if (anySampled) {
                rs_add64(&out->sampled, cSam), rs_add64(&out->inside, cIn);
                atomicMin(reinterpret_cast<unsigned*>(&out->min_s), key);  // a key until k_ct_finish
            }
            if (anyTouch) {
                rs_add64(&out->touching, cTouch), rs_add64(&out->normals, cNorm);
                rs_add64(&out->sum[0], sx), rs_add64(&out->sum[1], sy1), rs_add64(&out->sum[2], sz1);
                // two's complement: the wrap of the unsigned sum is the signed sum
                rs_add64(reinterpret_cast<uint64_t*>(&out->gsum[0]), static_cast<unsigned long long>(static_cast<long long>(g0)));
                rs_add64(reinterpret_cast<uint64_t*>(&out->gsum[1]), static_cast<unsigned long long>(static_cast<long long>(g1)));
                rs_add64(reinterpret_cast<uint64_t*>(&out->gsum[2]), static_cast<unsigned long long>(static_cast<long long>(g2)));
                touching.commit(out);
            }
        }
    }
}

// one lane per record: the neutral records
__global__ __launch_bounds__(256) void k_ct_init(const ContactArgs a) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.nPairs) return;
    const unsigned sa = static_cast<unsigned>(a.pairs[k].a);
    emf_contact_t r{};
    for (int j = 0; j < 3; ++j) {
        r.lo[j] = sa < a.nModels ? a.models[sa].res[j] : 0;
        r.hi[j] = -1;
    }
    r.min_s = __uint_as_float(kCtKeyInf);
    a.records[k] = r;
}

// one lane per record: the key of min_s -> the bits of the float
__global__ __launch_bounds__(256) void k_ct_finish(const ContactArgs a) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.nPairs) return;
    unsigned* m = reinterpret_cast<unsigned*>(&a.records[k].min_s);
    *m = ct_key_bits(*m);
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_contactProbe(const emf_model_t* models_dev, const int32_t* res_host, int32_t n_models,
                         const emf_contact_pair_t* pairs_dev, const emf_contact_pair_t* pairs_host, int32_t n_pairs,
                         emf_contact_t* records_dev, emf_stream_t stream) {
    if (!models_dev || !res_host) return fail(EMF_E_ARG, "contactProbe: the model table or its resolutions are NULL");
    if (!pairs_dev || !pairs_host || !records_dev) return fail(EMF_E_ARG, "contactProbe: the pairs or the records are NULL");
    if (n_models < 1 || n_models > EMF_MAX_MODELS)
        return fail(EMF_E_ARG, "contactProbe: a table of %d models, not 1 .. %d", n_models, EMF_MAX_MODELS);
    if (n_pairs <= 0) return fail(EMF_E_ARG, "contactProbe: %d pairs", n_pairs);
    if (n_pairs > EMF_CONTACT_MAX_PAIRS) return fail(EMF_E_LIMIT, "contactProbe: %d pairs, above %d", n_pairs, EMF_CONTACT_MAX_PAIRS);
    if ((reinterpret_cast<uintptr_t>(models_dev) | reinterpret_cast<uintptr_t>(records_dev)) & 7u)
        return fail(EMF_E_ARG, "contactProbe: a misaligned model table or misaligned records");
    if (reinterpret_cast<uintptr_t>(pairs_dev) & 3u) return fail(EMF_E_ARG, "contactProbe: misaligned pairs");
    ContactArgs a{};
    int probeOf[EMF_MAX_MODELS];
    bool checked[EMF_MAX_MODELS] = {};
    for (int m = 0; m < EMF_MAX_MODELS; ++m) probeOf[m] = -1;
    unsigned long long blocks = 0;
    for (int k = 0; k < n_pairs; ++k) {
        const int32_t pa = pairs_host[k].a, pb = pairs_host[k].b;
        if (pa < 0 || pa >= n_models || pb < 0 || pb >= n_models)
            return fail(EMF_E_ARG, "contactProbe: pair %d names the slots %d and %d of a table of %d", k, pa, pb, n_models);
        if (pa == pb) return fail(EMF_E_ARG, "contactProbe: pair %d probes slot %d against itself", k, pa);
        for (const int32_t m : {pa, pb}) {
            if (checked[m]) continue;
            const int32_t* r = res_host + 3 * m;
            for (int i = 0; i < 3; ++i) {
                if (r[i] < 1) return fail(EMF_E_ARG, "contactProbe: model %d has %d voxels on axis %d", m, r[i], i);
                if (r[i] > EMF_DF_MAX_AXIS)
                    return fail(EMF_E_LIMIT, "contactProbe: model %d has %d voxels on axis %d, above %d", m, r[i], i, EMF_DF_MAX_AXIS);
            }
            const unsigned long long voxels = static_cast<unsigned long long>(r[0]) * r[1] * static_cast<unsigned long long>(r[2]);
            if (voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "contactProbe: model %d has %llu voxels, above 2^31 - 1", m, voxels);
            checked[m] = true;
        }
        int p = probeOf[pa];
        if (p < 0) {
            p = probeOf[pa] = static_cast<int>(a.nProbes++);
            const int32_t* r = res_host + 3 * pa;
            a.slot[p] = static_cast<unsigned short>(pa);
            a.first[p] = static_cast<unsigned short>(k);
            a.start[p] = static_cast<unsigned>(blocks);
            blocks += static_cast<unsigned long long>((r[0] + kRsTileX - 1) / kRsTileX) * ((r[1] + kRsTileY - 1) / kRsTileY) *
                      ((r[2] + kRsTileZ - 1) / kRsTileZ);
            if (blocks > 0xffffffull) return fail(EMF_E_LIMIT, "contactProbe: more than 2^24 - 1 probe tiles in one call");
        }
        a.last[p] = static_cast<unsigned short>(k);
    }
    for (unsigned p = a.nProbes; p <= EMF_MAX_MODELS; ++p) a.start[p] = static_cast<unsigned>(blocks);
    a.models = models_dev;
    a.pairs = pairs_dev;
    a.records = records_dev;
    a.nModels = static_cast<unsigned>(n_models);
    a.nPairs = static_cast<unsigned>(n_pairs);
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ct_init, dim3(ceil_div(a.nPairs, 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_ct_probe, dim3(a.start[a.nProbes]), dim3(kRsBlock), 0, s, a);
    hipLaunchKernelGGL(k_ct_finish, dim3(ceil_div(a.nPairs, 256)), dim3(256), 0, s, a);
    return launch_status("contactProbe");
}

}  // extern "C"
