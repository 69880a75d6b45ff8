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
//                samples the field at its surface voxels: 8 + 8 dependent gathers per voxel inside the field.  The
//                pair and the field's table entry are wave-uniform (scalar loads).  Per pair and wave: wave_reduce
//                of what is not zero anywhere in the wave, then one integer atomic per non-zero quantity from lane
//                0.  A wave in which no lane sampled issues only its outside / unknown / masked counts (and their sum).
//                No LDS, no barrier.
//   k_ct_init / k_ct_finish  one lane per record: the neutral records before the pass, the key of min_s -> f32 bits
//                after it.
// Every float step is one float32 operation: the _rn intrinsics, and every product that feeds a sum goes through an
// identity DPP move (mul_rounded of wave_ops.hpp), so that a build with -ffp-contract=fast has no product left to fuse (DESIGN.md 5.26
// "CONTRACTION").  Integer atomics only: the records do not depend on the order of lanes, waves or workgroups.
#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {
namespace {

constexpr int kCtBlock = 256;
constexpr int kCtTileX = 32, kCtTileY = 8, kCtTileZ = 8;  // the tile of emf_model_t.unseenTiles
constexpr unsigned kCtKeyInf = 0xff800000u;               // the key of +inf

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

__global__ __launch_bounds__(kCtBlock) void k_ct_probe(const ContactArgs a) {
    const unsigned p = probe_of(a.start, a.nProbes, blockIdx.x);
    const unsigned sa = a.slot[p];
    const emf_model_t& ma = a.models[sa];
    const I3 n{ma.res[0], ma.res[1], ma.res[2]};
    const unsigned ntx = (n.x + kCtTileX - 1) / kCtTileX, nty = (n.y + kCtTileY - 1) / kCtTileY;
    const unsigned b = blockIdx.x - a.start[p];
    if (ma.unseenTiles != nullptr && ma.unseenTiles[b] != 0) return;  // every weight is 0: no solid, no surface voxel
    const unsigned tz = b / (ntx * nty), r = b - tz * ntx * nty, ty = r / ntx, tx = r - ty * ntx;
    const int x = static_cast<int>(tx) * kCtTileX + static_cast<int>(threadIdx.x & 31u);
    const int y = static_cast<int>(ty) * kCtTileY + static_cast<int>(threadIdx.x >> 5);
    const int z0 = static_cast<int>(tz) * kCtTileZ;
    const float* __restrict__ ta = ma.tsdf;
    const float* __restrict__ wa = ma.weights;
    const uint8_t* __restrict__ fa = ma.fgVolMask;
    const size_t sy = static_cast<size_t>(n.x), sz = sy * n.y;

    // the surface test, once per voxel: bit k of surf is plane z0 + k
    unsigned surf = 0u;
    if (x < n.x && y < n.y) {
#pragma unroll
        for (int k = 0; k < kCtTileZ; ++k) {
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
    const float pax = __fmul_rn(__fsub_rn(static_cast<float>(x), static_cast<float>(n.x - 1) / 2.f), voxA);
    const float pay = __fmul_rn(__fsub_rn(static_cast<float>(y), static_cast<float>(n.y - 1) / 2.f), voxA);
    const float halfAz = static_cast<float>(n.z - 1) / 2.f;

    for (unsigned k = a.first[p]; k <= a.last[p]; ++k) {
        const emf_contact_pair_t& pr = a.pairs[k];  // wave-uniform
        if (static_cast<unsigned>(pr.a) != sa) continue;
        const unsigned sb = static_cast<unsigned>(pr.b);
        if (sb >= a.nModels || sb == sa) continue;  // refused on the host; never followed here
        const emf_model_t& mb = a.models[sb];
        const I3 nb{mb.res[0], mb.res[1], mb.res[2]};
        const float* __restrict__ tb = mb.tsdf;
        const float* __restrict__ wb = mb.weights;
        const uint8_t* __restrict__ fb = mb.fgVolMask;
        const size_t by = static_cast<size_t>(nb.x), bz = by * nb.y;
        const float voxB = mb.voxelSize, touch = pr.touch;
        const V3 halfB = half_extent(nb);
        const float fnx = static_cast<float>(nb.x), fny = static_cast<float>(nb.y), fnz = static_cast<float>(nb.z);
        // the first two products of every row, summed left to right
        const float r0 = __fadd_rn(mul_rounded(pr.R[0], pax), mul_rounded(pr.R[1], pay));
        const float r1 = __fadd_rn(mul_rounded(pr.R[3], pax), mul_rounded(pr.R[4], pay));
        const float r2 = __fadd_rn(mul_rounded(pr.R[6], pax), mul_rounded(pr.R[7], pay));

        unsigned cOut = 0u, cUnk = 0u, cMask = 0u, cSam = 0u, cIn = 0u, cTouch = 0u, cNorm = 0u;
        unsigned sx = 0u, sy1 = 0u, sz1 = 0u, key = 0xffffffffu;
        int g0 = 0, g1 = 0, g2 = 0;
        int lox = n.x, loy = n.y, loz = n.z, hix = -1, hiy = -1, hiz = -1;

        for (unsigned bits = surf; bits != 0u; bits &= bits - 1u) {
            const int z = z0 + (__ffs(bits) - 1);
            const float paz = __fmul_rn(__fsub_rn(static_cast<float>(z), halfAz), voxA);
            const float pbx = __fadd_rn(__fadd_rn(r0, mul_rounded(pr.R[2], paz)), pr.t[0]);
            const float pby = __fadd_rn(__fadd_rn(r1, mul_rounded(pr.R[5], paz)), pr.t[1]);
            const float pbz = __fadd_rn(__fadd_rn(r2, mul_rounded(pr.R[8], paz)), pr.t[2]);
            const float qx = __fadd_rn(__fdiv_rn(pbx, voxB), halfB.x);
            const float qy = __fadd_rn(__fdiv_rn(pby, voxB), halfB.y);
            const float qz = __fadd_rn(__fdiv_rn(pbz, voxB), halfB.z);
            // the pad-1 rule of outside(), a NaN first: all eight corners of an inside cell lie in the volume
            if (!(qx == qx) || !(qy == qy) || !(qz == qz) || qx < 0.f || __fadd_rn(qx, 1.f) >= fnx || qy < 0.f ||
                __fadd_rn(qy, 1.f) >= fny || qz < 0.f || __fadd_rn(qz, 1.f) >= fnz) {
                cOut += 1u;
                continue;
            }
            const int lx = static_cast<int>(qx), ly = static_cast<int>(qy), lz = static_cast<int>(qz);
            const float fx = __fsub_rn(qx, static_cast<float>(lx)), fy = __fsub_rn(qy, static_cast<float>(ly)),
                        fz = __fsub_rn(qz, static_cast<float>(lz));
            const size_t c = (static_cast<size_t>(lz) * nb.y + ly) * by + lx;
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
            if (fb != nullptr) {  // the voxel nearest to q, ties to even: inside the volume by the rule above
                const int rx = __float2int_rn(qx), ry = __float2int_rn(qy), rz = __float2int_rn(qz);
                if (fb[(static_cast<size_t>(rz) * nb.y + ry) * by + rx] == 0) {
                    cMask += 1u;
                    continue;
                }
            }
            cSam += 1u;
            key = min(key, ct_float_key(s));
            if (s < 0.f) cIn += 1u;
            if (!(s <= touch)) continue;
            cTouch += 1u;
            sx += static_cast<unsigned>(x), sy1 += static_cast<unsigned>(y), sz1 += static_cast<unsigned>(z);
            lox = min(lox, x), hix = max(hix, x);
            loy = min(loy, y), hiy = max(hiy, y);
            loz = min(loz, z), hiz = max(hiz, z);
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
        const bool anySampled = __ballot(cSam != 0u) != 0ull, anyTouch = __ballot(cTouch != 0u) != 0ull;  // wave-uniform
        if (anySampled) {
            cSam = wave_reduce<OpAdd>(cSam), cIn = wave_reduce<OpAdd>(cIn);
            key = wave_reduce<OpMin>(key);
        }
        if (anyTouch) {
            cTouch = wave_reduce<OpAdd>(cTouch), cNorm = wave_reduce<OpAdd>(cNorm);
            sx = wave_reduce<OpAdd>(sx), sy1 = wave_reduce<OpAdd>(sy1), sz1 = wave_reduce<OpAdd>(sz1);
            g0 = wave_reduce<OpAdd>(g0), g1 = wave_reduce<OpAdd>(g1), g2 = wave_reduce<OpAdd>(g2);
            lox = wave_reduce<OpMin>(lox), loy = wave_reduce<OpMin>(loy), loz = wave_reduce<OpMin>(loz);
            hix = wave_reduce<OpMax>(hix), hiy = wave_reduce<OpMax>(hiy), hiz = wave_reduce<OpMax>(hiz);
        }
        if (lane == 0u) {
            emf_contact_t* out = a.records + k;
            auto add = [](uint64_t* q, unsigned long long v) {
                if (v) atomicAdd(reinterpret_cast<unsigned long long*>(q), v);
            };
            add(&out->surface, static_cast<unsigned long long>(cOut) + cUnk + cMask + cSam);  // the wave has a surface voxel
            add(&out->outside, cOut), add(&out->unknown, cUnk), add(&out->masked, cMask);
            if (anySampled) {
                add(&out->sampled, cSam), add(&out->inside, cIn);
                atomicMin(reinterpret_cast<unsigned*>(&out->min_s), key);  // a key until k_ct_finish
            }
            if (anyTouch) {
                add(&out->touching, cTouch), add(&out->normals, cNorm);
                add(&out->sum[0], sx), add(&out->sum[1], sy1), add(&out->sum[2], sz1);
                // two's complement: the wrap of the unsigned sum is the signed sum
                add(reinterpret_cast<uint64_t*>(&out->gsum[0]), static_cast<unsigned long long>(static_cast<long long>(g0)));
                add(reinterpret_cast<uint64_t*>(&out->gsum[1]), static_cast<unsigned long long>(static_cast<long long>(g1)));
                add(reinterpret_cast<uint64_t*>(&out->gsum[2]), static_cast<unsigned long long>(static_cast<long long>(g2)));
                atomicMin(&out->lo[0], lox), atomicMin(&out->lo[1], loy), atomicMin(&out->lo[2], loz);
                atomicMax(&out->hi[0], hix), atomicMax(&out->hi[1], hiy), atomicMax(&out->hi[2], hiz);
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
            blocks += static_cast<unsigned long long>((r[0] + kCtTileX - 1) / kCtTileX) * ((r[1] + kCtTileY - 1) / kCtTileY) *
                      ((r[2] + kCtTileZ - 1) / kCtTileZ);
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
    hipLaunchKernelGGL(k_ct_probe, dim3(a.start[a.nProbes]), dim3(kCtBlock), 0, s, a);
    hipLaunchKernelGGL(k_ct_finish, dim3(ceil_div(a.nPairs, 256)), dim3(256), 0, s, a);
    return launch_status("contactProbe");
}

}  // extern "C"
