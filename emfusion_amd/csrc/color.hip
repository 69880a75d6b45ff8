// color.hip -- per-voxel colour: the RGB frame fused into a colour volume beside each TSDF volume.
//
// The reference hands its RGB frames to Mask R-CNN only; this is new behaviour, defined in
// include/emf_hip.h (emf_hip_integrateColorBatched) and pinned to tests/color_reference.py.  A colour
// volume holds u16 x 4 per voxel, (R, G, B, Wc) in 8.8 fixed point, in the voxel order of the tsdf.
//
// Which voxels a frame colours is decided by the TSDF integration's own device functions
// (device_core.hpp: shoot_voxel, classify_shot): the same projection, rounded pixel, depth gate and
// band decision, so the coloured shell is exactly the set of voxels the integration fuses with the
// pixel's association weight, minus sdf == -truncdist.  Only those voxels touch colour memory: one
// 8-byte load and one 8-byte store each; everything else of a tile costs arithmetic and the depth gather.
#include "device_core.hpp"

namespace emf_hip {
namespace {

struct ColorPoseTable {
    emf_pose_t p[EMF_MAX_BATCH];
};

struct ColorBatchArgs {
    const emf_model_t* models;
    uint16_t* const* colors;  // device array: colour volume of model m, or nullptr (model skipped)
    ColorPoseTable poses;     // volume -> camera
    int nmodels;
    int tileStart[EMF_MAX_BATCH + 1];  // prefix sum of 32 x 8 x 8 tiles per model
    const int32_t* visible;
    unsigned long long* stats;
    Img<const float> depth, invLambda;
    Img<const uint8_t> rgb;
    int w, h;
    M33 K;
    bool pinhole;
};

// One channel of the running average, IEEE *, +, / in the order written (no contraction, also in the
// library flavour that is built with contraction on).
__device__ __forceinline__ uint16_t blend_channel(float W, uint16_t cq, float aw, float c) {
#pragma clang fp contract(off)
    const float cOld = static_cast<float>(cq) / 256.f;
    const float num = W * cOld + aw * c;
    const float v = (num / (W + aw)) * 256.f;
    return static_cast<uint16_t>(lrintf(v));
}
__device__ __forceinline__ uint16_t blend_weight(float W, float aw, float maxWeight) {
#pragma clang fp contract(off)
    return static_cast<uint16_t>(lrintf(fminf(W + aw, maxWeight) * 256.f));
}

// Every voxel of the tile lies behind the camera plane (p_cam.z <= 0: not visited).  The camera z is
// linear in the voxel index, so it is bounded by the 8 corners; the margin (1 mm against a float error
// of micrometres at these coordinates) makes the vote hold for the rounded interior values too.
__device__ __forceinline__ bool tile_behind_camera(const IntegrateGeom& a, const V3& half, int x0, int y0, int z0) {
    const int x1 = min(x0 + kTileX, a.n.x) - 1, y1 = min(y0 + kTileY, a.n.y) - 1, z1 = min(z0 + kTileZ, a.n.z) - 1;
    const int k = threadIdx.x & 7;
    const V3 p = voxel_in_camera(a, half, (k & 1) ? x1 : x0, (k & 2) ? y1 : y0, (k & 4) ? z1 : z0);
    return __all(p.z < -1e-3f);
}

// One workgroup per 32 x 8 x 8 tile, lanes along x: a wave covers two 32-voxel rows (2 x 256 contiguous
// bytes of colour), eight z slices in turn.
__global__ __launch_bounds__(256) void k_integrate_color_batched(const ColorBatchArgs a) {
    int m = 0;
    while (m + 1 < a.nmodels && static_cast<int>(blockIdx.x) >= a.tileStart[m + 1]) ++m;
    if (a.visible && a.visible[m] == 0) return;  // the gate of the TSDF update, decided on the device
    uint16_t* const color = a.colors[m];
    if (!color) return;
    const emf_model_t& md = a.models[m];
    IntegrateGeom g;
    g.depth = a.depth;
    g.invLambda = a.invLambda;
    g.assoc = Img<const float>{md.assoc, static_cast<size_t>(a.w) * sizeof(float)};
    g.w = a.w;
    g.h = a.h;
    g.R = M33{{a.poses.p[m].R[0], a.poses.p[m].R[1], a.poses.p[m].R[2]},
              {a.poses.p[m].R[3], a.poses.p[m].R[4], a.poses.p[m].R[5]},
              {a.poses.p[m].R[6], a.poses.p[m].R[7], a.poses.p[m].R[8]}};
    g.t = V3{a.poses.p[m].t[0], a.poses.p[m].t[1], a.poses.p[m].t[2]};
    g.K = a.K;
    g.pinhole = a.pinhole;
    g.n = I3{md.res[0], md.res[1], md.res[2]};
    g.voxelSize = md.voxelSize;
    g.truncdist = md.truncdist;
    g.maxWeight = md.maxWeight;
    const int b = blockIdx.x - a.tileStart[m];
    const int ntx = (g.n.x + kTileX - 1) / kTileX, nty = (g.n.y + kTileY - 1) / kTileY;
    const int x0 = (b % ntx) * kTileX, y0 = ((b / ntx) % nty) * kTileY, z0 = (b / (ntx * nty)) * kTileZ;
    const V3 half = half_extent(g.n);
    // block-uniform, exact: no voxel of such a tile is visited
    if (tile_culled(g, half, x0, y0, z0) || tile_behind_camera(g, half, x0, y0, z0)) return;
    const int x = x0 + (threadIdx.x & 31), y = y0 + ((threadIdx.x >> 5) & 7);
    // lanes beyond the volume in a tail tile stay in the wave (they take part in the count's shuffles below)
    const bool live = x < g.n.x && y < g.n.y;
    unsigned coloured = 0;
#pragma unroll 2
    for (int dz = 0; dz < kTileZ; ++dz) {
        const int z = z0 + dz;
        if (!live || z >= g.n.z) break;
        const VoxelShot s = shoot_voxel(g, half, x, y, z);
        if (!s.inImage) continue;
        const float d = g.depth.row(s.py)[s.px];
        if (!(d > 0.f)) continue;  // TSDF.cu:367 `d <= 0` leaves; so does a NaN here as there (band test false)
        const float il = g.invLambda.data ? g.invLambda.row(s.py)[s.px] : inv_lambda_at(g.K, s.px, s.py);
        float samp = 0.f;
        bool band = false;
        const int kind = classify_shot(g, s, d, il, samp, band);
        // band: -truncdist <= sdf < truncdist; the sample is exactly -1 only for sdf == -truncdist
        // (|sdf| < truncdist divides to at most 1 - 2^-24), which |sdf| < truncdist excludes
        if (kind != kFuse || !band || !(samp > -1.f)) continue;
        const float aw = g.assoc.row(s.py)[s.px];
        if (!(aw > 0.f)) continue;
        const uint8_t* px = a.rgb.row(s.py) + 3 * s.px;
        const float r = static_cast<float>(px[0]), gg = static_cast<float>(px[1]), bb = static_cast<float>(px[2]);
        ushort4* cell = reinterpret_cast<ushort4*>(color) + ((static_cast<size_t>(z) * g.n.y + y) * g.n.x + x);
        ushort4 c = *cell;
        const float W = static_cast<float>(c.w) / 256.f;  // read once, before any channel is written
        c.x = blend_channel(W, c.x, aw, r);
        c.y = blend_channel(W, c.y, aw, gg);
        c.z = blend_channel(W, c.z, aw, bb);
        c.w = blend_weight(W, aw, g.maxWeight);
        *cell = c;
        ++coloured;
    }
    if (a.stats) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) coloured += __shfl_xor(coloured, o);
        if ((threadIdx.x & 63) == 0 && coloured) atomicAdd(a.stats, static_cast<unsigned long long>(coloured));
    }
}

// ---- colour of the voxel under every pixel of a view (emf_hip_sampleColor) ---------------------------------------
struct SampleColorArgs {
    const emf_model_t* models;
    uint16_t* const* colors;  // device array parallel to the table, or nullptr: label colours only
    const emf_pose_t* poses;  // device: viewer -> volume per slot (emf_hip_renderView's)
    Img<const float> vertices;
    Img<const uint8_t> seg;
    Img<uint8_t> out;  // u8 x 3
    int w, h, nmodels;
    uint8_t slotOf[256];      // label -> table slot (255: no model carries the label)
    uint8_t colorMap[256 * 3];
};

__global__ __launch_bounds__(256) void k_sample_color(const SampleColorArgs a) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= a.w || y >= a.h) return;
    const float* pp = a.vertices.row(y) + 3 * x;
    const V3 p = v3(pp[0], pp[1], pp[2]);
    uint8_t* out = a.out.row(y) + 3 * x;
    if (p.x == 0.f && p.y == 0.f && p.z == 0.f) {  // no hit: the shading writes black whatever stands here
        out[0] = out[1] = out[2] = 0;
        return;
    }
    const unsigned label = a.seg.row(y)[x];
    uint8_t c[3] = {a.colorMap[3 * label], a.colorMap[3 * label + 1], a.colorMap[3 * label + 2]};
    const int m = a.slotOf[label];
    const ushort4* vol = (a.colors && m < a.nmodels) ? reinterpret_cast<const ushort4*>(a.colors[m]) : nullptr;
    if (vol) {
        const emf_model_t& md = a.models[m];
        const emf_pose_t& po = a.poses[m];
        const I3 n = I3{md.res[0], md.res[1], md.res[2]};
        const M33 R = M33{{po.R[0], po.R[1], po.R[2]}, {po.R[3], po.R[4], po.R[5]}, {po.R[6], po.R[7], po.R[8]}};
        const V3 q = to_voxel(mul(R, p) + V3{po.t[0], po.t[1], po.t[2]}, md.voxelSize, half_extent(n));
        const float fx = rintf(q.x), fy = rintf(q.y), fz = rintf(q.z);  // the nearest voxel, no interpolation
        if (fx >= 0.f && fx < static_cast<float>(n.x) && fy >= 0.f && fy < static_cast<float>(n.y) && fz >= 0.f &&
            fz < static_cast<float>(n.z)) {
            const ushort4 v = vol[(static_cast<size_t>(fz) * n.y + static_cast<size_t>(fy)) * n.x + static_cast<size_t>(fx)];
            if (v.w != 0) {  // coloured: 8.8 fixed point -> the nearest level
                c[0] = static_cast<uint8_t>(min((v.x + 128u) >> 8, 255u));
                c[1] = static_cast<uint8_t>(min((v.y + 128u) >> 8, 255u));
                c[2] = static_cast<uint8_t>(min((v.z + 128u) >> 8, 255u));
            }
        }
    }
    out[0] = c[0];
    out[1] = c[1];
    out[2] = c[2];
}

// the u16 x 4 sibling of k_copy_values (lifecycle.hip): dst(v) = src(v + off) inside the source, else 0
struct ColorCopyArgs {
    const ushort4* src;
    ushort4* dst;
    I3 off, srcRes, dstRes;
};

__global__ __launch_bounds__(256) void k_copy_color_values(const ColorCopyArgs a) {
    const size_t total = static_cast<size_t>(a.dstRes.x) * a.dstRes.y * a.dstRes.z;
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = static_cast<int>(i % a.dstRes.x);
    const size_t r = i / a.dstRes.x;
    const int y = static_cast<int>(r % a.dstRes.y), z = static_cast<int>(r / a.dstRes.y);
    const int sx = x + a.off.x, sy = y + a.off.y, sz = z + a.off.z;
    const bool in = sx >= 0 && sx < a.srcRes.x && sy >= 0 && sy < a.srcRes.y && sz >= 0 && sz < a.srcRes.z;
    ushort4 v = make_ushort4(0, 0, 0, 0);
    if (in) v = a.src[(static_cast<size_t>(sz) * a.srcRes.y + sy) * a.srcRes.x + sx];
    a.dst[i] = v;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_integrateColorBatched(const emf_model_t* models_dev, uint16_t* const* colors_dev,
                                  const emf_pose_t* poseOC_host, const int32_t* res_host, int nmodels,
                                  const int32_t* visible_dev, const emf_image_t* depth, const emf_image_t* invLambda,
                                  const emf_image_t* rgb, const float K[9], uint64_t* stats, emf_stream_t stream) {
    if (!models_dev) return fail(EMF_E_NULL, "integrateColorBatched: models_dev is NULL");
    EMF_REQUIRE_PTR(colors_dev);
    EMF_REQUIRE_PTR(poseOC_host);
    EMF_REQUIRE_PTR(res_host);
    EMF_REQUIRE_PTR(K);
    if (nmodels < 1 || nmodels > EMF_MAX_BATCH)
        return fail(EMF_E_LIMIT, "integrateColorBatched: nmodels = %d, expected 1..%d", nmodels, EMF_MAX_BATCH);
    EMF_TRY(check_image(depth, 4, "integrateColorBatched: depth"));
    EMF_TRY(check_image(rgb, 3, "integrateColorBatched: rgb"));
    EMF_TRY(check_same_size(depth, rgb, "depth", "rgb"));
    if (invLambda) {
        EMF_TRY(check_image(invLambda, 4, "integrateColorBatched: invLambda"));
        EMF_TRY(check_same_size(depth, invLambda, "depth", "invLambda"));
    }
    ColorBatchArgs a;
    a.models = models_dev;
    a.colors = colors_dev;
    a.nmodels = nmodels;
    a.tileStart[0] = 0;
    for (int m = 0; m < nmodels; ++m) {
        const int32_t* r = res_host + 3 * m;
        EMF_TRY(check_res(r));
        a.poses.p[m] = poseOC_host[m];
        const size_t tiles = static_cast<size_t>(ceil_div(r[0], kTileX)) * ceil_div(r[1], kTileY) * ceil_div(r[2], kTileZ);
        if (tiles > size_t(0x7fffffff) - a.tileStart[m])
            return fail(EMF_E_LIMIT, "integrateColorBatched: too many tiles for one launch at model %d", m);
        a.tileStart[m + 1] = a.tileStart[m] + static_cast<int>(tiles);
    }
    a.visible = visible_dev;
    a.stats = reinterpret_cast<unsigned long long*>(stats);
    a.depth = img<const float>(depth);
    a.invLambda = invLambda ? img<const float>(invLambda) : Img<const float>{nullptr, 0};
    a.rgb = img<const uint8_t>(rgb);
    a.w = depth->width;
    a.h = depth->height;
    a.K = m33_from(K);
    a.pinhole = is_pinhole(a.K);
    hipLaunchKernelGGL(k_integrate_color_batched, dim3(static_cast<unsigned>(a.tileStart[nmodels])), dim3(256), 0,
                       as_stream(stream), a);
    return launch_status("integrateColorBatched");
}

int emf_hip_sampleColor(const emf_model_t* models_dev, uint16_t* const* colors_dev, const emf_pose_t* poseVO_dev,
                        const int32_t* ids_host, int nmodels, const emf_image_t* vertices, const emf_image_t* segmentation,
                        const uint8_t colorMap[768], const emf_image_t* colors, emf_stream_t stream) {
    if (!models_dev) return fail(EMF_E_NULL, "sampleColor: models_dev is NULL");
    EMF_REQUIRE_PTR(poseVO_dev);
    EMF_REQUIRE_PTR(colorMap);
    if (nmodels < 1 || nmodels > EMF_MAX_MODELS)
        return fail(EMF_E_LIMIT, "sampleColor: nmodels = %d, expected 1..%d", nmodels, EMF_MAX_MODELS);
    if (nmodels > 1) EMF_REQUIRE_PTR(ids_host);
    EMF_TRY(check_image(vertices, 12, "sampleColor: vertices"));
    EMF_TRY(check_image(segmentation, 1, "sampleColor: segmentation"));
    EMF_TRY(check_image(colors, 3, "sampleColor: colors"));
    EMF_TRY(check_same_size(vertices, segmentation, "vertices", "segmentation"));
    EMF_TRY(check_same_size(vertices, colors, "vertices", "colors"));
    SampleColorArgs a;
    a.models = models_dev;
    a.colors = colors_dev;
    a.poses = poseVO_dev;
    a.vertices = img<const float>(vertices);
    a.seg = img<const uint8_t>(segmentation);
    a.out = img<uint8_t>(colors);
    a.w = vertices->width;
    a.h = vertices->height;
    a.nmodels = nmodels;
    std::memset(a.slotOf, 255, sizeof(a.slotOf));
    a.slotOf[0] = 0;
    // labels are the ids saturated to u8, as the composite writes them; the first slot that carries a label keeps it
    for (int s = nmodels - 1; s >= 1; --s) {
        const int32_t id = ids_host[s - 1];
        if (id >= 1 && s <= 254) a.slotOf[id > 255 ? 255 : id] = static_cast<uint8_t>(s);
    }
    std::memcpy(a.colorMap, colorMap, sizeof(a.colorMap));
    hipLaunchKernelGGL(k_sample_color, dim3(static_cast<unsigned>(ceil_div(a.w, 32)), static_cast<unsigned>(ceil_div(a.h, 8))),
                       dim3(256), 0, as_stream(stream), a);
    return launch_status("sampleColor");
}

int emf_hip_copyColorValues(const uint16_t* src, uint16_t* dst, const int32_t offset[3], const int32_t srcRes[3],
                            const int32_t dstRes[3], emf_stream_t stream) {
    EMF_REQUIRE_PTR(src);
    EMF_REQUIRE_PTR(dst);
    EMF_REQUIRE_PTR(offset);
    EMF_TRY(check_res(srcRes));
    EMF_TRY(check_res(dstRes));
    ColorCopyArgs a{reinterpret_cast<const ushort4*>(src), reinterpret_cast<ushort4*>(dst), i3_from(offset),
                    i3_from(srcRes), i3_from(dstRes)};
    const size_t total = static_cast<size_t>(dstRes[0]) * dstRes[1] * dstRes[2];
    hipLaunchKernelGGL(k_copy_color_values, dim3(static_cast<unsigned>(ceil_div(total, size_t(256)))), dim3(256), 0,
                       as_stream(stream), a);
    return launch_status("copyColorValues");
}

}  // extern "C"
