// view_render.hip -- level-3 ABI: the whole model table seen from a free viewpoint in ONE launch
// (the reference's --3d-vis view, EMFusion.cpp:162-231, ray-cast instead of meshed).
//
// The frame raycast (k_raycast_batched) writes W x H raylengths / vertices / normals / hit mask per model into the
// table's own buffers -- the frame's state, 29 B per pixel per model -- and the composite (k_composite), the hide step
// (k_hide_label) and the shading (k_render_phong) read them back.  A viewer needs none of those images: here one lane
// marches its pixel's ray through every model in table order, keeps the nearest object hit under the composite's rule in
// registers, and shades.  Nothing of the table is written.
//
// Per pixel, exactly the chain
//   raycastBatched (per model, fgVolMask-gated weights)  ->  compositeRaycast (zeroed diff: no history)
//   ->  hideLabel for every label in hideMask  ->  renderPhong
// with the same arithmetic in the same order (-ffp-contract=off like every kernel here): same bits.
// No far bounds, no brick flags (both are the frame camera's); a volume above 32-bit byte offsets is marched with the
// 64-bit per-lane march_ray (k_raycast_batched's MODE 0 does the same), everything else with march_wave.
#include "march_wave.hpp"

namespace emf_hip {
namespace {

constexpr int kViewTile = 16;  // a workgroup = a 16x16-pixel tile, a wave = an 8x8 cell (k_raycast_batched MODE 1)

struct ViewArgs {
    const emf_model_t* models;
    const emf_pose_t* poses;  // viewer -> volume, one per slot
    int nmodels, w, h, tilesX;
    float fx, fy, cx, cy;
    V3 light;
    Img<uint8_t> rgb;  // u8 x 3
    Img<float> ray, vert, nrm;  // data == nullptr: not written
    Img<uint8_t> seg;
    unsigned long long* stats;
    uint32_t hide[8];             // bit s: label s is hidden
    uint8_t ids[EMF_MAX_MODELS];  // seg label of each slot (slot 0, the background: unused)
    uint8_t colors[256 * 3];
};

// k_render_phong's fastpow / to_u8 / shading (EMFusion.cu:100-186), operation for operation
__device__ __forceinline__ float view_fastpow(float base, int exp) {
    float result = 1.f;
    while (exp) {
        if (exp & 1) result *= base;
        base *= base;
        exp >>= 1;
    }
    return result;
}
__device__ __forceinline__ uint8_t view_to_u8(float v) {
    return v >= 0.f ? static_cast<uint8_t>(v < 255.f ? static_cast<int>(v) : 255) : uint8_t{0};
}

// 5 waves per SIMD like k_raycast_batched<1> (its march is the same): 93 VGPRs, none spilled; uncapped the composite
// state carried across the model loop takes the kernel to 98 VGPRs = 4 waves
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_render_view(const ViewArgs a) {
    const int tyy = static_cast<int>(blockIdx.x) / a.tilesX, txx = static_cast<int>(blockIdx.x) - tyy * a.tilesX;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = txx * kViewTile + (wave & 1) * 8 + (lane & 7), y = tyy * kViewTile + (wave >> 1) * 8 + (lane >> 3);
    const bool valid = x < a.w && y < a.h;
    // composite state (k_composite, first chunk: r = 0, no label) and the background's hit
    float r = 0.f, bgRay = 0.f;
    V3 vv = v3(0.f, 0.f, 0.f), nn = v3(0.f, 0.f, 0.f), bgV = v3(0.f, 0.f, 0.f), bgN = v3(0.f, 0.f, 0.f);
    bool bgHit = false;
    unsigned s = 0, samples = 0, hits = 0, gathered = 0;
    for (int m = 0; m < a.nmodels; ++m) {  // (wave-uniform) table order: background, then objects in list order
        const emf_model_t& md = a.models[m];
        const emf_pose_t& p = a.poses[m];
        RayVolume v;
        v.tsdf = md.tsdf;
        v.grads = md.grads;
        v.weights = md.weights;
        v.fg = md.fgVolMask;
        v.bricks = nullptr;
        v.blendFromFlags = false;
        v.R = M33{{p.R[0], p.R[1], p.R[2]}, {p.R[3], p.R[4], p.R[5]}, {p.R[6], p.R[7], p.R[8]}};
        v.cam = v3(p.t[0], p.t[1], p.t[2]);
        v.n = I3{md.res[0], md.res[1], md.res[2]};
        v.voxelSize = md.voxelSize;
        v.truncdist = md.truncdist;
        // usable_reciprocal / fits_offsets32 of the frame launch, decided here because the poses live on the device
        const bool rcpOk = fabsf(p.t[0]) <= 1e15f && fabsf(p.t[1]) <= 1e15f && fabsf(p.t[2]) <= 1e15f;
        v.rcpVoxel = rcpOk ? md.rcpVoxel : 0.f;
        const bool off32 = static_cast<unsigned long long>(v.n.x) * static_cast<unsigned long long>(v.n.y) *
                               static_cast<unsigned long long>(v.n.z) <=
                           (1ull << 30);
        float hr = 0.f;
        V3 hv = v3(0.f, 0.f, 0.f), hn = v3(0.f, 0.f, 0.f);
        bool hit = false;
        if (off32) {
            auto sink = [&](float raylength, const V3& vertex, const V3& normal) {
                hr = raylength;
                hv = vertex;
                hn = normal;
            };
            const MarchCount c = march_wave(v, valid, x, y, a.fx, a.fy, a.cx, a.cy, 0.f, sink);
            hit = c.hit;
            samples += c.samples;
            gathered += c.gathered;
        } else if (valid) {
            const RayHit h = march_ray(v, x, y, a.fx, a.fy, a.cx, a.cy, 0.f);
            hit = h.hit;
            hr = h.raylength;  // zeros where there is no hit
            hv = h.vertex;
            hn = h.normal;
            samples += h.samples;
            gathered += h.gathered;
        }
        hits += hit ? 1u : 0u;
        if (m == 0) {
            bgHit = hit;
            bgRay = hr;
            bgV = hv;
            bgN = hn;
        } else if (hit && (r <= 0 || hr < r)) {  // list order, strict '<' (Q15)
            r = hr;
            vv = hv;
            nn = hn;
            s = a.ids[m];
        }
    }
    add_ray_stats(a.stats, samples, hits, gathered, 0u, lane);
    if (!valid) return;
    // last chunk of k_composite with a zeroed diff buffer: masked subtract, 0 elsewhere
    const float d = bgHit ? r - bgRay : 0.f;
    if (d > 0.05f) s = 0;  // background wins when it is > 5 cm in front
    if (s != 0 && ((a.hide[s >> 5] >> (s & 31u)) & 1u)) s = 0;  // k_hide_label: the label goes, the background shows
    if (s == 0) {  // vertices / normals fall back to the background, the raylength does not
        vv = bgV;
        nn = bgN;
    }
    if (a.ray.data) a.ray.row(y)[x] = r;
    if (a.seg.data) a.seg.row(y)[x] = static_cast<uint8_t>(s);
    if (a.vert.data) {
        float* o = a.vert.row(y) + 3 * x;
        o[0] = vv.x;
        o[1] = vv.y;
        o[2] = vv.z;
    }
    if (a.nrm.data) {
        float* o = a.nrm.row(y) + 3 * x;
        o[0] = nn.x;
        o[1] = nn.y;
        o[2] = nn.z;
    }
    // k_render_phong
    uint8_t* out = a.rgb.row(y) + 3 * x;
    const V3 pt = vv, n = nn;
    if (pt.x == 0.f && pt.y == 0.f && pt.z == 0.f) {
        out[0] = out[1] = out[2] = 0;
        return;
    }
    const uint8_t* c = a.colors + 3 * s;
    const float ka = 0.3f, kd = 0.5f, ks = 0.2f;
    const V3 Rd = v3(static_cast<float>(c[0]) / 255.f, static_cast<float>(c[1]) / 255.f,
                     static_cast<float>(c[2]) / 255.f);
    V3 l = v3(a.light.x - pt.x, a.light.y - pt.y, a.light.z - pt.z);
    l = l / norm(l);
    const V3 vw = v3(-pt.x, -pt.y, -pt.z) / norm(pt);
    const V3 two = n * (2.f * dot(l, n));
    V3 rf = v3(two.x - l.x, two.y - l.y, two.z - l.z);
    rf = rf / norm(rf);
    const float diff = dot(n, l), spec = view_fastpow(dot(rf, vw), 20);
    const V3 I = v3(ka * 1.f + (kd * Rd.x) * diff + (ks * 1.f) * spec, ka * 1.f + (kd * Rd.y) * diff + (ks * 1.f) * spec,
                    ka * 1.f + (kd * Rd.z) * diff + (ks * 1.f) * spec);
    out[0] = view_to_u8(I.x * 255.f);
    out[1] = view_to_u8(I.y * 255.f);
    out[2] = view_to_u8(I.z * 255.f);
}

// an optional output: NULL is "not wanted", anything else must be a valid width x height image
int view_output(const emf_image_t* im, size_t elem, int w, int h, const char* name) {
    if (!im) return EMF_OK;
    EMF_TRY(check_image(im, elem, name));
    if (im->width != w || im->height != h)
        return fail(EMF_E_SHAPE, "%s is %d x %d, the view is %d x %d", name, im->width, im->height, w, h);
    return EMF_OK;
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_renderView(const emf_model_t* models_dev, const emf_pose_t* poseVO_dev, const int32_t* ids_host,
                       int nmodels, int width, int height, const float K[9], const float lightPos[3],
                       const uint8_t colorMap[768], const uint8_t hideMask[32], const emf_image_t* rgb,
                       const emf_image_t* raylengths, const emf_image_t* segmentation, const emf_image_t* vertices,
                       const emf_image_t* normals, uint64_t* stats_dev, emf_stream_t stream) {
    EMF_REQUIRE_PTR(models_dev);
    EMF_REQUIRE_PTR(poseVO_dev);
    if (nmodels < 1 || nmodels > EMF_MAX_MODELS)
        return fail(EMF_E_LIMIT, "renderView: nmodels = %d, expected 1..%d", nmodels, EMF_MAX_MODELS);
    if (nmodels > 1) EMF_REQUIRE_PTR(ids_host);
    EMF_REQUIRE_PTR(K);
    EMF_REQUIRE_PTR(lightPos);
    EMF_REQUIRE_PTR(colorMap);
    EMF_REQUIRE_PTR(rgb);
    if (width <= 0 || height <= 0) return fail(EMF_E_SHAPE, "renderView: bad view size %d x %d", width, height);
    EMF_TRY(view_output(rgb, 3, width, height, "renderView: rgb"));
    EMF_TRY(view_output(raylengths, 4, width, height, "renderView: raylengths"));
    EMF_TRY(view_output(segmentation, 1, width, height, "renderView: segmentation"));
    EMF_TRY(view_output(vertices, 12, width, height, "renderView: vertices"));
    EMF_TRY(view_output(normals, 12, width, height, "renderView: normals"));
    ViewArgs a;
    a.models = models_dev;
    a.poses = poseVO_dev;
    a.nmodels = nmodels;
    a.w = width;
    a.h = height;
    a.tilesX = static_cast<int>(ceil_div(width, kViewTile));
    a.fx = K[0];
    a.fy = K[4];
    a.cx = K[2];
    a.cy = K[5];
    a.light = v3_from(lightPos);
    a.rgb = img<uint8_t>(rgb);
    a.ray = raylengths ? img<float>(raylengths) : Img<float>{nullptr, 0};
    a.seg = segmentation ? img<uint8_t>(segmentation) : Img<uint8_t>{nullptr, 0};
    a.vert = vertices ? img<float>(vertices) : Img<float>{nullptr, 0};
    a.nrm = normals ? img<float>(normals) : Img<float>{nullptr, 0};
    a.stats = reinterpret_cast<unsigned long long*>(stats_dev);
    for (int k = 0; k < 8; ++k)
        a.hide[k] = hideMask ? static_cast<uint32_t>(hideMask[4 * k]) | (static_cast<uint32_t>(hideMask[4 * k + 1]) << 8) |
                                   (static_cast<uint32_t>(hideMask[4 * k + 2]) << 16) |
                                   (static_cast<uint32_t>(hideMask[4 * k + 3]) << 24)
                             : 0u;
    a.ids[0] = 0;
    for (int m = 1; m < nmodels; ++m) {  // saturated like compositeRaycast's id table
        const int id = ids_host[m - 1];
        a.ids[m] = static_cast<uint8_t>(id < 0 ? 0 : (id > 255 ? 255 : id));
    }
    for (int m = nmodels; m < EMF_MAX_MODELS; ++m) a.ids[m] = 0;
    for (int i = 0; i < 768; ++i) a.colors[i] = colorMap[i];
    const unsigned tiles = ceil_div(width, kViewTile) * ceil_div(height, kViewTile);
    hipLaunchKernelGGL(k_render_view, dim3(tiles), dim3(256), 0, as_stream(stream), a);
    return launch_status("renderView");
}

}  // extern "C"
