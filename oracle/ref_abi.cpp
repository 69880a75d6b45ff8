/*
 * ref_abi.cpp -- C entry points over the REFERENCE's own kernels, compiled for the host.
 *
 * TEST INFRASTRUCTURE ONLY.  oracle/build_ref.py rewrites the launch syntax of the reference's
 * device sources into ref_launch() calls, writes the result to a temporary directory outside the
 * repository and compiles it together with this file (which includes it) into
 * oracle/_ref/libemf_ref.so.  This file is ours and holds no reference text; every entry point
 * wraps raw host pointers in GpuMat views and calls the reference's own host wrapper, so that the
 * launch geometry and the reinterpretations of Vec3i / Matx33f are the reference's too.
 *
 * Layouts are those of oracle/emf_oracle.h: continuous volumes of (Nz*Ny) rows x Nx cols,
 * res = {Nx, Ny, Nz}; continuous images H x W with interleaved channels; R[9], K[9] row-major.
 *
 * The reference reads masks through PtrStep<bool>.  A byte other than 0 / 1 behind a bool is
 * undefined in C++ (and what nvcc makes of it is not what g++ makes of it), so mask inputs are
 * normalised to 0 / 1 here before the call: "non-zero is true" is the only reading pinned.
 */
#include <cuda_runtime.h>
#include <vector>

thread_local uint3 threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

#include "TSDF_host.inc"
#include "ObjTSDF_host.inc"
#include "EMFusion_host.inc"

using cv::cuda::GpuMat;

namespace {
cv::Matx33f M(const float* p) { cv::Matx33f m; memcpy(m.val, p, sizeof m.val); return m; }
cv::Vec3f V(const float* p) { cv::Vec3f v; memcpy(v.val, p, sizeof v.val); return v; }
cv::Vec3i I(const int* p) { cv::Vec3i v; memcpy(v.val, p, sizeof v.val); return v; }
GpuMat vol(const int* res, int cn, const void* p) {
    return GpuMat(res[1] * res[2], res[0], CV_MAKETYPE(CV_32F, cn), (void*)p);
}
GpuMat img(int w, int h, int type, const void* p) { return GpuMat(h, w, type, (void*)p); }
std::vector<uchar> as_bool(const uchar* p, size_t n) {
    std::vector<uchar> b(n);
    for (size_t i = 0; i < n; ++i) b[i] = p[i] != 0;
    return b;
}
cv::cuda::Stream& S() { return cv::cuda::Stream::Null(); }
GpuMat g_vertices, g_normals, g_triangles; /* result of the last ref_marchingCubes */

/* the overloads the kernels' unqualified calls must reach; checked once at load */
struct SelfCheck {
    SelfCheck() {
        volatile float h = 0.5f, a = 2.5f, b = 3.5f;
        if (abs(h) != 0.5f) abort();                           /* float abs, not int abs */
        if (__float2int_rn(a) != 2 || __float2int_rn(b) != 4) abort(); /* half to even */
        if (__float2int_rn(-a) != -2) abort();
        volatile float n = NAN;
        if (min((float)n, 1.f) != 1.f) abort();                   /* fminf drops the NaN */
        static_assert(sizeof(float3) == 12 && sizeof(int3) == 12 && sizeof(bool) == 1, "layout");
    }
} self_check;
}  // namespace

extern "C" {

int ref_abi_version(void) { return 1; }

void ref_updateTSDF(const float* depth, const float* assoc, int w, int h, float* tsdf, float* wts,
                    const float* R, const float* t, const float* K, const int* res, float vox,
                    float trunc, float maxw) {
    GpuMat T = vol(res, 1, tsdf), W = vol(res, 1, wts);
    emf::cuda::TSDF::updateTSDF(img(w, h, CV_32FC1, depth), img(w, h, CV_32FC1, assoc), T, W, M(R),
                                V(t), M(K), I(res), vox, trunc, maxw, S());
}

/* grads is written only where the kernel writes: pre-zero it (TSDF::updateGradients does) */
void ref_computeTSDFGrads(const float* tsdf, float* grads, const int* res) {
    GpuMat G = vol(res, 3, grads);
    emf::cuda::TSDF::computeTSDFGrads(vol(res, 1, tsdf), G, I(res), S());
}

void ref_raycastTSDF(const float* tsdf, const float* grads, const float* wts, float* ray,
                     float* vert, float* nrm, uchar* mask, int w, int h, const float* R,
                     const float* t, const float* K, const int* res, float vox, float trunc) {
    GpuMat r = img(w, h, CV_32FC1, ray), v = img(w, h, CV_32FC3, vert), n = img(w, h, CV_32FC3, nrm),
           m = img(w, h, CV_8UC1, mask);
    emf::cuda::TSDF::raycastTSDF(vol(res, 1, tsdf), vol(res, 3, grads), vol(res, 1, wts), r, v, n, m,
                                 M(R), V(t), M(K), I(res), vox, trunc, S());
}

void ref_computePoseGradients(const float* gradsVol, const float* points, int w, int h,
                              const float* R, const float* t, const int* res, float vox,
                              float* grads6) {
    GpuMat g(w * h, 6, CV_32FC1, grads6);
    emf::cuda::TSDF::computePoseGradients(vol(res, 3, gradsVol), img(w, h, CV_32FC3, points), M(R),
                                          V(t), I(res), vox, g, S());
}

void ref_getVolumeVals(const float* v, int channels, const float* points, int w, int h,
                       const float* R, const float* t, const int* res, float vox, float* vals) {
    GpuMat o = img(w, h, CV_MAKETYPE(CV_32F, channels), vals);
    emf::cuda::TSDF::getVolumeVals(vol(res, channels, v), img(w, h, CV_32FC3, points), M(R), V(t),
                                   I(res), vox, o, S());
}

/* grads6: n x 6, tsdfVals: n values, As: n x 36, bs: n x 6 */
void ref_computeAb(const float* grads6, const float* tsdfVals, int n, float* As, float* bs) {
    GpuMat A(n, 36, CV_32FC1, As), b(n, 6, CV_32FC1, bs);
    emf::cuda::TSDF::computeAb(GpuMat(n, 6, CV_32FC1, (void*)grads6),
                               GpuMat(1, n, CV_32FC1, (void*)tsdfVals), A, b, S());
}

/* dst (n x cols) = m (n x cols) scaled row-wise by col (n x 1); dst may alias m, as TSDF::reduceAb does */
void ref_multSingletonCol(const float* col, const float* m, int n, int cols, float* dst) {
    GpuMat d(n, cols, CV_32FC1, dst);
    emf::cuda::TSDF::multSingletonCol(GpuMat(n, 1, CV_32FC1, (void*)col),
                                      GpuMat(n, cols, CV_32FC1, (void*)m), d, S());
}

void ref_copyValues(const float* src, float* dst, int channels, const int* offset,
                    const int* srcRes, const int* dstRes) {
    GpuMat d = vol(dstRes, channels, dst);
    emf::cuda::TSDF::copyValues(vol(srcRes, channels, src), d, I(offset), I(srcRes), I(dstRes));
}

/* runs the reference's marchingCubes with scratch buffers shaped and zeroed as TSDF::getMesh does;
 * returns the vertex count, *numTriInts the number of ints in the triangle list (4 per triangle).
 * ref_marchingCubesFetch copies the arrays of the last call. */
int ref_marchingCubes(const float* tsdf, const float* grads, const uchar* mask, const int* res,
                      float vox, int* numTriInts) {
    const int rows = (res[1] - 1) * (res[2] - 1), cols = res[0] - 1;
    GpuMat classes, vidx, tidx;
    createContinuous(rows, cols, CV_8UC1, classes);
    createContinuous(rows, cols, CV_32SC1, vidx);
    createContinuous(rows, cols, CV_32SC1, tidx);
    std::vector<uchar> mb = as_bool(mask, (size_t)res[0] * res[1] * res[2]);
    g_vertices = g_normals = g_triangles = GpuMat();
    emf::cuda::TSDF::marchingCubes(vol(res, 1, tsdf), vol(res, 3, grads),
                                   GpuMat(res[1] * res[2], res[0], CV_8UC1, mb.data()), I(res), vox,
                                   classes, vidx, tidx, g_vertices, g_normals, g_triangles);
    *numTriInts = g_triangles.cols;
    return g_vertices.cols;
}

void ref_marchingCubesFetch(float* vertices, float* normals, int* triangles) {
    if (g_vertices.cols) memcpy(vertices, g_vertices.data, (size_t)g_vertices.cols * 12);
    if (g_normals.cols) memcpy(normals, g_normals.data, (size_t)g_normals.cols * 12);
    if (g_triangles.cols) memcpy(triangles, g_triangles.data, (size_t)g_triangles.cols * 4);
    g_vertices = g_normals = g_triangles = GpuMat();
}

void ref_updateFgBgProbs(const uchar* mask, const uchar* occluded, int w, int h, const float* tsdf,
                         const float* wts, float* fgbg, const float* R, const float* t,
                         const float* K, const int* res, float vox) {
    std::vector<uchar> m = as_bool(mask, (size_t)w * h), o = as_bool(occluded, (size_t)w * h);
    GpuMat f = vol(res, 2, fgbg);
    emf::cuda::ObjTSDF::updateFgBgProbs(img(w, h, CV_8UC1, m.data()), img(w, h, CV_8UC1, o.data()),
                                        vol(res, 1, tsdf), vol(res, 1, wts), f, M(R), V(t), M(K),
                                        I(res), vox, S());
}

void ref_computePoints(const float* depth, float* points, int w, int h, const float* K) {
    GpuMat p = img(w, h, CV_32FC3, points);
    emf::cuda::EMFusion::computePoints(img(w, h, CV_32FC1, depth), p, M(K));
}

/* renderGPU's colour lookup (LUT of 256 x 3 bytes applied to the label replicated to 3 channels)
 * and launch geometry restated here, since they are OpenCV calls; the Phong kernel is the
 * reference's.  image is read-modify-write: pixels without a point keep what the caller put. */
void ref_renderPhong(const float* points, const float* normals, const uchar* seg,
                     const uchar* colorMap, const float* light, int w, int h, uchar* image) {
    std::vector<uchar> colors((size_t)w * h * 3);
    for (size_t i = 0; i < (size_t)w * h; ++i)
        for (int c = 0; c < 3; ++c) colors[3 * i + c] = colorMap[3 * seg[i] + c];
    dim3 threads(32, 32);
    dim3 blocks((w + threads.x - 1) / threads.x, (h + threads.y - 1) / threads.y);
    cv::cuda::PtrStep<float3> p = img(w, h, CV_32FC3, points), n = img(w, h, CV_32FC3, normals);
    cv::cuda::PtrStep<uchar3> c = img(w, h, CV_8UC3, colors.data());
    cv::cuda::PtrStepSz<uchar3> out = img(w, h, CV_8UC3, image);
    ref_launch(blocks, threads, emf::cuda::EMFusion::kernel_renderPhong, p, n, c, out,
               make_float3(light[0], light[1], light[2]));
}

}  // extern "C"
