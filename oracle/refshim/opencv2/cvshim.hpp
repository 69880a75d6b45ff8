/*
 * Stand-in for the four OpenCV headers the reference's common header names: cv::cuda::GpuMat and
 * the PtrStep views over HOST memory, the small fixed-size types, and the handful of functions the
 * exported entry points call.  TEST INFRASTRUCTURE ONLY; our own text, nothing of OpenCV's.
 *
 * Things that silently change results: PtrStep::ptr(y) steps in BYTES; setTo(Scalar::all(0)) fills
 * with zero bytes (any other value aborts); reshape keeps the bytes and recomputes cols/step;
 * sum() accumulates in double like OpenCV; createContinuous() gives zeroed memory.
 */
#pragma once
#include <cuda_runtime.h>
#include <memory>
typedef unsigned char uchar;
#define CV_8U 0
#define CV_32S 4
#define CV_32F 5
#define CV_MAKETYPE(depth, cn) ((depth) + (((cn) - 1) << 3))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_32SC1 CV_MAKETYPE(CV_32S, 1)
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_32FC3 CV_MAKETYPE(CV_32F, 3)
#define CV_Assert(x) do { if (!(x)) abort(); } while (0)
namespace cv {
struct Matx33f { float val[9]; };
struct Vec3f { float val[3]; };
struct Vec3i { int val[3]; };
struct Mat {};      /* named by declarations of functions this build does not export */
struct Affine3f {};
struct Scalar {
    double v[4];
    static Scalar all(double d) { return {{d, d, d, d}}; }
    double operator[](int i) const { return v[i]; }
};
template <class T> struct DataType;
template <> struct DataType<float> { static const int depth = CV_32F; };
template <> struct DataType<int> { static const int depth = CV_32S; };
template <> struct DataType<uchar> { static const int depth = CV_8U; };
template <> struct DataType<bool> { static const int depth = CV_8U; };
namespace cuda {
struct Stream { static Stream& Null() { static Stream s; return s; } };
struct StreamAccessor { static cudaStream_t getStream(const Stream&) { return nullptr; } };
template <class T> struct PtrStep {
    T* data;
    size_t step; /* bytes */
    T* ptr(int y = 0) const { return (T*)((char*)data + (size_t)y * step); }
    T& operator()(int y, int x) const { return ptr(y)[x]; }
};
template <class T> struct PtrStepSz : PtrStep<T> { int rows, cols; };
inline size_t ref_elem1(int depth) { return depth == CV_8U ? 1 : 4; }
struct GpuMat {
    int rows = 0, cols = 0, dep = CV_32F, cn = 1;
    size_t step = 0;
    uchar* data = nullptr;
    std::shared_ptr<uchar> own;
    GpuMat() {}
    /* view of caller-owned, continuous memory */
    GpuMat(int r, int c, int type, void* p)
        : rows(r), cols(c), dep(type & 7), cn((type >> 3) + 1),
          step((size_t)c * ((type >> 3) + 1) * ref_elem1(type & 7)), data((uchar*)p) {}
    int depth() const { return dep; }
    int channels() const { return cn; }
    int type() const { return CV_MAKETYPE(dep, cn); }
    bool empty() const { return data == nullptr; }
    template <class T> T* ptr(int y = 0) const { return (T*)(data + (size_t)y * step); }
    template <class T> operator PtrStepSz<T>() const {
        PtrStepSz<T> p;
        p.data = (T*)data; p.step = step; p.rows = rows; p.cols = cols;
        return p;
    }
    template <class T> operator PtrStep<T>() const { return PtrStep<T>{(T*)data, step}; }
    void setTo(const Scalar& s) {
        if (s.v[0] != 0 || s.v[1] != 0 || s.v[2] != 0 || s.v[3] != 0) abort();
        for (int y = 0; y < rows; ++y) memset(data + (size_t)y * step, 0, (size_t)cols * cn * ref_elem1(dep));
    }
    void setTo(const Scalar& s, Stream&) { setTo(s); }
    /* both forms need continuous memory, which is all this build ever makes */
    GpuMat reshape(int ncn, int nrows = 0) const {
        if (step != (size_t)cols * cn * ref_elem1(dep)) abort();
        GpuMat m = *this;
        const long total = (long)rows * cols * cn;
        m.cn = ncn;
        m.rows = nrows ? nrows : rows;
        if (total % ((long)ncn * m.rows)) abort();
        m.cols = (int)(total / ((long)ncn * m.rows));
        m.step = (size_t)m.cols * ncn * ref_elem1(dep);
        return m;
    }
};
inline void createContinuous(int rows, int cols, int type, GpuMat& m) {
    const size_t bytes = (size_t)rows * cols * ((type >> 3) + 1) * ref_elem1(type & 7);
    uchar* p = (uchar*)calloc(bytes ? bytes : 1, 1);
    m = GpuMat(rows, cols, type, p);
    m.own = std::shared_ptr<uchar>(p, free);
}
inline Scalar sum(const GpuMat& m) {
    Scalar s = Scalar::all(0);
    for (int y = 0; y < m.rows; ++y)
        for (int x = 0; x < m.cols; ++x)
            for (int c = 0; c < m.cn && c < 4; ++c) {
                const size_t i = (size_t)x * m.cn + c;
                s.v[c] += m.dep == CV_32S ? (double)m.ptr<int>(y)[i]
                        : m.dep == CV_32F ? (double)m.ptr<float>(y)[i] : (double)m.ptr<uchar>(y)[i];
            }
    return s;
}
}  // namespace cuda
}  // namespace cv
