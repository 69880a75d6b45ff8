// QueryBox.hpp -- the box of the background a scene query works on: the distance field, the
// frontiers and the plan all classify the voxels [lo, lo + size) of the background and map them to world points in
// one way, which is stated here once.
#pragma once

#include "types.hpp"

#include <algorithm>
#include <cmath>

namespace emf {

struct QueryBox {
    Vec3i lo, size;        // voxels of the background, (x, y, z)
    Vec3i bgRes;
    // A box of the world extent may leave the background.  It is described as a box of a VIRTUAL
    // background of bgRes = res + 2 pad voxels at lo = the volume voxel + pad: float(v + pad) - (res + 2 pad - 1) / 2.f
    // equals float(v) - (res - 1) / 2.f exactly -- half-integers far below 2^23 --, in double too, so everything below
    // and every kernel that takes (res, box_lo) gives the same bits as for the real background.  pad is 0 otherwise.
    Vec3i pad = Vec3i(0, 0, 0);
    /** The box's first voxel in voxels of the real background volume: what callers passed and get back. */
    Vec3i volumeLo() const { return Vec3i(lo[0] - pad[0], lo[1] - pad[1], lo[2] - pad[2]); }
    Affine3f bgPose;       // the background's pose the world points go through
    Affine3f boxPose;      // voxel (0, 0, 0) of the box -> world: the background's pose and the box origin, in float
    float voxelSize = 0.f;

    size_t voxels() const { return static_cast<size_t>(size[0]) * size[1] * size[2]; }
    /** The box voxel of a linear index (z * size[1] + y) * size[0] + x. */
    Vec3i unravel(int32_t linear) const {
        const int nx = size[0], ny = size[1];
        return Vec3i(linear % nx, linear / nx % ny, linear / (nx * ny));
    }
    /** A point in box voxels in the world frame: the voxel plus lo - (res - 1) / 2, times the voxel size, through the
     *  background's pose -- in double; what is printed or returned is this value rounded once to float. */
    void worldPoint(const double v[3], double out[3]) const {
        double p[3];
        for (int i = 0; i < 3; ++i)
            p[i] = (v[i] + (static_cast<double>(lo[i]) - (static_cast<double>(bgRes[i]) - 1.0) / 2.0)) * static_cast<double>(voxelSize);
        const float* R = bgPose.rotation().val;
        const float* t = bgPose.translation().val;
        for (int i = 0; i < 3; ++i)
            out[i] = static_cast<double>(R[3 * i]) * p[0] + static_cast<double>(R[3 * i + 1]) * p[1] +
                     static_cast<double>(R[3 * i + 2]) * p[2] + static_cast<double>(t[i]);
    }
    void worldPoint(const Vec3i& v, double out[3]) const {
        const double d[3] = {static_cast<double>(v[0]), static_cast<double>(v[1]), static_cast<double>(v[2])};
        worldPoint(d, out);
    }
    /** The inverse: the box voxel a world point lies in, rint(R^T (world - t) / voxel + (res - 1) / 2) - lo, in double
     *  and not yet cast, so that the caller clamps a point far outside before it becomes an integer. */
    void voxelAt(const float world[3], double out[3]) const {
        const float* R = bgPose.rotation().val;
        const float* t = bgPose.translation().val;
        for (int i = 0; i < 3; ++i) {
            double q = 0.0;
            for (int j = 0; j < 3; ++j) q += static_cast<double>(R[3 * j + i]) * (static_cast<double>(world[j]) - static_cast<double>(t[j]));
            out[i] = std::nearbyint(q / static_cast<double>(voxelSize) + (static_cast<double>(bgRes[i]) - 1.0) / 2.0) -
                     static_cast<double>(lo[i]);
        }
    }
};

/** The padding of the virtual background of a box [lo, lo + size) of a background of `res` voxels: per axis the voxels
 *  by which the box leaves it on either side, 0 for a box inside. */
inline Vec3i queryBoxPad(const Vec3i& lo, const Vec3i& size, const Vec3i& res) {
    Vec3i pad;
    for (int i = 0; i < 3; ++i) {
        const long long over = static_cast<long long>(lo[i]) + size[i] - res[i];
        pad[i] = static_cast<int>(std::max<long long>({0ll, -static_cast<long long>(lo[i]), over}));
    }
    return pad;
}

/** The bounding box [lo, lo + size), in voxels of a background of `res` voxels whose voxel 0 is lattice voxel `origin`,
 *  of that background and the tiles of `tile` voxels at the lattice TILE coordinates `keys` (x, y, z). */
template <class Keys>
inline void tilesExtent(const Keys& keys, const int tile[3], const Vec3i& origin, const Vec3i& res, Vec3i& lo, Vec3i& size) {
    long long a[3] = {0, 0, 0}, b[3] = {res[0], res[1], res[2]};
    for (const auto& key : keys)
        for (int i = 0; i < 3; ++i) {
            const long long first = static_cast<long long>(key[i]) * tile[i] - origin[i];
            a[i] = std::min(a[i], first);
            b[i] = std::max(b[i], first + tile[i]);
        }
    for (int i = 0; i < 3; ++i) {
        lo[i] = static_cast<int>(a[i]);
        size[i] = static_cast<int>(b[i] - a[i]);
    }
}

/** Metres rounded up to whole voxels, at most 4096 and 0 for "none" -- in float, as both apps and the Python layer do. */
inline int metresToVoxels(float metres, float voxel) {
    return metres > 0.f ? static_cast<int>(std::min(std::ceil(metres / voxel), 4096.f)) : 0;
}

}  // namespace emf
