// EMFusionShape.cpp -- emf::EMFusion: object shapes (new behaviour).  Where in its volume a model is,
// how large it is, how it is oriented and how much of its surface has been seen: the integer moments of the OBSERVED
// SOLID BAND of every asked model in one launch (emf_hip_shapeMoments), the frames from them on the host, the extents
// along those frames in a second launch (emf_hip_shapeExtents), the boxes on the host again.  What is measured is the
// band a TSDF observes around the surface, not the body: no volume in cubic metres comes out of this file.
// shapeFrame and shapeBox are float64 in the fixed operation order of include/emf_hip.h "Object shapes" and need no
// device.  This unit is compiled with a*b+c contraction off.
#include "EMFusion.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace emf {

namespace {

// one Jacobi rotation of the pair (p, q), r the third index
void rotate(double S[3][3], double V[3][3], int p, int q) {
    const double apq = S[p][q];
    if (apq == 0.0) return;
    const double diff = S[q][q] - S[p][p];
    const double twice = 2.0 * apq;
    const double theta = diff / twice;
    const double sq = theta * theta;
    const double root = std::sqrt(sq + 1.0);
    double t = 1.0 / (std::fabs(theta) + root);
    if (theta < 0.0) t = -t;
    const double tt = t * t;
    const double c = 1.0 / std::sqrt(tt + 1.0);
    const double s = t * c;
    const double h = t * apq;
    S[p][p] = S[p][p] - h;
    S[q][q] = S[q][q] + h;
    S[p][q] = S[q][p] = 0.0;
    const int r = 3 - p - q;
    const double srp = S[r][p], srq = S[r][q];
    const double a0 = c * srp, a1 = s * srq, b0 = s * srp, b1 = c * srq;
    S[r][p] = S[p][r] = a0 - a1;
    S[r][q] = S[q][r] = b0 + b1;
    for (int i = 0; i < 3; ++i) {
        const double vip = V[i][p], viq = V[i][q];
        const double c0 = c * vip, c1 = s * viq, d0 = s * vip, d1 = c * viq;
        V[i][p] = c0 - c1;
        V[i][q] = d0 + d1;
    }
}

}  // namespace

void shapeFrame(const emf_shape_moments_t& mom, emf_shape_frame_t& out) {
    out.valid = 0;
    if (mom.solid == 0) return;
    static const int kPairs[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
    const double n = static_cast<double>(mom.solid);
    const double den = n * n;
    double m[3], C[6];
    for (int j = 0; j < 3; ++j) m[j] = static_cast<double>(mom.sum[j]) / n;
    for (int i = 0; i < 6; ++i) {  // the numerator exact in 128 bits, rounded to double once
        const __int128 num = static_cast<__int128>(mom.solid) * static_cast<__int128>(mom.sum2[i]) -
                             static_cast<__int128>(mom.sum[kPairs[i][0]]) * static_cast<__int128>(mom.sum[kPairs[i][1]]);
        C[i] = static_cast<double>(num) / den;
    }
    double S[3][3] = {{C[0], C[3], C[4]}, {C[3], C[1], C[5]}, {C[4], C[5], C[2]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < EMF_SHAPE_JACOBI_SWEEPS; ++sweep) {
        rotate(S, V, 0, 1);
        rotate(S, V, 0, 2);
        rotate(S, V, 1, 2);
    }
    const double eig[3] = {S[0][0], S[1][1], S[2][2]};
    int order[3] = {0, 1, 2};
    std::stable_sort(order, order + 3, [&](int a, int b) { return eig[a] > eig[b]; });  // descending, ties to the lower index
    double A[3][3];
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) A[k][i] = V[i][order[k]];
    for (int k = 0; k < 2; ++k) {
        int big = 0;
        for (int i = 1; i < 3; ++i)
            if (std::fabs(A[k][i]) > std::fabs(A[k][big])) big = i;
        if (A[k][big] < 0.0)
            for (int i = 0; i < 3; ++i) A[k][i] = -A[k][i];
    }
    {
        const double* a = A[0];
        const double* b = A[1];
        const double x0 = a[1] * b[2], x1 = a[2] * b[1], y0 = a[2] * b[0], y1 = a[0] * b[2], z0 = a[0] * b[1], z1 = a[1] * b[0];
        A[2][0] = x0 - x1;
        A[2][1] = y0 - y1;
        A[2][2] = z0 - z1;
    }
    out.valid = 1;
    out.reserved = 0;
    for (int j = 0; j < 3; ++j) {
        out.centroid[j] = m[j];
        out.eigenvalues[j] = eig[order[j]];
        out.f32.c[j] = static_cast<float>(m[j]);
    }
    for (int i = 0; i < 6; ++i) out.covariance[i] = C[i];
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) {
            out.axes[3 * k + i] = A[k][i];
            out.f32.A[3 * k + i] = static_cast<float>(A[k][i]);
        }
}

void shapeBox(const emf_shape_moments_t& mom, const emf_shape_frame_t& frame, const emf_shape_extents_t& ext, const int32_t res[3],
              float voxelSize, const float R32[9], const float t32[3], emf_shape_box_t& out) {
    const double* A = frame.axes;
    const double vs = static_cast<double>(voxelSize);
    double R[9], t[3], mid[3];
    for (int i = 0; i < 9; ++i) R[i] = static_cast<double>(R32[i]);
    for (int i = 0; i < 3; ++i) t[i] = static_cast<double>(t32[i]);
    for (int k = 0; k < 3; ++k) {
        const double sum = static_cast<double>(ext.lo[k]) + static_cast<double>(ext.hi[k]);
        mid[k] = sum / 2.0;
    }
    for (int j = 0; j < 3; ++j) {
        double s = A[j] * mid[0];
        s = s + A[3 + j] * mid[1];
        s = s + A[6 + j] * mid[2];
        out.center_vox[j] = frame.centroid[j] + s;
    }
    for (int k = 0; k < 3; ++k) {
        double w = std::fabs(A[3 * k]) + std::fabs(A[3 * k + 1]);
        w = w + std::fabs(A[3 * k + 2]);
        const double span = static_cast<double>(ext.hi[k]) - static_cast<double>(ext.lo[k]);
        const double a = span / 2.0, b = w / 2.0;
        out.half_vox[k] = a + b;
    }
    const double ff = static_cast<double>(mom.faces_free), fu = static_cast<double>(mom.faces_unknown);
    const double faces = ff + fu;
    out.completeness = faces == 0.0 ? std::numeric_limits<double>::quiet_NaN() : ff / faces;
    for (int j = 0; j < 3; ++j) {
        const double half = (static_cast<double>(res[j]) - 1.0) / 2.0;
        const double d = out.center_vox[j] - half;
        out.center_obj[j] = d * vs;
        out.half_m[j] = out.half_vox[j] * vs;
    }
    auto toWorld = [&](const double* p, double* w) {
        for (int i = 0; i < 3; ++i) {
            double s = R[3 * i] * p[0];
            s = s + R[3 * i + 1] * p[1];
            s = s + R[3 * i + 2] * p[2];
            w[i] = s + t[i];
        }
    };
    for (int i = 0; i < 8; ++i) {
        double h[3];
        for (int k = 0; k < 3; ++k) h[k] = (i >> k) & 1 ? out.half_m[k] : -out.half_m[k];
        double* p = out.corners_obj + 3 * i;
        for (int j = 0; j < 3; ++j) {
            double s = out.center_obj[j] + h[0] * A[j];
            s = s + h[1] * A[3 + j];
            s = s + h[2] * A[6 + j];
            p[j] = s;
        }
        toWorld(p, out.corners_world + 3 * i);
    }
    toWorld(out.center_obj, out.center_world);
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) {
            double s = R[3 * i] * A[3 * k];
            s = s + R[3 * i + 1] * A[3 * k + 1];
            s = s + R[3 * i + 2] * A[3 * k + 2];
            out.axes_world[3 * k + i] = s;
        }
}

const std::vector<EMFusion::ObjectShape>& EMFusion::objectShapes(const std::vector<int>& ids, bool includeBackground) {
    if (sharded || world > 1) throw HipError("EMFusion::objectShapes: object shapes are not supported on the sharded path", EMF_E_ARG);
    std::vector<int> all;
    if (includeBackground) all.push_back(0);
    for (int id : ids) {
        if (id <= 0 || !getObject(id)) throw HipError("EMFusion::objectShapes: no object " + std::to_string(id), EMF_E_ARG);
        all.push_back(id);
    }
    const int n = static_cast<int>(all.size());
    if (n > EMF_MAX_MODELS) throw HipError("EMFusion::objectShapes: " + std::to_string(n) + " models", EMF_E_LIMIT);
    shLast.clear();
    if (n == 0) return shLast;
    drainForQuery();
    std::vector<ObjectShape> out(all.size());
    std::vector<emf_model_t> table(all.size());
    std::vector<int32_t> res(3 * all.size());
    for (int k = 0; k < n; ++k) {  // the volumes' current copies (describe() follows the background's flips)
        const TSDF* vol = all[k] == 0 ? static_cast<const TSDF*>(&background) : getObject(all[k]);
        vol->describe(table[k]);
        ObjectShape& s = out[k];
        s.id = all[k];
        s.res = vol->getVolumeRes();
        s.voxelSize = vol->getVoxelSize();
        s.pose = vol->getPose();
        std::copy(table[k].res, table[k].res + 3, res.begin() + 3 * k);
    }
    const size_t un = all.size();
    // one device block: the table, the moments, the frames, the extents
    const size_t tableBytes = un * sizeof(emf_model_t), momBytes = un * sizeof(emf_shape_moments_t),
                 axesBytes = un * sizeof(emf_shape_axes_t), extBytes = un * sizeof(emf_shape_extents_t);
    shScratch.reserve(tableBytes + momBytes + axesBytes + extBytes);
    uint8_t* base = shScratch.as<uint8_t>();
    auto* dTable = reinterpret_cast<emf_model_t*>(base);
    auto* dMom = reinterpret_cast<emf_shape_moments_t*>(base + tableBytes);
    auto* dAxes = reinterpret_cast<emf_shape_axes_t*>(base + tableBytes + momBytes);
    auto* dExt = reinterpret_cast<emf_shape_extents_t*>(base + tableBytes + momBytes + axesBytes);
    std::vector<emf_shape_moments_t> mom(un);
    std::vector<emf_shape_axes_t> axes(un);
    std::vector<emf_shape_extents_t> ext(un);
    hipCheck(hipMemcpyAsync(dTable, table.data(), tableBytes, hipMemcpyHostToDevice, main.get()), "EMFusion::objectShapes (table)");
    emfCheck(emf_hip_shapeMoments(dTable, res.data(), 0, n, dMom, main.abi()), "EMFusion::objectShapes (moments)");
    hipCheck(hipMemcpyAsync(mom.data(), dMom, momBytes, hipMemcpyDeviceToHost, main.get()), "EMFusion::objectShapes (records)");
    main.waitForCompletion();  // the frames come from the moments
    for (size_t k = 0; k < un; ++k) {
        out[k].moments = mom[k];
        std::memset(&out[k].frame, 0, sizeof(emf_shape_frame_t));
        shapeFrame(mom[k], out[k].frame);
        axes[k] = out[k].frame.f32;  // all zero for a model without a solid voxel: nothing is measured along it
    }
    hipCheck(hipMemcpyAsync(dAxes, axes.data(), axesBytes, hipMemcpyHostToDevice, main.get()), "EMFusion::objectShapes (frames)");
    emfCheck(emf_hip_shapeExtents(dTable, res.data(), 0, n, dAxes, dExt, main.abi()), "EMFusion::objectShapes (extents)");
    hipCheck(hipMemcpyAsync(ext.data(), dExt, extBytes, hipMemcpyDeviceToHost, main.get()), "EMFusion::objectShapes (extents back)");
    main.waitForCompletion();
    for (size_t k = 0; k < un; ++k) {
        out[k].extents = ext[k];
        std::memset(&out[k].box, 0, sizeof(emf_shape_box_t));
        if (out[k].frame.valid)
            shapeBox(mom[k], out[k].frame, ext[k], out[k].res.val, out[k].voxelSize, out[k].pose.rotation().val,
                     out[k].pose.translation().val, out[k].box);
    }
    shLast = std::move(out);
    return shLast;
}

// shapes.txt (setShapeOutput): after a comment line one line per live object, in id order:
//     id valid solid observed faces_free faces_unknown lo_x lo_y lo_z hi_x hi_y hi_z, the integers, then the world-frame
// box in %.9g: centre (3), half extents in metres (3), the three axes (9).  An object without a solid voxel has valid 0
// and zeros for the box.
void EMFusion::writeShapes(const std::string& dir) {
    std::vector<int> ids;
    for (const ObjTSDF& obj : objects) ids.push_back(obj.getID());
    std::sort(ids.begin(), ids.end());
    const std::vector<ObjectShape> shapes = objectShapes(ids, false);
    const std::string path = dir + "/shapes.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writeShapes: cannot create " + path);
    std::fprintf(file, "# id valid solid observed faces_free faces_unknown lo(3) hi(3) center_world(3) half_m(3) axes_world(9): "
                       "the observed solid band, not the body\n");
    for (const ObjectShape& s : shapes) {
        const emf_shape_moments_t& m = s.moments;
        std::fprintf(file, "%d %d %llu %llu %llu %llu %d %d %d %d %d %d", s.id, s.frame.valid, static_cast<unsigned long long>(m.solid),
                     static_cast<unsigned long long>(m.observed), static_cast<unsigned long long>(m.faces_free),
                     static_cast<unsigned long long>(m.faces_unknown), m.lo[0], m.lo[1], m.lo[2], m.hi[0], m.hi[1], m.hi[2]);
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", s.box.center_world[i]);
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", s.box.half_m[i]);
        for (int i = 0; i < 9; ++i) std::fprintf(file, " %.9g", s.box.axes_world[i]);
        std::fprintf(file, "\n");
    }
    std::fclose(file);
}

}  // namespace emf
