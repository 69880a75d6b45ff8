// EMFusionGround.cpp -- emf::EMFusion: the ground map of the scene (new behaviour, opt-in).  The
// occupancy classes of a box of the background, the live objects stamped, projected along "up" onto ground cells: three
// entries of include/emf_hip.h "Ground map" on the main stream, one wait.  The frame is float64 on the host in the
// operation order written out in that header; this unit is compiled without a*b+c contraction.
#include "EMFusion.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

namespace emf {

int groundFrame(const QueryBox& box, const double up[3], double cell, double bin, const double ref[3], double bandLo,
                double bandHi, emf_ground_frame_t& frame, double pose[12], std::string& why) {
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(up[i]) || !std::isfinite(ref[i])) {
            why = "a non-finite up or reference";
            return EMF_E_ARG;
        }
    if (!(cell > 0.0) || !(bin > 0.0) || !std::isfinite(cell) || !std::isfinite(bin)) {
        why = "cell and bin must be positive metres";
        return EMF_E_ARG;
    }
    if (!std::isfinite(bandLo) || !std::isfinite(bandHi) || !(bandHi > bandLo)) {
        why = "the height band is empty";
        return EMF_E_ARG;
    }
    // 1: h
    double s = up[0] * up[0];
    s = s + up[1] * up[1];
    s = s + up[2] * up[2];
    const double len = std::sqrt(s);
    if (!(len > 0.0) || !std::isfinite(len)) {
        why = "up has no direction";
        return EMF_E_ARG;
    }
    double E[3][3];  // rows u, v, h
    for (int i = 0; i < 3; ++i) E[2][i] = up[i] / len;
    const double* h = E[2];
    // 2: u from the background's x axis, or its z axis where x is along up
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = static_cast<double>(box.bgPose.rotation().val[i]);
    double w[3], n2 = 0.0;
    for (int column = 0; column <= 2; column += 2) {
        const double a[3] = {R[column], R[3 + column], R[6 + column]};
        double d = a[0] * h[0];
        d = d + a[1] * h[1];
        d = d + a[2] * h[2];
        for (int i = 0; i < 3; ++i) {
            const double along = d * h[i];
            w[i] = a[i] - along;
        }
        n2 = w[0] * w[0];
        n2 = n2 + w[1] * w[1];
        n2 = n2 + w[2] * w[2];
        if (!(n2 < 1e-6)) break;
    }
    const double wl = std::sqrt(n2);
    for (int i = 0; i < 3; ++i) E[0][i] = w[i] / wl;
    const double* u = E[0];
    // 3: v = h x u
    {
        double a, b;
        a = h[1] * u[2], b = h[2] * u[1], E[1][0] = a - b;
        a = h[2] * u[0], b = h[0] * u[2], E[1][1] = a - b;
        a = h[0] * u[1], b = h[1] * u[0], E[1][2] = a - b;
    }
    // 4: the map per voxel step and the ground metres of box voxel (0, 0, 0)
    const double vs = static_cast<double>(box.voxelSize);
    const double zero[3] = {0.0, 0.0, 0.0};
    double p0[3];
    box.worldPoint(zero, p0);
    double M[3][3], g[3];
    for (int j = 0; j < 3; ++j) {
        for (int k = 0; k < 3; ++k) {
            double m = E[j][0] * R[k];
            m = m + E[j][1] * R[3 + k];
            m = m + E[j][2] * R[6 + k];
            M[j][k] = m * vs;
        }
        double q = E[j][0] * p0[0];
        q = q + E[j][1] * p0[1];
        q = q + E[j][2] * p0[2];
        g[j] = q;
    }
    // 5: rows 0 and 1 in cells, shifted so that the lowest corner of the box lands in cell 0
    double A[3][4], mn[2];
    for (int j = 0; j < 2; ++j) {
        for (int k = 0; k < 3; ++k) A[j][k] = M[j][k] / cell;
        const double a = g[j] / cell;
        double lo = 0.0, hi = 0.0;
        for (int c = 0; c < 8; ++c) {
            double b[3];
            for (int k = 0; k < 3; ++k) b[k] = ((c >> k) & 1) ? static_cast<double>(box.size[k]) - 0.5 : -0.5;
            double q = A[j][0] * b[0];
            q = q + A[j][1] * b[1];
            q = q + A[j][2] * b[2];
            q = q + a;
            if (c == 0 || q < lo) lo = q;
            if (c == 0 || q > hi) hi = q;
        }
        mn[j] = lo;
        A[j][3] = a - lo;
        const double cells = std::floor(hi - lo) + 1.0;
        if (!(cells <= static_cast<double>(EMF_DF_MAX_AXIS))) {
            why = "the map has more than " + std::to_string(EMF_DF_MAX_AXIS) + " cells on an axis";
            return EMF_E_LIMIT;
        }
        frame.map[j] = static_cast<int32_t>(cells);
    }
    // 6: row 2 in bins above the lower end of the band
    for (int k = 0; k < 3; ++k) A[2][k] = M[2][k] / bin;
    double z0 = h[0] * ref[0];
    z0 = z0 + h[1] * ref[1];
    z0 = z0 + h[2] * ref[2];
    z0 = z0 + bandLo;
    const double above = g[2] - z0;
    A[2][3] = above / bin;
    // 7: the bins
    const double span = bandHi - bandLo;
    const double bins = std::ceil(span / bin);
    if (!(bins >= 1.0)) {
        why = "the height band holds no bin";
        return EMF_E_ARG;
    }
    if (!(bins <= static_cast<double>(EMF_GROUND_MAX_BINS))) {
        why = "more than " + std::to_string(EMF_GROUND_MAX_BINS) + " height bins";
        return EMF_E_LIMIT;
    }
    frame.bins = static_cast<int32_t>(bins);
    // 8: rounded once
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 4; ++k) frame.G[4 * j + k] = static_cast<float>(A[j][k]);
    // ground metres -> world: (u, v, h) as columns, the origin at the map's corner and the band's lower end
    const double ou = mn[0] * cell, ov = mn[1] * cell;
    for (int i = 0; i < 3; ++i) {
        pose[3 * i] = u[i], pose[3 * i + 1] = E[1][i], pose[3 * i + 2] = h[i];
        double o = u[i] * ou;
        o = o + E[1][i] * ov;
        o = o + h[i] * z0;
        pose[9 + i] = o;
    }
    return EMF_OK;
}

bool groundFrameAligned(const emf_ground_frame_t& frame) {
    for (int j = 0; j < 3; ++j) {
        const float* g = frame.G + 4 * j;
        const float a[3] = {std::fabs(g[0]), std::fabs(g[1]), std::fabs(g[2])};
        const float top = std::max(a[0], std::max(a[1], a[2]));
        int large = 0;
        for (int k = 0; k < 3; ++k)
            if (a[k] > top * 9.5367431640625e-07f) ++large;  // 2^-20
        if (large != 1) return false;
    }
    return true;
}

const EMFusion::GroundMap& EMFusion::groundMap(const Vec3i& boxLo, const Vec3i& boxSize, const double up[3], double cell,
                                               double bin, const double ref[3], double bandLo, double bandHi, int robotBins,
                                               int maxStepBins, const std::vector<int>& excludeIds) {
    GroundMap out;
    out.box = makeQueryBox("groundMap", "the ground map is", boxLo, boxSize);
    if (robotBins < 1) throw HipError("EMFusion::groundMap: a robot of " + std::to_string(robotBins) + " bins", EMF_E_ARG);
    if (maxStepBins < 0) throw HipError("EMFusion::groundMap: a negative step", EMF_E_ARG);
    std::string why;
    if (const int rc = groundFrame(out.box, up, cell, bin, ref, bandLo, bandHi, out.frame, out.pose, why))
        throw HipError("EMFusion::groundMap: " + why, rc);
    out.robotBins = robotBins;
    out.maxStepBins = maxStepBins;
    drainForQuery();
    const size_t cells = static_cast<size_t>(out.frame.map[0]) * out.frame.map[1];
    const size_t words = static_cast<size_t>((out.frame.bins + 63) / 64);
    gmBoxClasses.reserve(out.box.voxels());
    gmPlanes.reserve(2 * cells * words * sizeof(uint64_t));
    gmCells.reserve(cells * sizeof(emf_ground_cell_t));
    gmClasses.reserve(cells);
    uint64_t* occ = gmPlanes.as<uint64_t>();
    uint64_t* fre = occ + cells * words;
    enqueueOccupancy("groundMap", out.box, excludeIds, gmBoxClasses.as<uint8_t>(), nullptr, nullptr);
    emfCheck(emf_hip_groundColumns(gmBoxClasses.as<uint8_t>(), out.box.size.val, out.frame, occ, fre, main.abi()),
             "EMFusion::groundMap (columns)");
    emfCheck(emf_hip_groundCells(occ, fre, out.frame.map, out.frame.bins, robotBins, gmCells.as<emf_ground_cell_t>(), main.abi()),
             "EMFusion::groundMap (cells)");
    emfCheck(emf_hip_groundClasses(gmCells.as<emf_ground_cell_t>(), out.frame.map, maxStepBins, gmClasses.as<uint8_t>(), main.abi()),
             "EMFusion::groundMap (classes)");
    main.waitForCompletion();
    out.cells = gmCells.as<emf_ground_cell_t>();
    out.classes = gmClasses.as<uint8_t>();
    gmLast = out;
    return gmLast;
}

// ground.bin and ground.txt of the whole background (setGroundOutput); the reference is the camera position
void EMFusion::writeGround(const std::string& dir) {
    const GroundOutput& o = expGround_;
    const Vec3i n = background.getVolumeRes();
    Vec3i boxLo, boxSize;  // the whole background; the world extent with setQueryExtent(true)
    resultsBox("writeGround", boxLo, boxSize);
    const double voxel = static_cast<double>(background.getVoxelSize());
    const double cell = o.cell > 0.0 ? o.cell : 2.0 * voxel, bin = o.bin > 0.0 ? o.bin : 2.0 * voxel;
    double up[3] = {o.up[0], o.up[1], o.up[2]};
    if (expGroundUpFloor_) {  // --ground-up floor: the normal of the floor the plane search finds
        const emf_plane_params_t pp{15, 1, EMF_PLANE_MAX_PLANES, 2, 20.0, 0.0, 1.0, 2.0, 0};
        const Planes& found = planes(Vec3i(0, 0, 0), n, pp, false);
        std::vector<PlaneWorld> world;
        const double hint[3] = {0.0, 0.0, 0.0};
        const int floor = describePlanes(found, hint, 30.0, 10.0, world);
        if (floor < 0) throw HipError("EMFusion::writeGround: up is the floor's normal and the plane search finds no floor", EMF_E_ARG);
        for (int i = 0; i < 3; ++i) up[i] = world[static_cast<size_t>(floor)].normal[i];
    } else if (up[0] == 0.0 && up[1] == 0.0 && up[2] == 0.0) {
        const float* R = background.getPose().rotation().val;
        for (int i = 0; i < 3; ++i) up[i] = -static_cast<double>(R[3 * i + 1]);
    }
    const double ref[3] = {static_cast<double>(pose.translation().val[0]), static_cast<double>(pose.translation().val[1]),
                           static_cast<double>(pose.translation().val[2])};
    const int robot = groundRobotBins(static_cast<float>(o.robotHeight), static_cast<float>(bin));
    const int step = groundStepBins(static_cast<float>(o.maxStep), static_cast<float>(bin));
    if (cell < 2.0 * voxel || bin < 2.0 * voxel) {  // narrower slots leave holes unless up is along a box axis
        emf_ground_frame_t f{};
        double p[12];
        std::string why;
        const int rc = groundFrame(queryBoxAt(boxLo, boxSize), up, cell, bin, ref, o.bandLo, o.bandHi, f, p, why);
        if (rc) throw HipError("EMFusion::writeGround: " + why, rc);
        if (!groundFrameAligned(f))
            throw HipError("EMFusion::writeGround: cells and bins below two voxels need an up along a box axis", EMF_E_ARG);
    }
    const GroundMap& g = groundMap(boxLo, boxSize, up, cell, bin, ref, o.bandLo, o.bandHi, robot, step, {});
    const size_t cells = static_cast<size_t>(g.frame.map[0]) * g.frame.map[1];
    std::vector<uint8_t> classes(cells);
    std::vector<emf_ground_cell_t> records(cells);
    hipCheck(hipMemcpyAsync(classes.data(), g.classes, cells, hipMemcpyDeviceToHost, main.get()), "EMFusion::writeGround (classes)");
    hipCheck(hipMemcpyAsync(records.data(), g.cells, cells * sizeof(emf_ground_cell_t), hipMemcpyDeviceToHost, main.get()),
             "EMFusion::writeGround (cells)");
    main.waitForCompletion();
    std::ofstream bin_(dir + "/ground.bin", std::ios::binary);
    bin_.write(reinterpret_cast<const char*>(classes.data()), static_cast<std::streamsize>(cells));
    bin_.write(reinterpret_cast<const char*>(records.data()), static_cast<std::streamsize>(cells * sizeof(emf_ground_cell_t)));
    if (!bin_) throw HipError("EMFusion::writeGround: cannot write " + dir + "/ground.bin", EMF_E_ARG);
    std::FILE* txt = std::fopen((dir + "/ground.txt").c_str(), "w");
    if (!txt) throw HipError("EMFusion::writeGround: cannot write " + dir + "/ground.txt", EMF_E_ARG);
    std::fprintf(txt, "# ground map: ground.bin holds W * H class bytes (0 free, 1 occupied, 2 unknown), then W * H records of "
                      "four int16 (floor top clear levels); G maps a background voxel to (u cells, v cells, h bins); "
                      "pose maps ground metres to the world\n");
    std::fprintf(txt, "map %d %d\n", g.frame.map[0], g.frame.map[1]);
    std::fprintf(txt, "bins %d robot %d step %d\n", g.frame.bins, g.robotBins, g.maxStepBins);
    std::fprintf(txt, "cell %.9g bin %.9g\n", cell, bin);
    for (int j = 0; j < 3; ++j)
        std::fprintf(txt, "G %.9g %.9g %.9g %.9g\n", g.frame.G[4 * j], g.frame.G[4 * j + 1], g.frame.G[4 * j + 2], g.frame.G[4 * j + 3]);
    for (int j = 0; j < 4; ++j) std::fprintf(txt, "pose %.9g %.9g %.9g\n", g.pose[3 * j], g.pose[3 * j + 1], g.pose[3 * j + 2]);
    std::fclose(txt);
}

}  // namespace emf
