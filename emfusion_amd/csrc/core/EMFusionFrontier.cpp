// EMFusionFrontier.cpp -- emf::EMFusion: exploration frontiers of the scene (new behaviour).  The
// occupancy classes of a box of the background with the live objects stamped, exactly as the distance field forms
// them, then the free voxels that touch unknown space, their 26-connected clusters and one record per cluster: the
// entries of include/emf_hip.h "Frontiers" on the main stream, in buffers of their own.
#include "EMFusion.hpp"
#include "Output.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>

namespace emf {

const EMFusion::Frontiers& EMFusion::frontiers(const Vec3i& boxLo, const Vec3i& boxSize, int minVoxels, int clearanceVoxels,
                                               const std::vector<int>& excludeIds) {
    Frontiers out;
    out.box = makeQueryBox("frontiers", "frontiers are", boxLo, boxSize);
    if (minVoxels < 1) throw HipError("EMFusion::frontiers: minVoxels below 1", EMF_E_ARG);
    if (clearanceVoxels < 0) throw HipError("EMFusion::frontiers: a negative clearance", EMF_E_ARG);
    drainForQuery();
    frClasses.reserve(out.box.voxels());
    frLabels.reserve(out.box.voxels() * sizeof(int32_t));
    frCounters.reserve(4 * sizeof(uint32_t));

    out.minVoxels = minVoxels;
    out.clearanceVoxels = clearanceVoxels;
    uint8_t* classes = frClasses.as<uint8_t>();
    int32_t* labels = frLabels.as<int32_t>();
    uint32_t* counters = frCounters.as<uint32_t>();
    enqueueOccupancy("frontiers", out.box, excludeIds, classes, nullptr, nullptr);
    const Clearance clear = enqueueClearance("frontiers", out.box, classes, clearanceVoxels);
    emfCheck(emf_hip_frontierLabel(classes, boxSize.val, clear.d2, clear.minD2, labels, counters, main.abi()),
             "EMFusion::frontiers (labels)");
    uint32_t host[3] = {0u, 0u, 0u};
    hipCheck(hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, main.get()), "EMFusion::frontiers (counters)");
    main.waitForCompletion();  // the one number the per-cluster tables are sized by
    const uint32_t all = host[EMF_FRONTIER_CLUSTERS];
    const size_t scratch = emf_hip_frontierScratchBytes(boxSize.val, all);
    frScratch.reserve(scratch);
    frRecords.reserve(all * sizeof(emf_frontier_cluster_t));
    emfCheck(emf_hip_frontierClusters(labels, boxSize.val, minVoxels, all, frScratch.data(),
                                      all ? frRecords.as<emf_frontier_cluster_t>() : nullptr, static_cast<int32_t>(all), counters,
                                      main.abi()),
             "EMFusion::frontiers (clusters)");
    hipCheck(hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, main.get()), "EMFusion::frontiers (counters)");
    out.clusters.resize(all);  // the kept ones are the first of them
    if (all)
        hipCheck(hipMemcpyAsync(out.clusters.data(), frRecords.data(), all * sizeof(emf_frontier_cluster_t), hipMemcpyDeviceToHost,
                                main.get()),
                 "EMFusion::frontiers (records)");
    main.waitForCompletion();
    out.kept = host[EMF_FRONTIER_KEPT];
    out.all = host[EMF_FRONTIER_CLUSTERS];
    out.voxels = host[EMF_FRONTIER_VOXELS];
    out.clusters.resize(std::min(out.kept, all));
    std::sort(out.clusters.begin(), out.clusters.end(), [](const emf_frontier_cluster_t& a, const emf_frontier_cluster_t& b) {
        return a.count != b.count ? a.count > b.count : a.label < b.label;
    });
    out.classes = classes;
    out.labels = labels;
    frLast = std::move(out);
    return frLast;
}

void EMFusion::frontierWorldPoint(const Frontiers& f, const emf_frontier_cluster_t& c, bool representative, double out[3]) {
    double v[3];
    for (int i = 0; i < 3; ++i)
        v[i] = representative ? static_cast<double>(c.rep[i]) : static_cast<double>(c.sum[i]) / static_cast<double>(c.count);
    f.box.worldPoint(v, out);
}

// frontiers.txt of the whole background, or of the world extent after a second comment line that states it
// (setFrontierOutput).  After a comment line, one line per kept cluster, largest
// first (ties: smallest label):
//     count  rx ry rz  cx cy cz  x0 y0 z0 x1 y1 z1
// count: voxels, %d; r: the representative voxel and c: the centroid in the world frame, metres, each the double value
// rounded once to float and printed %.9g; the inclusive bounding box in voxels of the background, %d.
void EMFusion::writeFrontiers(const std::string& dir) {
    Vec3i lo, n;  // the whole background; the world extent with setQueryExtent(true)
    resultsBox("writeFrontiers", lo, n);
    const float voxel = background.getVoxelSize();
    const int clearance = metresToVoxels(frontierClearanceMetres_, voxel);
    const Frontiers& f = frontiers(lo, n, std::max(frontierMinVoxels_, 1), clearance, {});
    const std::string path = dir + "/frontiers.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writeFrontiers: cannot create " + path);
    std::fprintf(file, "# count rep_x rep_y rep_z centroid_x centroid_y centroid_z lo_x lo_y lo_z hi_x hi_y hi_z\n");
    if (queryWorld_)  // a second comment line: the box, in voxels of the current background
        std::fprintf(file, "# world extent: lo %d %d %d size %d %d %d\n", lo[0], lo[1], lo[2], n[0], n[1], n[2]);
    const Vec3i at = f.box.volumeLo();
    for (const emf_frontier_cluster_t& c : f.clusters) {
        double r[3], m[3];
        frontierWorldPoint(f, c, true, r);
        frontierWorldPoint(f, c, false, m);
        std::fprintf(file, "%d %.9g %.9g %.9g %.9g %.9g %.9g %d %d %d %d %d %d\n", c.count,
                     static_cast<double>(static_cast<float>(r[0])), static_cast<double>(static_cast<float>(r[1])),
                     static_cast<double>(static_cast<float>(r[2])), static_cast<double>(static_cast<float>(m[0])),
                     static_cast<double>(static_cast<float>(m[1])), static_cast<double>(static_cast<float>(m[2])),
                     at[0] + c.lo[0], at[1] + c.lo[1], at[2] + c.lo[2], at[0] + c.hi[0], at[1] + c.hi[1], at[2] + c.hi[2]);
    }
    std::fclose(file);
}

}  // namespace emf
