// EMFusionPlan.cpp -- emf::EMFusion: path planning over the scene (new behaviour).  The occupancy
// classes of a box of the background with the live objects stamped, exactly as the frontiers form them, then the
// cost-to-go field from the start voxels through free space and the paths from the goals back: the entries of
// include/emf_hip.h "Planning" on the main stream, in buffers of their own.
#include "EMFusion.hpp"
#include "Output.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>

namespace emf {

namespace {

std::vector<int32_t> flat(const std::vector<Vec3i>& voxels) {
    std::vector<int32_t> out;
    out.reserve(3 * voxels.size());
    for (const Vec3i& v : voxels) out.insert(out.end(), v.val, v.val + 3);
    return out;
}

}  // namespace

const EMFusion::Plan& EMFusion::plan(const Vec3i& boxLo, const Vec3i& boxSize, const std::vector<Vec3i>& startVoxels,
                                     int seedRadiusVoxels, bool throughUnknown, int clearanceVoxels, uint32_t maxCost,
                                     const std::vector<Vec3i>& goalVoxels, int pathCapacity, const std::vector<int>& excludeIds) {
    const QueryBox box = makeQueryBox("plan", "planning is", boxLo, boxSize);
    const size_t voxels = box.voxels();
    if (voxels > (1ull << 29)) throw HipError("EMFusion::plan: a box of more than 2^29 voxels", EMF_E_LIMIT);
    if (startVoxels.empty()) throw HipError("EMFusion::plan: no start voxel", EMF_E_ARG);
    if (seedRadiusVoxels < 0 || seedRadiusVoxels > 4096) throw HipError("EMFusion::plan: a start radius outside 0 .. 4096", EMF_E_ARG);
    if (clearanceVoxels < 0) throw HipError("EMFusion::plan: a negative clearance", EMF_E_ARG);
    if (maxCost >= EMF_PLAN_BLOCKED) throw HipError("EMFusion::plan: maxCost is no cost", EMF_E_ARG);
    if (goalVoxels.size() > 0x7fffffffull / 3) throw HipError("EMFusion::plan: too many goals", EMF_E_LIMIT);
    drainForQuery();
    plLast = Plan();  // its device arrays are about to be reused or freed: no last plan until this one is complete
    plShortcutWindow = 0;
    const size_t nGoals = goalVoxels.size();
    plClasses.reserve(voxels);
    plCost.reserve(voxels * sizeof(uint32_t));
    plScratch.reserve(emf_hip_planScratchBytes(boxSize.val));
    plCounters.reserve(4 * sizeof(uint32_t));
    plSeeds.reserve(3 * sizeof(int32_t) * startVoxels.size());
    plGoals.reserve(3 * sizeof(int32_t) * nGoals);
    plLengths.reserve(sizeof(int32_t) * nGoals);
    plGoalCost.reserve(sizeof(uint32_t) * nGoals);

    Plan out;
    out.box = box;
    out.seedRadiusVoxels = seedRadiusVoxels;
    out.clearanceVoxels = clearanceVoxels;
    out.throughUnknown = throughUnknown;
    out.maxCost = maxCost;
    uint8_t* classes = plClasses.as<uint8_t>();
    uint32_t* cost = plCost.as<uint32_t>();
    uint32_t* counters = plCounters.as<uint32_t>();
    enqueueOccupancy("plan", box, excludeIds, classes, nullptr, nullptr);
    const Clearance clear = enqueueClearance("plan", box, classes, clearanceVoxels);
    plClearanceSerial = clearanceSerial;
    const std::vector<int32_t> seeds = flat(startVoxels), goals = flat(goalVoxels);
    hipCheck(hipMemcpyAsync(plSeeds.data(), seeds.data(), seeds.size() * sizeof(int32_t), hipMemcpyHostToDevice, main.get()),
             "EMFusion::plan (seeds)");
    const uint32_t mask = (1u << EMF_OCC_FREE) | (throughUnknown ? 1u << EMF_OCC_UNKNOWN : 0u);
    // waits on the main stream, once per batch of rounds
    emfCheck(emf_hip_planCost(classes, boxSize.val, clear.d2, clear.minD2, mask,
                              plSeeds.as<int32_t>(), static_cast<int32_t>(startVoxels.size()), seedRadiusVoxels, maxCost, 0, cost,
                              plScratch.data(), counters, main.abi()),
             "EMFusion::plan (cost)");
    hipCheck(hipMemcpyAsync(out.counters, counters, sizeof(out.counters), hipMemcpyDeviceToHost, main.get()), "EMFusion::plan (counters)");
    std::vector<int32_t> lengths(nGoals, 0), paths;
    std::vector<uint32_t> goalCost(nGoals, EMF_PLAN_BLOCKED);
    int capacity = std::max(pathCapacity, 0);
    if (nGoals) {
        hipCheck(hipMemcpyAsync(plGoals.data(), goals.data(), goals.size() * sizeof(int32_t), hipMemcpyHostToDevice, main.get()),
                 "EMFusion::plan (goals)");
        auto walk = [&](int cap_) {
            emfCheck(emf_hip_planPaths(cost, boxSize.val, plGoals.as<int32_t>(), static_cast<int32_t>(nGoals), cap_,
                                       cap_ > 0 ? plPaths.as<int32_t>() : nullptr, plLengths.as<int32_t>(), plGoalCost.as<uint32_t>(),
                                       main.abi()),
                     "EMFusion::plan (paths)");
            hipCheck(hipMemcpyAsync(lengths.data(), plLengths.data(), nGoals * sizeof(int32_t), hipMemcpyDeviceToHost, main.get()),
                     "EMFusion::plan (lengths)");
        };
        if (pathCapacity < 0) {  // the lengths first: they size the paths
            walk(0);
            main.waitForCompletion();
            for (int32_t l : lengths) capacity = std::max(capacity, std::abs(l));
        }
        if (static_cast<unsigned long long>(capacity) * nGoals > 0x7fffffffull)
            throw HipError("EMFusion::plan: the paths of all goals exceed 2^31 - 1 voxels", EMF_E_LIMIT);
        paths.assign(static_cast<size_t>(capacity) * nGoals, -1);
        if (capacity > 0) plPaths.reserve(paths.size() * sizeof(int32_t));
        walk(capacity);
        hipCheck(hipMemcpyAsync(goalCost.data(), plGoalCost.data(), nGoals * sizeof(uint32_t), hipMemcpyDeviceToHost, main.get()),
                 "EMFusion::plan (goal costs)");
        if (capacity > 0)
            hipCheck(hipMemcpyAsync(paths.data(), plPaths.data(), paths.size() * sizeof(int32_t), hipMemcpyDeviceToHost, main.get()),
                     "EMFusion::plan (paths)");
    }
    main.waitForCompletion();
    out.goals.resize(nGoals);
    for (size_t g = 0; g < nGoals; ++g) {
        Plan::Goal& r = out.goals[g];
        r.voxel = goalVoxels[g];
        r.cost = goalCost[g];
        r.length = lengths[g];
        const int kept = std::min(std::max(r.length, 0), capacity);
        r.path.assign(paths.begin() + static_cast<size_t>(g) * capacity, paths.begin() + static_cast<size_t>(g) * capacity + kept);
        for (int k = 0; k + 1 < kept; ++k) {
            const Vec3i a = box.unravel(r.path[k]), b = box.unravel(r.path[k + 1]);
            const int moved = std::abs(a[0] - b[0]) + std::abs(a[1] - b[1]) + std::abs(a[2] - b[2]);
            (moved == 1 ? r.faces : moved == 2 ? r.edges : r.corners) += 1;
        }
    }
    out.classes = classes;
    out.cost = cost;
    plLast = std::move(out);
    return plLast;
}

Vec3i EMFusion::cameraVoxel() const {
    const Vec3i n = background.getVolumeRes();
    double v[3];
    queryBoxAt(Vec3i(0, 0, 0), n).voxelAt(pose.translation().val, v);
    // a camera outside the background (both apps place the volume's near face half a voxel behind the first
    // camera, so tracking leaves it a hair outside as often as inside): the nearest voxel of the background
    Vec3i out;
    for (int i = 0; i < 3; ++i) out.val[i] = static_cast<int>(std::min(std::max(v[i], 0.0), static_cast<double>(n[i] - 1)));
    return out;
}

// plan.txt of the whole background (setPlanOutput): the kept frontier clusters (setFrontierOutput's min_voxels, this
// plan's clearance) as goals, from the voxel under the camera.  After a comment line, per cluster in the order of
// frontiers.txt (largest first) one line
//     count reachable cost length_m rx ry rz n_path
// count: voxels of the cluster, %d; reachable 0 / 1; cost %u (the chamfer cost; 4294967295 / 4294967294 where there is
// no path); length_m = (faces + sqrt(2) edges + sqrt(3) corners) * voxel in double, %.9g; r: the representative in the
// world frame as in frontiers.txt; then n_path lines "x y z", the path's voxels in the world frame from the goal to the
// start, each the double value rounded once to float, %.9g.  With setPlanShortcutOutput(W > 0) the path lines of a
// reachable cluster are followed by one line "waypoints n i_0 .. i_(n-1)", shortcutPlan(W) of that path.
void EMFusion::writePlan(const std::string& dir) {
    Vec3i lo, n;  // the whole background; the world extent with setQueryExtent(true)
    resultsBox("writePlan", lo, n);
    const float voxel = background.getVoxelSize();
    const int clearance = metresToVoxels(planClearanceMetres_, voxel);
    const Frontiers& f = frontiers(lo, n, std::max(frontierMinVoxels_, 1), clearance, {});  // as writeFrontiers
    std::vector<Vec3i> goals;
    for (const emf_frontier_cluster_t& c : f.clusters) goals.push_back(Vec3i(c.rep[0], c.rep[1], c.rep[2]));
    const Vec3i cam = cameraVoxel();  // of the background; the start is a voxel of the box
    plan(lo, n, {Vec3i(cam[0] - lo[0], cam[1] - lo[1], cam[2] - lo[2])}, std::max(clearance, 1), planThroughUnknown_, clearance, 0u, goals, -1, {});
    const Plan& p = planShortcutWindow_ > 0 ? shortcutPlan(planShortcutWindow_) : lastPlan();
    const std::string path = dir + "/plan.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writePlan: cannot create " + path);
    std::fprintf(file, "# count reachable cost length_m rep_x rep_y rep_z n_path, then n_path lines x y z from the goal to the start\n");
    if (queryWorld_)  // as frontiers.txt
        std::fprintf(file, "# world extent: lo %d %d %d size %d %d %d\n", lo[0], lo[1], lo[2], n[0], n[1], n[2]);
    for (size_t k = 0; k < f.clusters.size(); ++k) {
        const Plan::Goal& g = p.goals[k];
        double r[3];
        frontierWorldPoint(f, f.clusters[k], true, r);
        const double length = (static_cast<double>(g.faces) + std::sqrt(2.0) * static_cast<double>(g.edges) +
                               std::sqrt(3.0) * static_cast<double>(g.corners)) * static_cast<double>(voxel);
        std::fprintf(file, "%d %d %u %.9g %.9g %.9g %.9g %d\n", f.clusters[k].count, g.length > 0 ? 1 : 0, g.cost, length,
                     static_cast<double>(static_cast<float>(r[0])), static_cast<double>(static_cast<float>(r[1])),
                     static_cast<double>(static_cast<float>(r[2])), static_cast<int>(g.path.size()));
        for (int32_t v : g.path) {
            double w[3];
            p.box.worldPoint(p.box.unravel(v), w);
            std::fprintf(file, "%.9g %.9g %.9g\n", static_cast<double>(static_cast<float>(w[0])),
                         static_cast<double>(static_cast<float>(w[1])), static_cast<double>(static_cast<float>(w[2])));
        }
        if (planShortcutWindow_ > 0 && g.length > 0) {  // "waypoints n i_0 .. i_(n-1)": indices into the path lines above
            std::fprintf(file, "waypoints %d", static_cast<int>(g.waypoints.size()));
            for (int32_t i : g.waypoints) std::fprintf(file, " %d", i);
            std::fprintf(file, "\n");
        }
    }
    std::fclose(file);
}

}  // namespace emf
