// EMFusionRays.cpp -- emf::EMFusion: voxel rays over the scene (new behaviour).  Line of sight between
// voxels, the unknown space a candidate view would see, and shortcuts of the last plan's paths: all three walk straight
// lines through the occupancy classes of a box of the background -- formed exactly as the other scene queries form them
// -- with emf_hip_castVoxelRays (include/emf_hip.h "Voxel rays") on the main stream, in buffers of their own.
// Floating point appears once, in viewRayTargets: float64 in a fixed operation order, on the host, without a device.
// This unit is compiled with a*b+c contraction off.
#include "EMFusion.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace emf {

namespace {

// a double that is a whole number or not finite -> i32: clipped to the range, -1 where it is not finite (the rule of the
// Python layer's to_voxels: a point that is no point lies outside every box)
int32_t toInt32(double v) {
    if (!std::isfinite(v)) return -1;
    return static_cast<int32_t>(std::min(std::max(v, -2147483648.0), 2147483647.0));
}

}  // namespace

void viewRayTargets(const double R[9], const double t[3], double fx, double fy, double cx, double cy, int gw, int gh, double range,
                    const float bgR[9], const float bgT[3], const Vec3i& bgRes, float voxelSize, const Vec3i& boxLo,
                    int32_t origin[3], int32_t* targets) {
    if (!R || !t || !bgR || !bgT || !origin || (!targets && gw > 0 && gh > 0))
        throw HipError("viewRayTargets: a NULL argument", EMF_E_ARG);
    if (gw < 0 || gh < 0 || static_cast<long long>(gw) * gh > 0x7fffffffll / 3)
        throw HipError("viewRayTargets: a grid of " + std::to_string(gw) + " x " + std::to_string(gh), EMF_E_ARG);
    if (!(voxelSize > 0.f) || !(range >= 0.0)) throw HipError("viewRayTargets: voxel size or range", EMF_E_ARG);
    const double voxel = static_cast<double>(voxelSize);
    const double scale = range / voxel;
    if (!(scale <= static_cast<double>(EMF_RAY_MAX_DELTA)))
        throw HipError("viewRayTargets: a range of more than " + std::to_string(EMF_RAY_MAX_DELTA) + " voxels", EMF_E_ARG);
    double B[9];
    for (int i = 0; i < 9; ++i) B[i] = static_cast<double>(bgR[i]);
    // the origin: rint(bgR^T (t - bgT) / voxel + (res - 1) / 2) - lo, the sums left to right
    double o[3];
    for (int i = 0; i < 3; ++i) {
        const double d0 = t[0] - static_cast<double>(bgT[0]), d1 = t[1] - static_cast<double>(bgT[1]),
                     d2 = t[2] - static_cast<double>(bgT[2]);
        double q = d0 * B[i];
        q = q + d1 * B[3 + i];
        q = q + d2 * B[6 + i];
        const double half = (static_cast<double>(bgRes[i]) - 1.0) / 2.0;
        o[i] = std::nearbyint(q / voxel + half) - static_cast<double>(boxLo[i]);
        origin[i] = toInt32(o[i]);
    }
    // M = bgR^T R, once per view
    double M[9];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            double m = B[i] * R[k];
            m = m + B[3 + i] * R[3 + k];
            m = m + B[6 + i] * R[6 + k];
            M[3 * i + k] = m;
        }
    for (int j = 0; j < gh; ++j)
        for (int i = 0; i < gw; ++i) {
            const double x = (static_cast<double>(i) - cx) / fx, y = (static_cast<double>(j) - cy) / fy;
            double s = x * x;
            s = s + y * y;
            s = s + 1.0;
            const double m = std::sqrt(s);
            const double c[3] = {x / m, y / m, 1.0 / m};
            int32_t* out = targets + 3 * (static_cast<size_t>(j) * gw + i);
            for (int a = 0; a < 3; ++a) {
                double d = M[3 * a] * c[0];
                d = d + M[3 * a + 1] * c[1];
                d = d + M[3 * a + 2] * c[2];
                const double step = std::nearbyint(d * scale);  // ties to even
                out[a] = toInt32(static_cast<double>(origin[a]) + step);
            }
        }
}

const EMFusion::Rays& EMFusion::castRays(const Vec3i& boxLo, const Vec3i& boxSize, const int32_t* from, const int32_t* to, int n,
                                         uint32_t passMask, uint32_t countMask, int clearanceVoxels,
                                         const std::vector<int>& excludeIds, int group, bool wantResults) {
    const QueryBox box = makeQueryBox("castRays", "casting rays is", boxLo, boxSize);
    if (n < 0 || (n > 0 && (!from || !to))) throw HipError("EMFusion::castRays: " + std::to_string(n) + " rays without a list", EMF_E_ARG);
    if (n > 0x7fffffff / 3) throw HipError("EMFusion::castRays: too many rays", EMF_E_LIMIT);
    if (passMask > 7u || countMask > 7u) throw HipError("EMFusion::castRays: a mask outside 0 .. 7", EMF_E_ARG);
    if (clearanceVoxels < 0) throw HipError("EMFusion::castRays: a negative clearance", EMF_E_ARG);
    if (group < 0) throw HipError("EMFusion::castRays: a negative group", EMF_E_ARG);
    if (group == 0 && !wantResults) throw HipError("EMFusion::castRays: neither records nor groups asked for", EMF_E_ARG);
    drainForQuery();
    ryLast = Rays();
    Rays out;
    out.box = box;
    out.clearanceVoxels = clearanceVoxels;
    out.passMask = passMask;
    out.countMask = countMask;
    out.group = group;
    const size_t un = static_cast<size_t>(n);
    out.from.assign(from, from + 3 * un);
    out.to.assign(to, to + 3 * un);
    ryClasses.reserve(box.voxels());
    uint8_t* classes = ryClasses.as<uint8_t>();
    enqueueOccupancy("castRays", box, excludeIds, classes, nullptr, nullptr);
    const Clearance clear = enqueueClearance("castRays", box, classes, clearanceVoxels);
    castOnDevice("castRays", box, classes, clear, passMask, countMask, out.from, out.to, group, wantResults, out.results, out.groups);
    ryLast = std::move(out);
    return ryLast;
}

// uploads the rays, launches once, copies the records back and waits once
void EMFusion::castOnDevice(const char* who, const QueryBox& box, const uint8_t* classes, const Clearance& clear, uint32_t passMask,
                            uint32_t countMask, const std::vector<int32_t>& from, const std::vector<int32_t>& to, int group,
                            bool wantResults, std::vector<emf_ray_result_t>& results, std::vector<emf_ray_group_t>& groups) {
    const std::string name = std::string("EMFusion::") + who;
    const size_t un = from.size() / 3;
    const size_t nGroups = group > 0 ? (un + group - 1) / group : 0;
    results.assign(wantResults ? un : 0, emf_ray_result_t{});
    groups.assign(nGroups, emf_ray_group_t{});
    if (un == 0) return;
    ryEnds.reserve(6 * un * sizeof(int32_t));
    if (wantResults) ryResults.reserve(un * sizeof(emf_ray_result_t));
    if (nGroups) ryGroups.reserve(nGroups * sizeof(emf_ray_group_t));
    int32_t* dFrom = ryEnds.as<int32_t>();
    int32_t* dTo = dFrom + 3 * un;
    hipCheck(hipMemcpyAsync(dFrom, from.data(), 3 * un * sizeof(int32_t), hipMemcpyHostToDevice, main.get()), (name + " (origins)").c_str());
    hipCheck(hipMemcpyAsync(dTo, to.data(), 3 * un * sizeof(int32_t), hipMemcpyHostToDevice, main.get()), (name + " (targets)").c_str());
    emfCheck(emf_hip_castVoxelRays(classes, box.size.val, clear.d2, clear.minD2, passMask, countMask, dFrom, dTo, static_cast<int32_t>(un),
                                   wantResults ? ryResults.as<emf_ray_result_t>() : nullptr, group,
                                   nGroups ? ryGroups.as<emf_ray_group_t>() : nullptr, main.abi()),
             name.c_str());
    if (wantResults)
        hipCheck(hipMemcpyAsync(results.data(), ryResults.data(), un * sizeof(emf_ray_result_t), hipMemcpyDeviceToHost, main.get()),
                 (name + " (records)").c_str());
    if (nGroups)
        hipCheck(hipMemcpyAsync(groups.data(), ryGroups.data(), nGroups * sizeof(emf_ray_group_t), hipMemcpyDeviceToHost, main.get()),
                 (name + " (groups)").c_str());
    main.waitForCompletion();
}

const EMFusion::Rays& EMFusion::viewGain(const std::vector<ViewPose>& views, int gw, int gh, const double K[4], double range,
                                         const Vec3i& boxLo, const Vec3i& boxSize, const std::vector<int>& excludeIds,
                                         bool wantResults) {
    const QueryBox box = makeQueryBox("viewGain", "view gain is", boxLo, boxSize);
    if (gw < 1 || gh < 1 || !K) throw HipError("EMFusion::viewGain: a grid of " + std::to_string(gw) + " x " + std::to_string(gh), EMF_E_ARG);
    const size_t per = static_cast<size_t>(gw) * gh;
    if (per > 0x7fffffffull / 3 || per * views.size() > 0x7fffffffull / 3) throw HipError("EMFusion::viewGain: too many rays", EMF_E_LIMIT);
    std::vector<int32_t> from(3 * per * views.size()), to(3 * per * views.size()), origins(3 * views.size());
    for (size_t v = 0; v < views.size(); ++v) {
        int32_t* o = origins.data() + 3 * v;
        viewRayTargets(views[v].R, views[v].t, K[0], K[1], K[2], K[3], gw, gh, range, box.bgPose.rotation().val,
                       box.bgPose.translation().val, box.bgRes, box.voxelSize, box.lo, o, to.data() + 3 * per * v);
        for (size_t k = 0; k < per; ++k) std::copy(o, o + 3, from.data() + 3 * (per * v + k));
    }
    castRays(boxLo, boxSize, from.data(), to.data(), static_cast<int>(per * views.size()),
             (1u << EMF_OCC_FREE) | (1u << EMF_OCC_UNKNOWN), 1u << EMF_OCC_UNKNOWN, 0, excludeIds, static_cast<int>(per), wantResults);
    ryLast.origins = std::move(origins);
    ryLast.gridW = gw;
    ryLast.gridH = gh;
    return ryLast;
}

std::vector<int32_t> shortcutGreedy(int k, int window, const std::vector<uint8_t>& reached, const std::vector<size_t>& rowStart) {
    std::vector<int32_t> way;
    if (k < 0) return way;
    way.push_back(0);
    int i = 0;
    while (i < k) {
        int next = i + 1;  // a step of the planner's own path: accepted untested
        const int hi = std::min(i + window, k);
        for (int j = hi; j >= i + 2; --j)
            if (reached[rowStart[i] + static_cast<size_t>(j - i - 2)]) {
                next = j;
                break;
            }
        way.push_back(next);
        i = next;
    }
    return way;
}

const EMFusion::Plan& EMFusion::shortcutPlan(int window) {
    if (sharded || world > 1) throw HipError("EMFusion::shortcutPlan: planning is not supported on the sharded path", EMF_E_ARG);
    if (window < 1) throw HipError("EMFusion::shortcutPlan: a window of " + std::to_string(window), EMF_E_ARG);
    if (!plLast.cost) throw HipError("EMFusion::shortcutPlan: no plan has been computed", EMF_E_ARG);
    Plan& p = plLast;
    // the rays p_i -> p_j of every goal, 2 <= j - i <= window, row by row
    std::vector<int32_t> from, to;
    std::vector<std::vector<size_t>> rowStart(p.goals.size());
    size_t count = 0;
    for (size_t g = 0; g < p.goals.size(); ++g) {
        const std::vector<int32_t>& path = p.goals[g].path;
        const int k = static_cast<int>(path.size()) - 1;
        rowStart[g].assign(std::max(k, 0) + 1, 0);
        for (int i = 0; i <= k; ++i) {
            rowStart[g][i] = count;
            const Vec3i a = p.box.unravel(path[i]);
            for (int j = i + 2; j <= std::min(i + window, k); ++j, ++count) {
                const Vec3i b = p.box.unravel(path[j]);
                from.insert(from.end(), a.val, a.val + 3);
                to.insert(to.end(), b.val, b.val + 3);
            }
        }
    }
    if (count > 0x7fffffffull / 3) throw HipError("EMFusion::shortcutPlan: too many rays", EMF_E_LIMIT);
    std::vector<emf_ray_result_t> results;
    std::vector<emf_ray_group_t> groups;
    if (count) {
        drainForQuery();
        Clearance clear{nullptr, 0};
        if (p.clearanceVoxels > 0) {
            // the plan's own gate: still in the shared scratch unless another query has used it since
            if (clearanceSerial == plClearanceSerial) {
                const int cap = std::min(p.clearanceVoxels, 4095);
                clear = Clearance{clearanceD2.as<int32_t>(), cap * cap};
            } else {
                clear = enqueueClearance("shortcutPlan", p.box, p.classes, p.clearanceVoxels);
                plClearanceSerial = clearanceSerial;
            }
        }
        const uint32_t mask = (1u << EMF_OCC_FREE) | (p.throughUnknown ? 1u << EMF_OCC_UNKNOWN : 0u);
        castOnDevice("shortcutPlan", p.box, p.classes, clear, mask, 0u, from, to, 0, true, results, groups);
    }
    std::vector<uint8_t> reached(count);
    for (size_t r = 0; r < count; ++r) reached[r] = results[r].status == EMF_RAY_REACHED;
    for (size_t g = 0; g < p.goals.size(); ++g)
        p.goals[g].waypoints = shortcutGreedy(static_cast<int>(p.goals[g].path.size()) - 1, window, reached, rowStart[g]);
    plShortcutWindow = window;
    return p;
}

}  // namespace emf
