// EMFusionPlanes.cpp -- emf::EMFusion: planes (new behaviour).  The dominant planes of a box of the
// background -- floor, walls, table tops -- by a three-stage vote on the TSDF gradients of the surface voxels
// (include/emf_hip.h "Planes"): direction votes, offset votes along the chosen directions, assignment with integer
// moments and a least-squares refit.  The decisions between the stages are taken here on the host: float64, one
// operation per line in the order include/emf_fusion.h "Planes" states, and this unit is compiled with a*b+c
// contraction off.  planeDirections, planeOffsetFrame, planePeaks and planeFit need no device.
#include "EMFusion.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace emf {

namespace {

constexpr double kPi = 3.141592653589793;
constexpr double kSupportGap = 0.05;  // metres: the policy of the support lines of planes.txt

double dot3(const double a[3], const double b[3]) {
    double s = a[0] * b[0];
    s = s + a[1] * b[1];
    s = s + a[2] * b[2];
    return s;
}

}  // namespace

void planeCellCentre(int b, int K, double n[3]) {
    const int face = b / (K * K), iv = b / K % K, iu = b % K;
    const int m = face / 2;
    const double half = static_cast<double>(K) / 2.0;
    double c[3] = {0.0, 0.0, 0.0};
    c[m] = face % 2 ? -1.0 : 1.0;
    c[(m + 1) % 3] = (static_cast<double>(iu) + 0.5) / half - 1.0;
    c[(m + 2) % 3] = (static_cast<double>(iv) + 0.5) / half - 1.0;
    const double norm = std::sqrt(dot3(c, c));
    for (int j = 0; j < 3; ++j) n[j] = c[j] / norm;
}

std::vector<PlaneDirection> planeDirections(const uint32_t* bins, int K, uint32_t minVotes, double separationDeg) {
    const int nb = 6 * K * K;
    std::vector<int> order(static_cast<size_t>(nb));
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bins[a] > bins[b]; });  // ties to the lower bin
    const double limit = std::cos(separationDeg * kPi / 180.0);
    std::vector<PlaneDirection> chosen;
    for (int b : order) {
        if (bins[b] < minVotes || chosen.size() == EMF_PLANE_MAX_DIRS) break;
        PlaneDirection d;
        d.bin = b;
        d.votes = bins[b];
        planeCellCentre(b, K, d.n);
        bool close = false;
        for (const PlaneDirection& c : chosen) close = close || dot3(d.n, c.n) > limit;
        if (!close) chosen.push_back(d);
    }
    return chosen;
}

PlaneOffsetFrame planeOffsetFrame(const double n[3], const int32_t size[3], double binVox) {
    double lo = INFINITY, hi = -INFINITY;
    for (int k = 0; k < 8; ++k) {  // the corners of the voxel cubes, x fastest
        double b[3];
        for (int j = 0; j < 3; ++j) b[j] = (k >> j) & 1 ? static_cast<double>(size[j]) - 0.5 : -0.5;
        const double s = dot3(n, b);
        lo = std::min(lo, s);
        hi = std::max(hi, s);
    }
    PlaneOffsetFrame f;
    f.lo = lo;
    const double span = hi - lo;
    f.slots = static_cast<int64_t>(std::floor(span / binVox)) + 1;
    f.invBin = 1.0 / binVox;
    f.shift = -lo * f.invBin;
    return f;
}

std::vector<std::pair<int, uint32_t>> planePeaks(const uint32_t* row, int slots, uint32_t minVotes, int peakGap) {
    std::vector<int> order(static_cast<size_t>(slots));
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return row[a] > row[b]; });
    std::vector<std::pair<int, uint32_t>> chosen;
    for (int s : order) {
        if (row[s] < minVotes) break;
        bool close = false;
        for (const auto& c : chosen) close = close || std::abs(s - c.first) <= peakGap;
        if (!close) chosen.emplace_back(s, row[s]);
    }
    return chosen;
}

void planeFit(const emf_plane_moments_t& mom, const double seedN[3], double seedD, emf_plane_t& out) {
    std::memset(&out, 0, sizeof(out));
    out.count = mom.count;
    for (int j = 0; j < 3; ++j) out.lo[j] = mom.lo[j], out.hi[j] = mom.hi[j];
    if (mom.count < 3) {  // the seed stays
        for (int j = 0; j < 3; ++j) out.n[j] = seedN[j];
        out.d = seedD;
        return;
    }
    emf_shape_moments_t sm{};
    sm.solid = mom.count;
    for (int j = 0; j < 3; ++j) sm.sum[j] = mom.sum[j];
    for (int j = 0; j < 6; ++j) sm.sum2[j] = mom.sum2[j];
    emf_shape_frame_t fr;
    std::memset(&fr, 0, sizeof(fr));
    shapeFrame(sm, fr);  // centroid, covariance and Jacobi frame of the object shapes, called, not restated
    const double* a = fr.axes + 6;  // the axis of the smallest eigenvalue
    const bool flip = dot3(a, seedN) < 0.0;
    for (int j = 0; j < 3; ++j) {
        out.n[j] = flip ? -a[j] : a[j];
        out.centroid[j] = fr.centroid[j];
        out.eigenvalues[j] = fr.eigenvalues[j];
    }
    for (int j = 0; j < 6; ++j) out.axes[j] = fr.axes[j];
    out.d = dot3(out.n, out.centroid);
    out.thickness = std::sqrt(std::max(fr.eigenvalues[2], 0.0));
    out.fitted = 1;
}

void planePatchRect(const emf_plane_t& plane, const emf_plane_patch_t& patch, emf_plane_patch_rect_t& out) {
    std::memset(&out, 0, sizeof(out));
    emf_plane_moments_t mom{};
    mom.count = patch.count;
    for (int j = 0; j < 3; ++j) mom.sum[j] = patch.sum[j], mom.lo[j] = patch.lo[j], mom.hi[j] = patch.hi[j];
    for (int j = 0; j < 6; ++j) mom.sum2[j] = patch.sum2[j];
    planeFit(mom, plane.n, plane.d, out.fit);  // called, not restated
    out.fit.label = plane.label;
    const double* u = plane.axes;
    const double* v = plane.axes + 3;
    const double a0 = static_cast<double>(patch.ulo) - 0.5;
    const double a1 = static_cast<double>(patch.uhi) + 0.5;
    const double b0 = static_cast<double>(patch.vlo) - 0.5;
    const double b1 = static_cast<double>(patch.vhi) + 0.5;
    const double su = a0 + a1, cu = su * 0.5;
    const double du = a1 - a0, hu = du * 0.5;
    const double sv = b0 + b1, cv = sv * 0.5;
    const double dv = b1 - b0, hv = dv * 0.5;
    auto point = [&](double eu, double ev, double* p) {
        for (int j = 0; j < 3; ++j) {
            double s = plane.d * plane.n[j];
            double t = u[j] * eu;
            s = s + t;
            t = v[j] * ev;
            s = s + t;
            p[j] = s;
        }
    };
    point(cu, cv, out.center);
    out.half[0] = hu, out.half[1] = hv;
    const double sign[4][2] = {{-1.0, -1.0}, {1.0, -1.0}, {1.0, 1.0}, {-1.0, 1.0}};
    for (int k = 0; k < 4; ++k) {
        const double ou = sign[k][0] * hu, ov = sign[k][1] * hv;
        const double eu = cu + ou, ev = cv + ov;
        point(eu, ev, out.corners + 3 * k);
    }
    double wu = static_cast<double>(patch.uhi) - static_cast<double>(patch.ulo);
    wu = wu + 1.0;
    double wv = static_cast<double>(patch.vhi) - static_cast<double>(patch.vlo);
    wv = wv + 1.0;
    const double nmax = std::max(std::fabs(plane.n[0]), std::max(std::fabs(plane.n[1]), std::fabs(plane.n[2])));
    double area = wu * wv;
    area = area * nmax;
    out.fill = static_cast<double>(patch.count) / area;
}

bool planeSupport(const double n[3], double d, const double center[3], const double axes[6], const double half[2],
                  const double boxCenter[3], const double boxAxes[9], const double boxHalf[3], double margin, double& s) {
    s = dot3(n, boxCenter);
    s = s - d;
    for (int k = 0; k < 3; ++k) {
        const double a = dot3(n, boxAxes + 3 * k);
        const double r = std::fabs(a) * boxHalf[k];
        s = s - r;
    }
    const double q[3] = {boxCenter[0] - center[0], boxCenter[1] - center[1], boxCenter[2] - center[2]};
    bool over = true;
    for (int j = 0; j < 2; ++j) {
        const double a = dot3(q, axes + 3 * j);
        const double reach = half[j] + margin;
        over = over && std::fabs(a) <= reach;
    }
    return over;
}

const EMFusion::PlanePatches& EMFusion::planePatches(int reach, int64_t minCount) {
    if (sharded || world > 1) throw HipError("EMFusion::planePatches: the plane search is not supported on the sharded path", EMF_E_ARG);
    if (!pnLast.records) throw HipError("EMFusion::planePatches: no planes have been computed", EMF_E_ARG);
    if (reach < 1 || reach > EMF_PLANE_MAX_REACH)
        throw HipError("EMFusion::planePatches: a reach outside 1 .. 2", reach < 1 ? EMF_E_ARG : EMF_E_LIMIT);
    if (minCount < 1) throw HipError("EMFusion::planePatches: min_count below 1", EMF_E_ARG);
    PlanePatches out;
    out.reach = reach, out.minCount = minCount;
    ppLast = PlanePatches();  // a call that throws leaves no result
    if (!pnLast.labels) {     // no plane: no member, no patch
        ppLast = out;
        return ppLast;
    }
    int P = 0;
    for (const emf_plane_t& p : pnLast.planes) P = std::max(P, p.label + 1);
    std::vector<float> axes(6 * static_cast<size_t>(P), 0.f);
    for (const emf_plane_t& p : pnLast.planes)
        for (int j = 0; j < 6; ++j) axes[6 * static_cast<size_t>(p.label) + j] = static_cast<float>(p.axes[j]);
    const uint32_t capacity = pnCapacity;
    auto* dCounters = pnSmall.as<uint32_t>();
    ppIds.reserve(static_cast<size_t>(capacity) * sizeof(int32_t));
    ppSmall.reserve(16);
    auto* dPc = ppSmall.as<uint32_t>();
    emfCheck(emf_hip_planePatchLabel(pnLast.records, pnLast.labels, dCounters, capacity, pnLast.box.size.val, reach, ppIds.as<int32_t>(),
                                     dPc, main.abi()), "EMFusion::planePatches (label)");
    hipCheck(hipMemcpyAsync(out.counters, dPc, 12, hipMemcpyDeviceToHost, main.get()), "EMFusion::planePatches (counters)");
    main.waitForCompletion();  // wait 1: the scratch and the records are sized by the number of patches
    const uint32_t nPatches = out.counters[EMF_PATCH_PATCHES];
    out.ids = ppIds.as<int32_t>();
    if (nPatches == 0u) {
        ppLast = out;
        return ppLast;
    }
    ppScratch.reserve(std::max<size_t>(emf_hip_planePatchScratchBytes(capacity, nPatches), 16));
    ppOut.reserve(static_cast<size_t>(nPatches) * sizeof(emf_plane_patch_t));
    emfCheck(emf_hip_planePatches(pnLast.records, pnLast.labels, ppIds.as<int32_t>(), dCounters, capacity, pnLast.box.size.val,
                                  axes.data(), P, minCount, nPatches, ppScratch.data(), ppOut.as<emf_plane_patch_t>(),
                                  static_cast<int32_t>(std::min<uint32_t>(nPatches, 0x7fffffffu)), dPc, main.abi()),
             "EMFusion::planePatches (records)");
    out.patches.resize(nPatches);
    hipCheck(hipMemcpyAsync(out.counters, dPc, 12, hipMemcpyDeviceToHost, main.get()), "EMFusion::planePatches (kept)");
    hipCheck(hipMemcpyAsync(out.patches.data(), ppOut.data(), static_cast<size_t>(nPatches) * sizeof(emf_plane_patch_t),
                            hipMemcpyDeviceToHost, main.get()), "EMFusion::planePatches (patches)");
    main.waitForCompletion();  // wait 2: the records
    out.patches.resize(out.counters[EMF_PATCH_KEPT]);  // behind the kept ones nothing was written
    ppLast = out;
    return ppLast;
}

void EMFusion::describePlanePatches(const Planes& r, const PlanePatches& pp, std::vector<PatchWorld>& out) {
    out.clear();
    const float* R = r.box.bgPose.rotation().val;
    const double vs = static_cast<double>(r.box.voxelSize);
    auto rotate = [&](const double* a, double* w) {
        for (int i = 0; i < 3; ++i) {
            double s = static_cast<double>(R[3 * i]) * a[0];
            s = s + static_cast<double>(R[3 * i + 1]) * a[1];
            s = s + static_cast<double>(R[3 * i + 2]) * a[2];
            w[i] = s;
        }
    };
    for (size_t k = 0; k < r.planes.size(); ++k) {
        const emf_plane_t& plane = r.planes[k];
        std::vector<const emf_plane_patch_t*> mine;
        for (const emf_plane_patch_t& p : pp.patches)
            if (p.plane == plane.label) mine.push_back(&p);
        std::stable_sort(mine.begin(), mine.end(), [](const emf_plane_patch_t* a, const emf_plane_patch_t* b) { return a->count > b->count; });
        for (const emf_plane_patch_t* p : mine) {
            PatchWorld w;
            w.plane = static_cast<int>(k), w.id = p->id;
            planePatchRect(plane, *p, w.rect);
            const emf_plane_t& f = w.rect.fit;
            rotate(f.n, w.normal);
            double m[3];
            for (int i = 0; i < 3; ++i) m[i] = f.fitted ? f.centroid[i] : f.n[i] * f.d;  // a point of the patch's plane
            r.box.worldPoint(m, w.point);
            w.d = dot3(w.normal, w.point);
            r.box.worldPoint(w.rect.center, w.center);
            rotate(plane.axes, w.axes);
            rotate(plane.axes + 3, w.axes + 3);
            w.halfM[0] = w.rect.half[0] * vs, w.halfM[1] = w.rect.half[1] * vs;
            for (int c = 0; c < 4; ++c) r.box.worldPoint(w.rect.corners + 3 * c, w.corners + 3 * c);
            out.push_back(w);
        }
    }
}

const EMFusion::Planes& EMFusion::planes(const Vec3i& boxLo, const Vec3i& boxSize, const emf_plane_params_t& p, bool keepLabels) {
    Planes out;
    out.box = makeQueryBox("planes", "the plane search is", boxLo, boxSize, true);  // tsdf values: the volume only
    pnLast = Planes();  // a call that throws leaves no result: the buffers of the last one are about to be rewritten
    ppLast = PlanePatches();  // ... and the patches of the last one are those of records that are about to go
    if (p.K < 1 || p.K > EMF_PLANE_MAX_K) throw HipError("EMFusion::planes: K outside 1 .. 31", p.K < 1 ? EMF_E_ARG : EMF_E_LIMIT);
    if (p.refine < 0 || p.max_planes < 1 || p.max_planes > EMF_PLANE_MAX_PLANES || p.peak_gap < 0)
        throw HipError("EMFusion::planes: refine, max_planes or peak_gap outside its range", EMF_E_ARG);
    if (!(p.angle_deg > 0.0 && p.angle_deg <= 90.0) || !(p.bin_vox > 0.0) || !(p.band_vox >= 0.0))
        throw HipError("EMFusion::planes: an angle outside (0, 90], a bin that is not positive or a negative band", EMF_E_ARG);
    const double separation = p.separation_deg > 0.0 ? p.separation_deg : p.angle_deg;
    const double c = std::cos(p.angle_deg * kPi / 180.0);
    const float cos2 = static_cast<float>(c * c);
    drainForQuery();
    emf_model_t bg{};
    background.describe(bg);
    const size_t voxels = out.box.voxels();
    // a surface is about one voxel in a hundred; an eighth of the box (at least 2^16 records) holds any scene worth asking
    const uint32_t capacity = static_cast<uint32_t>(std::min(voxels, std::max<size_t>(size_t(1) << 16, voxels / 8)));
    pnCapacity = capacity;
    const size_t nb = 6 * static_cast<size_t>(p.K) * p.K;
    const size_t histWords = static_cast<size_t>(EMF_PLANE_MAX_DIRS) * EMF_PLANE_MAX_SLOTS;
    pnRecords.reserve(static_cast<size_t>(capacity) * sizeof(emf_plane_voxel_t));
    pnLabels.reserve(static_cast<size_t>(capacity) * sizeof(int16_t));
    pnScratch.reserve(std::max<size_t>(emf_hip_planeSurfaceScratchBytes(out.box.size.val), 16));
    // counters (16 bytes), the moments, then the larger of the bins and the offset histogram
    const size_t momBytes = EMF_PLANE_MAX_PLANES * sizeof(emf_plane_moments_t);
    pnSmall.reserve(16 + momBytes + std::max(nb, histWords) * sizeof(uint32_t));
    auto* dCounters = pnSmall.as<uint32_t>();
    auto* dMom = reinterpret_cast<emf_plane_moments_t*>(pnSmall.as<uint8_t>() + 16);
    auto* dVotes = reinterpret_cast<uint32_t*>(pnSmall.as<uint8_t>() + 16 + momBytes);
    auto* dRec = pnRecords.as<emf_plane_voxel_t>();
    auto finish = [&]() -> const Planes& {
        out.records = dRec;
        out.labels = out.planes.empty() ? nullptr : pnLabels.as<int16_t>();
        out.keptLabels = keepLabels;
        pnLast = out;
        return pnLast;
    };

    emfCheck(emf_hip_planeSurface(bg.tsdf, bg.weights, bg.res, out.box.lo.val, out.box.size.val, bg.unseenTiles, dRec, capacity,
                                  dCounters, pnScratch.data(), main.abi()), "EMFusion::planes (surface)");
    emfCheck(emf_hip_planeDirections(dRec, dCounters, capacity, p.K, dVotes, main.abi()), "EMFusion::planes (directions)");
    std::vector<uint32_t> votes(std::max(nb, histWords));
    hipCheck(hipMemcpyAsync(out.counters, dCounters, 16, hipMemcpyDeviceToHost, main.get()), "EMFusion::planes (counters)");
    hipCheck(hipMemcpyAsync(votes.data(), dVotes, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, main.get()), "EMFusion::planes (bins)");
    main.waitForCompletion();  // wait 1: the directions come from the bins
    const uint32_t minVotes = p.min_votes > 0 ? static_cast<uint32_t>(std::min<int64_t>(p.min_votes, 0xffffffffll))
                                              : std::max<uint32_t>(50u, out.counters[2] / 200u);
    out.minVotes = minVotes;
    const std::vector<PlaneDirection> dirs = planeDirections(votes.data(), p.K, minVotes, separation);
    if (dirs.empty()) return finish();

    const int D = static_cast<int>(dirs.size());
    std::vector<PlaneOffsetFrame> frames;
    std::vector<float> dirF(3 * dirs.size()), shiftF(dirs.size());
    int64_t S = 1;
    for (int k = 0; k < D; ++k) {
        frames.push_back(planeOffsetFrame(dirs[k].n, out.box.size.val, p.bin_vox));
        S = std::max(S, frames[k].slots);
        for (int j = 0; j < 3; ++j) dirF[3 * k + j] = static_cast<float>(dirs[k].n[j]);
        shiftF[k] = static_cast<float>(frames[k].shift);
    }
    if (S > EMF_PLANE_MAX_SLOTS)
        throw HipError("EMFusion::planes: " + std::to_string(S) + " offset slots, above " + std::to_string(EMF_PLANE_MAX_SLOTS) +
                       ": a wider bin is needed", EMF_E_LIMIT);
    emfCheck(emf_hip_planeOffsets(dRec, dCounters, capacity, out.box.size.val, dirF.data(), shiftF.data(), D, cos2,
                                  static_cast<float>(frames[0].invBin), static_cast<int32_t>(S), dVotes, main.abi()),
             "EMFusion::planes (offsets)");
    hipCheck(hipMemcpyAsync(votes.data(), dVotes, static_cast<size_t>(D) * S * sizeof(uint32_t), hipMemcpyDeviceToHost, main.get()),
             "EMFusion::planes (histogram)");
    main.waitForCompletion();  // wait 2: the seeds come from the histogram
    struct Seed {
        uint32_t votes;
        int dir, slot;
    };
    std::vector<Seed> seeds;
    for (int k = 0; k < D; ++k)
        for (const auto& peak : planePeaks(votes.data() + static_cast<size_t>(k) * S, static_cast<int>(frames[k].slots), minVotes, p.peak_gap))
            seeds.push_back(Seed{peak.second, k, peak.first});
    std::stable_sort(seeds.begin(), seeds.end(), [](const Seed& a, const Seed& b) { return a.votes > b.votes; });  // ties: (direction, slot)
    if (seeds.size() > static_cast<size_t>(p.max_planes)) seeds.resize(static_cast<size_t>(p.max_planes));
    if (seeds.empty()) return finish();

    const int P = static_cast<int>(seeds.size());
    std::vector<emf_plane_t> fits(seeds.size());
    for (int k = 0; k < P; ++k) {
        std::memset(&fits[k], 0, sizeof(emf_plane_t));
        for (int j = 0; j < 3; ++j) fits[k].n[j] = dirs[seeds[k].dir].n[j];
        const double centre = (static_cast<double>(seeds[k].slot) + 0.5) * p.bin_vox;
        fits[k].d = frames[seeds[k].dir].lo + centre;
    }
    std::vector<emf_plane_moments_t> mom(seeds.size());
    std::vector<float> planesF(4 * seeds.size());
    for (int round = 0; round <= p.refine; ++round) {
        for (int k = 0; k < P; ++k) {
            for (int j = 0; j < 3; ++j) planesF[4 * k + j] = static_cast<float>(fits[k].n[j]);
            planesF[4 * k + 3] = static_cast<float>(fits[k].d);
        }
        emfCheck(emf_hip_planeAssign(dRec, dCounters, capacity, out.box.size.val, planesF.data(), P, cos2, static_cast<float>(p.band_vox),
                                     pnLabels.as<int16_t>(), dMom, main.abi()), "EMFusion::planes (assign)");
        hipCheck(hipMemcpyAsync(mom.data(), dMom, seeds.size() * sizeof(emf_plane_moments_t), hipMemcpyDeviceToHost, main.get()),
                 "EMFusion::planes (moments)");
        main.waitForCompletion();  // waits 3 .. 3 + refine: the fit comes from the moments
        for (int k = 0; k < P; ++k) {
            const double seedN[3] = {fits[k].n[0], fits[k].n[1], fits[k].n[2]};
            planeFit(mom[k], seedN, fits[k].d, fits[k]);
            fits[k].label = k;
        }
    }
    std::vector<int> order(seeds.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return fits[a].count > fits[b].count; });
    for (int k : order)
        if (fits[k].count > 0) out.planes.push_back(fits[k]);
    return finish();
}

int EMFusion::describePlanes(const Planes& r, const double upIn[3], double floorAngle, double kindAngle, std::vector<PlaneWorld>& out) {
    const float* R = r.box.bgPose.rotation().val;
    double up[3] = {upIn[0], upIn[1], upIn[2]};
    if (up[0] == 0.0 && up[1] == 0.0 && up[2] == 0.0)
        for (int i = 0; i < 3; ++i) up[i] = -static_cast<double>(R[3 * i + 1]);
    const double norm = std::sqrt(dot3(up, up));
    for (int i = 0; i < 3; ++i) up[i] = up[i] / norm;
    const double vs = static_cast<double>(r.box.voxelSize);
    out.assign(r.planes.size(), PlaneWorld());
    std::vector<double> height(r.planes.size());
    for (size_t k = 0; k < r.planes.size(); ++k) {
        const emf_plane_t& p = r.planes[k];
        PlaneWorld& w = out[k];
        for (int i = 0; i < 3; ++i) {
            double s = static_cast<double>(R[3 * i]) * p.n[0];
            s = s + static_cast<double>(R[3 * i + 1]) * p.n[1];
            s = s + static_cast<double>(R[3 * i + 2]) * p.n[2];
            w.normal[i] = s;
        }
        double m[3];
        for (int i = 0; i < 3; ++i) m[i] = p.fitted ? p.centroid[i] : p.n[i] * p.d;  // a point of the plane
        r.box.worldPoint(m, w.point);
        w.d = dot3(w.normal, w.point);
        w.thicknessM = p.thickness * vs;
        height[k] = dot3(w.point, up);
    }
    const double cosFloor = std::cos(floorAngle * kPi / 180.0);
    const double cosKind = std::cos(kindAngle * kPi / 180.0), sinKind = std::sin(kindAngle * kPi / 180.0);
    int floor = -1;
    for (size_t k = 0; k < out.size(); ++k)
        if (dot3(out[k].normal, up) >= cosFloor && (floor < 0 || height[k] < height[static_cast<size_t>(floor)])) floor = static_cast<int>(k);
    const double* ref = floor < 0 ? up : out[static_cast<size_t>(floor)].normal;
    for (size_t k = 0; k < out.size(); ++k) {
        const double c = dot3(out[k].normal, ref);
        out[k].kind = static_cast<int>(k) == floor ? "floor" : c >= cosKind ? "level" : c <= -cosKind ? "ceiling"
                      : std::fabs(c) <= sinKind ? "wall" : "slope";
    }
    return floor;
}

// planes.txt (setPlanesOutput): after a comment line one line per plane of the whole background, ordered by count:
//     kind count, then in %.9g the world normal (3), d, the point (3), the thickness in metres, then the bounds lo (3) hi (3)
//     in voxels of the background
void EMFusion::writePlanes(const std::string& dir) {
    emf_plane_params_t p{15, 1, EMF_PLANE_MAX_PLANES, 2, expPlanes_.angle, 0.0, 1.0, 2.0, expPlanes_.minVotes};
    const Planes& r = planes(Vec3i(0, 0, 0), background.getVolumeRes(), p, false);
    std::vector<PlaneWorld> world;
    const double up[3] = {0.0, 0.0, 0.0};
    describePlanes(r, up, 30.0, 10.0, world);
    std::vector<PatchWorld> patchWorld;  // stays empty without setPlanePatchesOutput: the file is as before
    std::vector<ObjectShape> shapes;
    if (expPatches_.on) {
        const int64_t minCount = expPatches_.minCount > 0 ? expPatches_.minCount : std::max<int64_t>(25, r.minVotes / 4);
        describePlanePatches(r, planePatches(expPatches_.reach, minCount), patchWorld);
        if (expShapes_) {
            std::vector<int> ids;
            for (const ObjTSDF& obj : objects) ids.push_back(obj.getID());
            std::sort(ids.begin(), ids.end());
            if (!ids.empty()) shapes = objectShapes(ids, false);
        }
    }
    const std::string path = dir + "/planes.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writePlanes: cannot create " + path);
    std::fprintf(file, "# kind count normal_world(3) d point_world(3) thickness_m lo(3) hi(3): the planes of the shell's voxel "
                       "centres, up to one voxel behind the surface\n");
    for (size_t k = 0; k < world.size(); ++k) {
        const PlaneWorld& w = world[k];
        const emf_plane_t& q = r.planes[k];
        std::fprintf(file, "%s %llu", w.kind, static_cast<unsigned long long>(q.count));
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", w.normal[i]);
        std::fprintf(file, " %.9g", w.d);
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", w.point[i]);
        std::fprintf(file, " %.9g %d %d %d %d %d %d\n", w.thicknessM, q.lo[0], q.lo[1], q.lo[2], q.hi[0], q.hi[1], q.hi[2]);
        // setPlanePatchesOutput: "patch" id count, then in %.9g the world point (3), the four corners (12) and fill
        for (const PatchWorld& pw : patchWorld) {
            if (pw.plane != static_cast<int>(k)) continue;
            std::fprintf(file, "patch %d %llu", pw.id, static_cast<unsigned long long>(pw.rect.fit.count));
            for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", pw.point[i]);
            for (int i = 0; i < 12; ++i) std::fprintf(file, " %.9g", pw.corners[i]);
            std::fprintf(file, " %.9g\n", pw.rect.fill);
        }
    }
    // ... and with the shapes output on as well: "support" object plane patch s, per object that rests on a patch
    for (const ObjectShape& s : shapes) {
        if (!s.frame.valid) continue;
        int best = -1;
        double bestS = 0.0;
        for (size_t j = 0; j < patchWorld.size(); ++j) {
            const PatchWorld& pw = patchWorld[j];
            const char* kind = world[static_cast<size_t>(pw.plane)].kind;
            if (std::strcmp(kind, "floor") != 0 && std::strcmp(kind, "level") != 0) continue;
            double h = 0.0;
            const bool over = planeSupport(pw.normal, pw.d, pw.center, pw.axes, pw.halfM, s.box.center_world, s.box.axes_world,
                                           s.box.half_m, 0.0, h);
            if (over && std::fabs(h) <= kSupportGap && (best < 0 || std::fabs(h) < std::fabs(bestS))) best = static_cast<int>(j), bestS = h;
        }
        if (best >= 0)
            std::fprintf(file, "support %d %d %d %.9g\n", s.id, patchWorld[static_cast<size_t>(best)].plane,
                         patchWorld[static_cast<size_t>(best)].id, bestS);
    }
    std::fclose(file);
}

}  // namespace emf
