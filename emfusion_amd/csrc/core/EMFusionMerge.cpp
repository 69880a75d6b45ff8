// EMFusionMerge.cpp -- emf::EMFusion: merging an object into another object (new behaviour), the third
// direction of EMFusionAbsorb.cpp and EMFusionLift.cpp.  A mask that matches no object's raycast segmentation and whose
// volume overlaps no object's box enough gives a physical thing a second volume; nothing repaired that.  mergeObjects
// grows the destination's cube until it holds the source's band (ObjTSDF::resize of the union of both bands), resamples the
// source's band through the relative pose into the destination and fuses it there by the destination's running average,
// the (fg, bg) counts of every fused voxel following the band (emf_hip_mergeVolume, one launch on the main stream; with
// colour emf_hip_mergeVolumeColor), sums the bookkeeping and deletes the source.  With setMergeObjects on, the end of every
// mask frame probes all ordered object pairs in one emf_hip_contactProbe launch and merges the DUPLICATES it finds -- the
// share of one surface that lies on the other's, the older object stays, an object once per frame; two parts that merely
// abut are not found.  mergeUnion is float64 in the fixed
// operation order stated in EMFusion.hpp and needs no device; the poses are absorbPose.  This unit is compiled with a*b+c
// contraction off.
#include "EMFusionDetail.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>
#include <set>

namespace emf {

bool mergeUnion(const int32_t dLo[3], const int32_t dHi[3], const int32_t dRes[3], float dVoxel, const int32_t sLo[3],
                const int32_t sHi[3], const int32_t sRes[3], float sVoxel, const float R[9], const float t[3], float lo[3], float hi[3]) {
    const bool hasD = dHi[0] >= 0, hasS = sHi[0] >= 0;
    if (!hasD && !hasS) return false;
    auto coord = [](int32_t v, int32_t n, float voxel) {
        const double half = (static_cast<double>(n) - 1.0) / 2.0;
        const double off = static_cast<double>(v) - half;
        return off * static_cast<double>(voxel);
    };
    double mn[3], mx[3];
    for (int i = 0; i < 3; ++i) {
        mn[i] = hasD ? coord(dLo[i], dRes[i], dVoxel) : std::numeric_limits<double>::infinity();
        mx[i] = hasD ? coord(dHi[i], dRes[i], dVoxel) : -std::numeric_limits<double>::infinity();
    }
    if (hasS) {
        double c[2][3];
        for (int j = 0; j < 3; ++j) c[0][j] = coord(sLo[j], sRes[j], sVoxel), c[1][j] = coord(sHi[j], sRes[j], sVoxel);
        for (int k = 0; k < 8; ++k) {
            const double c0 = c[k & 1][0], c1 = c[(k >> 1) & 1][1], c2 = c[(k >> 2) & 1][2];
            for (int i = 0; i < 3; ++i) {
                double x = static_cast<double>(R[3 * i]) * c0;
                x = x + static_cast<double>(R[3 * i + 1]) * c1;
                x = x + static_cast<double>(R[3 * i + 2]) * c2;
                x = x + static_cast<double>(t[i]);
                mn[i] = std::min(mn[i], x);
                mx[i] = std::max(mx[i], x);
            }
        }
    }
    for (int i = 0; i < 3; ++i) lo[i] = static_cast<float>(mn[i]), hi[i] = static_cast<float>(mx[i]);
    return true;
}

void EMFusion::setMergeObjects(bool on, const MergeParams& p) {
    if (on && (sharded || world > 1))
        throw HipError("EMFusion::setMergeObjects: merging objects is not supported on the sharded path", EMF_E_ARG);
    if (!(p.minOverlap == p.minOverlap) || p.touch != p.touch || p.minSurface < 0 || p.maxRes < 2)
        throw HipError("EMFusion::setMergeObjects: minOverlap or touch is NaN, minSurface < 0 or maxRes < 2", EMF_E_ARG);
    mergeParams_ = p;
    mergeOn_ = on;
}

EMFusion::MergeEvent EMFusion::mergeObjects(int dstId, int srcId) {
    if (sharded || world > 1)
        throw HipError("EMFusion::mergeObjects: merging objects is not supported on the sharded path", EMF_E_ARG);
    return mergeInto(dstId, srcId, false, 0.0, 0.0);
}

// runSchedule, the end of a mask frame with the switch on and at least two live objects: the probe over all ordered pairs,
// the quotients, the qualifying pairs in descending overlap (ties to the smaller pair of ids), an object at most once.
void EMFusion::mergeDuplicates() {
    std::vector<int> ids;
    for (const auto& obj : objects) ids.push_back(obj.getID());
    const double touch = mergeParams_.touch < 0.0 ? 0.5 * static_cast<double>(objects.front().getTruncDist()) : mergeParams_.touch;
    const ObjectContacts& c = objectContacts(ids, false, touch);
    struct Candidate {
        double best, ab, ba;  // a < b: overlap(a -> b), overlap(b -> a) and their maximum
        int a, b;
    };
    std::map<std::pair<int, int>, Candidate> found;
    std::map<std::pair<int, int>, int64_t> least;  // the smaller of the two surfaces
    for (const ObjectContact& pr : c.pairs) {
        const double surface = static_cast<double>(pr.record.surface);
        const double overlap = pr.record.surface ? static_cast<double>(pr.record.touching) / surface : 0.0;
        const std::pair<int, int> key(std::min(pr.a, pr.b), std::max(pr.a, pr.b));
        Candidate& cd = found.emplace(key, Candidate{0.0, 0.0, 0.0, key.first, key.second}).first->second;
        (pr.a < pr.b ? cd.ab : cd.ba) = overlap;
        const int64_t n = static_cast<int64_t>(pr.record.surface);
        auto it = least.emplace(key, n).first;
        it->second = std::min(it->second, n);
    }
    std::vector<Candidate> order;
    for (auto& kv : found) {
        Candidate cd = kv.second;
        cd.best = std::max(cd.ab, cd.ba);
        if (cd.best >= mergeParams_.minOverlap && least[kv.first] >= mergeParams_.minSurface) order.push_back(cd);
    }
    std::stable_sort(order.begin(), order.end(), [](const Candidate& x, const Candidate& y) {
        if (x.best != y.best) return x.best > y.best;
        return std::make_pair(x.a, x.b) < std::make_pair(y.a, y.b);
    });
    std::set<int> taken;
    for (const Candidate& cd : order) {
        if (taken.count(cd.a) || taken.count(cd.b)) continue;
        taken.insert(cd.a), taken.insert(cd.b);
        mergeInto(cd.a, cd.b, true, cd.ab, cd.ba);  // the older object is the destination
        lastDeleted.push_back(cd.b);
    }
}

EMFusion::MergeEvent EMFusion::mergeInto(int dstId, int srcId, bool automatic, double overlapDS, double overlapSD) {
    if (dstId == srcId && dstId != 0)
        throw HipError("EMFusion::mergeObjects: object " + std::to_string(dstId) + " cannot be merged into itself", EMF_E_ARG);
    auto dstIt = ownedObjectOrThrow("mergeObjects", dstId, "the background is no object to merge into");
    auto srcIt = ownedObjectOrThrow("mergeObjects", srcId, "the background cannot be merged into an object (liftObject lifts out of it)");
    const int maxRes = mergeParams_.maxRes;
    drainForQuery();
    ObjTSDF& dst = *dstIt;
    ObjTSDF& src = *srcIt;
    MergeEvent e;
    e.dst = dstId, e.src = srcId, e.frame = frameCount;
    e.automatic = automatic, e.overlap[0] = overlapDS, e.overlap[1] = overlapSD;
    e.resBefore = dst.getVolumeRes()[0];

    // one device block: the records of the merge, then the table and the moments of the growth
    constexpr size_t kRecords = sizeof(emf_absorb_t) + sizeof(emf_merge_counts_t) + sizeof(emf_color_moved_t);
    static_assert(sizeof(emf_absorb_t) % 8 == 0 && kRecords % 8 == 0, "the records are 8-byte aligned");
    mergeRecord_.reserve(kRecords + 2 * sizeof(emf_model_t) + 2 * sizeof(emf_shape_moments_t));
    uint8_t* base = mergeRecord_.as<uint8_t>();
    auto* rec = reinterpret_cast<emf_absorb_t*>(base);
    auto* cnt = reinterpret_cast<emf_merge_counts_t*>(rec + 1);
    auto* crec = reinterpret_cast<emf_color_moved_t*>(cnt + 1);
    auto* dTable = reinterpret_cast<emf_model_t*>(base + kRecords);
    auto* dMom = reinterpret_cast<emf_shape_moments_t*>(dTable + 2);

    // the destination's buffers may be new and the source goes: the table is rebuilt whatever becomes of the rest
    writeThenRenew([&] {
        // 1. grow: the bounds of both bands, the union in the destination's frame, the existing resize
        {
            emf_model_t table[2] = {};
            int32_t res[6];
            dst.describe(table[0]);
            src.describe(table[1]);
            for (int k = 0; k < 2; ++k) std::copy(table[k].res, table[k].res + 3, res + 3 * k);
            emf_shape_moments_t mom[2];
            hipCheck(hipMemcpyAsync(dTable, table, sizeof(table), hipMemcpyHostToDevice, main.get()), "EMFusion::mergeObjects (table)");
            emfCheck(emf_hip_shapeMoments(dTable, res, 0, 2, dMom, main.abi()), "EMFusion::mergeObjects (moments)");
            hipCheck(hipMemcpyAsync(mom, dMom, sizeof(mom), hipMemcpyDeviceToHost, main.get()), "EMFusion::mergeObjects (bounds)");
            main.waitForCompletion();
            const Affine3f dp = dst.getPose(), sp = src.getPose();
            float R[9], t[3], lo[3], hi[3];  // the destination's frame <- the source's
            absorbPose(sp.rotation().val, sp.translation().val, dp.rotation().val, dp.translation().val, R, t);
            if (mergeUnion(mom[0].lo, mom[0].hi, res, dst.getVoxelSize(), mom[1].lo, mom[1].hi, res + 3, src.getVoxelSize(), R, t, lo, hi)) {
                const Vec3f p10(lo[0], lo[1], lo[2]), p90(hi[0], hi[1], hi[2]);
                const int n = dst.resizedRes(p10, p90, params.volPad);
                if (n >= 2 && n <= maxRes) {  // beyond the cap the destination stays as it is: `clipped` says what that costs
                    const Vec3f offset = dst.resize(p10, p90, params.volPad, main);
                    if (poseLog) {  // as updateObject logs a resize: several between two frames add up
                        Vec3f& logged = obj_pose_offsets[dstId][frameCount];
                        logged = logged + offset;
                        obj_poses[dstId][frameCount] = dst.getPose();
                    }
                }
            }
        }
        e.resAfter = dst.getVolumeRes()[0];
        {
            // 2. merge
            const Affine3f dp = dst.getPose(), sp = src.getPose();
            std::copy(dp.rotation().val, dp.rotation().val + 9, e.dstR);
            std::copy(dp.translation().val, dp.translation().val + 3, e.dstT);
            std::copy(sp.rotation().val, sp.rotation().val + 9, e.srcR);
            std::copy(sp.translation().val, sp.translation().val + 3, e.srcT);
            absorbPose(e.dstR, e.dstT, e.srcR, e.srcT, e.R, e.t);
            absorbBox(dst, src, e.R, e.t, e.lo, e.size, e.clipped);
            const Vec3i n = dst.getVolumeRes(), r = src.getVolumeRes();
            emf_absorb_source_t s{};
            s.tsdf = src.tsdfPtr();
            s.weights = src.weightsPtr();
            s.fgVolMask = src.fgVolMaskPtr();
            for (int i = 0; i < 3; ++i) s.res[i] = r[i];
            s.voxelSize = src.getVoxelSize();
            s.truncdist = src.getTruncDist();
            float* const tsdf = const_cast<float*>(dst.tsdfPtr());
            float* const weights = const_cast<float*>(dst.weightsPtr());
            if (colorOn) {  // both volumes carry colour since the table that held them was built; a no-op then
                dst.enableColor();
                src.enableColor();
                emfCheck(emf_hip_mergeVolumeColor(tsdf, weights, dst.fgBgPtr(), dst.colorPtr(), n.val, dst.getVoxelSize(), dst.getTruncDist(),
                                                  params.tsdfParams.maxTSDFWeight, &s, src.fgBgPtr(), src.colorPtr(), e.R, e.t, e.lo, e.size,
                                                  rec, cnt, crec, main.abi()),
                         "EMFusion::mergeObjects (colour)");
                hipCheck(hipMemcpyAsync(&e.color, crec, sizeof(e.color), hipMemcpyDeviceToHost, main.get()), "EMFusion::mergeObjects (colour record)");
            } else {
                emfCheck(emf_hip_mergeVolume(tsdf, weights, dst.fgBgPtr(), n.val, dst.getVoxelSize(), dst.getTruncDist(),
                                             params.tsdfParams.maxTSDFWeight, &s, src.fgBgPtr(), e.R, e.t, e.lo, e.size, rec, cnt, main.abi()),
                         "EMFusion::mergeObjects");
            }
            hipCheck(hipMemcpyAsync(&e.record, rec, sizeof(e.record), hipMemcpyDeviceToHost, main.get()), "EMFusion::mergeObjects (record)");
            hipCheck(hipMemcpyAsync(&e.counts, cnt, sizeof(e.counts), hipMemcpyDeviceToHost, main.get()), "EMFusion::mergeObjects (counts)");
            main.waitForCompletion();
            dst.volumesWritten(main);  // brick flags, sign maps, gradients; fgProbs / fgVolMask from the summed counts

            // 3. bookkeeping: the sums of both; the source goes without a kept mesh -- its geometry lives on in the destination
            std::vector<double> scores = dst.classScores();
            const std::vector<double>& other = src.classScores();
            if (scores.size() < other.size()) scores.resize(other.size(), 0.0);
            for (size_t k = 0; k < other.size(); ++k) scores[k] = scores[k] + other[k];
            dst.restoreBookkeeping(dst.existCount() + src.existCount(), dst.nonExistCount() + src.nonExistCount(), std::move(scores));
            mergeLog_.push_back(e);
            deleteOwned(srcIt, false, false);
        }
    });
    return e;
}

// merged.txt (setMergedOutput): after a comment line one line per event of the log, pipeline.merged_line of it.
void EMFusion::writeMerged(const std::string& dir) {
    const std::string path = dir + "/merged.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writeMerged: cannot create " + path);
    std::fprintf(file, "# dst src frame clipped automatic res_before res_after box_lo(3) box_size(3) visited outside unknown masked "
                       "saturated fused fresh solid lo(3) hi(3) foreground gained colored uncolored overlap(dst->src) overlap(src->dst) "
                       "dst R(9) t(3) src R(9) t(3): volume -> world; R(9) t(3): source frame <- destination frame\n");
    for (const MergeEvent& e : mergeLog_) {
        const emf_absorb_t& r = e.record;
        std::fprintf(file, "%d %d %d %d %d %d %d", e.dst, e.src, e.frame, e.clipped ? 1 : 0, e.automatic ? 1 : 0, e.resBefore, e.resAfter);
        detail::printInts(file, e.lo), detail::printInts(file, e.size);
        detail::printCounts(file, {r.visited, r.outside, r.unknown, r.masked, r.saturated, r.fused, r.fresh, r.solid});
        detail::printInts(file, r.lo), detail::printInts(file, r.hi);
        detail::printCounts(file, {e.counts.foreground, e.counts.gained, e.color.colored, e.color.uncolored});
        std::fprintf(file, " %.9g %.9g", e.overlap[0], e.overlap[1]);
        detail::printFloats(file, e.dstR), detail::printFloats(file, e.dstT), detail::printFloats(file, e.srcR);
        detail::printFloats(file, e.srcT), detail::printFloats(file, e.R), detail::printFloats(file, e.t);
        std::fprintf(file, "\n");
    }
    std::fclose(file);
}

}  // namespace emf
