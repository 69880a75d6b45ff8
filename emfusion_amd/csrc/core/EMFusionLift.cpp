// EMFusionLift.cpp -- emf::EMFusion: lifting objects out of the background (new behaviour), the other
// half of EMFusionAbsorb.cpp.  An object that initNewObjVolume creates starts as an empty cube, whatever the background
// already holds of it -- the geometry of an absorbed object, or what the background fused before the object's first mask
// -- and the background keeps that geometry as a second explanation of the same surface.  With the switch on the new
// object is SEEDED from the background's front copy where it has no observation of its own (emf_hip_seedVolume), the
// frame's own integrateMask then classifies the seeded voxels by the instance mask, and the background RELEASES the band
// voxels the object holds as foreground (emf_hip_releaseVolume).  One launch each on the main stream.  Colour is not
// touched.  The poses are absorbPose (float64 in a fixed order, rounded once): this unit is compiled with a*b+c
// contraction off.
#include "EMFusion.hpp"

#include <algorithm>
#include <cstdio>

namespace emf {

void EMFusion::setLiftObjects(bool on) {
    if (on && (sharded || world > 1))
        throw HipError("EMFusion::setLiftObjects: lifting objects is not supported on the sharded path", EMF_E_ARG);
    liftOn_ = on;
}

// The seed's launch.  The caller has quiesced and joined the background's integration: the front copy is current and
// nothing of this instance is in flight.  The source is the whole background, unmasked; its unseen-tile map is not
// handed over, for the reason EMFusion::absorbInto gives.
void EMFusion::liftSeed(ObjTSDF& obj, LiftEvent& e) {
    e.id = obj.getID();
    e.frame = frameCount;
    const Affine3f bg = background.getPose(), op = obj.getPose();
    absorbPose(op.rotation().val, op.translation().val, bg.rotation().val, bg.translation().val, e.seedR, e.seedT);
    const Vec3i n = background.getVolumeRes(), r = obj.getVolumeRes();
    emf_absorb_source_t s{};
    s.tsdf = background.tsdfPtr();
    s.weights = background.weightsPtr();
    for (int i = 0; i < 3; ++i) s.res[i] = n[i];
    s.voxelSize = background.getVoxelSize();
    s.truncdist = background.getTruncDist();
    const int32_t lo[3] = {0, 0, 0};
    liftRecord_.reserve(sizeof(emf_seed_t) + sizeof(emf_release_t));
    emf_seed_t* rec = liftRecord_.as<emf_seed_t>();
    emfCheck(emf_hip_seedVolume(const_cast<float*>(obj.tsdfPtr()), const_cast<float*>(obj.weightsPtr()), r.val, obj.getVoxelSize(),
                                obj.getTruncDist(), params.tsdfParams.maxTSDFWeight, &s, e.seedR, e.seedT, lo, r.val, rec,
                                main.abi()),
             "EMFusion::lift (seed)");
    hipCheck(hipMemcpyAsync(&e.seed, rec, sizeof(emf_seed_t), hipMemcpyDeviceToHost, main.get()), "EMFusion::lift (seed record)");
    main.waitForCompletion();
    obj.volumesWritten(main);  // brick flags, sign maps, gradients, the foreground probabilities
}

// The release's launch and the log entry; the caller has quiesced.
void EMFusion::liftRelease(ObjTSDF& obj, LiftEvent& e) {
    const Affine3f bg = background.getPose(), op = obj.getPose();
    absorbPose(bg.rotation().val, bg.translation().val, op.rotation().val, op.translation().val, e.releaseR, e.releaseT);
    absorbBox(obj, e.releaseR, e.releaseT, e.lo, e.size, e.clipped);
    const Vec3i n = background.getVolumeRes(), r = obj.getVolumeRes();
    liftRecord_.reserve(sizeof(emf_seed_t) + sizeof(emf_release_t));
    emf_release_t* rec = reinterpret_cast<emf_release_t*>(liftRecord_.as<char>() + sizeof(emf_seed_t));
    emfCheck(emf_hip_releaseVolume(const_cast<float*>(background.tsdfPtr()), const_cast<float*>(background.weightsPtr()), n.val,
                                   background.getVoxelSize(), obj.fgVolMaskPtr(), r.val, obj.getVoxelSize(), e.releaseR, e.releaseT,
                                   e.lo, e.size, rec, main.abi()),
             "EMFusion::lift (release)");
    hipCheck(hipMemcpyAsync(&e.release, rec, sizeof(emf_release_t), hipMemcpyDeviceToHost, main.get()), "EMFusion::lift (release record)");
    main.waitForCompletion();
    absorbDirty_ = true;  // the background's front copy was written: absorbFinish() renews what is derived from it
    liftLog_.push_back(e);
}

// runSchedule, after integrateDepth() and before integrateMasks(): every object this frame created, in list order.
void EMFusion::liftSeedCreated() {
    liftPending_.clear();
    bool quiet = false;
    for (const int id : lastCreated) {
        if (id < 0) continue;  // a mask that initNewObjVolume rejected lifts nothing
        auto it = std::find_if(objects.begin(), objects.end(), [&](const ObjTSDF& o) { return o.getID() == id; });
        if (it == objects.end()) continue;
        if (!quiet) quiesce(), quiet = true;  // the object's own integration of this frame may still be in flight
        LiftEvent e;
        liftSeed(*it, e);
        liftPending_.push_back(e);
    }
}

// runSchedule, after integrateMasks() and before cleanUpObjs: the releases in the same order, then once the renewal of
// the background's derived state and the table.
void EMFusion::liftReleaseCreated() {
    if (liftPending_.empty()) return;
    quiesce();
    try {
        for (LiftEvent& e : liftPending_) {
            auto it = std::find_if(objects.begin(), objects.end(), [&](const ObjTSDF& o) { return o.getID() == e.id; });
            if (it != objects.end()) liftRelease(*it, e);
        }
    } catch (...) {  // the front copy may be written: what is derived from it is renewed whatever became of the rest
        liftPending_.clear();
        absorbFinish();
        rebuildModelTable();
        throw;
    }
    liftPending_.clear();
    absorbFinish();
    rebuildModelTable();
}

EMFusion::LiftEvent EMFusion::liftObject(int id) {
    if (sharded || world > 1)
        throw HipError("EMFusion::liftObject: lifting objects is not supported on the sharded path", EMF_E_ARG);
    if (id == 0) throw HipError("EMFusion::liftObject: the background cannot be lifted out of itself", EMF_E_ARG);
    auto it = std::find_if(objects.begin(), objects.end(), [&](const ObjTSDF& o) { return o.getID() == id; });
    if (it == objects.end()) {
        if (std::find(allIds.begin(), allIds.end(), id) != allIds.end())
            throw HipError("EMFusion::liftObject: object " + std::to_string(id) + " is not owned by this rank", EMF_E_ARG);
        throw HipError("EMFusion::liftObject: no object " + std::to_string(id), EMF_E_ARG);
    }
    drainForQuery();
    LiftEvent e;
    liftSeed(*it, e);
    try {
        liftRelease(*it, e);
    } catch (...) {  // the object's volume is written: the table describes it again before the exception goes on
        absorbFinish();
        rebuildModelTable();
        throw;
    }
    absorbFinish();
    rebuildModelTable();
    return e;
}

// lifted.txt (setLiftedOutput): after a comment line one line per event of the log: id frame clipped, the release's box
// (lo, size), the seed's eight counts and bounds, the release's seven counts and bounds, then the seed's R (9) and t (3)
// and the release's R (9) and t (3) in %.9g.
void EMFusion::writeLifted(const std::string& dir) {
    const std::string path = dir + "/lifted.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writeLifted: cannot create " + path);
    std::fprintf(file, "# id frame clipped box_lo(3) box_size(3) seed: visited kept outside unknown masked saturated seeded solid lo(3) "
                       "hi(3) release: visited empty free outside unclaimed released solid lo(3) hi(3) seed R(9) t(3): background "
                       "frame <- object frame; release R(9) t(3): object frame <- background frame\n");
    for (const LiftEvent& e : liftLog_) {
        const emf_seed_t& s = e.seed;
        const emf_release_t& r = e.release;
        std::fprintf(file, "%d %d %d", e.id, e.frame, e.clipped ? 1 : 0);
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %d", e.lo[i]);
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %d", e.size[i]);
        for (const uint64_t v : {s.visited, s.kept, s.outside, s.unknown, s.masked, s.saturated, s.seeded, s.solid})
            std::fprintf(file, " %llu", static_cast<unsigned long long>(v));
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %d", s.lo[i]);
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %d", s.hi[i]);
        for (const uint64_t v : {r.visited, r.empty, r.free_space, r.outside, r.unclaimed, r.released, r.solid})
            std::fprintf(file, " %llu", static_cast<unsigned long long>(v));
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %d", r.lo[i]);
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %d", r.hi[i]);
        for (int i = 0; i < 9; ++i) std::fprintf(file, " %.9g", static_cast<double>(e.seedR[i]));
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", static_cast<double>(e.seedT[i]));
        for (int i = 0; i < 9; ++i) std::fprintf(file, " %.9g", static_cast<double>(e.releaseR[i]));
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", static_cast<double>(e.releaseT[i]));
        std::fprintf(file, "\n");
    }
    std::fclose(file);
}

}  // namespace emf
