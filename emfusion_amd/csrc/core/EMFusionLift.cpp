// EMFusionLift.cpp -- emf::EMFusion: lifting objects out of the background (new behaviour), the other
// half of EMFusionAbsorb.cpp.  An object that initNewObjVolume creates starts as an empty cube, whatever the background
// already holds of it -- the geometry of an absorbed object, or what the background fused before the object's first mask
// -- and the background keeps that geometry as a second explanation of the same surface.  With the switch on the new
// object is SEEDED from the background's front copy where it has no observation of its own (emf_hip_seedVolume), the
// frame's own integrateMask then classifies the seeded voxels by the instance mask, and the background RELEASES the band
// voxels the object holds as foreground (emf_hip_releaseVolume).  One launch each on the main stream.  With colour on
// the seeded voxels take the background's colour entries and the released voxels' entries are cleared
// (emf_hip_seedVolumeColor, emf_hip_releaseVolumeColor); with colour off the plain entries are called
// exactly as before.  The poses are absorbPose (float64 in a fixed order, rounded once): this unit is compiled with a*b+c
// contraction off.
#include "EMFusionDetail.hpp"

#include <algorithm>
#include <cstdio>

namespace emf {

// liftRecord_: one emf_seed_t, one emf_release_t, then the colour records of the seed and of the release
static constexpr size_t kLiftRecordBytes = sizeof(emf_seed_t) + sizeof(emf_release_t) + 2 * sizeof(emf_color_moved_t);
static_assert((sizeof(emf_seed_t) + sizeof(emf_release_t)) % 8 == 0, "the colour records are 8-byte aligned");

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
    liftRecord_.reserve(kLiftRecordBytes);
    emf_seed_t* rec = liftRecord_.as<emf_seed_t>();
    if (colorOn) {  // both volumes carry colour since the table that held them was built; a no-op then
        background.enableColor();
        obj.enableColor();
        emf_color_moved_t* crec = reinterpret_cast<emf_color_moved_t*>(liftRecord_.as<char>() + sizeof(emf_seed_t) + sizeof(emf_release_t));
        launchedRecord(emf_hip_seedVolumeColor(const_cast<float*>(obj.tsdfPtr()), const_cast<float*>(obj.weightsPtr()), obj.colorPtr(),
                                               r.val, obj.getVoxelSize(), obj.getTruncDist(), params.tsdfParams.maxTSDFWeight, &s,
                                               background.colorPtr(), e.seedR, e.seedT, lo, r.val, rec, crec, main.abi()),
                       "EMFusion::lift (seed, colour)", rec, &e.seed, crec, &e.seedColor);
    } else {
        launchedRecord(emf_hip_seedVolume(const_cast<float*>(obj.tsdfPtr()), const_cast<float*>(obj.weightsPtr()), r.val,
                                          obj.getVoxelSize(), obj.getTruncDist(), params.tsdfParams.maxTSDFWeight, &s, e.seedR, e.seedT,
                                          lo, r.val, rec, main.abi()),
                       "EMFusion::lift (seed)", rec, &e.seed);
    }
    obj.volumesWritten(main);  // brick flags, sign maps, gradients, the foreground probabilities
}

// The release's launch and the log entry; the caller has quiesced.
void EMFusion::liftRelease(ObjTSDF& obj, LiftEvent& e) {
    const Affine3f bg = background.getPose(), op = obj.getPose();
    absorbPose(bg.rotation().val, bg.translation().val, op.rotation().val, op.translation().val, e.releaseR, e.releaseT);
    absorbBox(background, obj, e.releaseR, e.releaseT, e.lo, e.size, e.clipped);
    const Vec3i n = background.getVolumeRes(), r = obj.getVolumeRes();
    liftRecord_.reserve(kLiftRecordBytes);
    emf_release_t* rec = reinterpret_cast<emf_release_t*>(liftRecord_.as<char>() + sizeof(emf_seed_t));
    if (colorOn) {
        background.enableColor();
        emf_color_moved_t* crec = reinterpret_cast<emf_color_moved_t*>(liftRecord_.as<char>() + sizeof(emf_seed_t) + sizeof(emf_release_t)) + 1;
        launchedRecord(emf_hip_releaseVolumeColor(const_cast<float*>(background.tsdfPtr()), const_cast<float*>(background.weightsPtr()),
                                                  background.colorPtr(), n.val, background.getVoxelSize(), obj.fgVolMaskPtr(), r.val,
                                                  obj.getVoxelSize(), e.releaseR, e.releaseT, e.lo, e.size, rec, crec, main.abi()),
                       "EMFusion::lift (release, colour)", rec, &e.release, crec, &e.releaseColor);
    } else {
        launchedRecord(emf_hip_releaseVolume(const_cast<float*>(background.tsdfPtr()), const_cast<float*>(background.weightsPtr()), n.val,
                                             background.getVoxelSize(), obj.fgVolMaskPtr(), r.val, obj.getVoxelSize(), e.releaseR,
                                             e.releaseT, e.lo, e.size, rec, main.abi()),
                       "EMFusion::lift (release)", rec, &e.release);
    }
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
    // the front copy may be written: what is derived from it is renewed whatever becomes of the rest
    writeThenRenew([&] {
        std::vector<LiftEvent> pending;
        pending.swap(liftPending_);  // nothing stays owed, whatever becomes of the releases
        for (LiftEvent& e : pending) {
            auto it = std::find_if(objects.begin(), objects.end(), [&](const ObjTSDF& o) { return o.getID() == e.id; });
            if (it != objects.end()) liftRelease(*it, e);
        }
    });
}

EMFusion::LiftEvent EMFusion::liftObject(int id) {
    if (sharded || world > 1)
        throw HipError("EMFusion::liftObject: lifting objects is not supported on the sharded path", EMF_E_ARG);
    auto it = ownedObjectOrThrow("liftObject", id, "the background cannot be lifted out of itself");
    drainForQuery();
    LiftEvent e;
    liftSeed(*it, e);
    // the object's volume is written: the table describes it again whatever becomes of the release
    writeThenRenew([&] { liftRelease(*it, e); });
    return e;
}

// lifted.txt (setLiftedOutput): after a comment line one line per event of the log: id frame clipped, the release's box
// (lo, size), the seed's eight counts and bounds, the release's seven counts and bounds, then the seed's R (9) and t (3)
// and the release's R (9) and t (3) in %.9g; in a coloured session the colour counts of the seed and of the release follow
// and the comment line names them.  A colourless session writes the bytes it always wrote.
void EMFusion::writeLifted(const std::string& dir) {
    const std::string path = dir + "/lifted.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writeLifted: cannot create " + path);
    std::fprintf(file, "# id frame clipped box_lo(3) box_size(3) seed: visited kept outside unknown masked saturated seeded solid lo(3) "
                       "hi(3) release: visited empty free outside unclaimed released solid lo(3) hi(3) seed R(9) t(3): background "
                       "frame <- object frame; release R(9) t(3): object frame <- background frame%s\n",
                 colorOn ? "; seed: colored uncolored release: colored uncolored: the colour entries of the seeded / released voxels" : "");
    for (const LiftEvent& e : liftLog_) {
        const emf_seed_t& s = e.seed;
        const emf_release_t& r = e.release;
        std::fprintf(file, "%d %d %d", e.id, e.frame, e.clipped ? 1 : 0);
        detail::printInts(file, e.lo), detail::printInts(file, e.size);
        detail::printCounts(file, {s.visited, s.kept, s.outside, s.unknown, s.masked, s.saturated, s.seeded, s.solid});
        detail::printInts(file, s.lo), detail::printInts(file, s.hi);
        detail::printCounts(file, {r.visited, r.empty, r.free_space, r.outside, r.unclaimed, r.released, r.solid});
        detail::printInts(file, r.lo), detail::printInts(file, r.hi);
        detail::printFloats(file, e.seedR), detail::printFloats(file, e.seedT);
        detail::printFloats(file, e.releaseR), detail::printFloats(file, e.releaseT);
        if (colorOn) detail::printCounts(file, {e.seedColor.colored, e.seedColor.uncolored, e.releaseColor.colored, e.releaseColor.uncolored});
        std::fprintf(file, "\n");
    }
    std::fclose(file);
}

}  // namespace emf
