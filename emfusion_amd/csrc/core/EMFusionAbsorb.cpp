// EMFusionAbsorb.cpp -- emf::EMFusion: absorbing objects into the background (new behaviour).  An object
// that leaves view is deleted (cleanUpObjs, as the reference does) and with it everything the scene queries knew of it.
// With the switch on, the band of its signed-distance volume is first resampled through the relative pose into the
// background's front copy and fused there by the background's running average (emf_hip_absorbVolume, one launch on the
// main stream), so that every reader of the background keeps it.  It carries the band only, not the free space around
// it; with colour on the colour entries of the fused voxels go with it (emf_hip_absorbVolumeColor), with
// colour off the plain entry is called exactly as before; what lies outside the background's cube is clipped and lost.
// absorbPose is float64 in the fixed operation order of include/emf_hip.h "Object contacts" (the pose of a pair with
// a = the destination, b = the source) and needs no device.  This unit is compiled with a*b+c contraction off.
#include "EMFusionDetail.hpp"

#include <algorithm>
#include <cstdio>

namespace emf {

void absorbPose(const float Rd[9], const float td[3], const float Rs[9], const float ts[3], float R[9], float t[3]) {
    contactPose(Rd, td, Rs, ts, R, t);
}

void EMFusion::setAbsorbObjects(bool on) {
    if (on && (sharded || world > 1))
        throw HipError("EMFusion::setAbsorbObjects: absorbing objects is not supported on the sharded path", EMF_E_ARG);
    absorbOn_ = on;
}

// The covering box of the whole object in the voxels of dst -- the background, or another object --
// under (R, t) = the object's volume frame <- dst's, and whether dst's cube clips the object.  "Background" below is dst.
void EMFusion::absorbBox(const TSDF& dst, const ObjTSDF& obj, const float R[9], const float t[3], int32_t lo[3], int32_t size[3],
                         bool& clipped) {
    const Vec3i n = dst.getVolumeRes(), r = obj.getVolumeRes();
    // the covering box of the whole object, and the same box against a background with kPad more voxels on every side
    // (the same centre): that one, less the helper's one voxel of margin, is the extent of the object's cube in
    // background voxels (rounded outwards); where it leaves [0, n - 1] the background's cube clips the object.  A pose
    // without a finite inverse has the helper's fall-back "everywhere" on all axes: nothing to clip, nothing inside.
    constexpr int kPad = 4096;
    emf_occ_object_t o{};
    for (int i = 0; i < 3; ++i) o.res[i] = r[i];
    o.voxelSize = obj.getVoxelSize();
    std::copy(R, R + 9, o.R);
    std::copy(t, t + 3, o.t);
    emf_occ_object_t wide = o;
    const int32_t padded[3] = {n[0] + 2 * kPad, n[1] + 2 * kPad, n[2] + 2 * kPad};
    emfCheck(emf_hip_occupancyObjectBox(&o, n.val, dst.getVoxelSize()), "EMFusion::absorb (box)");
    emfCheck(emf_hip_occupancyObjectBox(&wide, padded, dst.getVoxelSize()), "EMFusion::absorb (unclipped box)");
    const bool everywhere = wide.lo[0] == 0 && wide.lo[1] == 0 && wide.lo[2] == 0 && wide.size[0] == padded[0] &&
                            wide.size[1] == padded[1] && wide.size[2] == padded[2];
    for (int i = 0; i < 3; ++i) {
        lo[i] = o.lo[i];
        size[i] = o.size[i];
        const int first = wide.lo[i] - kPad + 1, last = wide.lo[i] - kPad + wide.size[i] - 2;  // without the margin
        if (!everywhere && (wide.size[i] <= 0 || first < 0 || last > n[i] - 1)) clipped = true;
    }
}

// The launch and the log entry.  The caller has quiesced and joined the background's integration: the front copy is
// current and nothing of this instance is in flight.
void EMFusion::absorbInto(ObjTSDF& obj) {
    AbsorbEvent e;
    e.id = obj.getID();
    e.frame = frameCount;
    const Affine3f bg = background.getPose(), op = obj.getPose();
    absorbPose(bg.rotation().val, bg.translation().val, op.rotation().val, op.translation().val, e.R, e.t);
    const Vec3i n = background.getVolumeRes(), r = obj.getVolumeRes();
    absorbBox(background, obj, e.R, e.t, e.lo, e.size, e.clipped);
    emf_absorb_source_t s{};
    s.tsdf = obj.tsdfPtr();
    s.weights = obj.weightsPtr();
    s.fgVolMask = obj.fgVolMaskPtr();
    for (int i = 0; i < 3; ++i) s.res[i] = r[i];
    s.voxelSize = obj.getVoxelSize();
    s.truncdist = obj.getTruncDist();
    absorbRecord_.reserve(sizeof(emf_absorb_t) + sizeof(emf_color_moved_t));
    emf_absorb_t* rec = absorbRecord_.as<emf_absorb_t>();
    if (colorOn) {  // both volumes carry colour since the table that held them was built; a no-op then
        background.enableColor();
        obj.enableColor();
        emf_color_moved_t* crec = reinterpret_cast<emf_color_moved_t*>(rec + 1);
        launchedRecord(emf_hip_absorbVolumeColor(const_cast<float*>(background.tsdfPtr()), const_cast<float*>(background.weightsPtr()),
                                                 background.colorPtr(), n.val, background.getVoxelSize(), background.getTruncDist(),
                                                 params.tsdfParams.maxTSDFWeight, &s, obj.colorPtr(), e.R, e.t, e.lo, e.size, rec, crec,
                                                 main.abi()),
                       "EMFusion::absorb (colour)", rec, &e.record, crec, &e.color);
    } else {
        launchedRecord(emf_hip_absorbVolume(const_cast<float*>(background.tsdfPtr()), const_cast<float*>(background.weightsPtr()), n.val,
                                            background.getVoxelSize(), background.getTruncDist(), params.tsdfParams.maxTSDFWeight, &s,
                                            e.R, e.t, e.lo, e.size, rec, main.abi()),
                       "EMFusion::absorb", rec, &e.record);
    }
    absorbDirty_ = true;
    absorbLog_.push_back(e);
}

// Once after the last absorption of a frame or a call, before rebuildModelTable(): the front copy was written from
// outside the integration -- brick flags, sign and unseen maps, gradients, the back copy -- and the fork state is that
// of a background whose copies are equal, as after a roll.
void EMFusion::absorbFinish() {
    if (!absorbDirty_) return;
    background.volumesWritten(main);
    bgBackStale = false;
    bgPrepared = false;
    bgListPending = false;
    forkFrame = -2;
    farBoundsReady = false;
    absorbDirty_ = false;
}

std::list<ObjTSDF>::iterator EMFusion::ownedObjectOrThrow(const char* who, int id, const char* background) {
    const std::string w = std::string("EMFusion::") + who;
    if (id == 0) throw HipError(w + ": " + background, EMF_E_ARG);
    auto it = std::find_if(objects.begin(), objects.end(), [&](const ObjTSDF& o) { return o.getID() == id; });
    if (it == objects.end()) {
        if (std::find(allIds.begin(), allIds.end(), id) != allIds.end())
            throw HipError(w + ": object " + std::to_string(id) + " is not owned by this rank", EMF_E_ARG);
        throw HipError(w + ": no object " + std::to_string(id), EMF_E_ARG);
    }
    return it;
}

EMFusion::AbsorbEvent EMFusion::absorbObject(int id) {
    if (sharded || world > 1)
        throw HipError("EMFusion::absorbObject: absorbing objects is not supported on the sharded path", EMF_E_ARG);
    auto it = ownedObjectOrThrow("absorbObject", id, "the background cannot be absorbed into itself");
    // An explicit call absorbs what it names, a person under ignore_person too: the caller asked for this object.
    drainForQuery();
    absorbInto(*it);
    const AbsorbEvent e = absorbLog_.back();
    // the front copy is written: what is derived from it is renewed whatever becomes of the deletion
    writeThenRenew([&] { deleteOwned(it); });  // the kept mesh and the exp_vols copy as for any deletion
    return e;
}

// absorbed.txt (setAbsorbedOutput): after a comment line one line per event of the log: id frame clipped, the box
// (lo, size), the eight counts and the bounds of the fused voxels, then R (9) and t (3) in %.9g; in a coloured session the
// two colour counts follow and the comment line names them.  A colourless session writes the bytes it always wrote.
void EMFusion::writeAbsorbed(const std::string& dir) {
    const std::string path = dir + "/absorbed.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writeAbsorbed: cannot create " + path);
    std::fprintf(file, "# id frame clipped box_lo(3) box_size(3) visited outside unknown masked saturated fused fresh solid lo(3) hi(3) "
                       "R(9) t(3): object frame <- background frame; the band only, not the free space around it%s\n",
                 colorOn ? "; colored uncolored: the colour entries of the fused voxels" : "");
    for (const AbsorbEvent& e : absorbLog_) {
        const emf_absorb_t& r = e.record;
        std::fprintf(file, "%d %d %d", e.id, e.frame, e.clipped ? 1 : 0);
        detail::printInts(file, e.lo), detail::printInts(file, e.size);
        detail::printCounts(file, {r.visited, r.outside, r.unknown, r.masked, r.saturated, r.fused, r.fresh, r.solid});
        detail::printInts(file, r.lo), detail::printInts(file, r.hi);
        detail::printFloats(file, e.R), detail::printFloats(file, e.t);
        if (colorOn) detail::printCounts(file, {e.color.colored, e.color.uncolored});
        std::fprintf(file, "\n");
    }
    std::fclose(file);
}

}  // namespace emf
