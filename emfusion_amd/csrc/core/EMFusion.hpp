// EMFusion.hpp -- emf::EMFusion: per-frame schedule over one background volume + N object volumes.
//
// Keeps the orchestration surface of the reference's emf::EMFusion for the volumetric hot path
// (reference include/EMFusion/core/EMFusion.h:47-510, src/core/EMFusion.cpp:28-129, 635-670,
// 726-795, 865-906): processFrame() runs computePoints -> E-step -> [pose update] -> E-step ->
// raycast -> integrateDepth -> integrateMasks in the reference's order, with one HIP stream per
// volume (reference EMFusion.h:471) joined by events instead of host synchronisation.
//
// Outside this build's scope, and therefore supplied by the caller: camera / object poses
// (tracking), object creation and masks (Mask R-CNN + lifecycle, f-3), depth
// pre-filtering (f-2).  processFrame(RGBD) is kept for the reference call site
// (apps/EM-Fusion.cpp:152); it consumes poses / masks registered with setFrameInputs().
#pragma once

#include <algorithm>
#include <list>
#include <map>
#include <string>
#include <memory>
#include <set>
#include <vector>

#include "Communicator.hpp"
#include "KernelTimers.hpp"
#include "MeshPost.hpp"
#include "ObjTSDF.hpp"
#include "Output.hpp"
#include "QueryBox.hpp"
#include "Switches.hpp"
#include "TSDF.hpp"
#include "TileStore.hpp"

namespace emf {

/** Host-side RGB-D frame (stand-in for emf::RGBD, reference include/EMFusion/utils/data.h). */
struct RGBD {
    Size size;
    const float* depth = nullptr;   // metres, W x H, row-major, host memory
    const uint8_t* rgb = nullptr;   // optional u8 x 3, W x H: fused into the colour volumes when colour is on
};

/** What tracking and Mask R-CNN would have produced for one frame. */
struct FrameInputs {
    Affine3f cam_pose;                       // camera -> world for this frame
    std::map<int, Affine3f> obj_poses;       // object id -> volume-centre -> world
    std::map<int, emf_image_t> masks;        // object id -> u8 0/1 mask (device), mask frames only
    bool runMasks = false;                   // this frame is a mask frame (frame % maskRCNNFrames)
    // Tracking (reference EMFusion::performTracking, EMFusion.cpp:672-724).  When set, the
    // corresponding supplied pose(s) are ignored: the camera pose is tracked against the
    // background from the previous frame's pose, then every object's pose against its volume.
    bool trackCamera = false;
    bool trackObjects = false;
    // EMFusion::preprocessDepth (EMFusion.cpp:294-305): bilateral filter + NaN / zero patches on
    // the incoming depth.  The reference always runs it; off by default here so that the hot-path
    // frame keeps SURVEY 8(d)'s definition.  processFrame(const RGBD&) always filters.
    bool preprocessDepth = false;
    // Instance masks (device u8 W x H) that matched no existing object: after the raycast and
    // before the integration each one runs through initNewObjVolume (EMFusion.cpp:446-494, 104-109
    // of processFrame); a created object integrates this frame's depth and this mask.
    std::vector<emf_image_t> newObjectMasks;
    // The instance masks of a Mask R-CNN frame (device u8 W x H, MODIFIED in place by the carving
    // step): after the raycast they run through the reference's initOrMatchObjs -- match against
    // the visible models, resolve double matches, carve and spawn the unmatched ones, existence
    // bookkeeping (EMFusion.cpp:329-372, 417-494) -- and the resulting id -> mask map feeds
    // integrateMasks and cleanUpObjs.  Takes the place of `masks` / `newObjectMasks`.
    std::vector<emf_image_t> instanceMasks;
    // The 81 class scores of each instance mask (same order; may be empty): a matched object
    // accumulates them (ObjTSDF::updateClassProbs, EMFusion.cpp:830), which is what ignore_person reads.
    std::vector<std::vector<double>> instanceScores;
    // Run the reference's cleanUpObjs at the end of the frame (EMFusion.cpp:922-980): objects with
    // a low existence probability (mask frames), with too little association mass under their
    // mask, or not visible are deleted.  Needs the visible set on the host (one synchronisation),
    // which is why it is a switch here.
    bool cleanUp = false;
};

/** Outcome of the last tracking run of one model (0 = camera against the background). */
struct TrackResult {
    int iterations = 0;  // LM trial steps evaluated
    int accepted = 0;    // ... of which accepted
    bool converged = false;
    float error = 0.f;   // weighted squared residual sum at the final pose
};

/** What EMFusion::saveCheckpoint did (Checkpoint.cpp). */
struct CheckpointStats {
    uint64_t rawBytes = 0;    // bytes of the device buffers that were packed
    uint64_t fileBytes = 0;   // size of the file
    uint64_t chunks[3] = {0, 0, 0};  // 1 KiB chunks per class: zero, uniform, literal
    uint32_t records = 0;     // packed buffers
    double msClassify = 0, msGather = 0;  // device time (HIP events): classify + rank, gather
    double msCopy = 0, msFile = 0, msTotal = 0;  // host time: device-to-host copies, file writes, the whole call
};

/** emf_motion_params_t for EMFusion::setMotionMasks (include/emf_hip.h "Motion masks"). */
struct MotionMaskParams {
    float band = -1.f;        // m; negative: the background's truncation distance
    float continuity = 0.05f; // m
    int erode = 1;            // 0 .. 3
    int minPixels = 200;
    int maxMasks = 8;         // 1 .. EMF_MOTION_MAX_MASKS
};

/** EMFusion::setBackgroundFollow. */
struct BackgroundFollowParams {
    Vec3i step = Vec3i(64, 64, 64);  // voxels per axis a roll moves by: positive multiples of the tile (32, 8, 8)
    float lookAhead = 0.f;           // m along the optical axis: the followed point lies this far in front of the camera
    bool keepRetired = true;         // mesh what slides out of the cube before it is dropped
};

/** The marching cubes of one sub-box of the background that a roll removed, meshed before the roll. */
struct RetiredSlab {
    int frame = 0;   // the frame at whose end the roll happened (an explicit roll: the last one processed, frameIndex() - 1)
    Vec3i origin;    // lattice index of the sub-box's voxel (0, 0, 0): backgroundOrigin() then + its offset in the volume
    Vec3i res;       // voxels of the sub-box
    Mesh mesh;       // in the sub-box's own frame (its centre at 0), as TSDF::getMesh() of a volume of that size
};

/** Per-stage GPU time of the last processed frame (milliseconds, from HIP events). */
struct FrameTimings {
    float points = 0, estep = 0, raycast = 0, composite = 0, integrate = 0, masks = 0, total = 0;
};

class EMFusion {
public:
    explicit EMFusion(const Params& params, TSDF::Gradients gradients = TSDF::Gradients::OnTheFly,
                      std::shared_ptr<Communicator> comm = nullptr);
    ~EMFusion();

    /** Drop all objects and clear the background (reference EMFusion.cpp:58-68). */
    void reset();

    /**
     * Track the camera against the background volume (reference EMFusion.cpp:673-685) or all
     * objects against the camera (EMFusion.cpp:689-723) with the current association weights.
     * Device-resident Levenberg-Marquardt (emf_hip_trackStep, one launch per iteration, up to
     * params.maxTrackingIter): the host only stops enqueuing when the device reports every model
     * done; the poses are read back once per stage.
     */
    void trackCamera();
    void trackObjects();
    /**
     * Reference EMFusion::initNewObjVolume (EMFusion.cpp:498-557): spawn an object volume from an
     * instance mask (device u8 W x H, non-zero = inside) of the CURRENT frame's points.  Returns
     * the new object id, or -1 if the mask has too few valid points (visibilityThresh), overlaps an
     * existing volume too much (volIOUThresh) or lies too far away (distanceThresh).
     *
     * Object life cycle on the sharded path (this call, initOrMatchObjs, updateObject, cleanUpObjs, and the frame
     * inputs instanceMasks / newObjectMasks / cleanUp that drive them).  ASSUMPTION: every rank receives the same
     * instance masks and scores -- through FrameInputs, or because each rank reads the same Mask%04d.plk file
     * (usePreprocMasks) -- and every rank makes the same calls.  Decisions that need only replicated data (points,
     * camera pose, the joint modelSegmentation and visible set after the composite, allIds) are taken by every rank
     * alone; owner-only facts travel in fixed exchanges, so that lastCreated / lastMaskAssignment / lastDeleted come
     * out identical on every rank:
     *   - here, when the point count passes and objects exist: every rank tests the volume IoU of ITS objects, ONE
     *     allReduceSumF32 of 16 bytes says whether any owner blocks the mask, then all ranks call addObject or none;
     *   - resizes (updateObj), class scores and existence probabilities stay with the owner; updateObject(id, mask)
     *     is called on every rank and the owner broadcasts the 16-byte offset, so every rank returns it;
     *   - cleanUpObjs: ONE allReduceSumF32 of the per-object delete verdicts (round_up(nall, 4) floats, written by
     *     the owners' mass kernel) whenever the job has objects, then every rank deletes the same ids.
     */
    int initNewObjVolume(const emf_image_t& mask);
    /** Reference EMFusion::volumeIOU (EMFusion.cpp:559-611). */
    float volumeIOU(const ObjTSDF& obj, const Vec3f& p10, const Vec3f& p90) const;
    /**
     * Reference EMFusion::matchSegmentation (EMFusion.cpp:797-825): the visible object whose
     * raycast segmentation overlaps `mask` best; its id if the IoU exceeds matchIOUThresh, else
     * -1.  match_iou is updated as in the reference (in/out).
     */
    int matchSegmentation(const emf_image_t& mask, float& match_iou);
    /**
     * Reference EMFusion::initOrMatchObjs (EMFusion.cpp:329-372) without the class scores:
     * returns object id -> mask; `assigned[i]` = the id mask i ended up with (-1: none).
     */
    std::map<int, emf_image_t> initOrMatchObjs(std::vector<emf_image_t>& segs,
                                               std::vector<int>& assigned,
                                               const std::vector<std::vector<double>>& scores = {});
    /**
     * Params.ignore_person of the reference (data.h:198, config/tum.cfg): objects whose most likely
     * class is "person" (COCO index 1) are tracked and fused like all others but left out of the
     * rendering (their pixels show the background, EMFusion.cpp:139-150) and of the mesh files
     * (EMFusion.cpp:274-278, 962-966).
     */
    void setIgnorePerson(bool on) { ignorePerson = on; }
    static bool isPerson(const ObjTSDF& obj) { return obj.getClassID() == 1; }  // class_names[1]
    const std::vector<int>& lastMaskAssignment() const { return lastAssigned; }
    /**
     * Reference EMFusion::updateObj (EMFusion.cpp:827-863): grow / recentre a matched object's
     * volume around its surface and the newly matched points; returns the centre shift (0: none).
     * updateObject(id, mask) is the stand-alone form (looks the object up, refreshes the model table); on the
     * sharded path every rank calls it, the owner resizes and broadcasts the shift, all ranks return it.
     */
    Vec3f updateObj(ObjTSDF& obj, const emf_image_t& mask);
    Vec3f updateObject(int id, const emf_image_t& mask);
    static std::map<int, std::map<int, Affine3f>> addPoseOffsets(
        const std::map<int, std::map<int, Affine3f>>& poses,
        const std::map<int, std::map<int, Vec3f>>& offsets);
    /**
     * Reference EMFusion::cleanUpObjs (EMFusion.cpp:922-980); returns the deleted ids.  The association masses of all
     * objects of this rank come from two launches over the model table (emf_hip_maskAssociationMassBatched) and one
     * wait; on the sharded path the same launch writes the delete verdicts, which one all-reduce joins (see above).
     */
    std::vector<int> cleanUpObjs(bool maskFrame, const std::map<int, emf_image_t>& matches);
    const std::vector<int>& lastDeletedObjects() const { return lastDeleted; }
    /** Reference EMFusion::preprocessDepth (EMFusion.cpp:294-305), one launch. */
    void preprocessDepth(const emf_image_t& depthRaw, const emf_image_t& depthOut);
    /**
     * Wait for the reciprocal checks of volumes created so far and adopt their verdicts.  Volumes created
     * inside frames are checked in the background and divide meanwhile; an application that adds its objects up front
     * (emf_fusion_add_object does this) calls it once so that the checks -- some tens of microseconds per distinct voxel
     * size -- do not run beside its first frames.  Same results either way.
     */
    void settleReciprocals();
    /** Result of the last tracking run of model `id` (0 = camera), or nullptr. */
    const TrackResult* getTrackResult(int id) const;
    /**
     * Keep the camera / object poses of every processed frame (reference EMFusion::storePoses,
     * EMFusion.cpp:322-327) and write them and the volumes in the reference's formats:
     * <dir>/poses-cam.txt, poses-<id>.txt, poses-<id>-corrected.txt (writePoses, EMFusion.cpp:991-1007)
     * and, with volumes, <dir>/mesh_bg.ply, mesh_<id>.ply (writeMeshes, EMFusion.cpp:1147-1156) and
     * <dir>/tsdfs/{bg_tsdf,tsdf_<id>,weights_<id>,fgProbs_<id>}.bin (writeTSDFs, EMFusion.cpp:1187-1218).
     */
    void enablePoseLog(bool on) { poseLog = on; }
    /**
     * Reference EMFusion::setupOutput (EMFusion.cpp:243-247): turns the log on (saveOutput) and
     * chooses whether the volumes are exported too.  With exp_vols the volumes of objects deleted
     * during the run are kept on the host like their mesh (EMFusion.cpp:966-973).  With exp_frame_meshes every
     * frame ends (after cleanUpObjs) by meshing the background and every live object not hidden by ignore_person
     * (EMFusion.cpp:110-125) in one pass (extractMeshes); the meshes are kept on the host under the frame's number and
     * writeResults() writes them as frame_meshes/bg/%04d.ply and frame_meshes/<id>/%04d.ply (EMFusion.cpp:1158-1185).
     * Not on the sharded path: refused there.
     * From here on every frame also keeps the reference's per-frame debug images (as PNG bytes, not as raw
     * images): association weights before and after tracking (storeAssocs, EMFusion.cpp:79-91, 307-320), Huber
     * and combined tracking weights of the stages that ran (EMFusion.cpp:110-118; TSDF.cpp:346-354), the
     * objects' foreground-probability look-ups (ObjTSDF.cpp:237-240) and what render() produced
     * (EMFusion.cpp:158-160); writeResults() writes them where writeRenderings / writeAssocs / writeHuberWeights
     * / writeTrackWeights / writeFgProbs put them (EMFusion.cpp:1009-1145).  Each costs a device-to-host copy
     * and a synchronisation per image: a debugging mode, as in the reference.  One-rank path only.
     */
    void setupOutput(bool expFrameMeshes, bool exp_vols) {
        if (expFrameMeshes && sharded)  // like renderView: remote objects are not on this rank
            throw HipError("EMFusion::setupOutput: per-frame meshes are not available on the sharded path", EMF_E_ARG);
        expFrameMeshes_ = expFrameMeshes;
        poseLog = true;
        saveOutput = true;
        expVols = exp_vols;
    }
    /**
     * Per-voxel colour (include/emf_hip.h "Per-voxel colour"; new behaviour, off by default).  enableColor(true)
     * gives every model a colour volume -- now, and at creation for later objects -- and a frame that was handed a
     * colour image (setColorImage, or RGBD::rgb) fuses it behind its TSDF integration with the association
     * weights that integration used.  Before the first frame / after reset() only; one-rank batched path only.
     */
    void enableColor(bool on);
    bool colorEnabled() const { return colorOn; }
    /** u8 x 3 device image of the frame size for the NEXT frame only; it must stay valid until that frame has run. */
    void setColorImage(const emf_image_t& rgbDev);
    /** Voxels the colour pass has updated since the last call (synchronises). */
    uint64_t takeColoredVoxels();
    /**
     * Reference EMFusion::writeResults (EMFusion.cpp:248-292): pose files and meshes always, the
     * tsdfs/ dumps only with `volumes` (or setupOutput's exp_vols).
     */
    void writeResults(const std::string& dir, bool volumes);
    /**
     * Prepare for using preprocessed masks (reference EMFusion.h:98, EMFusion.cpp:249-251): from now on
     * processFrame(const RGBD&) reads `<path>/Mask%04d.plk` (numbered by the frame count, EMFusion.cpp:383-389) on
     * every maskRCNNFrames-th frame and runs its instances through initOrMatchObjs, as runMaskRCNN does with a
     * mask path set.  A missing file counts as "no instances" (the reference's loadPreprocessed returns -1).
     */
    void usePreprocMasks(const std::string& path) { maskPath = path; }
    /**
     * Get the last Mask R-CNN segmentation image (reference EMFusion.h:83, EMFusion.cpp:237-240: the visualisation
     * of the last mask frame).  Without the colour frame the instances are drawn in the reference's instance colours
     * (MaskRCNN.cpp:290-301) on black: rgb = W x H x 3 bytes; empty before the first mask frame.  Returns the number
     * of instances of that frame.
     */
    int getLastMasks(std::vector<uint8_t>& rgb);
    /**
     * Motion masks (include/emf_hip.h "Motion masks"; new behaviour, off by default, may be switched at any time).
     * With it on, a frame that ran a raycast (frameCount > 0), is a mask frame (FrameInputs::runMasks; every
     * maskRCNNFrames-th frame of processFrame(const RGBD&)) and was handed no masks of any kind (instanceMasks --
     * queued, or loaded by usePreprocMasks --, newObjectMasks, masks: those take precedence) proposes its own
     * instance masks: connected regions of pixels measured in front of the background's raycast by more than
     * `band`.  The kernels run on the main stream between raycast and integration, the count is read back (the one
     * wait) and the first `count` planes go through initOrMatchObjs exactly as queued instance masks do, without
     * class scores; matching, carving, spawning, integrateMasks, existence probabilities and clean-up see ordinary
     * masks.  Nothing is kept from frame to frame and nothing goes into a checkpoint (a resumed session calls this
     * again).  With it off no launch and no output byte changes.  Throws on the sharded path (the background's ray
     * lengths are gathered in bands there and the life cycle's exchanges assume masks every rank was handed).
     */
    void setMotionMasks(bool on, const MotionMaskParams& p = MotionMaskParams());
    bool motionMasksEnabled() const { return motionOn; }
    /** The proposals of the last processed frame (none if it did not propose) and, if wanted, the W x H rank image
     *  (-1: no proposal); waits for the device when it has labels to fetch. */
    const std::vector<emf_motion_info_t>& lastMotionMasks(std::vector<int32_t>* labels = nullptr);
    /**
     * Follow the camera (new behaviour, off by default, may be switched at any time; with it off no
     * launch and no output byte changes).  At the end of a frame -- after the integration and its join, before the
     * per-frame meshes -- the followed point q = bgPose^-1 (camT + camR (0, 0, lookAhead)) is put through followShift;
     * a non-zero result retires the leaving slabs (keepRetired), rolls the background by it (TSDF::roll), rebuilds the
     * model table and adds it to backgroundOrigin().  All rolls are whole voxels along the background's own axes, so
     * the background at any time and every retired slab sit on one integer voxel lattice whose index (0, 0, 0) is
     * voxel (0, 0, 0) of the background at its initial pose.  Objects are untouched: their poses are in the world
     * frame.  A step that is not a positive multiple of (32, 8, 8) is refused (EMF_E_ARG); so is the sharded path.
     * A checkpoint carries the switch and its parameters only once the background has rolled (version 2; a
     * never-rolled session writes version 1 byte for byte): a session saved before its first roll resumes with
     * follow off, and the caller sets it again, as with the motion masks.
     */
    void setBackgroundFollow(bool on, const BackgroundFollowParams& p = BackgroundFollowParams());
    bool backgroundFollowEnabled() const { return followOn; }
    /**
     * The policy, a pure function of floats that touches no device: per axis shift_i =
     * trunc(q_i / (float(step_i) * voxelSize)) * step_i, every operation in single precision.  False (nothing
     * written) for a step that is not a positive multiple of (32, 8, 8), a voxel size that is not positive and finite,
     * a q that is not finite or a quotient outside +-2^20 steps.
     */
    static bool followShift(const float q[3], const int32_t step[3], float voxelSize, int32_t shift[3]);
    /** Roll the background now by `shift` voxels (any integers): retire, roll, rebuild the table.  keepRetired < 0:
     *  as the session's follow parameters say (true by default, also with follow off); 0: only re-centre, nothing is
     *  meshed or kept; > 0: retire. */
    void rollBackground(const Vec3i& shift, int keepRetired = -1);
    Vec3i backgroundOrigin() const { return bgOrigin; }
    const std::vector<RetiredSlab>& retiredSlabs() const { return retired; }
    /**
     * Remember what rolls out (new behaviour, off by default; with it off no launch, no output byte
     * and no checkpoint byte changes).  With the store on a roll must be tile-granular -- shift, background
     * resolution and backgroundOrigin() multiples of (32, 8, 8), as every policy roll is: EMF_E_ARG otherwise, before
     * anything is changed.  After the slabs are retired the leaving tiles go to the host as the bytes they are
     * (emf::TileStore, at most maxBytes: the oldest spills are dropped first); the tiles that enter are looked up, taken
     * out of the store and written into the rolled volume, with their sign and unseen-tile entries, before the two
     * copies are made equal.  retiredSlabs() stays the chronological log it is: a region that leaves twice is logged
     * twice.  Turning the store off drops what it holds.  Refused on the sharded path, as follow is.  A session
     * with the store on writes a version-3 checkpoint that carries the store.
     */
    void setBackgroundStore(bool on, uint64_t maxBytes = TileStore::kDefaultBudget);
    bool backgroundStoreEnabled() const { return storeOn; }
    const TileStore& backgroundStore() const { return bgStore; }
    /** What the last worldMesh() was made of. */
    struct WorldMeshInfo {
        uint64_t volumeTiles = 0, storedTiles = 0, duplicateTiles = 0, storedSurfaceCubes = 0;
    };
    /**
     * One mesh of what the session has mapped: the tiles of the current background that hold an
     * observation, in place, plus every tile the background store holds, meshed as ONE lattice by emf_hip_meshTiles*
     * -- no duplicates, no seams; the current volume wins where both claim a coordinate.  Positions are in the frame
     * the retired slabs are written in (a never-rolled background gets its own mesh's positions).  weld < 0: the
     * session's switch; an active component filter implies the weld; colours when the session has colour.  Drains as a
     * roll does and changes nothing of the session: no volume, map, store, retired slab or checkpoint byte.  Refused
     * (EMF_E_ARG) on the sharded path and when the background's resolution or origin is not a multiple of the tile.
     */
    Mesh worldMesh(int weld = -1);
    /** writeResults also writes world.ply = writeMesh(worldMesh()); without it no output byte changes. */
    void setWorldMeshOutput(bool on) { expWorldMesh_ = on; }
    const WorldMeshInfo& worldMeshInfo() const { return worldInfo; }
    /**
     * The extent of the scene queries (new behaviour, off by default; with it off no launch, no output
     * byte and no refusal changes).  World: the box of distanceField(), frontiers(), plan(), castRays(), viewGain()
     * and groundMap() may leave the background -- it stays in voxels of the CURRENT background volume, so lo may be
     * negative and lo + size may exceed the resolution -- and its classes come from the tiles worldMesh() reads: the
     * observed tiles of the volume in place and every tile the background store holds (emf_hip_occupancyTiles);
     * what lies in no tile is unknown.  The limits of a box stay; refused (EMF_E_ARG) on the sharded path and when the
     * background's resolution or origin is not a multiple of the tile, with the session untouched.  planes() reads
     * tsdf values and keeps refusing a box that leaves the background.  Sticky; never in a checkpoint.
     */
    void setQueryExtent(bool world) { queryWorld_ = world; }
    bool queryExtentWorld() const { return queryWorld_; }
    /** The bounding box, in voxels of the current background volume, of the background and every tile the store
     *  holds: the whole background when nothing is stored.  With the extent on, writeResults uses it wherever
     *  distance.bin, nearest.bin, frontiers.txt, plan.txt and ground.bin / ground.txt take the whole background. */
    void worldExtent(Vec3i& lo, Vec3i& size) const;
    /** What the last distanceField() computed; the device arrays stay valid until the next one. */
    struct DistanceField {
        QueryBox box;
        const uint8_t* classes = nullptr;  // device, box (z, y, x) order: EMF_OCC_*
        const int32_t* d2 = nullptr;       // device: squared distance in voxels, EMF_DF_FAR
        const float* metres = nullptr;     // device, or NULL when not asked for
        const int32_t* nearest = nullptr;  // device, or NULL when not asked for: linear index of the nearest site, EMF_DF_NONE
        uint32_t siteMask = 0;
        std::vector<int> objectIds;        // the objects that were stamped, creation order
        std::vector<Affine3f> objectPoses; // object volume <- background volume, as passed to the kernel
    };
    /**
     * Distance field of the scene (include/emf_hip.h "Distance field"): the occupancy classes of the box
     * [boxLo, boxLo + boxSize) of the background, every live object that is not in excludeIds stamped at its current
     * pose (object <- background composed in float as the frame path composes poses), then the exact squared distance
     * to the nearest voxel whose class is in siteMask, capped at capVoxels (0: no cap).  Enqueued on the main stream
     * after the frame; buffers are allocated at first use and reused.  Changes nothing of the session and nothing goes
     * into a checkpoint.  Refused (EMF_E_ARG) on the sharded path.
     */
    const DistanceField& distanceField(const Vec3i& boxLo, const Vec3i& boxSize, uint32_t siteMask, int capVoxels,
                                       const std::vector<int>& excludeIds, bool metres, bool nearest = false);
    const DistanceField& lastDistanceField() const { return dfLast; }
    /**
     * Point queries on the last distance field (emf_hip_distanceQuery): for n voxels (x, y, z) in BOX
     * coordinates the class byte, d2 and the linear index of the nearest site, any of the three outputs NULL.  A voxel
     * outside the box reads as 255, EMF_DF_FAR and EMF_DF_NONE.  Answers from the device arrays of the last
     * distanceField(): only the n voxels go up and n records come down (waits for the main stream).  EMF_E_ARG when no
     * field has been computed, and for outNearest when the last one was computed without the index.
     */
    void queryDistance(const int32_t* voxels, int n, uint8_t* outClass, int32_t* outD2, int32_t* outNearest);
    /** writeResults of setDistanceOutput also writes nearest.bin (i32, the container of distance.bin): the linear index
     *  of the nearest obstacle voxel of the whole background, -1 without one.  Needs setDistanceOutput on. */
    void setDistanceNearestOutput(bool on) { expDistanceNearest_ = on; }
    /** writeResults also writes distance.bin (f32 metres, +inf beyond the cap or without an obstacle) and occupancy.bin
     *  (u8 classes) of the whole background, both io::writeVolume; without it no output byte changes. */
    void setDistanceOutput(bool on, float capMetres = 0.f, bool unknownIsObstacle = false) {
        expDistance_ = on;
        distanceCapMetres_ = capMetres;
        distanceUnknownObstacle_ = unknownIsObstacle;
    }
    void writeDistanceField(const std::string& dir);
    /** What the last frontiers() computed; the device arrays stay valid until the next one. */
    struct Frontiers {
        QueryBox box;
        int minVoxels = 1, clearanceVoxels = 0;
        std::vector<emf_frontier_cluster_t> clusters;  // the kept ones: count descending, ties by label ascending
        uint32_t kept = 0, all = 0, voxels = 0;        // the three counters: kept clusters, all clusters, frontier voxels
        const uint8_t* classes = nullptr;  // device, box (z, y, x) order: EMF_OCC_*
        const int32_t* labels = nullptr;   // device: the label volume, -1 off the frontier
    };
    /**
     * Exploration frontiers of the scene (include/emf_hip.h "Frontiers"): over the box
     * [boxLo, boxLo + boxSize) of the background the occupancy classes exactly as distanceField() forms them (every live
     * object not in excludeIds stamped as occupied), the free voxels that touch unknown space, their 26-connected
     * clusters and one record per cluster of at least minVoxels voxels.  clearanceVoxels > 0: only frontier voxels at
     * least that many voxels from the nearest occupied voxel of the box (the distance transform with sites = occupied).
     * Enqueued on the main stream after the frame, in buffers of its own allocated at first use and reused; waits once
     * for the number of clusters, which sizes the per-cluster tables, and once for the records, which are sorted on the
     * host.  Changes nothing of the session -- the last distance field included -- and nothing goes into a checkpoint.
     * Refused (EMF_E_ARG) on the sharded path.
     */
    const Frontiers& frontiers(const Vec3i& boxLo, const Vec3i& boxSize, int minVoxels, int clearanceVoxels,
                               const std::vector<int>& excludeIds);
    const Frontiers& lastFrontiers() const { return frLast; }
    /** The centroid (sum / count) or the representative of a record in the world frame (QueryBox::worldPoint). */
    static void frontierWorldPoint(const Frontiers& f, const emf_frontier_cluster_t& c, bool representative, double out[3]);
    /** writeResults also writes frontiers.txt of the whole background (writeFrontiers); without it no output byte changes. */
    void setFrontierOutput(bool on, int minVoxels = 8, float clearanceMetres = 0.f) {
        expFrontiers_ = on;
        frontierMinVoxels_ = minVoxels;
        frontierClearanceMetres_ = clearanceMetres;
    }
    void writeFrontiers(const std::string& dir);
    /** What the last plan() computed; the device arrays stay valid until the next one. */
    struct Plan {
        QueryBox box;
        int seedRadiusVoxels = 0, clearanceVoxels = 0;
        bool throughUnknown = false;
        uint32_t maxCost = 0;
        uint32_t counters[4] = {0u, 0u, 0u, 0u};  // EMF_PLAN_*: converged, rounds, voxels with a finite cost, seeds used
        struct Goal {
            Vec3i voxel;                         // box coordinates
            uint32_t cost = EMF_PLAN_BLOCKED;    // EMF_PLAN_UNREACHED / EMF_PLAN_BLOCKED: no path
            int32_t length = 0;                  // voxels of the whole path, the goal first (0: none)
            int32_t faces = 0, edges = 0, corners = 0;  // its steps by kind (of the whole path where it was kept whole)
            std::vector<int32_t> path;           // linear indices of the box, at most pathCapacity of them
            std::vector<int32_t> waypoints;      // shortcutPlan: ascending indices into path, from 0 to its last one
        };
        std::vector<Goal> goals;
        const uint8_t* classes = nullptr;  // device, box (z, y, x) order: EMF_OCC_*
        const uint32_t* cost = nullptr;    // device: the cost field
    };
    /**
     * Path planning over the scene (include/emf_hip.h "Planning"): over the box [boxLo, boxLo + boxSize)
     * of the background, on the occupancy classes exactly as frontiers() forms them (every live object not in excludeIds
     * stamped as occupied), the cost-to-go field from startVoxels (box coordinates) through the free voxels -- and the
     * unknown ones with throughUnknown -- that are at least clearanceVoxels from the nearest occupied voxel of the box
     * (the capped transform, as frontiers()), plus the start bubble of seedRadiusVoxels; maxCost 0: no cap.  Then the
     * paths from goalVoxels (box coordinates) back to a start: pathCapacity < 0 keeps every path whole (one more wait,
     * for the lengths), otherwise at most that many voxels of each.  Enqueued on the main stream after the frame, in
     * buffers of its own allocated at first use and reused; waits for the rounds' activity counters and the results.
     * Changes nothing of the session -- the last distance field and the last frontiers included -- and nothing goes into
     * a checkpoint.  Refused (EMF_E_ARG) on the sharded path; a box of more than 2^29 voxels is EMF_E_LIMIT.
     */
    const Plan& plan(const Vec3i& boxLo, const Vec3i& boxSize, const std::vector<Vec3i>& startVoxels, int seedRadiusVoxels,
                     bool throughUnknown, int clearanceVoxels, uint32_t maxCost, const std::vector<Vec3i>& goalVoxels,
                     int pathCapacity, const std::vector<int>& excludeIds);
    const Plan& lastPlan() const { return plLast; }
    /** The background voxel under the camera: rint(R^T (camera - t) / voxel + (res - 1) / 2), in double, clamped to
     *  the volume -- the nearest voxel of the background where the camera stands outside it. */
    Vec3i cameraVoxel() const;
    /** writeResults also writes plan.txt of the whole background from the camera (writePlan); without it no output byte changes. */
    void setPlanOutput(bool on, float clearanceMetres = 0.f, bool throughUnknown = false) {
        expPlan_ = on;
        planClearanceMetres_ = clearanceMetres;
        planThroughUnknown_ = throughUnknown;
    }
    void writePlan(const std::string& dir);
    /** writePlan also runs shortcutPlan(window) and adds one "waypoints" line per reachable goal; 0: plan.txt as before. */
    void setPlanShortcutOutput(int window) { planShortcutWindow_ = window; }
    /** What the last castRays() / viewGain() computed, on the host. */
    struct Rays {
        QueryBox box;
        int clearanceVoxels = 0, group = 0;
        uint32_t passMask = 0, countMask = 0;
        std::vector<int32_t> from, to;            // 3 per ray, box coordinates
        std::vector<emf_ray_result_t> results;    // one per ray, empty when not asked for
        std::vector<emf_ray_group_t> groups;      // ceil(n / group) with group > 0
        std::vector<int32_t> origins;             // viewGain: 3 per view, the voxel under each camera
        int gridW = 0, gridH = 0;                 // viewGain: the grid
    };
    /**
     * Voxel rays over the scene (include/emf_hip.h "Voxel rays"): n rays from[k] -> to[k] (3 * n i32 each,
     * box coordinates, used as they are) over the box [boxLo, boxLo + boxSize) of the background, on the occupancy
     * classes exactly as frontiers() forms them (every live object not in excludeIds stamped as occupied).  Each ray is
     * the integer walk of the header -- NOT symmetric in its ends -- and ends at the first voxel whose class is not in
     * passMask or, with clearanceVoxels > 0, that is nearer than that to an occupied voxel of the box (the capped
     * transform, as frontiers()).  countMask: the classes counted along the way.  group > 0: one record of sums per run
     * of `group` consecutive rays; wantResults false (with group > 0): the per-ray records are neither written nor
     * copied.  Uploads the rays, launches once, copies the records back and waits once.  Changes nothing of the session
     * -- the last distance field, frontiers and plan included -- and nothing goes into a checkpoint.  Refused (EMF_E_ARG)
     * on the sharded path.
     */
    const Rays& castRays(const Vec3i& boxLo, const Vec3i& boxSize, const int32_t* from, const int32_t* to, int n, uint32_t passMask,
                         uint32_t countMask, int clearanceVoxels, const std::vector<int>& excludeIds, int group,
                         bool wantResults = true);
    const Rays& lastRays() const { return ryLast; }
    /** A candidate view: viewer -> world, OpenCV camera (as renderView), in double. */
    struct ViewPose {
        double R[9];
        double t[3];
    };
    /**
     * The unknown space each candidate view would see: per view the rays of a gw x gh grid image with intrinsics K =
     * (fx, fy, cx, cy), range metres long (viewRayTargets), cast in ONE castRays with passMask = FREE | UNKNOWN and
     * countMask = UNKNOWN -- a ray sees through unknown space and stops at the first occupied voxel -- and group =
     * gw * gh: one group record per view.  A count over rays is a score, not a volume.  The per-ray records only with
     * wantResults.  A camera outside the box yields OUTSIDE rays: groups[v].invalid == gw * gh and zero counts.
     */
    const Rays& viewGain(const std::vector<ViewPose>& views, int gw, int gh, const double K[4], double range, const Vec3i& boxLo,
                         const Vec3i& boxSize, const std::vector<int>& excludeIds, bool wantResults = false);
    /**
     * Shortcuts of the last plan()'s paths: for every goal with a kept path p_0 .. p_k (goal first) the rays p_i -> p_j
     * for all i and 2 <= j - i <= window, clipped at k, over the plan's own classes with its traverse mask and clearance
     * gate (no bubble), in one launch for all goals; then greedily on the host from i the largest such j whose ray is
     * REACHED, else i + 1 -- a step of the planner's own path is accepted untested (a face walk may clip a corner a
     * diagonal move may cut, and inside the start bubble the gate does not hold).  Fills Goal::waypoints, the ascending
     * path indices from 0 to k, of the last plan and returns it.  EMF_E_ARG without a plan or with window < 1.
     */
    const Plan& shortcutPlan(int window);
    /** The window of the last shortcutPlan() on the last plan; 0: none since that plan. */
    int lastShortcutWindow() const { return plShortcutWindow; }
    /** One model of objectShapes(): the integer record, the frame from it, the extents along the frame and the box. */
    struct ObjectShape {
        int id = 0;
        Vec3i res;
        float voxelSize = 0.f;
        Affine3f pose;                // volume -> world, as the call found it
        emf_shape_moments_t moments;  // integers only
        emf_shape_frame_t frame;      // valid == 0: no solid voxel; frame and box are zeros then
        emf_shape_extents_t extents;
        emf_shape_box_t box;
    };
    /**
     * Object shapes (include/emf_hip.h "Object shapes"): where in its volume each asked model is, how
     * large it is, how it is oriented and how much of its surface has been seen.  WHAT IS MEASURED IS THE OBSERVED SOLID
     * BAND, NOT THE BODY: a TSDF observes a band around the surface, the interior has weight 0; no result of this call is
     * a volume in cubic metres.  ids: live objects, in the order of the result; includeBackground puts slot 0 in front.
     * Drains the frame as the other queries do, then one moments launch for all models and one wait, the frames on the
     * host (shapeFrame), one extents launch and one more wait, the boxes on the host (shapeBox).  An id that does not
     * exist is EMF_E_ARG; an object without a solid voxel is a record with frame.valid == 0.  Changes nothing of the
     * session and nothing goes into a checkpoint.  Refused (EMF_E_ARG) on the sharded path.
     */
    const std::vector<ObjectShape>& objectShapes(const std::vector<int>& ids, bool includeBackground = false);
    const std::vector<ObjectShape>& lastShapes() const { return shLast; }
    /** writeResults also writes shapes.txt, one line per live object in id order (writeShapes); without it no output byte changes. */
    void setShapeOutput(bool on) { expShapes_ = on; }
    void writeShapes(const std::string& dir);
    /** One ordered pair of objectContacts(): probe a, field b (ids; 0 = the background), what it carried and its record. */
    struct ObjectContact {
        int a = 0, b = 0;
        emf_contact_pair_t pair;  // a, b: the slots of the call's compact table; R, t: b's frame <- a's; touch
        emf_contact_t record;     // integers and min_s
    };
    /** What objectContacts() leaves: the models asked (fields; the probes are those with id != 0), the ordered pairs
     *  grouped by probe, and one summary per unordered pair {a, b}: recAB its record a -> b, recBA b -> a or -1. */
    struct ObjectContacts {
        std::vector<int> ids;
        std::vector<emf_contact_side_t> sides;  // per id: res, voxel size, truncation distance, pose
        std::vector<ObjectContact> pairs;
        struct Summary {
            int a = 0, b = 0, recAB = -1, recBA = -1;
            emf_contact_summary_t summary;
        };
        std::vector<Summary> summaries;
    };
    /**
     * Object contacts (include/emf_hip.h "Object contacts"): whether the asked objects touch each other
     * or the background, how far apart their surfaces are and whether they interpenetrate, read from the signed-distance
     * volumes.  IT MEASURES WHAT THE VOLUMES SAY: min_s == 1 is "at least one truncation distance apart", a penetration
     * deeper than the fused band reads UNKNOWN, a clearance reads up to one probe voxel large.  Probes are the asked
     * objects; fields are the asked objects and, with includeBackground, slot 0 (the background as a probe is not
     * built).  touchMetres < 0: one voxel of the probe -- a policy, not a measurement.  Drains the frame as the other
     * queries do, then one table, one device block, one launch and one wait; the summaries on the host.  An id that
     * does not exist or is named twice is EMF_E_ARG.  Changes nothing of the session and nothing goes into a
     * checkpoint.  Refused (EMF_E_ARG) on the sharded path.
     */
    const ObjectContacts& objectContacts(const std::vector<int>& ids, bool includeBackground = true, double touchMetres = -1.0);
    const ObjectContacts& lastContacts() const { return ctLast; }
    /** writeResults also writes contacts.txt (writeContacts); without it no output byte changes. */
    void setContactsOutput(bool on, double touchMetres = -1.0) { expContacts_ = on, expContactTouch_ = touchMetres; }
    void writeContacts(const std::string& dir);
    /** One absorption: what went where, and what became of the voxels of the box. */
    struct AbsorbEvent {
        int id = 0;             // the object that was absorbed
        int frame = 0;          // the frame index (frames()) at which it happened
        float R[9], t[3];       // the pose used: the object's volume frame <- the background's volume frame
        int32_t lo[3], size[3]; // the box of background voxels the launch covered
        bool clipped = false;   // the object's cube (background voxels, rounded outwards) leaves the background's: lost
        emf_absorb_t record;    // include/emf_hip.h "Absorbing a volume"
        emf_color_moved_t color{};  // the colour entries that went with the fused voxels; zeros in a colourless session
    };
    /**
     * Absorbing objects into the background (include/emf_hip.h "Absorbing a volume").  Off by default and
     * sticky.  When on, an object that cleanUpObjs deletes BECAUSE IT IS NOT VISIBLE any more has the band of its signed-
     * distance volume resampled through the relative pose into the background's front copy and fused there by the
     * background's running average, before it is erased -- so that the distance field, the planner, the ground map,
     * the world mesh, the tile store and a checkpoint keep what the robot mapped a second ago.  Objects deleted as
     * spurious (low existence, association mass below assocThresh) and a person under ignore_person are not absorbed.
     * IT CARRIES THE BAND ONLY, not the free space around it; in a coloured session (enableColor) the colour entry of every
     * fused voxel goes with it (emf_hip_absorbVolumeColor); an absorbed object that later moves
     * leaves a ghost until free space carves it; what lies outside the background's cube is clipped and lost.
     * The log (absorbed()) is session state: neither it nor the switch is written to a checkpoint, reset() clears the
     * log.  With the switch off no launch, no output byte and no checkpoint byte changes.  Refused (EMF_E_ARG) on the
     * sharded path.
     */
    void setAbsorbObjects(bool on);
    bool absorbObjects() const { return absorbOn_; }
    /** Absorbs the live object `id` now and removes it from the session as a deletion would (kept mesh, exp_vols copy).
     *  An explicit call absorbs what it names, a person under ignore_person too.
     *  Refuses (EMF_E_ARG) an unknown id, the background and an object this rank does not own. */
    AbsorbEvent absorbObject(int id);
    const std::vector<AbsorbEvent>& absorbed() const { return absorbLog_; }
    /** writeResults also writes absorbed.txt (writeAbsorbed); without it no output byte changes. */
    void setAbsorbedOutput(bool on) { expAbsorbed_ = on; }
    void writeAbsorbed(const std::string& dir);
    /** One lift: what the new object took from the background and what the background gave up. */
    struct LiftEvent {
        int id = 0;                    // the object that was lifted
        int frame = 0;                 // the frame index (frames()) at which it happened
        float seedR[9], seedT[3];      // the seed's pose: the background's volume frame <- the object's volume frame
        float releaseR[9], releaseT[3];  // the release's pose: the object's volume frame <- the background's
        int32_t lo[3], size[3];        // the box of background voxels the release covered
        bool clipped = false;          // the object's cube leaves the background's (as AbsorbEvent::clipped)
        emf_seed_t seed;               // include/emf_hip.h "Lifting a volume"
        emf_release_t release;
        emf_color_moved_t seedColor{}, releaseColor{};  // the colour entries of the seeded / released voxels; zeros without colour
    };
    /**
     * Lifting objects out of the background (include/emf_hip.h "Lifting a volume"): the other half of
     * setAbsorbObjects.  Off by default and sticky.  When on, every object that initNewObjVolume creates in a frame
     * (through newObjectMasks or initOrMatchObjs) is SEEDED, after the frame's integration and before its masks are
     * integrated, with the band the background's front copy holds inside its cube -- only where the object has no
     * observation of its own -- and, after the masks are integrated, the background RELEASES the band voxels the object
     * holds as foreground (its fgVolMask), so that one surface has one explanation.  The frame's own integrateMask
     * classifies the seeded voxels: under the instance mask they are foreground at once; seeded table or floor inside the
     * cube becomes background and is never raycast.  Several creations of a frame run in list order; the background's
     * derived state is renewed once after the last (absorbFinish), then the model table is rebuilt.
     * In a coloured session (enableColor) the seeded voxels take the background's colour entries and the released voxels'
     * entries are cleared (emf_hip_seedVolumeColor, emf_hip_releaseVolumeColor).  A voxel behind the object along
     * a mask ray inside the cube is claimed and released too (a hole in the table under a cup).  An object discovered by
     * motion masks sits where the background holds free space: the seed finds nothing, and the ghost at the OLD place
     * is not addressed.  The log (lifted()) is session state: neither it nor the switch is written to a checkpoint,
     * reset() and a loaded checkpoint clear the log.  With the switch off no launch, no output byte and no checkpoint
     * byte changes.  Refused (EMF_E_ARG) on the sharded path.
     */
    void setLiftObjects(bool on);
    bool liftObjects() const { return liftOn_; }
    /** Seed, then release, for the LIVE object `id` between frames; the object stays live.  ITS SEEDED VOXELS CARRY NO
     *  FOREGROUND COUNT UNTIL THE NEXT MASK FRAME: until then they are neither raycast nor released (the release of this
     *  call gives up what the object held as foreground before).  Refuses (EMF_E_ARG) an unknown id, the background and
     *  an object this rank does not own. */
    LiftEvent liftObject(int id);
    const std::vector<LiftEvent>& lifted() const { return liftLog_; }
    /** writeResults also writes lifted.txt (writeLifted); without it no output byte changes. */
    void setLiftedOutput(bool on) { expLifted_ = on; }
    void writeLifted(const std::string& dir);
    /** One merge: which object went into which, through what, and what became of the voxels of the box. */
    struct MergeEvent {
        int dst = 0, src = 0;       // the object that stays and the one that went into it
        int frame = 0;              // the frame index (frames()) at which it happened
        float dstR[9], dstT[3];     // the destination's pose (volume -> world) as the merge used it: after the growth
        float srcR[9], srcT[3];     // the source's pose
        float R[9], t[3];           // the pose used: the source's volume frame <- the destination's volume frame
        int32_t lo[3], size[3];     // the box of destination voxels the launch covered
        bool clipped = false;       // the source's cube (destination voxels, rounded outwards) leaves the destination's: lost
        bool automatic = false;     // merged by setMergeObjects at the end of a mask frame, not by a call
        double overlap[2] = {0.0, 0.0};  // what decided an automatic merge (dst -> src, src -> dst); 0 for an explicit call
        int resBefore = 0, resAfter = 0;  // the destination's resolution per axis before and after the growth
        emf_absorb_t record;        // include/emf_hip.h "Merging a volume"
        emf_merge_counts_t counts{};
        emf_color_moved_t color{};  // zeros in a colourless session
    };
    /**
     * Merging an object into another object (include/emf_hip.h "Merging a volume"), between frames: the
     * repair for one physical thing that ended up with two volumes.  Three steps.
     * GROW: the destination's cube must hold what the source holds.  The inclusive bounds lo, hi (voxels) of the OBSERVED
     * SOLID BAND of both objects come from one emf_hip_shapeMoments launch; a bound v on axis j is the coordinate
     * c_j = (v_j - (N_j - 1) / 2) * voxelSize of its volume frame; the eight corners of the source's bounds go through
     * (R', t') = absorbPose(source pose, destination pose) -- the destination's frame <- the source's, float32 -- as
     * x_i = ((R'_i0 * c_0 + R'_i1 * c_1) + R'_i2 * c_2) + t'_i; the minimum and maximum over them and the destination's own
     * two bounds, per axis, rounded to float32 once, go to ObjTSDF::resize(lo, hi, volPad).  Everything float64, every line
     * a single operation in that order.  An object without a solid voxel adds nothing to the union.  MergeParams::maxRes
     * caps the grown resolution per axis (default 256: a policy value, the largest object volume of BASELINE.json's
     * configs, not a measurement); where the growth would pass it the destination is not grown.
     * MERGE: absorbPose(destination pose, source pose), the covering box (absorbBox; `clipped` as 5.29 computes it), one
     * emf_hip_mergeVolume on the main stream -- emf_hip_mergeVolumeColor in a coloured session -- then the destination's
     * volumesWritten(): fgProbs / fgVolMask from the summed counts.  THE POSES ARE TAKEN AS THEY ARE: the two volumes are not
     * registered first, a drifted duplicate merges blurred.  It carries the band, not the free space around it.
     * BOOKKEEPING: the destination keeps its id and its tracking state, and its pose but for the shift of the growth (logged
     * as a resize is); its existence counts become the sums of both, its class scores the element-wise sums.  The source
     * is deleted; ITS KEPT MESH AND exp_vols COPY ARE NOT KEPT -- its geometry lives on in the destination.
     * Refuses (EMF_E_ARG) id 0, an unknown id, dstId == srcId, an object this rank does not own and the sharded path.
     * The log (merged()) is session state: not in checkpoints, emptied by reset() and by a loaded checkpoint.  Without a
     * call no launch, no output byte and no checkpoint byte changes.
     */
    MergeEvent mergeObjects(int dstId, int srcId);
    const std::vector<MergeEvent>& merged() const { return mergeLog_; }
    /** What decides an automatic merge.  THE DEFAULTS ARE POLICY, NOT MEASUREMENTS. */
    struct MergeParams {
        double minOverlap = 0.5;   // a pair qualifies when max(overlap(a -> b), overlap(b -> a)) >= minOverlap
        int64_t minSurface = 64;   // ... and both surfaces hold at least this many voxels
        double touch = -1.0;       // metres; < 0: half a truncation distance of the first live object (through contactTouch)
        int maxRes = 256;          // the cap of the growth, of explicit calls too
    };
    /**
     * Merging DUPLICATES automatically.  Sticky, off by default; the parameters are kept either way (an
     * explicit mergeObjects grows up to maxRes).  When on, at the end of every mask frame, after cleanUpObjs, with at least
     * two live objects: one emf_hip_contactProbe launch over all ordered object pairs (objectContacts without the
     * background); overlap(a -> b) = touching / surface of the record a -> b, a float64 quotient, 0 for an empty surface; a
     * pair qualifies by MergeParams; qualifying pairs are merged in descending max overlap, ties to the smaller pair of
     * ids; the older object (smaller id) is the destination; an object takes part in at most one merge per frame.
     * IT FINDS DUPLICATES: two halves that merely abut reach no sensible overlap and are merged by the explicit call or by
     * a caller's own rule on objectContacts().  Neither the switch nor the log is written to a checkpoint.  With the
     * switch off no launch, no output byte and no checkpoint byte changes.  Refused (EMF_E_ARG) on the sharded path.
     */
    void setMergeObjects(bool on, const MergeParams& p);
    void setMergeObjects(bool on) { setMergeObjects(on, mergeParams_); }
    bool mergeObjectsOn() const { return mergeOn_; }
    const MergeParams& mergeParams() const { return mergeParams_; }
    /** writeResults also writes merged.txt (writeMerged); without it no output byte changes. */
    void setMergedOutput(bool on) { expMerged_ = on; }
    void writeMerged(const std::string& dir);
    /** The result of groundMap(): the frame, the pose "ground metres -> world" and the arrays left on the device. */
    struct GroundMap {
        QueryBox box;
        emf_ground_frame_t frame{};
        double pose[12] = {};  // R row-major with (u, v, h) as columns, then t
        int robotBins = 0, maxStepBins = 0;
        const emf_ground_cell_t* cells = nullptr;  // device, map[0] * map[1] records
        const uint8_t* classes = nullptr;          // device, (1, H, W): an input of the 2-D distance, frontier and plan entries
    };
    /**
     * Ground map (include/emf_hip.h "Ground map"): where a robot that drives on a floor can stand.  The
     * occupancy classes of the box, every live object not in excludeIds stamped, are projected along `up` (world frame)
     * onto cells of `cell` metres with height bins of `bin` metres over the band [bandLo, bandHi) metres relative to the
     * world point `ref` along up; every column gives a floor level with robotBins FREE bins above it, and the cells a 2-D
     * class volume in which steps of more than maxStepBins bins are obstacles.  Drains the frame as the other queries do,
     * then the classes and the three ground entries on the main stream and one wait.  Changes nothing of the session and
     * nothing goes into a checkpoint.  Refused (EMF_E_ARG) on the sharded path.
     */
    const GroundMap& groundMap(const Vec3i& boxLo, const Vec3i& boxSize, const double up[3], double cell, double bin,
                               const double ref[3], double bandLo, double bandHi, int robotBins, int maxStepBins,
                               const std::vector<int>& excludeIds);
    const GroundMap& lastGroundMap() const { return gmLast; }
    /** The result of planes(): the planes ordered by count, the counters of the surface pass and what stays on the device. */
    struct Planes {
        QueryBox box;
        uint32_t counters[4] = {0, 0, 0, 0};  // surface voxels, those with a normal, records written, 0
        uint32_t minVotes = 0;                // the threshold that was applied
        std::vector<emf_plane_t> planes;
        const emf_plane_voxel_t* records = nullptr;  // device, counters[2] records
        const int16_t* labels = nullptr;             // device, one per record; NULL where no plane was found
        bool keptLabels = false;
    };
    /**
     * Planes (include/emf_hip.h "Planes"): the dominant planes of a box of the background -- floor, walls,
     * table tops -- from a vote of the surface voxels' TSDF gradients: direction, offset, then assignment with an integer
     * least-squares refit.  A plane is the plane of the shell's voxel centres: up to one voxel behind the surface.
     * Drains the frame as the other queries do; the surface pass skips tiles the background's unseen-tile map marks.
     * Waits 3 + refine times: the host decisions between the stages are inherent.  Changes nothing of the session and
     * nothing goes into a checkpoint.  Refused (EMF_E_ARG) on the sharded path.
     */
    const Planes& planes(const Vec3i& boxLo, const Vec3i& boxSize, const emf_plane_params_t& params, bool keepLabels = false);
    const Planes& lastPlanes() const { return pnLast; }
    /** The result of planePatches(): the kept patches in ascending id order and what stays on the device. */
    struct PlanePatches {
        uint32_t counters[3] = {0, 0, 0};  // EMF_PATCH_KEPT, _PATCHES, _MEMBERS
        int reach = 0;
        int64_t minCount = 0;
        std::vector<emf_plane_patch_t> patches;
        const int32_t* ids = nullptr;  // device, one per record of the planes it was computed from; NULL without a plane
    };
    /**
     * Plane patches (include/emf_hip.h "Planes", stage 4): the planes of the last planes() split into
     * connected surfaces -- two tables of one height are two patches of one plane.  Works on the records and labels that
     * planes() left on the device and refuses (EMF_E_ARG) where there are none; the extents are taken along each plane's
     * own in-plane axes, rounded to f32 once.  Waits twice: for the number of patches, then for the records.  Changes
     * nothing of the session and nothing goes into a checkpoint.  Refused (EMF_E_ARG) on the sharded path.
     */
    const PlanePatches& planePatches(int reach, int64_t minCount);
    const PlanePatches& lastPlanePatches() const { return ppLast; }
    /** A patch in the world frame (describePlanePatches). */
    struct PatchWorld {
        int plane = -1;  // index into Planes::planes
        int32_t id = 0;
        emf_plane_patch_rect_t rect;  // box voxel coordinates
        double point[3] = {0, 0, 0}, normal[3] = {0, 0, 0}, d = 0.0;  // the patch's own fit
        double center[3] = {0, 0, 0}, axes[6] = {0, 0, 0, 0, 0, 0}, halfM[2] = {0, 0}, corners[12] = {};  // the rectangle
    };
    /**
     * The patches of a result in the world frame, plane by plane in the planes' order, inside a plane by count descending,
     * ties to the lower id.  Points go through QueryBox::worldPoint, directions through the background's rotation,
     * lengths times the voxel size; float64, sums left to right.  pipeline.plane_patch_world states the same in Python.
     */
    static void describePlanePatches(const Planes& planes, const PlanePatches& patches, std::vector<PatchWorld>& out);
    /** A plane of planes() in the world frame, with its kind (describePlanes). */
    struct PlaneWorld {
        double normal[3] = {0, 0, 0}, point[3] = {0, 0, 0}, d = 0.0;  // normal . x = d; the point is the members' centroid
        double thicknessM = 0.0;
        const char* kind = "slope";  // floor, level, ceiling, wall or slope
    };
    /**
     * The planes of a result in the world frame and their kinds; returns the index of the floor or -1.  The normal goes
     * through the background's rotation, the centroid through QueryBox::worldPoint, d = n . point, all float64, sums left
     * to right.  The floor is, among planes whose normal is within floorAngle degrees of up (all zero: minus the
     * background's y axis), the one whose point is lowest along up, ties to the lowest index; the others are level
     * (within kindAngle of the floor's normal, or of up without a floor), ceiling (of its opposite), wall
     * (perpendicular within kindAngle) or slope.  pipeline.plane_kinds states the same in Python.
     */
    static int describePlanes(const Planes& planes, const double up[3], double floorAngle, double kindAngle,
                              std::vector<PlaneWorld>& out);
    /** The parameters of setPlanesOutput. */
    struct PlanesOutput {
        bool on = false;
        double angle = 20.0;    // degrees
        int64_t minVotes = 0;   // <= 0: the policy of emf_plane_params_t
    };
    /** writeResults also writes planes.txt of the whole background (writePlanes); without it no output byte changes. */
    void setPlanesOutput(const PlanesOutput& p) { expPlanes_ = p; }
    void writePlanes(const std::string& dir);
    /** The parameters of setPlanePatchesOutput. */
    struct PlanePatchesOutput {
        bool on = false;
        int reach = 1;
        int64_t minCount = 0;  // <= 0: max(25, min_votes / 4) of the planes
    };
    /** With setPlanesOutput on, planes.txt also lists every plane's patches and, with setShapeOutput on as well, which
     *  patch each object rests on (writePlanes); without it no output byte changes. */
    void setPlanePatchesOutput(const PlanePatchesOutput& p) { expPatches_ = p; }
    /** setGroundOutput's up becomes the normal of the floor planes() finds in the whole background (an error where it
     *  finds none): --ground-up floor. */
    void setGroundUpFloor(bool on) { expGroundUpFloor_ = on; }
    /** The parameters of setGroundOutput: metres; cell or bin <= 0: two voxels of the background. */
    struct GroundOutput {
        bool on = false;
        double up[3] = {0.0, 0.0, 0.0};  // all zero: minus the background's y axis in the world frame
        double cell = 0.0, bin = 0.0, bandLo = -1.5, bandHi = 0.5, robotHeight = 0.3, maxStep = 0.05;
    };
    /** writeResults also writes ground.bin and ground.txt of the whole background (writeGround); without it no output
     *  byte changes. */
    void setGroundOutput(const GroundOutput& g) { expGround_ = g; }
    void writeGround(const std::string& dir);
    /** Ids returned by initNewObjVolume for FrameInputs::newObjectMasks of the last frame (-1: none). */
    const std::vector<int>& lastCreatedObjects() const { return lastCreated; }
    Affine3f getCameraPose() const { return pose; }
    const ObjTSDF* getObject(int id) const;
    /**
     * Phong rendering of the current model view (reference EMFusion::render, EMFusion.cpp:131-160,
     * without the viz window): rgb = W x H x 3 bytes on the host.  Black before the first frame;
     * after the first frame the models are raycast once for it, as in the reference.
     */
    void render(uint8_t* rgb);
    const std::array<uint8_t, 768>& getColorMap() const { return colorMap; }
    /**
     * Free-viewpoint view of the whole map (the reference's --3d-vis view, EMFusion.cpp:162-231, ray-cast from the
     * viewer instead of meshed): the background and every live object at its current pose, composited and
     * Phong-shaded as render() does for the tracked camera (ignore_person hides the same objects), light at the
     * viewer.  viewerPose: viewer -> world (OpenCV camera: +z forward, +y down); K: the viewer's intrinsics.
     * Host outputs: rgb = size.area() x 3 bytes (required), raylengths (f32) and seg (u8) may be NULL.  Ordered
     * after every write of the last frame; reads the volumes only (one launch, emf_hip_renderView) and touches no
     * image, statistic or log of the frame path.  Black / zeros before the first frame.  Not on the sharded path.
     */
    void renderView(const Affine3f& viewerPose, const float K[9], Size size, uint8_t* rgb, float* raylengths = nullptr,
                    uint8_t* seg = nullptr, int shading = 0);
    /** Shading of a view: the label colour of the model under the pixel (today's bytes), or the colour of the voxel
     *  nearest to the pixel's vertex (enableColor; voxels nobody coloured fall back to the label colour). */
    enum { ShadeLabel = 0, ShadeColor = 1 };
    void set3dViewShading(int shading);
    /**
     * The logged 3D view (reference --3d-vis): from now on render() also renders this view and, with the log on
     * (setupOutput), keeps it as frame frameCount - 1's PNG; writeResults() then writes <dir>/mesh_vis_out/%04d.png
     * (EMFusion.cpp:1018-1025).  clear3dView() turns it off (no mesh_vis_out/ unless it was set).
     */
    void set3dView(const Affine3f& viewerPose, const float K[9], Size size);
    void clear3dView() { view3d = false; }
    /**
     * Multi-GPU: the depth image enters the node on ONE rank.  With a root >= 0 every frame starts
     * with a broadcast of the depth buffer handed to processFrame (source on `root`, destination on
     * the other ranks: same size and pitch everywhere) over the communicator -- the per-frame
     * broadcast SURVEY 8(e) lists next to the two reductions.  -1 (default): every rank already
     * holds the frame.
     */
    void setDepthBroadcastRoot(int root) { depthRoot = root; }
    /**
     * Welded meshes (include/emf_hip.h "Welded meshes"; new behaviour, off by default): getMesh(id), extractMeshes()
     * and everything writeResults() and the per-frame export write become one vertex per grid edge -- the first soup
     * copy's bits -- with the soup's triangles re-indexed, welded on the device before the copies to the host.  An
     * output form only: TSDF::getMesh() stays the soup wherever the life cycle uses it (the extent statistics, the
     * last mesh kept of a deleted object), so no tracking, life-cycle or clean-up decision depends on the switch.
     */
    void setMeshWeld(bool on) { meshWeld = on; }
    /**
     * The component filter (include/emf_hip.h "Mesh components"; new behaviour, off by default): wherever the weld
     * switch acts -- getMesh(id), extractMeshes(), writeResults()' meshes of the live models, the per-frame export --
     * connected components of fewer than minTriangles triangles are removed from every model's welded mesh and, with
     * largestObjects, every component but the largest from the OBJECT meshes (a background legitimately has several
     * pieces).  Labelled, filtered and compacted on the device behind the weld; only the filtered arrays travel to the
     * host.  An active filter (minTriangles > 1 or largestObjects) implies the welded form whatever setMeshWeld says.
     * An output form only, exactly as the weld: the life cycle's soup, the last mesh kept of a deleted object, poses,
     * decisions, volumes and images do not depend on it.  Not stored in a checkpoint.
     */
    void setMeshFilter(uint32_t minTriangles, bool largestObjects) {
        meshMinTriangles = minTriangles;
        meshLargestObjects = largestObjects;
    }
    /** Per model id of the last getMesh() / extractMeshes() under an active filter: what the filter met and kept. */
    const std::map<int, MeshFilterStats>& lastMeshFilter() const { return meshFilterStats; }
    /**
     * Simplified meshes (include/emf_hip.h "Simplified meshes"; new behaviour, off by default): wherever the weld switch
     * and the filter act -- getMesh(id), extractMeshes(), writeResults()' meshes of the live models, the per-frame
     * export -- and in worldMesh() and the retired slabs meshed after the call, the welded and filtered mesh is
     * clustered by cubic cells of cellMetres (counted from 0 in the mesh's own frame) on the device; only the simplified
     * arrays travel to the host.  It runs behind the filter, so fragment sizes are counted in original triangles.  A
     * cell > 0 implies the welded form whatever setMeshWeld says; 0 (or less) is off.  An output form only, exactly as
     * the weld: the life cycle's soup, the last mesh kept of a deleted object, poses, decisions, volumes and images
     * do not depend on it.  Not stored in a checkpoint.
     */
    void setMeshSimplify(float cellMetres) {
        if (!(cellMetres < 3.0e38f)) throw HipError("EMFusion::setMeshSimplify: the cell must be finite", EMF_E_ARG);
        meshSimplifyCell = cellMetres > 0.f ? cellMetres : 0.f;
    }
    /** Per model id of the last getMesh() / extractMeshes() with setMeshSimplify on: vertices and triangles in and out,
     *  and the clusters met. */
    const std::map<int, MeshSimplifyStats>& lastMeshSimplify() const { return meshSimplifyStats; }
    /** Labels and component sizes of model id's welded, unfiltered mesh (TSDF::getMeshComponents). */
    MeshComponents getMeshComponents(int id);
    /** getMesh() of the background (id 0) or of an object held by this rank (welded with setMeshWeld, filtered with
     *  setMeshFilter). */
    Mesh getMesh(int id);
    /**
     * getMesh() of each listed model (0 = background, else a live object id), in list order, in one pass over the
     * current model table: one count launch, one read-back of the counts (the only wait before the emit), one emit
     * launch into a pooled device arena grown when needed, three device-to-host copies.  Same bytes as getMesh().
     * Ordered after every write of the last frame.  On the sharded path: this rank's models.
     */
    std::vector<Mesh> extractMeshes(const std::vector<int>& ids);

    /**
     * Create an object volume centred at `center` (world) with edge length `volSize` metres --
     * the geometric tail of the reference's initNewObjVolume (EMFusion.cpp:541-557).  With more
     * than one rank every rank must issue the same calls; only the owning rank allocates the
     * volume.  Returns the object id (1-based, creation order = compositing order).
     */
    int addObject(const Vec3f& center, float volSize);
    int addObject(const Vec3f& center, float volSize, const Vec3i& res);

    /**
     * Checkpoint and resume (Checkpoint.cpp; new behaviour: the reference has none).  saveCheckpoint writes the
     * session's primary state -- parameters, frame count, poses, object table and bookkeeping, pose logs, kept meshes
     * and the volumes, packed losslessly on the device (include/emf_hip.h "Packed buffers") -- to path + ".tmp" and
     * renames it; it changes nothing in the session.  loadCheckpoint acts as reset() followed by the restore and may
     * be called at any time; a file that does not fit this instance (frame size, intrinsics, background geometry,
     * TSDF parameters), is damaged or truncated is refused with EMF_E_ARG and leaves the session as it was.  A
     * restored session continues with the bytes of one that was never interrupted.  Both throw on the sharded path.
     */
    CheckpointStats saveCheckpoint(const std::string& path);
    void loadCheckpoint(const std::string& path);
    /** The parameters, frame index, objects and per-record chunk counts of a checkpoint file as JSON; no device. */
    static std::string checkpointInfo(const std::string& path);
    /** The parameters a checkpoint was saved with (what --resume builds its instance from); no device. */
    static Params checkpointParams(const std::string& path, bool* materializedGradients = nullptr);

    /** Poses / masks the next processFrame(RGBD) call consumes. */
    void setFrameInputs(const FrameInputs& in) { pending = in; }
    void loadPreprocMasks(FrameInputs& in);

    /** Reference entry point (EMFusion.cpp:70): uploads the depth map, then runs the schedule. */
    void processFrame(const RGBD& frame);
    /** Same schedule on a depth map already resident in device memory (f32 W x H). */
    void processFrame(const emf_image_t& depthDev, const FrameInputs& in);

    // ---- the four path stages; public so they can be driven and timed one by one ----
    /** E-step over all models (reference EMFusion.cpp:635-670). */
    void computeAssociationWeights();
    /** Raycast all models + compositing + visibility (reference EMFusion.cpp:726-795). */
    void raycast();
    /** Fuse depth into the background and every visible object (reference EMFusion.cpp:865-889). */
    void integrateDepth();
    /** fg/bg update of the matched objects (reference EMFusion.cpp:891-906). */
    void integrateMasks(const std::map<int, emf_image_t>& matches);

    /** Block until everything enqueued so far has finished. */
    void synchronize();
    /** Wait for the work of this instance only (its streams), not for the device. */
    void quiesce();

    // ---- state access ----
    int frameIndex() const { return frameCount; }
    const Params& getParams() const { return params; }
    TSDF& getBackground() { return background; }
    std::list<ObjTSDF>& getObjects() { return objects; }
    ObjTSDF* findObject(int id);
    /** Objects classified visible by the last raycast (waits for the device if necessary). */
    const std::set<int>& visibleObjects();
    /** Voxels swept by the batched integration since the counter was last read (and reset). */
    uint64_t takeIntegratedVoxels();
    bool usesBatchedLaunches() const { return batched; }
    /** Launches per stage on the batched path: 1 up to EMF_MAX_BATCH models, then one per chunk of the model table. */
    int batchedChunks() const { return batched ? launchChunks() : 0; }
    /** The background is integrated out of place on a second stream, beside the raycast. */
    bool overlapsBackground() const { return overlapUsable(); }
    std::vector<int> objectIds() const { return allIds; }
    bool ownsObject(int id) const;
    /** Host seconds processFrame(const RGBD&) has spent so far handing the depth maps to the device (staging memcpy +
     *  enqueue with the double-buffered upload; the blocking copy with EMF_ASYNC_UPLOAD=0), and the number of frames. */
    std::pair<double, uint64_t> uploadHostTime() const { return {uploadHostSeconds, uploads}; }
    const FrameTimings& lastTimings() const { return timings; }
    void enableTimings(bool on) { timingsOn = on; }
    /** Per-launch HIP-event timers (see KernelTimers.hpp); maxLaunches = 0 switches them off. */
    KernelTimers& kernelTimers() { return ktimers; }
    /** Device counters [march samples, hits, gathered samples, fast-forwarded samples]
     *  accumulated by raycast() while enabled. */
    void enableRaycastStats(bool on);
    std::array<uint64_t, 4> raycastStats();

    // device images of the last frame (valid until the next call)
    const DeviceImage<float, 3>& getPoints() const { return points; }
    const DeviceImage<float>& getBgAssociation() const { return bg_associationWeights; }
    const DeviceImage<float>* getObjAssociation(int id) const;
    const DeviceImage<float>& getAssociationNorm() const { return associationNorm; }
    const DeviceImage<float>& getRaylengths() const { return raylengths; }
    const DeviceImage<float, 3>& getVertices() const { return vertices; }
    const DeviceImage<float, 3>& getNormals() const { return normals; }
    const DeviceImage<uint8_t>& getModelSegmentation() const { return modelSegmentation; }
    const DeviceImage<float>& getBgRaylengths() const { return bg_raylengths; }
    const DeviceImage<float>* getObjRaylengths(int id) const;
    Stream& mainStream() { return main; }

private:
    struct ObjImages {
        DeviceImage<float> raylengths;
        DeviceImage<float, 3> vertices, normals;
        DeviceImage<uint8_t> modelSegmentation;
        DeviceImage<float> associationWeights;
    };

    void createObj(int id);
    void runSchedule(const emf_image_t& depthDev, const FrameInputs& in);
    // batched (model-table) path: one launch per stage, no host synchronisation inside a frame
    void rebuildModelTable();
    void adoptReciprocals();
    void posesCO(std::vector<emf_pose_t>& out) const;
    void posesOC(std::vector<emf_pose_t>& out) const;
    void estepBatched();
    void estepSharded(const std::vector<emf_pose_t>& co, bool fromDepth);
    void launchEstep(const std::vector<emf_pose_t>& co, int first, int count, bool fromDepth, int normalize,
                     const emf_image_t* norm, const emf_image_t* objSum);
    bool pointsPending = false;   // the frame's first E-step makes the points (sw.fusePoints) and has not run yet
    bool visCountsClear = true;   // visCounts holds zeros (cleared at construction, left so by the fused pair)
    void raycastBatched();
    void integrateBatched();
    void compositeAndVisibility(bool deviceGate);
    void compositeAcrossRanks(bool deviceGate);
    struct ObjectViews {  // the owned objects' raycast images, creation order
        std::vector<int32_t> index;  // per object: its id, or its position in allIds
        std::vector<emf_image_t> ray, vert, norm, seg;
    };
    ObjectViews objectViews(bool byListPosition);
    struct FrameViews {  // the composite's ten frame images, in the order of the ABI's arguments
        emf_image_t bgRay, bgVert, bgNorm, bgMask, ray, vert, norm, seg, diff, noObj;
    };
    FrameViews frameViews();
    void visibleFromCounts(const std::vector<int32_t>& ids, bool deviceGate, bool mirrored);
    void reduceAndNormalize(const std::vector<emf_image_t>& maps, bool timed);
    void refreshVisibleFromDevice();
    // legacy path: one stream per volume, host-side visibility gate (reference structure)
    void estepPerVolume();
    void raycastPerVolume();
    void integratePerVolume();
    void forkVolumeStreams();
    void joinVolumeStreams();
    Stream& streamOf(int key);
    float stamp(int slot);
    double pixels() const;

    // Member order.  `sw` comes first: the environment is read once per construction, in front of everything that needs
    // a value (the streams' priorities) and of every allocation, so a refused value (EMF_MARCH_ROWS) throws with nothing
    // to undo.  ~EMFusion only waits for the device; the members then go in reverse order of declaration: first the
    // block at the END of this list -- pinned host memory that kernels of this instance write (visibleHost,
    // trackWatch, the mirrors) and every event recorded on the streams below -- while all streams still exist, then
    // device buffers, streams and volumes in the order they have always had.  A constructor that throws half-way
    // releases what it had built the same way.
    const Switches sw = Switches::fromEnvironment();
    Params params;
    TSDF::Gradients gradMode;
    std::shared_ptr<Communicator> comm;
    int rank = 0, world = 1;

    TSDF background;
    std::list<ObjTSDF> objects;          // objects owned by this rank, creation order
    std::vector<int> allIds;             // every object id of the job, creation order
    std::map<int, ObjImages> objImages;  // per owned object
    std::map<int, Stream> streams;       // key 0 = background, else object id
    // Queue priority classes of the frame's three streams: NONE of them in the "normal" class.  HIP serves each class
    // from its own pool of at most four hardware queues, and streams of an embedding application (the reference
    // creates one cv::cuda::Stream per object, EMFusion.h:471) are normal-priority ones: with `main` or `lists` in
    // that class the frame took 0.76-0.91 ms instead of 0.57 for 2, 5, 6 or 9 live foreign streams, and was flat
    // over 0 .. 9 of them with main = high, aux = lists = low (scripts/stream_history_probe.py --matrix3,
    // DESIGN.md section 6; tests/test_gpu_stream_history.py)
    Stream main{sw.prioMain};
    Affine3f pose;                       // current camera pose
    std::set<int> vis_objs;
    int frameCount = 0;
    int nextId = 1;
    FrameInputs pending;

    // frame-sized device images (reference EMFusion.h:447-489)
    emf_image_t depth{};  // view of the current depth map
    // processFrame(const RGBD&): the host depth map goes through one of TWO pinned staging buffers and, on a copy stream
    // of its own, into one of TWO device images, so that the transfer of frame k + 1 runs while frame k's kernels do
    // (what the reference's reader thread + upload amount to, RGBDReader.cpp:72-117, EMFusion.cpp:72); the frame's
    // `main` stream waits for the copy's event.  EMF_ASYNC_UPLOAD=0: hipMemcpyAsync from the caller's pageable memory on
    // `main` (rounds 1-5: the runtime stages it and the host blocks; A/B measurements).
    struct UploadSlot {
        DeviceImage<float> dev;
        PinnedBuffer pinned;
        Event copied;     // the H2D copy out of `pinned` into `dev` is through
        Event frameDone;  // the frame that read `dev` is through (recorded on `main` at its end)
    };
    Stream copyStream{sw.prioCopy};
    uint64_t uploads = 0;
    double uploadHostSeconds = 0.0;  // host time processFrame(RGBD) spent getting the depth map on its way (sum)
    emf_image_t stageDepth(const float* host, int& slotOut);
    std::string maskPath;                              // usePreprocMasks
    std::vector<DeviceImage<uint8_t>> preprocMaskDev;  // the instances of the last mask frame (device copies)
    std::vector<uint8_t> lastMaskVis;
    int lastMaskInstances = 0;
    // ---- motion masks (setMotionMasks; EMFusionLifecycle.cpp) ----
    bool motionOn = false;
    emf_motion_params_t motionParams{};
    DeviceBuffer motionScratch, motionPlanes;   // the kernels' scratch; EMF_MOTION_MAX_MASKS u8 planes
    DeviceBuffer motionInfoDev;                 // EMF_MOTION_MAX_MASKS emf_motion_info_t, then the count
    DeviceImage<int32_t> motionLabels;
    std::vector<emf_motion_info_t> motionInfo;  // the last frame's proposals
    bool motionFired = false;                   // the last frame ran the proposal (motionLabels is that frame's)
    bool motionVisStale = false;                // lastMaskVis is to be drawn from motionLabels when somebody asks
    void ensureMotionBuffers();
    void proposeMotionMasks(std::vector<emf_image_t>& segs);
    // ---- follow the camera (setBackgroundFollow; EMFusionFollow.cpp) ----
    bool followOn = false;
    BackgroundFollowParams followParams;
    Vec3i bgOrigin;                     // cumulative roll, in voxels on the lattice of the initial pose
    bool bgRolled = false;              // the background has been rolled since construction / reset()
    std::vector<RetiredSlab> retired;
    void followCamera();                // the end of a frame with follow on
    void rollBackgroundAt(const Vec3i& shift, int frame, bool keepRetired);
    // ---- the tile store (setBackgroundStore; EMFusionFollow.cpp) ----
    bool storeOn = false;
    WorldMeshInfo worldInfo;  // of the last worldMesh()
    // the tiles a session's map consists of: the table worldMesh() and the world queries read
    struct WorldTiles {
        std::vector<emf_mesh_tile_t> tiles;                      // sorted by (z, y, x), neighbours filled in
        std::map<std::array<int32_t, 3>, int32_t> index;         // key (z, y, x) -> table index
        std::vector<std::array<int32_t, 3>> storedKeys;          // the keys that came from the store
        TileGather stored;                                       // owns the arena
        emf_mesh_tiles_source_t src{};
        WorldMeshInfo info;
        DeviceBuffer tilesDev;
    };
    // refuses for EMFusion::`who` what worldMesh() refuses: the sharded path, a resolution or origin off the tile
    void requireTiledWorld(const char* who, const char* noun) const;
    // after a drain: an unseen-tile map of its own from the front copy, the observed tiles of the volume in place, the
    // stored tiles under their lattice coordinate -- the volume wins --, uploaded.  Waits for the main stream.
    WorldTiles listWorldTiles(const char* who);
    // ---- the world extent of the scene queries (setQueryExtent; EMFusionDistance.cpp) ----
    bool queryWorld_ = false;
    WorldTiles queryTiles;  // of the last world query: alive while its kernels may run
    // the box of writeResults' whole-scene outputs: the background, or worldExtent() with the switch on
    void resultsBox(const char* who, Vec3i& lo, Vec3i& size) const;
    // ---- the distance field (distanceField; EMFusionDistance.cpp): allocated at first use, never in a checkpoint ----
    DistanceField dfLast;
    DeviceBuffer dfClasses, dfD2, dfMetres, dfNearest, dfNearestScratch, dfQuery;
    bool expDistance_ = false, distanceUnknownObstacle_ = false;  // setDistanceOutput
    bool expDistanceNearest_ = false;                             // setDistanceNearestOutput
    float distanceCapMetres_ = 0.f;
    // the steps the scene queries share: the box -- unchecked, and checked for EMFusion::`who`, whose
    // refusal on the sharded path reads "`noun` not supported ..." --, the drain, classes + stamped objects into
    // `classes`, and the clearance of frontiers() and plan()
    QueryBox queryBoxAt(const Vec3i& lo, const Vec3i& size) const;
    // volumeOnly: a query that reads the volume itself (planes) keeps to the background whatever the extent
    QueryBox makeQueryBox(const char* who, const char* noun, const Vec3i& lo, const Vec3i& size, bool volumeOnly = false) const;
    void drainForQuery();
    void enqueueOccupancy(const char* who, const QueryBox& box, const std::vector<int>& excludeIds, uint8_t* classes,
                          std::vector<int>* ids, std::vector<Affine3f>* poses);
    struct Clearance {
        const int32_t* d2;  // device: the capped transform with sites = occupied, or NULL without a clearance
        int32_t minD2;
    };
    // into clearanceD2, which both callers consume on the main stream before they return: no result points into it
    Clearance enqueueClearance(const char* who, const QueryBox& box, const uint8_t* classes, int clearanceVoxels);
    DeviceBuffer clearanceD2;
    void castOnDevice(const char* who, const QueryBox& box, const uint8_t* classes, const Clearance& clear, uint32_t passMask,
                      uint32_t countMask, const std::vector<int32_t>& from, const std::vector<int32_t>& to, int group, bool wantResults,
                      std::vector<emf_ray_result_t>& results, std::vector<emf_ray_group_t>& groups);
    // ---- frontiers (frontiers; EMFusionFrontier.cpp): allocated at first use, never in a checkpoint ----
    Frontiers frLast;
    DeviceBuffer frClasses, frLabels, frCounters, frScratch, frRecords;
    bool expFrontiers_ = false;  // setFrontierOutput
    int frontierMinVoxels_ = 8;
    float frontierClearanceMetres_ = 0.f;
    // ---- planning (plan; EMFusionPlan.cpp): allocated at first use, never in a checkpoint ----
    Plan plLast;
    DeviceBuffer plClasses, plCost, plScratch, plCounters, plSeeds, plGoals, plPaths, plLengths, plGoalCost;
    bool expPlan_ = false, planThroughUnknown_ = false;  // setPlanOutput
    float planClearanceMetres_ = 0.f;
    TileStore bgStore;
    void retireSlabs(const Vec3i& shift, int frame);
    DeviceImage<float> depthFiltered;  // output of preprocessDepth
    DeviceImage<float> invLambda;  // per-pixel 1 / lambda of the integration, fixed by the intrinsics (sw.useLambdaTable)
    DeviceBuffer integrateCullScratch;  // survivor list of emf_hip_integrateBatchedCulled (empty: plain launch)
    bool ignorePerson = false;
    int depthRoot = -1;  // sharded path: rank whose depth image is broadcast each frame (-1: none)

    // ---- object creation / matching (SURVEY f-3) ----
    emf_point_stats_t maskedStats(const emf_image_t& mask, const Affine3f& frame);  // synchronises
    DeviceBuffer statsScratch, statsDev, overlapDev;
    std::vector<int> lastCreated, lastDeleted, lastAssigned;
    bool poseLog = false;
    std::map<int, Affine3f> poses;                    // frame -> camera pose
    std::map<int, std::map<int, Affine3f>> obj_poses;  // id -> frame -> pose
    std::map<int, std::map<int, Vec3f>> obj_pose_offsets;  // id -> frame -> centre shift of resize()
    std::array<uint8_t, 768> colorMap = io::randomColors();
    DeviceImage<uint8_t, 3> image;  // rendering
    // ---- free-viewpoint view (EMFusionView.cpp) ----
    DeviceBuffer viewPosesDev;
    DeviceBuffer viewTableDev;  // per-volume path: the host table uploaded for the view (no device table there)
    DeviceImage<uint8_t, 3> viewImage;
    DeviceImage<float> viewRay;
    DeviceImage<uint8_t> viewSeg;
    DeviceImage<float, 3> viewVert, viewNorm;  // colour shading only: what the view kernel hit, for the pixel pass
    DeviceImage<uint8_t, 3> viewColor;         // ... and the colour sampled under every pixel
    int view3dShading = 0;
    bool view3d = false;  // set3dView: render() renders (and logs) this view too
    Affine3f view3dPose;
    float view3dK[9] = {};
    Size view3dSize;
    std::vector<uint8_t> view3dRgb;
    void render3dView();  // render()'s part: the 3D view of set3dView, logged under frameCount - 1
    std::map<int, Mesh> meshes;                            // id -> last mesh (deleted objects keep theirs)
    // ---- per-frame meshes (setupOutput's exp_frame_meshes, EMFusionCapture.cpp) ----
    bool expFrameMeshes_ = false;
    bool expWorldMesh_ = false;  // setWorldMeshOutput: writeResults also writes world.ply
    std::map<int, Mesh> frame_meshes;                      // frame -> background mesh
    std::map<int, std::map<int, Mesh>> frame_obj_meshes;   // id -> frame -> mesh
    void storeFrameMeshes();                               // the end of a frame with exp_frame_meshes
    DeviceBuffer meshTableDev, meshCountsDev, meshScratch, meshArena;  // extractMeshes' pooled buffers
    bool meshWeld = false;                                 // setMeshWeld
    DeviceBuffer meshKeysDev, meshColorPtrsDev;            // the soup's grid-edge keys; the models' colour volumes
    MeshPost meshPost;                                     // weld -> filter -> simplify and the download (MeshPost.hpp)
    uint32_t meshMinTriangles = 0;                         // setMeshFilter
    bool meshLargestObjects = false;
    std::map<int, MeshFilterStats> meshFilterStats;        // lastMeshFilter
    float meshSimplifyCell = 0.f;                          // setMeshSimplify
    std::map<int, MeshSimplifyStats> meshSimplifyStats;    // lastMeshSimplify
    bool meshSimplifyActive() const { return meshSimplifyCell > 0.f; }
    MeshFilter meshFilterFor(int id) const {               // the background keeps its pieces
        return MeshFilter{meshMinTriangles, meshLargestObjects && id != 0, meshSimplifyCell};
    }
    bool meshFilterActive() const { return meshMinTriangles > 1 || meshLargestObjects; }
    void meshColors(const std::vector<int>& ids, const std::vector<int32_t>& res, uint64_t nv, DeviceBuffer& cDev);
    void extractWelded(const std::vector<int>& ids, const std::vector<int32_t>& res, uint64_t nv, uint64_t nt,
                       std::vector<Mesh>& out);
    bool expVols = false;                                  // setupOutput: keep / dump volumes too
    // ---- per-frame debug images of the reference's saveOutput mode, kept as encoded PNGs ----
    bool saveOutput = false;
    using ImageLog = std::map<int, std::vector<uint8_t>>;  // frame -> PNG bytes
    ImageLog meshVis;  // the 3D view of each rendered frame (mesh_vis_out/, set3dView)
    ImageLog renderings, bg_assocWeight_preTrack, bg_assocWeight_postTrack, bg_huberWeights, bg_trackWeights;
    std::map<int, ImageLog> obj_assocWeights_preTrack, obj_assocWeights_postTrack, obj_huberWeights, obj_trackWeights,
        obj_fgProbs;                                       // id -> frame -> PNG bytes
    std::vector<uint8_t> pngOf(const float* dev, size_t pitchBytes);  // x 255 -> u8 -> PNG; synchronises `main`
    void storeAssocs(ImageLog& bg, std::map<int, ImageLog>& objs);    // EMFusion.cpp:307-320
    void storeTrackWeights(int first, int count);                     // behind a tracking stage
    void storeFgProbs();                                              // behind the frame's last E-step
    DeviceBuffer logScratch;                                          // 2 x EMF_MAX_BATCH float images
    struct SavedVolumes {                                  // tsdfs / intWeights / fgProbs / meta of the reference
        std::vector<float> tsdf, weights, fgProbs;
        std::vector<uint16_t> color;                       // colour on only: u16 x 4 per voxel
        Vec3i res;
        float voxelSize = 0.f;
    };
    static SavedVolumes saveVolumes(ObjTSDF& obj);
    std::map<int, SavedVolumes> savedVolumes;              // id -> volumes of objects deleted while the log was on
    DeviceBuffer massDev;       // cleanUpObjs: EMF_MAX_MODELS emf_mask_mass_t, one answer per object
    DeviceBuffer massScratch;   // ... the row-band partials (emf_hip_maskAssociationMassScratchBytes)
    DeviceBuffer verdictDev;    // ... sharded: EMF_MAX_MODELS float verdicts by list position (all-reduced)
    DeviceBuffer lifecycleMsg;  // sharded: the 16-byte messages of initNewObjVolume / updateObject
    void deleteObj(int id);
    // cleanUpObjs' removal of an object of this rank; absorb: into the background first (setAbsorbObjects)
    // keep = false (mergeObjects): neither its mesh nor its exp_vols copy is kept
    void deleteOwned(std::list<ObjTSDF>::iterator it, bool absorb = false, bool keep = true);
    void ensureLifecycleBuffers();
    // layout of lifecycleHost: emf_point_stats_t / 513 x u32 / EMF_MAX_MODELS x emf_mask_mass_t, then EMF_MAX_MODELS
    // floats (verdicts, messages), then EMF_MAX_MODELS int32 (gate)
    static constexpr size_t kLcVerdictOff = EMF_MAX_MODELS * sizeof(emf_mask_mass_t);
    static constexpr size_t kLcGateOff = kLcVerdictOff + EMF_MAX_MODELS * sizeof(float);
    static constexpr size_t kLcHostBytes = kLcGateOff + EMF_MAX_MODELS * sizeof(int32_t);

    // ---- tracking (SURVEY f-1) ----
    void trackModels(int first, int count);    // LM-ICP of table slots [first, first + count)
    int trackPredicted[2] = {0, 0};            // iterations the camera / object stage took last frame
    int trackWindow = sw.trackWindow;          // launches kept ahead of the device's progress report (0: poll in chunks; set to 0 when trackWatch cannot be allocated); 2 ... 6 measured: 4 leaves a stage 3 idle launches instead of 5
    uint32_t trackStageTag = 0;                // upper half of the words of the stage in flight (trackModels)
    DeviceBuffer trackStates;                  // emf_track_state_t[EMF_MAX_MODELS]
    DeviceBuffer trackScratch;                 // one emf_hip_trackScratchBytes block per table slot (grown on demand)
    std::map<int, TrackResult> trackResults;   // by model id
    DeviceImage<float, 3> points;
    DeviceImage<float> raylengths, bg_raylengths, associationNorm, bg_associationWeights,
        diffRaylengths, objPartialSum;
    DeviceImage<float, 3> vertices, normals, bg_vertices, bg_normals;
    DeviceImage<uint8_t> modelSegmentation, bg_mask, noObjMask, occludedMask;
    DeviceBuffer visCounts;      // int32 per object
    DeviceBuffer hitKeys;        // u64 W x H, multi-GPU composite merge
    DeviceBuffer raycastStatsDev;  // 2 x u64
    bool statsOn = false;

    // device-resident model table for the batched launches (slot 0 = background)
    bool batched = true;            // false: per-volume launches (sw.perVolume or materialised gradients, see EMFusion.cpp)
    bool sharded = false;           // objects sharded over ranks: use the cross-rank exchanges
    DeviceBuffer modelTable;        // 2 x emf_model_t[EMF_MAX_MODELS]: [1] has the background's two copies swapped
    int tableSel = 0;               // which of the two describes the background's current front copy
    const emf_model_t* currentTable() const { return modelTable.as<emf_model_t>() + tableSel * EMF_MAX_MODELS; }
    // A launch takes at most EMF_MAX_BATCH table slots (its poses travel by value in the kernel arguments); a longer
    // model list -- the reference loops over any number of objects, EMFusion.cpp:635-670, 726-795, 865-889 -- is served
    // in chunks of the table: f(first slot, count) for the slots [first, n), cut at multiples of EMF_MAX_BATCH, so
    // that the chunk holding slot 0 is the only one with the background in it.
    template <class F>
    static void forChunks(int first, int n, F&& f) {
        while (first < n) {
            const int end = std::min(n, (first / EMF_MAX_BATCH + 1) * EMF_MAX_BATCH);
            f(first, end - first);
            first = end;
        }
    }
    int launchChunks() const { return (static_cast<int>(modelsHost.size()) + EMF_MAX_BATCH - 1) / EMF_MAX_BATCH; }
    uint32_t chunkMask(const std::vector<uint8_t>& flags, int first, int count) const {
        uint32_t m = 0;
        for (int k = 0; k < count; ++k) m |= flags[first + k] ? 1u << k : 0u;
        return m;
    }
    // Background kept twice (TSDF::enableDoubleBuffer): its integration runs out of place on `aux`,
    // concurrently with the raycast of the same frame, and the copies are flipped at the join.
    // EMF_BG_OVERLAP=0 keeps the reference's sequence raycast -> integrate (A/B measurements).
    bool bgInFlight = false;        // the out-of-place integration of this frame has been enqueued
    bool bgBackStale = false;       // the background was integrated in place: the copies differ
    // the background's sweep yields to the raycast when both have workgroups to place (its long chains should
    // start as early as they can): lowest queue priority for the second stream (+1 % frames/s)
    Stream aux{sw.prioAux};
    // Raycast far bounds (emf_hip_raycastFarBounds): per model and 8x8-pixel cell, where a march may
    // stop because nothing can be hit any more.  EMF_FAR_BOUNDS=0 marches every ray to the end.
    DeviceBuffer farBounds;       // two halves, written alternately (computeFarBounds)
    int farSel = 0;
    float* farBoundsHalf() const { return farBounds.as<float>() + static_cast<size_t>(farSel) * (farBounds.bytes() / 2 / sizeof(float)); }
    int forkFrame = -2;           // frame whose integrateBackgroundAsync forked `aux` (and re-recorded `main`'s event)
    bool farBoundsReady = false;
    bool peerFused = false;     // sharded over a direct peer-write transport: exchanges fused into the path's kernels
    int bandRowsPending = 0;    // background raycast bands waiting for the raycast's exchange
    Stream lists{sw.prioLists};  // relevant-tile list rebuilds: behind the integrations, waited for by the next far bounds
    bool bgListPending = false; // the background was forked; its list rebuild is not enqueued yet
    bool bgPrepared = false;    // bgCullScratch's counter and the next dirtyNext map are already cleared
    void rebuildBackgroundList();
    void computeFarBounds(const std::vector<emf_pose_t>& co);
    void joinFarBounds();
    DeviceBuffer bgCullScratch;     // box list of the background's own launch
    bool overlapUsable() const;
    void integrateBackgroundAsync();  // fork: enqueue on aux what integrateDepth() would do for slot 0
    void joinBackground();
    std::vector<emf_model_t> modelsHost;
    std::vector<int32_t> resHost;   // 3 per model
    std::vector<float> voxelHost;   // voxel size per model (object footprints of the batched raycast)
    std::vector<uint8_t> scanSlot, listSlot;  // far bounds, per table slot: sign maps scanned / keeps a relevant-tile list
    bool anyScan = false;
    DeviceBuffer visibleDev;        // int32 per model slot: integrate gate, written on the device
    DeviceBuffer integrateStatsDev; // u64: voxels swept by integrateBatched
    // ---- per-voxel colour (enableColor) ----
    bool colorOn = false;
    bool colorImageSet = false;     // colorImage goes with the next integration, and with that one only
    emf_image_t colorImage{};
    DeviceBuffer colorTable;        // uint16_t* per table slot, parallel to the model table (emf_model_t keeps its layout)
    DeviceBuffer colorStatsDev;     // u64: voxels coloured
    DeviceBuffer rgbUpload;         // device copy of RGBD::rgb (processFrame(const RGBD&))
    void integrateColor(const std::vector<emf_pose_t>& oc);
    bool visPending = false;
    std::vector<int32_t> visIds;    // object ids in the order of the pending counts

    KernelTimers ktimers;
    bool timingsOn = false;
    FrameTimings timings;

    // ---- pinned host memory and events: declared last, released first (see the top of the member list) ----
    UploadSlot uploadSlots[2];
    PinnedBuffer visCountsHost;    // int32 per object: the counts the host gate waits for
    PinnedBuffer visibleHost;      // int32 per object: mirror of visCounts for visibleObjects(), written by the gate kernels
    PinnedBuffer trackStatesHost;  // emf_track_state_t[EMF_MAX_MODELS]: mirror of trackStates
    PinnedBuffer trackWatch;       // mapped: the words the step kernel reports to while the stream runs (empty: chunked polls)
    PinnedBuffer lifecycleHost;    // kLcHostBytes, layout above
    PinnedBuffer motionHost;       // mirror of motionInfoDev
    PinnedBuffer viewPosesHost;    // EMF_MAX_MODELS viewer -> volume poses
    PinnedBuffer meshHost;         // EMF_MAX_MODELS emf_model_t, then the counts and bases read back
    std::vector<Event> stamps;     // the frame timings' marks on `main`

    // ---- voxel rays (castRays, viewGain, shortcutPlan; EMFusionRays.cpp): allocated at first use, never in a checkpoint.
    // Behind everything else so that the members the frame path touches stay where they were; ~EMFusion has waited for
    // the device before any member goes ----
    Rays ryLast;
    DeviceBuffer ryClasses, ryEnds, ryResults, ryGroups;
    uint64_t clearanceSerial = 0;    // counts the transforms written into clearanceD2 (5.18a)
    uint64_t plClearanceSerial = 0;  // ... and which of them is the gate of the last plan
    int plShortcutWindow = 0;        // of the last shortcutPlan on the last plan, 0: none
    int planShortcutWindow_ = 0;     // setPlanShortcutOutput

    // ---- object shapes (objectShapes; EMFusionShape.cpp): allocated at first use, never in a checkpoint; behind all
    // existing members ----
    std::vector<ObjectShape> shLast;
    DeviceBuffer shScratch;          // the compact model table, the moments, the frames and the extents of one call
    bool expShapes_ = false;         // setShapeOutput

    // ---- ground map (groundMap; EMFusionGround.cpp): allocated at first use, never in a checkpoint; behind all
    // existing members ----
    GroundMap gmLast;
    DeviceBuffer gmBoxClasses, gmPlanes, gmCells, gmClasses;  // the box's classes, occ + fre, the records, the 2-D classes
    GroundOutput expGround_;         // setGroundOutput

    // ---- planes (planes; EMFusionPlanes.cpp): allocated at first use, never in a checkpoint; behind all existing
    // members ----
    Planes pnLast;
    DeviceBuffer pnRecords, pnLabels, pnScratch, pnSmall;  // the records, their labels, the tiles' counts; counters, moments and votes
    PlanesOutput expPlanes_;         // setPlanesOutput
    // ---- plane patches (planePatches; EMFusionPlanes.cpp): as the planes' buffers
    PlanePatches ppLast;
    PlanePatchesOutput expPatches_;  // setPlanePatchesOutput
    uint32_t pnCapacity = 0;         // the capacity planes() gave stage 1: what the later stages bound the count by
    DeviceBuffer ppIds, ppScratch, ppOut, ppSmall;  // the ids, the slots' scratch, the records, the three counters
    bool expGroundUpFloor_ = false;  // setGroundUpFloor

    // ---- object contacts (objectContacts; EMFusionContacts.cpp): allocated at first use, never in a checkpoint;
    // behind all existing members ----
    ObjectContacts ctLast;
    DeviceBuffer ctScratch;          // the compact model table, the pairs and the records of one call
    bool expContacts_ = false;       // setContactsOutput
    double expContactTouch_ = -1.0;

    // ---- absorbing objects (setAbsorbObjects, absorbObject; EMFusionAbsorb.cpp): never in a checkpoint; behind all
    // existing members ----
    bool absorbOn_ = false;          // setAbsorbObjects
    bool absorbDirty_ = false;       // the background's front copy was written and volumesWritten() is still owed
    std::vector<AbsorbEvent> absorbLog_;
    DeviceBuffer absorbRecord_;      // one emf_absorb_t, then one emf_color_moved_t
    bool expAbsorbed_ = false;       // setAbsorbedOutput
    void absorbInto(ObjTSDF& obj);   // the launch and the log entry, on main; the caller has quiesced
    void absorbFinish();             // volumesWritten once after the last absorption, before rebuildModelTable()
    // the live object `id` of this rank for absorbObject / liftObject, or the HipError (EMF_E_ARG) that says why not:
    // `background` for id 0, "not owned by this rank", "no object"
    std::list<ObjTSDF>::iterator ownedObjectOrThrow(const char* who, int id, const char* background);
    // Runs `write`, which writes the background's front copy or an object's volume from outside the integration, and
    // renews what is derived from them -- absorbFinish(), rebuildModelTable() -- whether it returns or throws.
    template <typename Write>
    void writeThenRenew(Write&& write) {
        try {
            write();
        } catch (...) {
            absorbFinish();
            rebuildModelTable();
            throw;
        }
        absorbFinish();
        rebuildModelTable();
    }
    // a pass's launch on main (its return code), the copy of its record to the host -- and of its colour record, where it
    // has one -- and the wait
    template <typename Record>
    void launchedRecord(int rc, const char* what, const Record* dev, Record* host, const emf_color_moved_t* colorDev = nullptr,
                        emf_color_moved_t* colorHost = nullptr) {
        emfCheck(rc, what);
        hipCheck(hipMemcpyAsync(host, dev, sizeof(Record), hipMemcpyDeviceToHost, main.get()), what);
        if (colorDev) hipCheck(hipMemcpyAsync(colorHost, colorDev, sizeof(emf_color_moved_t), hipMemcpyDeviceToHost, main.get()), what);
        main.waitForCompletion();
    }
    // the covering box of the object's cube in the voxels of dst (the background, or another object) and whether dst's cube clips it
    void absorbBox(const TSDF& dst, const ObjTSDF& obj, const float R[9], const float t[3], int32_t lo[3], int32_t size[3], bool& clipped);
    // ---- lifting objects (setLiftObjects, liftObject; EMFusionLift.cpp): never in a checkpoint; with the switch off no
    // launch of the frame changes
    bool liftOn_ = false;            // setLiftObjects
    std::vector<LiftEvent> liftLog_;
    std::vector<LiftEvent> liftPending_;  // seeded in this frame, the release still owed
    DeviceBuffer liftRecord_;        // one emf_seed_t, one emf_release_t, then their two emf_color_moved_t
    bool expLifted_ = false;         // setLiftedOutput
    void liftSeed(ObjTSDF& obj, LiftEvent& e);     // the launch on main; the caller has quiesced
    void liftRelease(ObjTSDF& obj, LiftEvent& e);  // the launch on main and the log entry; the caller has quiesced
    void liftSeedCreated();          // runSchedule: after integrateDepth(), before integrateMasks()
    void liftReleaseCreated();       // runSchedule: after integrateMasks(), before cleanUpObjs
    // ---- merging objects (mergeObjects, setMergeObjects; EMFusionMerge.cpp): never in a checkpoint; with the switch off
    // and no call nothing changes
    bool mergeOn_ = false;           // setMergeObjects
    bool expMerged_ = false;         // setMergedOutput
    MergeParams mergeParams_;
    MergeEvent mergeInto(int dstId, int srcId, bool automatic, double overlapDS, double overlapSD);
    void mergeDuplicates();          // runSchedule: the end of a mask frame, after cleanUpObjs
    std::vector<MergeEvent> mergeLog_;
    DeviceBuffer mergeRecord_;       // one emf_absorb_t, one emf_merge_counts_t, one emf_color_moved_t; the growth's table and moments
};

/**
 * The integer ray targets of one candidate view, on the host, without a device.  (R, t): viewer ->
 * world, OpenCV camera; fx, fy, cx, cy: the intrinsics of a gw x gh grid image; range in metres; then the background's
 * pose, resolution and voxel size and the box origin.  origin: the box voxel under the camera, by the rounding of
 * QueryBox::voxelAt; targets: 3 * gw * gh i32, cell (i, j) at j * gw + i.  Everything in float64, every line a single
 * operation in this order:
 *     x = (i - cx) / fx;  y = (j - cy) / fy
 *     m = sqrt(x * x + y * y + 1.0)                  summed left to right
 *     c = (x / m, y / m, 1.0 / m)
 *     M = bgR^T * R                                  each element a three-term sum left to right, once per view
 *     dir = M c                                      rows summed left to right
 *     target = origin + rint(dir * (range / voxel))  ties to even
 * A value outside the i32 range is clipped to it, one that is not finite becomes -1.  range / voxel above
 * EMF_RAY_MAX_DELTA is EMF_E_ARG.
 */
void viewRayTargets(const double R[9], const double t[3], double fx, double fy, double cx, double cy, int gw, int gh, double range,
                    const float bgR[9], const float bgT[3], const Vec3i& bgRes, float voxelSize, const Vec3i& boxLo,
                    int32_t origin[3], int32_t* targets);

/**
 * The greedy choice of EMFusion::shortcutPlan over a path p_0 .. p_k: from i the largest j in i + 2 .. min(i + window, k)
 * with reached[rowStart[i] + (j - i - 2)] set, else i + 1, until k.  The ascending indices from 0 to k; empty for k < 0.
 */
std::vector<int32_t> shortcutGreedy(int k, int window, const std::vector<uint8_t>& reached, const std::vector<size_t>& rowStart);

/**
 * The frame of a model from its integer moments, on the host, without a device: centroid, covariance,
 * cyclic Jacobi with EMF_SHAPE_JACOBI_SWEEPS sweeps, axes sorted by eigenvalue and signed, rounded to f32 once for the
 * extents pass.  Float64 in the operation order written out in include/emf_hip.h "Object shapes".  mom.solid == 0 sets
 * valid = 0 and writes nothing else.
 */
void shapeFrame(const emf_shape_moments_t& mom, emf_shape_frame_t& out);
/** The host steps of the plane finder (include/emf_hip.h "Planes"): float64 in a fixed operation order, no device. */
struct PlaneDirection {
    int bin = 0;
    uint32_t votes = 0;
    double n[3] = {0.0, 0.0, 0.0};
};
struct PlaneOffsetFrame {
    double lo = 0.0, invBin = 0.0, shift = 0.0;
    int64_t slots = 0;
};
void planeCellCentre(int bin, int K, double n[3]);
std::vector<PlaneDirection> planeDirections(const uint32_t* bins, int K, uint32_t minVotes, double separationDeg);
PlaneOffsetFrame planeOffsetFrame(const double n[3], const int32_t size[3], double binVox);
std::vector<std::pair<int, uint32_t>> planePeaks(const uint32_t* row, int slots, uint32_t minVotes, int peakGap);
void planeFit(const emf_plane_moments_t& mom, const double seedN[3], double seedD, emf_plane_t& out);
/** The fit, the rectangle and the fill of a patch from its plane (include/emf_hip.h, the host steps behind stage 4). */
void planePatchRect(const emf_plane_t& plane, const emf_plane_patch_t& patch, emf_plane_patch_rect_t& out);
/**
 * One oriented box against one patch, world metres: s = (n . c - d) - sum_k |n . A_k| * h_k, the height
 * of the box's lowest point above the patch's plane, and whether the box centre, in the rectangle's axes about its
 * centre, lies within half + margin.  Float64, every line a single operation, sums left to right.
 */
bool planeSupport(const double n[3], double d, const double center[3], const double axes[6], const double half[2],
                  const double boxCenter[3], const double boxAxes[9], const double boxHalf[3], double margin, double& s);
/**
 * The box of a model from its frame and its extents along that frame: centre and half extents in voxels, completeness,
 * then metres in the model's own frame and the world frame through its pose (R, t: volume -> world).  Float64 in the
 * order of the header.  For a frame with valid != 0.
 */
void shapeBox(const emf_shape_moments_t& mom, const emf_shape_frame_t& frame, const emf_shape_extents_t& ext, const int32_t res[3],
              float voxelSize, const float R[9], const float t[3], emf_shape_box_t& out);

/**
 * The host stage of the object contacts, without a device: float64, every line a single operation in the
 * order written out in include/emf_hip.h "Object contacts".  contactPose: what a pair carries (b's frame <- a's frame)
 * from the two poses (world <- model), rounded to f32 once.  contactTouch: metres -> units of b's stored tsdf.
 * contactSummary: the unordered pair from the record a -> b and, where there is one, b -> a (else nullptr).
 */
void contactPose(const float Ra[9], const float ta[3], const float Rb[9], const float tb[3], float R[9], float t[3]);
/**
 * What an absorption carries: (R, t) taking the DESTINATION's volume frame into the SOURCE's, from the
 * poses (world <- volume) of the destination d and the source s, float64 in the fixed order of contactPose with a = d and
 * b = s, rounded to f32 once: R_ij = float((Rs_0i * Rd_0j + Rs_1i * Rd_1j) + Rs_2i * Rd_2j), t likewise from td - ts.
 */
void absorbPose(const float Rd[9], const float td[3], const float Rs[9], const float ts[3], float R[9], float t[3]);
/**
 * The growth of a merge (EMFusion::mergeObjects), without a device: the box of the destination's volume
 * frame, in metres, that holds the destination's band and the source's.  dLo, dHi / sLo, sHi: the inclusive bounds in
 * voxels of the two bands (emf_shape_moments_t lo, hi; hi[0] < 0: no solid voxel, the object adds nothing); (R, t): the
 * destination's volume frame <- the source's, float32.  Float64, every line a single operation in this order:
 *     c_j = (double(v_j) - (double(N_j) - 1.0) / 2.0) * double(voxelSize)       a bound on axis j
 *     x_i = ((R_i0 * c_0 + R_i1 * c_1) + R_i2 * c_2) + t_i                       each of the source's eight corners
 *     lo_i, hi_i = the minimum and the maximum over those and the destination's own c, rounded to float32 once
 * Returns false, lo and hi untouched, where neither object has a solid voxel.
 */
bool mergeUnion(const int32_t dLo[3], const int32_t dHi[3], const int32_t dRes[3], float dVoxel, const int32_t sLo[3],
                const int32_t sHi[3], const int32_t sRes[3], float sVoxel, const float R[9], const float t[3], float lo[3], float hi[3]);
float contactTouch(double touchMetres, float truncdistB);
void contactSummary(const emf_contact_t& ab, const emf_contact_t* ba, const emf_contact_side_t& a, const emf_contact_side_t& b,
                    emf_contact_summary_t& out);

/**
 * The frame of a ground map, on the host, without a device: float64 in the operation order written out
 * in include/emf_hip.h "Ground map", G rounded to f32 once.  pose: "ground metres -> world", R row-major with (u, v, h)
 * as columns, then t.  Returns EMF_OK, or EMF_E_ARG / EMF_E_LIMIT with the reason in `why`.
 */
int groundFrame(const QueryBox& box, const double up[3], double cell, double bin, const double ref[3], double bandLo,
                double bandHi, emf_ground_frame_t& frame, double pose[12], std::string& why);
/** Is up along a box axis to within float rounding of the frame: in every row of G all entries but the largest are at
 *  most 2^-20 of it.  Only then slots narrower than two voxels leave no holes. */
bool groundFrameAligned(const emf_ground_frame_t& frame);
/** Metres to height bins, in float as metresToVoxels: the robot's height rounded up and at least 1, the step rounded down
 *  -- both err on the careful side. */
inline int groundRobotBins(float height, float bin) {
    return std::max(static_cast<int>(std::min(std::ceil(height / bin), 4096.f)), 1);
}
inline int groundStepBins(float step, float bin) {
    return step > 0.f ? static_cast<int>(std::min(std::floor(step / bin), 4096.f)) : 0;
}

}  // namespace emf
