// emfusion_synth.cpp -- the reference's main loop (apps/EM-Fusion.cpp:139-156: read a frame,
// emf.processFrame(frame)) on the MI355X-native classes, fed by the deterministic synthetic RGB-D
// stream instead of a dataset reader.  Prints frames/s and per-stage GPU milliseconds.
//
//   emfusion_synth [--frames N] [--objects K] [--bg-res R] [--obj-res R] [--width W --height H]
//                  [--materialize-gradients] [--autonomous] [--out DIR] [--export-frame-meshes] [--3d-vis]
//                  [--weld-meshes] [--mesh-min-triangles N] [--mesh-largest-object] [--mesh-simplify CELL] [--world-mesh]
//                  [--distance-field] [--distance-cap M] [--distance-unknown-obstacle] [--distance-nearest]
//                  [--frontiers] [--frontier-min-voxels N] [--frontier-clearance M]
//                  [--plan] [--plan-clearance M] [--plan-through-unknown] [--plan-shortcut W] [--object-shapes]
//                  [--object-contacts] [--contact-touch M] [--absorb-objects] [--turn-away F] [--lift-objects]
//                  [--merge-objects] [--merge-overlap F] [--merge-max-res N]
//                  [--ground-map] [--ground-up X,Y,Z] [--ground-cell M] [--ground-bin M] [--ground-band LO,HI]
//                  [--ground-robot-height M] [--ground-max-step M] [--planes] [--planes-angle DEG] [--planes-min-votes N]
//                  [--plane-patches] [--plane-patch-reach R] [--plane-patch-min N]
//   emfusion_synth --sequence DIR/ [--masks DIR] [--mask-frames N] [--visibility-thresh N] [--frames N]
//                  [--bg-res R] [--bg-voxel M] [--obj-res R] [--volumes] --out DIR
//   emfusion_synth --dir BASE/ [--colordir colour] [--depthdir depth] [--intrinsics fx fy cx cy] ... --out DIR
// --export-frame-meshes (needs --out): the reference's per-frame mesh export (apps/EM-Fusion.cpp:240-242) -- every
// frame ends by meshing the background and every shown object, and writeResults writes them as
// DIR/frame_meshes/bg/%04d.ply and DIR/frame_meshes/<id>/%04d.ply.
// --weld-meshes: every mesh written (mesh_*.ply of the live models, frame_meshes/) is welded by grid edge on the device:
// one vertex per edge instead of one per cube that touches it, the triangles re-indexed (EMFusion::setMeshWeld).
// --mesh-min-triangles N / --mesh-largest-object: every mesh written is filtered by connected component on the device
// (EMFusion::setMeshFilter): components of fewer than N triangles are removed from every model and, with
// --mesh-largest-object, every component but the largest from the object meshes.  Either implies --weld-meshes; both
// are set again after --resume (a checkpoint does not store them).
// --mesh-simplify CELL: every mesh written, world.ply and the slabs retired from then on included, is simplified on the
// device behind the weld and the filter (EMFusion::setMeshSimplify): the vertices of a model that share a cubic cell of
// CELL metres become one vertex, collapsed triangles are dropped.  Implies --weld-meshes; set again after --resume.
// --3d-vis (needs --out): the reference's 3D view (apps/EM-Fusion.cpp:118-131) -- every frame is rendered (render())
// together with the whole map seen from a viewer 1 m behind the world origin at 1024 x 768, and writeResults writes
// those views as DIR/mesh_vis_out/%04d.png.  --3d-vis-eye x y z --3d-vis-target x y z place the viewer instead
// (looking from eye at target, world -y up).
// --color (with --sequence / --dir): the sequence's colour images (8-bit RGB / RGBA PNG) are fused into per-voxel colour
// volumes beside the TSDFs, and mesh_*.ply, frame_meshes/ and the volume dump carry colours.  Refused for the
// synthetic stream, which has no colour image.
// --configfile FILE (-c): with --sequence / --dir, take every parameter from one of the reference's configuration files
// (config/default.cfg, tum.cfg ...; core/Config.hpp) instead of the sizing options above.
// --dir: the same loop on a Co-Fusion style dataset (ColorNNNN.png + DepthNNNN.exr), the reference's ImageReader
// (apps/EM-Fusion.cpp:118-126; core/Readers.hpp ImageReader + readExr).
// --sequence: the reference's loop itself (apps/EM-Fusion.cpp:100-156) on a TUM RGB-D sequence: TUMRGBDReader
// (core/Readers.hpp) -> emf.usePreprocMasks(masks) -> processFrame(frame) with camera and object tracking from the
// second frame on -> writeResults.  What apps/run_tum.py does from Python, without Python.
// --out DIR: keep the pose log and write the reference's result files at the end (writeResults:
// poses-*.txt, mesh_*.ply, tsdfs/*.bin; EMFusion.cpp:258-292) into the existing directory DIR.
// --autonomous: nothing but depth and instance masks go in, as in the reference's own loop -- objects
// are spawned from the masks of frame 0 (initNewObjVolume), camera and object poses are tracked
// (performTracking), later masks are matched to the models (matchSegmentation); the ground-truth
// poses of the stream are only used to report the tracking error at the end.
// --motion-masks [--motion-band M] [--motion-min-pixels N] [--motion-max-masks N]: no instance masks go in either --
// every mask frame (--mask-frames N) proposes its own from the depth that lies more than M metres (default: the
// background's truncation distance) in front of the background model (EMFusion::setMotionMasks).
// Excludes --masks.  With --autonomous it replaces the generator's masks, and the spheres enter the scene at frame 5
// (the first frames show the empty room): what is there from the start and hardly moves belongs to the background.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Config.hpp"
#include "EMFusion.hpp"
#include "Readers.hpp"
#include "SyntheticScene.hpp"

// --3d-vis: the viewer of the reference's window (apps/EM-Fusion.cpp:127-130: setCamera(intr, frameSize),
// setViewerPose(translate(0, 0, -1)), 1024 x 768), or a camera at `eye` looking at `target`
struct View3d {
    bool on = false, placed = false;
    float eye[3] = {0.f, 0.f, -1.f}, target[3] = {0.f, 0.f, 0.f};
};
static void set3dView(emf::EMFusion& emf, const emf::Params& params, const View3d& v) {
    if (!v.on) return;
    const emf::Size size(1024, 768);
    const float sx = static_cast<float>(size.width) / static_cast<float>(params.frameSize.width),
                sy = static_cast<float>(size.height) / static_cast<float>(params.frameSize.height);
    const float K[9] = {params.intr(0, 0) * sx, 0.f, params.intr(0, 2) * sx, 0.f, params.intr(1, 1) * sy,
                        params.intr(1, 2) * sy, 0.f, 0.f, 1.f};
    emf::Matx33f R = emf::Matx33f::eye();
    if (v.placed) {  // OpenCV camera axes in world coordinates: z forward, x = down x z, y = z x x (down = +y)
        float z[3] = {v.target[0] - v.eye[0], v.target[1] - v.eye[1], v.target[2] - v.eye[2]};
        const float zn = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
        float x[3] = {z[2], 0.f, -z[0]};  // (0, 1, 0) x z
        const float xn = std::sqrt(x[0] * x[0] + x[2] * x[2]);
        if (!(zn > 0.f) || !(xn > 1e-6f * zn)) throw std::runtime_error("--3d-vis-eye / --3d-vis-target: no usable direction");
        for (int k = 0; k < 3; ++k) {
            z[k] /= zn;
            x[k] /= xn;
        }
        const float y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
        R = emf::Matx33f(x[0], y[0], z[0], x[1], y[1], z[1], x[2], y[2], z[2]);
    }
    emf.set3dView(emf::Affine3f(R, emf::Vec3f(v.eye[0], v.eye[1], v.eye[2])), K, size);
}

// The reference's main loop on a dataset (apps/EM-Fusion.cpp:100-156): a TUM sequence (`--sequence`, TUMRGBDReader) or a
// Co-Fusion style directory (`--dir`, ImageReader: ColorNNNN.png + DepthNNNN.exr), as apps/EM-Fusion.cpp:118-131 chooses
static bool weldMeshes = false;  // --weld-meshes
static bool worldMeshOut = false;  // --world-mesh: OUT/world.ply, one mesh of the background and its stored tiles
// --distance-field [--distance-cap M] [--distance-unknown-obstacle] (needs --out): writeResults also writes
// OUT/distance.bin (f32 metres to the nearest occupied -- or occupied or unknown -- voxel of the background, objects
// stamped in, +inf beyond M metres) and OUT/occupancy.bin (u8 classes); without it no output byte changes
static bool distanceOut = false, distanceUnknownObstacle = false;
// --distance-nearest (needs --distance-field): also OUT/nearest.bin, i32 in the container of distance.bin: the linear
// index of the nearest obstacle voxel of the background, -1 where distance.bin holds +inf.
static bool distanceNearest = false;
static float distanceCap = 0.f;
// --frontiers [--frontier-min-voxels N] [--frontier-clearance M] (needs --out): writeResults also writes
// OUT/frontiers.txt, one line per cluster of frontier voxels (free next to unknown) of the background of at least N
// (default 8) voxels, largest first; M metres of clearance from the nearest occupied voxel.
static bool frontiersOut = false;
static int frontierMinVoxels = 8;
static float frontierClearance = 0.f;
// --plan [--plan-clearance M] [--plan-through-unknown] (needs --out): writeResults also writes OUT/plan.txt, the plan
// from the voxel under the last camera position to the representative of every kept frontier cluster of the
// background (--frontier-min-voxels), M metres clear of the nearest occupied voxel.
static bool planOut = false, planThroughUnknown = false;
static float planClearance = 0.f;
// --plan-shortcut W (needs --plan): plan.txt also carries one "waypoints" line per reachable goal (EMFusion::shortcutPlan)
static int planShortcut = 0;
// --object-shapes (needs --out): writeResults also writes OUT/shapes.txt, one line per live object in id order: the
// integer moments of its observed solid band (not its body), then its box in the world frame;
// without it no output byte changes
static bool objectShapesOut = false;
// --object-contacts (needs --out): writeResults also writes OUT/contacts.txt, one line per ordered pair (probe object,
// field object or background) with a sampled surface voxel: the ids, the eight counts, min_s and the world contact point
// and normal; --contact-touch M: the touching threshold in metres (default: one voxel of the probe);
// without --object-contacts no output byte changes
static bool objectContactsOut = false, contactTouchGiven = false;
// --absorb-objects (needs --out): an object that the clean-up deletes because it left view is first absorbed into the
// background volume (the band of its signed-distance volume, not the free space around it), and
// writeResults also writes OUT/absorbed.txt, one line per absorbed object; without it no output byte changes.  Objects
// are deleted only where the clean-up runs: on a dataset, with --autonomous, or from the frame of --turn-away on; on the
// plain synthetic stream the switch would do nothing and is refused.
static bool absorbObjects = false;
// --lift-objects (needs --out): an object created from a mask is seeded with the band the background already holds inside
// its cube, and the background releases what the object then holds as foreground; writeResults also
// writes OUT/lifted.txt, one line per lifted object; without it no output byte changes.  Objects are created from masks
// on a dataset and with --autonomous; on the synthetic stream with given poses the switch would do nothing and is refused.
static bool liftObjects = false;
// --merge-objects [--merge-overlap F] [--merge-max-res N] (needs --out): duplicate objects -- one physical thing with two
// volumes -- are merged at the end of every mask frame, the older object stays; writeResults also writes
// OUT/merged.txt, one line per merge; without it no output byte changes.  Valid where objects are created from masks, as
// --lift-objects is.  F (default 0.5) and N (default 256) are policy values.
static bool mergeObjects = false, mergeParamGiven = false;
static emf::EMFusion::MergeParams mergeParams;
// --turn-away F (synthetic stream with given poses, not --autonomous): from frame F on the camera pose handed in looks
// the other way (half a turn about its y axis) and the clean-up runs, so every object leaves view and is deleted at F
static int turnAway = -1;
static double contactTouch = -1.0;
// --ground-map (needs --out): writeResults also writes OUT/ground.bin and OUT/ground.txt, the 2-D traversability map of
// the whole background with a floor height per cell; --ground-up X,Y,Z (world frame; default: minus the
// background's y axis), --ground-cell / --ground-bin M (default: two voxels), --ground-band LO,HI (metres relative to
// the camera along up), --ground-robot-height M, --ground-max-step M; without --ground-map no output byte changes
// --ground-up floor: up is the normal of the floor the plane search of DESIGN.md 5.25 finds in the whole background; the
// run ends with a message where it finds none
static emf::EMFusion::GroundOutput groundOut;
static bool groundGiven = false, groundBad = false, groundUpFloor = false;
// --planes (needs --out): writeResults also writes OUT/planes.txt, one line per dominant plane of the whole background
// ordered by count: kind count, the world normal, d, a point, the thickness in metres and the bounds in voxels
// (DESIGN.md 5.25); --planes-angle DEG (the alignment gate, default 20), --planes-min-votes N (default: max(50, records /
// 200)); without --planes no output byte changes
static emf::EMFusion::PlanesOutput planesOut;
static bool planesGiven = false;
// --plane-patches (needs --planes): planes.txt also lists every plane's connected patches and, with --object-shapes, which
// patch each object rests on; --plane-patch-reach R (1 or 2, default 1), --plane-patch-min N (default:
// max(25, min votes / 4)); without --plane-patches no output byte changes
static emf::EMFusion::PlanePatchesOutput patchesOut;
static bool patchesGiven = false;
// "a,b[,c]" into n doubles; false if it does not hold n numbers
static bool parseList(const char* text, double* out, int n) {
    char* end = nullptr;
    for (int i = 0; i < n; ++i) {
        out[i] = std::strtod(text, &end);
        if (end == text || (i + 1 < n && *end != ',')) return false;
        text = end + 1;
    }
    return *end == 0;
}
static bool planShortcutGiven = false;
// --motion-masks [--motion-band M] [--motion-min-pixels N] [--motion-max-masks N]: mask frames propose their own
// instance masks from the depth in front of the background model (EMFusion::setMotionMasks) instead of reading them
static bool motionMasks = false;
static emf::MotionMaskParams motionParams;
// --follow-camera [--follow-step X,Y,Z] [--follow-lookahead M]: the background is rolled by whole voxels after the camera
// (EMFusion::setBackgroundFollow); what leaves is meshed and written as OUT/bg_retired/.  A rolled
// session's checkpoint carries the switch and its parameters.
static bool followCamera = false;
static emf::BackgroundFollowParams followParams;
// --world-mesh (needs --out): writeResults also writes OUT/world.ply, ONE mesh of the current background and of the tiles
// the background store holds, without duplicates or seams; without it no output byte changes
// --follow-store [--follow-store-mib N]: what rolls out is kept on the host and put back when the camera returns
// (EMFusion::setBackgroundStore); N: the budget in MiB, 1024 by default -- a cap, not a measurement.
// Needs --follow-camera.
static bool followStore = false;
static long followStoreMib = 1024;
static bool followStoreMibGiven = false;
// --world-queries: the scene queries of writeResults cover the background AND the stored tiles
// (EMFusion::setQueryExtent).  Needs --follow-camera --follow-store.
static bool worldQueries = false;
static unsigned meshMinTriangles = 0;    // --mesh-min-triangles
static bool meshLargestObject = false;   // --mesh-largest-object
static float meshSimplifyCell = 0.f;     // --mesh-simplify
// --checkpoint PATH --checkpoint-every N: the session is saved to PATH after every N-th frame (EMFusion::saveCheckpoint);
// --resume PATH: the instance is built from the file's parameters, the file is loaded and the input stream continues at
// the stored frame index.  What the caller sets at start (output log, views, weld) is set again, as at start.
static std::string checkpointPath, resumePath;
static int checkpointEvery = 0;
static void maybeCheckpoint(emf::EMFusion& emf, size_t f) {
    if (checkpointPath.empty() || checkpointEvery <= 0 || (f + 1) % static_cast<size_t>(checkpointEvery) != 0) return;
    const emf::CheckpointStats st = emf.saveCheckpoint(checkpointPath);
    std::printf("checkpoint after frame %zu: %.1f MiB of volumes in a file of %.1f MiB, %.1f ms\n", f,
                st.rawBytes / 1048576.0, st.fileBytes / 1048576.0, st.msTotal);
}

static int runSequence(const std::string& seq, bool cofusion, const std::string& colordir, const std::string& depthdir,
                       const float* intrinsics, const std::string& configFile, const std::string& masks,
                       const std::string& outDir, int frames, int bgRes, float bgVoxel, int objRes, int maskFrames,
                       int visibilityThresh, bool volumes, const View3d& view3d, bool frameMeshes, bool color) {
    std::unique_ptr<emf::TUMRGBDReader> tum;
    std::unique_ptr<emf::ImageReader> dir;
    size_t available = 0;
    if (cofusion) {
        dir.reset(new emf::ImageReader(seq, colordir, depthdir));  // "<base><colordir>", "<base><depthdir>"
        available = dir->getNumFrames();
    } else {
        tum.reset(new emf::TUMRGBDReader(seq));  // "<dir>/associations.txt"
        available = tum->getNumFrames();
    }
    if (available == 0) throw std::runtime_error("no frames in " + seq);
    const size_t n = frames > 0 ? std::min<size_t>(frames, available) : available;
    std::vector<float> depth;
    auto readDepth = [&](size_t f) {
        return cofusion ? dir->readDepth(dir->firstIndex() + static_cast<int>(f), depth) : tum->readDepth(f, depth);
    };
    const emf::Size size = readDepth(0);
    emf::Params params;  // reference defaults (config/default.cfg)
    const bool configured = !configFile.empty();
    if (configured) {
        // --configfile: everything comes from the reference's configuration file (apps/EM-Fusion.cpp:268-371) and, for
        // --dir, from <base>calibration.txt (:399-410); the sizing options of this command line are not applied
        emf::loadConfigFile(params, configFile);
        if (cofusion) emf::loadCalibrationFile(params, seq + "calibration.txt");
        if (params.frameSize.width != size.width || params.frameSize.height != size.height)
            throw std::runtime_error("the configuration says " + std::to_string(params.frameSize.width) + " x " +
                                     std::to_string(params.frameSize.height) + ", the images are " + std::to_string(size.width) +
                                     " x " + std::to_string(size.height));
    } else {
        params.frameSize = size;
        params.setDefaultIntrinsics();
    }
    if (intrinsics) {  // the reference takes them from its config file (data.h: intr)
        params.intr = emf::Matx33f::eye();
        params.intr(0, 0) = intrinsics[0];
        params.intr(1, 1) = intrinsics[1];
        params.intr(0, 2) = intrinsics[2];
        params.intr(1, 2) = intrinsics[3];
    }
    if (!configured) {
        params.globalVolumeDims = emf::Vec3i::all(bgRes);
        params.globalVoxelSize = bgVoxel;
        params.volumePose = emf::Affine3f(emf::Matx33f::eye(), emf::Vec3f(0.f, 0.f, bgRes * bgVoxel / 2.f));
        params.objVolumeDims = emf::Vec3i::all(objRes);
        const float scale = static_cast<float>(size.width) / 640.f;
        params.visibilityThresh = visibilityThresh > 0 ? visibilityThresh : static_cast<int>(std::lround(1600 * scale * scale));
        params.boundary = static_cast<int>(std::lround(20 * scale));
        params.maskRCNNFrames = maskFrames;
    }
    if (!resumePath.empty()) params = emf::EMFusion::checkpointParams(resumePath);
    if (!resumePath.empty() && (params.frameSize.width != size.width || params.frameSize.height != size.height))
        throw std::runtime_error("--resume: the checkpoint was saved with another frame size than the images have");
    emf::EMFusion emf(params);
    if (!resumePath.empty()) emf.loadCheckpoint(resumePath);  // (restores colour on / off itself)
    else if (color) emf.enableColor(true);            // --color: the sequence's colour images go into the models
    color = emf.colorEnabled();
    emf.setMeshWeld(weldMeshes);
    emf.setMeshFilter(meshMinTriangles, meshLargestObject);
    emf.setMeshSimplify(meshSimplifyCell);
    if (motionMasks) emf.setMotionMasks(true, motionParams);  // (not stored in a checkpoint: set again on --resume)
    if (followCamera) emf.setBackgroundFollow(true, followParams);
    if (followStore) emf.setBackgroundStore(true, static_cast<uint64_t>(followStoreMib) << 20);
    if (worldQueries) emf.setQueryExtent(true);
    std::vector<uint8_t> rgb;
    if (!masks.empty()) emf.usePreprocMasks(masks);   // apps/EM-Fusion.cpp:115
    emf.setupOutput(frameMeshes, volumes);            // apps/EM-Fusion.cpp:112
    emf.setWorldMeshOutput(worldMeshOut);
    emf.setDistanceOutput(distanceOut, distanceCap, distanceUnknownObstacle);
    emf.setDistanceNearestOutput(distanceNearest);
    emf.setFrontierOutput(frontiersOut, frontierMinVoxels, frontierClearance);
    emf.setPlanOutput(planOut, planClearance, planThroughUnknown);
    if (planShortcut > 0) emf.setPlanShortcutOutput(planShortcut);
    if (objectShapesOut) emf.setShapeOutput(true);
    if (objectContactsOut) emf.setContactsOutput(true, contactTouch);
    if (absorbObjects) emf.setAbsorbObjects(true), emf.setAbsorbedOutput(true);  // (not stored in a checkpoint: set again on --resume)
    if (liftObjects) emf.setLiftObjects(true), emf.setLiftedOutput(true);          // (nor is this)
    if (mergeObjects) emf.setMergeObjects(true, mergeParams), emf.setMergedOutput(true);  // (nor this)
    if (groundOut.on) emf.setGroundOutput(groundOut);
    if (groundUpFloor) emf.setGroundUpFloor(true);
    if (planesOut.on) emf.setPlanesOutput(planesOut);
    if (patchesOut.on) emf.setPlanePatchesOutput(patchesOut);
    set3dView(emf, params, view3d);
    std::vector<uint8_t> rendered(3 * params.frameSize.area());
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t f = static_cast<size_t>(emf.frameIndex()); f < n; ++f) {  // while (reader->moreFrames())
        readDepth(f);                                 // frame = reader->getNextFrame()
        for (float& d : depth)
            if (!std::isfinite(d)) d = 0.f;
        emf::FrameInputs in;                          // frame 0 defines the world frame; then everything is tracked
        in.trackCamera = in.trackObjects = f > 0;
        in.cleanUp = true;
        emf.setFrameInputs(in);
        emf::RGBD frame;
        frame.size = size;
        frame.depth = depth.data();
        if (color) {
            const emf::Size cs = cofusion ? dir->readColor(dir->firstIndex() + static_cast<int>(f), rgb) : tum->readColor(f, rgb);
            if (cs.width != size.width || cs.height != size.height)
                throw std::runtime_error("frame " + std::to_string(f) + ": the colour image is " + std::to_string(cs.width) +
                                         " x " + std::to_string(cs.height) + ", the depth image " +
                                         std::to_string(size.width) + " x " + std::to_string(size.height));
            frame.rgb = rgb.data();
        }
        emf.processFrame(frame);                      // apps/EM-Fusion.cpp:152
        if (view3d.on) emf.render(rendered.data());   // apps/EM-Fusion.cpp:156: the rendering and the 3D view
        if (f % 50 == 0) {
            std::vector<uint8_t> maskim;
            const int inst = emf.getLastMasks(maskim);  // apps/EM-Fusion.cpp:162
            std::printf("frame %zu/%zu: %zu visible objects, %d instances in the last mask frame\n", f, n,
                        emf.visibleObjects().size(), inst);
        }
        maybeCheckpoint(emf, f);
    }
    emf.synchronize();
    emf.writeResults(outDir, volumes);                // apps/EM-Fusion.cpp:204
    std::printf("%zu frames of %s (%.1f Hz) in %.1f s incl. image decoding on the host; results in %s\n", n, seq.c_str(),
                cofusion ? 30.0 : tum->getFrameRate(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                outDir.c_str());
    return 0;
}

int main(int argc, char** argv) {
    int frames = 120, objects = 4, bgRes = 512, objRes = 128, width = 640, height = 480;
    bool materialize = false, autonomous = false;
    std::string outDir, sequence, maskDir, dataDir, colordir = "colour", depthdir = "depth", configFile;
    float intrinsics[4] = {0.f, 0.f, 0.f, 0.f};
    bool haveIntrinsics = false;
    int maskFrames = 30, visThresh = 0, framesGiven = 0;
    bool maskFramesGiven = false;
    float bgVoxel = 0.f;
    bool volumes = false;
    View3d view3d;
    bool frameMeshes = false, color = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() { return i + 1 < argc ? std::atoi(argv[++i]) : 0; };
        if (a == "--frames") frames = framesGiven = next();
        else if (a == "--sequence" && i + 1 < argc) sequence = argv[++i];
        else if (a == "--masks" && i + 1 < argc) maskDir = argv[++i];
        else if (a == "--dir" && i + 1 < argc) dataDir = argv[++i];
        else if ((a == "--configfile" || a == "-c") && i + 1 < argc) configFile = argv[++i];
        else if (a == "--colordir" && i + 1 < argc) colordir = argv[++i];
        else if (a == "--depthdir" && i + 1 < argc) depthdir = argv[++i];
        else if (a == "--intrinsics" && i + 4 < argc) {
            for (int k = 0; k < 4; ++k) intrinsics[k] = static_cast<float>(std::atof(argv[++i]));
            haveIntrinsics = true;
        }
        else if (a == "--mask-frames") {
            maskFrames = next();
            maskFramesGiven = true;
        }
        else if (a == "--motion-masks") motionMasks = true;
        else if (a == "--follow-camera") followCamera = true;
        else if (a == "--follow-step" && i + 1 < argc) {
            int x = 0, y = 0, z = 0;
            if (std::sscanf(argv[++i], "%d,%d,%d", &x, &y, &z) != 3) {
                std::fprintf(stderr, "usage: emfusion_synth: --follow-step X,Y,Z (voxels, positive multiples of 32,8,8)\n");
                return 2;
            }
            followParams.step = emf::Vec3i(x, y, z);
        }
        else if (a == "--follow-store") followStore = true;
        else if (a == "--world-queries") worldQueries = true;
        else if (a == "--follow-store-mib" && i + 1 < argc) {
            followStoreMib = std::atol(argv[++i]);
            followStoreMibGiven = true;
        }
        else if (a == "--follow-lookahead" && i + 1 < argc) followParams.lookAhead = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--motion-band" && i + 1 < argc) motionParams.band = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--motion-min-pixels") motionParams.minPixels = next();
        else if (a == "--motion-max-masks") motionParams.maxMasks = next();
        else if (a == "--visibility-thresh") visThresh = next();
        else if (a == "--bg-voxel" && i + 1 < argc) bgVoxel = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--volumes") volumes = true;
        else if (a == "--objects") objects = next();
        else if (a == "--bg-res") bgRes = next();
        else if (a == "--obj-res") objRes = next();
        else if (a == "--width") width = next();
        else if (a == "--height") height = next();
        else if (a == "--materialize-gradients") materialize = true;
        else if (a == "--autonomous") autonomous = true;
        else if (a == "--out" && i + 1 < argc) outDir = argv[++i];
        else if (a == "--3d-vis") view3d.on = true;
        else if (a == "--export-frame-meshes") frameMeshes = true;
        else if (a == "--weld-meshes") weldMeshes = true;
        else if (a == "--world-mesh") worldMeshOut = true;
        else if (a == "--distance-field") distanceOut = true;
        else if (a == "--distance-cap" && i + 1 < argc) distanceCap = std::max(static_cast<float>(std::atof(argv[++i])), 0.f);
        else if (a == "--distance-unknown-obstacle") distanceUnknownObstacle = true;
        else if (a == "--distance-nearest") distanceNearest = true;
        else if (a == "--object-shapes") objectShapesOut = true;
        else if (a == "--object-contacts") objectContactsOut = true;
        else if (a == "--absorb-objects") absorbObjects = true;
        else if (a == "--lift-objects") liftObjects = true;
        else if (a == "--merge-objects") mergeObjects = true;
        else if (a == "--merge-overlap" && i + 1 < argc) mergeParamGiven = true, mergeParams.minOverlap = std::atof(argv[++i]);
        else if (a == "--merge-max-res" && i + 1 < argc) mergeParamGiven = true, mergeParams.maxRes = std::atoi(argv[++i]);
        else if (a == "--turn-away" && i + 1 < argc) turnAway = std::atoi(argv[++i]);
        else if (a == "--contact-touch" && i + 1 < argc) contactTouchGiven = true, contactTouch = std::atof(argv[++i]);
        else if (a == "--ground-map") groundOut.on = true;
        else if (a == "--ground-up" && i + 1 < argc && std::string(argv[i + 1]) == "floor") groundGiven = true, groundUpFloor = true, ++i;
        else if (a == "--ground-up" && i + 1 < argc) groundGiven = true, groundBad |= !parseList(argv[++i], groundOut.up, 3);
        else if (a == "--planes") planesOut.on = true;
        else if (a == "--planes-angle" && i + 1 < argc) planesGiven = true, planesOut.angle = std::atof(argv[++i]);
        else if (a == "--planes-min-votes" && i + 1 < argc) planesGiven = true, planesOut.minVotes = std::atoll(argv[++i]);
        else if (a == "--plane-patches") patchesOut.on = true;
        else if (a == "--plane-patch-reach" && i + 1 < argc) patchesGiven = true, patchesOut.reach = std::atoi(argv[++i]);
        else if (a == "--plane-patch-min" && i + 1 < argc) patchesGiven = true, patchesOut.minCount = std::atoll(argv[++i]);
        else if (a == "--ground-band" && i + 1 < argc) {
            double band[2] = {0.0, 0.0};
            groundGiven = true, groundBad |= !parseList(argv[++i], band, 2);
            groundOut.bandLo = band[0], groundOut.bandHi = band[1];
        }
        else if (a == "--ground-cell" && i + 1 < argc) groundGiven = true, groundOut.cell = std::atof(argv[++i]);
        else if (a == "--ground-bin" && i + 1 < argc) groundGiven = true, groundOut.bin = std::atof(argv[++i]);
        else if (a == "--ground-robot-height" && i + 1 < argc) groundGiven = true, groundOut.robotHeight = std::atof(argv[++i]);
        else if (a == "--ground-max-step" && i + 1 < argc) groundGiven = true, groundOut.maxStep = std::atof(argv[++i]);
        else if (a == "--frontiers") frontiersOut = true;
        else if (a == "--frontier-min-voxels" && i + 1 < argc) frontierMinVoxels = std::max(std::atoi(argv[++i]), 1);
        else if (a == "--frontier-clearance" && i + 1 < argc) frontierClearance = std::max(static_cast<float>(std::atof(argv[++i])), 0.f);
        else if (a == "--plan") planOut = true;
        else if (a == "--plan-clearance" && i + 1 < argc) planClearance = std::max(static_cast<float>(std::atof(argv[++i])), 0.f);
        else if (a == "--plan-through-unknown") planThroughUnknown = true;
        else if (a == "--plan-shortcut" && i + 1 < argc) {
            planShortcut = std::atoi(argv[++i]);
            planShortcutGiven = true;
        }
        else if (a == "--mesh-min-triangles") meshMinTriangles = static_cast<unsigned>(std::max(next(), 0));
        else if (a == "--mesh-largest-object") meshLargestObject = true;
        else if (a == "--mesh-simplify" && i + 1 < argc) meshSimplifyCell = static_cast<float>(std::atof(argv[++i]));
        else if (a == "--color") color = true;
        else if (a == "--checkpoint" && i + 1 < argc) checkpointPath = argv[++i];
        else if (a == "--checkpoint-every") checkpointEvery = next();
        else if (a == "--resume" && i + 1 < argc) resumePath = argv[++i];
        else if ((a == "--3d-vis-eye" || a == "--3d-vis-target") && i + 3 < argc) {
            float* dst = a == "--3d-vis-eye" ? view3d.eye : view3d.target;
            for (int k = 0; k < 3; ++k) dst[k] = static_cast<float>(std::atof(argv[++i]));
            view3d.placed = true;
        }
        else {
            std::fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }
    if ((followStore && !followCamera) || (followStoreMibGiven && !followStore) || followStoreMib < 1) {  // (before any device is touched)
        std::fprintf(stderr, "usage: emfusion_synth: --follow-store needs --follow-camera, and --follow-store-mib N (>= 1) needs "
                             "--follow-store\n");
        return 2;
    }
    if (worldQueries && !(followCamera && followStore)) {  // (before any device is touched)
        std::fprintf(stderr, "usage: emfusion_synth: --world-queries needs --follow-camera --follow-store\n");
        return 2;
    }
    if (distanceNearest && !distanceOut) {  // (before any device is touched)
        std::fprintf(stderr, "usage: emfusion_synth: --distance-nearest writes nearest.bin beside distance.bin and needs --distance-field\n");
        return 2;
    }
    if (planShortcutGiven && (!planOut || planShortcut < 1)) {  // (before any device is touched)
        std::fprintf(stderr, "usage: emfusion_synth: --plan-shortcut W (>= 1) adds the waypoints lines to plan.txt and needs --plan\n");
        return 2;
    }
    if ((groundGiven && !groundOut.on) || groundBad || (groundOut.on && outDir.empty())) {  // (before any device is touched)
        std::fprintf(stderr, "usage: emfusion_synth: --ground-up X,Y,Z or floor, --ground-band LO,HI, --ground-cell, --ground-bin, "
                             "--ground-robot-height and --ground-max-step need --ground-map, which writes ground.bin and "
                             "ground.txt and needs --out DIR\n");
        return 2;
    }
    if ((planesGiven && !planesOut.on) || (planesOut.on && (outDir.empty() || !(planesOut.angle > 0.0 && planesOut.angle <= 90.0)))) {
        std::fprintf(stderr, "usage: emfusion_synth: --planes-angle DEG (in (0, 90]) and --planes-min-votes N need --planes, which "
                             "writes planes.txt and needs --out DIR\n");
        return 2;
    }
    if ((patchesGiven && !patchesOut.on) || (patchesOut.on && (!planesOut.on || patchesOut.reach < 1 || patchesOut.reach > EMF_PLANE_MAX_REACH))) {
        std::fprintf(stderr, "usage: emfusion_synth: --plane-patch-reach R (1 or 2) and --plane-patch-min N need --plane-patches, which "
                             "adds the patch lines to planes.txt and needs --planes\n");
        return 2;
    }
    if (absorbObjects && outDir.empty()) {
        std::fprintf(stderr, "usage: emfusion_synth: --absorb-objects writes absorbed.txt and needs --out DIR\n");
        return 2;
    }
    if (mergeParamGiven && !mergeObjects) {
        std::fprintf(stderr, "usage: emfusion_synth: --merge-overlap F and --merge-max-res N are parameters of --merge-objects\n");
        return 2;
    }
    if (mergeObjects && outDir.empty()) {
        std::fprintf(stderr, "usage: emfusion_synth: --merge-objects writes merged.txt and needs --out DIR\n");
        return 2;
    }
    if (mergeObjects && sequence.empty() && dataDir.empty() && !autonomous) {
        std::fprintf(stderr, "usage: emfusion_synth: --merge-objects acts where objects are created from masks: with --sequence / "
                             "--dir or --autonomous; on the synthetic stream with given poses it would do nothing\n");
        return 2;
    }
    if (liftObjects && outDir.empty()) {
        std::fprintf(stderr, "usage: emfusion_synth: --lift-objects writes lifted.txt and needs --out DIR\n");
        return 2;
    }
    if (liftObjects && sequence.empty() && dataDir.empty() && !autonomous) {
        std::fprintf(stderr, "usage: emfusion_synth: --lift-objects acts where objects are created from masks: with --sequence / "
                             "--dir or --autonomous; on the synthetic stream with given poses it would do nothing\n");
        return 2;
    }
    if (turnAway != -1 && (turnAway < 1 || autonomous || !sequence.empty() || !dataDir.empty())) {
        std::fprintf(stderr, "usage: emfusion_synth: --turn-away F (>= 1) turns the camera pose handed to the synthetic stream; "
                             "it excludes --autonomous, --sequence and --dir, where the pose is tracked\n");
        return 2;
    }
    if (absorbObjects && sequence.empty() && dataDir.empty() && !autonomous && turnAway < 0) {
        std::fprintf(stderr, "usage: emfusion_synth: --absorb-objects acts where the clean-up deletes objects: with --sequence / "
                             "--dir, --autonomous or --turn-away F; on the plain synthetic stream it would do nothing\n");
        return 2;
    }
    if ((contactTouchGiven && (!objectContactsOut || !(contactTouch >= 0.0))) || (objectContactsOut && outDir.empty())) {
        std::fprintf(stderr, "usage: emfusion_synth: --contact-touch M (>= 0, metres) needs --object-contacts, which writes "
                             "contacts.txt and needs --out DIR\n");
        return 2;
    }
    if (motionMasks && !maskDir.empty()) {  // (before any device is touched)
        std::fprintf(stderr, "usage: emfusion_synth: --motion-masks and --masks DIR exclude each other: a mask frame takes its "
                             "instance masks from the files or proposes them itself\n");
        return 2;
    }
    if (view3d.placed && !view3d.on) {
        std::fprintf(stderr, "emfusion_synth: --3d-vis-eye / --3d-vis-target need --3d-vis\n");
        return 2;
    }
    if (frameMeshes && outDir.empty()) {  // (before any device is touched)
        std::fprintf(stderr, "emfusion_synth: --export-frame-meshes writes DIR/frame_meshes/ and needs --out DIR\n");
        return 2;
    }
    if (color && sequence.empty() && dataDir.empty()) {  // (before any device is touched)
        std::fprintf(stderr, "emfusion_synth: --color needs the colour images of --sequence or --dir; the synthetic stream has none\n");
        return 2;
    }
    if (checkpointPath.empty() != (checkpointEvery <= 0)) {
        std::fprintf(stderr, "emfusion_synth: --checkpoint PATH and --checkpoint-every N (> 0) go together\n");
        return 2;
    }
    if (view3d.on && outDir.empty()) {
        std::fprintf(stderr, "emfusion_synth: --3d-vis writes DIR/mesh_vis_out/ and needs --out DIR\n");
        return 2;
    }
    try {
        if (!sequence.empty() || !dataDir.empty()) {
            if (outDir.empty()) throw std::runtime_error("--sequence / --dir need --out DIR");
            const bool cofusion = !dataDir.empty();
            return runSequence(cofusion ? dataDir : sequence, cofusion, colordir, depthdir, haveIntrinsics ? intrinsics : nullptr,
                               configFile, maskDir, outDir, framesGiven, bgRes, bgVoxel > 0 ? bgVoxel : 5.12f / static_cast<float>(bgRes),
                               objRes, maskFrames, visThresh, volumes, view3d, frameMeshes, color);
        }
        emf::Params params;  // reference defaults (config/default.cfg)
        params.frameSize = emf::Size(width, height);
        params.setDefaultIntrinsics();
        params.globalVolumeDims = emf::Vec3i::all(bgRes);
        params.globalVoxelSize = 5.12f / static_cast<float>(bgRes);
        params.objVolumeDims = emf::Vec3i::all(objRes);
        const float scale = static_cast<float>(width) / 640.f;
        params.visibilityThresh = static_cast<int>(1600 * scale * scale);
        params.boundary = static_cast<int>(20 * scale);

        if (motionMasks && maskFramesGiven && maskFrames > 0) params.maskRCNNFrames = maskFrames;

        if (!resumePath.empty()) params = emf::EMFusion::checkpointParams(resumePath, &materialize);
        emf::SyntheticScene scene(params.frameSize, params.intr, objects);
        // --autonomous --motion-masks: an object that is there from the first frame and hardly moves is fused into the
        // background and never proposed, so the spheres ENTER the scene: the first frames show the empty room
        const int motionEnter = 5;
        emf::SyntheticScene emptyRoom(params.frameSize, params.intr, 0);
        emf::EMFusion emf(params, materialize ? emf::TSDF::Gradients::Materialized
                                              : emf::TSDF::Gradients::OnTheFly);
        std::vector<int> ids;
        if (!resumePath.empty()) {
            emf.loadCheckpoint(resumePath);
            if (!autonomous) {
                ids = emf.objectIds();
                if (static_cast<int>(ids.size()) != objects)
                    throw std::runtime_error("--resume: the checkpoint holds " + std::to_string(ids.size()) +
                                             " objects, --objects says " + std::to_string(objects));
            }
        } else if (!autonomous)
            for (int k = 0; k < objects; ++k)
                ids.push_back(emf.addObject(scene.sphereCenter(k, 0), scene.objectVolumeSize(k)));
        const int firstFrame = emf.frameIndex();

        const size_t P = params.frameSize.area();
        std::vector<float> depth(P);
        std::vector<uint8_t> sid(P), mask(P);
        std::vector<emf::DeviceImage<uint8_t>> maskDev;
        for (int k = 0; k < objects; ++k) maskDev.emplace_back(params.frameSize);
        emf.enableTimings(true);
        emf.setMeshWeld(weldMeshes);
        emf.setMeshFilter(meshMinTriangles, meshLargestObject);
        emf.setMeshSimplify(meshSimplifyCell);
        if (motionMasks) emf.setMotionMasks(true, motionParams);
        if (followCamera) emf.setBackgroundFollow(true, followParams);
        if (followStore) emf.setBackgroundStore(true, static_cast<uint64_t>(followStoreMib) << 20);
        if (worldQueries) emf.setQueryExtent(true);
        if (!outDir.empty()) emf.setupOutput(frameMeshes, true);  // apps/EM-Fusion.cpp:112
        emf.setWorldMeshOutput(worldMeshOut);
        emf.setDistanceOutput(distanceOut, distanceCap, distanceUnknownObstacle);
        emf.setDistanceNearestOutput(distanceNearest);
        emf.setFrontierOutput(frontiersOut, frontierMinVoxels, frontierClearance);
        emf.setPlanOutput(planOut, planClearance, planThroughUnknown);
        if (planShortcut > 0) emf.setPlanShortcutOutput(planShortcut);
        if (objectShapesOut) emf.setShapeOutput(true);
        if (objectContactsOut) emf.setContactsOutput(true, contactTouch);
        if (absorbObjects) emf.setAbsorbObjects(true), emf.setAbsorbedOutput(true);
        if (liftObjects) emf.setLiftObjects(true), emf.setLiftedOutput(true);
        if (mergeObjects) emf.setMergeObjects(true, mergeParams), emf.setMergedOutput(true);
        if (groundOut.on) emf.setGroundOutput(groundOut);
        if (groundUpFloor) emf.setGroundUpFloor(true);
        if (planesOut.on) emf.setPlanesOutput(planesOut);
    if (patchesOut.on) emf.setPlanePatchesOutput(patchesOut);
        set3dView(emf, params, view3d);
        std::vector<uint8_t> rendered(3 * P);

        double gpuMs = 0;
        int spawned = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int f = firstFrame; f < frames; ++f) {  // while (reader->moreFrames())
            if (autonomous && motionMasks && f < motionEnter) emptyRoom.render(f, depth.data(), sid.data());
            else scene.render(f, depth.data(), sid.data());  // frame = reader->getNextFrame()
            emf::FrameInputs in;
            in.cam_pose = scene.cameraPose(f);
            in.runMasks = f % params.maskRCNNFrames == 0;
            if (in.runMasks && !(autonomous && motionMasks))
                for (int k = 0; k < objects; ++k) {
                    for (size_t i = 0; i < P; ++i) mask[i] = sid[i] == k + 1 ? 1 : 0;
                    maskDev[k].upload(mask.data(), emf.mainStream());
                    emf.mainStream().waitForCompletion();  // host buffer is reused
                }
            if (!autonomous) {
                const bool turned = turnAway >= 0 && f >= turnAway;
                if (turned) {  // x and z of the camera's frame flip: it looks the other way; no masks of what it cannot see
                    in.cam_pose = emf::Affine3f(in.cam_pose.rotation() * emf::Matx33f(-1, 0, 0, 0, 1, 0, 0, 0, -1),
                                                in.cam_pose.translation());
                    in.runMasks = false;
                    in.cleanUp = true;
                }
                for (int k = 0; k < objects; ++k)
                    if (emf.getObject(ids[k])) in.obj_poses[ids[k]] = emf::Affine3f(emf::Matx33f::eye(), scene.sphereCenter(k, f));
                if (in.runMasks)
                    for (int k = 0; k < objects; ++k)
                        if (emf.getObject(ids[k])) in.masks[ids[k]] = maskDev[k].view();
            } else {
                in.trackCamera = in.trackObjects = f > 0;
                in.cleanUp = true;
                // a "Mask R-CNN frame": all instance masks go through initOrMatchObjs inside the
                // frame (match / spawn / existence bookkeeping), then integrateMasks, cleanUpObjs
                // (--motion-masks: no masks go in; a mask frame stays one and proposes its own)
                if (in.runMasks && !motionMasks)
                    for (int k = 0; k < objects; ++k) in.instanceMasks.push_back(maskDev[k].view());
                if (!motionMasks) in.runMasks = false;
            }
            emf.setFrameInputs(in);
            emf::RGBD frame;
            frame.size = params.frameSize;
            frame.depth = depth.data();
            emf.processFrame(frame);  // reference EMFusion.cpp:70
            gpuMs += emf.lastTimings().total;
            if (view3d.on) emf.render(rendered.data());  // apps/EM-Fusion.cpp:156: the rendering and the 3D view
            if (autonomous)
                for (int id : emf.lastCreatedObjects()) spawned += id >= 0;
            maybeCheckpoint(emf, static_cast<size_t>(f));
        }
        emf.synchronize();
        if (autonomous) {
            const emf::Vec3f d = emf.getCameraPose().translation() - scene.cameraPose(frames - 1).translation();
            std::printf("autonomous: %d objects spawned from %s; camera position error after %d "
                        "tracked frames: %.1f mm",
                        spawned, motionMasks ? "motion masks" : "masks", frames - 1,
                        1e3 * std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
            if (const emf::TrackResult* r = emf.getTrackResult(0))
                std::printf(" (last frame: %d LM steps, %d accepted)", r->iterations, r->accepted);
            std::printf("\n");
        }
        const double wall =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const emf::FrameTimings& t = emf.lastTimings();
        std::printf("%d frames, %d objects, bg %d^3, obj %d^3, %dx%d: %.1f frames/s of GPU time "
                    "(%.3f ms/frame), %.1f frames/s wall incl. host rendering of the stream\n",
                    frames, objects, bgRes, objRes, width, height, 1e3 * frames / gpuMs,
                    gpuMs / frames, frames / wall);
        std::printf("last frame [ms]: points %.3f  estep(x3) %.3f  raycast %.3f  composite %.3f  "
                    "integrate %.3f  masks %.3f | visible objects %zu | batched launches: %s\n",
                    t.points, t.estep, t.raycast, t.composite, t.integrate, t.masks,
                    emf.visibleObjects().size(), emf.usesBatchedLaunches() ? "yes" : "no");
        if (absorbObjects) std::printf("absorbed into the background: %zu objects\n", emf.absorbed().size());
        if (liftObjects) std::printf("lifted out of the background: %zu objects\n", emf.lifted().size());
        if (mergeObjects) std::printf("merged into other objects: %zu objects\n", emf.merged().size());
        if (!outDir.empty()) {
            emf.writeResults(outDir, false);  // volumes follow setupOutput, as in the reference
            const emf::Mesh bg = emf.getMesh(0);
            std::printf("results in %s: background mesh %zu vertices, %zu triangles\n", outDir.c_str(),
                        bg.vertices(), bg.triangles());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "emfusion_synth: %s\n", e.what());
        return 1;
    }
    return 0;
}
