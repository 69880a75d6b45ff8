// EMFusionLifecycle.cpp -- emf::EMFusion: objects from masks (reference src/core/EMFusion.cpp:329-557, 797-863, 891-989).
#include "EMFusion.hpp"
#include "EMFusionDetail.hpp"
#include "Readers.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

namespace emf {

using namespace detail;

namespace {
// the reference's instance colours (MaskRCNN.cpp:290-301), index 0 = no instance
const unsigned char colors[31][3] = {
    {0, 0, 0},       {0, 0, 255},     {255, 0, 0},    {0, 255, 0},     {255, 26, 184},  {255, 211, 0},   {0, 131, 246},
    {0, 140, 70},    {167, 96, 61},   {79, 0, 105},   {0, 255, 246},   {61, 123, 140},  {237, 167, 255}, {211, 255, 149},
    {184, 79, 255},  {228, 26, 87},   {131, 131, 0},  {0, 255, 149},   {96, 0, 43},     {246, 131, 17},  {202, 255, 0},
    {43, 61, 0},     {0, 52, 193},    {255, 202, 131}, {0, 43, 96},    {158, 114, 140}, {79, 184, 17},   {158, 193, 255},
    {149, 158, 123}, {255, 123, 175}, {158, 8, 0}};
}  // namespace

// runMaskRCNN with a mask path (reference EMFusion.cpp:383-389) + the label image getLastMasks hands out
void EMFusion::loadPreprocMasks(FrameInputs& in) {
    char name[32];
    std::snprintf(name, sizeof(name), "Mask%04d.plk", frameCount);
    PreprocMasks pm;
    int n = 0;
    {
        std::ifstream probe(maskPath + "/" + name, std::ios::binary);
        if (probe.good()) n = loadPreprocessedMasks(maskPath + "/" + name, pm);
    }
    const int w = params.frameSize.width, h = params.frameSize.height;
    if (n > 0 && (pm.width != w || pm.height != h))
        throw HipError(std::string("EMFusion::usePreprocMasks: ") + name + " holds masks of another size than the frames",
                       EMF_E_SHAPE);
    main.waitForCompletion();  // the previous mask frame's device copies are being replaced
    preprocMaskDev.clear();
    in.instanceMasks.clear();
    in.instanceScores.clear();
    lastMaskVis.assign(static_cast<size_t>(w) * h * 3, 0);
    lastMaskInstances = n;
    motionVisStale = false;
    for (int k = 0; k < n; ++k) {
        preprocMaskDev.emplace_back(params.frameSize);
        preprocMaskDev.back().upload(pm.masks[k].data(), main);
        const unsigned char* c = colors[1 + k % 30];
        for (size_t i = 0; i < pm.masks[k].size(); ++i)
            if (pm.masks[k][i]) {
                lastMaskVis[3 * i] = c[0];
                lastMaskVis[3 * i + 1] = c[1];
                lastMaskVis[3 * i + 2] = c[2];
            }
    }
    main.waitForCompletion();  // (pm's host buffers go out of scope)
    for (auto& m : preprocMaskDev) in.instanceMasks.push_back(m.view());
    in.instanceScores = pm.scores;
}

// ---- motion masks: instance proposals from the frame's points and the background's raycast -------------

void EMFusion::setMotionMasks(bool on, const MotionMaskParams& p) {
    if (!on) {
        motionOn = false;
        return;
    }
    // the background's ray lengths are band-local until the composite's exchange there, and the life cycle's
    // exchanges assume masks that every rank was handed
    if (sharded) throw HipError("EMFusion::setMotionMasks: motion masks are not supported on the sharded path", EMF_E_ARG);
    if (p.erode < 0 || p.erode > 3) throw HipError("EMFusion::setMotionMasks: erode must be 0 .. 3", EMF_E_ARG);
    if (p.maxMasks < 1 || p.maxMasks > EMF_MOTION_MAX_MASKS)
        throw HipError("EMFusion::setMotionMasks: maxMasks must be 1 .. " + std::to_string(EMF_MOTION_MAX_MASKS), EMF_E_ARG);
    if (p.minPixels < 0) throw HipError("EMFusion::setMotionMasks: minPixels must not be negative", EMF_E_ARG);
    if (!(p.continuity >= 0.f)) throw HipError("EMFusion::setMotionMasks: continuity must not be negative", EMF_E_ARG);
    if (p.band != p.band) throw HipError("EMFusion::setMotionMasks: band is not a number", EMF_E_ARG);
    // by default the margin below which the TSDF itself does not tell "in front of the surface" from the surface
    motionParams.band = p.band < 0.f ? params.globalRelTruncDist * params.globalVoxelSize : p.band;
    motionParams.continuity = p.continuity;
    motionParams.erode = p.erode;
    motionParams.min_pixels = p.minPixels;
    motionParams.max_masks = p.maxMasks;
    motionOn = true;
}

void EMFusion::ensureMotionBuffers() {
    if (!motionScratch.empty()) return;
    const int w = params.frameSize.width, h = params.frameSize.height;
    const size_t bytes = emf_hip_motionMasksScratchBytes(w, h, EMF_MOTION_MAX_MASKS);
    if (bytes == 0) throw HipError("EMFusion::setMotionMasks: the frame size is beyond the motion masks' limits", EMF_E_LIMIT);
    motionScratch = DeviceBuffer(bytes);
    motionPlanes = DeviceBuffer(params.frameSize.area() * EMF_MOTION_MAX_MASKS);
    motionInfoDev = DeviceBuffer(EMF_MOTION_MAX_MASKS * sizeof(emf_motion_info_t) + 16);
    motionLabels = DeviceImage<int32_t>(params.frameSize);
    motionHost = PinnedBuffer(motionInfoDev.bytes());
}

// The hook of runSchedule: the proposals of this frame become its instance masks.  Everything on `main`, behind the
// raycast that wrote bg_raylengths (on the per-volume path the volume streams were joined into `main`) and the launch
// that made the points; the count and the info records come back in one small copy, the only wait.
void EMFusion::proposeMotionMasks(std::vector<emf_image_t>& segs) {
    ensureMotionBuffers();
    const int w = params.frameSize.width, h = params.frameSize.height;
    emf_motion_info_t* infoDev = motionInfoDev.as<emf_motion_info_t>();
    int32_t* countDev = reinterpret_cast<int32_t*>(infoDev + EMF_MOTION_MAX_MASKS);
    emfCheck(emf_hip_motionMasks(points.ptr(), bg_raylengths.ptr(), w, h, &motionParams, motionScratch.data(),
                                 motionLabels.ptr(), motionPlanes.as<uint8_t>(), infoDev, countDev, main.abi()),
             "motionMasks");
    const size_t used = motionParams.max_masks * sizeof(emf_motion_info_t);
    hipCheck(hipMemcpyAsync(motionHost.data(), infoDev, used, hipMemcpyDeviceToHost, main.get()), "hipMemcpyAsync");
    hipCheck(hipMemcpyAsync(motionHost.as<char>() + used, countDev, sizeof(int32_t), hipMemcpyDeviceToHost, main.get()),
             "hipMemcpyAsync");
    main.waitForCompletion();
    int32_t count = 0;
    std::memcpy(&count, motionHost.as<char>() + used, sizeof(count));
    count = std::max(0, std::min(count, motionParams.max_masks));
    const emf_motion_info_t* info = motionHost.as<const emf_motion_info_t>();
    motionInfo.assign(info, info + count);
    motionFired = true;
    lastMaskInstances = count;  // getLastMasks draws them when somebody asks
    motionVisStale = true;
    const size_t plane = params.frameSize.area();
    for (int r = 0; r < count; ++r)
        segs.push_back(imageView(motionPlanes.as<uint8_t>() + plane * r, params.frameSize, 1));
}

const std::vector<emf_motion_info_t>& EMFusion::lastMotionMasks(std::vector<int32_t>* labels) {
    if (labels) {
        if (motionFired) *labels = motionLabels.download(main);
        else labels->assign(params.frameSize.area(), -1);
    }
    return motionInfo;
}

int EMFusion::getLastMasks(std::vector<uint8_t>& rgb) {
    if (motionVisStale) {  // the proposals of the last frame that looked for any, in instance colours by rank
        const std::vector<int32_t> lab = motionLabels.download(main);
        lastMaskVis.assign(lab.size() * 3, 0);
        for (size_t i = 0; i < lab.size(); ++i) {
            if (lab[i] < 0) continue;
            const unsigned char* c = colors[1 + lab[i] % 30];
            lastMaskVis[3 * i] = c[0];
            lastMaskVis[3 * i + 1] = c[1];
            lastMaskVis[3 * i + 2] = c[2];
        }
        motionVisStale = false;
    }
    rgb = lastMaskVis;
    return lastMaskInstances;
}

// ---- object creation / matching from masks ---------------------------------------------------------

void EMFusion::ensureLifecycleBuffers() {
    if (!statsScratch.empty()) return;
    statsScratch = DeviceBuffer(emf_hip_pointStatsScratchBytes());
    statsDev = DeviceBuffer(sizeof(emf_point_stats_t));
    overlapDev = DeviceBuffer(513 * sizeof(uint32_t));
    massDev = DeviceBuffer(EMF_MAX_MODELS * sizeof(emf_mask_mass_t));
    verdictDev = DeviceBuffer(EMF_MAX_MODELS * sizeof(float));
    lifecycleMsg = DeviceBuffer(4 * sizeof(float));
    static_assert(EMF_MAX_MODELS * sizeof(emf_mask_mass_t) >= 513 * sizeof(uint32_t), "the larger of the two uses");
    lifecycleHost = PinnedBuffer(kLcHostBytes);
}

emf_point_stats_t EMFusion::maskedStats(const emf_image_t& mask, const Affine3f& frame) {
    ensureLifecycleBuffers();
    const emf_image_t pv = points.view();
    emfCheck(emf_hip_maskedPointStats(&pv, &mask, frame.rotation().val, frame.translation().val,
                                      statsScratch.data(), statsDev.as<emf_point_stats_t>(),
                                      main.abi()),
             "maskedPointStats");
    hipCheck(hipMemcpyAsync(lifecycleHost.data(), statsDev.data(), sizeof(emf_point_stats_t),
                            hipMemcpyDeviceToHost, main.get()),
             "hipMemcpyAsync");
    main.waitForCompletion();
    return *lifecycleHost.as<emf_point_stats_t>();
}

float EMFusion::volumeIOU(const ObjTSDF& obj, const Vec3f& p10, const Vec3f& p90) const {
    const Vec3f center = (p10 + p90) / 2.f;
    const Vec3f dims = p90 - p10;
    const float volSize = params.volPad * std::max(dims[0], std::max(dims[1], dims[2]));
    const Vec3f hv(volSize / 2, volSize / 2, volSize / 2);
    const Vec3f low_new = center - hv, high_new = center + hv;
    Vec3f low, high;
    obj.getCorners(low, high);
    const Vec3f prev = obj.getVolumeSize();
    const float vol = 1.f * prev[0] * prev[1] * prev[2];
    // pow(float, int) of the reference promotes to double (C++11 [c.math]); the float keeps its rounding
    const float vol_new = static_cast<float>(std::pow(static_cast<double>(volSize), 3));
    float vol_int = 1.f;
    for (int k = 0; k < 3; ++k) {
        const float d = std::min(high[k], high_new[k]) - std::max(low[k], low_new[k]);
        if (d < 0) return 0.f;  // no overlap
        vol_int = vol_int * d;
    }
    return vol_int / (vol_new + vol - vol_int);
}

int EMFusion::initNewObjVolume(const emf_image_t& mask) {
    // world frame first: the count decides whether anything else is needed (EMFusion.cpp:501-503)
    const emf_point_stats_t world_stats = maskedStats(mask, pose);
    if (static_cast<int>(world_stats.count) < params.visibilityThresh) return -1;
    bool blocked = false;
    for (const auto& obj : objects) {  // EMFusion.cpp:508-524 (sharded: this rank's objects)
        const emf_point_stats_t s = maskedStats(mask, obj.getPose().inv() * pose);
        const float iou = volumeIOU(obj, Vec3f(s.p10[0], s.p10[1], s.p10[2]),
                                    Vec3f(s.p90[0], s.p90[1], s.p90[2]));
        if (iou > params.volIOUThresh) {
            blocked = true;
            break;
        }
    }
    if (sharded && !allIds.empty()) {
        // the owners' verdicts joined: ONE all-reduce of a 16-byte message (a flag and padding), issued by every rank
        // whatever its own objects said, so that every rank creates the object or none does
        lifecycleMsg.setZero(main);
        if (blocked) hipCheck(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lifecycleMsg.data()), 0x3f800000, 1, main.get()),
                              "hipMemsetD32Async");
        comm->allReduceSumF32(lifecycleMsg.as<float>(), 4, main);
        float* h = reinterpret_cast<float*>(lifecycleHost.as<char>() + kLcVerdictOff);
        hipCheck(hipMemcpyAsync(h, lifecycleMsg.data(), 4 * sizeof(float), hipMemcpyDeviceToHost, main.get()),
                 "hipMemcpyAsync");
        main.waitForCompletion();
        blocked = h[0] > 0.f;
    }
    if (blocked) return -1;
    const Vec3f p10(world_stats.p10[0], world_stats.p10[1], world_stats.p10[2]);
    const Vec3f p90(world_stats.p90[0], world_stats.p90[1], world_stats.p90[2]);
    const Vec3f center = (p10 + p90) / 2.f;
    const Vec3f off = center - pose.translation();
    // cv::norm accumulates the squares in double (EMFusion.cpp:531-533)
    const double o0 = off[0], o1 = off[1], o2 = off[2];
    if (std::sqrt(o0 * o0 + o1 * o1 + o2 * o2) > static_cast<double>(params.distanceThresh)) return -1;
    const Vec3f dims = p90 - p10;
    const float volSize = params.volPad * std::max(dims[0], std::max(dims[1], dims[2]));
    if (static_cast<int>(allIds.size()) >= EMF_MAX_MODELS - 1) {
        // every slot of the model table is live: this mask gets no volume (the frame loop goes on,
        // as the reference's would); addObject() itself keeps rejecting the explicit call
        std::fprintf(stderr, "EMFusion::initNewObjVolume: %d live objects, no new volume for this mask\n",
                     static_cast<int>(allIds.size()));
        return -1;
    }
    return addObject(center, volSize);  // every rank; the owner allocates
}

int EMFusion::matchSegmentation(const emf_image_t& mask, float& match_iou) {
    refreshVisibleFromDevice();
    ensureLifecycleBuffers();
    const emf_image_t seg = modelSegmentation.view();
    emfCheck(emf_hip_maskOverlap(&mask, &seg, overlapDev.as<uint32_t>(), main.abi()), "maskOverlap");
    hipCheck(hipMemcpyAsync(lifecycleHost.data(), overlapDev.data(), 513 * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, main.get()),
             "hipMemcpyAsync");
    main.waitForCompletion();
    const uint32_t* c = lifecycleHost.as<const uint32_t>();
    int match_id = -1;
    for (const int id : allIds) {  // (every rank: the joint segmentation and visible set cover all objects)
        if (!vis_objs.count(id) || id > 255) continue;
        const float inter = static_cast<float>(c[1 + id]);
        const float uni = static_cast<float>(c[0] + c[257 + id] - c[1 + id]);
        const float iou = inter / uni;  // 0 / 0 = NaN never exceeds match_iou, as in the reference
        if (iou > match_iou) {
            match_iou = iou;
            match_id = id;
        }
    }
    return match_iou > params.matchIOUThresh ? match_id : -1;
}

std::map<int, emf_image_t> EMFusion::initOrMatchObjs(std::vector<emf_image_t>& segs,
                                                     std::vector<int>& assigned,
                                                     const std::vector<std::vector<double>>& scores) {
    ensureLifecycleBuffers();
    std::map<int, emf_image_t> matches;
    std::vector<int> unmatched;
    assigned.assign(segs.size(), -1);
    const emf_image_t modelSeg = modelSegmentation.view();
    auto overlapCounts = [&](const emf_image_t& seg) -> const uint32_t* {
        emfCheck(emf_hip_maskOverlap(&seg, &modelSeg, overlapDev.as<uint32_t>(), main.abi()), "maskOverlap");
        hipCheck(hipMemcpyAsync(lifecycleHost.data(), overlapDev.data(), 513 * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, main.get()),
                 "hipMemcpyAsync");
        main.waitForCompletion();
        return lifecycleHost.as<const uint32_t>();
    };
    // ---- matchSegmentation over all masks (EMFusion.cpp:417-444) ----
    for (size_t i = 0; i < segs.size(); ++i) {
        int matched = -1;
        if (frameCount > 0) {
            float new_iou = 0.f;
            matched = matchSegmentation(segs[i], new_iou);
            if (matched >= 0 && matches.count(matched)) {
                // a second mask for the same model: the better one becomes the match; THIS mask goes
                // on as unmatched either way (EMFusion.cpp:424-437).  Quirk Q20: when it replaced the
                // earlier match it is carved below against the match of that model -- itself, the
                // reference's matches[id] being a shallow GpuMat copy of seg_gpus[i] -- so the model
                // ends up matched to an all-zero mask.  Reproduced: matches[] holds views of the same
                // device buffers.
                const uint32_t* c = overlapCounts(matches[matched]);
                const float prev_iou = static_cast<float>(c[1 + matched]) /
                                       static_cast<float>(c[0] + c[257 + matched] - c[1 + matched]);
                if (new_iou > prev_iou) {
                    for (size_t k = 0; k < i; ++k)
                        if (assigned[k] == matched) assigned[k] = -1;
                    matches[matched] = segs[i];
                    assigned[i] = matched;
                }
                matched = -1;
            }
        }
        if (matched >= 0) {
            matches[matched] = segs[i];
            assigned[i] = matched;
        } else {
            unmatched.push_back(static_cast<int>(i));
        }
    }
    // ---- initObjsFromUnmatched (EMFusion.cpp:446-494) ----
    // (the carving loops over the job's ids, objects created earlier in this loop included: the same on every rank)
    for (int i : unmatched) {
        for (const int id : allIds) {
            if (id > 255) continue;
            auto it = matches.find(id);
            emfCheck(emf_hip_carveMask(&segs[i], &modelSeg, id, it == matches.end() ? nullptr : &it->second,
                                       overlapDev.as<uint32_t>(), main.abi()),
                     "carveMask");
            hipCheck(hipMemcpyAsync(lifecycleHost.data(), overlapDev.data(), 2 * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost, main.get()),
                     "hipMemcpyAsync");
            main.waitForCompletion();
            const uint32_t* c = lifecycleHost.as<const uint32_t>();
            // more than half of the mask belonged to an existing object: no new volume from it
            if (static_cast<float>(c[1]) / static_cast<float>(c[0]) < .5f)
                hipCheck(hipMemset2DAsync(segs[i].data, segs[i].pitch, 0, static_cast<size_t>(segs[i].width),
                                          static_cast<size_t>(segs[i].height), main.get()),
                         "hipMemset2DAsync");
        }
        const int id = initNewObjVolume(segs[i]);
        lastCreated.push_back(id);
        matches.insert(std::make_pair(id, segs[i]));  // even id == -1 (EMFusion.cpp:491); callers drop that key
        if (assigned[i] < 0) assigned[i] = id;        // a replacing mask keeps scoring its model (score_matches)
    }
    bool resized = false;
    for (auto& obj : objects) {  // EMFusion.cpp:358-369 (sharded: the owner's part, no exchange)
        auto it = matches.find(obj.getID());
        if (it != matches.end()) {
            // score_matches (EMFusion.cpp:442, 492): the scores of the mask that ended up with this object
            for (size_t i = 0; i < assigned.size() && i < scores.size(); ++i)
                if (assigned[i] == obj.getID()) obj.updateClassProbs(scores[i]);
            const Vec3i before = obj.getVolumeRes();
            const Vec3f offset = updateObj(obj, it->second);
            if (poseLog) obj_pose_offsets[obj.getID()][frameCount] = offset;
            resized |= offset[0] != 0.f || offset[1] != 0.f || offset[2] != 0.f ||
                       before[0] != obj.getVolumeRes()[0];
        }
        obj.updateExProb(it != matches.end());
    }
    if (resized) rebuildModelTable();  // new buffers, new resolution, new pose
    return matches;
}

// Reference EMFusion::updateObj (EMFusion.cpp:827-863) without the class scores: percentiles of the
// object's surface (the vertex cloud of its mesh) united with the newly matched points, in the
// object's frame, decide whether the volume has to grow or move (ObjTSDF::resize).  No mesh is
// built: emf_hip_objectExtentStats streams the marching-cubes vertices into the selection.
Vec3f EMFusion::updateObj(ObjTSDF& obj, const emf_image_t& mask) {
    ensureLifecycleBuffers();
    if (maskedStats(mask, pose).count == 0) return Vec3f::all(0.f);  // no valid point under the mask
    const Affine3f frame = obj.getPose().inv() * pose;
    const emf_image_t pv = points.view();
    const Vec3i res = obj.getVolumeRes();
    emfCheck(emf_hip_objectExtentStats(&pv, &mask, frame.rotation().val, frame.translation().val,
                                       obj.tsdfPtr(), obj.weightsPtr(), obj.fgVolMaskPtr(), res.val,
                                       obj.getVoxelSize(), statsScratch.data(),
                                       statsDev.as<emf_point_stats_t>(), main.abi()),
             "objectExtentStats");
    hipCheck(hipMemcpyAsync(lifecycleHost.data(), statsDev.data(), sizeof(emf_point_stats_t),
                            hipMemcpyDeviceToHost, main.get()),
             "hipMemcpyAsync");
    main.waitForCompletion();
    const emf_point_stats_t s = *lifecycleHost.as<emf_point_stats_t>();
    const Vec3f offset = obj.resize(Vec3f(s.p10[0], s.p10[1], s.p10[2]),
                                    Vec3f(s.p90[0], s.p90[1], s.p90[2]), params.volPad, main);
    // the pose may have moved with the volume centre (EMFusion.cpp:858-860)
    if (poseLog) obj_poses[obj.getID()][frameCount] = obj.getPose();
    return offset;
}

Vec3f EMFusion::updateObject(int id, const emf_image_t& mask) {
    if (std::find(allIds.begin(), allIds.end(), id) == allIds.end())
        throw HipError("EMFusion::updateObject: no object " + std::to_string(id), EMF_E_ARG);
    Vec3f offset = Vec3f::all(0.f);
    if (ObjTSDF* obj = findObject(id)) {
        quiesce();
        refreshVisibleFromDevice();  // rebuildModelTable below uploads the gate from the host set
        offset = updateObj(*obj, mask);
        if (poseLog) {  // several calls between two frames add up
            Vec3f& logged = obj_pose_offsets[id][frameCount];
            logged = logged + offset;
        }
        rebuildModelTable();
    }
    if (sharded) {  // every rank returns the owner's shift: ONE 16-byte broadcast from the owner
        ensureLifecycleBuffers();
        float* h = reinterpret_cast<float*>(lifecycleHost.as<char>() + kLcVerdictOff);
        if (ownsObject(id)) {
            h[0] = offset[0];
            h[1] = offset[1];
            h[2] = offset[2];
            h[3] = 0.f;
            hipCheck(hipMemcpyAsync(lifecycleMsg.data(), h, 4 * sizeof(float), hipMemcpyHostToDevice, main.get()),
                     "hipMemcpyAsync");
        }
        comm->broadcast(lifecycleMsg.data(), 4 * sizeof(float), ownerOf(id, world), main);
        hipCheck(hipMemcpyAsync(h, lifecycleMsg.data(), 4 * sizeof(float), hipMemcpyDeviceToHost, main.get()),
                 "hipMemcpyAsync");
        main.waitForCompletion();
        offset = Vec3f(h[0], h[1], h[2]);
    }
    return offset;
}

void EMFusion::deleteObj(int id) {  // reference EMFusion.cpp:982-989
    // the slot of a deleted object is free again: EMF_MAX_MODELS bounds the LIVE models, not the
    // number ever created (a long run spawns and cleans up spurious objects all the time)
    allIds.erase(std::remove(allIds.begin(), allIds.end(), id), allIds.end());
    streams.erase(id);
    objImages.erase(id);
    vis_objs.erase(id);
    trackResults.erase(id);
}

// The deletion of an object of this rank (EMFusion.cpp:951-976); the caller rebuilds the table afterwards.
void EMFusion::deleteOwned(std::list<ObjTSDF>::iterator it, bool absorb, bool keep) {
    const int id = it->getID();
    quiesce();  // nothing in flight may still use the volume
    // gone from view with setAbsorbObjects on: its band goes into the background first
    if (absorb && !(ignorePerson && isPerson(*it))) absorbInto(*it);
    deleteObj(id);
    if (keep && poseLog && !(ignorePerson && isPerson(*it))) {
        meshes[id] = it->getMesh();  // saveOutput: EMFusion.cpp:962-966
        if (expVols) savedVolumes[id] = saveVolumes(*it);  // EMFusion.cpp:967-973
    }
    objects.erase(it);
}

std::vector<int> EMFusion::cleanUpObjs(bool maskFrame, const std::map<int, emf_image_t>& matches) {
    ensureLifecycleBuffers();
    // The association masses of EVERY object of this rank in two launches over the model table (slots 1 .. n), before
    // the host waits for anything: ONE synchronisation per frame then yields both the visible set (it decides whose
    // mass counts, EMFusion.cpp:936) and the masses (rounds 3-5: a wait for the visible set, then a launch, a copy and
    // a wait per visible object; until the batched entry: two launches per object).
    const int nobj = static_cast<int>(objects.size());
    const int nall = static_cast<int>(allIds.size());
    const int w = params.frameSize.width, h = params.frameSize.height;
    std::vector<emf_image_t> matchImgs(static_cast<size_t>(nobj), emf_image_t{});
    std::vector<uint8_t> exLow(static_cast<size_t>(nobj), 0);
    std::vector<int32_t> listPos(static_cast<size_t>(nobj), 0);
    int k = 0;
    for (const auto& obj : objects) {
        auto it = matches.find(obj.getID());
        if (it != matches.end()) matchImgs[k] = it->second;
        exLow[k] = maskFrame && obj.getExProb() < params.existenceThresh;  // (owner-only fact, mask frames)
        listPos[k] = static_cast<int32_t>(std::find(allIds.begin(), allIds.end(), obj.getID()) - allIds.begin());
        ++k;
    }
    const size_t scratchBytes = emf_hip_maskAssociationMassScratchBytes(nobj);
    if (massScratch.bytes() < scratchBytes) massScratch = DeviceBuffer(scratchBytes);
    std::vector<int> deleted;
    if (!sharded) {
        if (nobj) {
            emfCheck(emf_hip_maskAssociationMassBatched(currentTable(), 1, nobj, w, h, matchImgs.data(), massScratch.data(),
                                                        massDev.as<emf_mask_mass_t>(), nullptr, 0, nullptr, nullptr,
                                                        nullptr, 0.f, main.abi()),
                     "maskAssociationMassBatched");
            hipCheck(hipMemcpyAsync(lifecycleHost.data(), massDev.data(), nobj * sizeof(emf_mask_mass_t), hipMemcpyDeviceToHost,
                                    main.get()),
                     "hipMemcpyAsync(mask masses)");
        }
        main.waitForCompletion();
        refreshVisibleFromDevice();  // the host copy of vis_objs decides (the stream is idle: no further wait)
        const emf_mask_mass_t* const massHost = lifecycleHost.as<const emf_mask_mass_t>();
        std::set<int> spurious;
        k = 0;
        for (const auto& obj : objects) {
            const emf_mask_mass_t mm = massHost[k];
            if (exLow[k] || (vis_objs.count(obj.getID()) && params.assocThresh * static_cast<float>(mm.count) > mm.sum))
                spurious.insert(obj.getID());
            ++k;
        }
        for (auto it = objects.begin(); it != objects.end();) {
            const int id = it->getID();
            if (spurious.count(id) || !vis_objs.count(id)) {
                deleted.push_back(id);
                deleteOwned(it++, absorbOn_ && !spurious.count(id));  // absorbed: deleted because it is not visible, only
            } else {
                ++it;
            }
        }
        absorbFinish();  // once, after the last deletion and before the table is rebuilt
        if (!deleted.empty()) rebuildModelTable();
        return deleted;
    }
    // Sharded: the owners' verdicts by list position, joined by ONE all-reduce -- issued whenever the job has objects,
    // also by a rank that owns none -- one copy back and one wait; every rank then deletes the same ids in list order.
    if (nall == 0) return deleted;
    if (!batched) {
        // the per-volume composite decides visibility on the host and leaves the device gate alone: make it current
        int32_t* gate = reinterpret_cast<int32_t*>(lifecycleHost.as<char>() + kLcGateOff);
        gate[0] = 1;
        k = 1;
        for (const auto& obj : objects) gate[k++] = vis_objs.count(obj.getID()) ? 1 : 0;
        hipCheck(hipMemcpyAsync(visibleDev.data(), gate, (nobj + 1) * sizeof(int32_t), hipMemcpyHostToDevice, main.get()),
                 "hipMemcpyAsync(gate)");
    }
    const int nslots = (nall + 3) / 4 * 4;
    emfCheck(emf_hip_maskAssociationMassBatched(currentTable(), 1, nobj, w, h, matchImgs.data(), massScratch.data(),
                                                massDev.as<emf_mask_mass_t>(), verdictDev.as<float>(), nall,
                                                listPos.data(), visibleDev.as<int32_t>(), exLow.data(),
                                                params.assocThresh, main.abi()),
             "maskAssociationMassBatched");
    comm->allReduceSumF32(verdictDev.as<float>(), static_cast<size_t>(nslots), main);
    float* verdict = reinterpret_cast<float*>(lifecycleHost.as<char>() + kLcVerdictOff);
    hipCheck(hipMemcpyAsync(verdict, verdictDev.data(), nall * sizeof(float), hipMemcpyDeviceToHost, main.get()),
             "hipMemcpyAsync(verdicts)");
    main.waitForCompletion();
    refreshVisibleFromDevice();
    const std::vector<int> ids = allIds;
    for (int p = 0; p < nall; ++p) {
        if (!(verdict[p] > 0.f)) continue;
        const int id = ids[p];
        deleted.push_back(id);
        auto it = std::find_if(objects.begin(), objects.end(), [&](const ObjTSDF& o) { return o.getID() == id; });
        if (it != objects.end()) deleteOwned(it);
        else deleteObj(id);
    }
    if (!deleted.empty()) rebuildModelTable();
    return deleted;
}

void EMFusion::integrateMasks(const std::map<int, emf_image_t>& matches) {
    const emf_image_t segv = modelSegmentation.view();
    const emf_image_t occv = occludedMask.view();
    for (auto& obj : objects) {
        auto it = matches.find(obj.getID());
        if (it == matches.end()) continue;
        // pixels where this object's own raycast hit but another model is in front are not
        // used for the foreground statistics (reference EMFusion.cpp:897-900)
        const emf_image_t objSeg = objImages.at(obj.getID()).modelSegmentation.view();
        emfCheck(emf_hip_occludedMask(&objSeg, &segv, obj.getID(), &occv, main.abi()),
                 "occludedMask");
        auto kt = ktimers.scope(KernelTimers::FgBg, static_cast<double>(obj.voxels()), main);
        obj.integrateMask(it->second, occv, pose, params.intr, main);
    }
}

}  // namespace emf
