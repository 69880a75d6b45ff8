// capi.cpp -- extern "C" handle API of include/emf_fusion.h over the C++ host classes.
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>

#include "EMFusion.hpp"
#include "Config.hpp"
#include "Readers.hpp"
#include "Output.hpp"
#include "SyntheticScene.hpp"
#include "emf_fusion.h"

using namespace emf;

struct emf_comm {
    std::shared_ptr<Communicator> impl;
};
struct emf_fusion {
    std::unique_ptr<EMFusion> impl;
    bool trackCamera = false, trackObjects = false, preprocess = false, cleanUp = false;
    std::vector<emf_image_t> queuedMasks, queuedInstances;
    std::vector<std::vector<double>> queuedScores;
    emf::Mesh mesh;  // result of the last emf_fusion_extract_mesh
    emf::MeshComponents components;  // result of the last emf_fusion_mesh_components
    std::vector<emf::Mesh> meshList;  // result of the last emf_fusion_extract_meshes
};
struct emf_synth {
    std::unique_ptr<SyntheticScene> impl;
};

namespace {

thread_local char g_err[512] = {0};

int report(const std::exception& e) {
    std::snprintf(g_err, sizeof(g_err), "%s", e.what());
    if (const auto* he = dynamic_cast<const HipError*>(&e)) return he->code() ? he->code() : -100;
    return -100;
}

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return EMF_OK;
    } catch (const std::exception& e) {
        return report(e);
    } catch (...) {
        std::snprintf(g_err, sizeof(g_err), "unknown exception");
        return -100;
    }
}

int nullArg(const char* fn, const char* what) {
    std::snprintf(g_err, sizeof(g_err), "%s: %s is NULL", fn, what);
    return EMF_E_NULL;
}

#define REQ(p)                                  \
    do {                                        \
        if (!(p)) return nullArg(__func__, #p); \
    } while (0)

Matx33f m33(const float* a) {
    return Matx33f(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
}

}  // namespace

extern "C" {

const char* emf_fusion_last_error_string(void) { return g_err; }

void emf_fusion_default_params(emf_fusion_params_t* p) {
    if (!p) return;
    const Params d;
    p->width = d.frameSize.width;
    p->height = d.frameSize.height;
    std::memcpy(p->K, d.intr.val, sizeof(p->K));
    std::memcpy(p->bg_res, d.globalVolumeDims.val, sizeof(p->bg_res));
    p->bg_voxel_size = d.globalVoxelSize;
    p->bg_rel_truncdist = d.globalRelTruncDist;
    std::memcpy(p->volume_pose_t, d.volumePose.translation().val, sizeof(p->volume_pose_t));
    std::memcpy(p->obj_res, d.objVolumeDims.val, sizeof(p->obj_res));
    p->obj_rel_truncdist = d.objRelTruncDist;
    p->max_tsdf_weight = d.tsdfParams.maxTSDFWeight;
    p->assoc_sigma = d.tsdfParams.assocSigma;
    p->alpha = d.tsdfParams.alpha;
    p->uni_prior = d.tsdfParams.uniPrior;
    p->visibility_thresh = d.visibilityThresh;
    p->boundary = d.boundary;
    p->mask_frames = d.maskRCNNFrames;
    p->materialize_gradients = 0;
    p->max_tracking_iter = d.maxTrackingIter;
}

int emf_fusion_create(const emf_fusion_params_t* p, emf_comm_t* comm, emf_fusion_t** out) {
    REQ(p);
    REQ(out);
    return guarded([&] {
        Params q;
        q.frameSize = Size(p->width, p->height);
        q.intr = m33(p->K);
        q.globalVolumeDims = Vec3i(p->bg_res[0], p->bg_res[1], p->bg_res[2]);
        q.globalVoxelSize = p->bg_voxel_size;
        q.globalRelTruncDist = p->bg_rel_truncdist;
        q.volumePose = Affine3f().translate(
            Vec3f(p->volume_pose_t[0], p->volume_pose_t[1], p->volume_pose_t[2]));
        q.objVolumeDims = Vec3i(p->obj_res[0], p->obj_res[1], p->obj_res[2]);
        q.objRelTruncDist = p->obj_rel_truncdist;
        q.tsdfParams.maxTSDFWeight = p->max_tsdf_weight;
        q.tsdfParams.assocSigma = p->assoc_sigma;
        q.tsdfParams.alpha = p->alpha;
        q.tsdfParams.uniPrior = p->uni_prior;
        q.visibilityThresh = p->visibility_thresh;
        q.boundary = p->boundary;
        q.maskRCNNFrames = p->mask_frames;
        if (p->max_tracking_iter > 0) q.maxTrackingIter = p->max_tracking_iter;
        auto h = std::make_unique<emf_fusion>();
        h->impl = std::make_unique<EMFusion>(
            q, p->materialize_gradients ? TSDF::Gradients::Materialized : TSDF::Gradients::OnTheFly,
            comm ? comm->impl : nullptr);
        *out = h.release();
    });
}

int emf_fusion_create_from_config(const char* path, const char* calibration, int materialize_gradients, emf_comm_t* comm,
                                  emf_fusion_params_t* params_out, emf_fusion_t** out) {
    REQ(out);
    return guarded([&] {
        // every field of the reference's Params, as apps/emfusion_synth --configfile builds them (apps/EM-Fusion.cpp:268-371):
        // emf_fusion_params_t carries a subset only (no ignore_person, LM / Huber / bilateral / lifecycle thresholds)
        Params q;
        if (path && path[0]) loadConfigFile(q, path);
        if (calibration && calibration[0]) loadCalibrationFile(q, calibration);
        auto h = std::make_unique<emf_fusion>();
        h->impl = std::make_unique<EMFusion>(q, materialize_gradients ? TSDF::Gradients::Materialized : TSDF::Gradients::OnTheFly,
                                             comm ? comm->impl : nullptr);
        if (params_out) {
            const int rc = emf_io_load_config(path, calibration, params_out, nullptr, 0);
            if (rc != 0) throw HipError("create_from_config: the configuration could not be re-read", rc);
            params_out->materialize_gradients = materialize_gradients;
        }
        *out = h.release();
    });
}

void emf_fusion_destroy(emf_fusion_t* h) { delete h; }

int emf_fusion_trim_pool(uint64_t* bytes_freed) {
    return guarded([&] {
        if (bytes_freed) *bytes_freed = emf::DeviceBuffer::pooledBytes();
        emf::DeviceBuffer::trimPool();
    });
}

int emf_fusion_describe_switches(char* json, size_t capacity) {
    REQ(json);
    return guarded([&] {
        const std::string s = emf::describeSwitches();
        if (s.size() + 1 > capacity) throw HipError("emf_fusion_describe_switches: buffer too small", EMF_E_ARG);
        std::memcpy(json, s.c_str(), s.size() + 1);
    });
}

int emf_fusion_save_checkpoint(emf_fusion_t* h, const char* path, emf_checkpoint_stats_t* stats) {
    REQ(h);
    REQ(path);
    return guarded([&] {
        const CheckpointStats st = h->impl->saveCheckpoint(path);
        if (!stats) return;
        *stats = emf_checkpoint_stats_t{};
        stats->raw_bytes = st.rawBytes;
        stats->file_bytes = st.fileBytes;
        for (int k = 0; k < 3; ++k) stats->chunks[k] = st.chunks[k];
        stats->ms_classify = st.msClassify;
        stats->ms_gather = st.msGather;
        stats->ms_copy = st.msCopy;
        stats->ms_file = st.msFile;
        stats->ms_total = st.msTotal;
        stats->records = st.records;
    });
}

int emf_fusion_load_checkpoint(emf_fusion_t* h, const char* path) {
    REQ(h);
    REQ(path);
    return guarded([&] {
        h->impl->loadCheckpoint(path);
        h->queuedMasks.clear();
        h->queuedInstances.clear();
        h->queuedScores.clear();
    });
}

int emf_fusion_checkpoint_info(const char* path, char* json, size_t capacity) {
    REQ(path);
    REQ(json);
    return guarded([&] {
        const std::string s = EMFusion::checkpointInfo(path);
        if (s.size() + 1 > capacity) throw HipError("emf_fusion_checkpoint_info: buffer too small", EMF_E_ARG);
        std::memcpy(json, s.c_str(), s.size() + 1);
    });
}

int emf_fusion_create_from_checkpoint(const char* path, emf_comm_t* comm, emf_fusion_params_t* params_out,
                                      emf_fusion_t** out) {
    REQ(path);
    REQ(out);
    return guarded([&] {
        bool materialized = false;
        const Params q = EMFusion::checkpointParams(path, &materialized);
        auto h = std::make_unique<emf_fusion>();
        h->impl = std::make_unique<EMFusion>(q, materialized ? TSDF::Gradients::Materialized : TSDF::Gradients::OnTheFly,
                                             comm ? comm->impl : nullptr);
        h->impl->loadCheckpoint(path);
        if (params_out) {
            emf_fusion_params_t* p = params_out;
            p->width = q.frameSize.width;
            p->height = q.frameSize.height;
            std::memcpy(p->K, q.intr.val, sizeof(p->K));
            std::memcpy(p->bg_res, q.globalVolumeDims.val, sizeof(p->bg_res));
            p->bg_voxel_size = q.globalVoxelSize;
            p->bg_rel_truncdist = q.globalRelTruncDist;
            std::memcpy(p->volume_pose_t, q.volumePose.translation().val, sizeof(p->volume_pose_t));
            std::memcpy(p->obj_res, q.objVolumeDims.val, sizeof(p->obj_res));
            p->obj_rel_truncdist = q.objRelTruncDist;
            p->max_tsdf_weight = q.tsdfParams.maxTSDFWeight;
            p->assoc_sigma = q.tsdfParams.assocSigma;
            p->alpha = q.tsdfParams.alpha;
            p->uni_prior = q.tsdfParams.uniPrior;
            p->visibility_thresh = q.visibilityThresh;
            p->boundary = q.boundary;
            p->mask_frames = q.maskRCNNFrames;
            p->materialize_gradients = materialized ? 1 : 0;
            p->max_tracking_iter = q.maxTrackingIter;
        }
        *out = h.release();
    });
}

int emf_fusion_reset(emf_fusion_t* h) {
    REQ(h);
    return guarded([&] { h->impl->reset(); });
}

int emf_fusion_add_object(emf_fusion_t* h, const float center[3], float vol_size,
                          int32_t* id_out) {
    REQ(h);
    REQ(center);
    return guarded([&] {
        const int id = h->impl->addObject(Vec3f(center[0], center[1], center[2]), vol_size);
        h->impl->settleReciprocals();  // an explicit call, outside any frame: the check ends here, not beside the first frames
        if (id_out) *id_out = id;
    });
}

int emf_fusion_process_frame(emf_fusion_t* h, const emf_image_t* depth_dev, const float cam_R[9],
                             const float cam_t[3], int nposes, const int32_t* pose_ids,
                             const float* obj_R, const float* obj_t, int nmasks,
                             const int32_t* mask_ids, const emf_image_t* masks, int run_masks) {
    REQ(h);
    REQ(depth_dev);
    REQ(cam_R);
    REQ(cam_t);
    if (nposes > 0) {
        REQ(pose_ids);
        REQ(obj_R);
        REQ(obj_t);
    }
    if (nmasks > 0) {
        REQ(mask_ids);
        REQ(masks);
    }
    return guarded([&] {
        FrameInputs in;
        in.cam_pose = Affine3f(m33(cam_R), Vec3f(cam_t[0], cam_t[1], cam_t[2]));
        for (int i = 0; i < nposes; ++i)
            in.obj_poses[pose_ids[i]] = Affine3f(
                m33(obj_R + 9 * i), Vec3f(obj_t[3 * i], obj_t[3 * i + 1], obj_t[3 * i + 2]));
        for (int i = 0; i < nmasks; ++i) in.masks[mask_ids[i]] = masks[i];
        in.runMasks = run_masks != 0;
        in.trackCamera = h->trackCamera;
        in.trackObjects = h->trackObjects;
        in.preprocessDepth = h->preprocess;
        in.cleanUp = h->cleanUp;
        in.newObjectMasks.swap(h->queuedMasks);
        in.instanceMasks.swap(h->queuedInstances);
        in.instanceScores.swap(h->queuedScores);
        h->impl->processFrame(*depth_dev, in);
    });
}

int emf_fusion_process_rgbd(emf_fusion_t* h, const float* depth_host, int32_t width, int32_t height) {
    REQ(h);
    REQ(depth_host);
    return guarded([&] {
        FrameInputs in;  // poses stay as tracked (or identity): the reference's entry takes nothing but the frame
        in.cam_pose = h->impl->getCameraPose();
        in.trackCamera = h->trackCamera;
        in.trackObjects = h->trackObjects;
        in.cleanUp = h->cleanUp;
        in.newObjectMasks.swap(h->queuedMasks);
        in.instanceMasks.swap(h->queuedInstances);
        in.instanceScores.swap(h->queuedScores);
        h->impl->setFrameInputs(in);
        RGBD frame;
        frame.size = Size(width, height);
        frame.depth = depth_host;
        h->impl->processFrame(frame);
    });
}

int emf_fusion_set_color(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->enableColor(on != 0); });
}

int emf_fusion_set_mesh_weld(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setMeshWeld(on != 0); });
}

int emf_fusion_set_mesh_filter(emf_fusion_t* h, uint32_t min_triangles, int largest_objects) {
    REQ(h);
    return guarded([&] { h->impl->setMeshFilter(min_triangles, largest_objects != 0); });
}

int emf_fusion_set_mesh_simplify(emf_fusion_t* h, float cell_metres) {
    REQ(h);
    return guarded([&] { h->impl->setMeshSimplify(cell_metres); });
}

int emf_fusion_last_mesh_simplify(emf_fusion_t* h, int32_t* ids, uint32_t* stats, int capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] {
        const auto& last = h->impl->lastMeshSimplify();
        *count = static_cast<int32_t>(last.size());
        int k = 0;
        for (const auto& kv : last) {
            if (k >= capacity) break;
            if (ids) ids[k] = kv.first;
            if (stats) {
                stats[5 * k] = kv.second.verticesIn;
                stats[5 * k + 1] = kv.second.trianglesIn;
                stats[5 * k + 2] = kv.second.verticesOut;
                stats[5 * k + 3] = kv.second.trianglesOut;
                stats[5 * k + 4] = kv.second.clusters;
            }
            ++k;
        }
    });
}

int emf_fusion_mesh_components(emf_fusion_t* h, int id, uint32_t* num_vertices) {
    REQ(h);
    REQ(num_vertices);
    return guarded([&] {
        h->components = h->impl->getMeshComponents(id);
        *num_vertices = static_cast<uint32_t>(h->components.labels.size());
    });
}

int emf_fusion_copy_mesh_components(emf_fusion_t* h, int32_t* labels, uint32_t* sizes) {
    REQ(h);
    return guarded([&] {
        if (labels) std::copy(h->components.labels.begin(), h->components.labels.end(), labels);
        if (sizes) std::copy(h->components.sizes.begin(), h->components.sizes.end(), sizes);
    });
}

int emf_fusion_last_mesh_filter(emf_fusion_t* h, int32_t* ids, uint32_t* stats, int capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] {
        const auto& last = h->impl->lastMeshFilter();
        *count = static_cast<int32_t>(last.size());
        int k = 0;
        for (const auto& kv : last) {
            if (k >= capacity) break;
            if (ids) ids[k] = kv.first;
            if (stats) {
                stats[4 * k] = kv.second.components;
                stats[4 * k + 1] = kv.second.keptComponents;
                stats[4 * k + 2] = kv.second.triangles;
                stats[4 * k + 3] = kv.second.keptTriangles;
            }
            ++k;
        }
    });
}

int emf_fusion_set_color_image(emf_fusion_t* h, const emf_image_t* rgb_dev) {
    REQ(h);
    REQ(rgb_dev);
    return guarded([&] { h->impl->setColorImage(*rgb_dev); });
}

int emf_fusion_process_rgbd_color(emf_fusion_t* h, const float* depth_host, const uint8_t* rgb_host, int32_t width,
                                  int32_t height) {
    REQ(h);
    REQ(depth_host);
    REQ(rgb_host);
    return guarded([&] {
        if (!h->impl->colorEnabled()) throw HipError("emf_fusion_process_rgbd_color: colour is not enabled", EMF_E_ARG);
        FrameInputs in;  // as emf_fusion_process_rgbd
        in.cam_pose = h->impl->getCameraPose();
        in.trackCamera = h->trackCamera;
        in.trackObjects = h->trackObjects;
        in.cleanUp = h->cleanUp;
        in.newObjectMasks.swap(h->queuedMasks);
        in.instanceMasks.swap(h->queuedInstances);
        in.instanceScores.swap(h->queuedScores);
        h->impl->setFrameInputs(in);
        RGBD frame;
        frame.size = Size(width, height);
        frame.depth = depth_host;
        frame.rgb = rgb_host;
        h->impl->processFrame(frame);
    });
}

int emf_fusion_colored_voxels(emf_fusion_t* h, uint64_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] { *count = h->impl->takeColoredVoxels(); });
}

int emf_fusion_use_preproc_masks(emf_fusion_t* h, const char* path) {
    REQ(h);
    REQ(path);
    return guarded([&] { h->impl->usePreprocMasks(path); });
}

int emf_fusion_get_last_masks(emf_fusion_t* h, uint8_t* rgb, size_t capacity, int32_t* instances) {
    REQ(h);
    return guarded([&] {
        std::vector<uint8_t> img;
        const int n = h->impl->getLastMasks(img);
        if (instances) *instances = n;
        if (rgb && capacity >= img.size() && !img.empty()) std::memcpy(rgb, img.data(), img.size());
    });
}

int emf_fusion_set_motion_masks(emf_fusion_t* h, int on, const emf_motion_params_t* params) {
    REQ(h);
    return guarded([&] {
        MotionMaskParams p;
        if (params) {
            p.band = params->band;
            p.continuity = params->continuity;
            p.erode = params->erode;
            p.minPixels = params->min_pixels;
            p.maxMasks = params->max_masks;
        }
        h->impl->setMotionMasks(on != 0, p);
    });
}

int emf_fusion_last_motion_masks(emf_fusion_t* h, int32_t* labels_out, emf_motion_info_t* info_out, int capacity,
                                 int32_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] {
        std::vector<int32_t> labels;
        const auto& info = h->impl->lastMotionMasks(labels_out ? &labels : nullptr);
        *count = static_cast<int32_t>(info.size());
        for (int i = 0; info_out && i < capacity && i < static_cast<int>(info.size()); ++i) info_out[i] = info[i];
        if (labels_out) std::copy(labels.begin(), labels.end(), labels_out);
    });
}

int emf_fusion_set_background_follow(emf_fusion_t* h, int on, const emf_follow_params_t* params) {
    REQ(h);
    return guarded([&] {
        BackgroundFollowParams p;
        if (params) {
            p.step = Vec3i(params->step[0], params->step[1], params->step[2]);
            p.lookAhead = params->look_ahead;
            p.keepRetired = params->keep_retired != 0;
        }
        h->impl->setBackgroundFollow(on != 0, p);
    });
}

int emf_fusion_roll_background(emf_fusion_t* h, const int32_t shift[3], int keep_retired) {
    REQ(h);
    REQ(shift);
    return guarded([&] { h->impl->rollBackground(Vec3i(shift[0], shift[1], shift[2]), keep_retired); });
}

int emf_fusion_set_background_store(emf_fusion_t* h, int on, uint64_t max_bytes) {
    REQ(h);
    return guarded([&] { h->impl->setBackgroundStore(on != 0, max_bytes ? max_bytes : TileStore::kDefaultBudget); });
}

int emf_fusion_background_store_info(emf_fusion_t* h, uint64_t out[5]) {
    REQ(h);
    REQ(out);
    return guarded([&] {
        const TileStore::Counters& c = h->impl->backgroundStore().counters();
        out[0] = c.tilesHeld;
        out[1] = c.bytesHeld;
        out[2] = c.tilesSpilled;
        out[3] = c.tilesRestored;
        out[4] = c.tilesEvicted;
    });
}

int emf_fusion_background_origin(emf_fusion_t* h, int32_t origin[3], float R[9], float t[3]) {
    REQ(h);
    REQ(origin);
    return guarded([&] {
        const Vec3i o = h->impl->backgroundOrigin();
        std::memcpy(origin, o.val, sizeof(o.val));
        const Affine3f pose = h->impl->getBackground().getPose();
        if (R) std::memcpy(R, pose.rotation().val, 9 * sizeof(float));
        if (t) std::memcpy(t, pose.translation().val, 3 * sizeof(float));
    });
}

int emf_fusion_retired_slabs(emf_fusion_t* h, int32_t* info, int capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] {
        const std::vector<RetiredSlab>& slabs = h->impl->retiredSlabs();
        *count = static_cast<int32_t>(slabs.size());
        for (int k = 0; info && k < capacity && k < static_cast<int>(slabs.size()); ++k) {
            int32_t* row = info + 7 * k;
            row[0] = slabs[k].frame;
            for (int i = 0; i < 3; ++i) {
                row[1 + i] = slabs[k].origin[i];
                row[4 + i] = slabs[k].res[i];
            }
        }
    });
}

int emf_fusion_retired_slab_mesh(emf_fusion_t* h, int index, uint32_t* num_vertices, uint32_t* num_triangles) {
    REQ(h);
    REQ(num_vertices);
    REQ(num_triangles);
    return guarded([&] {
        const std::vector<RetiredSlab>& slabs = h->impl->retiredSlabs();
        if (index < 0 || index >= static_cast<int>(slabs.size()))
            throw HipError("emf_fusion_retired_slab_mesh: no slab " + std::to_string(index), EMF_E_ARG);
        h->mesh = slabs[index].mesh;
        *num_vertices = static_cast<uint32_t>(h->mesh.vertices());
        *num_triangles = static_cast<uint32_t>(h->mesh.triangles());
    });
}

int emf_fusion_world_mesh(emf_fusion_t* h, int weld, uint32_t* num_vertices, uint32_t* num_triangles) {
    REQ(h);
    REQ(num_vertices);
    REQ(num_triangles);
    return guarded([&] {
        h->mesh = h->impl->worldMesh(weld);
        *num_vertices = static_cast<uint32_t>(h->mesh.vertices());
        *num_triangles = static_cast<uint32_t>(h->mesh.triangles());
    });
}

int emf_fusion_set_world_mesh_output(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setWorldMeshOutput(on != 0); });
}

int emf_fusion_world_mesh_info(emf_fusion_t* h, uint64_t out[4]) {
    REQ(h);
    REQ(out);
    return guarded([&] {
        const EMFusion::WorldMeshInfo& i = h->impl->worldMeshInfo();
        out[0] = i.volumeTiles;
        out[1] = i.storedTiles;
        out[2] = i.duplicateTiles;
        out[3] = i.storedSurfaceCubes;
    });
}

int emf_fusion_set_query_extent(emf_fusion_t* h, int world) {
    REQ(h);
    return guarded([&] { h->impl->setQueryExtent(world != 0); });
}

int emf_fusion_world_extent(emf_fusion_t* h, int32_t lo[3], int32_t size[3]) {
    REQ(h);
    REQ(lo);
    REQ(size);
    return guarded([&] {
        Vec3i a, n;
        h->impl->worldExtent(a, n);
        std::memcpy(lo, a.val, sizeof(a.val));
        std::memcpy(size, n.val, sizeof(n.val));
    });
}

// ---- what the scene queries (distance field, frontiers, plan) share ----
struct QueryArgs {
    Vec3i lo, size;  // no box: the whole background
    std::vector<int> exclude;
};

// the (box_lo, box_size, exclude_ids, num_exclude) arguments of the entry `who`; EMF_E_ARG with the message set
static int queryArgs(const char* who, emf_fusion_t* h, const int32_t* box_lo, const int32_t* box_size, const int32_t* exclude_ids,
                     int32_t num_exclude, QueryArgs& out) {
    if (num_exclude < 0 || (num_exclude > 0 && !exclude_ids)) {
        std::snprintf(g_err, sizeof(g_err), "%s: %d excluded ids without a list", who, num_exclude);
        return EMF_E_ARG;
    }
    if ((box_lo == nullptr) != (box_size == nullptr)) {
        std::snprintf(g_err, sizeof(g_err), "%s: box_lo and box_size go together", who);
        return EMF_E_ARG;
    }
    out.lo = box_lo ? Vec3i(box_lo[0], box_lo[1], box_lo[2]) : Vec3i(0, 0, 0);
    out.size = box_size ? Vec3i(box_size[0], box_size[1], box_size[2]) : h->impl->getBackground().getVolumeRes();
    out.exclude.assign(exclude_ids, exclude_ids + num_exclude);
    return EMF_OK;
}

// a result's box into the entry's outputs, each of which may be NULL
static void putBox(const QueryBox& b, int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3]) {
    const Vec3i lo = b.volumeLo();  // (a world box is kept with the padding of its virtual background)
    if (lo_out) std::memcpy(lo_out, lo.val, sizeof(lo.val));
    if (size_out) std::memcpy(size_out, b.size.val, sizeof(b.size.val));
    if (R) std::memcpy(R, b.boxPose.rotation().val, 9 * sizeof(float));
    if (t) std::memcpy(t, b.boxPose.translation().val, 3 * sizeof(float));
}

// one device array of the box, `elem` bytes per voxel, to the host on the main stream; NULL: not asked for
static void copyBoxArray(emf_fusion_t* h, const QueryBox& b, void* host, const void* dev, size_t elem, const char* what) {
    if (!host) return;
    Stream& s = h->impl->mainStream();
    hipCheck(hipMemcpyAsync(host, dev, b.voxels() * elem, hipMemcpyDeviceToHost, s.get()), what);
    s.waitForCompletion();
}

static int distance_field_entry(const char* who, emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3],
                                uint32_t site_mask, int32_t cap_voxels, const int32_t* exclude_ids, int32_t num_exclude,
                                int metres, bool nearest, int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3]) {
    REQ(h);
    QueryArgs a;
    if (const int rc = queryArgs(who, h, box_lo, box_size, exclude_ids, num_exclude, a)) return rc;
    return guarded([&] {
        putBox(h->impl->distanceField(a.lo, a.size, site_mask, cap_voxels, a.exclude, metres != 0, nearest).box, lo_out, size_out, R, t);
    });
}

int emf_fusion_distance_field(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], uint32_t site_mask,
                              int32_t cap_voxels, const int32_t* exclude_ids, int32_t num_exclude, int metres,
                              int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3]) {
    return distance_field_entry("emf_fusion_distance_field", h, box_lo, box_size, site_mask, cap_voxels, exclude_ids, num_exclude,
                                metres, false, lo_out, size_out, R, t);
}

int emf_fusion_distance_field_nearest(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], uint32_t site_mask,
                                      int32_t cap_voxels, const int32_t* exclude_ids, int32_t num_exclude, int metres,
                                      int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3]) {
    return distance_field_entry("emf_fusion_distance_field_nearest", h, box_lo, box_size, site_mask, cap_voxels, exclude_ids,
                                num_exclude, metres, true, lo_out, size_out, R, t);
}

int emf_fusion_copy_distance_nearest(emf_fusion_t* h, int32_t* nearest) {
    REQ(h);
    REQ(nearest);
    return guarded([&] {
        const EMFusion::DistanceField& df = h->impl->lastDistanceField();
        if (!df.classes) throw HipError("emf_fusion_copy_distance_nearest: no distance field has been computed", EMF_E_ARG);
        if (!df.nearest)
            throw HipError("emf_fusion_copy_distance_nearest: the last distance field was computed without the nearest-site index", EMF_E_ARG);
        copyBoxArray(h, df.box, nearest, df.nearest, sizeof(int32_t), "copy_distance_nearest");
    });
}

int emf_fusion_query_distance(emf_fusion_t* h, const int32_t* voxels, int32_t n, uint8_t* classes, int32_t* d2, int32_t* nearest,
                              int32_t lo_out[3], int32_t size_out[3]) {
    REQ(h);
    return guarded([&] {
        h->impl->queryDistance(voxels, n, classes, d2, nearest);
        putBox(h->impl->lastDistanceField().box, lo_out, size_out, nullptr, nullptr);
    });
}

int emf_fusion_set_distance_nearest_output(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setDistanceNearestOutput(on != 0); });
}

int emf_fusion_copy_distance_field(emf_fusion_t* h, uint8_t* classes, int32_t* d2, float* metres) {
    REQ(h);
    return guarded([&] {
        const EMFusion::DistanceField& df = h->impl->lastDistanceField();
        if (!df.classes) throw HipError("emf_fusion_copy_distance_field: no distance field has been computed", EMF_E_ARG);
        if (metres && !df.metres) throw HipError("emf_fusion_copy_distance_field: the last distance field has no metres", EMF_E_ARG);
        copyBoxArray(h, df.box, classes, df.classes, sizeof(uint8_t), "copy_distance_field");
        copyBoxArray(h, df.box, d2, df.d2, sizeof(int32_t), "copy_distance_field");
        copyBoxArray(h, df.box, metres, df.metres, sizeof(float), "copy_distance_field");
    });
}

int emf_fusion_distance_field_objects(emf_fusion_t* h, int32_t* ids, float* R, float* t, int capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] {
        const EMFusion::DistanceField& df = h->impl->lastDistanceField();
        *count = static_cast<int32_t>(df.objectIds.size());
        for (int k = 0; k < std::min<int>(capacity, *count); ++k) {
            if (ids) ids[k] = df.objectIds[k];
            if (R) std::memcpy(R + 9 * k, df.objectPoses[k].rotation().val, 9 * sizeof(float));
            if (t) std::memcpy(t + 3 * k, df.objectPoses[k].translation().val, 3 * sizeof(float));
        }
    });
}

int emf_fusion_set_distance_output(emf_fusion_t* h, int on, float cap_metres, int unknown_is_obstacle) {
    REQ(h);
    if (!(cap_metres >= 0.f)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_set_distance_output: cap %g", static_cast<double>(cap_metres));
        return EMF_E_ARG;
    }
    return guarded([&] { h->impl->setDistanceOutput(on != 0, cap_metres, unknown_is_obstacle != 0); });
}

int emf_fusion_frontiers(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], int32_t min_voxels,
                         int32_t clearance_voxels, const int32_t* exclude_ids, int32_t num_exclude, int32_t lo_out[3],
                         int32_t size_out[3], float R[9], float t[3], uint32_t counters[3]) {
    REQ(h);
    QueryArgs a;
    if (const int rc = queryArgs("emf_fusion_frontiers", h, box_lo, box_size, exclude_ids, num_exclude, a)) return rc;
    return guarded([&] {
        const EMFusion::Frontiers& f = h->impl->frontiers(a.lo, a.size, min_voxels, clearance_voxels, a.exclude);
        putBox(f.box, lo_out, size_out, R, t);
        if (counters) {
            counters[EMF_FRONTIER_KEPT] = f.kept;
            counters[EMF_FRONTIER_CLUSTERS] = f.all;
            counters[EMF_FRONTIER_VOXELS] = f.voxels;
        }
    });
}

int emf_fusion_copy_frontiers(emf_fusion_t* h, emf_frontier_cluster_t* records, int32_t capacity, double* rep_world,
                              double* centroid_world, int32_t* labels) {
    REQ(h);
    if (capacity < 0) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_copy_frontiers: capacity %d", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const EMFusion::Frontiers& f = h->impl->lastFrontiers();
        if (!f.labels) throw HipError("emf_fusion_copy_frontiers: no frontiers have been computed", EMF_E_ARG);
        const size_t n = std::min<size_t>(f.clusters.size(), static_cast<size_t>(capacity));
        for (size_t k = 0; k < n; ++k) {
            if (records) records[k] = f.clusters[k];
            if (rep_world) EMFusion::frontierWorldPoint(f, f.clusters[k], true, rep_world + 3 * k);
            if (centroid_world) EMFusion::frontierWorldPoint(f, f.clusters[k], false, centroid_world + 3 * k);
        }
        copyBoxArray(h, f.box, labels, f.labels, sizeof(int32_t), "copy_frontiers");
    });
}

int emf_fusion_set_frontier_output(emf_fusion_t* h, int on, int32_t min_voxels, float clearance_metres) {
    REQ(h);
    if (min_voxels < 1 || !(clearance_metres >= 0.f)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_set_frontier_output: min_voxels %d, clearance %g", min_voxels,
                      static_cast<double>(clearance_metres));
        return EMF_E_ARG;
    }
    return guarded([&] { h->impl->setFrontierOutput(on != 0, min_voxels, clearance_metres); });
}

int emf_fusion_plan(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], const int32_t* start_voxels,
                    int32_t num_start, int32_t seed_radius_voxels, int through_unknown, int32_t clearance_voxels,
                    uint32_t max_cost, const int32_t* goal_voxels, int32_t num_goals, int32_t path_capacity,
                    const int32_t* exclude_ids, int32_t num_exclude, int32_t lo_out[3], int32_t size_out[3], float R[9],
                    float t[3], uint32_t counters[4], int32_t* longest_path) {
    REQ(h);
    if (num_exclude < 0 || (num_exclude > 0 && !exclude_ids) || num_goals < 0 || (num_goals > 0 && !goal_voxels) ||
        num_start < 0 || (num_start > 0 && !start_voxels)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_plan: %d start voxels, %d goals or %d excluded ids without a list",
                      num_start, num_goals, num_exclude);
        return EMF_E_ARG;
    }
    QueryArgs a;
    if (const int rc = queryArgs("emf_fusion_plan", h, box_lo, box_size, exclude_ids, num_exclude, a)) return rc;
    return guarded([&] {
        std::vector<Vec3i> start, goals;
        if (num_start == 0) {  // the voxel under the camera
            const Vec3i c = h->impl->cameraVoxel();
            start.push_back(Vec3i(c[0] - a.lo[0], c[1] - a.lo[1], c[2] - a.lo[2]));
        }
        for (int32_t k = 0; k < num_start; ++k) start.push_back(Vec3i(start_voxels[3 * k], start_voxels[3 * k + 1], start_voxels[3 * k + 2]));
        for (int32_t k = 0; k < num_goals; ++k) goals.push_back(Vec3i(goal_voxels[3 * k], goal_voxels[3 * k + 1], goal_voxels[3 * k + 2]));
        const EMFusion::Plan& p = h->impl->plan(a.lo, a.size, start, seed_radius_voxels, through_unknown != 0, clearance_voxels,
                                                max_cost, goals, path_capacity, a.exclude);
        putBox(p.box, lo_out, size_out, R, t);
        if (counters) std::memcpy(counters, p.counters, sizeof(p.counters));
        if (longest_path) {
            *longest_path = 0;
            for (const EMFusion::Plan::Goal& g : p.goals) *longest_path = std::max<int32_t>(*longest_path, static_cast<int32_t>(g.path.size()));
        }
    });
}

int emf_fusion_copy_plan(emf_fusion_t* h, uint32_t* goal_cost, int32_t* lengths, int32_t* steps, int32_t* paths,
                         int32_t capacity, double* path_world, uint32_t* cost) {
    REQ(h);
    if (capacity < 0) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_copy_plan: capacity %d", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const EMFusion::Plan& p = h->impl->lastPlan();
        if (!p.cost) throw HipError("emf_fusion_copy_plan: no plan has been computed", EMF_E_ARG);
        for (size_t g = 0; g < p.goals.size(); ++g) {
            const EMFusion::Plan::Goal& r = p.goals[g];
            if (goal_cost) goal_cost[g] = r.cost;
            if (lengths) lengths[g] = r.length;
            if (steps) {
                steps[3 * g] = r.faces;
                steps[3 * g + 1] = r.edges;
                steps[3 * g + 2] = r.corners;
            }
            const size_t kept = std::min<size_t>(r.path.size(), static_cast<size_t>(capacity));
            for (size_t k = 0; k < kept; ++k) {
                if (paths) paths[g * capacity + k] = r.path[k];
                if (path_world) p.box.worldPoint(p.box.unravel(r.path[k]), path_world + 3 * (g * capacity + k));
            }
        }
        copyBoxArray(h, p.box, cost, p.cost, sizeof(uint32_t), "copy_plan");
    });
}

int emf_fusion_plan_cost_ptr(emf_fusion_t* h, const uint32_t** cost_dev) {
    REQ(h);
    REQ(cost_dev);
    return guarded([&] { *cost_dev = h->impl->lastPlan().cost; });
}

int emf_fusion_set_plan_output(emf_fusion_t* h, int on, float clearance_metres, int through_unknown) {
    REQ(h);
    if (!(clearance_metres >= 0.f)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_set_plan_output: clearance %g", static_cast<double>(clearance_metres));
        return EMF_E_ARG;
    }
    return guarded([&] { h->impl->setPlanOutput(on != 0, clearance_metres, through_unknown != 0); });
}

int emf_fusion_cast_rays(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], const int32_t* from,
                         const int32_t* to, int32_t n, uint32_t pass_mask, uint32_t count_mask, int32_t clearance_voxels,
                         const int32_t* exclude_ids, int32_t num_exclude, int32_t group, emf_ray_result_t* results,
                         emf_ray_group_t* groups, int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3]) {
    REQ(h);
    if (n < 0 || (n > 0 && (!from || !to)) || group < 0 || (group > 0) != (groups != nullptr) || (!results && !groups)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_cast_rays: %d rays in groups of %d without their lists or outputs", n, group);
        return EMF_E_ARG;
    }
    QueryArgs a;
    if (const int rc = queryArgs("emf_fusion_cast_rays", h, box_lo, box_size, exclude_ids, num_exclude, a)) return rc;
    return guarded([&] {
        const EMFusion::Rays& r = h->impl->castRays(a.lo, a.size, from, to, n, pass_mask, count_mask, clearance_voxels, a.exclude,
                                                    group, results != nullptr);
        putBox(r.box, lo_out, size_out, R, t);
        if (results) std::copy(r.results.begin(), r.results.end(), results);
        if (groups) std::copy(r.groups.begin(), r.groups.end(), groups);
    });
}

int emf_fusion_view_ray_targets(const double R[9], const double t[3], const double K[4], int32_t gw, int32_t gh, double range,
                                const float bg_R[9], const float bg_t[3], const int32_t res[3], float voxel_size,
                                const int32_t box_lo[3], int32_t origin[3], int32_t* targets) {
    REQ(R);
    REQ(t);
    REQ(K);
    REQ(bg_R);
    REQ(bg_t);
    REQ(res);
    REQ(box_lo);
    REQ(origin);
    return guarded([&] {
        viewRayTargets(R, t, K[0], K[1], K[2], K[3], gw, gh, range, bg_R, bg_t, Vec3i(res[0], res[1], res[2]), voxel_size,
                       Vec3i(box_lo[0], box_lo[1], box_lo[2]), origin, targets);
    });
}

int emf_fusion_view_gain(emf_fusion_t* h, const double* views_R, const double* views_t, int32_t num_views, int32_t gw, int32_t gh,
                         const double K[4], double range, const int32_t box_lo[3], const int32_t box_size[3],
                         const int32_t* exclude_ids, int32_t num_exclude, emf_ray_group_t* groups, int32_t* origins,
                         int32_t* targets, emf_ray_result_t* results, int32_t lo_out[3], int32_t size_out[3], float R[9],
                         float t[3]) {
    REQ(h);
    REQ(K);
    if (num_views < 0 || (num_views > 0 && (!views_R || !views_t || !groups))) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_view_gain: %d views without their poses or group records", num_views);
        return EMF_E_ARG;
    }
    QueryArgs a;
    if (const int rc = queryArgs("emf_fusion_view_gain", h, box_lo, box_size, exclude_ids, num_exclude, a)) return rc;
    return guarded([&] {
        std::vector<EMFusion::ViewPose> views(static_cast<size_t>(num_views));
        for (int32_t v = 0; v < num_views; ++v) {
            std::copy(views_R + 9 * v, views_R + 9 * v + 9, views[v].R);
            std::copy(views_t + 3 * v, views_t + 3 * v + 3, views[v].t);
        }
        const EMFusion::Rays& r = h->impl->viewGain(views, gw, gh, K, range, a.lo, a.size, a.exclude, results != nullptr);
        putBox(r.box, lo_out, size_out, R, t);
        std::copy(r.groups.begin(), r.groups.end(), groups);
        if (origins) std::copy(r.origins.begin(), r.origins.end(), origins);
        if (targets) std::copy(r.to.begin(), r.to.end(), targets);
        if (results) std::copy(r.results.begin(), r.results.end(), results);
    });
}

int emf_fusion_plan_shortcut(emf_fusion_t* h, int32_t window, int32_t* counts, int32_t* longest) {
    REQ(h);
    return guarded([&] {
        const EMFusion::Plan& p = h->impl->shortcutPlan(window);
        if (longest) *longest = 0;
        for (size_t g = 0; g < p.goals.size(); ++g) {
            const int32_t n = p.goals[g].length > 0 ? static_cast<int32_t>(p.goals[g].waypoints.size()) : 0;
            if (counts) counts[g] = n;
            if (longest) *longest = std::max(*longest, n);
        }
    });
}

int emf_fusion_copy_plan_shortcut(emf_fusion_t* h, int32_t* waypoints, int32_t capacity) {
    REQ(h);
    if (capacity < 0 || (capacity > 0 && !waypoints)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_copy_plan_shortcut: capacity %d", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const EMFusion::Plan& p = h->impl->lastPlan();
        if (!p.cost || h->impl->lastShortcutWindow() < 1) throw HipError("emf_fusion_copy_plan_shortcut: no shortcuts have been computed", EMF_E_ARG);
        for (size_t g = 0; g < p.goals.size(); ++g) {
            if (p.goals[g].length <= 0) continue;
            const std::vector<int32_t>& w = p.goals[g].waypoints;
            std::copy(w.begin(), w.begin() + std::min<size_t>(w.size(), static_cast<size_t>(capacity)), waypoints + g * static_cast<size_t>(capacity));
        }
    });
}

int emf_fusion_set_plan_shortcut_output(emf_fusion_t* h, int32_t window) {
    REQ(h);
    if (window < 0) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_set_plan_shortcut_output: window %d", window);
        return EMF_E_ARG;
    }
    return guarded([&] { h->impl->setPlanShortcutOutput(window); });
}

int emf_fusion_object_shapes(emf_fusion_t* h, const int32_t* ids, int32_t n, int32_t include_background, int32_t* ids_out,
                             int32_t* res_out, float* voxel_size_out, float* poses_out, emf_shape_moments_t* moments,
                             emf_shape_frame_t* frames, emf_shape_extents_t* extents, emf_shape_box_t* boxes) {
    REQ(h);
    if (n < 0 || (n > 0 && !ids)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_object_shapes: %d ids without a list", n);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const std::vector<EMFusion::ObjectShape>& shapes =
            h->impl->objectShapes(std::vector<int>(ids, ids + n), include_background != 0);
        for (size_t k = 0; k < shapes.size(); ++k) {
            const EMFusion::ObjectShape& s = shapes[k];
            if (ids_out) ids_out[k] = s.id;
            if (res_out) std::copy(s.res.val, s.res.val + 3, res_out + 3 * k);
            if (voxel_size_out) voxel_size_out[k] = s.voxelSize;
            if (poses_out) {
                std::copy(s.pose.rotation().val, s.pose.rotation().val + 9, poses_out + 12 * k);
                std::copy(s.pose.translation().val, s.pose.translation().val + 3, poses_out + 12 * k + 9);
            }
            if (moments) moments[k] = s.moments;
            if (frames) frames[k] = s.frame;
            if (extents) extents[k] = s.extents;
            if (boxes) boxes[k] = s.box;
        }
    });
}

int emf_fusion_shape_frame(const emf_shape_moments_t* moments, emf_shape_frame_t* frame) {
    REQ(moments);
    REQ(frame);
    return guarded([&] { shapeFrame(*moments, *frame); });
}

int emf_fusion_shape_box(const emf_shape_moments_t* moments, const emf_shape_frame_t* frame, const emf_shape_extents_t* extents,
                         const int32_t res[3], float voxel_size, const float R[9], const float t[3], emf_shape_box_t* box) {
    REQ(moments);
    REQ(frame);
    REQ(extents);
    REQ(res);
    REQ(R);
    REQ(t);
    REQ(box);
    if (!frame->valid) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_shape_box: a frame with valid == 0 has no box");
        return EMF_E_ARG;
    }
    return guarded([&] { shapeBox(*moments, *frame, *extents, res, voxel_size, R, t, *box); });
}

int emf_fusion_set_shape_output(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setShapeOutput(on != 0); });
}

int emf_fusion_object_contacts(emf_fusion_t* h, const int32_t* ids, int32_t n, int32_t include_background, double touch_m,
                               int32_t* ids_out, emf_contact_side_t* sides_out, int32_t* pair_ids_out, emf_contact_pair_t* pairs_out,
                               emf_contact_t* records_out, int32_t* summary_ids_out, emf_contact_summary_t* summaries_out,
                               int32_t* n_pairs_out, int32_t* n_summaries_out) {
    REQ(h);
    if (n < 0 || (n > 0 && !ids)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_object_contacts: %d ids without a list", n);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const EMFusion::ObjectContacts& c = h->impl->objectContacts(std::vector<int>(ids, ids + n), include_background != 0, touch_m);
        for (size_t k = 0; k < c.ids.size(); ++k) {
            if (ids_out) ids_out[k] = c.ids[k];
            if (sides_out && k < c.sides.size()) sides_out[k] = c.sides[k];
        }
        for (size_t k = 0; k < c.pairs.size(); ++k) {
            if (pair_ids_out) pair_ids_out[2 * k] = c.pairs[k].a, pair_ids_out[2 * k + 1] = c.pairs[k].b;
            if (pairs_out) pairs_out[k] = c.pairs[k].pair;
            if (records_out) records_out[k] = c.pairs[k].record;
        }
        for (size_t k = 0; k < c.summaries.size(); ++k) {
            const EMFusion::ObjectContacts::Summary& s = c.summaries[k];
            if (summary_ids_out) {
                int32_t* o = summary_ids_out + 4 * k;
                o[0] = s.a, o[1] = s.b, o[2] = s.recAB, o[3] = s.recBA;
            }
            if (summaries_out) summaries_out[k] = s.summary;
        }
        if (n_pairs_out) *n_pairs_out = static_cast<int32_t>(c.pairs.size());
        if (n_summaries_out) *n_summaries_out = static_cast<int32_t>(c.summaries.size());
    });
}

int emf_fusion_contact_pose(const float Ra[9], const float ta[3], const float Rb[9], const float tb[3], float R[9], float t[3]) {
    REQ(Ra);
    REQ(ta);
    REQ(Rb);
    REQ(tb);
    REQ(R);
    REQ(t);
    return guarded([&] { contactPose(Ra, ta, Rb, tb, R, t); });
}

int emf_fusion_contact_touch(double touch_m, float truncdist_b, float* touch) {
    REQ(touch);
    return guarded([&] { *touch = contactTouch(touch_m, truncdist_b); });
}

int emf_fusion_contact_summary(const emf_contact_t* ab, const emf_contact_t* ba, const emf_contact_side_t* a,
                               const emf_contact_side_t* b, emf_contact_summary_t* summary) {
    REQ(ab);
    REQ(a);
    REQ(b);
    REQ(summary);
    return guarded([&] { contactSummary(*ab, ba, *a, *b, *summary); });
}

int emf_fusion_set_contacts_output(emf_fusion_t* h, int on, double touch_m) {
    REQ(h);
    if (touch_m != touch_m) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_set_contacts_output: the touch distance is NaN");
        return EMF_E_ARG;
    }
    return guarded([&] { h->impl->setContactsOutput(on != 0, touch_m); });
}

static_assert(sizeof(emf_absorb_event_t) == 176, "mirrored by emfusion_amd/pipeline.py");

static emf_absorb_event_t absorbEvent(const EMFusion::AbsorbEvent& e) {
    emf_absorb_event_t o{};
    o.id = e.id, o.frame = e.frame, o.clipped = e.clipped ? 1 : 0;
    std::copy(e.R, e.R + 9, o.R);
    std::copy(e.t, e.t + 3, o.t);
    std::copy(e.lo, e.lo + 3, o.lo);
    std::copy(e.size, e.size + 3, o.size);
    o.record = e.record;
    return o;
}

int emf_fusion_absorb_pose(const float Rd[9], const float td[3], const float Rs[9], const float ts[3], float R[9], float t[3]) {
    REQ(Rd);
    REQ(td);
    REQ(Rs);
    REQ(ts);
    REQ(R);
    REQ(t);
    return guarded([&] { absorbPose(Rd, td, Rs, ts, R, t); });
}

int emf_fusion_set_absorb_objects(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setAbsorbObjects(on != 0); });
}

int emf_fusion_absorb_object(emf_fusion_t* h, int32_t id, emf_absorb_event_t* event) {
    REQ(h);
    return guarded([&] {
        const EMFusion::AbsorbEvent e = h->impl->absorbObject(id);
        if (event) *event = absorbEvent(e);
    });
}

int emf_fusion_absorbed(emf_fusion_t* h, emf_absorb_event_t* events, int32_t capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    if (capacity < 0 || (capacity > 0 && !events)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_absorbed: capacity %d without a list", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const std::vector<EMFusion::AbsorbEvent>& log = h->impl->absorbed();
        *count = static_cast<int32_t>(log.size());
        for (size_t k = 0; k < log.size() && k < static_cast<size_t>(capacity); ++k) events[k] = absorbEvent(log[k]);
    });
}

int emf_fusion_absorbed_colors(emf_fusion_t* h, emf_color_moved_t* records, int32_t capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    if (capacity < 0 || (capacity > 0 && !records)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_absorbed_colors: capacity %d without a list", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const std::vector<EMFusion::AbsorbEvent>& log = h->impl->absorbed();
        *count = static_cast<int32_t>(log.size());
        for (size_t k = 0; k < log.size() && k < static_cast<size_t>(capacity); ++k) records[k] = log[k].color;
    });
}

int emf_fusion_set_absorbed_output(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setAbsorbedOutput(on != 0); });
}

static_assert(sizeof(emf_lift_event_t) == 304, "mirrored by emfusion_amd/pipeline.py");

static emf_lift_event_t liftEvent(const EMFusion::LiftEvent& e) {
    emf_lift_event_t o{};
    o.id = e.id, o.frame = e.frame, o.clipped = e.clipped ? 1 : 0;
    std::copy(e.seedR, e.seedR + 9, o.seed_R);
    std::copy(e.seedT, e.seedT + 3, o.seed_t);
    std::copy(e.releaseR, e.releaseR + 9, o.release_R);
    std::copy(e.releaseT, e.releaseT + 3, o.release_t);
    std::copy(e.lo, e.lo + 3, o.lo);
    std::copy(e.size, e.size + 3, o.size);
    o.seed = e.seed;
    o.release = e.release;
    return o;
}

int emf_fusion_set_lift_objects(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setLiftObjects(on != 0); });
}

int emf_fusion_lift_object(emf_fusion_t* h, int32_t id, emf_lift_event_t* event) {
    REQ(h);
    return guarded([&] {
        const EMFusion::LiftEvent e = h->impl->liftObject(id);
        if (event) *event = liftEvent(e);
    });
}

int emf_fusion_lifted(emf_fusion_t* h, emf_lift_event_t* events, int32_t capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    if (capacity < 0 || (capacity > 0 && !events)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_lifted: capacity %d without a list", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const std::vector<EMFusion::LiftEvent>& log = h->impl->lifted();
        *count = static_cast<int32_t>(log.size());
        for (size_t k = 0; k < log.size() && k < static_cast<size_t>(capacity); ++k) events[k] = liftEvent(log[k]);
    });
}

int emf_fusion_lifted_colors(emf_fusion_t* h, emf_color_moved_t* records, int32_t capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    if (capacity < 0 || (capacity > 0 && !records)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_lifted_colors: capacity %d without a list", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const std::vector<EMFusion::LiftEvent>& log = h->impl->lifted();
        *count = static_cast<int32_t>(log.size());
        for (size_t k = 0; k < log.size() && k < static_cast<size_t>(capacity); ++k)
            records[2 * k] = log[k].seedColor, records[2 * k + 1] = log[k].releaseColor;
    });
}

int emf_fusion_set_lifted_output(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setLiftedOutput(on != 0); });
}

static_assert(sizeof(emf_merge_event_t) == 336, "mirrored by emfusion_amd/pipeline.py");

static emf_merge_event_t mergeEvent(const EMFusion::MergeEvent& e) {
    emf_merge_event_t o{};
    o.dst = e.dst, o.src = e.src, o.frame = e.frame, o.clipped = e.clipped ? 1 : 0, o.automatic = e.automatic ? 1 : 0;
    o.res_before = e.resBefore, o.res_after = e.resAfter;
    std::copy(e.dstR, e.dstR + 9, o.dst_R);
    std::copy(e.dstT, e.dstT + 3, o.dst_t);
    std::copy(e.srcR, e.srcR + 9, o.src_R);
    std::copy(e.srcT, e.srcT + 3, o.src_t);
    std::copy(e.R, e.R + 9, o.R);
    std::copy(e.t, e.t + 3, o.t);
    std::copy(e.lo, e.lo + 3, o.lo);
    std::copy(e.size, e.size + 3, o.size);
    o.overlap[0] = e.overlap[0], o.overlap[1] = e.overlap[1];
    o.record = e.record;
    o.counts = e.counts;
    o.color = e.color;
    return o;
}

int emf_fusion_merge_union(const int32_t dst_lo[3], const int32_t dst_hi[3], const int32_t dst_res[3], float dst_voxel_size,
                           const int32_t src_lo[3], const int32_t src_hi[3], const int32_t src_res[3], float src_voxel_size,
                           const float R[9], const float t[3], float lo[3], float hi[3], int32_t* any) {
    REQ(dst_lo);
    REQ(dst_hi);
    REQ(dst_res);
    REQ(src_lo);
    REQ(src_hi);
    REQ(src_res);
    REQ(R);
    REQ(t);
    REQ(lo);
    REQ(hi);
    REQ(any);
    return guarded([&] {
        *any = mergeUnion(dst_lo, dst_hi, dst_res, dst_voxel_size, src_lo, src_hi, src_res, src_voxel_size, R, t, lo, hi) ? 1 : 0;
    });
}

int emf_fusion_set_merge_objects(emf_fusion_t* h, int on, double min_overlap, int64_t min_surface, double touch_m, int32_t max_res) {
    REQ(h);
    return guarded([&] {
        EMFusion::MergeParams p;
        p.minOverlap = min_overlap, p.minSurface = min_surface, p.touch = touch_m, p.maxRes = max_res;
        h->impl->setMergeObjects(on != 0, p);
    });
}

int emf_fusion_object_bookkeeping(emf_fusion_t* h, int32_t id, int32_t* exists, int32_t* not_exists, double* scores, int32_t capacity,
                                  int32_t* count) {
    REQ(h);
    REQ(exists);
    REQ(not_exists);
    REQ(count);
    if (capacity < 0 || (capacity > 0 && !scores)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_object_bookkeeping: capacity %d without a list", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const ObjTSDF* o = h->impl->getObject(id);
        if (!o) throw HipError("object_bookkeeping: no object " + std::to_string(id), EMF_E_ARG);
        *exists = o->existCount(), *not_exists = o->nonExistCount();
        const std::vector<double>& s = o->classScores();
        *count = static_cast<int32_t>(s.size());
        std::copy(s.begin(), s.begin() + std::min<size_t>(s.size(), static_cast<size_t>(capacity)), scores);
    });
}

int emf_fusion_set_merged_output(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setMergedOutput(on != 0); });
}

int emf_fusion_merge_objects(emf_fusion_t* h, int32_t dst, int32_t src, emf_merge_event_t* event) {
    REQ(h);
    return guarded([&] {
        const EMFusion::MergeEvent e = h->impl->mergeObjects(dst, src);
        if (event) *event = mergeEvent(e);
    });
}

int emf_fusion_merged(emf_fusion_t* h, emf_merge_event_t* events, int32_t capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    if (capacity < 0 || (capacity > 0 && !events)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_merged: capacity %d without a list", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const std::vector<EMFusion::MergeEvent>& log = h->impl->merged();
        *count = static_cast<int32_t>(log.size());
        for (size_t k = 0; k < log.size() && k < static_cast<size_t>(capacity); ++k) events[k] = mergeEvent(log[k]);
    });
}

int emf_fusion_planes(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], const emf_plane_params_t* params,
                      int32_t lo_out[3], int32_t size_out[3], float R[9], float t[3], uint32_t counters[4], uint32_t* min_votes,
                      emf_plane_t* planes, int32_t capacity, int32_t* count) {
    REQ(h);
    if (capacity < 0 || (capacity > 0 && !planes)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_planes: capacity %d", capacity);
        return EMF_E_ARG;
    }
    QueryArgs a;
    if (const int rc = queryArgs("emf_fusion_planes", h, box_lo, box_size, nullptr, 0, a)) return rc;
    return guarded([&] {
        emf_plane_params_t p{15, 1, EMF_PLANE_MAX_PLANES, 2, 20.0, 0.0, 1.0, 2.0, 0};
        if (params) p = *params;
        const EMFusion::Planes& r = h->impl->planes(a.lo, a.size, p, true);
        putBox(r.box, lo_out, size_out, R, t);
        if (counters) std::copy(r.counters, r.counters + 4, counters);
        if (min_votes) *min_votes = r.minVotes;
        if (count) *count = static_cast<int32_t>(r.planes.size());
        std::copy(r.planes.begin(), r.planes.begin() + std::min<size_t>(r.planes.size(), static_cast<size_t>(capacity)), planes);
    });
}

int emf_fusion_set_planes_output(emf_fusion_t* h, int on, double angle_deg, int64_t min_votes, int ground_up_floor) {
    REQ(h);
    if (on && !(angle_deg > 0.0 && angle_deg <= 90.0)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_set_planes_output: an angle of %g degrees", angle_deg);
        return EMF_E_ARG;
    }
    return guarded([&] {
        EMFusion::PlanesOutput p;
        p.on = on != 0, p.angle = on ? angle_deg : 20.0, p.minVotes = min_votes;
        h->impl->setPlanesOutput(p);
        h->impl->setGroundUpFloor(ground_up_floor != 0);
    });
}

int emf_fusion_copy_plane_labels(emf_fusion_t* h, emf_plane_voxel_t* records, int16_t* labels, int64_t capacity) {
    REQ(h);
    if (capacity < 0) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_copy_plane_labels: capacity %lld", static_cast<long long>(capacity));
        return EMF_E_ARG;
    }
    return guarded([&] {
        const EMFusion::Planes& r = h->impl->lastPlanes();
        if (!r.records) throw HipError("emf_fusion_copy_plane_labels: no planes have been computed", EMF_E_ARG);
        const size_t n = std::min<size_t>(static_cast<size_t>(capacity), r.counters[2]);
        Stream& s = h->impl->mainStream();
        if (records && n) hipCheck(hipMemcpyAsync(records, r.records, n * sizeof(emf_plane_voxel_t), hipMemcpyDeviceToHost, s.get()), "copy_plane_labels (records)");
        if (labels && n) {
            if (r.labels) hipCheck(hipMemcpyAsync(labels, r.labels, n * sizeof(int16_t), hipMemcpyDeviceToHost, s.get()), "copy_plane_labels (labels)");
            else std::fill(labels, labels + n, static_cast<int16_t>(-1));
        }
        s.waitForCompletion();
    });
}

int emf_fusion_plane_directions(const uint32_t* bins, int32_t K, uint32_t min_votes, double separation_deg, double* dirs,
                                int32_t* bins_out, uint32_t* votes_out, int32_t* count) {
    REQ(bins);
    REQ(dirs);
    REQ(count);
    if (K < 1 || K > EMF_PLANE_MAX_K) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_plane_directions: K = %d", K);
        return K < 1 ? EMF_E_ARG : EMF_E_LIMIT;
    }
    return guarded([&] {
        const std::vector<PlaneDirection> d = planeDirections(bins, K, min_votes, separation_deg);
        *count = static_cast<int32_t>(d.size());
        for (size_t k = 0; k < d.size(); ++k) {
            std::copy(d[k].n, d[k].n + 3, dirs + 3 * k);
            if (bins_out) bins_out[k] = d[k].bin;
            if (votes_out) votes_out[k] = d[k].votes;
        }
    });
}

int emf_fusion_plane_offsets(const double n[3], const int32_t box_size[3], double bin_vox, double* lo, int64_t* slots,
                             double* inv_bin, double* shift, const uint32_t* row, uint32_t min_votes, int32_t peak_gap,
                             int32_t* peak_slots, uint32_t* peak_votes, int32_t capacity, int32_t* count) {
    REQ(n);
    REQ(box_size);
    if (!(bin_vox > 0.0) || box_size[0] < 1 || box_size[1] < 1 || box_size[2] < 1 || peak_gap < 0 || capacity < 0) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_plane_offsets: a bin that is not positive, an empty box or a negative gap");
        return EMF_E_ARG;
    }
    return guarded([&] {
        const PlaneOffsetFrame f = planeOffsetFrame(n, box_size, bin_vox);
        if (lo) *lo = f.lo;
        if (slots) *slots = f.slots;
        if (inv_bin) *inv_bin = f.invBin;
        if (shift) *shift = f.shift;
        if (!row) return;
        if (f.slots > EMF_PLANE_MAX_SLOTS) throw HipError("emf_fusion_plane_offsets: more than 4096 slots", EMF_E_LIMIT);
        const auto peaks = planePeaks(row, static_cast<int>(f.slots), min_votes, peak_gap);
        if (count) *count = static_cast<int32_t>(peaks.size());
        for (size_t k = 0; k < peaks.size() && k < static_cast<size_t>(capacity); ++k) {
            if (peak_slots) peak_slots[k] = peaks[k].first;
            if (peak_votes) peak_votes[k] = peaks[k].second;
        }
    });
}

int emf_fusion_plane_fit(const emf_plane_moments_t* moments, const double seed_n[3], double seed_d, emf_plane_t* plane) {
    REQ(moments);
    REQ(seed_n);
    REQ(plane);
    return guarded([&] { planeFit(*moments, seed_n, seed_d, *plane); });
}

int emf_fusion_plane_patches(emf_fusion_t* h, int32_t reach, int64_t min_count, uint32_t counters[3], emf_plane_patch_t* patches,
                             int32_t capacity, int32_t* count) {
    REQ(h);
    if (capacity < 0 || (capacity > 0 && !patches)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_plane_patches: capacity %d", capacity);
        return EMF_E_ARG;
    }
    return guarded([&] {
        const EMFusion::PlanePatches& r = h->impl->planePatches(reach, min_count);
        if (counters) std::copy(r.counters, r.counters + 3, counters);
        if (count) *count = static_cast<int32_t>(r.patches.size());
        std::copy(r.patches.begin(), r.patches.begin() + std::min<size_t>(r.patches.size(), static_cast<size_t>(capacity)), patches);
    });
}

int emf_fusion_copy_plane_patch_ids(emf_fusion_t* h, int32_t* ids, int64_t capacity) {
    REQ(h);
    if (capacity < 0) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_copy_plane_patch_ids: capacity %lld", static_cast<long long>(capacity));
        return EMF_E_ARG;
    }
    return guarded([&] {
        const EMFusion::Planes& r = h->impl->lastPlanes();
        const EMFusion::PlanePatches& p = h->impl->lastPlanePatches();
        if (!r.records || p.reach == 0) throw HipError("emf_fusion_copy_plane_patch_ids: no plane patches have been computed", EMF_E_ARG);
        const size_t n = std::min<size_t>(static_cast<size_t>(capacity), r.counters[2]);
        if (!ids || !n) return;
        if (!p.ids) {  // no plane was found: no record has a patch
            std::fill(ids, ids + n, -1);
            return;
        }
        Stream& s = h->impl->mainStream();
        hipCheck(hipMemcpyAsync(ids, p.ids, n * sizeof(int32_t), hipMemcpyDeviceToHost, s.get()), "copy_plane_patch_ids");
        s.waitForCompletion();
    });
}

int emf_fusion_plane_patch_rect(const emf_plane_t* plane, const emf_plane_patch_t* patch, emf_plane_patch_rect_t* rect) {
    REQ(plane);
    REQ(patch);
    REQ(rect);
    return guarded([&] { planePatchRect(*plane, *patch, *rect); });
}

int emf_fusion_plane_support(const double n[3], double d, const double center[3], const double axes[6], const double half[2],
                             const double box_center[3], const double box_axes[9], const double box_half[3], double margin,
                             double* s, int32_t* over) {
    REQ(n);
    REQ(center);
    REQ(axes);
    REQ(half);
    REQ(box_center);
    REQ(box_axes);
    REQ(box_half);
    REQ(s);
    REQ(over);
    return guarded([&] { *over = planeSupport(n, d, center, axes, half, box_center, box_axes, box_half, margin, *s) ? 1 : 0; });
}

int emf_fusion_set_plane_patches_output(emf_fusion_t* h, int on, int32_t reach, int64_t min_count) {
    REQ(h);
    if (on && (reach < 1 || reach > EMF_PLANE_MAX_REACH)) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_set_plane_patches_output: a reach of %d voxels", reach);
        return reach < 1 ? EMF_E_ARG : EMF_E_LIMIT;
    }
    return guarded([&] {
        EMFusion::PlanePatchesOutput p;
        p.on = on != 0, p.reach = on ? reach : 1, p.minCount = min_count;
        h->impl->setPlanePatchesOutput(p);
    });
}

static void copyGround(emf_fusion_t* h, const EMFusion::GroundMap& g, emf_ground_cell_t* cells, uint8_t* classes) {
    if (!g.cells) throw HipError("emf_fusion_copy_ground_map: no ground map has been computed", EMF_E_ARG);
    const size_t n = static_cast<size_t>(g.frame.map[0]) * g.frame.map[1];
    Stream& s = h->impl->mainStream();
    if (cells) hipCheck(hipMemcpyAsync(cells, g.cells, n * sizeof(emf_ground_cell_t), hipMemcpyDeviceToHost, s.get()), "copy_ground_map (cells)");
    if (classes) hipCheck(hipMemcpyAsync(classes, g.classes, n, hipMemcpyDeviceToHost, s.get()), "copy_ground_map (classes)");
    if (cells || classes) s.waitForCompletion();
}

int emf_fusion_ground_map(emf_fusion_t* h, const int32_t box_lo[3], const int32_t box_size[3], const int32_t* exclude_ids,
                          int32_t num_exclude, const double up[3], double cell, double bin, const double reference[3],
                          double band_lo, double band_hi, int32_t robot_bins, int32_t max_step_bins, int32_t lo_out[3],
                          int32_t size_out[3], emf_ground_frame_t* frame, double ground_pose[12], emf_ground_cell_t* cells,
                          uint8_t* classes, int64_t capacity) {
    REQ(h);
    REQ(up);
    REQ(reference);
    QueryArgs a;
    if (const int rc = queryArgs("emf_fusion_ground_map", h, box_lo, box_size, exclude_ids, num_exclude, a)) return rc;
    return guarded([&] {
        const EMFusion::GroundMap& g =
            h->impl->groundMap(a.lo, a.size, up, cell, bin, reference, band_lo, band_hi, robot_bins, max_step_bins, a.exclude);
        putBox(g.box, lo_out, size_out, nullptr, nullptr);
        if (frame) *frame = g.frame;
        if (ground_pose) std::copy(g.pose, g.pose + 12, ground_pose);
        if ((cells || classes) && capacity < static_cast<int64_t>(g.frame.map[0]) * g.frame.map[1])
            throw HipError("emf_fusion_ground_map: the outputs hold fewer cells than the map has", EMF_E_ARG);
        copyGround(h, g, cells, classes);
    });
}

int emf_fusion_copy_ground_map(emf_fusion_t* h, emf_ground_cell_t* cells, uint8_t* classes) {
    REQ(h);
    return guarded([&] { copyGround(h, h->impl->lastGroundMap(), cells, classes); });
}

int emf_fusion_ground_classes_ptr(emf_fusion_t* h, void** classes_dev, void** cells_dev) {
    REQ(h);
    return guarded([&] {
        const EMFusion::GroundMap& g = h->impl->lastGroundMap();
        if (!g.cells) throw HipError("emf_fusion_ground_classes_ptr: no ground map has been computed", EMF_E_ARG);
        if (classes_dev) *classes_dev = const_cast<uint8_t*>(g.classes);
        if (cells_dev) *cells_dev = const_cast<emf_ground_cell_t*>(g.cells);
    });
}

int emf_fusion_set_ground_output(emf_fusion_t* h, int on, const double up[3], double cell, double bin, double band_lo,
                                 double band_hi, double robot_height, double max_step) {
    REQ(h);
    return guarded([&] {
        EMFusion::GroundOutput g;
        g.on = on != 0;
        if (up) std::copy(up, up + 3, g.up);
        g.cell = cell, g.bin = bin, g.bandLo = band_lo, g.bandHi = band_hi, g.robotHeight = robot_height, g.maxStep = max_step;
        h->impl->setGroundOutput(g);
    });
}

int emf_fusion_ground_frame(const int32_t box_lo[3], const int32_t box_size[3], const int32_t bg_res[3], float voxel_size,
                            const float R[9], const float t[3], const double up[3], double cell, double bin,
                            const double reference[3], double band_lo, double band_hi, emf_ground_frame_t* frame,
                            double ground_pose[12]) {
    REQ(box_lo);
    REQ(box_size);
    REQ(bg_res);
    REQ(R);
    REQ(t);
    REQ(up);
    REQ(reference);
    REQ(frame);
    REQ(ground_pose);
    return guarded([&] {
        QueryBox box;
        box.lo = Vec3i(box_lo[0], box_lo[1], box_lo[2]);
        box.size = Vec3i(box_size[0], box_size[1], box_size[2]);
        box.bgRes = Vec3i(bg_res[0], bg_res[1], bg_res[2]);
        box.voxelSize = voxel_size;
        box.bgPose = Affine3f(Matx33f(R), Vec3f(t[0], t[1], t[2]));
        for (int i = 0; i < 3; ++i)
            if (box.size[i] < 1) throw HipError("emf_fusion_ground_frame: an empty box", EMF_E_ARG);
        if (!(voxel_size > 0.f)) throw HipError("emf_fusion_ground_frame: a voxel size that is not positive", EMF_E_ARG);
        std::string why;
        emf_ground_frame_t f{};
        double pose[12];
        if (const int rc = groundFrame(box, up, cell, bin, reference, band_lo, band_hi, f, pose, why))
            throw HipError("emf_fusion_ground_frame: " + why, rc);
        *frame = f;
        std::copy(pose, pose + 12, ground_pose);
    });
}

int emf_fusion_follow_shift(const float q[3], const int32_t step[3], float voxel_size, int32_t shift[3]) {
    REQ(q);
    REQ(step);
    REQ(shift);
    return guarded([&] {
        if (!EMFusion::followShift(q, step, voxel_size, shift))
            throw HipError("emf_fusion_follow_shift: the step must be a positive multiple of the tile (32, 8, 8), the voxel "
                           "size positive and q finite",
                           EMF_E_ARG);
    });
}

int emf_io_read_color_png(const char* path, uint8_t* out, size_t capacity, int32_t* width, int32_t* height) {
    REQ(path);
    return guarded([&] {
        std::vector<uint8_t> px;
        int w = 0, hgt = 0;
        readPngColor(path, px, w, hgt);
        if (width) *width = w;
        if (height) *height = hgt;
        if (out) {
            if (capacity < px.size()) throw HipError("emf_io_read_color_png: buffer too small", EMF_E_ARG);
            std::memcpy(out, px.data(), px.size());
        }
    });
}

int emf_io_read_depth_png(const char* path, float scale, float* out, size_t capacity, int32_t* width, int32_t* height) {
    REQ(path);
    return guarded([&] {
        std::vector<uint16_t> px;
        int w = 0, hgt = 0;
        readPngGray(path, px, w, hgt);
        if (width) *width = w;
        if (height) *height = hgt;
        if (out) {
            if (capacity < px.size()) throw HipError("emf_io_read_depth_png: buffer too small", EMF_E_ARG);
            for (size_t i = 0; i < px.size(); ++i) out[i] = static_cast<float>(px[i]) * scale;
        }
    });
}

int emf_io_load_config(const char* path, const char* calibration, emf_fusion_params_t* p, char* dump, size_t dump_capacity) {
    return guarded([&] {
        Params q;
        if (path && path[0]) loadConfigFile(q, path);
        if (calibration && calibration[0]) loadCalibrationFile(q, calibration);
        if (p) {
            emf_fusion_default_params(p);
            p->width = q.frameSize.width;
            p->height = q.frameSize.height;
            for (int k = 0; k < 9; ++k) p->K[k] = q.intr.val[k];
            for (int k = 0; k < 3; ++k) {
                p->bg_res[k] = q.globalVolumeDims[k];
                p->obj_res[k] = q.objVolumeDims[k];
                p->volume_pose_t[k] = q.volumePose.translation()[k];
            }
            p->bg_voxel_size = q.globalVoxelSize;
            p->bg_rel_truncdist = q.globalRelTruncDist;
            p->obj_rel_truncdist = q.objRelTruncDist;
            p->max_tsdf_weight = q.tsdfParams.maxTSDFWeight;
            p->assoc_sigma = q.tsdfParams.assocSigma;
            p->alpha = q.tsdfParams.alpha;
            p->uni_prior = q.tsdfParams.uniPrior;
            p->visibility_thresh = q.visibilityThresh;
            p->boundary = q.boundary;
            p->mask_frames = q.maskRCNNFrames;
            p->max_tracking_iter = q.maxTrackingIter;
        }
        if (dump && dump_capacity) std::snprintf(dump, dump_capacity, "%s", dumpConfig(q).c_str());
    });
}

int emf_io_read_exr(const char* path, const char* channel, float* out, size_t capacity, int32_t* width, int32_t* height) {
    REQ(path);
    return guarded([&] {
        std::vector<float> px;
        const Size s = readExr(path, px, channel ? channel : "");
        if (width) *width = s.width;
        if (height) *height = s.height;
        if (out) {
            if (capacity < px.size()) throw HipError("emf_io_read_exr: buffer too small", EMF_E_ARG);
            std::copy(px.begin(), px.end(), out);
        }
    });
}

int emf_io_image_reader(const char* base, const char* colordir, const char* depthdir, int32_t* num_frames, int32_t* first) {
    REQ(base);
    REQ(colordir);
    REQ(depthdir);
    return guarded([&] {
        const ImageReader r(base, colordir, depthdir);
        if (num_frames) *num_frames = static_cast<int32_t>(r.getNumFrames());
        if (first) *first = r.firstIndex();
    });
}

int emf_io_tum_associations(const char* file, int index, char* depth_name, int name_capacity, double* stamp, int32_t* count) {
    REQ(file);
    return guarded([&] {
        std::vector<std::string> rgb, depth;
        std::vector<double> stamps;
        TUMRGBDReader::readFileAssociations(file, rgb, depth, &stamps);
        if (count) *count = static_cast<int32_t>(depth.size());
        if (index >= 0 && index < static_cast<int>(depth.size())) {
            if (depth_name && name_capacity > 0) std::snprintf(depth_name, static_cast<size_t>(name_capacity), "%s", depth[index].c_str());
            if (stamp) *stamp = stamps[index];
        }
    });
}

int emf_io_load_preproc_masks(const char* path, int32_t* n, int32_t* width, int32_t* height, uint8_t* masks,
                              size_t mask_capacity, double* boxes, size_t box_capacity, double* scores, size_t score_capacity,
                              int32_t* nscores) {
    REQ(path);
    return guarded([&] {
        PreprocMasks pm;
        const int k = loadPreprocessedMasks(path, pm);
        if (n) *n = k;
        if (width) *width = pm.width;
        if (height) *height = pm.height;
        const size_t per = static_cast<size_t>(pm.width) * pm.height;
        const size_t ns = pm.scores.empty() ? 0 : pm.scores[0].size();
        for (const auto& row : pm.scores)  // (a list of lists may be ragged; the flat output is not)
            if (row.size() != ns) throw HipError("emf_io_load_preproc_masks: class-score rows of different lengths", EMF_E_ARG);
        if (nscores) *nscores = static_cast<int32_t>(ns);
        if (masks && mask_capacity >= per * k)
            for (int i = 0; i < k; ++i) std::memcpy(masks + per * i, pm.masks[i].data(), per);
        if (boxes && box_capacity >= 4 * static_cast<size_t>(k))
            for (int i = 0; i < k; ++i) std::memcpy(boxes + 4 * i, pm.boxes[i].data(), 4 * sizeof(double));
        if (scores && score_capacity >= ns * pm.scores.size())
            for (size_t i = 0; i < pm.scores.size(); ++i) std::memcpy(scores + ns * i, pm.scores[i].data(), ns * sizeof(double));
    });
}

int emf_fusion_set_tracking(emf_fusion_t* h, int track_camera, int track_objects) {
    REQ(h);
    h->trackCamera = track_camera != 0;
    h->trackObjects = track_objects != 0;
    return EMF_OK;
}

int emf_fusion_create_object_from_mask(emf_fusion_t* h, const emf_image_t* mask, int32_t* id) {
    REQ(h);
    REQ(mask);
    REQ(id);
    return guarded([&] { *id = h->impl->initNewObjVolume(*mask); });
}

int emf_fusion_queue_new_object_masks(emf_fusion_t* h, int n, const emf_image_t* masks) {
    REQ(h);
    if (n > 0) REQ(masks);
    return guarded([&] { h->queuedMasks.assign(masks, masks + (n > 0 ? n : 0)); });
}

int emf_fusion_queue_instance_masks(emf_fusion_t* h, int n, const emf_image_t* masks) {
    REQ(h);
    if (n > 0) REQ(masks);
    return guarded([&] { h->queuedInstances.assign(masks, masks + (n > 0 ? n : 0)); });
}

int emf_fusion_queue_instance_scores(emf_fusion_t* h, int n, int num_classes, const double* scores) {
    REQ(h);
    if (n > 0) REQ(scores);
    return guarded([&] {
        h->queuedScores.clear();
        for (int i = 0; i < n; ++i)
            h->queuedScores.emplace_back(scores + static_cast<size_t>(i) * num_classes,
                                         scores + static_cast<size_t>(i + 1) * num_classes);
    });
}

int emf_fusion_object_class(emf_fusion_t* h, int id, int32_t* class_id) {
    REQ(h);
    REQ(class_id);
    return guarded([&] {
        const ObjTSDF* o = h->impl->getObject(id);
        if (!o) throw HipError("object_class: no object " + std::to_string(id), EMF_E_ARG);
        *class_id = o->getClassID();
    });
}

int emf_fusion_object_info(emf_fusion_t* h, int id, int32_t res[3], float* voxel_size, float* truncdist, float* existence) {
    REQ(h);
    return guarded([&] {
        const ObjTSDF* o = h->impl->getObject(id);
        if (!o) throw HipError("object_info: no object " + std::to_string(id), EMF_E_ARG);
        const Vec3i r = o->getVolumeRes();
        if (res) { res[0] = r[0]; res[1] = r[1]; res[2] = r[2]; }
        if (voxel_size) *voxel_size = o->getVoxelSize();
        if (truncdist) *truncdist = o->getTruncDist();
        if (existence) *existence = o->getExProb();
    });
}

int emf_fusion_set_ignore_person(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->setIgnorePerson(on != 0); });
}

int emf_fusion_last_mask_assignment(emf_fusion_t* h, int32_t* ids, int capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] {
        const auto& v = h->impl->lastMaskAssignment();
        *count = static_cast<int32_t>(v.size());
        for (int i = 0; ids && i < capacity && i < static_cast<int>(v.size()); ++i) ids[i] = v[i];
    });
}

int emf_fusion_last_created(emf_fusion_t* h, int32_t* ids, int capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] {
        const auto& v = h->impl->lastCreatedObjects();
        *count = static_cast<int32_t>(v.size());
        for (int i = 0; ids && i < capacity && i < static_cast<int>(v.size()); ++i) ids[i] = v[i];
    });
}

int emf_fusion_match_mask(emf_fusion_t* h, const emf_image_t* mask, int32_t* id, float* iou) {
    REQ(h);
    REQ(mask);
    REQ(id);
    REQ(iou);
    return guarded([&] { *id = h->impl->matchSegmentation(*mask, *iou); });
}

int emf_fusion_update_object(emf_fusion_t* h, int id, const emf_image_t* mask, float offset[3]) {
    REQ(h);
    REQ(mask);
    REQ(offset);
    return guarded([&] {
        const emf::Vec3f o = h->impl->updateObject(id, *mask);
        for (int i = 0; i < 3; ++i) offset[i] = o[i];
    });
}

int emf_fusion_extract_mesh(emf_fusion_t* h, int id, uint32_t* num_vertices, uint32_t* num_triangles) {
    REQ(h);
    REQ(num_vertices);
    REQ(num_triangles);
    return guarded([&] {
        h->mesh = h->impl->getMesh(id);
        *num_vertices = static_cast<uint32_t>(h->mesh.vertices());
        *num_triangles = static_cast<uint32_t>(h->mesh.triangles());
    });
}

int emf_fusion_copy_mesh(emf_fusion_t* h, float* vertices, float* normals, int32_t* triangles) {
    REQ(h);
    return guarded([&] {
        const emf::Mesh& m = h->mesh;
        if (vertices) std::copy(m.cloud.begin(), m.cloud.end(), vertices);
        if (normals) std::copy(m.normals.begin(), m.normals.end(), normals);
        if (triangles) std::copy(m.polygons.begin(), m.polygons.end(), triangles);
    });
}

int emf_fusion_copy_mesh_colors(emf_fusion_t* h, uint8_t* colors) {
    REQ(h);
    REQ(colors);
    return guarded([&] {
        const emf::Mesh& m = h->mesh;
        if (m.colors.size() != m.cloud.size())
            throw HipError("emf_fusion_copy_mesh_colors: the mesh has no colours (emf_fusion_set_color)", EMF_E_ARG);
        std::copy(m.colors.begin(), m.colors.end(), colors);
    });
}

int emf_fusion_copy_meshes_colors(emf_fusion_t* h, uint8_t* colors) {
    REQ(h);
    REQ(colors);
    return guarded([&] {
        for (const emf::Mesh& m : h->meshList) {
            if (m.colors.size() != m.cloud.size())
                throw HipError("emf_fusion_copy_meshes_colors: the meshes have no colours (emf_fusion_set_color)", EMF_E_ARG);
            colors = std::copy(m.colors.begin(), m.colors.end(), colors);
        }
    });
}

int emf_fusion_extract_meshes(emf_fusion_t* h, const int32_t* ids, int n, uint32_t* counts) {
    REQ(h);
    REQ(ids);
    REQ(counts);
    if (n < 1 || n > EMF_MAX_MODELS) {
        std::snprintf(g_err, sizeof(g_err), "emf_fusion_extract_meshes: %d models (1 .. %d)", n, EMF_MAX_MODELS);
        return EMF_E_LIMIT;
    }
    return guarded([&] {
        h->meshList = h->impl->extractMeshes(std::vector<int>(ids, ids + n));
        for (int k = 0; k < n; ++k) {
            counts[2 * k] = static_cast<uint32_t>(h->meshList[k].vertices());
            counts[2 * k + 1] = static_cast<uint32_t>(h->meshList[k].triangles());
        }
    });
}

int emf_fusion_copy_meshes(emf_fusion_t* h, float* vertices, float* normals, int32_t* triangles) {
    REQ(h);
    return guarded([&] {
        for (const emf::Mesh& m : h->meshList) {
            if (vertices) vertices = std::copy(m.cloud.begin(), m.cloud.end(), vertices);
            if (normals) normals = std::copy(m.normals.begin(), m.normals.end(), normals);
            if (triangles) triangles = std::copy(m.polygons.begin(), m.polygons.end(), triangles);
        }
    });
}

int emf_io_write_mesh(const char* filename, uint32_t num_vertices, const float* vertices,
                      const float* normals, uint32_t num_triangles, const int32_t* triangles) {
    REQ(filename);
    if (num_vertices) {
        REQ(vertices);
        REQ(normals);
    }
    if (num_triangles) REQ(triangles);
    return guarded([&] {
        emf::Mesh m;
        m.cloud.assign(vertices, vertices + 3 * static_cast<size_t>(num_vertices));
        m.normals.assign(normals, normals + 3 * static_cast<size_t>(num_vertices));
        m.polygons.assign(triangles, triangles + 4 * static_cast<size_t>(num_triangles));
        io::writeMesh(filename, m);
    });
}

int emf_io_write_mesh_colors(const char* filename, uint32_t num_vertices, const float* vertices, const float* normals,
                             const uint8_t* colors, uint32_t num_triangles, const int32_t* triangles) {
    REQ(filename);
    if (num_vertices) {
        REQ(vertices);
        REQ(normals);
        REQ(colors);
    }
    if (num_triangles) REQ(triangles);
    return guarded([&] {
        emf::Mesh m;
        m.cloud.assign(vertices, vertices + 3 * static_cast<size_t>(num_vertices));
        m.normals.assign(normals, normals + 3 * static_cast<size_t>(num_vertices));
        m.colors.assign(colors, colors + 3 * static_cast<size_t>(num_vertices));
        m.colored = true;
        m.polygons.assign(triangles, triangles + 4 * static_cast<size_t>(num_triangles));
        io::writeMesh(filename, m);
    });
}

int emf_fusion_render(emf_fusion_t* h, uint8_t* rgb, uint8_t* color_map) {
    REQ(h);
    REQ(rgb);
    return guarded([&] {
        h->impl->render(rgb);
        if (color_map) std::copy(h->impl->getColorMap().begin(), h->impl->getColorMap().end(), color_map);
    });
}

int emf_fusion_render_view(emf_fusion_t* h, const float R[9], const float t[3], const float K[9], int32_t width,
                           int32_t height, uint8_t* rgb, float* raylengths, uint8_t* seg) {
    REQ(h);
    REQ(R);
    REQ(t);
    REQ(K);
    REQ(rgb);
    return guarded([&] {
        h->impl->renderView(Affine3f(m33(R), Vec3f(t[0], t[1], t[2])), K, Size(width, height), rgb, raylengths, seg);
    });
}

int emf_fusion_render_view_shaded(emf_fusion_t* h, const float R[9], const float t[3], const float K[9], int32_t width,
                                  int32_t height, int shading, uint8_t* rgb, float* raylengths, uint8_t* seg) {
    REQ(h);
    REQ(R);
    REQ(t);
    REQ(K);
    REQ(rgb);
    return guarded([&] {
        h->impl->renderView(Affine3f(m33(R), Vec3f(t[0], t[1], t[2])), K, Size(width, height), rgb, raylengths, seg, shading);
    });
}

int emf_fusion_set_3d_view_shading(emf_fusion_t* h, int shading) {
    REQ(h);
    return guarded([&] { h->impl->set3dViewShading(shading); });
}

int emf_fusion_set_3d_view(emf_fusion_t* h, const float R[9], const float t[3], const float K[9], int32_t width,
                           int32_t height) {
    REQ(h);
    REQ(R);
    REQ(t);
    REQ(K);
    return guarded([&] { h->impl->set3dView(Affine3f(m33(R), Vec3f(t[0], t[1], t[2])), K, Size(width, height)); });
}

int emf_fusion_clear_3d_view(emf_fusion_t* h) {
    REQ(h);
    return guarded([&] { h->impl->clear3dView(); });
}

int emf_fusion_set_depth_broadcast(emf_fusion_t* h, int root) {
    REQ(h);
    return guarded([&] { h->impl->setDepthBroadcastRoot(root); });
}

int emf_fusion_enable_pose_log(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->enablePoseLog(on != 0); });
}

int emf_fusion_setup_output(emf_fusion_t* h, int exp_frame_meshes, int exp_vols) {
    REQ(h);
    return guarded([&] { h->impl->setupOutput(exp_frame_meshes != 0, exp_vols != 0); });
}

int emf_fusion_write_results(emf_fusion_t* h, const char* dir, int volumes) {
    REQ(h);
    REQ(dir);
    return guarded([&] { h->impl->writeResults(dir, volumes != 0); });
}

int emf_io_write_volume(const char* filename, const float* voxels, const int32_t res[3], float voxel_size) {
    REQ(filename);
    REQ(voxels);
    REQ(res);
    return guarded([&] {
        io::writeVolume(filename, voxels, sizeof(float), Vec3i(res[0], res[1], res[2]), voxel_size);
    });
}

int emf_io_write_pose_file(const char* filename, int n, const int32_t* frames, const float* R,
                           const float* t) {
    REQ(filename);
    if (n > 0) {
        REQ(frames);
        REQ(R);
        REQ(t);
    }
    return guarded([&] {
        std::map<int, Affine3f> poses;
        for (int i = 0; i < n; ++i)
            poses[frames[i]] = Affine3f(m33(R + 9 * i), Vec3f(t[3 * i], t[3 * i + 1], t[3 * i + 2]));
        io::writePoseFile(filename, poses);
    });
}

int emf_io_png_unfilter(const uint8_t* rows, int height, int stride, int bpp, uint8_t* out) {
    REQ(rows);
    REQ(out);
    if (height < 0 || stride <= 0 || bpp < 1 || bpp > 4) return EMF_E_ARG;
    // PNG specification 9.2: each scan line is preceded by its filter type; Sub / Average / Paeth
    // predict from the reconstructed byte bpp positions to the left (a), above (b), above-left (c)
    const uint8_t* prev = nullptr;
    for (int y = 0; y < height; ++y) {
        const uint8_t* in = rows + static_cast<size_t>(y) * (stride + 1);
        uint8_t* cur = out + static_cast<size_t>(y) * stride;
        const int f = in[0];
        if (f > 4) return EMF_E_ARG;
        for (int x = 0; x < stride; ++x) {
            const int a = x >= bpp ? cur[x - bpp] : 0;
            const int b = prev ? prev[x] : 0;
            const int c = (prev && x >= bpp) ? prev[x - bpp] : 0;
            int pred = 0;
            if (f == 1) pred = a;
            else if (f == 2) pred = b;
            else if (f == 3) pred = (a + b) >> 1;
            else if (f == 4) {
                const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
                pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
            }
            cur[x] = static_cast<uint8_t>(in[1 + x] + pred);
        }
        prev = cur;
    }
    return EMF_OK;
}

int emf_fusion_set_cleanup(emf_fusion_t* h, int on) {
    REQ(h);
    h->cleanUp = on != 0;
    return EMF_OK;
}

int emf_fusion_last_deleted(emf_fusion_t* h, int32_t* ids, int capacity, int32_t* count) {
    REQ(h);
    REQ(count);
    return guarded([&] {
        const auto& v = h->impl->lastDeletedObjects();
        *count = static_cast<int32_t>(v.size());
        for (int i = 0; ids && i < capacity && i < static_cast<int>(v.size()); ++i) ids[i] = v[i];
    });
}

int emf_fusion_set_preprocess(emf_fusion_t* h, int on) {
    REQ(h);
    h->preprocess = on != 0;
    return EMF_OK;
}

int emf_fusion_get_pose(emf_fusion_t* h, int id, float R[9], float t[3]) {
    REQ(h);
    REQ(R);
    REQ(t);
    return guarded([&] {
        Affine3f p;
        if (id == 0) {
            p = h->impl->getCameraPose();
        } else {
            const ObjTSDF* o = h->impl->getObject(id);
            if (!o) throw HipError("emf_fusion_get_pose: no such object on this rank", EMF_E_ARG);
            p = o->getPose();
        }
        for (int k = 0; k < 9; ++k) R[k] = p.rotation().val[k];
        for (int k = 0; k < 3; ++k) t[k] = p.translation()[k];
    });
}

int emf_fusion_track_result(emf_fusion_t* h, int id, int32_t* iterations, int32_t* accepted,
                            int32_t* converged, float* error) {
    REQ(h);
    return guarded([&] {
        const TrackResult* r = h->impl->getTrackResult(id);
        if (!r) throw HipError("emf_fusion_track_result: model was never tracked", EMF_E_ARG);
        if (iterations) *iterations = r->iterations;
        if (accepted) *accepted = r->accepted;
        if (converged) *converged = r->converged ? 1 : 0;
        if (error) *error = r->error;
    });
}

int emf_fusion_stage_estep(emf_fusion_t* h) {
    REQ(h);
    return guarded([&] { h->impl->computeAssociationWeights(); });
}
int emf_fusion_stage_raycast(emf_fusion_t* h) {
    REQ(h);
    return guarded([&] { h->impl->raycast(); });
}
int emf_fusion_stage_integrate(emf_fusion_t* h) {
    REQ(h);
    return guarded([&] { h->impl->integrateDepth(); });
}

int emf_fusion_synchronize(emf_fusion_t* h) {
    REQ(h);
    return guarded([&] { h->impl->synchronize(); });
}

int emf_fusion_enable_timings(emf_fusion_t* h, int on) {
    REQ(h);
    h->impl->enableTimings(on != 0);
    return EMF_OK;
}

int emf_fusion_last_timings(emf_fusion_t* h, emf_frame_timings_t* out) {
    REQ(h);
    REQ(out);
    const FrameTimings& t = h->impl->lastTimings();
    *out = emf_frame_timings_t{t.points, t.estep, t.raycast, t.composite, t.integrate, t.masks,
                               t.total};
    return EMF_OK;
}

int emf_fusion_enable_raycast_stats(emf_fusion_t* h, int on) {
    REQ(h);
    return guarded([&] { h->impl->enableRaycastStats(on != 0); });
}

int emf_fusion_raycast_stats(emf_fusion_t* h, uint64_t counters[4]) {
    REQ(h);
    REQ(counters);
    return guarded([&] {
        const auto c = h->impl->raycastStats();
        for (int i = 0; i < 4; ++i) counters[i] = c[i];
    });
}

int emf_fusion_kernel_timers_enable(emf_fusion_t* h, uint64_t max_launches) {
    REQ(h);
    return guarded([&] {
        h->impl->synchronize();
        h->impl->kernelTimers().enable(static_cast<size_t>(max_launches));
    });
}

int emf_fusion_kernel_timers_clear(emf_fusion_t* h) {
    REQ(h);
    h->impl->kernelTimers().clear();
    return EMF_OK;
}

int emf_fusion_kernel_timers_select(emf_fusion_t* h, uint32_t kind_mask) {
    REQ(h);
    return guarded([&] { h->impl->kernelTimers().select(kind_mask); });
}

int emf_fusion_kernel_timers_stride(emf_fusion_t* h, uint32_t every) {
    REQ(h);
    return guarded([&] { h->impl->kernelTimers().setStride(every); });
}

int emf_fusion_kernel_timers_collect(emf_fusion_t* h, emf_kernel_summary_t out[EMF_K_NUM_KINDS],
                                     uint64_t* dropped) {
    REQ(h);
    REQ(out);
    static_assert(static_cast<int>(EMF_K_NUM_KINDS) == static_cast<int>(KernelTimers::kNumKinds),
                  "kernel kind enums out of sync");
    return guarded([&] {
        h->impl->synchronize();
        const auto s = h->impl->kernelTimers().collect();
        for (int k = 0; k < EMF_K_NUM_KINDS; ++k)
            out[k] = emf_kernel_summary_t{s[k].launches, s[k].total_ms, s[k].units};
        if (dropped) *dropped = h->impl->kernelTimers().droppedLaunches();
    });
}

int emf_fusion_get_image(emf_fusion_t* h, int which, int obj_id, emf_image_t* view) {
    REQ(h);
    REQ(view);
    EMFusion& f = *h->impl;
    auto missing = [&]() {
        std::snprintf(g_err, sizeof(g_err), "get_image: object %d is not held by this rank", obj_id);
        return EMF_E_ARG;
    };
    switch (which) {
        case EMF_IMG_POINTS: *view = f.getPoints().view(); return EMF_OK;
        case EMF_IMG_BG_ASSOC: *view = f.getBgAssociation().view(); return EMF_OK;
        case EMF_IMG_OBJ_ASSOC: {
            const auto* im = f.getObjAssociation(obj_id);
            if (!im) return missing();
            *view = im->view();
            return EMF_OK;
        }
        case EMF_IMG_ASSOC_NORM: *view = f.getAssociationNorm().view(); return EMF_OK;
        case EMF_IMG_RAYLENGTHS: *view = f.getRaylengths().view(); return EMF_OK;
        case EMF_IMG_VERTICES: *view = f.getVertices().view(); return EMF_OK;
        case EMF_IMG_NORMALS: *view = f.getNormals().view(); return EMF_OK;
        case EMF_IMG_SEGMENTATION: *view = f.getModelSegmentation().view(); return EMF_OK;
        case EMF_IMG_BG_RAYLENGTHS: *view = f.getBgRaylengths().view(); return EMF_OK;
        case EMF_IMG_OBJ_RAYLENGTHS: {
            const auto* im = f.getObjRaylengths(obj_id);
            if (!im) return missing();
            *view = im->view();
            return EMF_OK;
        }
        default:
            std::snprintf(g_err, sizeof(g_err), "get_image: unknown selector %d", which);
            return EMF_E_ARG;
    }
}

int emf_fusion_get_volume(emf_fusion_t* h, int which, int obj_id, void** dev_ptr, int32_t res[3]) {
    REQ(h);
    REQ(dev_ptr);
    REQ(res);
    EMFusion& f = *h->impl;
    TSDF* vol = obj_id == 0 ? static_cast<TSDF*>(&f.getBackground()) : f.findObject(obj_id);
    if (!vol) {
        std::snprintf(g_err, sizeof(g_err), "get_volume: object %d is not held by this rank", obj_id);
        return EMF_E_ARG;
    }
    const Vec3i r = vol->getVolumeRes();
    res[0] = r[0];
    res[1] = r[1];
    res[2] = r[2];
    ObjTSDF* obj = obj_id == 0 ? nullptr : static_cast<ObjTSDF*>(vol);
    switch (which) {
        case EMF_VOL_TSDF: *dev_ptr = const_cast<float*>(vol->tsdfPtr()); return EMF_OK;
        case EMF_VOL_WEIGHTS: *dev_ptr = const_cast<float*>(vol->weightsPtr()); return EMF_OK;
        case EMF_VOL_BRICKS:
            *dev_ptr = vol->brickFlagsPtr();
            res[0] = (r[0] + 3) / 4;
            res[1] = (r[1] + 3) / 4;
            res[2] = (r[2] + 3) / 4;
            return EMF_OK;
        case EMF_VOL_COLOR:
            if (vol->colorPtr()) {
                *dev_ptr = vol->colorPtr();
                return EMF_OK;
            }
            break;
        case EMF_VOL_FGPROBS:
            if (obj) {
                *dev_ptr = const_cast<float*>(obj->fgProbsPtr());
                return EMF_OK;
            }
            break;
        case EMF_VOL_FGBG:
            if (obj) {
                *dev_ptr = obj->fgBgPtr();
                return EMF_OK;
            }
            break;
        case EMF_VOL_FGMASK:
            if (obj) {
                *dev_ptr = const_cast<uint8_t*>(obj->fgVolMaskPtr());
                return EMF_OK;
            }
            break;
        default: break;
    }
    std::snprintf(g_err, sizeof(g_err), "get_volume: selector %d not available for id %d", which,
                  obj_id);
    return EMF_E_ARG;
}

int emf_fusion_visible_objects(emf_fusion_t* h, int32_t* ids, int cap, int* n) {
    REQ(h);
    REQ(n);
    int c = 0;
    for (int id : h->impl->visibleObjects()) {
        if (c < cap && ids) ids[c] = id;
        ++c;
    }
    *n = c < cap ? c : cap;
    return EMF_OK;
}

int emf_fusion_object_ids(emf_fusion_t* h, int32_t* ids, int cap, int* n) {
    REQ(h);
    REQ(n);
    int c = 0;
    for (int id : h->impl->objectIds()) {
        if (c < cap && ids) ids[c] = id;
        ++c;
    }
    *n = c < cap ? c : cap;
    return EMF_OK;
}

int emf_fusion_upload_host_time(emf_fusion_t* h, double* seconds, uint64_t* frames) {
    REQ(h);
    REQ(seconds);
    REQ(frames);
    return guarded([&] {
        const auto t = h->impl->uploadHostTime();
        *seconds = t.first;
        *frames = t.second;
    });
}
int emf_fusion_batched_chunks(emf_fusion_t* h) { return h ? h->impl->batchedChunks() : EMF_E_NULL; }
int emf_fusion_background_overlap(emf_fusion_t* h) { return h ? (h->impl->overlapsBackground() ? 1 : 0) : EMF_E_NULL; }

int emf_fusion_frame_index(emf_fusion_t* h) { return h ? h->impl->frameIndex() : EMF_E_NULL; }

int emf_fusion_owns_object(emf_fusion_t* h, int obj_id) {
    return h && h->impl->ownsObject(obj_id) ? 1 : 0;
}

int emf_comm_unique_id(void* out128) {
    REQ(out128);
    return guarded([&] { rcclGetUniqueId(out128); });
}

int emf_comm_create(const void* unique_id128, int rank, int world, emf_comm_t** out) {
    REQ(unique_id128);
    REQ(out);
    return guarded([&] {
        auto c = std::make_unique<emf_comm>();
        c->impl = makeRcclCommunicator(unique_id128, rank, world);
        *out = c.release();
    });
}

void emf_comm_destroy(emf_comm_t* c) { delete c; }

int emf_comm_create_host_staged(const emf_comm_callbacks_t* cb, emf_comm_t** out) {
    REQ(cb);
    REQ(out);
    return guarded([&] {
        HostStagedCallbacks h;
        h.rank = cb->rank;
        h.world = cb->world;
        h.allReduceSumF32 = cb->all_reduce_sum_f32;
        h.allReduceMinU64 = cb->all_reduce_min_u64;
        h.broadcast = cb->broadcast;
        h.user = cb->user;
        auto c = std::make_unique<emf_comm>();
        c->impl = makeHostStagedCommunicator(h);
        *out = c.release();
    });
}

int emf_comm_create_peer_local_group(int world, size_t slot_bytes, emf_comm_t** out) {
    REQ(out);
    return guarded([&] {
        auto group = makePeerCommunicatorsLocal(world, slot_bytes);
        for (int r = 0; r < world; ++r) {
            auto c = std::make_unique<emf_comm>();
            c->impl = group[r];
            out[r] = c.release();
        }
    });
}

int emf_comm_create_peer(int rank, int world, size_t slot_bytes, emf_allgather_fn all_gather, void* user,
                         emf_comm_t** out) {
    REQ(all_gather);
    REQ(out);
    return guarded([&] {
        PeerBootstrap b;
        b.rank = rank;
        b.world = world;
        b.allGather = all_gather;
        b.user = user;
        auto c = std::make_unique<emf_comm>();
        c->impl = makePeerCommunicator(b, slot_bytes);
        *out = c.release();
    });
}

int emf_comm_all_reduce_sum_f32(emf_comm_t* c, float* dev, size_t count, void* stream) {
    REQ(c);
    return guarded([&] {
        Stream s(static_cast<hipStream_t>(stream));
        c->impl->allReduceSumF32(dev, count, s);
    });
}
int emf_comm_all_reduce_min_u64(emf_comm_t* c, uint64_t* dev, size_t count, void* stream) {
    REQ(c);
    return guarded([&] {
        Stream s(static_cast<hipStream_t>(stream));
        c->impl->allReduceMinU64(dev, count, s);
    });
}
int emf_comm_broadcast(emf_comm_t* c, void* dev, size_t bytes, int root, void* stream) {
    REQ(c);
    return guarded([&] {
        Stream s(static_cast<hipStream_t>(stream));
        c->impl->broadcast(dev, bytes, root, s);
    });
}
int emf_comm_gather_row_bands(emf_comm_t* c, void* dev, size_t bytes_per_row, int band_rows, int total_rows,
                              void* stream) {
    REQ(c);
    return guarded([&] {
        Stream s(static_cast<hipStream_t>(stream));
        c->impl->gatherRowBands(dev, bytes_per_row, band_rows, total_rows, s);
    });
}

int emf_comm_create_delayed(emf_comm_t* inner, int microseconds, emf_comm_t** out) {
    REQ(inner);
    REQ(out);
    return guarded([&] {
        auto c = std::make_unique<emf_comm>();
        c->impl = makeDelayedCommunicator(inner->impl, microseconds);
        *out = c.release();
    });
}

int emf_comm_describe(emf_comm_t* c, char* json, size_t cap) {
    REQ(c);
    REQ(json);
    return guarded([&] {
        const std::string s = c->impl->describe();
        if (s.size() + 1 > cap) throw HipError("emf_comm_describe: buffer too small", EMF_E_ARG);
        std::memcpy(json, s.c_str(), s.size() + 1);
    });
}

int emf_comm_exchanges(emf_comm_t* c, uint64_t* out) {
    REQ(c);
    REQ(out);
    return guarded([&] { *out = c->impl->exchangesIssued(); });
}

int emf_comm_create_local_group(int world, emf_comm_t** out) {
    REQ(out);
    return guarded([&] {
        auto group = makeLocalCommunicators(world);
        for (int r = 0; r < world; ++r) {
            auto c = std::make_unique<emf_comm>();
            c->impl = group[r];
            out[r] = c.release();
        }
    });
}

int emf_synth_create(int width, int height, const float K[9], int num_spheres, uint64_t seed,
                     float noise_sigma, float dropout, emf_synth_t** out) {
    REQ(K);
    REQ(out);
    return guarded([&] {
        auto s = std::make_unique<emf_synth>();
        s->impl = std::make_unique<SyntheticScene>(Size(width, height), m33(K), num_spheres, seed,
                                                   noise_sigma, dropout);
        *out = s.release();
    });
}

void emf_synth_destroy(emf_synth_t* s) { delete s; }

int emf_synth_render(emf_synth_t* s, int frame, float* depth, uint8_t* ids) {
    REQ(s);
    REQ(depth);
    return guarded([&] { s->impl->render(frame, depth, ids); });
}

int emf_synth_camera_pose(emf_synth_t* s, int frame, float R[9], float t[3]) {
    REQ(s);
    REQ(R);
    REQ(t);
    const Affine3f p = s->impl->cameraPose(frame);
    std::memcpy(R, p.rotation().val, 9 * sizeof(float));
    std::memcpy(t, p.translation().val, 3 * sizeof(float));
    return EMF_OK;
}

int emf_synth_sphere(emf_synth_t* s, int k, int frame, float center[3], float* radius,
                     float* volume_size) {
    REQ(s);
    if (k < 0 || k >= s->impl->numSpheres()) {
        std::snprintf(g_err, sizeof(g_err), "emf_synth_sphere: index %d out of range", k);
        return EMF_E_ARG;
    }
    const Vec3f c = s->impl->sphereCenter(k, frame);
    if (center) std::memcpy(center, c.val, 3 * sizeof(float));
    if (radius) *radius = s->impl->sphere(k).radius;
    if (volume_size) *volume_size = s->impl->objectVolumeSize(k);
    return EMF_OK;
}

}  // extern "C"
