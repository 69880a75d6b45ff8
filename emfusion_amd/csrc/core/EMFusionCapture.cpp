// EMFusionCapture.cpp -- emf::EMFusion: results and debug captures (reference src/core/EMFusion.cpp:131-160, 243-327, 991-1236).
#include "EMFusion.hpp"
#include "EMFusionDetail.hpp"
#include "Output.hpp"

#include <sys/stat.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace emf {

using namespace detail;

void EMFusion::writeResults(const std::string& dir, bool volumes) {
    synchronize();
    // boost::filesystem::create_directories(p) (EMFusion.cpp:254-255): every missing component of the path
    for (size_t k = 1; k <= dir.size(); ++k)
        if (k == dir.size() || dir[k] == '/') {
            const std::string part = dir.substr(0, k);
            if (!part.empty() && mkdir(part.c_str(), 0777) != 0 && errno != EEXIST)
                throw std::runtime_error("EMFusion::writeResults: cannot create " + part);
        }
    io::writePoseFile(dir + "/poses-cam.txt", poses);
    for (const auto& op : obj_poses)
        io::writePoseFile(dir + "/poses-" + std::to_string(op.first) + ".txt", op.second);
    for (const auto& op : addPoseOffsets(obj_poses, obj_pose_offsets))  // EMFusion.cpp:1000-1006
        io::writePoseFile(dir + "/poses-" + std::to_string(op.first) + "-corrected.txt", op.second);
    // writeMeshes (EMFusion.cpp:1147-1156) runs whether or not volumes are exported: the background,
    // the live objects, and the objects that were deleted while the log was on (their last mesh,
    // EMFusion.cpp:966)
    std::vector<int> ids{0};
    for (const auto& obj : objects)
        if (!(ignorePerson && isPerson(obj))) ids.push_back(obj.getID());
    std::vector<Mesh> live = extractMeshes(ids);  // one pass over the table, the bytes getMesh() gives
    io::writeMesh(dir + "/mesh_bg.ply", live[0]);
    for (size_t k = 1; k < ids.size(); ++k) meshes[ids[k]] = std::move(live[k]);
    for (const auto& m : meshes) io::writeMesh(dir + "/mesh_" + std::to_string(m.first) + ".ply", m.second);
    if (expWorldMesh_) io::writeMesh(dir + "/world.ply", worldMesh());  // one mesh of the volume and the store (5.16)
    if (expDistance_) writeDistanceField(dir);  // distance.bin + occupancy.bin of the whole background (5.18)
    if (expFrontiers_) writeFrontiers(dir);     // frontiers.txt of the whole background (5.19)
    if (expPlan_) writePlan(dir);               // plan.txt of the whole background from the camera (5.20)
    if (expShapes_) writeShapes(dir);           // shapes.txt of the live objects (5.23)
    if (expGround_.on) writeGround(dir);        // ground.bin + ground.txt of the whole background (5.24)
    if (expPlanes_.on) writePlanes(dir);        // planes.txt of the whole background (5.25)
    if (expContacts_) writeContacts(dir);       // contacts.txt of the live objects and the background (5.27)
    if (expAbsorbed_) writeAbsorbed(dir);       // absorbed.txt, the session's log of absorbed objects (5.29)
    if (expLifted_) writeLifted(dir);           // lifted.txt, the session's log of lifted objects (5.30)
    if (expMerged_) writeMerged(dir);           // merged.txt, the session's log of merged objects (5.32)
    if (expFrameMeshes_) {  // writeFrameMeshes (EMFusion.cpp:1158-1185); the reference creates frame_meshes/ always
        auto writeAll = [](const std::string& d, const std::map<int, Mesh>& log) {
            io::createDirectories(d);
            char name[32];
            for (const auto& fm : log) {
                std::snprintf(name, sizeof(name), "/%04d.ply", fm.first);
                io::writeMesh(d + name, fm.second);
            }
        };
        writeAll(dir + "/frame_meshes/bg", frame_meshes);
        for (const auto& o : frame_obj_meshes) writeAll(dir + "/frame_meshes/" + std::to_string(o.first), o.second);
    }
    if (!retired.empty()) {  // what the rolls removed (setBackgroundFollow / rollBackground), in the frame of the INITIAL pose
        const std::string d = dir + "/bg_retired";
        io::createDirectories(d);
        const Vec3i n = background.getVolumeRes();
        const double vox = static_cast<double>(background.getVoxelSize());
        std::FILE* f = std::fopen((d + "/origins.txt").c_str(), "w");
        if (!f) throw std::runtime_error("EMFusion::writeResults: cannot create " + d + "/origins.txt");
        char name[32];
        for (size_t k = 0; k < retired.size(); ++k) {
            const RetiredSlab& r = retired[k];
            Mesh m = r.mesh;
            for (int i = 0; i < 3; ++i) {  // the sub-box's centre on the lattice, from the initial volume's centre
                const double off = (static_cast<double>(r.origin[i]) + (r.res[i] - 1) / 2.0 - (n[i] - 1) / 2.0) * vox;
                for (size_t v = 0; v < m.vertices(); ++v)
                    m.cloud[3 * v + i] = static_cast<float>(static_cast<double>(m.cloud[3 * v + i]) + off);
            }
            std::snprintf(name, sizeof(name), "/%04d.ply", static_cast<int>(k));
            io::writeMesh(d + name, m);
            std::fprintf(f, "%d %d %d %d %d %d %d\n", r.frame, r.origin[0], r.origin[1], r.origin[2], r.res[0], r.res[1], r.res[2]);
        }
        std::fclose(f);
    }
    // writeRenderings / writeAssocs / writeHuberWeights / writeTrackWeights / writeFgProbs (EMFusion.cpp:1009-1145):
    // directories are created whether or not the log holds anything, like the reference's
    io::writeImageLog(dir + "/output", renderings);
    if (view3d || !meshVis.empty()) io::writeImageLog(dir + "/mesh_vis_out", meshVis);  // writeMeshVis, EMFusion.cpp:1018-1025
    io::writeImageLog(dir + "/assoc_weights/bg/preTrack", bg_assocWeight_preTrack);
    io::writeImageLog(dir + "/assoc_weights/bg/postTrack", bg_assocWeight_postTrack);
    for (const auto& o : obj_assocWeights_preTrack)
        io::writeImageLog(dir + "/assoc_weights/" + std::to_string(o.first) + "/preTrack", o.second);
    for (const auto& o : obj_assocWeights_postTrack)
        io::writeImageLog(dir + "/assoc_weights/" + std::to_string(o.first) + "/postTrack", o.second);
    io::writeImageLog(dir + "/huber_weights/bg", bg_huberWeights);
    for (const auto& o : obj_huberWeights) io::writeImageLog(dir + "/huber_weights/" + std::to_string(o.first), o.second);
    io::writeImageLog(dir + "/track_weights/bg", bg_trackWeights);
    for (const auto& o : obj_trackWeights) io::writeImageLog(dir + "/track_weights/" + std::to_string(o.first), o.second);
    io::createDirectories(dir + "/fg_probs");
    for (const auto& o : obj_fgProbs) io::writeImageLog(dir + "/fg_probs/" + std::to_string(o.first), o.second);
    if (!(volumes || expVols)) return;  // `if ( expVols ) writeTSDFs ( p )` (EMFusion.cpp:290-291)
    const std::string t = dir + "/tsdfs";
    if (mkdir(t.c_str(), 0777) != 0 && errno != EEXIST)
        throw std::runtime_error("EMFusion::writeResults: cannot create " + t);
    auto dump = [&](const std::string& name, const std::vector<float>& v, const Vec3i& res, float vox) {
        io::writeVolume(t + "/" + name + ".bin", v.data(), sizeof(float), res, vox);
    };
    dump("bg_tsdf", background.getTSDF(), background.getVolumeRes(), background.getVoxelSize());
    // colour on only: one colour volume per model in the same container, element = u16 x 4 (R, G, B, Wc in 8.8)
    auto dumpColor = [&](const std::string& name, const std::vector<uint16_t>& v, const Vec3i& res, float vox) {
        if (!v.empty()) io::writeVolume(t + "/" + name + ".bin", v.data(), 4 * sizeof(uint16_t), res, vox);
    };
    dumpColor("bg_color", background.getColorVol(), background.getVolumeRes(), background.getVoxelSize());
    for (auto& obj : objects) {
        if (ignorePerson && isPerson(obj)) continue;  // the same `continue` skips them (EMFusion.cpp:274-277)
        savedVolumes[obj.getID()] = saveVolumes(obj);
    }
    for (const auto& sv : savedVolumes) {  // writeTSDFs (EMFusion.cpp:1195-1216): live and deleted objects
        const std::string id = std::to_string(sv.first);
        dump("tsdf_" + id, sv.second.tsdf, sv.second.res, sv.second.voxelSize);
        dump("weights_" + id, sv.second.weights, sv.second.res, sv.second.voxelSize);
        dump("fgProbs_" + id, sv.second.fgProbs, sv.second.res, sv.second.voxelSize);
        dumpColor("color_" + id, sv.second.color, sv.second.res, sv.second.voxelSize);
    }
}

EMFusion::SavedVolumes EMFusion::saveVolumes(ObjTSDF& obj) {  // EMFusion.cpp:279-285, 967-973
    SavedVolumes sv;
    sv.tsdf = obj.getTSDF();
    sv.weights = obj.getWeightsVol();
    sv.fgProbs = obj.getFgProbVol();
    sv.color = obj.getColorVol();
    sv.res = obj.getVolumeRes();
    sv.voxelSize = obj.getVoxelSize();
    return sv;
}

// Reference EMFusion::addPoseOffsets (EMFusion.cpp:1220-1236): undo the accumulated centre shifts so
// that the trajectory refers to the volume centre the object was created with.
std::map<int, std::map<int, Affine3f>> EMFusion::addPoseOffsets(
    const std::map<int, std::map<int, Affine3f>>& all,
    const std::map<int, std::map<int, Vec3f>>& offsets) {
    std::map<int, std::map<int, Affine3f>> cleaned;
    for (const auto& op : all) {
        Vec3f cum = Vec3f::all(0.f);
        const auto off = offsets.find(op.first);
        for (const auto& fp : op.second) {
            if (off != offsets.end()) {
                const auto o = off->second.find(fp.first);
                if (o != off->second.end()) cum = cum - o->second;
            }
            cleaned[op.first][fp.first] = fp.second.translate(fp.second.rotation() * cum);
        }
    }
    return cleaned;
}

void EMFusion::render(uint8_t* rgb) {
    if (sharded)
        throw HipError("EMFusion::render: not available on the sharded path (vertices / normals of "
                       "remote objects and background bands stay on their ranks)", EMF_E_ARG);
    const size_t bytes = static_cast<size_t>(params.frameSize.area()) * 3;
    if (frameCount < 1) {
        std::fill(rgb, rgb + bytes, uint8_t{0});
        return;
    }
    if (frameCount == 1) raycast();  // frame 0 ran without one (EMFusion.cpp:135-137)
    if (image.empty()) image = DeviceImage<uint8_t, 3>(params.frameSize);
    const emf_image_t vv = vertices.view(), nv = normals.view(), sv = modelSegmentation.view(),
                      iv = image.view();
    if (ignorePerson) {  // EMFusion.cpp:139-150: in place, like the reference
        const emf_image_t bv = bg_vertices.view(), bn = bg_normals.view();
        for (const auto& obj : objects)
            if (isPerson(obj))
                emfCheck(emf_hip_hideLabel(&sv, obj.getID(), &vv, &nv, &bv, &bn, main.abi()), "hideLabel");
    }
    const float light[3] = {0.f, 0.f, 0.f};  // cv::Affine3f::Identity()
    emfCheck(emf_hip_renderPhong(&vv, &nv, &sv, colorMap.data(), light, &iv, main.abi()), "renderPhong");
    hipCheck(hipMemcpyAsync(rgb, image.ptr(), bytes, hipMemcpyDeviceToHost, main.get()), "render D2H");
    main.waitForCompletion();
    if (saveOutput)  // `rendered.copyTo ( renderings[frameCount-1] )`, EMFusion.cpp:158-160
        renderings[frameCount - 1] = io::encodePng(rgb, params.frameSize.width, params.frameSize.height, 3);
    render3dView();  // the viz window's view (EMFusion.cpp:162-231), when set3dView turned it on
}

// ---- per-frame debug images (reference saveOutput mode) ---------------------------------------------------

std::vector<uint8_t> EMFusion::pngOf(const float* dev, size_t pitchBytes) {
    const int w = params.frameSize.width, h = params.frameSize.height;
    std::vector<float> host(static_cast<size_t>(w) * h);
    hipCheck(hipMemcpy2DAsync(host.data(), static_cast<size_t>(w) * sizeof(float), dev, pitchBytes,
                              static_cast<size_t>(w) * sizeof(float), static_cast<size_t>(h), hipMemcpyDeviceToHost,
                              main.get()),
             "hipMemcpy2DAsync(debug image)");
    main.waitForCompletion();
    const std::vector<uint8_t> u8 = io::toU8Times255(host.data(), w, h, static_cast<size_t>(w));
    return io::encodePng(u8.data(), w, h, 1);
}

void EMFusion::storeAssocs(ImageLog& bg, std::map<int, ImageLog>& objs) {
    if (sharded) return;  // (remote objects' maps are not on this rank; the reference is single-GPU)
    const emf_image_t b = bg_associationWeights.view();
    bg[frameCount] = pngOf(static_cast<const float*>(b.data), b.pitch);
    for (const auto& obj : objects) {
        const emf_image_t a = objImages.at(obj.getID()).associationWeights.view();
        objs[obj.getID()][frameCount] = pngOf(static_cast<const float*>(a.data), a.pitch);
    }
}

void EMFusion::storeTrackWeights(int first, int count) {
    if (count <= 0 || trackStates.empty()) return;
    const int w = params.frameSize.width, h = params.frameSize.height;
    const size_t px = static_cast<size_t>(w) * h, per = emf_hip_trackScratchBytes(w, h);
    if (logScratch.bytes() < 2 * px * sizeof(float) * count) logScratch = DeviceBuffer(2 * px * sizeof(float) * count);
    emf_track_params_t tp;
    tp.huberThresh = params.tsdfParams.huberThresh;
    tp.maxWeight = params.tsdfParams.maxTSDFWeight;
    tp.tau = params.tsdfParams.tau;
    tp.eps1 = params.tsdfParams.eps1;
    tp.eps2 = params.tsdfParams.eps2;
    tp.nuInit = params.tsdfParams.nu_init;
    const emf_image_t pv = points.view();
    float* huber = logScratch.as<float>();
    float* track = huber + px * count;
    // the stage's states are final and the models' association maps are still the ones it tracked with
    forChunks(first, first + count, [&](int from, int cnt) {  // (a stage of more than EMF_MAX_BATCH models ran chunk by chunk too)
        emfCheck(emf_hip_trackWeightImages(currentTable() + from, trackStates.as<emf_track_state_t>() + from, cnt, &pv, &tp,
                                           static_cast<const char*>(trackScratch.data()) + per * from, per,
                                           huber + px * (from - first), track + px * (from - first), main.abi()),
                 "trackWeightImages");
    });
    auto it = objects.begin();
    for (int m = 0; m < count; ++m) {
        const std::vector<uint8_t> hp = pngOf(huber + px * m, static_cast<size_t>(w) * sizeof(float));
        const std::vector<uint8_t> tpng = pngOf(track + px * m, static_cast<size_t>(w) * sizeof(float));
        if (first + m == 0) {
            bg_huberWeights[frameCount] = hp;
            bg_trackWeights[frameCount] = tpng;
        } else {
            const int id = (it++)->getID();
            obj_huberWeights[id][frameCount] = hp;
            obj_trackWeights[id][frameCount] = tpng;
        }
    }
}

void EMFusion::storeFgProbs() {
    if (sharded || objects.empty()) return;
    const int w = params.frameSize.width, h = params.frameSize.height;
    const size_t px = static_cast<size_t>(w) * h;
    if (logScratch.bytes() < px * sizeof(float)) logScratch = DeviceBuffer(px * sizeof(float));
    const emf_image_t pv = points.view();
    const emf_image_t out{logScratch.data(), static_cast<size_t>(w) * sizeof(float), w, h};
    for (auto& obj : objects) {
        // cuda::TSDF::getVolumeVals ( fgProbs, points, rel_pose_CO ... fgProbVals ), ObjTSDF.cpp:189-191
        const Affine3f co = obj.getPose().inv() * pose;
        const Vec3i res = obj.getVolumeRes();
        const int32_t r[3] = {res[0], res[1], res[2]};
        emfCheck(emf_hip_getVolumeVals(obj.fgProbsPtr(), 1, &pv, co.rotation().val, co.translation().val, r,
                                       obj.getVoxelSize(), &out, main.abi()),
                 "getVolumeVals(fgProbs)");
        obj_fgProbs[obj.getID()][frameCount] = pngOf(logScratch.as<float>(), out.pitch);
    }
}

// ---- meshes of many models at once (emf_hip_meshCountBatched / emf_hip_meshEmitBatched) --------------------

std::vector<Mesh> EMFusion::extractMeshes(const std::vector<int>& ids) {
    const int n = static_cast<int>(ids.size());
    std::vector<Mesh> out(ids.size());
    for (Mesh& m : out) m.colored = colorOn;
    meshFilterStats.clear();
    meshSimplifyStats.clear();
    if (n == 0) return out;
    if (n > EMF_MAX_MODELS) throw HipError("EMFusion::extractMeshes: " + std::to_string(n) + " models", EMF_E_LIMIT);
    if (meshHost.empty())
        meshHost = PinnedBuffer(EMF_MAX_MODELS * sizeof(emf_model_t) + EMF_MAX_MODELS * sizeof(emf_mesh_counts_t) +
                                2 * (EMF_MAX_MODELS + 1) * sizeof(uint64_t));
    emf_model_t* table = meshHost.as<emf_model_t>();
    auto* counts = reinterpret_cast<emf_mesh_counts_t*>(table + EMF_MAX_MODELS);
    auto* bases = reinterpret_cast<uint64_t*>(counts + EMF_MAX_MODELS);
    std::vector<int32_t> res(3 * ids.size());
    for (int k = 0; k < n; ++k) {  // the volumes' current copies (describe() follows the background's flips)
        const int id = ids[k];
        emf_model_t& m = table[k];
        m = emf_model_t{};
        if (id == 0) {
            background.describe(m);
        } else {
            const ObjTSDF* obj = getObject(id);
            if (!obj) throw HipError("EMFusion::extractMeshes: no object " + std::to_string(id) + " on this rank", EMF_E_ARG);
            obj->describe(m);
        }
        std::copy(m.res, m.res + 3, res.begin() + 3 * k);
    }
    // ordered after every write of the last frame, as renderView is
    if (bgInFlight) joinBackground();
    main.waitFor(aux);
    for (auto& kv : streams) main.waitFor(kv.second);
    if (meshTableDev.empty()) meshTableDev = DeviceBuffer(EMF_MAX_MODELS * sizeof(emf_model_t));
    if (meshCountsDev.empty())
        meshCountsDev = DeviceBuffer(EMF_MAX_MODELS * sizeof(emf_mesh_counts_t) + 2 * (EMF_MAX_MODELS + 1) * sizeof(uint64_t));
    const size_t scratchBytes = emf_hip_meshScratchBytesBatched(res.data(), n);
    if (scratchBytes == 0) throw HipError("EMFusion::extractMeshes: bad volume resolution", EMF_E_SHAPE);
    if (meshScratch.bytes() < scratchBytes) meshScratch = DeviceBuffer(scratchBytes);
    hipCheck(hipMemcpyAsync(meshTableDev.data(), table, n * sizeof(emf_model_t), hipMemcpyHostToDevice, main.get()),
             "mesh table upload");
    auto* countsDev = meshCountsDev.as<emf_mesh_counts_t>();
    auto* basesDev = reinterpret_cast<uint64_t*>(countsDev + EMF_MAX_MODELS);
    emfCheck(emf_hip_meshCountBatched(meshTableDev.as<emf_model_t>(), res.data(), n, meshScratch.data(), countsDev, basesDev,
                                      main.abi()),
             "meshCountBatched");
    hipCheck(hipMemcpyAsync(counts, countsDev, meshCountsDev.bytes(), hipMemcpyDeviceToHost, main.get()), "mesh counts D2H");
    main.waitForCompletion();  // the one wait before the emit: the outputs' sizes
    const uint64_t nv = bases[2 * n], nt = bases[2 * n + 1];
    if (nv == 0) {  // nothing to mesh: the filter met nothing
        if (meshFilterActive())
            for (int id : ids) meshFilterStats[id] = MeshFilterStats{};
        if (meshSimplifyActive())
            for (int id : ids) meshSimplifyStats[id] = MeshSimplifyStats{};
        return out;
    }
    const size_t vb = 3 * sizeof(float) * nv, tb = 4 * sizeof(int32_t) * std::max<uint64_t>(nt, 1);
    if (meshArena.bytes() < 2 * vb + tb) meshArena = DeviceBuffer(2 * vb + tb);
    float* vDev = meshArena.as<float>();
    float* nDev = vDev + 3 * nv;
    int32_t* tDev = reinterpret_cast<int32_t*>(nDev + 3 * nv);
    emfCheck(emf_hip_meshEmitBatched(meshTableDev.as<emf_model_t>(), res.data(), n, meshScratch.data(), vDev, nDev, tDev,
                                     main.abi()),
             "meshEmitBatched");
    if (meshWeld || meshFilterActive() || meshSimplifyActive()) {  // the welded form of the same soup: welded (filtered,
                                                                   // simplified) on the device
        extractWelded(ids, res, nv, nt, out);
        return out;
    }
    DeviceBuffer cDev;
    if (colorOn) meshColors(ids, res, nv, cDev);
    std::vector<MeshSlice> slices(n);
    for (int k = 0; k < n; ++k) slices[k] = MeshSlice{bases[2 * k], counts[k].vertices, bases[2 * k + 1], counts[k].triangles};
    meshPost.download(main, DeviceMesh{vDev, nDev, tDev, colorOn ? cDev.as<uint8_t>() : nullptr, nv, nt}, slices, out.data());
    return out;
}

// the soup's vertices coloured: one more walk over the surface chunks the count listed, enqueued on main
void EMFusion::meshColors(const std::vector<int>& ids, const std::vector<int32_t>& res, uint64_t nv, DeviceBuffer& cDev) {
    const int n = static_cast<int>(ids.size());
    std::vector<uint16_t*> ptrs(n, nullptr);
    for (int k = 0; k < n; ++k) ptrs[k] = ids[k] == 0 ? background.colorPtr() : getObject(ids[k])->colorPtr();
    meshColorPtrsDev.reserve(sizeof(uint16_t*) * EMF_MAX_MODELS);  // (a member: the kernel reads it after this returns)
    cDev = DeviceBuffer(3 * nv);
    hipCheck(hipMemcpyAsync(meshColorPtrsDev.data(), ptrs.data(), sizeof(uint16_t*) * n, hipMemcpyHostToDevice, main.get()),
             "mesh colour table upload");
    emfCheck(emf_hip_meshColorsBatched(meshTableDev.as<emf_model_t>(), meshColorPtrsDev.as<uint16_t*>(), res.data(), n,
                                       meshScratch.data(), cDev.as<uint8_t>(), main.abi()),
             "meshColorsBatched");
}

// extractMeshes' tail with setMeshWeld(true) (include/emf_hip.h "Welded meshes").  The soup of the n models lies in
// meshArena ([vertices][normals][triangles], as the emit wrote it) and the counting scratch is still valid: colours and
// edge keys walk the surface chunks once more, and the chain of MeshPost.hpp welds on the keys, filters by component
// with setMeshFilter and clusters by cell with setMeshSimplify; what is left is what travels.
void EMFusion::extractWelded(const std::vector<int>& ids, const std::vector<int32_t>& res, uint64_t nv, uint64_t nt,
                             std::vector<Mesh>& out) {
    const int n = static_cast<int>(ids.size());
    auto* counts = reinterpret_cast<emf_mesh_counts_t*>(meshHost.as<emf_model_t>() + EMF_MAX_MODELS);
    auto* bases = reinterpret_cast<uint64_t*>(counts + EMF_MAX_MODELS);
    auto* basesDev = reinterpret_cast<uint64_t*>(meshCountsDev.as<emf_mesh_counts_t>() + EMF_MAX_MODELS);
    float* vDev = meshArena.as<float>();
    float* nDev = vDev + 3 * nv;
    int32_t* tDev = reinterpret_cast<int32_t*>(nDev + 3 * nv);
    DeviceBuffer cDev;
    if (colorOn) meshColors(ids, res, nv, cDev);
    meshKeysDev.reserve(sizeof(uint64_t) * nv);
    emfCheck(emf_hip_meshEdgeKeysBatched(meshTableDev.as<emf_model_t>(), res.data(), n, meshScratch.data(),
                                         meshKeysDev.as<uint64_t>(), main.abi()),
             "meshEdgeKeysBatched");
    std::vector<MeshFilter> filters(n);
    for (int k = 0; k < n; ++k) filters[k] = meshFilterFor(ids[k]);
    MeshPost::Request req;
    req.filter = meshFilterActive();
    req.simplify = meshSimplifyActive();
    req.perModel = filters.data();
    const MeshPost::Result r = meshPost.run(
        main, MeshPost::Soup{vDev, nDev, tDev, colorOn ? cDev.as<uint8_t>() : nullptr, meshKeysDev.as<uint64_t>(), nv, nt},
        MeshPost::Table{n, basesDev, bases}, req, "EMFusion::extractMeshes");
    for (int k = 0; k < n; ++k) {
        if (req.filter) meshFilterStats[ids[k]] = r.filterStats[k];
        if (req.simplify) meshSimplifyStats[ids[k]] = r.simplifyStats[k];
    }
    meshPost.download(main, r.mesh, r.slices, out.data());
}

// EMFusion.cpp:110-125 (exp_frame_meshes): the background and every live object not hidden by ignore_person, meshed
// from the current table at the end of the frame and kept under the frame's number
void EMFusion::storeFrameMeshes() {
    std::vector<int> ids{0};
    for (const auto& obj : objects)
        if (!(ignorePerson && isPerson(obj))) ids.push_back(obj.getID());
    std::vector<Mesh> all = extractMeshes(ids);
    frame_meshes[frameCount] = std::move(all[0]);
    for (size_t k = 1; k < ids.size(); ++k) frame_obj_meshes[ids[k]][frameCount] = std::move(all[k]);
}

Mesh EMFusion::getMesh(int id) {
    synchronize();
    meshFilterStats.clear();
    meshSimplifyStats.clear();
    TSDF* model = id == 0 ? &background : nullptr;
    for (auto& o : objects)
        if (o.getID() == id) model = &o;
    if (!model) throw HipError("EMFusion::getMesh: no object " + std::to_string(id) + " on this rank", EMF_E_ARG);
    if (meshFilterActive() || meshSimplifyActive()) {
        MeshFilterStats stats;
        Mesh m = model->getFilteredMesh(meshFilterFor(id), &stats);
        if (meshFilterActive()) meshFilterStats[id] = stats;
        if (meshSimplifyActive()) meshSimplifyStats[id] = stats.simplify;
        return m;
    }
    return meshWeld ? model->getWeldedMesh() : model->getMesh();
}

MeshComponents EMFusion::getMeshComponents(int id) {
    synchronize();
    if (id == 0) return background.getMeshComponents();
    for (auto& o : objects)
        if (o.getID() == id) return o.getMeshComponents();
    throw HipError("EMFusion::getMeshComponents: no object " + std::to_string(id) + " on this rank", EMF_E_ARG);
}

}  // namespace emf
