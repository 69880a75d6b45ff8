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
    meshStage.grow(2 * vb + tb);
    float* vHost = meshStage.as<float>();
    float* nHost = vHost + 3 * nv;
    int32_t* tHost = reinterpret_cast<int32_t*>(nHost + 3 * nv);
    hipCheck(hipMemcpyAsync(vHost, vDev, vb, hipMemcpyDeviceToHost, main.get()), "mesh vertices D2H");
    hipCheck(hipMemcpyAsync(nHost, nDev, vb, hipMemcpyDeviceToHost, main.get()), "mesh normals D2H");
    if (nt) hipCheck(hipMemcpyAsync(tHost, tDev, 4 * sizeof(int32_t) * nt, hipMemcpyDeviceToHost, main.get()), "mesh triangles D2H");
    main.waitForCompletion();
    std::vector<uint8_t> cHost;
    if (colorOn) {  // the same vertices, coloured: one more walk over the surface chunks the count listed
        std::vector<uint16_t*> ptrs(n, nullptr);
        for (int k = 0; k < n; ++k) ptrs[k] = ids[k] == 0 ? background.colorPtr() : getObject(ids[k])->colorPtr();
        DeviceBuffer ptrsDev(sizeof(uint16_t*) * n), cDev(3 * nv);
        hipCheck(hipMemcpyAsync(ptrsDev.data(), ptrs.data(), sizeof(uint16_t*) * n, hipMemcpyHostToDevice, main.get()),
                 "mesh colour table upload");
        emfCheck(emf_hip_meshColorsBatched(meshTableDev.as<emf_model_t>(), ptrsDev.as<uint16_t*>(), res.data(), n,
                                           meshScratch.data(), cDev.as<uint8_t>(), main.abi()),
                 "meshColorsBatched");
        cHost.resize(3 * nv);
        hipCheck(hipMemcpyAsync(cHost.data(), cDev.data(), 3 * nv, hipMemcpyDeviceToHost, main.get()), "mesh colours D2H");
        main.waitForCompletion();
    }
    for (int k = 0; k < n; ++k) {  // model k's slice is its own mesh (local triangle indices)
        const size_t v0 = bases[2 * k], t0 = bases[2 * k + 1];
        Mesh& m = out[k];
        m.cloud.assign(vHost + 3 * v0, vHost + 3 * (v0 + counts[k].vertices));
        m.normals.assign(nHost + 3 * v0, nHost + 3 * (v0 + counts[k].vertices));
        m.polygons.assign(tHost + 4 * t0, tHost + 4 * (t0 + counts[k].triangles));
        if (!cHost.empty()) m.colors.assign(cHost.begin() + 3 * v0, cHost.begin() + 3 * (v0 + counts[k].vertices));
    }
    return out;
}

// extractMeshes' tail with setMeshWeld(true) (include/emf_hip.h "Welded meshes").  The soup of the n models lies in
// meshArena ([vertices][normals][triangles], as the emit wrote it) and the counting scratch is still valid: colours and
// edge keys walk the surface chunks once more, the weld runs on the keys, and the welded vertex arrays land behind the
// soup in the same arena (grown when needed; the soup is copied over, it is a quarter of what a frame's soup D2H was).
// With setMeshFilter the components are labelled, filtered and compacted behind the weld (include/emf_hip.h "Mesh
// components") and the kept arrays are what travels; with setMeshSimplify those are clustered by cell behind the filter
// (include/emf_hip.h "Simplified meshes") and the simplified arrays travel instead.
void EMFusion::extractWelded(const std::vector<int>& ids, const std::vector<int32_t>& res, uint64_t nv, uint64_t nt,
                             std::vector<Mesh>& out) {
    const int n = static_cast<int>(ids.size());
    auto* counts = reinterpret_cast<emf_mesh_counts_t*>(meshHost.as<emf_model_t>() + EMF_MAX_MODELS);
    auto* bases = reinterpret_cast<uint64_t*>(counts + EMF_MAX_MODELS);
    auto* basesDev = reinterpret_cast<uint64_t*>(meshCountsDev.as<emf_mesh_counts_t>() + EMF_MAX_MODELS);
    const size_t vb = 3 * sizeof(float) * nv, tb = 4 * sizeof(int32_t) * std::max<uint64_t>(nt, 1);
    const size_t weldBytes = emf_hip_meshWeldScratchBytes(nv);
    if (weldBytes == 0) throw HipError("EMFusion::extractMeshes: " + std::to_string(nv) + " soup vertices", EMF_E_LIMIT);
    // [keys u64 x nv][welded counts u32 x MAX][welded bases u64 x (MAX + 1)][weld scratch]
    const size_t keyBytes = sizeof(uint64_t) * nv, cntBytes = sizeof(uint32_t) * EMF_MAX_MODELS,
                 baseBytes = sizeof(uint64_t) * (EMF_MAX_MODELS + 1);
    if (meshWeldScratch.bytes() < keyBytes + cntBytes + baseBytes + weldBytes)
        meshWeldScratch = DeviceBuffer(keyBytes + cntBytes + baseBytes + weldBytes);
    auto* keysDev = meshWeldScratch.as<uint64_t>();
    auto* wBasesDev = keysDev + nv;
    auto* wCountsDev = reinterpret_cast<uint32_t*>(wBasesDev + EMF_MAX_MODELS + 1);
    void* weldScratch = reinterpret_cast<char*>(meshWeldScratch.data()) + keyBytes + baseBytes + cntBytes;
    float* vDev = meshArena.as<float>();
    float* nDev = vDev + 3 * nv;
    int32_t* tDev = reinterpret_cast<int32_t*>(nDev + 3 * nv);
    DeviceBuffer ptrsDev, cDev, wcDev;
    if (colorOn) {
        std::vector<uint16_t*> ptrs(n, nullptr);
        for (int k = 0; k < n; ++k) ptrs[k] = ids[k] == 0 ? background.colorPtr() : getObject(ids[k])->colorPtr();
        ptrsDev = DeviceBuffer(sizeof(uint16_t*) * n);
        cDev = DeviceBuffer(3 * nv);
        hipCheck(hipMemcpyAsync(ptrsDev.data(), ptrs.data(), sizeof(uint16_t*) * n, hipMemcpyHostToDevice, main.get()),
                 "mesh colour table upload");
        emfCheck(emf_hip_meshColorsBatched(meshTableDev.as<emf_model_t>(), ptrsDev.as<uint16_t*>(), res.data(), n,
                                           meshScratch.data(), cDev.as<uint8_t>(), main.abi()),
                 "meshColorsBatched");
    }
    emfCheck(emf_hip_meshEdgeKeysBatched(meshTableDev.as<emf_model_t>(), res.data(), n, meshScratch.data(), keysDev,
                                         main.abi()),
             "meshEdgeKeysBatched");
    emfCheck(emf_hip_meshWeldCountBatched(keysDev, nv, basesDev, n, weldScratch, wCountsDev, wBasesDev, main.abi()),
             "meshWeldCountBatched");
    std::vector<uint32_t> wCounts(n);
    std::vector<uint64_t> wBases(n + 1);
    hipCheck(hipMemcpyAsync(wCounts.data(), wCountsDev, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, main.get()),
             "welded counts D2H");
    hipCheck(hipMemcpyAsync(wBases.data(), wBasesDev, sizeof(uint64_t) * (n + 1), hipMemcpyDeviceToHost, main.get()),
             "welded bases D2H");
    emfCheck(emf_hip_meshWeldStatus(weldScratch, nv, main.abi()), "meshWeld (table)");  // waits: the welded sizes
    const uint64_t nw = wBases[n];
    const size_t wvb = 3 * sizeof(float) * nw;
    if (meshArena.bytes() < 2 * vb + tb + 2 * wvb) {  // grow, keeping the soup
        DeviceBuffer grown(2 * vb + tb + 2 * wvb);
        hipCheck(hipMemcpyAsync(grown.data(), meshArena.data(), 2 * vb + tb, hipMemcpyDeviceToDevice, main.get()),
                 "mesh arena grow");
        main.waitForCompletion();
        meshArena = std::move(grown);
        vDev = meshArena.as<float>();
        nDev = vDev + 3 * nv;
        tDev = reinterpret_cast<int32_t*>(nDev + 3 * nv);
    }
    float* wvDev = reinterpret_cast<float*>(reinterpret_cast<char*>(meshArena.data()) + 2 * vb + tb);
    float* wnDev = wvDev + 3 * nw;
    if (colorOn) wcDev = DeviceBuffer(3 * nw);
    emfCheck(emf_hip_meshWeldEmitBatched(weldScratch, nv, nt, basesDev, wBasesDev, n, vDev, nDev,
                                         colorOn ? cDev.as<uint8_t>() : nullptr, tDev, wvDev, wnDev,
                                         colorOn ? wcDev.as<uint8_t>() : nullptr, tDev, main.abi()),
             "meshWeldEmitBatched");
    // what travels: the welded arrays, or the filter's kept arrays
    struct Slice {
        size_t v0, vc, t0, tc;
    };
    std::vector<Slice> slices(n);
    for (int k = 0; k < n; ++k) slices[k] = Slice{wBases[k], wCounts[k], bases[2 * k + 1], counts[k].triangles};
    const float* outV = wvDev;
    const float* outN = wnDev;
    const int32_t* outT = tDev;
    const uint8_t* outC = colorOn ? wcDev.as<uint8_t>() : nullptr;
    uint64_t outNv = nw, outNt = nt;
    DeviceBuffer kcDev;
    if (meshFilterActive()) {
        const size_t ccBytes = emf_hip_meshComponentsScratchBytes(nw, nt);
        if (ccBytes == 0) throw HipError("EMFusion::extractMeshes: " + std::to_string(nw) + " welded vertices", EMF_E_LIMIT);
        // [kept bases u64 x 2 (MAX + 1)][kept counts u32 x 2 MAX][components u32 x MAX][kept components u32 x MAX][scratch]
        const size_t kbBytes = sizeof(uint64_t) * 2 * (EMF_MAX_MODELS + 1), kcBytes = sizeof(uint32_t) * 2 * EMF_MAX_MODELS,
                     cBytes = sizeof(uint32_t) * EMF_MAX_MODELS, head = kbBytes + kcBytes + 2 * cBytes;
        if (meshFilterScratch.bytes() < head + ccBytes) meshFilterScratch = DeviceBuffer(head + ccBytes);
        auto* kBasesDev = meshFilterScratch.as<uint64_t>();
        auto* kCountsDev = reinterpret_cast<uint32_t*>(kBasesDev + 2 * (EMF_MAX_MODELS + 1));
        uint32_t* compsDev = kCountsDev + 2 * EMF_MAX_MODELS;
        uint32_t* kCompsDev = compsDev + EMF_MAX_MODELS;
        void* ccScratch = reinterpret_cast<char*>(meshFilterScratch.data()) + head;
        std::vector<uint32_t> mins(n, meshMinTriangles);
        std::vector<uint8_t> largest(n);
        for (int k = 0; k < n; ++k) largest[k] = meshFilterFor(ids[k]).largestOnly ? 1 : 0;
        emfCheck(emf_hip_meshComponentsLabelBatched(tDev, nw, nt, basesDev, wBasesDev, n, ccScratch, nullptr, nullptr,
                                                    main.abi()),
                 "meshComponentsLabelBatched");
        emfCheck(emf_hip_meshComponentsFilterCountBatched(tDev, nw, nt, basesDev, wBasesDev, n, ccScratch, mins.data(),
                                                          largest.data(), kCountsDev, kBasesDev, compsDev, kCompsDev,
                                                          main.abi()),
                 "meshComponentsFilterCountBatched");
        std::vector<uint64_t> kBases(2 * (n + 1));
        std::vector<uint32_t> kCounts(2 * n), comps(n), kComps(n);
        hipCheck(hipMemcpyAsync(kBases.data(), kBasesDev, sizeof(uint64_t) * 2 * (n + 1), hipMemcpyDeviceToHost, main.get()),
                 "kept bases D2H");
        hipCheck(hipMemcpyAsync(kCounts.data(), kCountsDev, sizeof(uint32_t) * 2 * n, hipMemcpyDeviceToHost, main.get()),
                 "kept counts D2H");
        hipCheck(hipMemcpyAsync(comps.data(), compsDev, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, main.get()),
                 "components D2H");
        hipCheck(hipMemcpyAsync(kComps.data(), kCompsDev, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, main.get()),
                 "kept components D2H");
        emfCheck(emf_hip_meshComponentsStatus(ccScratch, nw, nt, main.abi()), "meshComponents (indices)");  // waits
        const uint64_t knv = kBases[2 * n], knt = kBases[2 * n + 1];
        const size_t kvb = 3 * sizeof(float) * std::max<uint64_t>(knv, 1), ktb = 4 * sizeof(int32_t) * std::max<uint64_t>(knt, 1);
        if (meshFilterArena.bytes() < 2 * kvb + ktb) meshFilterArena = DeviceBuffer(2 * kvb + ktb);
        float* kvDev = meshFilterArena.as<float>();
        float* knDev = kvDev + 3 * std::max<uint64_t>(knv, 1);
        int32_t* ktDev = reinterpret_cast<int32_t*>(knDev + 3 * std::max<uint64_t>(knv, 1));
        if (colorOn) kcDev = DeviceBuffer(3 * std::max<uint64_t>(knv, 1));
        emfCheck(emf_hip_meshComponentsEmitBatched(ccScratch, nw, nt, basesDev, wBasesDev, n, wvDev, wnDev, outC, tDev, kvDev,
                                                   knDev, colorOn ? kcDev.as<uint8_t>() : nullptr, ktDev, main.abi()),
                 "meshComponentsEmitBatched");
        for (int k = 0; k < n; ++k) {
            meshFilterStats[ids[k]] = MeshFilterStats{comps[k], kComps[k], counts[k].triangles, kCounts[2 * k + 1], {}};
            slices[k] = Slice{kBases[2 * k], kCounts[2 * k], kBases[2 * k + 1], kCounts[2 * k + 1]};
        }
        outV = kvDev;
        outN = knDev;
        outT = ktDev;
        outC = colorOn ? kcDev.as<uint8_t>() : nullptr;
        outNv = knv;
        outNt = knt;
    }
    DeviceBuffer scDev;
    if (meshSimplifyActive() && outNv == 0) {
        for (int k = 0; k < n; ++k) meshSimplifyStats[ids[k]] = MeshSimplifyStats{};
    } else if (meshSimplifyActive()) {
        const size_t spBytes = emf_hip_meshSimplifyScratchBytes(outNv, outNt);
        if (spBytes == 0) throw HipError("EMFusion::extractMeshes: " + std::to_string(outNv) + " vertices to simplify", EMF_E_LIMIT);
        // [triangle bases u64 x 2 (MAX + 1)][vertex bases u64 x (MAX + 1)][kept bases u64 x 2 (MAX + 1)]
        // [kept counts u32 x 2 MAX][clusters u32 x MAX][scratch]
        const size_t tbBytes = sizeof(uint64_t) * 2 * (EMF_MAX_MODELS + 1), vbBytes = sizeof(uint64_t) * (EMF_MAX_MODELS + 1),
                     kcBytes = sizeof(uint32_t) * 2 * EMF_MAX_MODELS, clBytes = sizeof(uint32_t) * EMF_MAX_MODELS,
                     head = 2 * tbBytes + vbBytes + kcBytes + clBytes;
        if (meshSimplifyScratch.bytes() < head + spBytes) meshSimplifyScratch = DeviceBuffer(head + spBytes);
        auto* tBasesDev = meshSimplifyScratch.as<uint64_t>();
        auto* vBasesDev = tBasesDev + 2 * (EMF_MAX_MODELS + 1);
        auto* sBasesDev = vBasesDev + (EMF_MAX_MODELS + 1);
        auto* sCountsDev = reinterpret_cast<uint32_t*>(sBasesDev + 2 * (EMF_MAX_MODELS + 1));
        uint32_t* clustersDev = sCountsDev + 2 * EMF_MAX_MODELS;
        void* spScratch = reinterpret_cast<char*>(meshSimplifyScratch.data()) + head;
        // the bases of what the weld (or the filter) left, in the layout the entries take
        std::vector<uint64_t> tBases(2 * (n + 1), 0), vBases(n + 1, 0);
        for (int k = 0; k < n; ++k) {
            vBases[k] = slices[k].v0;
            tBases[2 * k] = slices[k].v0;
            tBases[2 * k + 1] = slices[k].t0;
        }
        vBases[n] = tBases[2 * n] = outNv;
        tBases[2 * n + 1] = outNt;
        hipCheck(hipMemcpyAsync(tBasesDev, tBases.data(), sizeof(uint64_t) * 2 * (n + 1), hipMemcpyHostToDevice, main.get()),
                 "simplify triangle bases upload");
        hipCheck(hipMemcpyAsync(vBasesDev, vBases.data(), sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, main.get()),
                 "simplify vertex bases upload");
        const std::vector<float> cells(n, meshSimplifyCell);
        emfCheck(emf_hip_meshSimplifyCount(outV, outN, outC, outT, outNv, outNt, tBasesDev, vBasesDev, n, cells.data(), nullptr,
                                           spScratch, sCountsDev, sBasesDev, clustersDev, main.abi()),
                 "meshSimplifyCount");
        std::vector<uint64_t> sBases(2 * (n + 1));
        std::vector<uint32_t> sCounts(2 * n), clusters(n);
        hipCheck(hipMemcpyAsync(sBases.data(), sBasesDev, sizeof(uint64_t) * 2 * (n + 1), hipMemcpyDeviceToHost, main.get()),
                 "simplified bases D2H");
        hipCheck(hipMemcpyAsync(sCounts.data(), sCountsDev, sizeof(uint32_t) * 2 * n, hipMemcpyDeviceToHost, main.get()),
                 "simplified counts D2H");
        hipCheck(hipMemcpyAsync(clusters.data(), clustersDev, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, main.get()),
                 "clusters D2H");
        emfCheck(emf_hip_meshSimplifyStatus(spScratch, outNv, outNt, main.abi()), "meshSimplify");  // waits; the uploads too
        const uint64_t snv = sBases[2 * n], snt = sBases[2 * n + 1];
        const size_t svb = 3 * sizeof(float) * std::max<uint64_t>(snv, 1), stb = 4 * sizeof(int32_t) * std::max<uint64_t>(snt, 1);
        if (meshSimplifyArena.bytes() < 2 * svb + stb) meshSimplifyArena = DeviceBuffer(2 * svb + stb);
        float* svDev = meshSimplifyArena.as<float>();
        float* snDev = svDev + 3 * std::max<uint64_t>(snv, 1);
        int32_t* stDev = reinterpret_cast<int32_t*>(snDev + 3 * std::max<uint64_t>(snv, 1));
        if (colorOn) scDev = DeviceBuffer(3 * std::max<uint64_t>(snv, 1));
        emfCheck(emf_hip_meshSimplifyEmit(spScratch, outNv, outNt, tBasesDev, vBasesDev, n, outV, outN, outC, outT, svDev, snDev,
                                          colorOn ? scDev.as<uint8_t>() : nullptr, stDev, main.abi()),
                 "meshSimplifyEmit");
        for (int k = 0; k < n; ++k) {
            meshSimplifyStats[ids[k]] = MeshSimplifyStats{static_cast<uint32_t>(slices[k].vc), static_cast<uint32_t>(slices[k].tc),
                                                          sCounts[2 * k], sCounts[2 * k + 1], clusters[k]};
            slices[k] = Slice{sBases[2 * k], sCounts[2 * k], sBases[2 * k + 1], sCounts[2 * k + 1]};
        }
        outV = svDev;
        outN = snDev;
        outT = stDev;
        outC = colorOn ? scDev.as<uint8_t>() : nullptr;
        outNv = snv;
        outNt = snt;
    }
    const size_t ovb = 3 * sizeof(float) * outNv;
    meshStage.grow(2 * ovb + 4 * sizeof(int32_t) * std::max<uint64_t>(outNt, 1));
    float* vHost = meshStage.as<float>();
    float* nHost = vHost + 3 * outNv;
    int32_t* tHost = reinterpret_cast<int32_t*>(nHost + 3 * outNv);
    if (outNv) {
        hipCheck(hipMemcpyAsync(vHost, outV, ovb, hipMemcpyDeviceToHost, main.get()), "welded vertices D2H");
        hipCheck(hipMemcpyAsync(nHost, outN, ovb, hipMemcpyDeviceToHost, main.get()), "welded normals D2H");
    }
    if (outNt) hipCheck(hipMemcpyAsync(tHost, outT, 4 * sizeof(int32_t) * outNt, hipMemcpyDeviceToHost, main.get()), "welded triangles D2H");
    std::vector<uint8_t> cHost;
    if (colorOn && outNv) {
        cHost.resize(3 * outNv);
        hipCheck(hipMemcpyAsync(cHost.data(), outC, 3 * outNv, hipMemcpyDeviceToHost, main.get()), "welded colours D2H");
    }
    main.waitForCompletion();
    for (int k = 0; k < n; ++k) {  // model k's slice is its own welded (filtered) mesh (local triangle indices)
        const Slice& s = slices[k];
        Mesh& m = out[k];
        m.cloud.assign(vHost + 3 * s.v0, vHost + 3 * (s.v0 + s.vc));
        m.normals.assign(nHost + 3 * s.v0, nHost + 3 * (s.v0 + s.vc));
        m.polygons.assign(tHost + 4 * s.t0, tHost + 4 * (s.t0 + s.tc));
        if (!cHost.empty()) m.colors.assign(cHost.begin() + 3 * s.v0, cHost.begin() + 3 * (s.v0 + s.vc));
    }
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
