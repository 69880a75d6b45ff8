// EMFusionView.cpp -- emf::EMFusion: the map seen from a free viewpoint (reference --3d-vis, apps/EM-Fusion.cpp:118-131,
// EMFusion::render's viz window, src/core/EMFusion.cpp:162-231, and its mesh_vis_out/ log, EMFusion.cpp:1018-1025).
//
// The reference meshes every model every frame and draws the meshes with VTK.  Here the viewer's rays are marched
// through the volumes directly, in one launch (emf_hip_renderView): the same raycast, composite, hide and Phong steps
// render() runs for the tracked camera, at any pose, intrinsics and size, without touching the frame's images.
#include "EMFusion.hpp"
#include "EMFusionDetail.hpp"
#include "Output.hpp"

#include <algorithm>

namespace emf {

using namespace detail;

void EMFusion::renderView(const Affine3f& viewerPose, const float K[9], Size size, uint8_t* rgb, float* raylengths,
                          uint8_t* seg, int shading) {
    if (shading != ShadeLabel && shading != ShadeColor)
        throw HipError("EMFusion::renderView: unknown shading " + std::to_string(shading), EMF_E_ARG);
    if (shading == ShadeColor && !colorOn)
        throw HipError("EMFusion::renderView: colour shading needs colour (enableColor)", EMF_E_ARG);
    if (sharded)  // like render(): remote objects are not on this rank
        throw HipError("EMFusion::renderView: not available on the sharded path (remote objects stay on their ranks)",
                       EMF_E_ARG);
    if (!rgb || !K) throw HipError("EMFusion::renderView: rgb and K are required", EMF_E_NULL);
    if (size.width <= 0 || size.height <= 0)
        throw HipError("EMFusion::renderView: bad view size " + std::to_string(size.width) + " x " +
                           std::to_string(size.height),
                       EMF_E_SHAPE);
    const size_t px = size.area();
    if (frameCount < 1) {  // nothing fused yet: black, like render()
        std::fill(rgb, rgb + 3 * px, uint8_t{0});
        if (raylengths) std::fill(raylengths, raylengths + px, 0.f);
        if (seg) std::fill(seg, seg + px, uint8_t{0});
        return;
    }
    // A frame that threw between the fork of the background's integration and its join left the fork open: join it
    // here as the next frame would (the copies flip once).  Then order `main` behind every stream of the frame.
    if (bgInFlight) joinBackground();
    main.waitFor(aux);
    for (auto& kv : streams) main.waitFor(kv.second);

    const int n = static_cast<int>(modelsHost.size());
    if (n < 1 || n > EMF_MAX_MODELS) throw HipError("EMFusion::renderView: " + std::to_string(n) + " models", EMF_E_LIMIT);
    if (viewPosesHost.empty()) viewPosesHost = PinnedBuffer(sizeof(emf_pose_t) * EMF_MAX_MODELS);
    emf_pose_t* const posesHost = viewPosesHost.as<emf_pose_t>();
    if (viewPosesDev.empty()) viewPosesDev = DeviceBuffer(sizeof(emf_pose_t) * EMF_MAX_MODELS);
    // viewer -> volume in table order (reference TSDF.cpp:141,162 with the viewer as the camera)
    std::vector<int32_t> ids;
    uint8_t hide[32] = {};
    posesHost[0] = toPose(background.getPose().inv() * viewerPose);
    int slot = 1;
    for (const auto& obj : objects) {
        posesHost[slot++] = toPose(obj.getPose().inv() * viewerPose);
        ids.push_back(obj.getID());
        if (ignorePerson && isPerson(obj) && obj.getID() >= 1 && obj.getID() <= 255)  // render(): EMFusion.cpp:139-150
            hide[obj.getID() >> 3] |= static_cast<uint8_t>(1u << (obj.getID() & 7));
    }
    if (slot != n) throw HipError("EMFusion::renderView: model table out of step with the object list", EMF_E_ARG);
    hipCheck(hipMemcpyAsync(viewPosesDev.data(), posesHost, sizeof(emf_pose_t) * n, hipMemcpyHostToDevice,
                            main.get()),
             "view poses upload");
    // the table that describes the volumes' current copies: the batched path's (after the ping-pong), or one built
    // from the host description for the per-volume path, which keeps none on the device
    const emf_model_t* table = currentTable();
    if (!batched) {
        if (viewTableDev.empty()) viewTableDev = DeviceBuffer(sizeof(emf_model_t) * EMF_MAX_MODELS);
        hipCheck(hipMemcpyAsync(viewTableDev.data(), modelsHost.data(), sizeof(emf_model_t) * n, hipMemcpyHostToDevice,
                                main.get()),
                 "view table upload");
        table = viewTableDev.as<emf_model_t>();
    }
    if (viewImage.empty() || viewImage.size().width != size.width || viewImage.size().height != size.height) {
        viewImage = DeviceImage<uint8_t, 3>(size);
        viewRay = DeviceImage<float>(size);
        viewSeg = DeviceImage<uint8_t>(size);
        viewVert = DeviceImage<float, 3>();
    }
    const bool shadeColor = shading == ShadeColor;
    if (shadeColor && viewVert.empty()) {
        viewVert = DeviceImage<float, 3>(size);
        viewNorm = DeviceImage<float, 3>(size);
        viewColor = DeviceImage<uint8_t, 3>(size);
    }
    const emf_image_t iv = viewImage.view(), rv = viewRay.view(), sv = viewSeg.view();
    const float light[3] = {0.f, 0.f, 0.f};  // at the viewer, as render() has it at the camera
    emf_image_t vv{}, nv{}, cv{};
    if (shadeColor) {
        vv = viewVert.view();
        nv = viewNorm.view();
        cv = viewColor.view();
    }
    emfCheck(emf_hip_renderView(table, viewPosesDev.as<emf_pose_t>(), ids.data(), n, size.width, size.height, K, light,
                                colorMap.data(), hide, &iv, raylengths ? &rv : nullptr, (seg || shadeColor) ? &sv : nullptr,
                                shadeColor ? &vv : nullptr, shadeColor ? &nv : nullptr, nullptr, main.abi()),
             "renderView");
    if (shadeColor) {
        // A pixel pass over what the view kernel hit (it stays as it is): the colour of the voxel nearest to each
        // vertex in the model the segmentation names, then the same Phong terms fed with it.  Labels hidden by
        // ignore_person were replaced by the background's hit in the view kernel, so they sample the background.
        emfCheck(emf_hip_sampleColor(table, colorTable.as<uint16_t*>(), viewPosesDev.as<emf_pose_t>(), ids.data(), n, &vv,
                                     &sv, colorMap.data(), &cv, main.abi()),
                 "sampleColor");
        emfCheck(emf_hip_renderPhongColor(&vv, &nv, &cv, light, &iv, main.abi()), "renderPhongColor");
    }
    hipCheck(hipMemcpyAsync(rgb, viewImage.ptr(), 3 * px, hipMemcpyDeviceToHost, main.get()), "view D2H");
    if (raylengths)
        hipCheck(hipMemcpyAsync(raylengths, viewRay.ptr(), sizeof(float) * px, hipMemcpyDeviceToHost, main.get()),
                 "view D2H");
    if (seg) hipCheck(hipMemcpyAsync(seg, viewSeg.ptr(), px, hipMemcpyDeviceToHost, main.get()), "view D2H");
    main.waitForCompletion();
}

void EMFusion::set3dView(const Affine3f& viewerPose, const float K[9], Size size) {
    if (!K) throw HipError("EMFusion::set3dView: K is NULL", EMF_E_NULL);
    if (size.width <= 0 || size.height <= 0) throw HipError("EMFusion::set3dView: bad view size", EMF_E_SHAPE);
    view3d = true;
    view3dPose = viewerPose;
    std::copy(K, K + 9, view3dK);
    view3dSize = size;
}

void EMFusion::set3dViewShading(int shading) {
    if (shading != ShadeLabel && shading != ShadeColor)
        throw HipError("EMFusion::set3dViewShading: unknown shading " + std::to_string(shading), EMF_E_ARG);
    if (shading == ShadeColor && !colorOn)
        throw HipError("EMFusion::set3dViewShading: colour shading needs colour (enableColor)", EMF_E_ARG);
    view3dShading = shading;
}

// render()'s 3D view: EMFusion::render draws the viz window every frame and writeResults writes what it showed
void EMFusion::render3dView() {
    if (!view3d) return;
    view3dRgb.resize(3 * view3dSize.area());
    renderView(view3dPose, view3dK, view3dSize, view3dRgb.data(), nullptr, nullptr, colorOn ? view3dShading : ShadeLabel);
    if (saveOutput)  // `mesh_vis[frameCount-1]`, EMFusion.cpp:228-230
        meshVis[frameCount - 1] = io::encodePng(view3dRgb.data(), view3dSize.width, view3dSize.height, 3);
}

}  // namespace emf
