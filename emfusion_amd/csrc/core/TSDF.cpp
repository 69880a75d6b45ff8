// TSDF.cpp -- emf::TSDF over the emf_hip_* C ABI (see TSDF.hpp).
#include "TSDF.hpp"

#include "MeshPost.hpp"
#include "Switches.hpp"
#include "TileStore.hpp"

#include <algorithm>
#include <atomic>
#include <mutex>

namespace emf {

TSDF::TSDF(Vec3i _volumeRes, float _voxelSize, float _truncdist, Affine3f _pose,
           TSDFParams _params, Size _frameSize, Gradients gradients)
    : params(_params),
      volumeRes(_volumeRes),
      voxelSize(_voxelSize),
      truncdist(_truncdist),
      gradMode(gradients),
      frameSize(_frameSize),
      tsdfVol(voxels() * sizeof(float)),
      tsdfWeights(voxels() * sizeof(float)),
      brickFlags(2 * static_cast<size_t>((_volumeRes[0] + 3) / 4) * ((_volumeRes[1] + 3) / 4) *
                 ((_volumeRes[2] + 3) / 4)) {  // raw flags + dilated flags
    if (gradMode == Gradients::Materialized) tsdfGrads = DeviceBuffer(voxels() * 3 * sizeof(float));
    obtainReciprocal();
    reset(_pose);
}

// ---- checked reciprocal of the voxel size ---------------------------------------------------------
// Is 1 / voxelSize usable in place of the march's divisions?  An exhaustive device check per distinct
// voxel size and process (emf_hip_voxelReciprocal*); EMF_VOXEL_RCP=0 keeps the divisions for A/B runs.
namespace {
std::atomic<bool> g_deferReciprocal{false};
std::mutex g_rcpSlotMutex;
// Process-lifetime slots: pinned host words the verdicts are COPIED to, allocated once, never freed -- they live as long
// as the process, by design, hence the raw hipHostMalloc below instead of a PinnedBuffer
unsigned long long* g_rcpSlots = nullptr;
unsigned long long* g_rcpSlotsDev = nullptr;  // the device counters the check adds into (no atomics across PCIe)
constexpr int kRcpSlots = 256;
bool g_rcpSlotUsed[kRcpSlots] = {};
hipStream_t g_rcpStream = nullptr;         // lowest priority: the check must not delay a frame

int take_rcp_slot() {
    std::lock_guard<std::mutex> lock(g_rcpSlotMutex);
    if (!g_rcpSlots) {
        void* p = nullptr;
        if (hipHostMalloc(&p, sizeof(unsigned long long) * kRcpSlots, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        g_rcpSlots = static_cast<unsigned long long*>(p);
        void* dp = nullptr;
        if (hipMalloc(&dp, sizeof(unsigned long long) * kRcpSlots) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        g_rcpSlotsDev = static_cast<unsigned long long*>(dp);
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&g_rcpStream, hipStreamNonBlocking, least) != hipSuccess) {
            (void)hipGetLastError();
            g_rcpStream = nullptr;
            return -1;
        }
    }
    if (!g_rcpStream || !g_rcpSlotsDev) return -1;
    for (int i = 0; i < kRcpSlots; ++i)
        if (!g_rcpSlotUsed[i]) {
            g_rcpSlotUsed[i] = true;
            return i;
        }
    return -1;
}
void give_rcp_slot(int i) {
    std::lock_guard<std::mutex> lock(g_rcpSlotMutex);
    g_rcpSlotUsed[i] = false;
}
}  // namespace

struct TSDF::PendingReciprocal {
    int slot = -1;
    Event done;
};
void TSDF::PendingDeleter::operator()(PendingReciprocal* p) const {
    if (!p) return;
    // the check may still be running and will write its slot: wait for THAT kernel (rare: a volume
    // destroyed within milliseconds of its creation), then hand the slot back
    if (!p->done.empty()) (void)hipEventSynchronize(p->done.get());
    if (p->slot >= 0) give_rcp_slot(p->slot);
    delete p;  // (and the event with it)
}

void TSDF::deferReciprocalChecks(bool on) { g_deferReciprocal = on; }

void TSDF::obtainReciprocal() {
    rcpVoxel = 0.f;
    if (!switchValue(Switch::voxelRcp)) return;
    const int known = emf_hip_voxelReciprocalCached(voxelSize, &rcpVoxel);
    if (known == EMF_OK) return;            // this size has been checked in this process
    if (known != EMF_E_NOTREADY) return;    // outside the checked range: the march divides
    if (g_deferReciprocal) {
        const int slot = take_rcp_slot();
        if (slot >= 0) {
            std::unique_ptr<PendingReciprocal, PendingDeleter> p(new PendingReciprocal);
            p->slot = slot;
            try {
                p->done = Event(hipEventDisableTiming);
            } catch (const HipError&) {  // no event: the check below runs now instead
            }
            if (!p->done.empty() &&
                emf_hip_voxelReciprocalBegin(voxelSize, g_rcpSlotsDev + slot,
                                             reinterpret_cast<emf_stream_t>(g_rcpStream)) == EMF_OK &&
                hipMemcpyAsync(g_rcpSlots + slot, g_rcpSlotsDev + slot, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               g_rcpStream) == hipSuccess &&
                p->done.tryRecord(g_rcpStream)) {
                pendingRcp = std::move(p);
                return;  // rcpVoxel stays 0 until pollReciprocal() sees the verdict
            }
            (void)hipGetLastError();
        }
    }
    if (emf_hip_voxelReciprocal(voxelSize, &rcpVoxel) != EMF_OK) rcpVoxel = 0.f;
}

bool TSDF::pollReciprocal() {
    if (!pendingRcp) return false;
    if (hipEventQuery(pendingRcp->done.get()) != hipSuccess) {
        (void)hipGetLastError();  // not ready
        return false;
    }
    const unsigned long long bad = g_rcpSlots[pendingRcp->slot];
    pendingRcp.reset();
    if (emf_hip_voxelReciprocalEnd(voxelSize, bad, &rcpVoxel) != EMF_OK) rcpVoxel = 0.f;
    return rcpVoxel != 0.f;
}

void TSDF::settleReciprocal() {
    if (pendingRcp && !pendingRcp->done.empty()) (void)hipEventSynchronize(pendingRcp->done.get());
}

void TSDF::reset(const Affine3f& _pose) {
    Stream& s = Stream::Null();
    tsdfVol.setZero(s);
    tsdfWeights.setZero(s);
    if (!tsdfGrads.empty()) tsdfGrads.setZero(s);
    if (!colorVol.empty()) colorVol.setZero(s);
    emfCheck(emf_hip_resetBrickFlags(brickFlags.as<uint8_t>(), volumeRes.val, s.abi()),
             "TSDF::reset");
    if (volumeRes[0] % 4 == 0) {  // an all-zero volume has neither sign anywhere
        if (signMaps.empty()) signMaps = DeviceBuffer(emf_hip_signMapBytes(volumeRes.val));
        signMaps.setZero(s);
        signMapsValid = true;
        if (relevantTiles.empty()) relevantTiles = DeviceBuffer(emf_hip_relevantTileBytes(volumeRes.val));
        relevantTiles.setZero(s);  // count 0: nothing can be hit in an empty volume
        // ... and every tile of it is unseen (allocation rounded up to whole words for the fill)
        if (unseenTiles.empty()) unseenTiles = DeviceBuffer((emf_hip_unseenTileBytes(volumeRes.val) + 3) / 4 * 4);
        unseenTiles.fill32(0x01010101u, s);
    } else {
        signMaps = DeviceBuffer();
        signMapsValid = false;
        relevantTiles = DeviceBuffer();
        unseenTiles = DeviceBuffer();
    }
    if (doubleBuffered()) {  // equal copies, clean maps
        tsdfBack.setZero(s);
        weightsBack.setZero(s);
        dirtyMaps[0].setZero(s);
        dirtyMaps[1].setZero(s);
    }
    s.waitForCompletion();  // per-volume streams are non-blocking: do not race the clears
    pose = _pose;
}

void TSDF::refreshSignMaps(Stream& stream) {
    if (signMapsValid || volumeRes[0] % 4 != 0) return;
    const size_t bytes = emf_hip_signMapBytes(volumeRes.val);
    if (signMaps.empty() || signMaps.bytes() != bytes) signMaps = DeviceBuffer(bytes);
    emfCheck(emf_hip_rebuildSignMaps(tsdfVol.as<float>(), volumeRes.val, signMaps.as<uint8_t>(), stream.abi()),
             "TSDF::refreshSignMaps");
    signMapsValid = true;
    const size_t rb = emf_hip_relevantTileBytes(volumeRes.val);
    if (relevantTiles.empty() || relevantTiles.bytes() != rb) relevantTiles = DeviceBuffer(rb);
    relevantTiles.setZero(stream);  // the owner rebuilds the list (emf_hip_updateRelevantTiles) before it is used
    const size_t ub = (emf_hip_unseenTileBytes(volumeRes.val) + 3) / 4 * 4;
    if (unseenTiles.empty() || unseenTiles.bytes() != ub) unseenTiles = DeviceBuffer(ub);
    emfCheck(emf_hip_rebuildUnseenTiles(tsdfVol.as<float>(), tsdfWeights.as<float>(), volumeRes.val,
                                        unseenTiles.as<uint8_t>(), stream.abi()),
             "TSDF::refreshSignMaps");
}

void TSDF::enableDoubleBuffer() {
    if (doubleBuffered()) return;
    hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
    tsdfBack = DeviceBuffer(voxels() * sizeof(float));
    weightsBack = DeviceBuffer(voxels() * sizeof(float));
    hipCheck(hipMemcpy(tsdfBack.data(), tsdfVol.data(), voxels() * sizeof(float), hipMemcpyDeviceToDevice),
             "TSDF::enableDoubleBuffer");
    hipCheck(hipMemcpy(weightsBack.data(), tsdfWeights.data(), voxels() * sizeof(float), hipMemcpyDeviceToDevice),
             "TSDF::enableDoubleBuffer");
    const size_t bytes = emf_hip_integrateDirtyMapBytes(volumeRes.val);
    for (auto& d : dirtyMaps) {
        d = DeviceBuffer(bytes);
        d.setZero(Stream::Null());
    }
    Stream::Null().waitForCompletion();
    dirtyPrev = 0;
}

emf_volume_out_t TSDF::backBuffers() const {
    emf_volume_out_t o;
    o.tsdf = tsdfBack.as<float>();
    o.weights = weightsBack.as<float>();
    o.dirtyPrev = dirtyMaps[dirtyPrev].as<uint8_t>();
    o.dirtyNext = dirtyMaps[1 - dirtyPrev].as<uint8_t>();
    return o;
}

void TSDF::resyncBack() {
    if (!doubleBuffered()) return;
    hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hipCheck(hipMemcpy(tsdfBack.data(), tsdfVol.data(), voxels() * sizeof(float), hipMemcpyDeviceToDevice),
             "TSDF::resyncBack");
    hipCheck(hipMemcpy(weightsBack.data(), tsdfWeights.data(), voxels() * sizeof(float), hipMemcpyDeviceToDevice),
             "TSDF::resyncBack");
    dirtyMaps[0].setZero(Stream::Null());
    dirtyMaps[1].setZero(Stream::Null());
    Stream::Null().waitForCompletion();
}

void TSDF::volumesWritten(Stream& stream) {
    brickFlags.setZero(stream);  // every brick "mixed": always correct; integrate() refines them
    signMapsValid = false;
    updateGradients(stream);
    stream.waitForCompletion();
    resyncBack();
}

void TSDF::roll(const Vec3i& shift, Stream& stream, const TileFill* fill) {
    const bool twice = doubleBuffered();
    DeviceBuffer newVol, newWeights, newColor, newSign, newUnseen;
    if (!twice) {
        newVol = DeviceBuffer(voxels() * sizeof(float));
        newWeights = DeviceBuffer(voxels() * sizeof(float));
    }
    if (!colorVol.empty()) newColor = DeviceBuffer(voxels() * 4 * sizeof(uint16_t));
    // maps that describe the values travel with them on the tile-granular path; stale ones stay stale
    const bool moveMaps = emf_hip_rollVolumeIsTiled(volumeRes.val, shift.val) && signMapsValid && !signMaps.empty() &&
                          !unseenTiles.empty();
    if (moveMaps) {
        newSign = DeviceBuffer(signMaps.bytes());
        newUnseen = DeviceBuffer(unseenTiles.bytes());
    }
    emfCheck(emf_hip_rollVolume(tsdfVol.as<float>(), tsdfWeights.as<float>(), colorVol.empty() ? nullptr : colorVol.as<uint16_t>(),
                                moveMaps ? signMaps.as<uint8_t>() : nullptr, moveMaps ? unseenTiles.as<uint8_t>() : nullptr,
                                twice ? tsdfBack.as<float>() : newVol.as<float>(),
                                twice ? weightsBack.as<float>() : newWeights.as<float>(),
                                newColor.empty() ? nullptr : newColor.as<uint16_t>(),
                                moveMaps ? newSign.as<uint8_t>() : nullptr, moveMaps ? newUnseen.as<uint8_t>() : nullptr,
                                volumeRes.val, shift.val, stream.abi()),
             "TSDF::roll");
    if (fill && fill->n)  // what the store kept of the entering region, maps included when they travel
        emfCheck(emf_hip_fillTiles(twice ? tsdfBack.as<float>() : newVol.as<float>(),
                                   twice ? weightsBack.as<float>() : newWeights.as<float>(),
                                   newColor.empty() ? nullptr : newColor.as<uint16_t>(), moveMaps ? newSign.as<uint8_t>() : nullptr,
                                   moveMaps ? newUnseen.as<uint8_t>() : nullptr, volumeRes.val, fill->coords.as<int32_t>(),
                                   fill->classes.as<uint8_t>(), fill->classesHost.data(), fill->words.as<uint32_t>(),
                                   fill->lits.as<uint32_t>(), fill->arena.data(), fill->arenaUnits, fill->n, stream.abi()),
                 "TSDF::roll (fill)");
    stream.waitForCompletion();  // the old buffers are released below
    if (twice) {
        flip();
    } else {
        tsdfVol = std::move(newVol);
        tsdfWeights = std::move(newWeights);
    }
    if (!newColor.empty()) colorVol = std::move(newColor);
    if (moveMaps) {
        signMaps = std::move(newSign);
        unseenTiles = std::move(newUnseen);
    }
    Vec3f offset;  // as ObjTSDF::resize forms its newCenter
    for (int i = 0; i < 3; ++i) offset[i] = static_cast<float>(shift[i]) * voxelSize;
    pose = pose.translate(pose.rotation() * offset);
    brickFlags.setZero(stream);  // every brick "mixed": always correct; integrate() refines them
    signMapsValid = moveMaps;
    if (!relevantTiles.empty()) relevantTiles.setZero(stream);  // the owner rebuilds the list before it is used
    updateGradients(stream);
    stream.waitForCompletion();
    resyncBack();
}

TSDF TSDF::cutBox(const Vec3i& lo, const Vec3i& res, Stream& stream) const {
    Vec3f centre;  // of the box, in this volume's frame: voxel index i sits at (i - (N - 1) / 2) * voxelSize
    for (int i = 0; i < 3; ++i)
        centre[i] = (static_cast<float>(lo[i]) + static_cast<float>(res[i] - 1) / 2.f - static_cast<float>(volumeRes[i] - 1) / 2.f) *
                    voxelSize;
    TSDF box(res, voxelSize, truncdist, pose.translate(pose.rotation() * centre), params, frameSize, gradMode);
    emfCheck(emf_hip_copyValues(tsdfVol.as<float>(), box.tsdfVol.as<float>(), 1, lo.val, volumeRes.val, res.val, stream.abi()),
             "TSDF::cutBox");
    emfCheck(emf_hip_copyValues(tsdfWeights.as<float>(), box.tsdfWeights.as<float>(), 1, lo.val, volumeRes.val, res.val,
                                stream.abi()),
             "TSDF::cutBox");
    if (!colorVol.empty()) {
        box.enableColor();
        emfCheck(emf_hip_copyColorValues(colorVol.as<uint16_t>(), box.colorVol.as<uint16_t>(), lo.val, volumeRes.val, res.val,
                                         stream.abi()),
                 "TSDF::cutBox (colour)");
    }
    box.signMapsValid = false;
    box.updateGradients(stream);
    stream.waitForCompletion();
    return box;
}

void TSDF::flip() {
    std::swap(tsdfVol, tsdfBack);
    std::swap(tsdfWeights, weightsBack);
    dirtyPrev = 1 - dirtyPrev;
}

void TSDF::getCorners(Vec3f& low, Vec3f& high) const {
    // (res - 1) * voxelSize / 2 (reference TSDF.cpp:84-89)
    const Vec3f corner(static_cast<float>(volumeRes[0] - 1) * voxelSize / 2,
                       static_cast<float>(volumeRes[1] - 1) * voxelSize / 2,
                       static_cast<float>(volumeRes[2] - 1) * voxelSize / 2);
    low = -corner;
    high = corner;
}

Vec3f TSDF::getVolumeSize() const {
    return Vec3f(static_cast<float>(volumeRes[0]) * voxelSize,
                 static_cast<float>(volumeRes[1]) * voxelSize,
                 static_cast<float>(volumeRes[2]) * voxelSize);
}

void TSDF::integrate(const emf_image_t& depth, const emf_image_t& weights,
                     const Affine3f& cam_pose, const Matx33f& intr, Stream& stream,
                     const emf_image_t* invLambda) {
    const Affine3f rel_pose_OC = cam_pose.inv() * pose;  // volume -> camera
    signMapsValid = false;  // the per-volume launch does not keep them
    emfCheck(emf_hip_updateTSDF(&depth, &weights, tsdfVol.as<float>(), tsdfWeights.as<float>(),
                                brickFlagMode() ? brickFlags.as<uint8_t>() : nullptr,
                                rel_pose_OC.rotation().val, rel_pose_OC.translation().val,
                                intr.val, volumeRes.val, voxelSize, truncdist,
                                params.maxTSDFWeight, invLambda, stream.abi()),
             "TSDF::integrate");
}

void TSDF::updateGradients(Stream& stream) {
    if (gradMode != Gradients::Materialized) return;
    emfCheck(emf_hip_computeTSDFGrads(tsdfVol.as<float>(), tsdfGrads.as<float>(), volumeRes.val,
                                      stream.abi()),
             "TSDF::updateGradients");
}

void TSDF::raycast(const Affine3f& cam_pose, const Matx33f& intr, const emf_image_t& raylengths,
                   const emf_image_t& vertices, const emf_image_t& normals,
                   const emf_image_t& mask, Stream& stream, uint64_t* stats) {
    pollReciprocal();  // a volume used outside an emf::EMFusion adopts its deferred verdict here
    const Affine3f rel_pose_CO = pose.inv() * cam_pose;  // camera -> volume
    emfCheck(emf_hip_raycastTSDF(tsdfVol.as<float>(), gradsPtr(), tsdfWeights.as<float>(), nullptr,
                                 brickFlagMode() ? brickFlags.as<uint8_t>() : nullptr, &raylengths, &vertices, &normals, &mask,
                                 rel_pose_CO.rotation().val, rel_pose_CO.translation().val,
                                 intr.val, volumeRes.val, voxelSize, truncdist, rcpVoxel, stats,
                                 stream.abi()),
             "TSDF::raycast");
}

void TSDF::computeAssociation(const emf_image_t& points, const Affine3f& cam_pose,
                              const emf_image_t& associationWeights, Stream& stream) {
    const Affine3f rel_pose_CO = pose.inv() * cam_pose;
    emfCheck(emf_hip_computeAssociation(tsdfVol.as<float>(), nullptr, &points,
                                        rel_pose_CO.rotation().val,
                                        rel_pose_CO.translation().val, volumeRes.val, voxelSize,
                                        truncdist, params.assocSigma, params.alpha,
                                        params.uniPrior, &associationWeights, stream.abi()),
             "TSDF::computeAssociation");
}

int TSDF::brickFlagMode() {  // (read on every call: an instance picks the switch up when it is constructed)
    return static_cast<int>(switchValue(Switch::brickFlags));
}

void TSDF::describe(emf_model_t& m) const {
    m.tsdf = tsdfVol.as<float>();
    m.weights = tsdfWeights.as<float>();
    m.grads = gradsPtr();
    m.fgProbs = nullptr;
    m.fgVolMask = nullptr;
    m.res[0] = volumeRes[0];
    m.res[1] = volumeRes[1];
    m.res[2] = volumeRes[2];
    m.id = 0;
    m.voxelSize = voxelSize;
    m.truncdist = truncdist;
    m.maxWeight = params.maxTSDFWeight;
    m.assocC1 = -truncdist / params.assocSigma;         // reference TSDF.cpp:151
    m.assocC2 = 1.f / (2.f * params.assocSigma);        // reference TSDF.cpp:154
    m.alpha = params.alpha;
    m.assocC3 = (1 - params.alpha) * params.uniPrior;   // reference TSDF.cpp:133
    // EMF_BRICK_FLAGS selects how the brick uniformity flags are used by the class-level path:
    //   0 (default) not maintained, not used -- on the bench scene the march time is set by a few
    //     hundred image-border rays that graze seen/unseen space through MIXED bricks, so skipping
    //     work elsewhere does not shorten the kernel while maintaining the flags costs ~0.2 ms
    //   1 maintained by integrate, raycast fast-forwards through deep-uniform bricks
    //   2 as 1, and uniform lookups are answered from the flags without gathering
    const int mode = brickFlagMode();
    m.brickFlags = mode ? brickFlags.as<uint8_t>() : nullptr;
    m.reserved = mode == 2 ? 2 : 0;
    m.rcpVoxel = rcpVoxel;
    m.signMaps = signMapsValid && !signMaps.empty() ? signMaps.as<uint8_t>() : nullptr;
    // a list pays for large volumes (the far bounds then project a few thousand tiles instead of scanning
    // 65 536 neighbourhoods); an object volume's thousand tiles are scanned faster than a list is kept
    m.relevantTiles = m.signMaps && !relevantTiles.empty() && emf_hip_signMapBytes(volumeRes.val) / 2 >= 8192
                          ? relevantTiles.as<uint32_t>()
                          : nullptr;
    // (kept valid together with the sign maps: the same launches maintain both)
    const bool useUnseen = switchValue(Switch::unseenTiles) != 0;
    m.unseenTiles = useUnseen && m.signMaps && !unseenTiles.empty() ? unseenTiles.as<uint8_t>() : nullptr;
    m.pad_ = 0;
}

Mesh TSDF::getMesh() { return extractMesh(nullptr); }
Mesh TSDF::getWeldedMesh() { return extractMesh(nullptr, true); }
Mesh TSDF::getFilteredMesh(const MeshFilter& filter, MeshFilterStats* stats) {
    return extractMesh(nullptr, true, &filter, stats);
}
MeshComponents TSDF::getMeshComponents() {
    MeshComponents c;
    extractMesh(nullptr, true, nullptr, nullptr, &c);
    return c;
}

// count -> read back two numbers -> emit; the gradient volume is used when it is materialised.  weld: keys, first
// occurrences and ranks on the device, one more number read back, then the welded arrays are what is downloaded.
// filter (an active one, on the welded mesh): labels, keep flags and ranks on the device, the kept counts read back,
// then the filtered arrays are what is downloaded; a filter with a simplifyCell: the welded (and filtered) mesh
// clustered by cell on the device, the simplified arrays downloaded.  components: the welded mesh's labels and sizes
// instead.
Mesh TSDF::extractMesh(const uint8_t* fgVolMask, bool weld, const MeshFilter* filter, MeshFilterStats* stats,
                       MeshComponents* components) {
    if (stats) *stats = MeshFilterStats{};
    hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
    Stream& s = Stream::Null();
    DeviceBuffer scratch(std::max<size_t>(emf_hip_meshScratchBytes(volumeRes.val), 8));
    DeviceBuffer countsDev(sizeof(emf_mesh_counts_t));
    emfCheck(emf_hip_meshCount(tsdfVol.as<float>(), tsdfWeights.as<float>(), fgVolMask, volumeRes.val,
                               scratch.data(), countsDev.as<emf_mesh_counts_t>(), s.abi()),
             "TSDF::getMesh");
    emf_mesh_counts_t counts{};
    countsDev.download(&counts, s);
    Mesh mesh;
    mesh.colored = !colorVol.empty();
    if (counts.vertices == 0) return mesh;
    const size_t soup = counts.vertices;
    DeviceBuffer v(soup * 3 * sizeof(float)), n(soup * 3 * sizeof(float)),
        t(std::max<size_t>(counts.triangles, 1) * 4 * sizeof(int32_t)), c;
    emfCheck(emf_hip_meshEmit(tsdfVol.as<float>(), gradsPtr(), tsdfWeights.as<float>(), fgVolMask,
                              volumeRes.val, voxelSize, scratch.data(), v.as<float>(), n.as<float>(),
                              t.as<int32_t>(), s.abi()),
             "TSDF::getMesh");
    if (!colorVol.empty()) {  // the same vertices, coloured
        c = DeviceBuffer(soup * 3);
        emfCheck(emf_hip_meshColors(tsdfVol.as<float>(), tsdfWeights.as<float>(), fgVolMask, colorVol.as<uint16_t>(),
                                    volumeRes.val, scratch.data(), c.as<uint8_t>(), s.abi()),
                 "TSDF::getMesh (colours)");
    }
    DeviceBuffer keys;
    if (weld) {
        keys = DeviceBuffer(soup * sizeof(uint64_t));
        emfCheck(emf_hip_meshEdgeKeys(tsdfVol.as<float>(), tsdfWeights.as<float>(), fgVolMask, volumeRes.val,
                                      scratch.data(), keys.as<uint64_t>(), s.abi()),
                 "TSDF::getWeldedMesh (keys)");
    }
    return finishMesh(std::move(mesh), counts, std::move(v), std::move(n), std::move(t), std::move(c), std::move(keys), weld,
                      filter, stats, components);
}

// What every mesher here does with its soup on the device (vertices, normals, triangles, colours or an empty buffer,
// and with `weld` one u64 grid-edge key per vertex): the chain of MeshPost.hpp for one model on the null stream, and
// only what is left comes to the host.  mesh: the empty result with its `colored` flag set.  The chain's buffers and
// the soup's live until this function returns, behind the download's wait: nothing in between waits for the stream
// but the Status calls that read the sizes.
Mesh TSDF::finishMesh(Mesh mesh, emf_mesh_counts_t counts, DeviceBuffer v, DeviceBuffer n, DeviceBuffer t, DeviceBuffer c,
                      DeviceBuffer keys, bool weld, const MeshFilter* filter, MeshFilterStats* stats,
                      MeshComponents* components) {
    Stream& s = Stream::Null();
    MeshPost post;
    DeviceMesh left{v.as<float>(), n.as<float>(), t.as<int32_t>(), c.empty() ? nullptr : c.as<uint8_t>(), counts.vertices,
                    counts.triangles};
    std::vector<MeshSlice> slices{MeshSlice{0, counts.vertices, 0, counts.triangles}};
    if (weld) {
        MeshPost::Request req;
        req.filter = filter && filter->active();
        req.simplify = filter && filter->simplifying();  // clustered by cell behind the filter
        req.perModel = filter;
        req.components = components;
        MeshPost::Result r = post.run(s, MeshPost::Soup{left.v, left.n, t.as<int32_t>(), left.c, keys.as<uint64_t>(), left.nv, left.nt},
                                      MeshPost::Table{1, nullptr, nullptr}, req, "TSDF::getWeldedMesh");
        if (stats && req.filter) *stats = r.filterStats[0];
        if (stats && req.simplify) stats->simplify = r.simplifyStats[0];
        left = r.mesh;
        slices = r.slices;
    }
    post.download(s, left, slices, &mesh);
    return mesh;
}

std::vector<float> TSDF::getTSDF() const {
    hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
    std::vector<float> h(voxels());
    tsdfVol.download(h.data(), Stream::Null());
    return h;
}

std::vector<float> TSDF::getWeightsVol() const {
    hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
    std::vector<float> h(voxels());
    tsdfWeights.download(h.data(), Stream::Null());
    return h;
}

void TSDF::enableColor() {
    if (!colorVol.empty()) return;
    colorVol = DeviceBuffer(voxels() * 4 * sizeof(uint16_t));
    Stream& s = Stream::Null();
    colorVol.setZero(s);
    s.waitForCompletion();
}

std::vector<uint16_t> TSDF::getColorVol() const {
    std::vector<uint16_t> h;
    if (colorVol.empty()) return h;
    hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
    h.resize(voxels() * 4);
    colorVol.download(h.data(), Stream::Null());
    return h;
}

}  // namespace emf
