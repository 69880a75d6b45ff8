// TSDF.hpp -- emf::TSDF: one TSDF volume with its per-frame operations.
//
// Keeps the method surface of the reference's emf::TSDF for the per-frame volumetric path
// (reference include/EMFusion/core/TSDF.h:39-330, src/core/TSDF.cpp:28-168): constructor
// arguments, integrate / updateGradients / raycast / computeAssociation / reset and the getters.
// Every method enqueues hand-written gfx950 kernels through the emf_hip_* C ABI on the given
// stream and returns; nothing here computes on the host.  Tracking (prepareTracking ...
// syncTrack) and meshing are outside this build's scope.
#pragma once

#include <memory>
#include <vector>

#include "data.hpp"
#include "types.hpp"

namespace emf {

struct TileFill;  // TileStore.hpp

class TSDF {
public:
    /** How raycast() obtains the surface normal. */
    enum class Gradients {
        OnTheFly,     // blend forward differences of the TSDF at the hit (no gradient volume)
        Materialized  // keep the reference's N^3 x 3 gradient volume, rebuilt by updateGradients()
    };

    TSDF(Vec3i volumeRes, float voxelSize, float truncdist, Affine3f pose, TSDFParams params,
         Size frameSize, Gradients gradients = Gradients::OnTheFly);
    virtual ~TSDF() = default;
    TSDF(TSDF&&) = default;
    TSDF& operator=(TSDF&&) = default;

    /** Zero the volume (tsdf, weights, gradients) and set its pose (reference TSDF.cpp:77-82). */
    virtual void reset(const Affine3f& pose);

    void getCorners(Vec3f& low, Vec3f& high) const;
    Vec3f getVolumeSize() const;
    Vec3i getVolumeRes() const { return volumeRes; }
    float getVoxelSize() const { return voxelSize; }
    float getTruncDist() const { return truncdist; }
    Affine3f getPose() const { return pose; }
    /** Externally supplied pose (stands in for the tracking update of syncTrack()). */
    void setPose(const Affine3f& p) { pose = p; }
    size_t voxels() const {
        return static_cast<size_t>(volumeRes[0]) * volumeRes[1] * volumeRes[2];
    }

    /**
     * Fuse one depth frame, weighted per pixel by the association weights
     * (reference TSDF::integrate, TSDF.cpp:108-118).  depth, weights: f32 W x H device images.
     * invLambda: optional emf_hip_computeInvLambda table for `intr` (same results, fewer
     * instructions per voxel).
     */
    void integrate(const emf_image_t& depth, const emf_image_t& weights, const Affine3f& cam_pose,
                   const Matx33f& intr, Stream& stream = Stream::Null(),
                   const emf_image_t* invLambda = nullptr);

    /**
     * Refresh the gradient volume (reference TSDF::updateGradients, TSDF.cpp:120-123).  A no-op in
     * Gradients::OnTheFly mode, where raycast() differences the TSDF directly.
     */
    void updateGradients(Stream& stream = Stream::Null());

    /**
     * Ray-march the volume from cam_pose (reference TSDF::raycast, TSDF.cpp:158-168).  The four
     * outputs must be zeroed by the caller beforehand, as in the reference.
     */
    virtual void raycast(const Affine3f& cam_pose, const Matx33f& intr,
                         const emf_image_t& raylengths, const emf_image_t& vertices,
                         const emf_image_t& normals, const emf_image_t& mask,
                         Stream& stream = Stream::Null(), uint64_t* stats = nullptr);

    /**
     * Un-normalised association likelihood of the camera-frame points with this volume
     * (reference TSDF::computeAssociation + computeLaplace, TSDF.cpp:125-156), one fused kernel.
     */
    void computeAssociation(const emf_image_t& points, const Affine3f& cam_pose,
                            const emf_image_t& associationWeights,
                            Stream& stream = Stream::Null());

    /**
     * The second half of every mesh extraction, on a soup that lies on the device: weld by `keys` (one u64 per vertex,
     * needed with `weld`), label / filter by connected component, download.  `mesh`: the empty result, `colored` set.
     */
    static Mesh finishMesh(Mesh mesh, emf_mesh_counts_t counts, DeviceBuffer v, DeviceBuffer n, DeviceBuffer t, DeviceBuffer c,
                           DeviceBuffer keys, bool weld, const MeshFilter* filter = nullptr, MeshFilterStats* stats = nullptr,
                           MeshComponents* components = nullptr);
    /**
     * Iso-surface of the observed part of the volume (weights > 0), marching cubes on the device
     * (reference TSDF::getMesh, TSDF.cpp:356-373).  Synchronises.
     */
    virtual Mesh getMesh();
    /**
     * getMesh() welded by grid edge on the device (include/emf_hip.h "Welded meshes"): one vertex per edge -- the
     * first copy's bits -- and the soup's triangles re-indexed.  An output form only: whatever the life cycle
     * measures on a mesh (extent statistics count duplicates as the reference does) goes through getMesh().
     */
    virtual Mesh getWeldedMesh();
    /**
     * getWeldedMesh() with its small connected components removed on the device (include/emf_hip.h "Mesh
     * components"): only the filtered arrays travel to the host.  An output form only, as getWeldedMesh().
     */
    virtual Mesh getFilteredMesh(const MeshFilter& filter, MeshFilterStats* stats = nullptr);
    /** Labels and component sizes of getWeldedMesh()'s vertices, unfiltered. */
    virtual MeshComponents getMeshComponents();

    /** Host copies in the reference layout, (Nz*Ny) rows x Nx cols (TSDF.cpp:398-408). */
    std::vector<float> getTSDF() const;
    std::vector<float> getWeightsVol() const;

    const float* tsdfPtr() const { return tsdfVol.as<float>(); }
    const float* weightsPtr() const { return tsdfWeights.as<float>(); }
    const float* gradsPtr() const { return tsdfGrads.empty() ? nullptr : tsdfGrads.as<float>(); }
    uint8_t* brickFlagsPtr() const { return brickFlags.as<uint8_t>(); }
    Gradients gradientMode() const { return gradMode; }

    /**
     * Colour volume (include/emf_hip.h "Per-voxel colour"): u16 x 4 per voxel, allocated and zeroed by
     * enableColor() (a no-op when it exists), zeroed by reset(), shifted by ObjTSDF::resize.
     */
    void enableColor();
    void dropColor() { colorVol = DeviceBuffer(); }
    bool hasColor() const { return !colorVol.empty(); }
    uint16_t* colorPtr() const { return colorVol.empty() ? nullptr : colorVol.as<uint16_t>(); }
    /** Host copy, (Nz*Ny*Nx) x 4 u16; empty without a colour volume. */
    std::vector<uint16_t> getColorVol() const;

    /**
     * Keep the volume twice (MI355X has the memory: 1 GB more for a 512^3 background) so that a
     * frame's integration can run out of place, concurrently with the same frame's raycast
     * (emf_hip_integrateBatchedCulledOut; EMFusion::integrateBatched).  Everything else keeps reading
     * tsdfPtr() / weightsPtr(), the FRONT copy; after an out-of-place integration into backBuffers()
     * the owner calls flip().  Allocates the second copy (equal to the first) and the two dirty maps.
     */
    void enableDoubleBuffer();
    bool doubleBuffered() const { return !tsdfBack.empty(); }
    /** Second copy + dirty maps in the roles emf_hip_integrateBatchedCulledOut expects now. */
    emf_volume_out_t backBuffers() const;
    /** The back copy holds the newly integrated state: make it the front. */
    void flip();
    /** After an IN-PLACE integration of a double-buffered volume: make the copies equal again. */
    void resyncBack();

    /**
     * Sign maps (emf_model_t.signMaps, include/emf_hip.h): kept by the tile integration launches through
     * the model table, read by emf_hip_raycastFarBounds.  Anything else that writes the tsdf volume
     * calls invalidateSignMaps(); refreshSignMaps() rebuilds them from the values when they are stale
     * (the owner calls it before describe()).  Volumes with Nx % 4 != 0 have none (no tile launches).
     */
    void invalidateSignMaps() { signMapsValid = false; }
    /**
     * The tsdf / weights (and colour) of the FRONT copy were written from outside the integration (a checkpoint being
     * restored): what is derived from them is invalidated or rebuilt the way ObjTSDF::resize does it -- brick flags
     * "mixed" everywhere, sign maps stale (the owner's rebuildModelTable() refreshes them and the tile lists),
     * materialised gradients recomputed, the back copy made equal.  Waits for `stream`.
     */
    virtual void volumesWritten(Stream& stream);
    /**
     * Shift the contents by whole voxels (include/emf_hip.h "Rolling a volume"): afterwards voxel v holds what voxel
     * v + shift held, zeros where that lay outside, and the pose is translated by the same amount exactly as
     * ObjTSDF::resize moves an object's: pose.translate(pose.rotation() * (float(shift_i) * voxelSize)).  One launch,
     * front copy -> back copy and flip() (a volume kept once, and the colour volume, roll into a fresh buffer that
     * takes the old one's place); then the other copy is made equal (resyncBack).  Derived state ends as
     * volumesWritten() leaves it -- brick flags "mixed", relevant-tile list emptied for the owner's
     * rebuildModelTable(), materialised gradients recomputed -- except that valid sign / unseen maps stay valid on
     * the tile-granular path: the launch moves their entries.  Waits for `stream`; the owner has joined every other
     * stream that touches this volume.
     * fill (emf::TileStore::takeFill; needs a resolution that is a multiple of the tile): tiles to write into the
     * rolled volume with emf_hip_fillTiles, after the roll's launch and before the copies change roles -- into the
     * destination arrays, the new colour buffer and, only when the roll moved the maps, the new maps -- so that the
     * gradients and the other copy are made from the restored values.
     */
    void roll(const Vec3i& shift, Stream& stream, const TileFill* fill = nullptr);
    /**
     * A volume of its own holding the voxels [lo, lo + res) of this one's front copy (and colour), cut with
     * emf_hip_copyValues / emf_hip_copyColorValues; the parts of the box outside this volume read as zeros.  Its
     * pose is this volume's, translated to the box's centre.  Waits for `stream`.
     */
    TSDF cutBox(const Vec3i& lo, const Vec3i& res, Stream& stream) const;
    void refreshSignMaps(Stream& stream = Stream::Null());

    /**
     * Static part of this volume's entry in the device model table used by the batched launches
     * (emf_model_t, include/emf_hip.h); image pointers are filled in by the owner of the images.
     */
    virtual void describe(emf_model_t& m) const;
    /** 0 / 1 / 2 from the environment variable EMF_BRICK_FLAGS, see TSDF.cpp. */
    static int brickFlagMode();

    /**
     * The checked reciprocal of the voxel size (emf_hip_voxelReciprocal) is a device-side verdict
     * (3 x 2^23 inputs, ~20 microseconds) the first time a size is seen in the process.  With deferral on,
     * a constructor that meets a new size does not wait for it: the check is enqueued on a stream of
     * its own, the march divides (same results) and pollReciprocal() adopts the verdict once it is in.
     * emf::EMFusion turns this on after its background exists, so objects created inside a frame
     * (reference EMFusion.cpp:495-560) never stall it.
     */
    static void deferReciprocalChecks(bool on);
    /** True if the verdict arrived with this call (the owner refreshes its model table). */
    bool pollReciprocal();
    /** Wait for a deferred check in flight (it ends here); pollReciprocal() then adopts it. */
    void settleReciprocal();
    float reciprocal() const { return rcpVoxel; }

protected:
    Mesh extractMesh(const uint8_t* fgVolMask, bool weld = false, const MeshFilter* filter = nullptr,
                     MeshFilterStats* stats = nullptr, MeshComponents* components = nullptr);
    TSDFParams params;
    Vec3i volumeRes;
    float voxelSize;
    float truncdist;
    float rcpVoxel = 0.f;  // emf_hip_voxelReciprocal(voxelSize): checked stand-in for x / voxelSize
    Affine3f pose;  // volume-centre frame -> world
    Gradients gradMode;
    Size frameSize;

    DeviceBuffer tsdfVol;      // N^3 f32
    DeviceBuffer tsdfWeights;  // N^3 f32
    DeviceBuffer tsdfGrads;    // N^3 x 3 f32, only in Materialized mode
    DeviceBuffer brickFlags;   // ceil(N/8)^3 u8 uniformity flags kept by integrate(), read by raycast()
    DeviceBuffer colorVol;     // N^3 x 4 u16 (R, G, B, Wc in 8.8 fixed point), only after enableColor()
    // double buffering (enableDoubleBuffer): the other copy, and per 32x8x8 tile "the copies differ"
    DeviceBuffer tsdfBack, weightsBack;
    DeviceBuffer dirtyMaps[2];
    DeviceBuffer signMaps;      // per 32x8x8 tile: holds a positive tsdf / holds a negative tsdf
    bool signMapsValid = false;
    DeviceBuffer relevantTiles; // count + indices of the tiles in which a raycast hit can be completed
    DeviceBuffer unseenTiles;   // per tile: every weight is 0 (emf_model_t.unseenTiles); valid with the sign maps
    int dirtyPrev = 0;  // index of the map the last out-of-place integration wrote

private:
    struct PendingReciprocal;
    struct PendingDeleter {
        void operator()(PendingReciprocal* p) const;
    };
    std::unique_ptr<PendingReciprocal, PendingDeleter> pendingRcp;  // a deferred check in flight
    void obtainReciprocal();
};

}  // namespace emf
