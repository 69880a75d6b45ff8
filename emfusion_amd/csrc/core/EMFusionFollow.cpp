// EMFusionFollow.cpp -- emf::EMFusion: the background follows the camera (new behaviour, the
// reference's background is built once at params.volumePose and never moves).
#include "EMFusion.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace emf {

namespace {
constexpr int kTile[3] = {32, 8, 8};  // the integration tile (include/emf_hip.h "Rolling a volume")
}

bool EMFusion::followShift(const float q[3], const int32_t step[3], float voxelSize, int32_t shift[3]) {
    if (!q || !step || !shift) return false;
    if (!(voxelSize > 0.f) || !std::isfinite(voxelSize)) return false;
    int32_t k[3];
    for (int i = 0; i < 3; ++i) {
        if (step[i] <= 0 || step[i] % kTile[i] != 0 || !std::isfinite(q[i])) return false;
        const float cell = static_cast<float>(step[i]) * voxelSize;
        const float n = std::trunc(q[i] / cell);
        if (!(std::fabs(n) <= 1048576.f) || static_cast<double>(n) * step[i] > 2147483647.0 ||
            static_cast<double>(n) * step[i] < -2147483647.0)
            return false;
        k[i] = static_cast<int32_t>(n) * step[i];
    }
    for (int i = 0; i < 3; ++i) shift[i] = k[i];
    return true;
}

void EMFusion::setBackgroundFollow(bool on, const BackgroundFollowParams& p) {
    if (on && (sharded || world > 1))
        throw HipError("EMFusion::setBackgroundFollow: following the camera is not supported on the sharded path", EMF_E_ARG);
    for (int i = 0; i < 3; ++i)
        if (p.step[i] <= 0 || p.step[i] % kTile[i] != 0)
            throw HipError("EMFusion::setBackgroundFollow: step " + std::to_string(p.step[0]) + ", " + std::to_string(p.step[1]) +
                               ", " + std::to_string(p.step[2]) + " is not a positive multiple of the tile (32, 8, 8)",
                           EMF_E_ARG);
    if (!std::isfinite(p.lookAhead))
        throw HipError("EMFusion::setBackgroundFollow: lookAhead is not finite", EMF_E_ARG);
    followOn = on;
    followParams = p;
}

void EMFusion::setBackgroundStore(bool on, uint64_t maxBytes) {
    if (on && (sharded || world > 1))
        throw HipError("EMFusion::setBackgroundStore: the background store is not supported on the sharded path", EMF_E_ARG);
    if (!on) bgStore.clear();
    storeOn = on;
    bgStore.setBudget(maxBytes);
}

namespace {
// The tiles of a volume of nt tiles that a roll by k tiles (|k_i| <= nt_i) moves out of it -- or, entering = true, the
// tiles of the rolled volume that nothing moved into -- in at most three disjoint boxes: x first over all y, z, then
// y over the x that stays, then z over the x, y that stay (as retireSlabs cuts, without its extra voxel layer).
// dst(t) = src(t + k): with k > 0 the low tiles [0, k) leave and the high tiles [nt - k, nt) enter.
std::vector<TileBox> rollBoxes(const int nt[3], const int k[3], bool entering) {
    std::vector<TileBox> boxes;
    int lo[3] = {0, 0, 0}, hi[3] = {nt[0], nt[1], nt[2]};
    for (int axis = 0; axis < 3; ++axis) {
        if (k[axis] == 0) continue;
        const int m = std::abs(k[axis]);
        const bool low = (k[axis] > 0) != entering;  // the box sits at the low end of the axis
        TileBox b;
        for (int i = 0; i < 3; ++i) {
            b.lo[i] = lo[i];
            b.size[i] = hi[i] - lo[i];
        }
        b.lo[axis] = low ? 0 : nt[axis] - m;
        b.size[axis] = m;
        if (b.size[0] > 0 && b.size[1] > 0 && b.size[2] > 0) boxes.push_back(b);
        if (low)
            lo[axis] = m;
        else
            hi[axis] = nt[axis] - m;
        if (hi[axis] <= lo[axis]) break;  // everything left (entered): the later boxes are empty
    }
    return boxes;
}
}  // namespace

// The end of a frame with follow on: where is the followed point in the background's frame, and has it left the
// dead zone of one step around the centre?
void EMFusion::followCamera() {
    const Affine3f bg = background.getPose();
    const Vec3f p = pose.translation() + pose.rotation() * Vec3f(0.f, 0.f, followParams.lookAhead);
    const Vec3f q = bg.rotation().t() * (p - bg.translation());
    int32_t k[3];
    if (!followShift(q.val, followParams.step.val, background.getVoxelSize(), k)) return;  // a pose that is not finite
    if (k[0] == 0 && k[1] == 0 && k[2] == 0) return;
    rollBackgroundAt(Vec3i(k[0], k[1], k[2]), frameCount, followParams.keepRetired);  // processFrame counts the frame after this
}

// Between frames the frame at whose end this happens is the last one processed, as it is for the policy.
void EMFusion::rollBackground(const Vec3i& shift, int keepRetired) {
    rollBackgroundAt(shift, frameCount > 0 ? frameCount - 1 : 0, keepRetired < 0 ? followParams.keepRetired : keepRetired > 0);
}

void EMFusion::rollBackgroundAt(const Vec3i& shift, int frame, bool keepRetired) {
    if (sharded || world > 1)
        throw HipError("EMFusion::rollBackground: rolling the background is not supported on the sharded path", EMF_E_ARG);
    if (shift[0] == 0 && shift[1] == 0 && shift[2] == 0) return;
    if (storeOn) {  // before anything is changed
        const Vec3i n = background.getVolumeRes();
        if (!emf_hip_rollVolumeIsTiled(n.val, shift.val) || !emf_hip_rollVolumeIsTiled(n.val, bgOrigin.val))
            throw HipError("EMFusion::rollBackground: with the background store on, the shift (" + std::to_string(shift[0]) + ", " +
                               std::to_string(shift[1]) + ", " + std::to_string(shift[2]) +
                               "), the background resolution and the background origin must be multiples of the tile (32, 8, 8)",
                           EMF_E_ARG);
    }
    // as saveCheckpoint: nothing of this instance in flight, the visible set on the host (the table is rebuilt below)
    quiesce();
    refreshVisibleFromDevice();
    if (bgInFlight) joinBackground();
    quiesce();
    if (keepRetired) retireSlabs(shift, frame);
    if (storeOn) {
        const Vec3i n = background.getVolumeRes();
        int nt[3], k[3];
        TileKey before, after;  // lattice coordinate of the volume's tile (0, 0, 0)
        for (int i = 0; i < 3; ++i) {
            nt[i] = n[i] / kTile[i];
            k[i] = std::clamp(shift[i] / kTile[i], -nt[i], nt[i]);
            before[i] = bgOrigin[i] / kTile[i];
            after[i] = (bgOrigin[i] + shift[i]) / kTile[i];
        }
        bgStore.spill(background.tsdfPtr(), background.weightsPtr(), background.colorPtr(), n, rollBoxes(nt, k, false), before, main);
        const TileFill fill = bgStore.takeFill(rollBoxes(nt, k, true), after, main);
        background.roll(shift, main, &fill);
    } else {
        background.roll(shift, main);  // leaves the two copies equal, whatever they were
    }
    bgBackStale = false;
    bgPrepared = false;
    bgListPending = false;
    forkFrame = -2;
    farBoundsReady = false;
    rebuildModelTable();  // the copies changed roles; the relevant-tile list; sign maps of the general path
    for (int i = 0; i < 3; ++i) bgOrigin[i] += shift[i];
    bgRolled = true;
}

// The cubes of the old volume with at least one leaving voxel, in at most three disjoint sub-boxes: x first over all
// y, z, then y over the x that stays, then z over the x, y that stay.  Each sub-box is one voxel layer thicker than
// its slab on the staying side, so that each such cube is meshed exactly once and no cube whose eight voxels all stay
// is meshed.
void EMFusion::retireSlabs(const Vec3i& shift, int frame) {
    const Vec3i n = background.getVolumeRes();
    int lo[3] = {0, 0, 0}, hi[3] = {n[0], n[1], n[2]};  // the voxels that still stay, per axis, as the boxes are cut
    for (int axis = 0; axis < 3; ++axis) {
        const int k = shift[axis], N = n[axis];
        if (k == 0) continue;
        int b0, b1;  // the sub-box's voxel range on this axis
        if (k >= N || -k >= N) {  // everything leaves
            b0 = 0;
            b1 = N;
        } else if (k > 0) {  // voxels [0, k) leave: cubes 0 .. k - 1, voxels [0, k + 1)
            b0 = 0;
            b1 = k + 1;
        } else {  // voxels [N + k, N) leave: cubes N + k - 1 .. N - 2, voxels [N + k - 1, N)
            b0 = N + k - 1;
            b1 = N;
        }
        Vec3i boxLo(lo[0], lo[1], lo[2]), boxRes(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]);
        boxLo[axis] = b0;
        boxRes[axis] = b1 - b0;
        if (boxRes[0] >= 2 && boxRes[1] >= 2 && boxRes[2] >= 2) {  // (a box one voxel thin holds no cube)
            TSDF box = background.cutBox(boxLo, boxRes, main);
            RetiredSlab slab;
            slab.frame = frame;
            slab.origin = Vec3i(bgOrigin[0] + boxLo[0], bgOrigin[1] + boxLo[1], bgOrigin[2] + boxLo[2]);
            slab.res = boxRes;
            if (meshFilterActive())
                slab.mesh = box.getFilteredMesh(meshFilterFor(0));
            else
                slab.mesh = meshWeld ? box.getWeldedMesh() : box.getMesh();
            retired.push_back(std::move(slab));
        }
        // what stays on this axis, for the boxes of the later axes
        if (k >= N || -k >= N) {
            hi[axis] = lo[axis];  // nothing: the later boxes are empty
        } else if (k > 0) {
            lo[axis] = k;
        } else {
            hi[axis] = N + k;
        }
        if (hi[axis] - lo[axis] < 2) break;  // no cube is left for the later axes
    }
}

}  // namespace emf
