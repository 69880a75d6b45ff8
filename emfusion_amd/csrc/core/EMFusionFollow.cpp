// EMFusionFollow.cpp -- emf::EMFusion: the background follows the camera (new behaviour, the
// reference's background is built once at params.volumePose and never moves).
#include "EMFusion.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>

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

void EMFusion::requireTiledWorld(const char* who, const char* noun) const {
    const std::string name = std::string("EMFusion::") + who;
    if (sharded || world > 1) throw HipError(name + ": " + noun + " not supported on the sharded path", EMF_E_ARG);
    const Vec3i n = background.getVolumeRes();
    const int32_t none[3] = {0, 0, 0};
    if (!emf_hip_rollVolumeIsTiled(n.val, none) || !emf_hip_rollVolumeIsTiled(n.val, bgOrigin.val))
        throw HipError(name + ": the background resolution and the background origin must be multiples of the "
                              "tile (32, 8, 8)",
                       EMF_E_ARG);
}

void EMFusion::worldExtent(Vec3i& lo, Vec3i& size) const {
    std::vector<TileKey> keys;
    if (storeOn)
        for (const auto& held : bgStore.inOrder()) keys.push_back(held.first);
    tilesExtent(keys, kTile, bgOrigin, background.getVolumeRes(), lo, size);
}

EMFusion::WorldTiles EMFusion::listWorldTiles(const char* who) {
    const std::string name = std::string("EMFusion::") + who;
    WorldTiles out;
    const Vec3i n = background.getVolumeRes();
    const int nt[3] = {n[0] / kTile[0], n[1] / kTile[1], n[2] / kTile[2]};
    // an unseen-tile map of its own, from the front copy: the session's maps, valid or stale, are not touched
    DeviceBuffer unseenDev((emf_hip_unseenTileBytes(n.val) + 3) / 4 * 4);
    emfCheck(emf_hip_rebuildUnseenTiles(background.tsdfPtr(), background.weightsPtr(), n.val, unseenDev.as<uint8_t>(), main.abi()),
             (name + " (unseen tiles)").c_str());
    std::vector<uint8_t> unseen(unseenDev.bytes());
    unseenDev.download(unseen.data(), main);
    TileGather& stored = out.stored;
    if (storeOn && !bgStore.empty()) stored = bgStore.gather(main);

    // the table, sorted by (z, y, x) of the lattice tile coordinate
    const uint16_t* color = background.colorPtr();
    std::map<std::array<int32_t, 3>, emf_mesh_tile_t> table;  // key (z, y, x)
    const int32_t first[3] = {bgOrigin[0] / kTile[0], bgOrigin[1] / kTile[1], bgOrigin[2] / kTile[2]};
    for (int z = 0; z < nt[2]; ++z)
        for (int y = 0; y < nt[1]; ++y)
            for (int x = 0; x < nt[0]; ++x) {
                if (unseen[(static_cast<size_t>(z) * nt[1] + y) * nt[0] + x]) continue;
                emf_mesh_tile_t e{};
                e.coord[0] = first[0] + x;
                e.coord[1] = first[1] + y;
                e.coord[2] = first[2] + z;
                const uint64_t at = (static_cast<uint64_t>(z) * kTile[2] * n[1] + static_cast<uint64_t>(y) * kTile[1]) * n[0] +
                                    static_cast<uint64_t>(x) * kTile[0];
                e.cls[0] = e.cls[1] = 3;
                e.cls[2] = color ? 3 : 0;
                e.at[0] = e.at[1] = at;
                e.at[2] = color ? at : 0;
                table[{e.coord[2], e.coord[1], e.coord[0]}] = e;
                ++out.info.volumeTiles;
            }
    for (size_t i = 0; i < stored.keys.size(); ++i) {
        const TileKey& k = stored.keys[i];
        const std::array<int32_t, 3> key{k[2], k[1], k[0]};
        if (table.count(key)) {  // should not happen: a returned tile is taken out of the store
            ++out.info.duplicateTiles;
            continue;
        }
        emf_mesh_tile_t e{};
        for (int a = 0; a < 3; ++a) {
            e.coord[a] = k[a];
            e.cls[a] = stored.cls[3 * i + a];
            e.at[a] = stored.at[3 * i + a];
        }
        for (int a = 0; a < 4; ++a) e.words[a] = stored.words[4 * i + a];
        table[key] = e;
        out.storedKeys.push_back(key);
        ++out.info.storedTiles;
    }
    std::vector<emf_mesh_tile_t>& tiles = out.tiles;
    tiles.reserve(table.size());
    for (const auto& [key, e] : table) {
        out.index[key] = static_cast<int32_t>(tiles.size());
        tiles.push_back(e);
    }
    for (emf_mesh_tile_t& e : tiles)
        for (int k = 1; k < 8; ++k) {
            const auto it = out.index.find({e.coord[2] + ((k >> 2) & 1), e.coord[1] + ((k >> 1) & 1), e.coord[0] + (k & 1)});
            e.nbr[k - 1] = it == out.index.end() ? -1 : it->second;
        }
    emf_mesh_tiles_source_t& src = out.src;
    src.arena = stored.arena.empty() ? nullptr : stored.arena.data();
    src.arena_units = stored.arenaUnits;
    src.tsdf = background.tsdfPtr();
    src.weights = background.weightsPtr();
    src.color = color;
    src.volume_elements = static_cast<uint64_t>(n[0]) * n[1] * n[2];
    src.row_stride = n[0];
    src.plane_stride = static_cast<uint64_t>(n[0]) * n[1];
    if (!tiles.empty()) {
        out.tilesDev = DeviceBuffer(tiles.size() * sizeof(emf_mesh_tile_t));
        out.tilesDev.upload(tiles.data(), main);
    }
    return out;
}

Mesh EMFusion::worldMesh(int weld) {
    requireTiledWorld("worldMesh", "the world mesh is");
    const Vec3i n = background.getVolumeRes();
    // as rollBackgroundAt: nothing of this instance in flight, the front copy current
    quiesce();
    refreshVisibleFromDevice();
    if (bgInFlight) joinBackground();
    quiesce();
    const bool filtering = meshFilterActive() || meshSimplifyActive();  // (finishMesh does what the filter it gets asks)
    const bool welded = filtering || (weld < 0 ? meshWeld : weld > 0);
    WorldTiles listing = listWorldTiles("worldMesh");
    worldInfo = listing.info;
    const std::vector<emf_mesh_tile_t>& tiles = listing.tiles;
    std::map<std::array<int32_t, 3>, int32_t>& index = listing.index;
    const std::vector<std::array<int32_t, 3>>& storedKeys = listing.storedKeys;
    const emf_mesh_tiles_source_t& src = listing.src;
    const DeviceBuffer& tilesDev = listing.tilesDev;
    const uint16_t* color = background.colorPtr();

    Mesh mesh;
    mesh.colored = color != nullptr;
    const uint32_t count = static_cast<uint32_t>(tiles.size());
    if (count == 0) return mesh;
    const size_t scratchBytes = emf_hip_meshTilesScratchBytes(count);
    if (scratchBytes == 0) throw HipError("EMFusion::worldMesh: " + std::to_string(count) + " tiles", EMF_E_LIMIT);
    DeviceBuffer scratch(scratchBytes), countsDev(sizeof(emf_mesh_counts_t));
    emfCheck(emf_hip_meshTilesCount(tilesDev.as<emf_mesh_tile_t>(), tiles.data(), count, &src, scratch.data(),
                                    countsDev.as<emf_mesh_counts_t>(), main.abi()),
             "EMFusion::worldMesh (count)");
    emf_mesh_counts_t counts{};
    countsDev.download(&counts, main);
    {  // surface cubes owned by stored tiles: the third array of the scratch
        std::vector<uint32_t> all(scratchBytes / sizeof(uint32_t));
        scratch.download(all.data(), main);
        const uint32_t* cubes = all.data() + 2 * (static_cast<size_t>(count) + 1);
        for (const auto& key : storedKeys) worldInfo.storedSurfaceCubes += cubes[index[key]];
    }
    if (counts.vertices == 0) return mesh;
    const size_t soup = counts.vertices;
    const float half[3] = {static_cast<float>(n[0] - 1) / 2.f, static_cast<float>(n[1] - 1) / 2.f, static_cast<float>(n[2] - 1) / 2.f};
    DeviceBuffer v(soup * 3 * sizeof(float)), nn(soup * 3 * sizeof(float)),
        t(std::max<size_t>(counts.triangles, 1) * 4 * sizeof(int32_t)), c, keys;
    emfCheck(emf_hip_meshTilesEmit(tilesDev.as<emf_mesh_tile_t>(), count, &src, half, background.getVoxelSize(), scratch.data(),
                                   v.as<float>(), nn.as<float>(), t.as<int32_t>(), main.abi()),
             "EMFusion::worldMesh (emit)");
    if (color) {
        c = DeviceBuffer(soup * 3);
        emfCheck(emf_hip_meshTilesColors(tilesDev.as<emf_mesh_tile_t>(), count, &src, scratch.data(), c.as<uint8_t>(), main.abi()),
                 "EMFusion::worldMesh (colours)");
    }
    if (welded) {
        keys = DeviceBuffer(soup * sizeof(uint64_t));
        emfCheck(emf_hip_meshTilesEdgeKeys(tilesDev.as<emf_mesh_tile_t>(), count, &src, scratch.data(), keys.as<uint64_t>(), main.abi()),
                 "EMFusion::worldMesh (keys)");
    }
    main.waitForCompletion();  // the weld and the filter run on the null stream
    const MeshFilter filter = meshFilterFor(0);
    return TSDF::finishMesh(std::move(mesh), counts, std::move(v), std::move(nn), std::move(t), std::move(c), std::move(keys),
                            welded, filtering ? &filter : nullptr);
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
            if (meshFilterActive() || meshSimplifyActive())
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
