// EMFusionDistance.cpp -- emf::EMFusion: the distance field of the scene (new behaviour, the reference
// exports meshes only).  Occupancy classes of a box of the background, the live objects stamped at their current
// poses, and the exact Euclidean distance transform over them: three entries of include/emf_hip.h "Distance field"
// on the main stream.
#include "EMFusion.hpp"
#include "Output.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace emf {

QueryBox EMFusion::queryBoxAt(const Vec3i& lo, const Vec3i& size) const {
    QueryBox box;
    box.size = size;
    box.bgPose = background.getPose();
    box.voxelSize = background.getVoxelSize();
    // a box that leaves the background (the world extent) is one of a virtual background, padded by as
    // many voxels on both sides of an axis as the box leaves it on either: every expression below gives the same bits
    const Vec3i res = background.getVolumeRes();
    box.pad = queryBoxPad(lo, size, res);
    for (int i = 0; i < 3; ++i) {
        box.lo[i] = lo[i] + box.pad[i];
        box.bgRes[i] = res[i] + 2 * box.pad[i];
    }
    const Vec3i n = box.bgRes;
    const float voxel = box.voxelSize;
    const Vec3i at = box.lo;
    const Vec3f corner((static_cast<float>(at[0]) - static_cast<float>(n[0] - 1) / 2.f) * voxel,
                       (static_cast<float>(at[1]) - static_cast<float>(n[1] - 1) / 2.f) * voxel,
                       (static_cast<float>(at[2]) - static_cast<float>(n[2] - 1) / 2.f) * voxel);
    box.boxPose = Affine3f(box.bgPose.rotation(), box.bgPose.rotation() * corner + box.bgPose.translation());
    return box;
}

QueryBox EMFusion::makeQueryBox(const char* who, const char* noun, const Vec3i& lo, const Vec3i& size, bool volumeOnly) const {
    const std::string name = std::string("EMFusion::") + who;
    const bool worldBox = queryWorld_ && !volumeOnly;
    if (worldBox)
        requireTiledWorld(who, noun);
    else if (sharded || world > 1)
        throw HipError(name + ": " + noun + " not supported on the sharded path", EMF_E_ARG);
    const Vec3i n = background.getVolumeRes();
    constexpr long long kLattice = 1ll << 19;  // lattice voxels in [-2^19, 2^19), as the tiles of emf_hip_meshTiles*
    unsigned long long voxels = 1;
    for (int i = 0; i < 3; ++i) {
        if (size[i] < 1 || (!worldBox && (lo[i] < 0 || lo[i] > n[i] - size[i])))
            throw HipError(name + ": the box leaves the background on axis " + std::to_string(i), EMF_E_ARG);
        if (size[i] > EMF_DF_MAX_AXIS)
            throw HipError(name + ": a box axis of " + std::to_string(size[i]) + " voxels", EMF_E_LIMIT);
        const long long first = static_cast<long long>(lo[i]) + bgOrigin[i];
        if (worldBox && (first < -kLattice || first + size[i] > kLattice))
            throw HipError(name + ": the box leaves the lattice on axis " + std::to_string(i), EMF_E_LIMIT);
        voxels *= static_cast<unsigned long long>(size[i]);
    }
    if (voxels > 0x7fffffffull) throw HipError(name + ": a box of more than 2^31 - 1 voxels", EMF_E_LIMIT);
    return queryBoxAt(lo, size);
}

void EMFusion::resultsBox(const char* who, Vec3i& lo, Vec3i& size) const {
    lo = Vec3i(0, 0, 0);
    size = background.getVolumeRes();
    if (!queryWorld_) return;
    worldExtent(lo, size);
    for (int i = 0; i < 3; ++i)
        if (size[i] > EMF_DF_MAX_AXIS)
            throw HipError(std::string("EMFusion::") + who + ": the world extent has " + std::to_string(size[i]) + " voxels on axis " +
                               std::to_string(i) + ", above " + std::to_string(EMF_DF_MAX_AXIS),
                           EMF_E_LIMIT);
    if (static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]) > 0x7fffffffull)
        throw HipError(std::string("EMFusion::") + who + ": the world extent has more than 2^31 - 1 voxels (axes " +
                           std::to_string(size[0]) + ", " + std::to_string(size[1]) + ", " + std::to_string(size[2]) + ")",
                       EMF_E_LIMIT);
}

// as worldMesh: nothing of this instance in flight, the front copies current
void EMFusion::drainForQuery() {
    quiesce();
    refreshVisibleFromDevice();
    if (bgInFlight) joinBackground();
    quiesce();
}

// the classes of the box and the live objects stamped into them, on the main stream
void EMFusion::enqueueOccupancy(const char* who, const QueryBox& box, const std::vector<int>& excludeIds, uint8_t* classes,
                                std::vector<int>* ids, std::vector<Affine3f>* poses) {
    const std::string name = std::string("EMFusion::") + who;
    const Vec3i n = box.bgRes, boxLo = box.lo, boxSize = box.size;
    const float voxel = box.voxelSize;
    const Affine3f bgPose = box.bgPose;
    if (queryWorld_) {  // the tiles of the session's map instead of the dense volume, on the lattice
        queryTiles = listWorldTiles(who);
        const Vec3i at = box.volumeLo();
        const int32_t latticeLo[3] = {at[0] + bgOrigin[0], at[1] + bgOrigin[1], at[2] + bgOrigin[2]};
        const uint32_t count = static_cast<uint32_t>(queryTiles.tiles.size());
        emfCheck(emf_hip_occupancyTiles(count ? queryTiles.tilesDev.as<emf_mesh_tile_t>() : nullptr, queryTiles.tiles.data(), count,
                                        &queryTiles.src, latticeLo, boxSize.val, classes, main.abi()),
                 (name + " (tile classes)").c_str());
    } else {
        emfCheck(emf_hip_occupancyClasses(background.tsdfPtr(), background.weightsPtr(), n.val, boxLo.val, boxSize.val, classes,
                                          main.abi()),
                 (name + " (classes)").c_str());
    }
    std::vector<emf_occ_object_t> table;
    for (const ObjTSDF& obj : objects) {
        if (std::find(excludeIds.begin(), excludeIds.end(), obj.getID()) != excludeIds.end()) continue;
        const Affine3f ob = obj.getPose().inv() * bgPose;  // object volume <- background volume
        emf_occ_object_t o{};
        o.tsdf = obj.tsdfPtr();
        o.weights = obj.weightsPtr();
        o.fgVolMask = obj.fgVolMaskPtr();
        const Vec3i r = obj.getVolumeRes();
        for (int i = 0; i < 3; ++i) o.res[i] = r[i];
        o.voxelSize = obj.getVoxelSize();
        std::copy(ob.rotation().val, ob.rotation().val + 9, o.R);
        std::copy(ob.translation().val, ob.translation().val + 3, o.t);
        emfCheck(emf_hip_occupancyObjectBox(&o, n.val, voxel), (name + " (object box)").c_str());
        table.push_back(o);
        if (ids) ids->push_back(obj.getID());
        if (poses) poses->push_back(ob);
    }
    if (!table.empty())
        emfCheck(emf_hip_occupancyStampObjects(classes, n.val, voxel, boxLo.val, boxSize.val, table.data(),
                                               static_cast<int32_t>(table.size()), main.abi()),
                 (name + " (objects)").c_str());
}

// the clearance of frontiers() and plan(): at least clearanceVoxels from the nearest occupied voxel of the box.  The cap
// keeps the scans of the transform short; what lies beyond it comes back as "far", which passes the gate as every d2
// above it would
EMFusion::Clearance EMFusion::enqueueClearance(const char* who, const QueryBox& box, const uint8_t* classes, int clearanceVoxels) {
    const int cap = std::min(clearanceVoxels, 4095);
    const Clearance out{nullptr, cap * cap};  // 4095^2 is above every distance of a box: only "far" passes then
    if (clearanceVoxels <= 0) return out;
    clearanceD2.reserve(box.voxels() * sizeof(int32_t));
    ++clearanceSerial;
    emfCheck(emf_hip_distanceTransform(classes, box.size.val, 1u << EMF_OCC_OCCUPIED, cap, clearanceD2.as<int32_t>(), nullptr, 0.f,
                                       main.abi()),
             (std::string("EMFusion::") + who + " (clearance)").c_str());
    return Clearance{clearanceD2.as<int32_t>(), out.minD2};
}

const EMFusion::DistanceField& EMFusion::distanceField(const Vec3i& boxLo, const Vec3i& boxSize, uint32_t siteMask, int capVoxels,
                                                       const std::vector<int>& excludeIds, bool metres, bool nearest) {
    DistanceField out;
    out.box = makeQueryBox("distanceField", "the distance field is", boxLo, boxSize);
    if (siteMask < 1u || siteMask > 7u) throw HipError("EMFusion::distanceField: siteMask outside 1 .. 7", EMF_E_ARG);
    if (capVoxels < 0) throw HipError("EMFusion::distanceField: a negative cap", EMF_E_ARG);
    drainForQuery();
    // buffers of the types.hpp owner, at first use and whenever a larger box comes
    const size_t voxels = out.box.voxels();
    dfClasses.reserve(voxels);
    dfD2.reserve(voxels * sizeof(int32_t));
    if (metres) dfMetres.reserve(voxels * sizeof(float));
    if (nearest) dfNearest.reserve(voxels * sizeof(int32_t));
    if (nearest) dfNearestScratch.reserve(voxels * sizeof(int32_t));

    const float voxel = out.box.voxelSize;
    enqueueOccupancy("distanceField", out.box, excludeIds, dfClasses.as<uint8_t>(), &out.objectIds, &out.objectPoses);
    if (nearest)
        emfCheck(emf_hip_distanceTransformNearest(dfClasses.as<uint8_t>(), boxSize.val, siteMask, capVoxels, dfD2.as<int32_t>(),
                                                  metres ? dfMetres.as<float>() : nullptr, dfNearest.as<int32_t>(),
                                                  dfNearestScratch.as<int32_t>(), voxel, main.abi()),
                 "EMFusion::distanceField (transform, nearest)");
    else
        emfCheck(emf_hip_distanceTransform(dfClasses.as<uint8_t>(), boxSize.val, siteMask, capVoxels, dfD2.as<int32_t>(),
                                           metres ? dfMetres.as<float>() : nullptr, voxel, main.abi()),
                 "EMFusion::distanceField (transform)");
    out.classes = dfClasses.as<uint8_t>();
    out.d2 = dfD2.as<int32_t>();
    out.metres = metres ? dfMetres.as<float>() : nullptr;
    out.nearest = nearest ? dfNearest.as<int32_t>() : nullptr;
    out.siteMask = siteMask;
    dfLast = std::move(out);
    return dfLast;
}

void EMFusion::queryDistance(const int32_t* voxels, int n, uint8_t* outClass, int32_t* outD2, int32_t* outNearest) {
    if (sharded || world > 1)
        throw HipError("EMFusion::queryDistance: the distance field is not supported on the sharded path", EMF_E_ARG);
    if (n < 0 || (n > 0 && !voxels)) throw HipError("EMFusion::queryDistance: " + std::to_string(n) + " points without a list", EMF_E_ARG);
    if (!dfLast.classes) throw HipError("EMFusion::queryDistance: no distance field has been computed", EMF_E_ARG);
    if (outNearest && !dfLast.nearest)
        throw HipError("EMFusion::queryDistance: the last distance field was computed without the nearest-site index", EMF_E_ARG);
    if (n == 0 || (!outClass && !outD2 && !outNearest)) return;
    // one device block: the voxels, then the three outputs (i32, i32, u8)
    const size_t un = static_cast<size_t>(n), need = un * (3 + 1 + 1) * sizeof(int32_t) + (un + 3) / 4 * 4;
    dfQuery.reserve(need);
    int32_t* dVox = dfQuery.as<int32_t>();
    int32_t* dD2 = dVox + 3 * un;
    int32_t* dNear = dD2 + un;
    uint8_t* dClass = reinterpret_cast<uint8_t*>(dNear + un);
    hipCheck(hipMemcpyAsync(dVox, voxels, 3 * un * sizeof(int32_t), hipMemcpyHostToDevice, main.get()), "EMFusion::queryDistance (voxels)");
    emfCheck(emf_hip_distanceQuery(outClass ? dfLast.classes : nullptr, outD2 ? dfLast.d2 : nullptr,
                                   outNearest ? dfLast.nearest : nullptr, dfLast.box.size.val, dVox, n, outClass ? dClass : nullptr,
                                   outD2 ? dD2 : nullptr, outNearest ? dNear : nullptr, main.abi()),
             "EMFusion::queryDistance");
    if (outClass) hipCheck(hipMemcpyAsync(outClass, dClass, un, hipMemcpyDeviceToHost, main.get()), "EMFusion::queryDistance (class)");
    if (outD2) hipCheck(hipMemcpyAsync(outD2, dD2, un * sizeof(int32_t), hipMemcpyDeviceToHost, main.get()), "EMFusion::queryDistance (d2)");
    if (outNearest)
        hipCheck(hipMemcpyAsync(outNearest, dNear, un * sizeof(int32_t), hipMemcpyDeviceToHost, main.get()), "EMFusion::queryDistance (nearest)");
    main.waitForCompletion();
}

// distance.bin and occupancy.bin of the whole background (setDistanceOutput), in the container of the tsdfs/ dumps;
// with setDistanceNearestOutput also nearest.bin
void EMFusion::writeDistanceField(const std::string& dir) {
    Vec3i lo, n;  // the whole background; the world extent with setQueryExtent(true)
    resultsBox("writeDistanceField", lo, n);
    const float voxel = background.getVoxelSize();
    const int cap = metresToVoxels(distanceCapMetres_, voxel);
    const uint32_t sites = (1u << EMF_OCC_OCCUPIED) | (distanceUnknownObstacle_ ? 1u << EMF_OCC_UNKNOWN : 0u);
    const DistanceField& df = distanceField(lo, n, sites, cap, {}, true, expDistanceNearest_);
    const size_t voxels = static_cast<size_t>(n[0]) * n[1] * n[2];
    std::vector<float> metres(voxels);
    std::vector<uint8_t> classes(voxels);
    hipCheck(hipMemcpyAsync(metres.data(), df.metres, voxels * sizeof(float), hipMemcpyDeviceToHost, main.get()),
             "EMFusion::writeDistanceField (metres)");
    hipCheck(hipMemcpyAsync(classes.data(), df.classes, voxels, hipMemcpyDeviceToHost, main.get()),
             "EMFusion::writeDistanceField (classes)");
    main.waitForCompletion();
    io::writeVolume(dir + "/distance.bin", metres.data(), sizeof(float), n, voxel);
    io::writeVolume(dir + "/occupancy.bin", classes.data(), sizeof(uint8_t), n, voxel);
    if (expDistanceNearest_) {
        std::vector<int32_t> nearest(voxels);
        hipCheck(hipMemcpyAsync(nearest.data(), df.nearest, voxels * sizeof(int32_t), hipMemcpyDeviceToHost, main.get()),
                 "EMFusion::writeDistanceField (nearest)");
        main.waitForCompletion();
        io::writeVolume(dir + "/nearest.bin", nearest.data(), sizeof(int32_t), n, voxel);
    }
}

}  // namespace emf
