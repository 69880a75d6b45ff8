// Checkpoint.cpp -- EMFusion::saveCheckpoint / loadCheckpoint / checkpointInfo (see EMFusion.hpp).
//
// The file (little-endian, every block a multiple of 8 bytes):
//   header   char magic[8] "EMFCKPT\0"; u32 version (1; 2 once the background has been rolled; 3 with the background store on); u32 headerBytes; the Params block (putParams below: 56 words);
//            u64 FNV-1a of every header byte before it
//   sections {u32 tag; i32 id; u32 which; u32 0; u64 payloadBytes} + payload, zero-padded to 8 bytes:
//     "SESS"  frame count, nextId, colour on/off, camera pose, allIds, the visible set, the colour map
//     "OBJ "  per live object, creation order (id): resolution, voxel size, truncation, pose, exCount / nonExCount,
//             class scores
//     "LOGS"  poses, obj_poses, obj_pose_offsets
//     "MESH"  per kept mesh of a deleted object (id)
//     "PACK"  one packed record (include/emf_hip.h "Packed buffers") per volume buffer: id 0 = background, `which` an
//             emf_fusion_volume selector -- tsdf, weights, [colour] of the background, then tsdf, weights, fg/bg counts,
//             [colour] of every object in creation order; always the FRONT copy
//     "ROLL"  version 2 only, exactly once, behind the last packed record: the background's cumulative origin, the
//             follow switch and parameters, the background's current pose, the retired slabs.  A session that has never
//             rolled writes version 1, byte for byte the file it always wrote
//     "TILE"  version 3 only (a session with the background store on; its "ROLL" section is always
//             present), exactly once, behind the roll section: u32 store on; u32 the background has rolled; u64 budget;
//             u64 tiles held, bytes held, tiles spilled, restored, evicted; u64 last spill sequence; u64 tile count;
//             then per stored tile, in store order: i32 lattice coordinate x y z; u64 spill sequence; u8 class x 3;
//             u8 0; u32 word x 4 (40 bytes) and its literal arrays (8 KiB per unit).  A session with the store off
//             writes version 1 or 2, byte for byte the file it always wrote
//     "END!"  empty; the file ends behind it
// Saved: the PRIMARY state.  Not saved because derived, rebuilt by the load the way ObjTSDF::resize and reset() do
// (TSDF::volumesWritten, rebuildModelTable): fgProbs / fgVolMask, materialised gradients, sign maps, tile lists, dirty
// maps, brick flags, the back copy.  Not saved because they belong to the process that made them: the debug image logs
// of setupOutput, per-frame meshes and the volumes kept of deleted objects (savedVolumes).  Not saved because the
// caller sets them again, as at start: tracking, clean-up, preprocess, ignore_person, weld, views, the pose log switch.
// The accelerators never change a result, so a restored session continues with the bytes of one that
// was never interrupted (tests/test_gpu_checkpoint.py).
//
// A volume moves through a bounded device arena and ONE pinned slab of at most 64 MiB (emf::PinnedBuffer), never
// through a second copy of itself: classify + rank on the device, the class array and the uniform words come over in
// slab-sized pieces, the literals rank range by rank range (emf_hip_packGather).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>

#include "EMFusion.hpp"
#include "EMFusionDetail.hpp"
#include "emf_fusion.h"

namespace emf {

namespace {

constexpr char kMagic[8] = {'E', 'M', 'F', 'C', 'K', 'P', 'T', '\0'};
constexpr uint32_t kVersion = 1, kVersionRolled = 2, kVersionStore = 3;
constexpr uint32_t kParamWords = 56;
constexpr uint32_t kHeaderBytes = 16 + 4 * kParamWords + 8;
constexpr uint64_t kChunk = 1024;
constexpr size_t kSlabBytes = 64u << 20;  // pinned staging, and the device arena of the literals

constexpr uint32_t fourcc(char a, char b, char c, char d) {
    return static_cast<uint32_t>(static_cast<uint8_t>(a)) | static_cast<uint32_t>(static_cast<uint8_t>(b)) << 8 |
           static_cast<uint32_t>(static_cast<uint8_t>(c)) << 16 | static_cast<uint32_t>(static_cast<uint8_t>(d)) << 24;
}
constexpr uint32_t kSess = fourcc('S', 'E', 'S', 'S'), kObj = fourcc('O', 'B', 'J', ' '), kLogs = fourcc('L', 'O', 'G', 'S'),
                   kMesh = fourcc('M', 'E', 'S', 'H'), kPack = fourcc('P', 'A', 'C', 'K'), kEnd = fourcc('E', 'N', 'D', '!'),
                   kRoll = fourcc('R', 'O', 'L', 'L'), kTile = fourcc('T', 'I', 'L', 'E');
constexpr uint32_t kVolFgBg = 6;  // EMF_VOL_FGBG

struct SectionHeader {
    uint32_t tag;
    int32_t id;
    uint32_t which;
    uint32_t zero;
    uint64_t bytes;
};
static_assert(sizeof(SectionHeader) == 24, "section header layout");

struct RecordHeader {
    uint64_t nbytes;
    uint32_t nchunks, nuniform, nliteral, zero;
};
static_assert(sizeof(RecordHeader) == 24, "packed record header layout");

inline uint64_t pad8(uint64_t n) { return (n + 7) / 8 * 8; }
inline uint64_t recordBytes(const RecordHeader& r) {
    return 24 + pad8(r.nchunks) + pad8(4ull * r.nuniform) + kChunk * r.nliteral;
}

[[noreturn]] void refuse(const std::string& path, const std::string& why) {
    throw HipError("checkpoint " + path + ": " + why, EMF_E_ARG);
}

uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

// ---- byte blobs of the small sections ----
struct Blob {
    std::vector<uint8_t> b;
    template <typename T>
    void put(const T& v) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
        b.insert(b.end(), p, p + sizeof(T));
    }
    void putBytes(const void* p, size_t n) {
        const uint8_t* q = static_cast<const uint8_t*>(p);
        b.insert(b.end(), q, q + n);
    }
    void putPose(const Affine3f& a) {
        putBytes(a.rotation().val, 9 * sizeof(float));
        putBytes(a.translation().val, 3 * sizeof(float));
    }
    void pad() { b.resize(pad8(b.size()), 0); }
};

struct Cursor {
    const uint8_t* p;
    const uint8_t* end;
    const std::string& path;
    void need(size_t n) const {
        if (static_cast<size_t>(end - p) < n) refuse(path, "a section is shorter than its contents");
    }
    template <typename T>
    T get() {
        need(sizeof(T));
        T v;
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
    void getBytes(void* dst, size_t n) {
        need(n);
        std::memcpy(dst, p, n);
        p += n;
    }
    // a count of items of at least `each` bytes that are still to come
    size_t count(size_t each) {
        const int32_t n = get<int32_t>();
        if (n < 0 || static_cast<size_t>(n) > static_cast<size_t>(end - p) / (each ? each : 1)) refuse(path, "a count exceeds its section");
        return static_cast<size_t>(n);
    }
    Affine3f getPose() {
        float r[9], t[3];
        getBytes(r, sizeof(r));
        getBytes(t, sizeof(t));
        return Affine3f(Matx33f(r), Vec3f(t[0], t[1], t[2]));
    }
};

void putParams(Blob& o, const Params& p, bool materialized) {
    const size_t at = o.b.size();
    o.put<int32_t>(p.frameSize.width);
    o.put<int32_t>(p.frameSize.height);
    o.putBytes(p.intr.val, 9 * sizeof(float));
    o.put<float>(p.bilateral_sigma_depth);
    o.put<float>(p.bilateral_sigma_spatial);
    o.put<int32_t>(p.bilateral_kernel_size);
    o.putBytes(p.globalVolumeDims.val, 3 * sizeof(int32_t));
    o.put<float>(p.globalVoxelSize);
    o.put<float>(p.globalRelTruncDist);
    o.putBytes(p.objVolumeDims.val, 3 * sizeof(int32_t));
    o.put<float>(p.objRelTruncDist);
    o.putPose(p.volumePose);
    o.put<float>(p.volPad);
    o.put<int32_t>(p.maxTrackingIter);
    o.put<int32_t>(p.maskRCNNFrames);
    o.put<float>(p.existenceThresh);
    o.put<float>(p.volIOUThresh);
    o.put<float>(p.matchIOUThresh);
    o.put<float>(p.distanceThresh);
    o.put<int32_t>(p.visibilityThresh);
    o.put<float>(p.assocThresh);
    o.put<int32_t>(p.boundary);
    o.put<float>(p.tsdfParams.tau);
    o.put<float>(p.tsdfParams.eps1);
    o.put<float>(p.tsdfParams.eps2);
    o.put<float>(p.tsdfParams.nu_init);
    o.put<float>(p.tsdfParams.huberThresh);
    o.put<float>(p.tsdfParams.maxTSDFWeight);
    o.put<float>(p.tsdfParams.assocSigma);
    o.put<float>(p.tsdfParams.alpha);
    o.put<float>(p.tsdfParams.uniPrior);
    o.put<int32_t>(p.ignore_person ? 1 : 0);
    o.put<int32_t>(materialized ? 1 : 0);
    if (o.b.size() - at != 4 * kParamWords) throw std::logic_error("checkpoint: Params block size");
}

void getParams(Cursor& c, Params& p, bool& materialized) {
    p.frameSize.width = c.get<int32_t>();
    p.frameSize.height = c.get<int32_t>();
    c.getBytes(p.intr.val, 9 * sizeof(float));
    p.bilateral_sigma_depth = c.get<float>();
    p.bilateral_sigma_spatial = c.get<float>();
    p.bilateral_kernel_size = c.get<int32_t>();
    c.getBytes(p.globalVolumeDims.val, 3 * sizeof(int32_t));
    p.globalVoxelSize = c.get<float>();
    p.globalRelTruncDist = c.get<float>();
    c.getBytes(p.objVolumeDims.val, 3 * sizeof(int32_t));
    p.objRelTruncDist = c.get<float>();
    p.volumePose = c.getPose();
    p.volPad = c.get<float>();
    p.maxTrackingIter = c.get<int32_t>();
    p.maskRCNNFrames = c.get<int32_t>();
    p.existenceThresh = c.get<float>();
    p.volIOUThresh = c.get<float>();
    p.matchIOUThresh = c.get<float>();
    p.distanceThresh = c.get<float>();
    p.visibilityThresh = c.get<int32_t>();
    p.assocThresh = c.get<float>();
    p.boundary = c.get<int32_t>();
    p.tsdfParams.tau = c.get<float>();
    p.tsdfParams.eps1 = c.get<float>();
    p.tsdfParams.eps2 = c.get<float>();
    p.tsdfParams.nu_init = c.get<float>();
    p.tsdfParams.huberThresh = c.get<float>();
    p.tsdfParams.maxTSDFWeight = c.get<float>();
    p.tsdfParams.assocSigma = c.get<float>();
    p.tsdfParams.alpha = c.get<float>();
    p.tsdfParams.uniPrior = c.get<float>();
    p.ignore_person = c.get<int32_t>() != 0;
    materialized = c.get<int32_t>() != 0;
}

// ---- what a file holds, read and checked without a device ----
struct ObjMeta {
    int id = 0;
    Vec3i res;
    float voxelSize = 0.f, truncdist = 0.f;
    Affine3f pose;
    int exCount = 0, nonExCount = 0;
    std::vector<double> scores;
    size_t voxels() const { return static_cast<size_t>(res[0]) * res[1] * res[2]; }
};
struct RecordRef {
    int id = 0;
    uint32_t which = 0;
    uint64_t offset = 0;  // of the record's header in the file
    RecordHeader head{};
};
struct FileIndex {
    Params params;
    bool materialized = false;
    int frameCount = 0, nextId = 1;
    bool colorOn = false;
    Affine3f pose;
    std::vector<int> allIds, visible;
    std::array<uint8_t, 768> colorMap{};
    std::vector<ObjMeta> objects;
    std::map<int, Affine3f> poses;
    std::map<int, std::map<int, Affine3f>> objPoses;
    std::map<int, std::map<int, Vec3f>> objOffsets;
    std::map<int, Mesh> meshes;
    std::vector<RecordRef> records;
    uint64_t fileBytes = 0;
    uint32_t version = kVersion;
    // version 2: the "ROLL" section
    Vec3i origin;
    bool followOn = false;
    BackgroundFollowParams follow;
    Affine3f bgPose;
    std::vector<RetiredSlab> retired;
    // version 3: the "TILE" section
    struct TileRef {
        TileKey key{};
        uint64_t seq = 0;
        uint8_t cls[3] = {0, 0, 0};
        uint32_t words[4] = {0, 0, 0, 0};
        uint64_t offset = 0;  // of its literals in the file
        uint64_t bytes = 0;
    };
    bool storeOn = false, storeRolled = false;
    uint64_t storeBudget = 0, storeSeq = 0;
    TileStore::Counters storeCounters;
    std::vector<TileRef> tiles;
};
constexpr uint64_t kTileHead = 72, kTileRecord = 40;
static_assert(kTileRecord == TileStore::kRecordBytes, "a stored tile costs its checkpoint header plus its literals");

void putMesh(Blob& b, const Mesh& m) {
    b.put<uint64_t>(m.vertices());
    b.put<uint64_t>(m.triangles());
    b.put<uint32_t>(m.colored ? 1 : 0);
    const bool colors = m.colors.size() == 3 * m.vertices() && m.vertices() > 0;
    b.put<uint32_t>(colors ? 1 : 0);
    b.putBytes(m.cloud.data(), m.cloud.size() * sizeof(float));
    b.putBytes(m.normals.data(), m.normals.size() * sizeof(float));
    b.putBytes(m.polygons.data(), m.polygons.size() * sizeof(int32_t));
    if (colors) b.putBytes(m.colors.data(), m.colors.size());
}

Mesh getMesh(Cursor& c, uint64_t sectionBytes, const std::string& path) {
    Mesh m;
    const uint64_t nv = c.get<uint64_t>(), nt = c.get<uint64_t>();
    m.colored = c.get<uint32_t>() != 0;
    const bool colors = c.get<uint32_t>() != 0;
    if (nv > sectionBytes / 24 || nt > sectionBytes / 16) refuse(path, "a mesh exceeds its section");
    m.cloud.resize(3 * nv);
    m.normals.resize(3 * nv);
    m.polygons.resize(4 * nt);
    c.getBytes(m.cloud.data(), m.cloud.size() * sizeof(float));
    c.getBytes(m.normals.data(), m.normals.size() * sizeof(float));
    c.getBytes(m.polygons.data(), m.polygons.size() * sizeof(int32_t));
    if (colors) {
        m.colors.resize(3 * nv);
        c.getBytes(m.colors.data(), m.colors.size());
    }
    return m;
}

struct File {
    FILE* f = nullptr;
    File(const std::string& path, const char* mode) : f(std::fopen(path.c_str(), mode)) {}
    ~File() {
        if (f) std::fclose(f);
    }
    File(const File&) = delete;
    File& operator=(const File&) = delete;
};

void readExact(FILE* f, void* dst, size_t n, const std::string& path) {
    if (n && std::fread(dst, 1, n, f) != n) refuse(path, "truncated");
}
void seekTo(FILE* f, uint64_t off, const std::string& path) {
    if (fseeko(f, static_cast<off_t>(off), SEEK_SET) != 0) refuse(path, "cannot seek");
}

uint64_t expectedBytes(uint32_t which, size_t voxels) {
    switch (which) {
        case EMF_VOL_TSDF:
        case EMF_VOL_WEIGHTS: return voxels * sizeof(float);
        case EMF_VOL_COLOR: return voxels * 4 * sizeof(uint16_t);
        case kVolFgBg: return voxels * 2 * sizeof(float);
        default: return 0;
    }
}

// Reads and checks everything but the uniform words and the literals: header and checksum, every section's length
// against the file's, the order and sizes of the packed records against the object table, every class array against
// its record's counts, the end marker at the end of the file.  headerOnly: stop behind the checksum.
FileIndex scanFile(const std::string& path, bool headerOnly = false) {
    File in(path, "rb");
    if (!in.f) refuse(path, "cannot be opened");
    FileIndex ix;
    if (fseeko(in.f, 0, SEEK_END) != 0) refuse(path, "cannot seek");
    ix.fileBytes = static_cast<uint64_t>(ftello(in.f));
    seekTo(in.f, 0, path);
    uint8_t head[kHeaderBytes];
    if (ix.fileBytes < kHeaderBytes) refuse(path, "truncated (shorter than a header)");
    readExact(in.f, head, kHeaderBytes, path);
    if (std::memcmp(head, kMagic, 8) != 0) refuse(path, "not a checkpoint (magic)");
    uint32_t version, headerBytes;
    std::memcpy(&version, head + 8, 4);
    std::memcpy(&headerBytes, head + 12, 4);
    if (version != kVersion && version != kVersionRolled && version != kVersionStore)
        refuse(path, "format version " + std::to_string(version) + ", this build reads " + std::to_string(kVersion) + ", " +
                         std::to_string(kVersionRolled) + " and " + std::to_string(kVersionStore));
    ix.version = version;
    uint64_t sum;
    std::memcpy(&sum, head + kHeaderBytes - 8, 8);
    if (headerBytes != kHeaderBytes || sum != fnv1a(head, kHeaderBytes - 8)) refuse(path, "header checksum");
    {
        Cursor c{head + 16, head + kHeaderBytes - 8, path};
        getParams(c, ix.params, ix.materialized);
    }
    const Params& p = ix.params;
    auto sane = [](int v) { return v > 0 && v <= 4096; };
    if (!sane(p.frameSize.width) || !sane(p.frameSize.height) || !sane(p.globalVolumeDims[0]) || !sane(p.globalVolumeDims[1]) ||
        !sane(p.globalVolumeDims[2]))
        refuse(path, "parameters out of range");
    if (headerOnly) return ix;

    // the records that must come, in order, once the object table is known
    std::vector<std::pair<int, uint32_t>> expect;
    size_t nextRecord = 0;
    bool sawSess = false, sawLogs = false, sawEnd = false, sawRoll = false, sawTile = false;
    size_t nobjects = 0;
    uint64_t at = kHeaderBytes;
    std::vector<uint8_t> buf;
    while (!sawEnd) {
        SectionHeader sh;
        if (ix.fileBytes - at < sizeof(sh)) refuse(path, "truncated (no end marker)");
        seekTo(in.f, at, path);
        readExact(in.f, &sh, sizeof(sh), path);
        at += sizeof(sh);
        if (sh.zero != 0 || sh.bytes > ix.fileBytes - at || pad8(sh.bytes) > ix.fileBytes - at)
            refuse(path, "truncated (a section runs past the end of the file)");
        const bool small = sh.tag != kPack && sh.tag != kTile;  // (those two are read piece by piece)
        if (small) {
            if (sh.bytes > (1ull << 31)) refuse(path, "a section is implausibly large");
            buf.resize(sh.bytes);
            readExact(in.f, buf.data(), buf.size(), path);
        }
        Cursor c{buf.data(), buf.data() + (small ? buf.size() : 0), path};
        if (sh.tag == kSess) {
            if (sawSess) refuse(path, "two session sections");
            sawSess = true;
            ix.frameCount = c.get<int32_t>();
            ix.nextId = c.get<int32_t>();
            ix.colorOn = c.get<int32_t>() != 0;
            nobjects = c.count(4);
            ix.pose = c.getPose();
            for (size_t k = 0; k < nobjects; ++k) ix.allIds.push_back(c.get<int32_t>());
            const size_t nvis = c.count(4);
            for (size_t k = 0; k < nvis; ++k) ix.visible.push_back(c.get<int32_t>());
            c.getBytes(ix.colorMap.data(), ix.colorMap.size());
            if (ix.frameCount < 0 || ix.nextId < 1 || nobjects > EMF_MAX_MODELS - 1) refuse(path, "session state out of range");
            for (size_t k = 0; k < nobjects; ++k)
                if (ix.allIds[k] < 1 || ix.allIds[k] >= ix.nextId || (k && ix.allIds[k] <= ix.allIds[k - 1]))
                    refuse(path, "object ids are not in creation order");
            expect.push_back({0, EMF_VOL_TSDF});
            expect.push_back({0, EMF_VOL_WEIGHTS});
            if (ix.colorOn) expect.push_back({0, EMF_VOL_COLOR});
        } else if (sh.tag == kObj) {
            if (!sawSess || ix.objects.size() >= nobjects) refuse(path, "an object section out of place");
            ObjMeta o;
            o.id = c.get<int32_t>();
            c.getBytes(o.res.val, sizeof(o.res.val));
            o.voxelSize = c.get<float>();
            o.truncdist = c.get<float>();
            o.pose = c.getPose();
            o.exCount = c.get<int32_t>();
            o.nonExCount = c.get<int32_t>();
            const size_t ns = c.count(8);
            c.get<int32_t>();
            o.scores.resize(ns);
            c.getBytes(o.scores.data(), ns * sizeof(double));
            if (o.id != sh.id || o.id != ix.allIds[ix.objects.size()]) refuse(path, "object table and object sections disagree");
            if (o.res[0] < 2 || o.res[1] < 2 || o.res[2] < 2 || o.res[0] > 4096 || o.res[1] > 4096 || o.res[2] > 4096 ||
                !(o.voxelSize > 0.f) || !(o.truncdist > 0.f))
                refuse(path, "object geometry out of range");
            expect.push_back({o.id, EMF_VOL_TSDF});
            expect.push_back({o.id, EMF_VOL_WEIGHTS});
            expect.push_back({o.id, kVolFgBg});
            if (ix.colorOn) expect.push_back({o.id, EMF_VOL_COLOR});
            ix.objects.push_back(std::move(o));
        } else if (sh.tag == kLogs) {
            if (sawLogs) refuse(path, "two log sections");
            sawLogs = true;
            const size_t np = c.count(52);
            for (size_t k = 0; k < np; ++k) {
                const int fr = c.get<int32_t>();
                ix.poses[fr] = c.getPose();
            }
            const size_t no = c.count(8);
            for (size_t k = 0; k < no; ++k) {
                const int id = c.get<int32_t>();
                auto& log = ix.objPoses[id];
                const size_t n = c.count(52);
                for (size_t j = 0; j < n; ++j) {
                    const int fr = c.get<int32_t>();
                    log[fr] = c.getPose();
                }
            }
            const size_t nf = c.count(8);
            for (size_t k = 0; k < nf; ++k) {
                const int id = c.get<int32_t>();
                auto& log = ix.objOffsets[id];
                const size_t n = c.count(16);
                for (size_t j = 0; j < n; ++j) {
                    const int fr = c.get<int32_t>();
                    float v[3];
                    c.getBytes(v, sizeof(v));
                    log[fr] = Vec3f(v[0], v[1], v[2]);
                }
            }
        } else if (sh.tag == kMesh) {
            ix.meshes[sh.id] = getMesh(c, sh.bytes, path);
        } else if (sh.tag == kRoll) {
            if ((version != kVersionRolled && version != kVersionStore) || sawRoll || sawTile || !sawSess ||
                nextRecord != expect.size())
                refuse(path, "a roll section out of place");
            sawRoll = true;
            c.getBytes(ix.origin.val, sizeof(ix.origin.val));
            ix.followOn = c.get<int32_t>() != 0;
            c.getBytes(ix.follow.step.val, sizeof(ix.follow.step.val));
            ix.follow.lookAhead = c.get<float>();
            ix.follow.keepRetired = c.get<int32_t>() != 0;
            ix.bgPose = c.getPose();
            const size_t ns = c.count(28 + 24);
            for (size_t k = 0; k < ns; ++k) {
                RetiredSlab r;
                r.frame = c.get<int32_t>();
                c.getBytes(r.origin.val, sizeof(r.origin.val));
                c.getBytes(r.res.val, sizeof(r.res.val));
                r.mesh = getMesh(c, sh.bytes, path);
                ix.retired.push_back(std::move(r));
            }
            const int tile[3] = {32, 8, 8};  // as EMFusion::setBackgroundFollow: positive multiples of the tile
            for (int i = 0; i < 3; ++i)
                if (ix.follow.step[i] <= 0 || ix.follow.step[i] % tile[i] != 0) refuse(path, "follow parameters out of range");
            if (!std::isfinite(ix.follow.lookAhead)) refuse(path, "follow parameters out of range");
        } else if (sh.tag == kTile) {
            if (version != kVersionStore || sawTile || !sawRoll) refuse(path, "a tile section out of place");
            sawTile = true;
            if (sh.bytes < kTileHead) refuse(path, "a tile section is shorter than its header");
            uint8_t th[kTileHead];
            readExact(in.f, th, sizeof(th), path);
            Cursor t{th, th + sizeof(th), path};
            ix.storeOn = t.get<uint32_t>() != 0;
            ix.storeRolled = t.get<uint32_t>() != 0;
            ix.storeBudget = t.get<uint64_t>();
            TileStore::Counters& sc = ix.storeCounters;
            sc.tilesHeld = t.get<uint64_t>();
            sc.bytesHeld = t.get<uint64_t>();
            sc.tilesSpilled = t.get<uint64_t>();
            sc.tilesRestored = t.get<uint64_t>();
            sc.tilesEvicted = t.get<uint64_t>();
            ix.storeSeq = t.get<uint64_t>();
            const uint64_t ntiles = t.get<uint64_t>();
            if (!ix.storeOn || ntiles != sc.tilesHeld || ntiles > (sh.bytes - kTileHead) / kTileRecord)
                refuse(path, "a tile section and its counts disagree");
            uint64_t used = kTileHead, held = 0, lastSeq = 0;
            std::set<TileKey> seen;
            for (uint64_t k = 0; k < ntiles; ++k) {
                if (sh.bytes - used < kTileRecord) refuse(path, "a tile section is shorter than its contents");
                uint8_t rec[kTileRecord];
                seekTo(in.f, at + used, path);
                readExact(in.f, rec, sizeof(rec), path);
                used += kTileRecord;
                FileIndex::TileRef r;
                std::memcpy(r.key.data(), rec, 12);
                std::memcpy(&r.seq, rec + 12, 8);
                std::memcpy(r.cls, rec + 20, 3);
                std::memcpy(r.words, rec + 24, 16);
                if (r.cls[0] > 2 || r.cls[1] > 2 || r.cls[2] > 2 || rec[23] != 0) refuse(path, "a stored tile holds an unknown class");
                if ((r.cls[0] | r.cls[1] | r.cls[2]) == 0 || r.seq < lastSeq || r.seq == 0 || r.seq > ix.storeSeq ||
                    !seen.insert(r.key).second)
                    refuse(path, "the stored tiles are not in store order");
                lastSeq = r.seq;
                r.bytes = TileStore::unitsOf(r.cls) * TileStore::kUnitBytes;
                if (sh.bytes - used < r.bytes) refuse(path, "a tile section is shorter than its contents");
                r.offset = at + used;
                used += r.bytes;
                held += kTileRecord + r.bytes;
                ix.tiles.push_back(r);
            }
            if (used != sh.bytes || held != sc.bytesHeld) refuse(path, "a tile section and its counts disagree");
        } else if (sh.tag == kPack) {
            if (sawRoll || ix.objects.size() != nobjects || !sawSess || nextRecord >= expect.size() ||
                expect[nextRecord] != std::make_pair(static_cast<int>(sh.id), sh.which))
                refuse(path, "a packed record out of place");
            RecordRef r;
            r.id = sh.id;
            r.which = sh.which;
            r.offset = at;
            if (sh.bytes < sizeof(RecordHeader)) refuse(path, "a packed record is shorter than its header");
            readExact(in.f, &r.head, sizeof(RecordHeader), path);
            size_t voxels = static_cast<size_t>(p.globalVolumeDims[0]) * p.globalVolumeDims[1] * p.globalVolumeDims[2];
            for (const ObjMeta& o : ix.objects)
                if (o.id == r.id) voxels = o.voxels();
            const RecordHeader& h = r.head;
            if (h.nbytes != expectedBytes(r.which, voxels) || h.nchunks != (h.nbytes + kChunk - 1) / kChunk || h.zero != 0 ||
                h.nuniform > h.nchunks || h.nliteral > h.nchunks || recordBytes(h) != sh.bytes)
                refuse(path, "a packed record does not describe its volume");
            uint64_t counts[3] = {0, 0, 0};
            std::vector<uint8_t> cls(std::min<uint64_t>(h.nchunks, 1u << 20));
            for (uint64_t done = 0; done < h.nchunks; done += cls.size()) {
                const size_t n = static_cast<size_t>(std::min<uint64_t>(cls.size(), h.nchunks - done));
                readExact(in.f, cls.data(), n, path);
                for (size_t k = 0; k < n; ++k) {
                    if (cls[k] > 2) refuse(path, "a class array holds an unknown class");
                    ++counts[cls[k]];
                }
            }
            if (counts[1] != h.nuniform || counts[2] != h.nliteral) refuse(path, "a class array and its counts disagree");
            ix.records.push_back(r);
            ++nextRecord;
        } else if (sh.tag == kEnd) {
            if (sh.bytes != 0) refuse(path, "end marker with a payload");
            sawEnd = true;
        } else {
            refuse(path, "unknown section");
        }
        at += pad8(sh.bytes);
    }
    if (at != ix.fileBytes) refuse(path, "bytes behind the end marker");
    if (!sawSess || !sawLogs || ix.objects.size() != nobjects || nextRecord != expect.size())
        refuse(path, "truncated (sections are missing)");
    if (version == kVersionRolled && !sawRoll) refuse(path, "format version 2 without its roll section");
    if (version == kVersionStore && !sawRoll) refuse(path, "format version 3 without its roll section");
    if (version == kVersionStore && !sawTile) refuse(path, "format version 3 without its tile section");
    return ix;
}

// ---- file writing ----
struct Writer {
    FILE* f;
    const std::string& path;
    double msFile = 0;
    uint64_t written = 0;
    void bytes(const void* p, size_t n) {
        const auto t0 = std::chrono::steady_clock::now();
        if (n && std::fwrite(p, 1, n, f) != n) throw std::runtime_error("checkpoint " + path + ": write failed");
        msFile += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        written += n;
    }
    void padTo8() {
        static const uint8_t zeros[8] = {0};
        bytes(zeros, static_cast<size_t>(pad8(written) - written));
    }
    void section(uint32_t tag, int id, uint32_t which, uint64_t n) {
        const SectionHeader sh{tag, id, which, 0u, n};
        bytes(&sh, sizeof(sh));
    }
    void section(uint32_t tag, int id, Blob& b) {
        section(tag, id, 0, b.b.size());
        bytes(b.b.data(), b.b.size());
        padTo8();
    }
};

// Device arrays of the packer, sized for the largest buffer of the session, the literal arena and the pinned slab
struct Workspace {
    DeviceBuffer classes, words, ranks, uniform, literalChunks, totals, scan, arena;
    PinnedBuffer slab;
    void reserve(uint64_t nbytes) {
        const uint64_t nchunks = (nbytes + kChunk - 1) / kChunk;
        if (classes.bytes() < pad8(nchunks)) {
            classes = DeviceBuffer(pad8(nchunks));
            words = DeviceBuffer(4 * nchunks);
            ranks = DeviceBuffer(4 * nchunks);
            uniform = DeviceBuffer(4 * nchunks);
            literalChunks = DeviceBuffer(4 * nchunks);
        }
        const size_t sb = emf_hip_packScratchBytes(nbytes);
        if (scan.bytes() < sb) scan = DeviceBuffer(sb);
        if (totals.empty()) totals = DeviceBuffer(16);
        const size_t want = static_cast<size_t>(std::min<uint64_t>(kSlabBytes, std::max<uint64_t>(nchunks * kChunk, 4096)));
        if (slab.bytes() < want) {
            slab = PinnedBuffer(want);
            arena = DeviceBuffer(want);
        }
    }
};

double msSince(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// ---- save ----------------------------------------------------------------------------------------------------

CheckpointStats EMFusion::saveCheckpoint(const std::string& path) {
    if (sharded) throw HipError("EMFusion::saveCheckpoint: checkpoints are not available on the sharded path", EMF_E_ARG);
    const auto tStart = std::chrono::steady_clock::now();
    quiesce();
    refreshVisibleFromDevice();
    if (bgInFlight) joinBackground();  // (a frame that threw between fork and join: the integration was its own)
    quiesce();
    CheckpointStats st;
    const std::string tmp = path + ".tmp";
    {
        File out(tmp, "wb");
        if (!out.f) throw HipError("EMFusion::saveCheckpoint: cannot create " + tmp, EMF_E_ARG);
        Writer w{out.f, tmp};
        {
            Blob h;
            h.putBytes(kMagic, 8);
            h.put<uint32_t>(storeOn ? kVersionStore : (bgRolled ? kVersionRolled : kVersion));
            h.put<uint32_t>(kHeaderBytes);
            putParams(h, params, gradMode == TSDF::Gradients::Materialized);
            h.put<uint64_t>(fnv1a(h.b.data(), h.b.size()));
            w.bytes(h.b.data(), h.b.size());
        }
        {
            Blob s;
            s.put<int32_t>(frameCount);
            s.put<int32_t>(nextId);
            s.put<int32_t>(colorOn ? 1 : 0);
            s.put<int32_t>(static_cast<int32_t>(allIds.size()));
            s.putPose(pose);
            for (int id : allIds) s.put<int32_t>(id);
            s.put<int32_t>(static_cast<int32_t>(vis_objs.size()));
            for (int id : vis_objs) s.put<int32_t>(id);
            s.putBytes(colorMap.data(), colorMap.size());
            w.section(kSess, 0, s);
        }
        for (const ObjTSDF& o : objects) {
            Blob b;
            b.put<int32_t>(o.getID());
            const Vec3i res = o.getVolumeRes();
            b.putBytes(res.val, sizeof(res.val));
            b.put<float>(o.getVoxelSize());
            b.put<float>(o.getTruncDist());
            b.putPose(o.getPose());
            b.put<int32_t>(o.existCount());
            b.put<int32_t>(o.nonExistCount());
            b.put<int32_t>(static_cast<int32_t>(o.classScores().size()));
            b.put<int32_t>(0);
            b.putBytes(o.classScores().data(), o.classScores().size() * sizeof(double));
            w.section(kObj, o.getID(), b);
        }
        {
            Blob b;
            b.put<int32_t>(static_cast<int32_t>(poses.size()));
            for (const auto& fp : poses) {
                b.put<int32_t>(fp.first);
                b.putPose(fp.second);
            }
            b.put<int32_t>(static_cast<int32_t>(obj_poses.size()));
            for (const auto& op : obj_poses) {
                b.put<int32_t>(op.first);
                b.put<int32_t>(static_cast<int32_t>(op.second.size()));
                for (const auto& fp : op.second) {
                    b.put<int32_t>(fp.first);
                    b.putPose(fp.second);
                }
            }
            b.put<int32_t>(static_cast<int32_t>(obj_pose_offsets.size()));
            for (const auto& op : obj_pose_offsets) {
                b.put<int32_t>(op.first);
                b.put<int32_t>(static_cast<int32_t>(op.second.size()));
                for (const auto& fo : op.second) {
                    b.put<int32_t>(fo.first);
                    b.putBytes(fo.second.val, 3 * sizeof(float));
                }
            }
            b.pad();
            w.section(kLogs, 0, b);
        }
        for (const auto& im : meshes) {
            const Mesh& m = im.second;
            Blob b;
            putMesh(b, m);
            w.section(kMesh, im.first, b);
        }

        // the volumes: classify + rank on the device, then the three arrays through the slab
        Workspace ws;
        Event e0(hipEventDefault), e1(hipEventDefault), e2(hipEventDefault);
        auto pack = [&](int id, uint32_t which, const void* dev, uint64_t nbytes) {
            ws.reserve(nbytes);
            const uint32_t nchunks = static_cast<uint32_t>((nbytes + kChunk - 1) / kChunk);
            e0.record(main.get());
            emfCheck(emf_hip_packClassify(dev, nbytes, ws.classes.as<uint8_t>(), ws.words.as<uint32_t>(), main.abi()),
                     "packClassify");
            emfCheck(emf_hip_packRank(ws.classes.as<uint8_t>(), ws.words.as<uint32_t>(), nbytes, ws.scan.data(),
                                      ws.ranks.as<uint32_t>(), ws.uniform.as<uint32_t>(), ws.literalChunks.as<uint32_t>(),
                                      ws.totals.as<uint32_t>(), main.abi()),
                     "packRank");
            e1.record(main.get());
            auto t0 = std::chrono::steady_clock::now();
            uint32_t* tot = ws.slab.as<uint32_t>();
            hipCheck(hipMemcpyAsync(tot, ws.totals.data(), 8, hipMemcpyDeviceToHost, main.get()), "hipMemcpyAsync D2H");
            main.waitForCompletion();
            st.msCopy += msSince(t0);
            float ms = 0.f;
            hipCheck(hipEventElapsedTime(&ms, e0.get(), e1.get()), "hipEventElapsedTime");
            st.msClassify += ms;
            const RecordHeader head{nbytes, nchunks, tot[0], tot[1], 0u};
            w.section(kPack, id, which, recordBytes(head));
            w.bytes(&head, sizeof(head));
            // a device array through the slab to the file, zero-padded to 8 bytes
            auto through = [&](const void* src, uint64_t n) {
                for (uint64_t done = 0; done < n; done += ws.slab.bytes()) {
                    const size_t piece = static_cast<size_t>(std::min<uint64_t>(ws.slab.bytes(), n - done));
                    t0 = std::chrono::steady_clock::now();
                    hipCheck(hipMemcpyAsync(ws.slab.data(), static_cast<const char*>(src) + done, piece, hipMemcpyDeviceToHost,
                                            main.get()),
                             "hipMemcpyAsync D2H");
                    main.waitForCompletion();
                    st.msCopy += msSince(t0);
                    w.bytes(ws.slab.data(), piece);
                }
                w.padTo8();
            };
            through(ws.classes.data(), nchunks);
            through(ws.uniform.data(), 4ull * head.nuniform);
            const uint32_t perRange = static_cast<uint32_t>(ws.slab.bytes() / kChunk);
            for (uint32_t first = 0; first < head.nliteral; first += perRange) {
                const uint32_t count = std::min(perRange, head.nliteral - first);
                e1.record(main.get());
                emfCheck(emf_hip_packGather(dev, nbytes, ws.literalChunks.as<uint32_t>(), first, count, ws.arena.data(),
                                            main.abi()),
                         "packGather");
                e2.record(main.get());
                through(ws.arena.data(), kChunk * count);
                hipCheck(hipEventElapsedTime(&ms, e1.get(), e2.get()), "hipEventElapsedTime");
                st.msGather += ms;
            }
            st.rawBytes += nbytes;
            st.chunks[0] += nchunks - head.nuniform - head.nliteral;
            st.chunks[1] += head.nuniform;
            st.chunks[2] += head.nliteral;
            ++st.records;
        };
        auto packVolume = [&](int id, const TSDF& v) {
            pack(id, EMF_VOL_TSDF, v.tsdfPtr(), v.voxels() * sizeof(float));
            pack(id, EMF_VOL_WEIGHTS, v.weightsPtr(), v.voxels() * sizeof(float));
        };
        auto packColor = [&](int id, const TSDF& v) {
            if (!colorOn) return;
            if (!v.hasColor()) throw HipError("EMFusion::saveCheckpoint: a model without its colour volume", EMF_E_ARG);
            pack(id, EMF_VOL_COLOR, v.colorPtr(), v.voxels() * 4 * sizeof(uint16_t));
        };
        packVolume(0, background);
        packColor(0, background);
        for (const ObjTSDF& o : objects) {
            packVolume(o.getID(), o);
            pack(o.getID(), kVolFgBg, o.fgBgPtr(), o.voxels() * 2 * sizeof(float));
            packColor(o.getID(), o);
        }
        if (bgRolled || storeOn) {  // version 2's trailing section; version 3 always has it
            Blob b;
            b.putBytes(bgOrigin.val, sizeof(bgOrigin.val));
            b.put<int32_t>(followOn ? 1 : 0);
            b.putBytes(followParams.step.val, sizeof(followParams.step.val));
            b.put<float>(followParams.lookAhead);
            b.put<int32_t>(followParams.keepRetired ? 1 : 0);
            b.putPose(background.getPose());
            b.put<int32_t>(static_cast<int32_t>(retired.size()));
            for (const RetiredSlab& r : retired) {
                b.put<int32_t>(r.frame);
                b.putBytes(r.origin.val, sizeof(r.origin.val));
                b.putBytes(r.res.val, sizeof(r.res.val));
                putMesh(b, r.mesh);
            }
            b.pad();
            w.section(kRoll, 0, b);
        }
        if (storeOn) {  // version 3's trailing section: the store, tile by tile (never a second copy of it)
            const TileStore::Counters& sc = bgStore.counters();
            const auto tiles = bgStore.inOrder();
            w.section(kTile, 0, 0, kTileHead + sc.bytesHeld);
            Blob b;
            b.put<uint32_t>(1);
            b.put<uint32_t>(bgRolled ? 1 : 0);
            b.put<uint64_t>(bgStore.budget());
            b.put<uint64_t>(sc.tilesHeld);
            b.put<uint64_t>(sc.bytesHeld);
            b.put<uint64_t>(sc.tilesSpilled);
            b.put<uint64_t>(sc.tilesRestored);
            b.put<uint64_t>(sc.tilesEvicted);
            b.put<uint64_t>(bgStore.sequence());
            b.put<uint64_t>(tiles.size());
            w.bytes(b.b.data(), b.b.size());
            for (const auto& t : tiles) {
                Blob r;
                r.putBytes(t.first.data(), 12);
                r.put<uint64_t>(t.second->seq);
                r.putBytes(t.second->cls, 3);
                r.put<uint8_t>(0);
                r.putBytes(t.second->words, 16);
                w.bytes(r.b.data(), r.b.size());
                w.bytes(t.second->literals.data(), t.second->literals.size());
            }
            w.padTo8();
        }
        w.section(kEnd, 0, 0, 0);
        const auto t0 = std::chrono::steady_clock::now();
        if (std::fflush(out.f) != 0) throw std::runtime_error("checkpoint " + tmp + ": write failed");
        st.msFile = w.msFile + msSince(t0);
        st.fileBytes = w.written;
    }
    if (std::rename(tmp.c_str(), path.c_str()) != 0)
        throw HipError("EMFusion::saveCheckpoint: cannot rename " + tmp + " to " + path, EMF_E_ARG);
    st.msTotal = msSince(tStart);
    return st;
}

// ---- load ----------------------------------------------------------------------------------------------------

void EMFusion::loadCheckpoint(const std::string& path) {
    if (sharded) throw HipError("EMFusion::loadCheckpoint: checkpoints are not available on the sharded path", EMF_E_ARG);
    // everything that can refuse the file happens before the session is touched
    const FileIndex ix = scanFile(path);
    const Params& q = ix.params;
    auto same = [](const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; };
    if (q.frameSize.width != params.frameSize.width || q.frameSize.height != params.frameSize.height)
        refuse(path, "saved with another frame size");
    if (!same(q.intr.val, params.intr.val, sizeof(q.intr.val))) refuse(path, "saved with other intrinsics");
    if (!same(q.globalVolumeDims.val, params.globalVolumeDims.val, sizeof(q.globalVolumeDims.val)))
        refuse(path, "saved with another background resolution");
    if (!same(&q.globalVoxelSize, &params.globalVoxelSize, sizeof(float)) ||
        !same(&q.globalRelTruncDist, &params.globalRelTruncDist, sizeof(float)))
        refuse(path, "saved with another background voxel size or truncation distance");
    const TSDFParams &a = q.tsdfParams, &b = params.tsdfParams;
    const float ta[] = {a.tau, a.eps1, a.eps2, a.nu_init, a.huberThresh, a.maxTSDFWeight, a.assocSigma, a.alpha, a.uniPrior};
    const float tb[] = {b.tau, b.eps1, b.eps2, b.nu_init, b.huberThresh, b.maxTSDFWeight, b.assocSigma, b.alpha, b.uniPrior};
    if (!same(ta, tb, sizeof(ta))) refuse(path, "saved with other TSDF parameters");
    if (ix.colorOn && (sw.perVolume || gradMode != TSDF::Gradients::OnTheFly))
        refuse(path, "saved with colour on, which the per-volume path does not support");
    File in(path, "rb");
    if (!in.f) refuse(path, "cannot be opened");

    reset();
    try {
        trackResults.clear();
        lastCreated.clear();
        lastDeleted.clear();
        lastAssigned.clear();
        enableColor(ix.colorOn);  // (frame count 0 here: allowed)
        // the objects, ids in creation order, at the geometry they had (a resized object is created at its last size)
        for (const ObjMeta& o : ix.objects) {
            allIds.push_back(o.id);
            objects.emplace_back(o.id, o.res, o.voxelSize, o.truncdist, o.pose, params.tsdfParams, params.frameSize, gradMode);
            objects.back().restoreBookkeeping(o.exCount, o.nonExCount, o.scores);
            createObj(o.id);
        }
        rebuildModelTable();  // colour volumes of the new objects

        Workspace ws;
        auto unpack = [&](const RecordRef& r, void* dst) {
            const RecordHeader& h = r.head;
            ws.reserve(h.nbytes);
            seekTo(in.f, r.offset + sizeof(RecordHeader), path);
            // a block of the file through the slab into a device array (the file's padding is skipped)
            auto through = [&](void* dev, uint64_t n) {
                for (uint64_t done = 0; done < n; done += ws.slab.bytes()) {
                    const size_t piece = static_cast<size_t>(std::min<uint64_t>(ws.slab.bytes(), n - done));
                    readExact(in.f, ws.slab.data(), piece, path);
                    hipCheck(hipMemcpyAsync(static_cast<char*>(dev) + done, ws.slab.data(), piece, hipMemcpyHostToDevice,
                                            main.get()),
                             "hipMemcpyAsync H2D");
                    main.waitForCompletion();  // the slab is read again
                }
                uint8_t skip[8];
                readExact(in.f, skip, static_cast<size_t>(pad8(n) - n), path);
            };
            through(ws.classes.data(), h.nchunks);
            through(ws.uniform.data(), 4ull * h.nuniform);
            emfCheck(emf_hip_packRank(ws.classes.as<uint8_t>(), nullptr, h.nbytes, ws.scan.data(), ws.ranks.as<uint32_t>(),
                                      nullptr, ws.literalChunks.as<uint32_t>(), ws.totals.as<uint32_t>(), main.abi()),
                     "packRank");
            emfCheck(emf_hip_unpackFill(dst, h.nbytes, ws.classes.as<uint8_t>(), ws.ranks.as<uint32_t>(),
                                        ws.uniform.as<uint32_t>(), h.nuniform, main.abi()),
                     "unpackFill");
            const uint32_t perRange = static_cast<uint32_t>(ws.slab.bytes() / kChunk);
            for (uint32_t first = 0; first < h.nliteral; first += perRange) {
                const uint32_t count = std::min(perRange, h.nliteral - first);
                through(ws.arena.data(), kChunk * count);
                emfCheck(emf_hip_unpackLiterals(dst, h.nbytes, ws.literalChunks.as<uint32_t>(), first, count, ws.arena.data(),
                                                main.abi()),
                         "unpackLiterals");
            }
            main.waitForCompletion();
        };
        for (const RecordRef& r : ix.records) {
            TSDF* vol = r.id == 0 ? static_cast<TSDF*>(&background) : findObject(r.id);
            void* dst = nullptr;
            switch (r.which) {
                case EMF_VOL_TSDF: dst = const_cast<float*>(vol->tsdfPtr()); break;
                case EMF_VOL_WEIGHTS: dst = const_cast<float*>(vol->weightsPtr()); break;
                case EMF_VOL_COLOR: dst = vol->colorPtr(); break;
                default: dst = static_cast<ObjTSDF*>(vol)->fgBgPtr(); break;
            }
            if (!dst) throw HipError("EMFusion::loadCheckpoint: no buffer for a packed record", EMF_E_ARG);
            unpack(r, dst);
        }
        // what is derived from the volumes, as resize() and reset() leave it
        background.volumesWritten(main);
        for (ObjTSDF& o : objects) o.volumesWritten(main);
        pose = ix.pose;
        frameCount = ix.frameCount;
        nextId = ix.nextId;
        colorMap = ix.colorMap;
        vis_objs.clear();
        vis_objs.insert(ix.visible.begin(), ix.visible.end());
        visPending = false;
        poses = ix.poses;
        obj_poses = ix.objPoses;
        obj_pose_offsets = ix.objOffsets;
        meshes = ix.meshes;
        if (ix.version == kVersionRolled || ix.version == kVersionStore) {  // the background where the rolls had taken it
            background.setPose(ix.bgPose);
            bgOrigin = ix.origin;
            bgRolled = ix.version == kVersionRolled || ix.storeRolled;
            followOn = ix.followOn;
            followParams = ix.follow;
            retired = ix.retired;
        }
        if (ix.version == kVersionStore) {  // the store as it was: switch, budget, counters, every tile in its order
            storeOn = true;
            bgStore.restore(ix.storeBudget, ix.storeCounters, ix.storeSeq);
            uint32_t index = 0;
            for (const FileIndex::TileRef& r : ix.tiles) {
                StoredTile t;
                t.seq = r.seq;
                t.index = index++;  // store order is file order
                std::memcpy(t.cls, r.cls, 3);
                std::memcpy(t.words, r.words, 16);
                t.literals.resize(r.bytes);
                seekTo(in.f, r.offset, path);
                readExact(in.f, t.literals.data(), t.literals.size(), path);
                bgStore.restoreTile(r.key, std::move(t));
            }
        }
        forkFrame = -2;
        farBoundsReady = false;
        rebuildModelTable();  // sign maps, tile lists, the visibility gate, the table
        settleReciprocals();
    } catch (...) {
        try {
            reset();  // never a half-restored session
        } catch (...) {
        }
        throw;
    }
}

Params EMFusion::checkpointParams(const std::string& path, bool* materializedGradients) {
    const FileIndex ix = scanFile(path, true);
    if (materializedGradients) *materializedGradients = ix.materialized;
    return ix.params;
}

std::string EMFusion::checkpointInfo(const std::string& path) {
    const FileIndex ix = scanFile(path);
    const Params& p = ix.params;
    std::string s;
    char buf[768];
    auto add = [&](const char* fmt, auto... v) {
        std::snprintf(buf, sizeof(buf), fmt, v...);
        s += buf;
    };
    auto floats = [&](const float* v, int n) {
        s += "[";
        for (int k = 0; k < n; ++k) add(k ? ", %.9g" : "%.9g", static_cast<double>(v[k]));
        s += "]";
    };
    add("{\"version\": %u, \"file_bytes\": %llu, \"frame_index\": %d, \"next_id\": %d, \"color\": %s, ", ix.version,
        static_cast<unsigned long long>(ix.fileBytes), ix.frameCount, ix.nextId, ix.colorOn ? "true" : "false");
    add("\"background_origin\": [%d, %d, %d], \"retired_slabs\": %d, ", ix.origin[0], ix.origin[1], ix.origin[2],
        static_cast<int>(ix.retired.size()));
    add("\"stored_tiles\": %llu, \"stored_bytes\": %llu, ", static_cast<unsigned long long>(ix.tiles.size()),
        static_cast<unsigned long long>(ix.storeCounters.bytesHeld));
    add("\"params\": {\"width\": %d, \"height\": %d, \"K\": ", p.frameSize.width, p.frameSize.height);
    floats(p.intr.val, 9);
    add(", \"bg_res\": [%d, %d, %d], \"bg_voxel_size\": %.9g, \"bg_rel_truncdist\": %.9g, \"volume_pose_t\": ",
        p.globalVolumeDims[0], p.globalVolumeDims[1], p.globalVolumeDims[2], static_cast<double>(p.globalVoxelSize),
        static_cast<double>(p.globalRelTruncDist));
    floats(p.volumePose.translation().val, 3);
    add(", \"obj_res\": [%d, %d, %d], \"obj_rel_truncdist\": %.9g, ", p.objVolumeDims[0], p.objVolumeDims[1],
        p.objVolumeDims[2], static_cast<double>(p.objRelTruncDist));
    add("\"max_tsdf_weight\": %.9g, \"assoc_sigma\": %.9g, \"alpha\": %.9g, \"uni_prior\": %.9g, ",
        static_cast<double>(p.tsdfParams.maxTSDFWeight), static_cast<double>(p.tsdfParams.assocSigma),
        static_cast<double>(p.tsdfParams.alpha), static_cast<double>(p.tsdfParams.uniPrior));
    add("\"visibility_thresh\": %d, \"boundary\": %d, \"mask_frames\": %d, \"materialize_gradients\": %d, "
        "\"max_tracking_iter\": %d, \"ignore_person\": %s}, ",
        p.visibilityThresh, p.boundary, p.maskRCNNFrames, ix.materialized ? 1 : 0, p.maxTrackingIter,
        p.ignore_person ? "true" : "false");
    s += "\"objects\": [";
    for (size_t k = 0; k < ix.objects.size(); ++k) {
        const ObjMeta& o = ix.objects[k];
        add("%s{\"id\": %d, \"res\": [%d, %d, %d], \"voxel_size\": %.9g, \"truncdist\": %.9g, \"ex_count\": %d, "
            "\"non_ex_count\": %d}",
            k ? ", " : "", o.id, o.res[0], o.res[1], o.res[2], static_cast<double>(o.voxelSize),
            static_cast<double>(o.truncdist), o.exCount, o.nonExCount);
    }
    s += "], \"kept_meshes\": [";
    bool firstMesh = true;
    for (const auto& m : ix.meshes) {
        add("%s%d", firstMesh ? "" : ", ", m.first);
        firstMesh = false;
    }
    add("], \"logged_frames\": %d, \"records\": [", static_cast<int>(ix.poses.size()));
    for (size_t k = 0; k < ix.records.size(); ++k) {
        const RecordRef& r = ix.records[k];
        add("%s{\"id\": %d, \"which\": %u, \"offset\": %llu, \"bytes\": %llu, \"packed_bytes\": %llu, \"chunks\": [%u, %u, %u]}",
            k ? ", " : "", r.id, r.which, static_cast<unsigned long long>(r.offset),
            static_cast<unsigned long long>(r.head.nbytes), static_cast<unsigned long long>(recordBytes(r.head)),
            r.head.nchunks - r.head.nuniform - r.head.nliteral, r.head.nuniform, r.head.nliteral);
    }
    s += "]}";
    return s;
}

}  // namespace emf
