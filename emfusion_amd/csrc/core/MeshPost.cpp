// MeshPost.cpp -- the mesh post-passes as one chain (MeshPost.hpp).
#include "MeshPost.hpp"

#include <algorithm>
#include <string>

namespace emf {
namespace {

template <typename T>
T* at(const DeviceBuffer& b, size_t offset) {
    return reinterpret_cast<T*>(static_cast<char*>(b.data()) + offset);
}

void check(int rc, const char* who, const char* step) { emfCheck(rc, (std::string(who) + " (" + step + ")").c_str()); }

[[noreturn]] void beyond(const char* who, uint64_t count, const char* what) {
    throw HipError(std::string(who) + ": " + std::to_string(count) + " " + what, EMF_E_LIMIT);
}

template <typename T>
void fetch(std::vector<T>& host, const T* dev, const Stream& s, const char* what) {
    hipCheck(hipMemcpyAsync(host.data(), dev, sizeof(T) * host.size(), hipMemcpyDeviceToHost, s.get()), what);
}

// the arrays a pass writes, in one arena with one spare element each: [vertices][normals][triangles][colours]
struct Arrays {
    float* v;
    float* n;
    int32_t* t;  // nullptr without `triangles`: the pass rewrites them in place
    uint8_t* c;  // nullptr without `colours`
};

Arrays arraysIn(DeviceBuffer& arena, uint64_t nv, uint64_t nt, bool triangles, bool colours) {
    const size_t v1 = std::max<uint64_t>(nv, 1), t1 = std::max<uint64_t>(nt, 1);
    Carve c;
    const size_t ov = c.take<float>(3 * v1), on = c.take<float>(3 * v1), ot = c.take<int32_t>(triangles ? 4 * t1 : 0),
                 oc = c.take<uint8_t>(colours ? 3 * v1 : 0);
    arena.reserve(c.off);
    return Arrays{at<float>(arena, ov), at<float>(arena, on), triangles ? at<int32_t>(arena, ot) : nullptr,
                  colours ? at<uint8_t>(arena, oc) : nullptr};
}

}  // namespace

MeshPost::Result MeshPost::run(const Stream& s, const Soup& soup, const Table& table, const Request& req, const char* who) {
    const int n = table.n;
    const bool batched = table.basesDev != nullptr;  // else the one-model entries: the table entries with null bases
    const uint64_t nv = soup.nv, nt = soup.nt;
    const bool colours = soup.c != nullptr;
    Result r;

    // ---- weld: [welded bases u64 x (MAX + 1)][welded counts u32 x MAX][scratch]
    const size_t weldBytes = emf_hip_meshWeldScratchBytes(nv);
    if (weldBytes == 0) beyond(who, nv, "soup vertices");
    Carve wc;
    const size_t oWBases = wc.take<uint64_t>(EMF_MAX_MODELS + 1), oWCounts = wc.take<uint32_t>(EMF_MAX_MODELS),
                 oWeld = wc.take<char>(weldBytes);
    weldScratch.reserve(wc.off);
    uint64_t* wBasesDev = at<uint64_t>(weldScratch, oWBases);
    uint32_t* wCountsDev = at<uint32_t>(weldScratch, oWCounts);
    void* weld = at<char>(weldScratch, oWeld);
    std::vector<uint32_t> wCounts(n);
    std::vector<uint64_t> wBases(n + 1);
    if (batched) {
        check(emf_hip_meshWeldCountBatched(soup.keys, nv, table.basesDev, n, weld, wCountsDev, wBasesDev, s.abi()), who, "weld count");
        fetch(wCounts, wCountsDev, s, "welded counts D2H");
        fetch(wBases, wBasesDev, s, "welded bases D2H");
    } else {
        check(emf_hip_meshWeldCount(soup.keys, nv, weld, wCountsDev, s.abi()), who, "weld count");
        fetch(wCounts, wCountsDev, s, "welded counts D2H");
    }
    check(emf_hip_meshWeldStatus(weld, nv, s.abi()), who, "weld table");  // waits: the welded sizes
    const uint64_t nw = batched ? wBases[n] : wCounts[0];
    const Arrays w = arraysIn(weldArena, nw, 0, false, colours);
    if (batched)
        check(emf_hip_meshWeldEmitBatched(weld, nv, nt, table.basesDev, wBasesDev, n, soup.v, soup.n, soup.c, soup.t, w.v, w.n,
                                          w.c, soup.t, s.abi()),
              who, "weld emit");
    else
        check(emf_hip_meshWeldEmit(weld, nv, nt, soup.v, soup.n, soup.c, soup.t, w.v, w.n, w.c, soup.t, s.abi()), who, "weld emit");
    r.mesh = DeviceMesh{w.v, w.n, soup.t, w.c, nw, nt};
    r.slices = slicesOfWeld(n, batched ? wBases.data() : nullptr, wCounts.data(), table.bases, nt);

    // ---- label / filter: [kept bases u64 x 2 (MAX + 1)][kept counts u32 x 2 MAX][components u32 x MAX]
    //      [kept components u32 x MAX][scratch]
    if (req.filter || req.components) {
        const size_t ccBytes = emf_hip_meshComponentsScratchBytes(nw, nt);
        if (ccBytes == 0) beyond(who, nw, "welded vertices");
        Carve fc;
        const size_t oKBases = fc.take<uint64_t>(2 * (EMF_MAX_MODELS + 1)), oKCounts = fc.take<uint32_t>(2 * EMF_MAX_MODELS),
                     oComps = fc.take<uint32_t>(EMF_MAX_MODELS), oKComps = fc.take<uint32_t>(EMF_MAX_MODELS),
                     oCc = fc.take<char>(ccBytes);
        filterScratch.reserve(fc.off);
        uint64_t* kBasesDev = at<uint64_t>(filterScratch, oKBases);
        uint32_t* kCountsDev = at<uint32_t>(filterScratch, oKCounts);
        uint32_t* compsDev = at<uint32_t>(filterScratch, oComps);
        uint32_t* kCompsDev = at<uint32_t>(filterScratch, oKComps);
        void* cc = at<char>(filterScratch, oCc);
        int32_t* labelsDev = nullptr;
        uint32_t* sizesDev = nullptr;
        if (req.components) {
            labels.reserve(std::max<size_t>(nw, 1) * sizeof(int32_t));
            sizes.reserve(std::max<size_t>(nw, 1) * sizeof(uint32_t));
            labelsDev = labels.as<int32_t>();
            sizesDev = sizes.as<uint32_t>();
        }
        if (batched)
            check(emf_hip_meshComponentsLabelBatched(soup.t, nw, nt, table.basesDev, wBasesDev, n, cc, labelsDev, sizesDev, s.abi()),
                  who, "label");
        else
            check(emf_hip_meshComponentsLabel(soup.t, nw, nt, cc, labelsDev, sizesDev, s.abi()), who, "label");
        if (req.components) {
            check(emf_hip_meshComponentsStatus(cc, nw, nt, s.abi()), who, "components");  // waits
            req.components->labels.resize(nw);
            req.components->sizes.resize(nw);
            if (nw) {
                hipCheck(hipMemcpy(req.components->labels.data(), labelsDev, nw * sizeof(int32_t), hipMemcpyDeviceToHost), "labels D2H");
                hipCheck(hipMemcpy(req.components->sizes.data(), sizesDev, nw * sizeof(uint32_t), hipMemcpyDeviceToHost), "sizes D2H");
            }
        }
        if (req.filter) {
            std::vector<uint32_t> mins(n);
            std::vector<uint8_t> largest(n);
            for (int k = 0; k < n; ++k) {
                mins[k] = req.perModel[k].minTriangles;
                largest[k] = req.perModel[k].largestOnly ? 1 : 0;
            }
            std::vector<uint64_t> kBases(2 * (n + 1));
            std::vector<uint32_t> kCounts(2 * n), comps(n), kComps(n);
            if (batched) {
                check(emf_hip_meshComponentsFilterCountBatched(soup.t, nw, nt, table.basesDev, wBasesDev, n, cc, mins.data(),
                                                               largest.data(), kCountsDev, kBasesDev, compsDev, kCompsDev, s.abi()),
                      who, "filter count");
                fetch(kBases, kBasesDev, s, "kept bases D2H");
            } else {
                check(emf_hip_meshComponentsFilterCount(soup.t, nw, nt, cc, mins.data(), largest.data(), kCountsDev, compsDev,
                                                        kCompsDev, s.abi()),
                      who, "filter count");
            }
            fetch(kCounts, kCountsDev, s, "kept counts D2H");
            fetch(comps, compsDev, s, "components D2H");
            fetch(kComps, kCompsDev, s, "kept components D2H");
            check(emf_hip_meshComponentsStatus(cc, nw, nt, s.abi()), who, "filter indices");  // waits
            const std::vector<MeshSlice> kept = slicesOf(n, batched ? kBases.data() : nullptr, kCounts.data());
            const uint64_t knv = kept.back().v0 + kept.back().vc, knt = kept.back().t0 + kept.back().tc;
            const Arrays k = arraysIn(filterArena, knv, knt, true, colours);
            if (batched)
                check(emf_hip_meshComponentsEmitBatched(cc, nw, nt, table.basesDev, wBasesDev, n, w.v, w.n, w.c, soup.t, k.v, k.n,
                                                        k.c, k.t, s.abi()),
                      who, "filter emit");
            else
                check(emf_hip_meshComponentsEmit(cc, nw, nt, w.v, w.n, w.c, soup.t, k.v, k.n, k.c, k.t, s.abi()), who, "filter emit");
            r.filterStats.resize(n);
            for (int i = 0; i < n; ++i)
                r.filterStats[i] = MeshFilterStats{comps[i], kComps[i], static_cast<uint32_t>(r.slices[i].tc),
                                                   static_cast<uint32_t>(kept[i].tc), {}};
            r.mesh = DeviceMesh{k.v, k.n, k.t, k.c, knv, knt};
            r.slices = kept;
        }
    }

    // ---- simplify: [triangle bases u64 x 2 (MAX + 1)][vertex bases u64 x (MAX + 1)][kept bases u64 x 2 (MAX + 1)]
    //      [kept counts u32 x 2 MAX][clusters u32 x MAX][scratch]
    if (req.simplify) r.simplifyStats.assign(n, MeshSimplifyStats{});
    if (req.simplify && r.mesh.nv != 0) {
        const DeviceMesh in = r.mesh;
        const size_t spBytes = emf_hip_meshSimplifyScratchBytes(in.nv, in.nt);
        if (spBytes == 0) beyond(who, in.nv, "vertices to simplify");
        Carve sc;
        const size_t oTBases = sc.take<uint64_t>(2 * (EMF_MAX_MODELS + 1)), oVBases = sc.take<uint64_t>(EMF_MAX_MODELS + 1),
                     oSBases = sc.take<uint64_t>(2 * (EMF_MAX_MODELS + 1)), oSCounts = sc.take<uint32_t>(2 * EMF_MAX_MODELS),
                     oClusters = sc.take<uint32_t>(EMF_MAX_MODELS), oSp = sc.take<char>(spBytes);
        simplifyScratch.reserve(sc.off);
        uint64_t* tBasesDev = batched ? at<uint64_t>(simplifyScratch, oTBases) : nullptr;
        uint64_t* vBasesDev = batched ? at<uint64_t>(simplifyScratch, oVBases) : nullptr;
        uint64_t* sBasesDev = batched ? at<uint64_t>(simplifyScratch, oSBases) : nullptr;
        uint32_t* sCountsDev = at<uint32_t>(simplifyScratch, oSCounts);
        uint32_t* clustersDev = at<uint32_t>(simplifyScratch, oClusters);
        void* sp = at<char>(simplifyScratch, oSp);
        std::vector<uint64_t> tBases, vBases;  // the bases of what the weld (or the filter) left; read by the upload
        if (batched) {                         // until the Status call below has waited
            basesOf(r.slices, in.nv, in.nt, tBases, vBases);
            hipCheck(hipMemcpyAsync(tBasesDev, tBases.data(), sizeof(uint64_t) * tBases.size(), hipMemcpyHostToDevice, s.get()),
                     "simplify triangle bases upload");
            hipCheck(hipMemcpyAsync(vBasesDev, vBases.data(), sizeof(uint64_t) * vBases.size(), hipMemcpyHostToDevice, s.get()),
                     "simplify vertex bases upload");
        }
        std::vector<float> cells(n);
        for (int k = 0; k < n; ++k) cells[k] = req.perModel[k].simplifyCell;
        check(emf_hip_meshSimplifyCount(in.v, in.n, in.c, in.t, in.nv, in.nt, tBasesDev, vBasesDev, n, cells.data(), nullptr, sp,
                                        sCountsDev, sBasesDev, clustersDev, s.abi()),
              who, "simplify count");
        std::vector<uint64_t> sBases(2 * (n + 1));
        std::vector<uint32_t> sCounts(2 * n), clusters(n);
        if (batched) fetch(sBases, sBasesDev, s, "simplified bases D2H");
        fetch(sCounts, sCountsDev, s, "simplified counts D2H");
        fetch(clusters, clustersDev, s, "clusters D2H");
        check(emf_hip_meshSimplifyStatus(sp, in.nv, in.nt, s.abi()), who, "simplify");  // waits; the uploads too
        const std::vector<MeshSlice> kept = slicesOf(n, batched ? sBases.data() : nullptr, sCounts.data());
        const uint64_t snv = kept.back().v0 + kept.back().vc, snt = kept.back().t0 + kept.back().tc;
        const Arrays k = arraysIn(simplifyArena, snv, snt, true, colours);
        check(emf_hip_meshSimplifyEmit(sp, in.nv, in.nt, tBasesDev, vBasesDev, n, in.v, in.n, in.c, in.t, k.v, k.n, k.c, k.t, s.abi()),
              who, "simplify emit");
        for (int i = 0; i < n; ++i)
            r.simplifyStats[i] = MeshSimplifyStats{static_cast<uint32_t>(r.slices[i].vc), static_cast<uint32_t>(r.slices[i].tc),
                                                   static_cast<uint32_t>(kept[i].vc), static_cast<uint32_t>(kept[i].tc), clusters[i]};
        r.mesh = DeviceMesh{k.v, k.n, k.t, k.c, snv, snt};
        r.slices = kept;
    }
    return r;
}

void MeshPost::download(const Stream& s, const DeviceMesh& m, const std::vector<MeshSlice>& slices, Mesh* out) {
    const size_t vb = 3 * sizeof(float) * m.nv;
    stage.grow(2 * vb + 4 * sizeof(int32_t) * std::max<uint64_t>(m.nt, 1));
    float* vHost = stage.as<float>();
    float* nHost = vHost + 3 * m.nv;
    int32_t* tHost = reinterpret_cast<int32_t*>(nHost + 3 * m.nv);
    if (m.nv) {
        hipCheck(hipMemcpyAsync(vHost, m.v, vb, hipMemcpyDeviceToHost, s.get()), "mesh vertices D2H");
        hipCheck(hipMemcpyAsync(nHost, m.n, vb, hipMemcpyDeviceToHost, s.get()), "mesh normals D2H");
    }
    if (m.nt) hipCheck(hipMemcpyAsync(tHost, m.t, 4 * sizeof(int32_t) * m.nt, hipMemcpyDeviceToHost, s.get()), "mesh triangles D2H");
    std::vector<uint8_t> cHost;
    if (m.c && m.nv) {
        cHost.resize(3 * m.nv);
        hipCheck(hipMemcpyAsync(cHost.data(), m.c, 3 * m.nv, hipMemcpyDeviceToHost, s.get()), "mesh colours D2H");
    }
    s.waitForCompletion();
    for (size_t k = 0; k < slices.size(); ++k) {  // model k's slice is its own mesh (local triangle indices)
        const MeshSlice& c = slices[k];
        Mesh& mesh = out[k];
        mesh.cloud.assign(vHost + 3 * c.v0, vHost + 3 * (c.v0 + c.vc));
        mesh.normals.assign(nHost + 3 * c.v0, nHost + 3 * (c.v0 + c.vc));
        mesh.polygons.assign(tHost + 4 * c.t0, tHost + 4 * (c.t0 + c.tc));
        if (!cHost.empty()) mesh.colors.assign(cHost.begin() + 3 * c.v0, cHost.begin() + 3 * (c.v0 + c.vc));
    }
}

}  // namespace emf
