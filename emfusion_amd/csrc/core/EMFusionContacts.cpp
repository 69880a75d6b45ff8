// EMFusionContacts.cpp -- emf::EMFusion: object contacts (new behaviour).  Whether two models touch, how
// far apart their surfaces are and whether they interpenetrate: every surface voxel of a probe is taken into a field's
// volume and the field's tsdf is sampled there (emf_hip_contactProbe, one launch for all ordered pairs), the records
// become one summary per unordered pair on the host.  It measures what the volumes say: a tsdf is clamped, so
// min_s == 1 is "at least one truncation distance apart" and no distance.
// contactPose, contactTouch and contactSummary are float64 in the fixed operation order of include/emf_hip.h "Object
// contacts" and need no device.  This unit is compiled with a*b+c contraction off.
#include "EMFusion.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace emf {

void contactPose(const float Ra[9], const float ta[3], const float Rb[9], const float tb[3], float R[9], float t[3]) {
    double A[9], B[9], d[3];
    for (int i = 0; i < 9; ++i) A[i] = static_cast<double>(Ra[i]), B[i] = static_cast<double>(Rb[i]);
    for (int k = 0; k < 3; ++k) d[k] = static_cast<double>(ta[k]) - static_cast<double>(tb[k]);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            double s = B[i] * A[j];
            s = s + B[3 + i] * A[3 + j];
            s = s + B[6 + i] * A[6 + j];
            R[3 * i + j] = static_cast<float>(s);
        }
        double s = B[i] * d[0];
        s = s + B[3 + i] * d[1];
        s = s + B[6 + i] * d[2];
        t[i] = static_cast<float>(s);
    }
}

float contactTouch(double touchMetres, float truncdistB) { return static_cast<float>(touchMetres / static_cast<double>(truncdistB)); }

void contactSummary(const emf_contact_t& ab, const emf_contact_t* ba, const emf_contact_side_t& a, const emf_contact_side_t& b,
                    emf_contact_summary_t& out) {
    std::memset(&out, 0, sizeof(out));
    const uint64_t inside = ab.inside + (ba ? ba->inside : 0), touching = ab.touching + (ba ? ba->touching : 0),
                   sampled = ab.sampled + (ba ? ba->sampled : 0);
    out.state = inside > 0 ? EMF_CONTACT_PENETRATING : touching > 0 ? EMF_CONTACT_TOUCHING : sampled > 0 ? EMF_CONTACT_APART
                                                                                                      : EMF_CONTACT_UNSEEN;
    const double dab = static_cast<double>(ab.min_s) * static_cast<double>(b.truncdist);
    out.distance_m = dab;
    float deciding = ab.min_s;
    if (ba) {
        const double dba = static_cast<double>(ba->min_s) * static_cast<double>(a.truncdist);
        if (dba < dab) out.distance_m = dba, deciding = ba->min_s;
    }
    out.saturated = deciding == 1.f ? 1 : 0;
    out.direction = -1;
    const emf_contact_t* rec = nullptr;
    const emf_contact_side_t* side = nullptr;
    if (ab.touching > 0 && (!ba || ab.touching >= ba->touching)) rec = &ab, side = &a, out.direction = 0;
    else if (ba && ba->touching > 0) rec = ba, side = &b, out.direction = 1;
    if (!rec) return;
    const double vs = static_cast<double>(side->voxelSize), n = static_cast<double>(rec->touching);
    double R[9], t[3], half[3];
    for (int i = 0; i < 9; ++i) R[i] = static_cast<double>(side->R[i]);
    for (int i = 0; i < 3; ++i) {
        t[i] = static_cast<double>(side->t[i]);
        half[i] = (static_cast<double>(side->res[i]) - 1.0) / 2.0;
    }
    auto rotate = [&](const double* p, double* w) {
        for (int i = 0; i < 3; ++i) {
            double s = R[3 * i] * p[0];
            s = s + R[3 * i + 1] * p[1];
            s = s + R[3 * i + 2] * p[2];
            w[i] = s;
        }
    };
    auto toWorld = [&](const double* vox, double* w) {  // voxel coordinates -> the probe's metres -> world
        double o[3];
        for (int j = 0; j < 3; ++j) {
            const double c = vox[j] - half[j];
            o[j] = c * vs;
        }
        rotate(o, w);
        for (int i = 0; i < 3; ++i) w[i] = w[i] + t[i];
    };
    double m[3];
    for (int j = 0; j < 3; ++j) m[j] = static_cast<double>(rec->sum[j]) / n;
    toWorld(m, out.point);
    const double g[3] = {static_cast<double>(rec->gsum[0]), static_cast<double>(rec->gsum[1]), static_cast<double>(rec->gsum[2])};
    double sq = g[0] * g[0];
    sq = sq + g[1] * g[1];
    sq = sq + g[2] * g[2];
    const double len = std::sqrt(sq);
    if (rec->normals > 0 && len > 0.0) {
        const double u[3] = {g[0] / len, g[1] / len, g[2] / len};
        rotate(u, out.normal);
        out.has_normal = 1;
    }
    for (int c = 0; c < 8; ++c) {
        double v[3];
        for (int j = 0; j < 3; ++j) v[j] = static_cast<double>((c >> j) & 1 ? rec->hi[j] : rec->lo[j]);
        toWorld(v, out.corners + 3 * c);
    }
}

const EMFusion::ObjectContacts& EMFusion::objectContacts(const std::vector<int>& ids, bool includeBackground, double touchMetres) {
    if (sharded || world > 1)
        throw HipError("EMFusion::objectContacts: object contacts are not supported on the sharded path", EMF_E_ARG);
    if (std::isnan(touchMetres)) throw HipError("EMFusion::objectContacts: the touch distance is NaN", EMF_E_ARG);
    std::vector<int> all;
    if (includeBackground) all.push_back(0);
    for (int id : ids) {
        if (id <= 0 || !getObject(id)) throw HipError("EMFusion::objectContacts: no object " + std::to_string(id), EMF_E_ARG);
        if (std::find(all.begin(), all.end(), id) != all.end())
            throw HipError("EMFusion::objectContacts: object " + std::to_string(id) + " is named twice", EMF_E_ARG);
        all.push_back(id);
    }
    const int n = static_cast<int>(all.size());
    if (n > EMF_MAX_MODELS) throw HipError("EMFusion::objectContacts: " + std::to_string(n) + " models", EMF_E_LIMIT);
    const size_t nProbes = ids.size(), nPairs = nProbes * static_cast<size_t>(n > 0 ? n - 1 : 0);
    if (nPairs > EMF_CONTACT_MAX_PAIRS)
        throw HipError("EMFusion::objectContacts: " + std::to_string(nPairs) + " ordered pairs, above " +
                           std::to_string(EMF_CONTACT_MAX_PAIRS),
                       EMF_E_LIMIT);
    ObjectContacts out;
    out.ids = all;
    if (nPairs == 0) {
        ctLast = std::move(out);
        return ctLast;
    }
    drainForQuery();
    std::vector<emf_model_t> table(all.size());
    std::vector<int32_t> res(3 * all.size());
    out.sides.resize(all.size());
    for (int k = 0; k < n; ++k) {  // the volumes' current copies (describe() follows the background's flips)
        const TSDF* vol = all[k] == 0 ? static_cast<const TSDF*>(&background) : getObject(all[k]);
        vol->describe(table[k]);
        emf_contact_side_t& s = out.sides[k];
        const Affine3f pose = vol->getPose();
        std::copy(table[k].res, table[k].res + 3, res.begin() + 3 * k);
        std::copy(table[k].res, table[k].res + 3, s.res);
        s.voxelSize = vol->getVoxelSize();
        s.truncdist = vol->getTruncDist();
        std::copy(pose.rotation().val, pose.rotation().val + 9, s.R);
        std::copy(pose.translation().val, pose.translation().val + 3, s.t);
    }
    // the ordered pairs, grouped by probe: every asked object against every other model of the table
    std::vector<emf_contact_pair_t> pairs;
    pairs.reserve(nPairs);
    for (int a = includeBackground ? 1 : 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            if (a == b) continue;
            emf_contact_pair_t p{};
            p.a = a, p.b = b;
            contactPose(out.sides[a].R, out.sides[a].t, out.sides[b].R, out.sides[b].t, p.R, p.t);
            p.touch = contactTouch(touchMetres < 0.0 ? static_cast<double>(out.sides[a].voxelSize) : touchMetres, out.sides[b].truncdist);
            pairs.push_back(p);
        }
    // one device block: the table, the pairs, the records
    const size_t tableBytes = all.size() * sizeof(emf_model_t), pairBytes = pairs.size() * sizeof(emf_contact_pair_t),
                 recBytes = pairs.size() * sizeof(emf_contact_t);
    ctScratch.reserve(tableBytes + pairBytes + recBytes);
    uint8_t* base = ctScratch.as<uint8_t>();
    auto* dTable = reinterpret_cast<emf_model_t*>(base);
    auto* dPairs = reinterpret_cast<emf_contact_pair_t*>(base + tableBytes);
    auto* dRec = reinterpret_cast<emf_contact_t*>(base + tableBytes + pairBytes);
    std::vector<emf_contact_t> rec(pairs.size());
    hipCheck(hipMemcpyAsync(dTable, table.data(), tableBytes, hipMemcpyHostToDevice, main.get()), "EMFusion::objectContacts (table)");
    hipCheck(hipMemcpyAsync(dPairs, pairs.data(), pairBytes, hipMemcpyHostToDevice, main.get()), "EMFusion::objectContacts (pairs)");
    emfCheck(emf_hip_contactProbe(dTable, res.data(), n, dPairs, pairs.data(), static_cast<int32_t>(pairs.size()), dRec, main.abi()),
             "EMFusion::objectContacts (probe)");
    hipCheck(hipMemcpyAsync(rec.data(), dRec, recBytes, hipMemcpyDeviceToHost, main.get()), "EMFusion::objectContacts (records)");
    main.waitForCompletion();
    out.pairs.resize(pairs.size());
    std::vector<int> at(static_cast<size_t>(n) * n, -1);  // (a, b) -> its record
    for (size_t k = 0; k < pairs.size(); ++k) {
        ObjectContact& c = out.pairs[k];
        c.a = all[pairs[k].a], c.b = all[pairs[k].b];
        c.pair = pairs[k];
        c.record = rec[k];
        at[static_cast<size_t>(pairs[k].a) * n + pairs[k].b] = static_cast<int>(k);
    }
    // one summary per unordered pair, in the order of the first record that belongs to it
    for (size_t k = 0; k < pairs.size(); ++k) {
        const int a = pairs[k].a, b = pairs[k].b;
        const int back = at[static_cast<size_t>(b) * n + a];
        if (back >= 0 && static_cast<size_t>(back) < k) continue;  // summarised from the other side
        ObjectContacts::Summary s;
        s.a = all[a], s.b = all[b];
        s.recAB = static_cast<int>(k), s.recBA = back;
        contactSummary(rec[k], back >= 0 ? &rec[back] : nullptr, out.sides[a], out.sides[b], s.summary);
        out.summaries.push_back(s);
    }
    ctLast = std::move(out);
    return ctLast;
}

// contacts.txt (setContactsOutput): after a comment line one line per ordered pair (probe a, field b) with sampled > 0,
// the live objects in id order against each other and the background:
//     a b surface outside unknown masked sampled inside touching normals, the integers, then min_s and the world contact
// point (3) and normal (3) of this record alone in %.9g, zeros where the record has no touching voxel or no normal.
void EMFusion::writeContacts(const std::string& dir) {
    std::vector<int> ids;
    for (const ObjTSDF& obj : objects) ids.push_back(obj.getID());
    std::sort(ids.begin(), ids.end());
    const ObjectContacts found = objectContacts(ids, true, expContactTouch_);
    const std::string path = dir + "/contacts.txt";
    std::FILE* file = std::fopen(path.c_str(), "w");
    if (!file) throw std::runtime_error("EMFusion::writeContacts: cannot create " + path);
    std::fprintf(file, "# a b surface outside unknown masked sampled inside touching normals min_s point_world(3) normal_world(3): "
                       "what the volumes say; min_s 1 is at least one truncation distance, not a distance\n");
    for (const ObjectContact& c : found.pairs) {
        const emf_contact_t& r = c.record;
        if (r.sampled == 0) continue;
        emf_contact_summary_t s;
        contactSummary(r, nullptr, found.sides[c.pair.a], found.sides[c.pair.b], s);
        std::fprintf(file, "%d %d", c.a, c.b);
        for (const uint64_t v : {r.surface, r.outside, r.unknown, r.masked, r.sampled, r.inside, r.touching, r.normals})
            std::fprintf(file, " %llu", static_cast<unsigned long long>(v));
        std::fprintf(file, " %.9g", static_cast<double>(r.min_s));
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", s.point[i]);
        for (int i = 0; i < 3; ++i) std::fprintf(file, " %.9g", s.normal[i]);
        std::fprintf(file, "\n");
    }
    std::fclose(file);
}

}  // namespace emf
