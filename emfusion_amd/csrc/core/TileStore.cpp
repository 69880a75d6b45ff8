// TileStore.cpp -- emf::TileStore (see TileStore.hpp).
#include "TileStore.hpp"

#include <algorithm>
#include <cstring>

namespace emf {

namespace {
constexpr size_t kSlabBytes = 64u << 20;  // pinned staging, and the largest device arena of one spill call

// cut `box` until no piece holds more than `cap` tiles: halve z while it can be halved, then y, then x
void cutBox(const TileBox& box, uint64_t cap, std::vector<TileBox>& out) {
    const uint64_t n = static_cast<uint64_t>(box.size[0]) * box.size[1] * static_cast<uint64_t>(box.size[2]);
    if (n == 0) return;
    if (n <= cap) {
        out.push_back(box);
        return;
    }
    const int axis = box.size[2] > 1 ? 2 : (box.size[1] > 1 ? 1 : 0);
    TileBox a = box, b = box;
    a.size[axis] = box.size[axis] / 2;
    b.lo[axis] = box.lo[axis] + a.size[axis];
    b.size[axis] = box.size[axis] - a.size[axis];
    cutBox(a, cap, out);
    cutBox(b, cap, out);
}

struct SpillCall {
    TileBox box;
    uint32_t n = 0;
    DeviceBuffer scratch, classes, words, lits, totals, arena;
};
}  // namespace

void TileStore::clear() {
    tiles.clear();
    order.clear();
    c.tilesHeld = 0;
    c.bytesHeld = 0;
}

void TileStore::erase(std::map<TileKey, StoredTile>::iterator it) {
    c.tilesHeld -= 1;
    c.bytesHeld -= kRecordBytes + it->second.literals.size();
    order.erase({it->second.seq, it->second.index});
    tiles.erase(it);
}

void TileStore::insert(const TileKey& key, uint64_t seq, const uint8_t cls[3], const uint32_t words[4], const uint8_t* literals) {
    if (cls[0] == 0 && cls[1] == 0 && cls[2] == 0) return;
    if (seq != lastSeq) throw HipError("TileStore::insert: not the spill that beginSpill() opened", EMF_E_ARG);
    auto old = tiles.find(key);
    if (old != tiles.end()) erase(old);
    StoredTile t;
    t.seq = seq;
    t.index = nextIndex++;
    std::memcpy(t.cls, cls, 3);
    std::memcpy(t.words, words, 16);
    const size_t bytes = static_cast<size_t>(unitsOf(cls)) * kUnitBytes;
    if (bytes) t.literals.assign(literals, literals + bytes);
    order[{t.seq, t.index}] = key;
    tiles.emplace(key, std::move(t));
    c.tilesHeld += 1;
    c.bytesHeld += kRecordBytes + bytes;
    c.tilesSpilled += 1;
}

void TileStore::endSpill() {
    nextIndex = 0;
    while (c.bytesHeld > maxBytes && !order.empty()) {
        const uint64_t oldest = order.begin()->first.first;
        while (!order.empty() && order.begin()->first.first == oldest) {
            erase(tiles.find(order.begin()->second));
            c.tilesEvicted += 1;
        }
    }
}

bool TileStore::take(const TileKey& key, StoredTile& out) {
    auto it = tiles.find(key);
    if (it == tiles.end()) return false;
    c.tilesHeld -= 1;
    c.bytesHeld -= kRecordBytes + it->second.literals.size();
    order.erase({it->second.seq, it->second.index});
    out = std::move(it->second);
    tiles.erase(it);
    c.tilesRestored += 1;
    return true;
}

std::vector<std::pair<TileKey, const StoredTile*>> TileStore::inOrder() const {
    std::vector<std::pair<TileKey, const StoredTile*>> v;
    v.reserve(order.size());
    for (const auto& o : order) v.emplace_back(o.second, &tiles.at(o.second));
    return v;
}

void TileStore::restore(uint64_t budgetBytes, const Counters& saved, uint64_t seq) {
    clear();
    maxBytes = budgetBytes;
    c = saved;
    c.tilesHeld = 0;
    c.bytesHeld = 0;
    lastSeq = seq;
    nextIndex = 0;
}

void TileStore::restoreTile(const TileKey& key, StoredTile&& t) {
    if (tiles.count(key) || order.count({t.seq, t.index})) throw HipError("TileStore::restoreTile: a tile is stored twice", EMF_E_ARG);
    c.tilesHeld += 1;
    c.bytesHeld += kRecordBytes + t.literals.size();
    order[{t.seq, t.index}] = key;
    tiles.emplace(key, std::move(t));
}

void TileStore::needSlab(size_t bytes) {
    if (slab.bytes() < bytes) slab.grow(bytes);
}

void TileStore::spill(const float* tsdf, const float* weights, const uint16_t* color, const Vec3i& res,
                      const std::vector<TileBox>& boxes, const TileKey& lattice, Stream& stream) {
    const uint64_t perTile = color ? 4 : 2;  // worst case, in units
    std::vector<TileBox> cut;
    for (const TileBox& b : boxes) cutBox(b, kSlabBytes / (perTile * kUnitBytes), cut);
    std::vector<SpillCall> calls(cut.size());
    for (size_t i = 0; i < cut.size(); ++i) {
        SpillCall& s = calls[i];
        s.box = cut[i];
        s.n = static_cast<uint32_t>(s.box.size[0]) * s.box.size[1] * s.box.size[2];
        s.scratch = DeviceBuffer(emf_hip_spillScratchBytes(s.n));
        s.classes = DeviceBuffer(3 * static_cast<size_t>(s.n));
        s.words = DeviceBuffer(16 * static_cast<size_t>(s.n));
        s.lits = DeviceBuffer(12 * static_cast<size_t>(s.n));
        s.totals = DeviceBuffer(4);
        s.arena = DeviceBuffer(s.n * perTile * kUnitBytes);
        emfCheck(emf_hip_spillTiles(tsdf, weights, color, res.val, s.box.lo.val, s.box.size.val, s.scratch.data(),
                                    s.classes.as<uint8_t>(), s.words.as<uint32_t>(), s.lits.as<uint32_t>(), s.totals.as<uint32_t>(),
                                    s.arena.data(), s.n * perTile, stream.abi()),
                 "TileStore::spill");
    }
    stream.waitForCompletion();  // once, for every box
    const uint64_t seq = beginSpill();
    for (SpillCall& s : calls) {
        // headers: classes | words | lits | totals, each 16-byte aligned in the slab
        const size_t oWords = (3 * static_cast<size_t>(s.n) + 15) / 16 * 16, oLits = oWords + 16 * static_cast<size_t>(s.n),
                     oTotals = oLits + (12 * static_cast<size_t>(s.n) + 15) / 16 * 16, headerBytes = oTotals + 16;
        needSlab(std::max<size_t>(headerBytes, 4096));
        char* h = slab.as<char>();
        hipCheck(hipMemcpyAsync(h, s.classes.data(), 3 * static_cast<size_t>(s.n), hipMemcpyDeviceToHost, stream.get()), "hipMemcpyAsync D2H");
        hipCheck(hipMemcpyAsync(h + oWords, s.words.data(), 16 * static_cast<size_t>(s.n), hipMemcpyDeviceToHost, stream.get()), "hipMemcpyAsync D2H");
        hipCheck(hipMemcpyAsync(h + oLits, s.lits.data(), 12 * static_cast<size_t>(s.n), hipMemcpyDeviceToHost, stream.get()), "hipMemcpyAsync D2H");
        hipCheck(hipMemcpyAsync(h + oTotals, s.totals.data(), 4, hipMemcpyDeviceToHost, stream.get()), "hipMemcpyAsync D2H");
        stream.waitForCompletion();
        std::vector<uint8_t> cls(h, h + 3 * static_cast<size_t>(s.n));
        std::vector<uint32_t> words(4 * static_cast<size_t>(s.n)), lits(3 * static_cast<size_t>(s.n));
        std::memcpy(words.data(), h + oWords, 16 * static_cast<size_t>(s.n));
        std::memcpy(lits.data(), h + oLits, 12 * static_cast<size_t>(s.n));
        uint32_t units;
        std::memcpy(&units, h + oTotals, 4);
        const size_t litBytes = static_cast<size_t>(units) * kUnitBytes;  // at most the arena: 64 MiB
        if (litBytes > s.arena.bytes()) throw HipError("TileStore::spill: the literals exceed their arena", EMF_E_LIMIT);
        if (litBytes) {
            needSlab(litBytes);
            hipCheck(hipMemcpyAsync(slab.data(), s.arena.data(), litBytes, hipMemcpyDeviceToHost, stream.get()), "hipMemcpyAsync D2H");
            stream.waitForCompletion();
        }
        const uint8_t* arena = slab.as<uint8_t>();
        uint32_t cand = 0;
        for (int z = 0; z < s.box.size[2]; ++z)
            for (int y = 0; y < s.box.size[1]; ++y)
                for (int x = 0; x < s.box.size[0]; ++x, ++cand) {
                    const uint8_t* k = &cls[3 * static_cast<size_t>(cand)];
                    const uint32_t u = unitsOf(k);
                    // the literals of a candidate are contiguous, tsdf / weights / colour: they start at the first one's unit
                    uint32_t first = 0;
                    for (int a = 0; a < 3; ++a)
                        if (k[a] == 2) {
                            first = lits[3 * static_cast<size_t>(cand) + a];
                            break;
                        }
                    if (u && static_cast<uint64_t>(first) + u > units) throw HipError("TileStore::spill: a literal lies outside the arena", EMF_E_LIMIT);
                    insert(TileKey{lattice[0] + s.box.lo[0] + x, lattice[1] + s.box.lo[1] + y, lattice[2] + s.box.lo[2] + z}, seq, k,
                           &words[4 * static_cast<size_t>(cand)], arena + static_cast<size_t>(first) * kUnitBytes);
                }
    }
    endSpill();
}

TileFill TileStore::takeFill(const std::vector<TileBox>& boxes, const TileKey& lattice, Stream& stream) {
    TileFill f;
    if (tiles.empty()) return f;
    std::vector<int32_t> coords;
    std::vector<uint32_t> words, lits;
    std::vector<StoredTile> found;
    uint64_t units = 0;
    for (const TileBox& b : boxes)
        for (int z = b.lo[2]; z < b.lo[2] + b.size[2]; ++z)
            for (int y = b.lo[1]; y < b.lo[1] + b.size[1]; ++y)
                for (int x = b.lo[0]; x < b.lo[0] + b.size[0]; ++x) {
                    StoredTile t;
                    if (!take(TileKey{lattice[0] + x, lattice[1] + y, lattice[2] + z}, t)) continue;
                    coords.insert(coords.end(), {x, y, z});
                    f.classesHost.insert(f.classesHost.end(), t.cls, t.cls + 3);
                    words.insert(words.end(), t.words, t.words + 4);
                    uint32_t at = static_cast<uint32_t>(units);
                    for (int a = 0; a < 3; ++a) {
                        lits.push_back(t.cls[a] == 2 ? at : 0u);
                        if (t.cls[a] == 2) at += a == 2 ? 2 : 1;
                    }
                    units += unitsOf(t.cls);
                    found.push_back(std::move(t));
                }
    f.n = static_cast<uint32_t>(found.size());
    if (f.n == 0) return f;
    if (units > 0xffffffffull) throw HipError("TileStore::takeFill: more literals than one fill addresses", EMF_E_LIMIT);
    f.arenaUnits = units;
    f.coords = DeviceBuffer(coords.size() * 4);
    f.classes = DeviceBuffer(f.classesHost.size());
    f.words = DeviceBuffer(words.size() * 4);
    f.lits = DeviceBuffer(lits.size() * 4);
    if (units) f.arena = DeviceBuffer(units * kUnitBytes);
    // host -> device through the slab, a piece at a time; the slab is reused only after the piece has landed
    auto upload = [&](void* dev, const void* host, size_t bytes) {
        for (size_t done = 0; done < bytes;) {
            const size_t piece = std::min(kSlabBytes, bytes - done);
            needSlab(std::max<size_t>(piece, 4096));
            std::memcpy(slab.data(), static_cast<const char*>(host) + done, piece);
            hipCheck(hipMemcpyAsync(static_cast<char*>(dev) + done, slab.data(), piece, hipMemcpyHostToDevice, stream.get()), "hipMemcpyAsync H2D");
            stream.waitForCompletion();
            done += piece;
        }
    };
    upload(f.coords.data(), coords.data(), coords.size() * 4);
    upload(f.classes.data(), f.classesHost.data(), f.classesHost.size());
    upload(f.words.data(), words.data(), words.size() * 4);
    upload(f.lits.data(), lits.data(), lits.size() * 4);
    // the literals: consecutive tiles share a slab piece (a tile is at most 32 KiB)
    size_t at = 0, held = 0;
    needSlab(std::min<size_t>(kSlabBytes, std::max<size_t>(units * kUnitBytes, 4096)));
    auto flush = [&]() {
        if (!held) return;
        hipCheck(hipMemcpyAsync(static_cast<char*>(f.arena.data()) + at, slab.data(), held, hipMemcpyHostToDevice, stream.get()), "hipMemcpyAsync H2D");
        stream.waitForCompletion();
        at += held;
        held = 0;
    };
    for (const StoredTile& t : found) {
        if (t.literals.empty()) continue;
        if (held + t.literals.size() > slab.bytes()) flush();
        std::memcpy(slab.as<char>() + held, t.literals.data(), t.literals.size());
        held += t.literals.size();
    }
    flush();
    return f;
}

TileGather TileStore::gather(Stream& stream) {
    TileGather g;
    uint64_t units = 0;
    for (const auto& [key, t] : tiles) {
        g.keys.push_back(key);
        g.cls.insert(g.cls.end(), t.cls, t.cls + 3);
        g.words.insert(g.words.end(), t.words, t.words + 4);
        uint64_t at = units;
        for (int a = 0; a < 3; ++a) {
            g.at.push_back(t.cls[a] == 2 ? at : 0ull);
            if (t.cls[a] == 2) at += a == 2 ? 2 : 1;
        }
        units += unitsOf(t.cls);
    }
    g.arenaUnits = units;
    if (units == 0) return g;
    g.arena = DeviceBuffer(units * kUnitBytes);
    // the literals: consecutive tiles share a slab piece (a tile is at most 32 KiB), as takeFill moves them
    size_t at = 0, held = 0;
    needSlab(std::min<size_t>(kSlabBytes, std::max<size_t>(units * kUnitBytes, 4096)));
    auto flush = [&]() {
        if (!held) return;
        hipCheck(hipMemcpyAsync(static_cast<char*>(g.arena.data()) + at, slab.data(), held, hipMemcpyHostToDevice, stream.get()), "hipMemcpyAsync H2D");
        stream.waitForCompletion();
        at += held;
        held = 0;
    };
    for (const auto& [key, t] : tiles) {
        if (t.literals.empty()) continue;
        if (held + t.literals.size() > slab.bytes()) flush();
        std::memcpy(slab.as<char>() + held, t.literals.data(), t.literals.size());
        held += t.literals.size();
    }
    flush();
    return g;
}

}  // namespace emf
