// TileStore.hpp -- emf::TileStore: what rolled out of the background, kept on the host as the bytes it was, and put
// back when the camera returns (new behaviour, the reference's background never moves).
//
// A map from LATTICE tile coordinate -- (backgroundOrigin() + the tile's first voxel) / (32, 8, 8), the same for a
// piece of space whatever the volume's position -- to a tile record: the three class bytes, the four words and the
// literal arrays of include/emf_hip.h "Storing and restoring tiles".  A tile whose three arrays are all class 0 is
// never stored: zeros are what a roll leaves anyway.  The store has a byte budget; a tile costs kRecordBytes plus its
// literals.  When a spill has pushed the store past the budget, whole spills are dropped, the oldest first (FIFO by
// spill sequence, so the same session drops the same tiles on every run), until it fits -- the newest one too if it
// is larger than the budget on its own.
// Device traffic goes through one emf::PinnedBuffer slab of at most 64 MiB, as Checkpoint.cpp moves its records.
#pragma once

#include <array>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "types.hpp"

namespace emf {

using TileKey = std::array<int32_t, 3>;  // lattice tile coordinate (x, y, z); ordered as std::array compares

/** A box of whole tiles of a volume: first tile and size, in tiles. */
struct TileBox {
    Vec3i lo, size;
};

struct StoredTile {
    uint64_t seq = 0;    // the spill that brought it
    uint32_t index = 0;  // its position in that spill
    uint8_t cls[3] = {0, 0, 0};
    uint32_t words[4] = {0, 0, 0, 0};
    std::vector<uint8_t> literals;  // the class-2 arrays: tsdf (8 KiB), weights (8 KiB), colour (16 KiB), in that order
};

/** The argument list of emf_hip_fillTiles for one roll, on the device (TSDF::roll). */
struct TileFill {
    uint32_t n = 0;
    DeviceBuffer coords, classes, words, lits, arena;
    std::vector<uint8_t> classesHost;
    uint64_t arenaUnits = 0;
};

/** Every held tile, read-only, with its literals in one device arena (TileStore::gather). */
struct TileGather {
    std::vector<TileKey> keys;    // map order
    std::vector<uint8_t> cls;     // 3 per tile
    std::vector<uint32_t> words;  // 4 per tile
    std::vector<uint64_t> at;     // 3 per tile: the arena unit of a class-2 array, else 0
    DeviceBuffer arena;
    uint64_t arenaUnits = 0;
};

class TileStore {
public:
    static constexpr uint64_t kRecordBytes = 40;  // what a tile costs besides its literals (its checkpoint header)
    static constexpr uint64_t kUnitBytes = 8192;  // one arena unit
    static constexpr uint64_t kDefaultBudget = 1ull << 30;

    struct Counters {
        uint64_t tilesHeld = 0, bytesHeld = 0, tilesSpilled = 0, tilesRestored = 0, tilesEvicted = 0;
    };

    uint64_t budget() const { return maxBytes; }
    void setBudget(uint64_t bytes) { maxBytes = bytes; }
    const Counters& counters() const { return c; }
    /** Drop every tile (the cumulative counters stay). */
    void clear();

    /** Literal units of a tile with these classes. */
    static uint32_t unitsOf(const uint8_t cls[3]) { return (cls[0] == 2) + (cls[1] == 2) + 2 * (cls[2] == 2); }

    // ---- the host-side map ----
    uint64_t beginSpill() {
        nextIndex = 0;
        return ++lastSeq;
    }
    /** literals: unitsOf(cls) * kUnitBytes bytes.  An all-class-0 tile is ignored; a key already held is replaced. */
    void insert(const TileKey& key, uint64_t seq, const uint8_t cls[3], const uint32_t words[4], const uint8_t* literals);
    /** Enforce the budget after a spill's insertions. */
    void endSpill();
    /** Move the tile at `key` out of the store; false if it holds none. */
    bool take(const TileKey& key, StoredTile& out);
    bool empty() const { return tiles.empty(); }
    /** (key, tile) in store order: by spill, then by position in the spill. */
    std::vector<std::pair<TileKey, const StoredTile*>> inOrder() const;
    /** Checkpoint restore: the state exactly as it was saved. */
    void restore(uint64_t budgetBytes, const Counters& saved, uint64_t seq);
    void restoreTile(const TileKey& key, StoredTile&& t);
    uint64_t sequence() const { return lastSeq; }

    // ---- device traffic ----
    /**
     * Spill `boxes` (tile boxes of a volume of `res` voxels whose tile (0, 0, 0) has lattice coordinate `lattice`) as
     * ONE spill: every classify / gather is enqueued on `stream`, then one wait, then headers and literals come over
     * through the pinned slab and are inserted in box order, candidate order within a box.  A box of more tiles than
     * one 64 MiB arena covers in the worst case is cut first.
     */
    void spill(const float* tsdf, const float* weights, const uint16_t* color, const Vec3i& res, const std::vector<TileBox>& boxes,
               const TileKey& lattice, Stream& stream);
    /**
     * Look up the tiles of `boxes` (tile boxes of the volume AFTER the roll, lattice coordinate of its tile (0, 0, 0)
     * `lattice`), take the found ones out of the store -- the volume owns them again and spills them again when they
     * next leave -- and upload them as a fill list.  n == 0 if none was found.  Waits for `stream`.
     */
    TileFill takeFill(const std::vector<TileBox>& boxes, const TileKey& lattice, Stream& stream);
    /**
     * Every held tile's record, and the literals uploaded into one device arena through the pinned slab.  Read-only:
     * the tiles, their order and the counters stay exactly as they were.  Waits for `stream`.
     */
    TileGather gather(Stream& stream);

private:
    std::map<TileKey, StoredTile> tiles;
    std::map<std::pair<uint64_t, uint32_t>, TileKey> order;  // (seq, index) -> key
    uint64_t maxBytes = kDefaultBudget;
    uint64_t lastSeq = 0;
    uint32_t nextIndex = 0;  // within the current spill
    Counters c;
    PinnedBuffer slab;
    void erase(std::map<TileKey, StoredTile>::iterator it);
    void needSlab(size_t bytes);
};

}  // namespace emf
