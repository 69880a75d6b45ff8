"""Shared by the background-store tests: a numpy restatement of the tile classes, of
emf_hip_spillTiles and emf_hip_fillTiles (include/emf_hip.h "Storing and restoring tiles"), of the per-tile sign and
unseen-tile entries, a dict-based tile store with emf::TileStore's FIFO budget, a roll that spills into it and fills
from it, the version-3 checkpoint layout, and a stream built on tests/roll_reference.py whose camera walks out along
x until the policy rolls and walks back until it rolls the other way.  Everything is compared as bits."""
import struct
from collections import OrderedDict

import numpy as np

from tests import roll_reference as rr

TILE = rr.TILE
UNIT = 8192         # bytes of one arena unit
RECORD_BYTES = 40   # what a stored tile costs besides its literals


def tiles_of(res):
    return tuple(n // t for n, t in zip(res, TILE))


def tile_slices(t):
    """numpy slices (z, y, x) of tile t = (x, y, z)."""
    return (slice(t[2] * TILE[2], (t[2] + 1) * TILE[2]), slice(t[1] * TILE[1], (t[1] + 1) * TILE[1]),
            slice(t[0] * TILE[0], (t[0] + 1) * TILE[0]))


def _words(a):
    """The tile's bytes in tile order (z, y, x; x fastest) as u32 words."""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def classify(words, element):
    """(class, the first element's words) of one array of a tile; element = words per element (1, or 2 for colour)."""
    e = words.reshape(-1, element)
    first = e[0].copy()
    if (e == first).all():
        return (0 if not first.any() else 1), first
    return 2, first


def spill(tsdf, wts, color, box_lo, box_size):
    """emf_hip_spillTiles: (classes (n, 3) u8, words (n, 4) u32, lits (n, 3) u32, units, arena (units, 8192) u8)."""
    classes, words, lits, arena, units = [], [], [], [], 0
    for z in range(box_size[2]):
        for y in range(box_size[1]):
            for x in range(box_size[0]):
                sl = tile_slices((box_lo[0] + x, box_lo[1] + y, box_lo[2] + z))
                arrays = [(_words(tsdf[sl]), 1), (_words(wts[sl]), 1)]
                arrays.append((_words(color[sl]), 2) if color is not None else (np.zeros(4096, np.uint32), 2))
                k, w, l = [], [], []
                for a, (wd, el) in enumerate(arrays):
                    c, first = classify(wd, el)
                    k.append(c)
                    w.extend(int(v) for v in first)
                    l.append(units if c == 2 else 0)
                    if c == 2:
                        arena.append(wd.view(np.uint8).reshape(-1, UNIT))
                        units += el
                classes.append(k)
                words.append(w)
                lits.append(l)
    n = len(classes)
    return (np.array(classes, np.uint8).reshape(n, 3), np.array(words, np.uint32).reshape(n, 4),
            np.array(lits, np.uint32).reshape(n, 3), units,
            np.concatenate(arena) if arena else np.zeros((0, UNIT), np.uint8))


def tile_arrays(classes, words, lits, arena, with_color):
    """The (8, 8, 32) f32 tsdf and weights and the (8, 8, 32, 4) u16 colour (None without) that one tile's record holds."""
    out = []
    for a, (el, count) in enumerate(((1, 2048), (1, 2048), (2, 2048))):
        if a == 2 and not with_color:
            out.append(None)
            continue
        if classes[a] == 2:
            u = el * UNIT
            w = np.ascontiguousarray(arena.reshape(-1)[int(lits[a]) * UNIT:int(lits[a]) * UNIT + u]).view(np.uint32)
        elif classes[a] == 1:
            w = np.tile(np.asarray(words[a:a + 1] if a < 2 else words[2:4], np.uint32), count)
        else:
            w = np.zeros(count * el, np.uint32)
        out.append(w.view(np.float32).reshape(8, 8, 32) if a < 2 else w.view(np.uint16).reshape(8, 8, 32, 4))
    return out


def fill(tsdf, wts, color, coords, classes, words, lits, arena):
    """emf_hip_fillTiles on numpy volumes, in place."""
    for i, t in enumerate(coords):
        sl = tile_slices(t)
        t_, w_, c_ = tile_arrays(classes[i], words[i], lits[i], arena, color is not None)
        tsdf[sl], wts[sl] = t_, w_
        if color is not None:
            color[sl] = c_


def maps_of(tsdf, wts):
    """(sign maps (2 * tiles) u8, unseen-tile map (tiles) u8) as emf_hip_rebuildSignMaps / emf_hip_rebuildUnseenTiles
    compute them on a volume of whole tiles: tile index (z * nty + y) * ntx + x."""
    nz, ny, nx = tsdf.shape
    nt = tiles_of((nx, ny, nz))
    n = nt[0] * nt[1] * nt[2]
    sign, unseen = np.zeros(2 * n, np.uint8), np.zeros(n, np.uint8)
    for z in range(nt[2]):
        for y in range(nt[1]):
            for x in range(nt[0]):
                sl, i = tile_slices((x, y, z)), (z * nt[1] + y) * nt[0] + x
                with np.errstate(invalid="ignore"):
                    sign[i], sign[n + i] = (tsdf[sl] > 0).any(), (tsdf[sl] < 0).any()
                    unseen[i] = ((wts[sl] == 0).all() and (np.abs(tsdf[sl]) <= np.float32(3.0e38)).all())
    return sign, unseen


# ---- the store ---------------------------------------------------------------------------------------------------

class DictStore:
    """emf::TileStore restated: lattice tile coordinate -> record, in insertion order; a tile costs RECORD_BYTES plus
    its literals; after a spill that exceeds the budget whole spills are dropped, the oldest first."""

    def __init__(self, budget=1 << 30):
        self.budget, self.tiles, self.seq = budget, OrderedDict(), 0
        self.spilled = self.restored = self.evicted = 0

    @property
    def bytes_held(self):
        return sum(RECORD_BYTES + t["literals"].size for t in self.tiles.values())

    def info(self):
        return dict(tiles_held=len(self.tiles), bytes_held=self.bytes_held, tiles_spilled=self.spilled,
                    tiles_restored=self.restored, tiles_evicted=self.evicted)

    def begin_spill(self):
        self.seq += 1
        self.index = 0

    def insert(self, key, classes, words, literals):
        if not np.asarray(classes).any():
            return
        self.tiles.pop(key, None)
        self.tiles[key] = dict(seq=self.seq, index=self.index, classes=np.array(classes, np.uint8),
                               words=np.array(words, np.uint32), literals=np.array(literals, np.uint8).reshape(-1))
        self.index += 1
        self.spilled += 1

    def end_spill(self):
        while self.bytes_held > self.budget and self.tiles:
            oldest = min(t["seq"] for t in self.tiles.values())
            for key in [k for k, t in self.tiles.items() if t["seq"] == oldest]:
                del self.tiles[key]
                self.evicted += 1

    def take(self, key):
        t = self.tiles.pop(key, None)
        if t is not None:
            self.restored += 1
        return t


def units_of(classes):
    return int(classes[0] == 2) + int(classes[1] == 2) + 2 * int(classes[2] == 2)


def roll_boxes(nt, k, entering):
    """EMFusionFollow.cpp's rollBoxes: the tile boxes (lo, size) that a roll by k tiles moves out of a volume of nt
    tiles, or -- entering -- the boxes of the rolled volume that nothing moved into: x first over all y, z, then y
    over the x that stays, then z."""
    lo, hi, out = [0, 0, 0], list(nt), []
    for a in range(3):
        if k[a] == 0:
            continue
        m, low = abs(k[a]), (k[a] > 0) != entering
        blo, bsz = list(lo), [h - l for l, h in zip(lo, hi)]
        blo[a], bsz[a] = (0 if low else nt[a] - m), m
        if min(bsz) > 0:
            out.append((tuple(blo), tuple(bsz)))
        if low:
            lo[a] = m
        else:
            hi[a] = nt[a] - m
        if hi[a] <= lo[a]:
            break
    return out


def roll_with_store(store, tsdf, wts, color, origin, shift):
    """EMFusion::rollBackgroundAt with the store on, restated: spill what leaves, roll, fill what the store holds of
    what enters.  origin: the cumulative roll in voxels BEFORE this one.  Returns the rolled (tsdf, wts, color)."""
    res = tsdf.shape[::-1]
    nt = tiles_of(res)
    k = [max(-n, min(n, s // t)) for s, t, n in zip(shift, TILE, nt)]  # shifts are tile multiples
    before = [o // t for o, t in zip(origin, TILE)]
    after = [(o + s) // t for o, s, t in zip(origin, shift, TILE)]
    store.begin_spill()
    for lo, size in roll_boxes(nt, k, False):
        classes, words, lits, units, arena = spill(tsdf, wts, color, lo, size)
        c = 0
        for z in range(size[2]):
            for y in range(size[1]):
                for x in range(size[0]):
                    u = units_of(classes[c])
                    first = next((int(lits[c][a]) for a in range(3) if classes[c][a] == 2), 0)
                    store.insert((before[0] + lo[0] + x, before[1] + lo[1] + y, before[2] + lo[2] + z), classes[c], words[c],
                                 arena[first:first + u])
                    c += 1
    store.end_spill()
    out_t, out_w = rr.rolled(tsdf, shift), rr.rolled(wts, shift)
    out_c = None if color is None else rr.rolled(color, shift)
    for lo, size in roll_boxes(nt, k, True):
        for z in range(lo[2], lo[2] + size[2]):
            for y in range(lo[1], lo[1] + size[1]):
                for x in range(lo[0], lo[0] + size[0]):
                    t = store.take((after[0] + x, after[1] + y, after[2] + z))
                    if t is None:
                        continue
                    lits, at = [], 0
                    for a in range(3):
                        lits.append(at if t["classes"][a] == 2 else 0)
                        at += (2 if a == 2 else 1) if t["classes"][a] == 2 else 0
                    fill(out_t, out_w, out_c, [(x, y, z)], [t["classes"]], [t["words"]], [lits], t["literals"].reshape(-1, UNIT))
    return out_t, out_w, out_c


# ---- the out-and-back stream -------------------------------------------------------------------------------------
FRAMES = 15
ROLLS = {6: (32, 0, 0), 12: (-32, 0, 0)}  # frame -> what the policy decides at its end


def camera_t(f):
    """0.11 m per frame along x for six frames (0.66 m > one x cell of 0.64 m at frame 6: the policy rolls by +32), then
    0.12 m per frame back: 0.06 m at frame 11 (0.58 m behind the rolled centre: nothing) and -0.06 m at frame 12
    (0.70 m behind it: the policy rolls by -32)."""
    x = 0.11 * min(f, 6) - 0.12 * max(0, f - 6)
    return np.array([x, 0.0, 0.0], np.float32)


def render(f):
    """roll_reference.render's wall from this stream's camera."""
    K = np.array(rr.params().K, np.float64).reshape(3, 3)
    c = camera_t(f).astype(np.float64)
    xs, ys = np.meshgrid(np.arange(rr.W), np.arange(rr.H))
    dx, dy = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]
    t = (1.5 + 0.4 * c[0] + 0.05 * c[1] - c[2]) / (1.0 - 0.4 * dx - 0.05 * dy)
    return t.astype(np.float32)


# ---- checkpoint version 3 ------------------------------------------------------------------------------------------
# The version 2 layout (tests/checkpoint_format.py, its "ROLL" section always present) plus one trailing "TILE" section:
#   u32 store on; u32 the background has rolled; u64 budget; u64 tiles held, bytes held, tiles spilled, restored,
#   evicted; u64 last spill sequence; u64 tile count; then per stored tile, in store order: i32 lattice coordinate
#   x y z; u64 spill sequence; u8 class x 3; u8 0; u32 word x 4 (40 bytes) and its literal arrays.

def tile_payload(store, rolled=True, on=1):
    info = store.info()
    out = struct.pack("<IIQ", on, int(rolled), store.budget)
    out += struct.pack("<5Q", info["tiles_held"], info["bytes_held"], info["tiles_spilled"], info["tiles_restored"],
                       info["tiles_evicted"])
    out += struct.pack("<QQ", store.seq, len(store.tiles))
    for key, t in store.tiles.items():
        out += struct.pack("<3iQ", *key, t["seq"]) + bytes(int(c) for c in t["classes"]) + b"\0"
        out += np.asarray(t["words"], "<u4").tobytes() + t["literals"].tobytes()
    return out


def small_store():
    """Two spills: a literal tsdf over a repeated weight, then a tile of one repeated colour voxel and a full literal."""
    rng = np.random.default_rng(33)
    store = DictStore(budget=1 << 20)
    store.begin_spill()
    store.insert((-1, 2, 0), (2, 1, 0), (7, 0x42800000, 0, 0), rng.integers(0, 256, UNIT, dtype=np.uint8))
    store.end_spill()
    store.begin_spill()
    store.insert((5, -3, 1), (0, 0, 1), (0, 0, 0x00020001, 0x00040003), np.zeros(0, np.uint8))
    store.insert((5, -2, 1), (2, 2, 2), (1, 2, 3, 4), rng.integers(0, 256, 4 * UNIT, dtype=np.uint8))
    store.end_spill()
    return store
