"""Shared by the world-query tests (include/emf_hip.h "Occupancy of a set of tiles"): the occupancy
classes of a box of the LATTICE from a tile set, restated on the dense box the set stands for, and the maps between the
three voxel coordinates a world query speaks of.  Everything is integers and single float comparisons: compared as
bytes, no tolerance.

  lattice voxel   the integer lattice of the initial background pose: volume voxel + background_origin()
  volume voxel    voxels of the CURRENT background volume; a world box may have lo < 0 and lo + size > res
  virtual voxel   volume voxel + pad, in a virtual background of res + 2 * pad voxels: the description under which the
                  unchanged stamping and the frame arithmetic give the same bits (float(v + pad) - (res + 2 pad - 1) / 2
                  == float(v) - (res - 1) / 2 exactly, all half-integers far below 2^23)

A tile set is the dict of tests/world_reference.py and emfusion_amd.ops.mesh_tiles; a box is (lo, size), both (x, y, z)."""
import numpy as np

from tests import distance_reference as dr
from tests import world_reference as wr

TILE = wr.TILE
UNKNOWN = dr.UNKNOWN


def classes_of_tiles(tiles, res, box):
    """(bz, by, bx) u8: distance_reference.classes_of of world_reference.assemble(tiles, res) cropped to the LATTICE box
    `box`; what the crop does not cover -- space beyond every listed tile -- is UNKNOWN.  res: the resolution (x, y, z)
    the assembled box is grown from, whole tiles; any will do, the result does not depend on it."""
    tsdf, wts, _, pv = wr.assemble(tiles, res)
    dense = dr.classes_of(tsdf, wts)
    (x0, y0, z0), (sx, sy, sz) = box
    out = np.full((sz, sy, sx), UNKNOWN, np.uint8)
    src, dst = [], []
    for lo, size, pad, n in zip((z0, y0, x0), (sz, sy, sx), pv[::-1], dense.shape):
        a, b = max(lo + pad, 0), min(lo + pad + size, n)       # in the dense box
        if b <= a:
            return out
        src.append(slice(a, b))
        dst.append(slice(a - lo - pad, b - lo - pad))
    out[tuple(dst)] = dense[tuple(src)]
    return out


# (tile (x, y, z), tsdf or None to keep the volume's, weights or None) planted into a volume of at least 2 x 6 x 5 tiles
PLANTED = [((0, 0, 0), 0.0, 0.0),     # both arrays all zero: classes (0, 0), unknown
           ((1, 2, 1), 0.5, 3.0),     # both one repeated word: (1, 1), free, decided once
           ((0, 3, 2), -0.25, 1.0),   # (1, 1), occupied
           ((1, 4, 3), 0.75, 0.0),    # (1, 0): the weights are the repeated word 0 -- a whole tile that reads unknown
           ((0, 5, 4), None, 2.0),    # (2, 1): a literal tsdf under one repeated weight, read voxel by voxel
           ((1, 1, 4), 0.0, None)]    # (0, 2): an all-zero tsdf under literal weights: occupied wherever seen


def planted(tsdf, wts):
    """Copies of a fused volume with the tiles of PLANTED overwritten.  The fused volumes of tests/world_volumes.py cut
    into literals only -- every tile holds some surface or some noise --, so the tiles that are all zero or one
    repeated word, which emf_hip_occupancyTiles decides once, are planted."""
    t, w = tsdf.copy(), wts.copy()
    for tile, tv, wv in PLANTED:
        sl = wr.sr.tile_slices(tile)
        if tv is not None:
            t[sl] = np.float32(tv)
        if wv is not None:
            w[sl] = np.float32(wv)
    return t, w


def without(tiles, drop):
    """The tile set without the tiles whose index is in `drop` (arena and volume stay as they are)."""
    keep = np.ones(len(tiles["coords"]), bool)
    keep[list(drop)] = False
    out = dict(tiles)
    for k in ("coords", "classes", "words", "at"):
        out[k] = np.asarray(tiles[k])[keep]
    return out


def extent_of(tiles):
    """The LATTICE box (lo, size) that bounds every listed tile."""
    c = np.asarray(tiles["coords"], np.int64).reshape(-1, 3)
    lo = c.min(axis=0) * np.array(TILE)
    hi = (c.max(axis=0) + 1) * np.array(TILE)
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo)


# ---- the coordinate maps --------------------------------------------------------------------------------------------

def lattice_of(volume_voxel, origin):
    return tuple(int(v) + int(o) for v, o in zip(volume_voxel, origin))


def volume_of(lattice_voxel, origin):
    return tuple(int(v) - int(o) for v, o in zip(lattice_voxel, origin))


def pad_of(box, res):
    """Per axis the voxels a box (volume voxels) leaves a background of `res` by, on either side; 0 inside."""
    lo, size = box
    return tuple(max(0, -int(a), int(a) + int(s) - int(n)) for a, s, n in zip(lo, size, res))


def virtual_of(box, res, pad=None):
    """(virtual resolution, the box in virtual voxels) of a box in volume voxels."""
    pad = pad_of(box, res) if pad is None else pad
    lo, size = box
    return (tuple(int(n) + 2 * p for n, p in zip(res, pad)),
            (tuple(int(a) + p for a, p in zip(lo, pad)), tuple(int(s) for s in size)))


def stamping_coordinate(v, n):
    """float32(v) - (n - 1) / 2.f as emf_hip_occupancyStampObjects computes it, for integer arrays v."""
    f = np.float32
    return np.asarray(v).astype(f) - f(n - 1) / f(2)
