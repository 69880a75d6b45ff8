"""Shared by the world-mesh tests (include/emf_hip.h "Meshing a set of tiles"): the dense box that a
set of tiles stands for, the oracle's soup of that box permuted into the canonical order of the tile mesher, and the
lattice edge keys restated.  Everything is compared as bits.

A tile set is the dict that emfusion_amd.ops.mesh_tiles takes: coords (n, 3) lattice tile coordinates (x, y, z), sorted
ascending in (z, y, x); classes (n, 3) u8; words (n, 4) u32; at (n, 3) u64 (class 2: arena unit, class 3: element
offset into `volume`); arena (units, 8192) u8 or None; volume: None or dict(tsdf, weights[, color]).

The box is the volume of `res` voxels whose voxel 0 is lattice voxel 0, grown by the SAME number of voxels on both
sides of an axis (a multiple of the tile): then (N_box - 1) / 2 = (N - 1) / 2 + pad exactly, hence
x_box - half_box == x_lattice - half exactly, and the oracle's positions are the tile mesher's bit for bit."""
import numpy as np

from tests import store_reference as sr
from tests.weld_reference import CORNERS, EDGES

TILE = sr.TILE
UNIT = sr.UNIT
BIAS = 1 << 19


def auto_pad(coords, res):
    """Tiles of padding per axis: every listed tile and the tile after and before it lie inside the box."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    pad = []
    for a in range(3):
        nt = res[a] // TILE[a]
        lo = int(coords[:, a].min()) - 1 if len(coords) else 0
        hi = int(coords[:, a].max()) + 2 if len(coords) else nt  # one past the tile after the last
        pad.append(max(0, -lo, hi - nt, 1))
    return tuple(pad)


def tile_content(tiles, i, with_color):
    """The (8, 8, 32) tsdf and weights and the (8, 8, 32, 4) colour (None without) of tile i of a set."""
    classes, words, at = tiles["classes"][i], tiles["words"][i], tiles["at"][i]
    arena = tiles.get("arena")
    arena = np.zeros((0, UNIT), np.uint8) if arena is None else arena
    stored = [int(c) if c != 3 else 0 for c in classes]
    out = sr.tile_arrays(stored, words, [int(v) for v in at], arena, with_color)
    vol = tiles.get("volume")
    for a, name in enumerate(("tsdf", "weights", "color")):
        if classes[a] != 3 or (a == 2 and not with_color):
            continue
        v = vol[name]
        nz, ny, nx = v.shape[:3]
        off = int(at[a])
        z, y, x = off // (nx * ny), (off // nx) % ny, off % nx
        out[a] = v[z:z + TILE[2], y:y + TILE[1], x:x + TILE[0]]
    return out


def assemble(tiles, res, pad=None, with_color=False):
    """(tsdf, weights, colour or None, pad in voxels (x, y, z)): the dense box of the tile set."""
    coords = np.asarray(tiles["coords"], np.int64).reshape(-1, 3)
    pad = auto_pad(coords, res) if pad is None else pad
    pv = tuple(p * t for p, t in zip(pad, TILE))
    shape = (res[2] + 2 * pv[2], res[1] + 2 * pv[1], res[0] + 2 * pv[0])
    tsdf, wts = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    col = np.zeros(shape + (4,), np.uint16) if with_color else None
    for i, c in enumerate(coords):
        t, w, k = tile_content(tiles, i, with_color)
        sl = sr.tile_slices(tuple(int(c[a]) + pad[a] for a in range(3)))
        assert min(s.start for s in sl) >= 0 and all(s.stop <= n for s, n in zip(sl, shape)), "pad too small"
        tsdf[sl], wts[sl] = t, w
        if with_color and k is not None:
            col[sl] = k
    return tsdf, wts, col, pv


def soup_cubes(tsdf, weights):
    """(z, y, x, e) of every soup vertex of oracle.marching_cubes(tsdf, weights), in its order: the anchor of the
    vertex's cube and its edge -- tests/weld_reference.edge_keys' enumeration."""
    nz, ny, nx = tsdf.shape
    ok, neg = weights > 0, tsdf < 0

    def at(a, c):
        dx, dy, dz = CORNERS[c]
        return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        valid &= at(ok, c)
    active = np.zeros(valid.shape + (12,), bool)
    for e, (a, b) in enumerate(EDGES):
        active[..., e] = valid & (at(neg, a) != at(neg, b))
    return np.nonzero(active)


def cube_rank(z, y, x, pad):
    """Sort key of a cube in the canonical order: its tile in (z, y, x) order, then its anchor inside the tile."""
    lz, ly, lx = z.astype(np.int64) - pad[2], y.astype(np.int64) - pad[1], x.astype(np.int64) - pad[0]
    tz, ty, tx = lz // TILE[2], ly // TILE[1], lx // TILE[0]
    return tz, ty, tx, lz - tz * TILE[2], ly - ty * TILE[1], lx - tx * TILE[0]


def canonical(soup, cubes, pad, extra=()):
    """The oracle's soup (vertices, normals, triangles) permuted into the canonical order: tiles in (z, y, x) order,
    cubes in (z, y, x) order inside a tile, a cube's vertices and triangles as they were.  cubes: soup_cubes' (z, y, x,
    e); pad: the box's padding in voxels (x, y, z); extra: per-vertex arrays (colours, keys) permuted alike.
    Returns (vertices, normals, triangles, *extra, order) -- order[i] = the soup index of canonical vertex i."""
    v, n, t = soup
    z, y, x, _ = cubes
    assert len(z) == len(v)
    key = cube_rank(z, y, x, pad)
    order = np.lexsort(key[::-1])            # stable: a cube's vertices keep their edge-bit order
    inverse = np.empty(len(order), np.int64)
    inverse[order] = np.arange(len(order))
    if len(t):
        first = t[:, 1]                      # a triangle's cube is that of its vertices
        torder = np.lexsort(tuple(k[first] for k in key)[::-1])
        ct = t[torder].copy()
        ct[:, 1:] = inverse[ct[:, 1:]].astype(t.dtype)
    else:
        ct = t.copy()
    return (v[order], n[order], ct) + tuple(a[order] for a in extra) + (order,)


def lattice_keys(cubes, pad):
    """3 * (((z + 2^19) << 40) | ((y + 2^19) << 20) | (x + 2^19)) + axis of the lower lattice voxel of every soup
    vertex's grid edge, in soup order."""
    z, y, x, e = cubes
    lo = np.array([np.minimum(CORNERS[a], CORNERS[b]) for a, b in EDGES], np.int64)           # (12, 3): dx, dy, dz
    axis = np.array([np.flatnonzero(np.array(CORNERS[a]) != np.array(CORNERS[b]))[0] for a, b in EDGES], np.uint64)
    X = (x.astype(np.int64) - pad[0] + lo[e, 0] + BIAS).astype(np.uint64)
    Y = (y.astype(np.int64) - pad[1] + lo[e, 1] + BIAS).astype(np.uint64)
    Z = (z.astype(np.int64) - pad[2] + lo[e, 2] + BIAS).astype(np.uint64)
    return np.uint64(3) * ((Z << np.uint64(40)) | (Y << np.uint64(20)) | X) + axis[e]


def reference(oracle, tiles, res, voxel_size, with_color=False, pad=None):
    """dict(soup=(v, n, t) canonical, keys, colours or None, cubes=(tile coordinate (n, 3), local anchor (n, 3)) per
    canonical vertex, box=(tsdf, weights, colour), pad) of a tile set."""
    from tests.mesh_color_reference import vertex_colours
    tsdf, wts, col, pv = assemble(tiles, res, pad, with_color)
    soup = oracle.marching_cubes(tsdf, wts, voxel_size)
    cubes = soup_cubes(tsdf, wts)
    extra = [lattice_keys(cubes, pv)]
    if with_color:
        extra.append(vertex_colours(tsdf, wts, col))
    out = canonical(soup, cubes, pv, extra)
    order = out[-1]
    tz, ty, tx, lz, ly, lx = (k[order] for k in cube_rank(cubes[0], cubes[1], cubes[2], pv))
    return dict(soup=out[:3], keys=out[3], colours=out[4] if with_color else None,
                cubes=(np.stack([tx, ty, tz], 1), np.stack([lx, ly, lz], 1)), box=(tsdf, wts, col), pad=pv)


def half_of(res):
    """(N - 1) / 2.f per axis (x, y, z): what a session passes for its background."""
    return tuple(np.float32(n - 1) / np.float32(2) for n in res)


# ---- tile sets out of dense volumes -------------------------------------------------------------------------------

def cut(tsdf, wts, color=None, offset=(0, 0, 0), mode="literal", seed=0, keep=None):
    """The tile set of a dense (Nz, Ny, Nx) volume of whole tiles, its tile (0, 0, 0) at lattice tile `offset`.  mode:
    "literal" -- every array by its spill class (0, 1 or 2); "inplace" -- every array class 3 over the volume itself;
    "mixed" -- a seeded choice per tile.  keep: a boolean per tile (z, y, x order) or None for all."""
    nz, ny, nx = tsdf.shape
    nt = sr.tiles_of((nx, ny, nz))
    rng = np.random.default_rng(seed)
    coords, classes, words, at, arena, units, i = [], [], [], [], [], 0, -1
    for z in range(nt[2]):
        for y in range(nt[1]):
            for x in range(nt[0]):
                i += 1
                if keep is not None and not keep[i]:
                    continue
                inplace = mode == "inplace" or (mode == "mixed" and rng.integers(0, 2) == 1)
                k, w, l = sr.spill(tsdf, wts, color, (x, y, z), (1, 1, 1))[:3]
                k, w, l = [int(v) for v in k[0]], [int(v) for v in w[0]], [0, 0, 0]
                if inplace:
                    k = [3, 3, 3 if color is not None else 0]
                    l = [(z * TILE[2] * ny + y * TILE[1]) * nx + x * TILE[0]] * 3
                    if color is None:
                        l[2] = 0
                else:
                    sl = sr.tile_slices((x, y, z))
                    for a, src in enumerate((tsdf, wts, color)):
                        if k[a] == 2:
                            l[a] = units
                            arena.append(np.ascontiguousarray(src[sl]).view(np.uint8).reshape(-1, UNIT))
                            units += 2 if a == 2 else 1
                coords.append((x + offset[0], y + offset[1], z + offset[2]))
                classes.append(k)
                words.append(w)
                at.append(l)
    n = len(coords)
    vol = dict(tsdf=tsdf, weights=wts)
    if color is not None:
        vol["color"] = color
    return dict(coords=np.array(coords, np.int32).reshape(n, 3), classes=np.array(classes, np.uint8).reshape(n, 3),
                words=np.array(words, np.uint32).reshape(n, 4), at=np.array(at, np.uint64).reshape(n, 3),
                arena=np.concatenate(arena) if arena else None, volume=vol if mode != "literal" else None)
