"""Welded meshes restated in numpy (include/emf_hip.h "Welded meshes"): the grid-edge key of every soup vertex from the
volume alone -- no marching-cubes table: an edge carries a vertex iff its two corners' signs differ -- and the weld
itself by np.unique in first-occurrence order."""
import numpy as np

# corner i -> (dx, dy, dz); edge e -> its two corners (the reference's numbering, TSDF.cu:896-903)
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def edge_keys(tsdf, weights, fg=None, slot=0):
    """u64 key per soup vertex, in soup order: cubes in (z, y, x) order, a cube valid iff all 8 corners have
    weights > 0 and fg != 0, its edges ascending; key = slot << 48 | 3 * linear(lower voxel) + axis."""
    nz, ny, nx = tsdf.shape
    ok = weights > 0 if fg is None else (weights > 0) & (fg != 0)
    neg = tsdf < 0

    def at(a, c):  # the corner's value for every cube
        dx, dy, dz = CORNERS[c]
        return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        valid &= at(ok, c)
    active = np.zeros(valid.shape + (12,), bool)
    offset, axes = np.zeros(12, np.uint64), np.zeros(12, np.uint64)
    for e, (a, b) in enumerate(EDGES):
        active[..., e] = valid & (at(neg, a) != at(neg, b))
        lo = np.minimum(CORNERS[a], CORNERS[b])
        offset[e] = lo[0] + lo[1] * nx + lo[2] * nx * ny
        axes[e] = np.flatnonzero(np.array(CORNERS[a]) != np.array(CORNERS[b]))[0]
    # only the active (cube, edge) pairs get a key (a 256^3 volume has 2 * 10^8 pairs and a few 10^5 vertices)
    z, y, x, e = (i.astype(np.uint64) for i in np.nonzero(active))
    linear = (z * np.uint64(ny) + y) * np.uint64(nx) + x
    return (np.uint64(3) * (linear + offset[e]) + axes[e]) | (np.uint64(slot) << np.uint64(48))


def weld(v, n, t, keys, c=None):
    """Welded (vertices, normals, triangles[, colours]): vertex j is the first soup vertex of the j-th distinct key in
    order of first occurrence, bits unchanged; triangles keep order and layout, indices mapped through the keys."""
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # distinct keys by first occurrence
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    firsts, remap = first[order], rank[inverse.reshape(-1)]
    wt = t.copy()
    if len(t):
        wt[:, 1:] = remap[t[:, 1:]].astype(t.dtype)
    return (v[firsts], n[firsts], wt) + (() if c is None else (c[firsts],))
