"""Vertex colours restated in numpy (include/emf_hip.h "Per-voxel colour"; color_cube of meshing.hip): per soup vertex,
in emission order, the colour interpolated between the two voxels of its grid edge, in float32 and in the kernel's
operation order, so the result is the kernel's byte for byte (numpy does not contract, and the kernel has contraction
off).  No marching-cubes table: an edge carries a vertex iff its two corners' signs differ."""
import numpy as np

from tests.weld_reference import CORNERS, EDGES

f32 = np.float32


def vertex_colours(tsdf, weights, colour, fg=None):
    """(n, 3) u8: cubes in (z, y, x) order, a cube valid iff all 8 corners have weights > 0 and fg != 0, its edges
    ascending; colour is the (nz, ny, nx, 4) u16 volume (R, G, B in 1/256 levels, Wc), None for a model without one."""
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
    for e, (a, b) in enumerate(EDGES):
        active[..., e] = valid & (at(neg, a) != at(neg, b))
    z, y, x, e = np.nonzero(active)                                 # emission order
    if colour is None:
        return np.zeros((len(e), 3), np.uint8)
    ends = np.array(EDGES)[e]                                       # the edge's corners, first and second
    off = np.array(CORNERS)                                         # corner -> (dx, dy, dz)
    val, col = [], []
    for s in range(2):
        d = off[ends[:, s]]
        idx = (z + d[:, 2], y + d[:, 1], x + d[:, 0])
        val.append(tsdf[idx])
        col.append(colour[idx].copy())
    # an uncoloured endpoint (Wc == 0) contributes the other endpoint's colour -- the first is replaced first, and the
    # second then looks at what the first has become; neither coloured: black
    first_bare = col[0][:, 3] == 0
    col[0][first_bare] = col[1][first_bare]
    second_bare = col[1][:, 3] == 0
    col[1][second_bare] = col[0][second_bare]
    none = col[0][:, 3] == 0
    # vertexInterp's three outcomes (the comparisons are against the double 0.00001)
    v1, v2 = val
    with np.errstate(all="ignore"):
        take1 = np.abs(v1).astype(np.float64) < 0.00001
        take2 = ~take1 & (np.abs(v2).astype(np.float64) < 0.00001)
        take1 |= ~take2 & (np.abs(v1 - v2).astype(np.float64) < 0.00001)
        mu = (-v1 / (v2 - v1)).astype(f32)
        out = np.zeros((len(e), 3), np.uint8)
        for j in range(3):
            c1 = col[0][:, j].astype(f32) / f32(256)
            c2 = col[1][:, j].astype(f32) / f32(256)
            v = np.where(take1, c1, np.where(take2, c2, c1 + mu * (c2 - c1))).astype(f32)
            out[:, j] = np.minimum(np.maximum(np.rint(v), f32(0)), f32(255)).astype(np.uint8)
    out[none] = 0
    return out
