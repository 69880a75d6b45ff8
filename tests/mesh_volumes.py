"""The volumes of the marching-cubes shape tests (tests/test_mesh_volumes_cpu.py, tests/test_gpu_mesh_shapes.py): shapes
chosen by the branch of meshing.hip they steer, filled so that every 252-position chunk carries surface.  Nothing here
touches the GPU; `layout` restates plan()'s arithmetic so that the CPU tests can say which branch a shape takes.

Shapes are (nx, ny, nz); arrays are (nz, ny, nx) like every volume of the project."""
import numpy as np

f32 = np.float32
CHUNK = 252                      # positions per chunk (4 waves of 63 cubes)
LARGE_VOXELS = 1 << 24           # from here on a counting workgroup takes 32 chunks, below it 8
XCDS = 8
VOXEL_SIZE = 0.01

# one wave spans many rows and planes: a row holds 1 - 4 cubes, rowY / rowZ differ lane by lane
THIN = [(2, 2, 700), (3, 2, 300), (5, 3, 70), (2, 130, 40)]
# retired slabs, thin on each axis in turn (the last: 6 workgroups per plane)
SLABS = [(9, 96, 130), (130, 9, 96), (130, 96, 9)]
# either side of classify_wave's nx >= 64 switch; rows of exactly a chunk and of a chunk plus one
ROWS = [(63, 7, 40), (64, 7, 40), (65, 7, 40), (252, 4, 6), (253, 4, 6)]
# workgroups per plane 2, 3 (band 1, five idle XCD columns, Nx % 4 != 0) and 9 (band 2, a padded grid)
BANDS = [(64, 64, 20), (74, 90, 66), (130, 140, 30)]
# 1057 workgroups: a second scan pass with carry; 8456 chunks: the emit grid strides
CARRY = (160, 128, 104)
DENSE_SMALL = THIN + SLABS + ROWS + BANDS            # the cases that also run with a gradient volume and in the table
DENSE = DENSE_SMALL + [CARRY]
# the largest 8-chunk neighbour of the threshold, the threshold itself, 32-chunk mode with 11 workgroups per plane;
# and 2^24 - 1 voxels (4095 * 4097 = 273 * 241 * 255), the one voxel count that tells `>= 2^24` from `>= 2^24 - 1`
SPARSE = [(256, 256, 255), (256, 256, 256), (300, 300, 187), (273, 241, 255)]
COLOURED = [(5, 3, 70), (74, 90, 66), CARRY]
FILTERED = [(9, 96, 130), (74, 90, 66), (130, 140, 30), CARRY]

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)]  # (dx, dy, dz)


def name_of(shape):
    return "x".join(str(s) for s in shape)


def layout(shape):
    """plan()'s numbers for one volume: chunks per workgroup, counting workgroups, workgroups per plane, XCD band,
    the padded grid, scan passes, chunks."""
    nx, ny, nz = shape
    nvox = nx * ny * nz
    per = 32 if nvox >= LARGE_VOXELS else 8
    span = CHUNK * per
    nblocks = -(-nvox // span)
    plane = nx * ny
    wpp = plane // span if plane >= span else 1
    band = -(-wpp // XCDS)
    rows = -(-nblocks // wpp)
    return dict(per=per, span=span, nblocks=nblocks, wpp=wpp, band=band, grid=XCDS * band * rows,
                scan_passes=-(-nblocks // 1024), chunks=nblocks * per)


def _seed(shape, salt):
    nx, ny, nz = shape
    return [salt, nx, ny, nz]


def _corner(a, c):
    nz, ny, nx = a.shape
    dx, dy, dz = CORNERS[c]
    return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def cube_classes(tsdf, weights, fg=None):
    """(complete, cls) per cube, shape (nz - 1, ny - 1, nx - 1): all 8 corners observed (weights > 0) and in the
    foreground (fg != 0); bit i of cls set where corner i is negative."""
    ok = weights > 0 if fg is None else (weights > 0) & (fg != 0)
    neg = tsdf < 0
    complete = np.ones(tuple(s - 1 for s in tsdf.shape), bool)
    cls = np.zeros(complete.shape, np.uint8)
    for c in range(8):
        complete &= _corner(ok, c)
        cls |= _corner(neg, c).astype(np.uint8) << np.uint8(c)
    return complete, cls


def surface_cubes(tsdf, weights, fg=None):
    """Per cube anchor (the voxel's own shape; False on the last x, y and z index, where no cube is anchored): the
    cube is complete and shows both signs."""
    complete, cls = cube_classes(tsdf, weights, fg)
    out = np.zeros(tsdf.shape, bool)
    out[:-1, :-1, :-1] = complete & (cls != 0) & (cls != 255)
    return out


def anchors(shape):
    """Per voxel: a cube is anchored here (all 8 corners lie inside the volume)."""
    nx, ny, nz = shape
    a = np.zeros((nz, ny, nx), bool)
    a[:-1, :-1, :-1] = True
    return a


def per_group(mask, size):
    """A per-voxel mask or count summed over every run of `size` linear positions."""
    flat = mask.reshape(-1)
    n = -(-flat.size // size)
    pad = np.zeros(n * size, np.int64)
    pad[:flat.size] = flat
    return pad.reshape(n, size).sum(axis=1)


def vertices_per_chunk(tsdf, weights, fg=None):
    """What k_mesh_count must put into the low half of chunkTot: the soup vertices of every 252-position chunk."""
    complete, cls = cube_classes(tsdf, weights, fg)
    edges = np.zeros(complete.shape, np.int64)
    for a, b in [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]:
        edges += ((cls >> np.uint8(a)) ^ (cls >> np.uint8(b))) & np.uint8(1)
    v = np.zeros(tsdf.shape, np.int64)
    v[:-1, :-1, :-1] = np.where(complete, edges, 0)
    return per_group(v, CHUNK)


def _hostile(rng, t):
    """About 5 % of the voxels from the values at which comparisons and vertexInterp's branches turn."""
    pick = rng.uniform(size=t.shape) < 0.05
    kind = rng.integers(0, 9, size=t.shape)
    values = [0.0, -0.0, 1e-40, -1e-40, 5e-6, -5e-6, 1.0, -1.0]  # 1e-40: denormal; 5e-6: inside the 1e-5 branches
    for k, v in enumerate(values):
        t[pick & (kind == k)] = f32(v)
    same = pick & (kind == 8)
    same[:, :, 0] = False
    z, y, x = np.nonzero(same)  # ascending x: a run of copies takes the value at its start
    for zz, yy, xx in zip(z.tolist(), y.tolist(), x.tolist()):
        t[zz, yy, xx] = t[zz, yy, xx - 1]


def _plant_full_chunks(t, w, fg):
    """Three fully observed planes of alternating signs mid-volume: every cube between them has all 12 edges active,
    so the chunks inside hold close to the 3024 vertices the packed fields must carry."""
    nz, ny, nx = t.shape
    z0 = nz // 2 - 1
    zz, yy, xx = np.meshgrid(np.arange(z0, z0 + 3), np.arange(ny), np.arange(nx), indexing="ij")
    sign = np.where((xx + yy + zz) % 2 == 0, f32(1), f32(-1))
    t[z0:z0 + 3] = np.maximum(np.abs(t[z0:z0 + 3]), f32(0.1)) * sign
    w[z0:z0 + 3] = np.where(w[z0:z0 + 3] > 0, w[z0:z0 + 3], f32(1))
    fg[z0:z0 + 3] = np.where(fg[z0:z0 + 3] != 0, fg[z0:z0 + 3], np.uint8(255))


def _fill_bare_chunks(t, w, fg):
    """Every chunk in which a cube is anchored gets a surface cube: where the draw left none, the chunk's first
    anchored cube is made complete and its anchor given the sign its x neighbour lacks."""
    nz, ny, nx = t.shape
    anchored = per_group(anchors((nx, ny, nz)), CHUNK) > 0
    for _ in range(4):
        bare = np.flatnonzero(anchored & (per_group(surface_cubes(t, w, fg), CHUNK) == 0))
        if not len(bare):
            return
        flat = anchors((nx, ny, nz)).reshape(-1)
        for c in bare.tolist():
            p = c * CHUNK + int(np.flatnonzero(flat[c * CHUNK:(c + 1) * CHUNK])[0])
            x, y, z = p % nx, (p // nx) % ny, p // (nx * ny)
            cube = (slice(z, z + 2), slice(y, y + 2), slice(x, x + 2))
            w[cube] = np.where(w[cube] > 0, w[cube], f32(1))
            fg[cube] = np.where(fg[cube] != 0, fg[cube], np.uint8(255))
            t[z, y, x] = f32(0.5) if t[z, y, x + 1] < 0 else f32(-0.5)
    raise AssertionError("a chunk stays without surface")


_dense = {}


def dense(shape):
    """(tsdf, weights, fg, voxel size) of a dense case, computed once and to be left unchanged.  Random signs on
    magnitudes in [0.1, 1), 5 % hostile values, 12 % of the weights not positive or denormal; fg is the foreground
    variant's mask (bytes 0, 1, 2, 128, 255, about 7 % zeros) -- the plain variant passes None instead.  Every chunk
    with a cube holds surface under the mask, hence also without it."""
    shape = tuple(shape)
    if shape not in _dense:
        nx, ny, nz = shape
        rng = np.random.default_rng(_seed(shape, 252))
        dims = (nz, ny, nx)
        t = (rng.uniform(0.1, 1.0, size=dims) * rng.choice([-1.0, 1.0], size=dims)).astype(f32)
        _hostile(rng, t)
        w = f32(64) * (f32(1) - rng.uniform(0.0, 1.0, size=dims).astype(f32))           # (0, 64]
        w = np.where(w > 0, w, f32(64)).astype(f32)
        u = rng.uniform(size=dims)
        dead = rng.integers(0, 3, size=dims)
        for k, v in enumerate([0.0, -0.0, -1.0]):
            w[(u < 0.10) & (dead == k)] = f32(v)
        w[(u >= 0.10) & (u < 0.12)] = f32(1e-40)  # a positive denormal: observed (the reference's w > 0)
        fg = rng.choice(np.array([1, 2, 128, 255], np.uint8), size=dims)
        fg[rng.uniform(size=dims) < 0.07] = 0
        if nx * ny * nz >= 10 ** 5:
            _plant_full_chunks(t, w, fg)
        _fill_bare_chunks(t, w, fg)
        for a in (t, w, fg):
            a.setflags(write=False)
        _dense[shape] = (t, w, fg, VOXEL_SIZE)
    return _dense[shape]


_sparse = {}


def sparse(shape):
    """(tsdf, weights, None, voxel size) of a sparse case, computed once: +0.5 everywhere, weights 1, one negative
    voxel of random magnitude at every 1009th linear position (less than the 2016 positions of the smallest workgroup
    span), the first voxel negative and the last voxel that anchors a cube."""
    shape = tuple(shape)
    if shape not in _sparse:
        nx, ny, nz = shape
        rng = np.random.default_rng(_seed(shape, 1009))
        t = np.full(nx * ny * nz, f32(0.5), f32)
        at = np.arange(0, t.size, 1009)
        t[at] = -rng.uniform(0.1, 1.0, size=len(at)).astype(f32)
        t = t.reshape(nz, ny, nx)
        t[nz - 2, ny - 2, nx - 2] = -rng.uniform(0.1, 1.0)
        w = np.ones_like(t)
        for a in (t, w):
            a.setflags(write=False)
        _sparse[shape] = (t, w, None, VOXEL_SIZE)
    return _sparse[shape]


def colours(shape):
    """A random (nz, ny, nx, 4) u16 colour volume, a third of the voxels uncoloured (Wc == 0) with colours that must
    not leak."""
    nx, ny, nz = shape
    rng = np.random.default_rng(_seed(shape, 65281))
    col = rng.integers(0, 65281, (nz, ny, nx, 4), dtype=np.uint16)
    col[..., 3] = rng.integers(0, 3, (nz, ny, nx)) * 128
    return col
