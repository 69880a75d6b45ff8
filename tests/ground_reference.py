"""A restatement of the ground map (include/emf_hip.h "Ground map") for the tests: the slot of a voxel
by explicit np.float32 operations in the stated order, the bit planes twice (np.bitwise_or.at, and a plain Python loop
over the voxels), the cell records and the 2-D classes as loops over Python ints, and the frame in Python floats.
Nothing here is fast and nothing here touches a device."""
import math

import numpy as np

FREE, OCCUPIED, UNKNOWN = 0, 1, 2
CELL_DTYPE = np.dtype([("floor", "<i2"), ("top", "<i2"), ("clear", "<i2"), ("levels", "<i2")])
MAX_AXIS, MAX_BINS = 2048, 256


def words_of(bins):
    return (int(bins) + 63) // 64


def slots(size, G, W, H, B):
    """(iu, iv, ih, keep) of every voxel of a box of size (x, y, z), each (nz, ny, nx): q_j = ((G_j0 x + G_j1 y) + G_j2 z)
    + G_j3 in single float32 operations, floor, and the range test in float before any cast."""
    nx, ny, nz = (int(v) for v in size)
    G = np.asarray(G, np.float32).reshape(3, 4)
    x = np.arange(nx, dtype=np.float32)[None, None, :]
    y = np.arange(ny, dtype=np.float32)[None, :, None]
    z = np.arange(nz, dtype=np.float32)[:, None, None]
    out = []
    keep = np.ones((nz, ny, nx), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, n in enumerate((W, H, B)):
            a = (G[j, 0] * x).astype(np.float32)
            b = (G[j, 1] * y).astype(np.float32)
            c = (G[j, 2] * z).astype(np.float32)
            q = ((((a + b).astype(np.float32) + c).astype(np.float32)) + G[j, 3]).astype(np.float32)
            q = np.broadcast_to(q, (nz, ny, nx))
            i = np.floor(q)
            assert i.dtype == np.float32
            keep &= (i >= np.float32(0)) & (i < np.float32(n))  # a NaN fails both
            out.append(i)
    ints = [np.where(keep, i, 0).astype(np.int64) for i in out]
    return ints[0], ints[1], ints[2], keep


def planes(classes, G, W, H, B):
    """(occ, fre), each (H, W, words) u64, of a (nz, ny, nx) u8 class volume, by np.bitwise_or.at."""
    classes = np.asarray(classes, np.uint8)
    nz, ny, nx = classes.shape
    iu, iv, ih, keep = slots((nx, ny, nz), G, W, H, B)
    words = words_of(B)
    out = []
    for cls in (OCCUPIED, FREE):
        plane = np.zeros(H * W * words, np.uint64)
        m = keep & (classes == cls)
        dest = (iv[m] * W + iu[m]) * words + (ih[m] >> 6)
        bits = np.uint64(1) << (ih[m] & 63).astype(np.uint64)
        np.bitwise_or.at(plane, dest, bits)
        out.append(plane.reshape(H, W, words))
    return out[0], out[1]


def planes_loop(classes, G, W, H, B):
    """The same planes once more: a plain loop over the voxels, one np.float32 scalar operation at a time."""
    classes = np.asarray(classes, np.uint8)
    nz, ny, nx = classes.shape
    G = np.asarray(G, np.float32).reshape(3, 4)
    words = words_of(B)
    occ = [[[0] * words for _ in range(W)] for _ in range(H)]
    fre = [[[0] * words for _ in range(W)] for _ in range(H)]
    limits = (np.float32(W), np.float32(H), np.float32(B))
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    c = int(classes[z, y, x])
                    if c > 1:
                        continue
                    idx = []
                    for j in range(3):
                        q = f32(f32(f32(f32(G[j, 0] * f32(x)) + f32(G[j, 1] * f32(y))) + f32(G[j, 2] * f32(z))) + G[j, 3])
                        i = f32(math.floor(q)) if math.isfinite(q) else q
                        if not (i >= f32(0) and i < limits[j]):
                            idx = None
                            break
                        idx.append(int(i))
                    if idx is None:
                        continue
                    iu, iv, ih = idx
                    (occ if c == OCCUPIED else fre)[iv][iu][ih >> 6] |= 1 << (ih & 63)
    return np.array(occ, np.uint64).reshape(H, W, words), np.array(fre, np.uint64).reshape(H, W, words)


def column_states(occ_words, fre_words, B):
    """The slot states of one column as a string of 'O', 'F', 'U', bin 0 first."""
    o = sum(int(w) << (64 * k) for k, w in enumerate(occ_words))
    f = sum(int(w) << (64 * k) for k, w in enumerate(fre_words))
    return "".join("O" if (o >> k) & 1 else ("F" if (f >> k) & 1 else "U") for k in range(B))


def cell_of_states(states, R):
    """(floor, top, clear, levels) of a column given as a string of 'O' / 'F' / 'U', for a robot of R bins: the
    definition, word for word."""
    B = len(states)
    floor, top, clear, levels = -1, -1, 0, 0
    for k in range(B):
        if states[k] != "O":
            continue
        top = k
        standable = k + R <= B - 1 and all(states[j] == "F" for j in range(k + 1, k + R + 1))
        if standable:
            levels += 1
            if floor < 0:
                floor = k
                j = k + 1
                while j < B and states[j] == "F":
                    j += 1
                clear = j - (k + 1)
    return floor, top, clear, levels


def cells(occ, fre, B, R):
    """The (H, W) CELL_DTYPE records of (H, W, words) planes."""
    H, W, _ = occ.shape
    out = np.zeros((H, W), CELL_DTYPE)
    for v in range(H):
        for u in range(W):
            out[v, u] = cell_of_states(column_states(occ[v, u], fre[v, u], B), R)
    return out


def classes2d(records, S):
    """The (1, H, W) u8 classes of (H, W) cell records for a largest step of S bins."""
    H, W = records.shape
    out = np.zeros((1, H, W), np.uint8)
    for v in range(H):
        for u in range(W):
            floor, top = int(records[v, u]["floor"]), int(records[v, u]["top"])
            if floor < 0:
                out[0, v, u] = OCCUPIED if top >= 0 else UNKNOWN
                continue
            cls = FREE
            for dv in (-1, 0, 1):
                for du in (-1, 0, 1):
                    nu, nv = u + du, v + dv
                    if (du == 0 and dv == 0) or not (0 <= nu < W and 0 <= nv < H):
                        continue
                    fn = int(records[nv, nu]["floor"])
                    if fn >= 0 and abs(floor - fn) > S:
                        cls = OCCUPIED
            out[0, v, u] = cls
    return out


def ground_map(classes, G, W, H, B, R, S):
    """(occ, fre, cells, classes2d) of a class volume."""
    occ, fre = planes(classes, G, W, H, B)
    rec = cells(occ, fre, B, R)
    return occ, fre, rec, classes2d(rec, S)


class FrameError(ValueError):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


E_ARG, E_LIMIT = -4, -5  # EMF_E_ARG, EMF_E_LIMIT of include/emf_hip.h


def frame(lo, size, res, voxel, R, t, up, cell, bin, ref, band, max_axis=MAX_AXIS):
    """The frame of a ground map in Python floats, one operation per line in the order of the header: returns
    (G (3, 4) f32, W, H, B, pose (12,) f64 = R row-major with (u, v, h) as columns, then t)."""
    lo, size, res = ([int(v) for v in a] for a in (lo, size, res))
    vs = float(np.float32(voxel))
    R = [float(v) for v in np.asarray(R, np.float32).reshape(9)]
    t = [float(v) for v in np.asarray(t, np.float32).reshape(3)]
    up, ref = [float(v) for v in up], [float(v) for v in ref]
    cell, bin, band_lo, band_hi = float(cell), float(bin), float(band[0]), float(band[1])
    if not all(math.isfinite(v) for v in up + ref):
        raise FrameError(E_ARG, "a non-finite up or reference")
    if not (cell > 0.0 and bin > 0.0 and math.isfinite(cell) and math.isfinite(bin)):
        raise FrameError(E_ARG, "cell and bin must be positive metres")
    if not (math.isfinite(band_lo) and math.isfinite(band_hi) and band_hi > band_lo):
        raise FrameError(E_ARG, "the height band is empty")
    s = up[0] * up[0]
    s = s + up[1] * up[1]
    s = s + up[2] * up[2]
    length = math.sqrt(s)
    if not (length > 0.0 and math.isfinite(length)):
        raise FrameError(E_ARG, "up has no direction")
    h = [up[i] / length for i in range(3)]
    for column in (0, 2):
        a = [R[column], R[3 + column], R[6 + column]]
        d = a[0] * h[0]
        d = d + a[1] * h[1]
        d = d + a[2] * h[2]
        w = []
        for i in range(3):
            along = d * h[i]
            w.append(a[i] - along)
        n2 = w[0] * w[0]
        n2 = n2 + w[1] * w[1]
        n2 = n2 + w[2] * w[2]
        if not n2 < 1e-6:
            break
    wl = math.sqrt(n2)
    u = [w[i] / wl for i in range(3)]
    v = []
    for i, j in ((1, 2), (2, 0), (0, 1)):
        a = h[i] * u[j]
        b = h[j] * u[i]
        v.append(a - b)
    E = [u, v, h]
    # the world point of box voxel (0, 0, 0), as QueryBox::worldPoint
    c = []
    for i in range(3):
        half = (float(res[i]) - 1.0) / 2.0
        off = float(lo[i]) - half
        c.append((0.0 + off) * vs)
    p0 = []
    for i in range(3):
        q = R[3 * i] * c[0]
        q = q + R[3 * i + 1] * c[1]
        q = q + R[3 * i + 2] * c[2]
        q = q + t[i]
        p0.append(q)
    M, g = [], []
    for j in range(3):
        row = []
        for k in range(3):
            m = E[j][0] * R[k]
            m = m + E[j][1] * R[3 + k]
            m = m + E[j][2] * R[6 + k]
            row.append(m * vs)
        M.append(row)
        q = E[j][0] * p0[0]
        q = q + E[j][1] * p0[1]
        q = q + E[j][2] * p0[2]
        g.append(q)
    A, mn, dims = [], [], []
    for j in range(2):
        row = [M[j][k] / cell for k in range(3)]
        a = g[j] / cell
        lo_q = hi_q = None
        for corner in range(8):
            b = [float(size[k]) - 0.5 if (corner >> k) & 1 else -0.5 for k in range(3)]
            q = row[0] * b[0]
            q = q + row[1] * b[1]
            q = q + row[2] * b[2]
            q = q + a
            lo_q = q if lo_q is None or q < lo_q else lo_q
            hi_q = q if hi_q is None or q > hi_q else hi_q
        mn.append(lo_q)
        row.append(a - lo_q)
        A.append(row)
        n = math.floor(hi_q - lo_q) + 1.0
        if not n <= max_axis:
            raise FrameError(E_LIMIT, "the map has too many cells on an axis")
        dims.append(int(n))
    row = [M[2][k] / bin for k in range(3)]
    z0 = h[0] * ref[0]
    z0 = z0 + h[1] * ref[1]
    z0 = z0 + h[2] * ref[2]
    z0 = z0 + band_lo
    above = g[2] - z0
    row.append(above / bin)
    A.append(row)
    span = band_hi - band_lo
    bins = math.ceil(span / bin)
    if not bins >= 1:
        raise FrameError(E_ARG, "the height band holds no bin")
    if not bins <= MAX_BINS:
        raise FrameError(E_LIMIT, "too many height bins")
    G = np.array(A, np.float64).astype(np.float32)
    ou = mn[0] * cell
    ov = mn[1] * cell
    pose = np.zeros(12, np.float64)
    for i in range(3):
        pose[3 * i], pose[3 * i + 1], pose[3 * i + 2] = u[i], v[i], h[i]
        o = u[i] * ou
        o = o + v[i] * ov
        o = o + h[i] * z0
        pose[9 + i] = o
    return G, dims[0], dims[1], int(bins), pose


def ground_point(pose, cu, cv, ch):
    """Ground metres -> world, float64: ((o + u cu) + v cv) + h ch, per component."""
    pose = np.asarray(pose, np.float64)
    out = []
    for i in range(3):
        q = pose[9 + i] + pose[3 * i] * np.asarray(cu, np.float64)
        q = q + pose[3 * i + 1] * np.asarray(cv, np.float64)
        q = q + pose[3 * i + 2] * np.asarray(ch, np.float64)
        out.append(q)
    return np.stack(np.broadcast_arrays(*out), axis=-1)


def aligned(G):
    """In every row of G[:, :3] all entries but the largest are at most 2^-20 of it (float32)."""
    G = np.abs(np.asarray(G, np.float32).reshape(3, 4)[:, :3])
    return all(int((row > row.max() * np.float32(2.0 ** -20)).sum()) == 1 for row in G)


def rotation(axis, degrees):
    """A rotation matrix (float64) about `axis` by `degrees` (Rodrigues)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


# ---- fixtures the tests share -------------------------------------------------------------------------------------

# box shapes (x, y, z): the tile edges (32 x 8 x 8) and the ragged 16-byte rows
SHAPES = [(1, 1, 1), (65, 1, 1), (2, 5, 3), (32, 8, 8), (31, 8, 7), (33, 9, 8), (65, 17, 9), (70, 21, 19), (2048, 2, 1)]
CONTENTS = ["unknown", "free", "occupied", "random", "scene", "bytes_above_2"]
BINS = [1, 63, 64, 65, 256]
AXES = [(k, s) for k in range(3) for s in (1, -1)]
# frame specs: the six axis-aligned ups at cells of 1, 2 and 3 voxels, two tilted ups at 2 and 3, a frame that maps every
# voxel outside the map and a frame with a NaN entry
FRAME_SPECS = ([("axis", k, s, c) for c in (1, 2, 3) for k, s in AXES] + [("tilt20", c) for c in (2, 3)] +
               [("generic", c) for c in (2, 3)] + [("outside",), ("nan",)])
GENERIC_R = rotation((0.3, -0.8, 0.52), 37.0).astype(np.float32)
GENERIC_T = np.array([0.1, -0.2, 0.3], np.float32)


def volume(shape, content, seed=0):
    """A (nz, ny, nx) u8 class volume of a box of `shape` (x, y, z)."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed + 7919 * (nx + 31 * ny + 977 * nz))
    if content in ("unknown", "free", "occupied"):
        return np.full((nz, ny, nx), {"unknown": UNKNOWN, "free": FREE, "occupied": OCCUPIED}[content], np.uint8)
    if content == "random":  # about 30 % known
        r = rng.random((nz, ny, nx))
        return np.where(r < 0.15, FREE, np.where(r < 0.30, OCCUPIED, UNKNOWN)).astype(np.uint8)
    if content == "bytes_above_2":
        v = rng.integers(0, 256, (nz, ny, nx)).astype(np.uint8)
        v[rng.random((nz, ny, nx)) < 0.3] = FREE
        return v
    assert content == "scene"
    # up is +z: a floor slab at z = 1 with free space above it, a box on it, a table (a plate with free space under it)
    # and a pole one voxel thick; whatever does not fit a small shape is clipped away
    v = np.full((nz, ny, nx), UNKNOWN, np.uint8)
    v[2:max(nz - 1, 2), :, :] = FREE
    v[1:2, :, :] = OCCUPIED
    v[2:6, ny // 4:ny // 2, nx // 8:nx // 4] = OCCUPIED           # the box
    v[5:6, ny // 2:, nx // 2:3 * nx // 4] = OCCUPIED              # a low table: 3 free voxels under the plate
    v[12:13, : ny // 2, 3 * nx // 4:] = OCCUPIED                  # a high table: 10 free voxels under it
    if nx > 7 and ny > 4:
        v[2:max(nz - 1, 2), 4, 7] = OCCUPIED                      # the pole, inside the cell (2, 1) of 3 voxels
    return v


def spec_frame(shape, spec, bins):
    """(G (3, 4) f32, W, H, B) of a frame spec on a box of `shape`: through frame() for a background that is the box
    itself, with the band's lower end at the box's lower face along up (voxel 1) and `bins` bins of one cell each."""
    kind = spec[0]
    R, t, voxel = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 1.0
    ref = (0.0, 0.0, 0.0)
    if kind in ("axis", "nan"):
        k, s, c = spec[1:] if kind == "axis" else (2, 1, 2)
        up = [0.0, 0.0, 0.0]
        up[k] = float(s)
        extent = shape[k]
    elif kind in ("tilt20", "outside"):
        c = spec[1] if kind == "tilt20" else 2
        up = rotation((1, 0, 0), 20.0) @ np.array([0.0, 0.0, 1.0])
        extent = shape[2]
        if kind == "outside":
            ref = (0.0, 0.0, 4096.0)
    else:
        c = spec[1]
        R, t, voxel = GENERIC_R, GENERIC_T, 0.05
        up = (0.3, -0.5, 0.8)
        extent = shape[2]
        ref = tuple(float(v) for v in t)
    vs = float(np.float32(voxel))
    cell = c * vs
    lo = -extent * vs / 2.0
    G, W, H, B, _ = frame((0, 0, 0), shape, shape, voxel, R, t, up, cell, cell, ref, (lo, lo + (bins - 0.5) * cell),
                          max_axis=2 * MAX_AXIS)
    assert B == bins, (B, bins)
    # a face of the box that falls exactly on a cell boundary opens one more, empty cell: 2049 for 2048 voxels at a cell of
    # one.  The entries take any frame, so the map is cut at their limit; what would land beyond it is dropped
    W, H = min(W, MAX_AXIS), min(H, MAX_AXIS)
    if kind == "nan":
        G = G.copy()
        G[1, 2] = np.nan
    return G, W, H, B


def kernel_cases():
    """[(shape, content, spec, bins, robot, step)]: every shape meets every frame spec once and every content four times;
    bins, robot heights (1, 5, B) and steps (0, 2) rotate."""
    out = []
    n = len(FRAME_SPECS)
    for si, shape in enumerate(SHAPES):
        for fi in range(n):
            spec = FRAME_SPECS[(fi + 5 * si) % n]
            content = CONTENTS[fi % len(CONTENTS)]
            bins = BINS[(fi // len(CONTENTS) + fi + si) % len(BINS)]
            robot = (1, 5, bins)[(fi + si) % 3]
            out.append((shape, content, spec, bins, robot, (0, 2)[(fi // 3 + si) % 2]))
    # the scene where it means something: up along +z and tilted, overhangs lower and higher than the robot
    for k, spec in enumerate([("axis", 2, 1, 1), ("axis", 2, 1, 2), ("axis", 2, 1, 3), ("tilt20", 2), ("tilt20", 3), ("generic", 2)]):
        for robot in (1, 5):
            out.append(((70, 21, 19), "scene", spec, (63, 64, 65)[k % 3], robot, (0, 2)[(k + robot) % 2]))
    return out
