"""Restatement of include/emf_hip.h "Frontiers"  for the tests, in numpy and scipy: the flags from
shifted comparisons of the class array, the clusters from scipy.ndimage.label with the full 3 x 3 x 3 structure,
relabelled to the smallest linear index, the statistics in int64, the representative from the 64-bit key the header
defines, the filter, the two orders (label order: the kernels; count descending: the session) and the world points in
float64, rounded once to float32.  Everything but the world points is an integer: comparisons are tobytes()."""
import numpy as np
from scipy import ndimage

FREE, OCCUPIED, UNKNOWN = 0, 1, 2
FAR = 0x7fffffff
KEPT, CLUSTERS, VOXELS = 0, 1, 2

RECORD = np.dtype([("label", "<i4"), ("count", "<i4"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("sum", "<u8", 3),
                   ("rep", "<i4", 3), ("reserved", "<i4")])
assert RECORD.itemsize == 72

# (nz, ny, nx): the chunk carries of a row (63, 64, 65, more than two chunks), an axis of 1, the longest row
SHAPES = [(3, 3, 1), (1, 1, 70), (1, 7, 33), (6, 9, 1), (4, 5, 63), (4, 5, 64), (4, 5, 65), (3, 4, 130),
          (2, 3, 600), (2, 600, 3), (600, 3, 2), (9, 17, 65), (1, 1, 2048)]
CONTENTS = ["all_free", "all_unknown", "random_a", "random_b", "checker", "lattice", "serpentine", "halves", "row_ends"]
SEEDS = {"random_a": 0xF0, "random_b": 0xF1}


def class_field(shape, content):
    """u8 (nz, ny, nx) classes of a named content."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = np.full(shape, UNKNOWN, np.uint8)
    if content == "all_free":
        c[:] = FREE
    elif content == "all_unknown":
        pass
    elif content in SEEDS:  # 3 is no class: neither free nor unknown
        c = np.random.default_rng([SEEDS[content], nz, ny, nx]).integers(0, 4, shape).astype(np.uint8)
    elif content == "checker":  # every free voxel touches unknown and its free diagonal neighbours: one cluster
        c[(x + y + z) % 2 == 0] = FREE
    elif content == "lattice":  # isolated voxels, three apart: as many clusters as a box can hold, each of one voxel
        c[(x % 3 == 0) & (y % 3 == 0) & (z % 3 == 0)] = FREE
    elif content == "serpentine":
        c[tuple(np.array(serpentine_path(shape)).T)] = FREE
    elif content == "halves":  # two free blocks that share one corner only: their shells meet diagonally
        hz, hy, hx = (nz + 1) // 2, (ny + 1) // 2, (nx + 1) // 2
        c[:hz, :hy, :hx] = FREE
        c[hz:, hy:, hx:] = FREE
    elif content == "row_ends":
        # free at the last voxel of every even row and the first of every odd row (rows counted through the slices):
        # neighbours in linear index across every row end and slice end, neighbours in space only where the box is
        # two voxels wide
        row = z * ny + y
        c[(row % 2 == 0) & (x == nx - 1)] = FREE
        c[(row % 2 == 1) & (x == 0)] = FREE
    else:
        raise AssertionError(content)
    return c


def serpentine_path(shape):
    """(z, y, x) of a one voxel wide walk through the whole box: whole rows at even y of even planes, joined by single
    voxels at alternating row ends in the odd rows and, in the odd planes, above the end of the plane below -- one
    cluster, hooked along its whole length."""
    nz, ny, nx = shape
    pts, x_dir, y_dir = [], 1, 1
    last_even_y = (ny - 1) - (ny - 1) % 2
    for z in range(0, nz, 2):
        ys = list(range(0, ny, 2)) if y_dir > 0 else list(range(last_even_y, -1, -2))
        x_end = 0
        for j, y in enumerate(ys):
            if j > 0:
                pts.append((z, y - y_dir, x_end))
            pts.extend((z, y, x) for x in range(nx))
            x_end = nx - 1 if x_dir > 0 else 0
            x_dir = -x_dir
        if z + 1 < nz:
            pts.append((z + 1, ys[-1], x_end))
        y_dir = -y_dir
    return pts


def d2_field(shape, seed=7):
    """A random i32 "d2" with values around the gates the tests use, EMF_DF_FAR among them."""
    rng = np.random.default_rng([seed, *shape])
    d2 = rng.integers(0, 7, shape).astype(np.int32)
    d2[rng.random(shape) < 0.1] = FAR
    return d2


def flags_of(classes, d2=None, min_d2=0):
    """bool (nz, ny, nx): the frontier voxels."""
    unknown = classes == UNKNOWN
    near = np.zeros(classes.shape, bool)
    for axis in range(3):
        n = classes.shape[axis]
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        near[tuple(lo)] |= unknown[tuple(hi)]  # the neighbour at +1
        near[tuple(hi)] |= unknown[tuple(lo)]  # the neighbour at -1
    f = (classes == FREE) & near
    if d2 is not None and min_d2 > 0:
        f &= d2.astype(np.int64) >= min_d2
    return f


def labels_of(flags):
    """i32 (nz, ny, nx): the smallest linear index of the voxel's 26-connected cluster, -1 off the frontier."""
    lab, n = ndimage.label(flags, structure=np.ones((3, 3, 3), bool))
    out = np.full(flags.size, -1, np.int32)
    idx = np.flatnonzero(flags)
    which = lab.reshape(-1)[idx]
    smallest = np.full(n + 1, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(smallest, which, idx)
    out[idx] = smallest[which]
    return out.reshape(flags.shape)


def records_of(labels):
    """Every cluster's record, in ascending label order."""
    nz, ny, nx = labels.shape
    flat = labels.reshape(-1).astype(np.int64)
    idx = np.flatnonzero(flat >= 0)
    roots = np.unique(flat[idx])
    slot = np.searchsorted(roots, flat[idx])
    xyz = np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], axis=1).astype(np.int64)
    m = len(roots)
    count = np.zeros(m, np.int64)
    np.add.at(count, slot, 1)
    total = np.zeros((m, 3), np.int64)
    lo = np.full((m, 3), np.iinfo(np.int64).max, np.int64)
    hi = np.full((m, 3), -1, np.int64)
    for a in range(3):
        np.add.at(total[:, a], slot, xyz[:, a])
        np.minimum.at(lo[:, a], slot, xyz[:, a])
        np.maximum.at(hi[:, a], slot, xyz[:, a])
    centre = (2 * total + count[:, None]) // (2 * count[:, None])
    dist2 = ((xyz - centre[slot]) ** 2).sum(axis=1)
    assert dist2.max(initial=0) < 1 << 24 and labels.size < 1 << 31
    key = np.full(m, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(key, slot, (dist2 << 31) | idx)
    rep = key & 0x7fffffff
    r = np.zeros(m, RECORD)
    r["label"], r["count"], r["lo"], r["hi"], r["sum"] = roots, count, lo, hi, total
    r["rep"] = np.stack([rep % nx, (rep // nx) % ny, rep // (nx * ny)], axis=1)
    return r


def keep(records, min_voxels):
    return records[records["count"] >= min_voxels]


def session_order(records):
    """count descending, ties by label ascending."""
    return records[np.lexsort((records["label"], -records["count"].astype(np.int64)))]


def frontiers(classes, d2=None, min_d2=0, min_voxels=1):
    """(labels, kept records in label order, (kept, clusters, voxels))."""
    labels = labels_of(flags_of(classes, d2, min_d2))
    every = records_of(labels)
    kept = keep(every, min_voxels)
    return labels, kept, (len(kept), len(every), int((labels >= 0).sum()))


def world_points(records, box_lo, res, voxel_size, R, t):
    """(centroid_world, rep_world), float32 (n, 3): sum / count or rep, plus box_lo - (res - 1) / 2, times the voxel
    size, through the pose (R, t) of the background volume -- in float64, rounded once."""
    off = np.asarray(box_lo, np.float64) - (np.asarray(res, np.float64) - 1) / 2
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)

    def through(v):
        p = (v + off) * np.float64(voxel_size)
        return (p @ R.T + t).astype(np.float32)

    centroid = records["sum"].astype(np.float64) / records["count"].astype(np.float64)[:, None]
    return through(centroid), through(records["rep"].astype(np.float64))
