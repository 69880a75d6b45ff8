"""Stage 4 of include/emf_hip.h "Planes"  restated on the host: a helper, not a test file.

The device stage, stated twice:
    patch_ids       vectorised: the record indices scattered into a dense volume, the links of the half neighbourhood
                    read off shifted views of it, components by scipy.sparse.csgraph, ids remapped to the smallest
                    record index (patch_ids_label: the same at reach 1 by scipy.ndimage.label per label)
    patch_ids_loop  a plain loop: union-find over a dict keyed by voxel
    patch_records / patch_records_loop   the records of all patches in ascending id order, extents in np.float32
Host steps in Python floats (float64, one operation per line): rect, support, rests_on.
Fixtures: two_slabs, doorway, recurring."""
import math

import numpy as np

from tests import planes_reference as pr

PATCH = np.dtype([("id", "<i4"), ("plane", "<i4"), ("count", "<u8"), ("sum", "<u8", 3), ("sum2", "<u8", 6), ("lo", "<i4", 3),
                  ("hi", "<i4", 3), ("ulo", "<f4"), ("uhi", "<f4"), ("vlo", "<f4"), ("vhi", "<f4")])
MAX_REACH = 2
KEPT, PATCHES, MEMBERS = 0, 1, 2
f32 = np.float32


def half_offsets(reach):
    """The offsets (dx, dy, dz) that precede (0, 0, 0) in (z, y, x) order: 13 at reach 1, 62 at reach 2."""
    r = range(-reach, reach + 1)
    return [(dx, dy, dz) for dz in r for dy in r for dx in r if (dz, dy, dx) < (0, 0, 0)]


def _valid(rec, size):
    index = rec["index"].astype(np.int64)
    return (index >= 0) & (index < size[0] * size[1] * size[2])


def patch_ids(rec, labels, size, reach):
    """patch (i32 per record): the smallest record index of the record's component, -1 where labels < 0."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(rec)
    labels = np.asarray(labels)[:n]
    out = np.full(n, -1, np.int32)
    if n == 0:
        return out
    live = (labels >= 0) & _valid(rec, size)
    x, y, z = pr.voxel_of(np.where(live, rec["index"], 0), size)
    dense = np.full((size[2] + 2 * reach, size[1] + 2 * reach, size[0] + 2 * reach), -1, np.int64)
    who = np.nonzero(live)[0]
    dense[z[who] + reach, y[who] + reach, x[who] + reach] = who
    a, b = [], []
    for dx, dy, dz in half_offsets(reach):
        other = dense[z[who] + reach + dz, y[who] + reach + dy, x[who] + reach + dx]
        link = other >= 0
        link[link] = labels[other[link]] == labels[who[link]]
        a.append(who[link])
        b.append(other[link])
    a, b = np.concatenate(a), np.concatenate(b)
    _, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)), directed=False)
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    members = labels >= 0  # a member without a voxel links nothing: a patch of its own
    out[members] = first[comp[members]]
    return out


def patch_ids_label(rec, labels, size):
    """The same at reach 1 by scipy.ndimage.label with the full 3 x 3 x 3 structure, plane by plane."""
    from scipy import ndimage
    n = len(rec)
    labels = np.asarray(labels)[:n]
    out = np.full(n, -1, np.int32)
    x, y, z = pr.voxel_of(rec["index"], size)
    for k in np.unique(labels[labels >= 0]):
        who = np.nonzero(labels == k)[0]
        dense = np.zeros((size[2], size[1], size[0]), bool)
        dense[z[who], y[who], x[who]] = True
        comp, count = ndimage.label(dense, structure=np.ones((3, 3, 3), bool))
        mine = comp[z[who], y[who], x[who]]
        first = np.full(count + 1, n, np.int64)
        np.minimum.at(first, mine, who)
        out[who] = first[mine]
    return out


def patch_ids_loop(rec, labels, size, reach):
    n = len(rec)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    voxels = {}
    total = size[0] * size[1] * size[2]
    for i in range(n):
        index = int(rec["index"][i])
        if labels[i] >= 0 and 0 <= index < total:
            row = index // size[0]
            voxels[(index - row * size[0], row % size[1], row // size[1])] = i
    for (x, y, z), i in voxels.items():
        for dx in range(-reach, reach + 1):
            for dy in range(-reach, reach + 1):
                for dz in range(-reach, reach + 1):
                    j = voxels.get((x + dx, y + dy, z + dz))
                    if j is not None and labels[j] == labels[i]:
                        a, b = find(i), find(j)
                        if a != b:
                            parent[max(a, b)] = min(a, b)
    return np.array([find(i) if labels[i] >= 0 else -1 for i in range(n)], np.int32).reshape(n)


def patch_records(rec, labels, patch, size, axes):
    """One PATCH record per patch, ascending id: integer moments and bounds of the members, and the extents of
    e = (a0 * x + a1 * y) + a2 * z in float32 along the two axes (axes: P x 6 f32) of the members' plane."""
    axes = np.asarray(axes, f32).reshape(-1, 6)
    n = len(rec)
    labels, patch = np.asarray(labels)[:n], np.asarray(patch)[:n]
    ok = _valid(rec, size)
    x, y, z = pr.voxel_of(np.where(ok, rec["index"], 0), size)
    who = np.nonzero(patch >= 0)[0]
    ids, slot = np.unique(patch[who], return_inverse=True)
    out = np.zeros(len(ids), PATCH)
    if len(ids) == 0:
        return out
    out["id"], out["plane"] = ids, labels[ids]
    c = [v[who].astype(np.uint64) for v in (x, y, z)]
    np.add.at(out["count"], slot, np.uint64(1))
    out["lo"], out["hi"] = size, -1
    for j in range(3):
        np.add.at(out["sum"][:, j], slot, c[j])
        np.minimum.at(out["lo"][:, j], slot, c[j].astype(np.int32))
        np.maximum.at(out["hi"][:, j], slot, c[j].astype(np.int32))
    for j, (p, q) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
        np.add.at(out["sum2"][:, j], slot, c[p] * c[q])
    out["ulo"] = out["vlo"] = np.inf
    out["uhi"] = out["vhi"] = -np.inf
    has = labels[who] < len(axes)  # a label without axes adds nothing to the extents
    a = axes[np.where(has, labels[who], 0)]
    fx, fy, fz = (v.astype(f32) for v in c)
    with np.errstate(all="ignore"):
        eu = (a[:, 0] * fx + a[:, 1] * fy) + a[:, 2] * fz
        ev = (a[:, 3] * fx + a[:, 4] * fy) + a[:, 5] * fz
    np.minimum.at(out["ulo"], slot[has], eu[has])
    np.maximum.at(out["uhi"], slot[has], eu[has])
    np.minimum.at(out["vlo"], slot[has], ev[has])
    np.maximum.at(out["vhi"], slot[has], ev[has])
    return out


def patch_records_loop(rec, labels, patch, size, axes):
    axes = np.asarray(axes, f32).reshape(-1, 6)
    slots = {}
    for i in range(len(rec)):
        if patch[i] < 0:
            continue
        v = [int(c) for c in pr.voxel_of(rec["index"][i], size)]
        m = slots.get(int(patch[i]))
        if m is None:
            m = slots[int(patch[i])] = np.zeros((), PATCH)
            m["id"], m["plane"] = patch[i], labels[patch[i]]
            m["lo"], m["hi"] = size, -1
            m["ulo"] = m["vlo"] = np.inf
            m["uhi"] = m["vhi"] = -np.inf
        m["count"] += 1
        for j in range(3):
            m["sum"][j] += v[j]
            m["lo"][j], m["hi"][j] = min(m["lo"][j], v[j]), max(m["hi"][j], v[j])
        for j, (p, q) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
            m["sum2"][j] += v[p] * v[q]
        if labels[i] < len(axes):
            a = axes[labels[i]]
            fx, fy, fz = f32(v[0]), f32(v[1]), f32(v[2])
            eu = (a[0] * fx + a[1] * fy) + a[2] * fz
            ev = (a[3] * fx + a[4] * fy) + a[5] * fz
            m["ulo"], m["uhi"] = min(m["ulo"], eu), max(m["uhi"], eu)
            m["vlo"], m["vhi"] = min(m["vlo"], ev), max(m["vhi"], ev)
    out = np.zeros(len(slots), PATCH)
    for s, i in enumerate(sorted(slots)):
        out[s] = slots[i]
    return out


def emitted(records, min_count, n_patches, capacity_patches):
    """(the records the device writes, the kept counter): of the first n_patches patches those of at least min_count
    members, in id order, at most capacity_patches of them."""
    first = records[:n_patches]
    kept = first[first["count"] >= min_count]
    return kept[:capacity_patches], len(kept)


def counters(labels, patch, kept):
    patch = np.asarray(patch)
    return np.array([kept, len(np.unique(patch[patch >= 0])), int((np.asarray(labels) >= 0).sum())], np.uint32)


# ---- the host steps, Python floats --------------------------------------------------------------------------------

def rect(plane, patch):
    """dict(fit, center, half, corners, fill) of a patch from its plane dict (n, d, axes of planes_reference.fit), box
    voxel coordinates, in the operation order of include/emf_hip.h."""
    mom = np.zeros((), pr.MOMENTS)
    for k in ("count", "sum", "sum2", "lo", "hi"):
        mom[k] = patch[k]
    n, d = [float(v) for v in plane["n"]], float(plane["d"])
    fit = pr.fit(mom, n, d)
    if plane.get("axes") is None:
        u, v = [0.0] * 3, [0.0] * 3
    else:
        u, v = [float(c) for c in plane["axes"][0]], [float(c) for c in plane["axes"][1]]
    a0 = float(patch["ulo"]) - 0.5
    a1 = float(patch["uhi"]) + 0.5
    b0 = float(patch["vlo"]) - 0.5
    b1 = float(patch["vhi"]) + 0.5
    cu = (a0 + a1) * 0.5
    hu = (a1 - a0) * 0.5
    cv = (b0 + b1) * 0.5
    hv = (b1 - b0) * 0.5

    def point(eu, ev):
        out = []
        for j in range(3):
            s = d * n[j]
            t = u[j] * eu
            s = s + t
            t = v[j] * ev
            s = s + t
            out.append(s)
        return out

    corners = []
    for su, sv in ((-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)):
        eu = cu + su * hu
        ev = cv + sv * hv
        corners.append(point(eu, ev))
    wu = float(patch["uhi"]) - float(patch["ulo"])
    wu = wu + 1.0
    wv = float(patch["vhi"]) - float(patch["vlo"])
    wv = wv + 1.0
    nmax = max(abs(n[0]), abs(n[1]), abs(n[2]))
    area = wu * wv
    area = area * nmax
    return dict(fit=fit, center=point(cu, cv), half=[hu, hv], corners=corners, fill=float(int(patch["count"])) / area)


def support(n, d, center, axes, half, box_center, box_axes, box_half, margin):
    """(s, over) of one oriented box against one patch, world metres: s is the height of the box's lowest point above
    the patch's plane, over says whether the box centre lies above the rectangle widened by margin."""
    s = n[0] * box_center[0]
    s = s + n[1] * box_center[1]
    s = s + n[2] * box_center[2]
    s = s - d
    for k in range(3):
        a = n[0] * box_axes[k][0]
        a = a + n[1] * box_axes[k][1]
        a = a + n[2] * box_axes[k][2]
        s = s - abs(a) * box_half[k]
    q = [box_center[0] - center[0], box_center[1] - center[1], box_center[2] - center[2]]
    over = True
    for j in range(2):
        a = q[0] * axes[j][0]
        a = a + q[1] * axes[j][1]
        a = a + q[2] * axes[j][2]
        over = over and abs(a) <= half[j] + margin
    return s, over


def rests_on(patches, box, gap=0.05, margin=0.0):
    """(index into patches, s) of the patch the box rests on, or None: the smallest |s| among the floor and level
    patches it is over with |s| <= gap; ties to the earlier patch."""
    best = None
    for k, p in enumerate(patches):
        if p["kind"] not in ("floor", "level"):
            continue
        s, over = support(p["normal"], p["d"], p["rect"]["center"], p["rect"]["axes"], p["rect"]["half_m"], box["center"],
                          box["axes"], box["half"], margin)
        if over and abs(s) <= gap and (best is None or abs(s) < abs(best[1])):
            best = (k, s)
    return best


# ---- fixtures ------------------------------------------------------------------------------------------------------

SLABS = (((6, 7, 6), (20, 20, 40)), ((28, 7, 8), (44, 20, 22)))  # (lo, hi) in voxels: 14 x 34 and 16 x 14, one top level
FLOOR = 6.0


def _box_sd(p, lo, hi):
    """The signed distance of the points p (..., 3) to the solid box [lo - 0.5, hi - 0.5]: the voxels lo .. hi - 1."""
    c = (np.asarray(lo, np.float64) + np.asarray(hi, np.float64) - 1.0) / 2.0
    h = (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / 2.0
    q = np.abs(p - c) - h
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def two_slabs(noise=0.0, tilt=0.0, seed=3, trunc=3.0):
    """(tsdf, weights) of a 48^3 scene: a floor (free space above y = 6) and two separate slabs standing on it whose top
    faces lie on one level.  tilt: the scene turned by that many degrees about the axis (1, 0, 1) through the centre;
    noise: Gaussian noise on the tsdf."""
    n = 48
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    p = np.stack([x, y, z], -1).astype(np.float64)
    if tilt:
        k = np.array([1.0, 0.0, 1.0]) / math.sqrt(2.0)
        t = math.radians(tilt)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
        c = np.full(3, (n - 1) / 2.0)
        p = (p - c) @ R + c  # the scene's own coordinates of every voxel
    sd = p[..., 1] - FLOOR
    for lo, hi in SLABS:
        sd = np.minimum(sd, _box_sd(p, lo, hi))
    tsdf = np.clip(sd / trunc, -1.0, 1.0)
    if noise:
        tsdf = tsdf + np.random.default_rng(seed).normal(0.0, noise, tsdf.shape)
    return tsdf.astype(f32), (sd > -trunc).astype(f32)


def doorway():
    """(records, labels, size): one wall plane x = 5 of a 16 x 24 x 12 box, labelled 0, with a gap of 4 voxels (z = 4 .. 7)
    over its full height: two patches at either reach."""
    size = (16, 24, 12)
    vox = [(5, y, z) for z in range(size[2]) for y in range(size[1]) if not 4 <= z < 8]
    return records_of(vox, size), np.zeros(len(vox), np.int16), size


def records_of(vox, size):
    """VOXEL records of the voxels (x, y, z) in stage 1's order, gradient (1, 0, 0)."""
    v = np.asarray(vox, np.int64).reshape(-1, 3)
    order = pr.tile_order(v[:, 0], v[:, 1], v[:, 2], size)
    v = v[order]
    rec = np.zeros(len(v), pr.VOXEL)
    rec["index"] = (v[:, 2] * size[1] + v[:, 1]) * size[0] + v[:, 0]
    rec["g"] = (1.0, 0.0, 0.0)
    return rec


def recurring():
    """(records, labels, size): 64 records, one wave of the statistics kernel, in stage 1's order, all in the plane z = 0
    of one tile.  Rows y = 0, 1, 2 hold x = 0 .. 15 with labels A, B, A; rows y = 0 .. 3 hold x = 20 .. 23 with label A.
    At reach 1 that is p (row 0), q (row 1, label B), s (row 2, two rows from p) and the block r, five voxels from the
    rows.  In record order the patches read p, r, q, r, s, r: the label A comes back after B, and the patch r comes
    back after q and, within one label, after s.  A sum over a run must not cross to an earlier run of the same patch."""
    size = (32, 8, 8)
    vox, lab = [], []
    for y, label in ((0, 0), (1, 1), (2, 0)):
        for x in range(16):
            vox.append((x, y, 0))
            lab.append(label)
    for y in range(4):
        for x in range(20, 24):
            vox.append((x, y, 0))
            lab.append(0)
    v = np.asarray(vox, np.int64)
    order = pr.tile_order(v[:, 0], v[:, 1], v[:, 2], size)
    return records_of(vox, size), np.asarray(lab, np.int16)[order], size
