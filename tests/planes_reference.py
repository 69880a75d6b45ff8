"""The plane finder of include/emf_hip.h "Planes"  restated on the host: a helper, not a test file.

Device stages, each stated twice -- vectorised numpy in float32 and a plain loop over np.float32 scalars:
    records / records_loop         surface voxels with a normal, in the tile order of the header
    direction_bins / _loop         the cube-map histogram
    offset_hist / _loop            the offset votes along given directions
    assign / assign_loop           labels and integer moments
Host steps between the stages in Python floats (float64, one operation per line):
    directions, offset_frame, offset_peaks, fit, find_planes, kinds
Every float32 step is one numpy float32 operation, so nothing is contracted."""
import math

import numpy as np

from tests import shape_reference as sr

VOXEL = np.dtype([("index", "<i4"), ("g", "<f4", 3)])
MOMENTS = np.dtype([("count", "<u8"), ("sum", "<u8", 3), ("sum2", "<u8", 6), ("lo", "<i4", 3), ("hi", "<i4", 3)])
TILE = (32, 8, 8)  # x, y, z
MAX_K, MAX_DIRS, MAX_SLOTS, MAX_PLANES = 31, 16, 4096, 64
f32 = np.float32


def _box(tsdf, box):
    nz, ny, nx = tsdf.shape
    return ((0, 0, 0), (nx, ny, nz)) if box is None else (tuple(box[0]), tuple(box[1]))


def tile_order(x, y, z, size):
    """The permutation that puts box voxels into the records' order."""
    ntx, nty = -(-size[0] // TILE[0]), -(-size[1] // TILE[1])
    tile = ((z // TILE[2]) * nty + y // TILE[1]) * ntx + x // TILE[0]
    within = ((z % TILE[2]) * TILE[1] + y % TILE[1]) * TILE[0] + x % TILE[0]
    return np.lexsort((within, tile))


def masks(tsdf, weights):
    """(surface, normal, g) of the WHOLE volume: two bool volumes and the (nz, ny, nx, 3) f32 differences."""
    obs = weights > 0
    solid = obs & ~(tsdf > 0)
    free = np.pad(obs & (tsdf > 0), 1)
    seen = np.pad(obs, 1)
    t = np.pad(tsdf, 1)
    c = slice(1, -1)
    lo, hi = slice(0, -2), slice(2, None)
    nbrs = [(c, c, lo), (c, c, hi), (c, lo, c), (c, hi, c), (lo, c, c), (hi, c, c)]
    any_free = np.zeros(tsdf.shape, bool)
    all_seen = np.ones(tsdf.shape, bool)
    for s in nbrs:
        any_free |= free[s]
        all_seen &= seen[s]
    inside = np.zeros(tsdf.shape, bool)
    inside[1:-1, 1:-1, 1:-1] = True  # all six neighbours lie inside the volume
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.stack([t[c, c, hi] - t[c, c, lo], t[c, hi, c] - t[c, lo, c], t[hi, c, c] - t[lo, c, c]], -1).astype(f32)
    surface = solid & any_free
    normal = surface & inside & all_seen & np.isfinite(g).all(-1) & (g != 0).any(-1)
    return surface, normal, g


def records(tsdf, weights, box=None):
    """(records, counters[0:2]) of the box: the VOXEL records in tile order, the surface and the normal counts."""
    lo, size = _box(tsdf, box)
    surface, normal, g = masks(tsdf, weights)
    crop = (slice(lo[2], lo[2] + size[2]), slice(lo[1], lo[1] + size[1]), slice(lo[0], lo[0] + size[0]))
    z, y, x = np.nonzero(normal[crop])
    order = tile_order(x, y, z, size)
    z, y, x = z[order], y[order], x[order]
    out = np.zeros(len(x), VOXEL)
    out["index"] = (z * size[1] + y) * size[0] + x
    out["g"] = g[crop][z, y, x]
    return out, (int(surface[crop].sum()), len(x))


def records_loop(tsdf, weights, box=None):
    lo, size = _box(tsdf, box)
    nz, ny, nx = tsdf.shape
    out, n_surface = [], 0
    steps = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    for tz in range(0, size[2], TILE[2]):
        for ty in range(0, size[1], TILE[1]):
            for tx in range(0, size[0], TILE[0]):
                for bz in range(tz, min(tz + TILE[2], size[2])):
                    for by in range(ty, min(ty + TILE[1], size[1])):
                        for bx in range(tx, min(tx + TILE[0], size[0])):
                            v = (bx + lo[0], by + lo[1], bz + lo[2])
                            if not (weights[v[2], v[1], v[0]] > 0) or tsdf[v[2], v[1], v[0]] > 0:
                                continue
                            any_free, all_seen, g = False, True, []
                            for e in steps:
                                pair = []
                                for sgn in (1, -1):
                                    n = (v[0] + sgn * e[0], v[1] + sgn * e[1], v[2] + sgn * e[2])
                                    if not (0 <= n[0] < nx and 0 <= n[1] < ny and 0 <= n[2] < nz):
                                        all_seen = False
                                        continue
                                    w, t = weights[n[2], n[1], n[0]], tsdf[n[2], n[1], n[0]]
                                    if w > 0 and t > 0:
                                        any_free = True
                                    if not (w > 0):
                                        all_seen = False
                                    pair.append(t)
                                if len(pair) == 2:
                                    with np.errstate(invalid="ignore", over="ignore"):
                                        g.append(f32(pair[0]) - f32(pair[1]))
                            if not any_free:
                                continue
                            n_surface += 1
                            if not all_seen or not all(np.isfinite(c) for c in g) or all(c == 0 for c in g):
                                continue
                            out.append(((bz * size[1] + by) * size[0] + bx, g))
    rec = np.zeros(len(out), VOXEL)
    for k, (i, g) in enumerate(out):
        rec[k] = (i, g)
    return rec, (n_surface, len(out))


def counters(counts, capacity):
    return np.array([counts[0], counts[1], min(counts[1], capacity), 0], np.uint32)


# ---- direction votes ---------------------------------------------------------------------------------------------

def direction_bins(rec, K):
    g = rec["g"]
    a = np.abs(g)
    ok = np.isfinite(g).all(-1) & (a.max(-1) > 0) if len(g) else np.zeros(0, bool)
    g, a = g[ok], a[ok]
    m = np.argmax(a, -1)  # the first largest
    i = np.arange(len(g))
    am, gm = a[i, m], g[i, m]
    half = f32(K) / f32(2)
    with np.errstate(all="ignore"):
        u, v = g[i, (m + 1) % 3] / am, g[i, (m + 2) % 3] / am
        iu = np.minimum(np.floor((u + f32(1)) * half).astype(np.int64), K - 1)
        iv = np.minimum(np.floor((v + f32(1)) * half).astype(np.int64), K - 1)
    face = 2 * m + (gm < 0)
    return np.bincount((face * K + iv) * K + iu, minlength=6 * K * K).astype(np.uint32).reshape(6, K, K)


def direction_bins_loop(rec, K):
    bins = np.zeros(6 * K * K, np.uint32)
    half = f32(K) / f32(2)
    for r in rec:
        g = [f32(c) for c in r["g"]]
        if not all(np.isfinite(c) for c in g):
            continue
        m, am = 0, abs(g[0])
        for j in (1, 2):
            if abs(g[j]) > am:
                m, am = j, abs(g[j])
        if not am > 0:
            continue
        cells = []
        for j in (1, 2):
            u = g[(m + j) % 3] / am
            cells.append(min(int(math.floor((u + f32(1)) * half)), K - 1))
        bins[((2 * m + (1 if g[m] < 0 else 0)) * K + cells[1]) * K + cells[0]] += 1
    return bins.reshape(6, K, K)


# ---- offset votes and assignment ---------------------------------------------------------------------------------

def voxel_of(index, size):
    index = np.asarray(index).astype(np.int64)
    row = index // size[0]
    return index - row * size[0], row % size[1], row // size[1]


def _dot(n, a, b, c):
    return (n[0] * a + n[1] * b) + n[2] * c


def _aligned(n, g, cos2):
    with np.errstate(all="ignore"):
        a = _dot(n, g[:, 0], g[:, 1], g[:, 2])
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        return (a > 0) & (a * a >= f32(cos2) * gg)


def offset_hist(rec, size, dirs, shift, cos2, inv_bin, S):
    dirs, shift = np.asarray(dirs, f32).reshape(-1, 3), np.asarray(shift, f32).reshape(-1)
    x, y, z = (c.astype(f32) for c in voxel_of(rec["index"], size))
    hist = np.zeros((len(dirs), S), np.uint32)
    for k, n in enumerate(dirs):
        with np.errstate(all="ignore"):
            s = np.floor(_dot(n, x, y, z) * f32(inv_bin) + shift[k])
            vote = _aligned(n, rec["g"], cos2) & (s >= 0) & (s < f32(S))
        hist[k] = np.bincount(s[vote].astype(np.int64), minlength=S)
    return hist


def offset_hist_loop(rec, size, dirs, shift, cos2, inv_bin, S):
    dirs, shift = np.asarray(dirs, f32).reshape(-1, 3), np.asarray(shift, f32).reshape(-1)
    hist = np.zeros((len(dirs), S), np.uint32)
    with np.errstate(all="ignore"):
        for r in rec:
            g = [f32(c) for c in r["g"]]
            x, y, z = (f32(int(c)) for c in voxel_of(r["index"], size))
            gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
            for k, n in enumerate(dirs):
                a = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2]
                if not (a > 0 and a * a >= f32(cos2) * gg):
                    continue
                s = np.floor(((n[0] * x + n[1] * y) + n[2] * z) * f32(inv_bin) + shift[k])
                if s >= 0 and s < f32(S):
                    hist[k, int(s)] += 1
    return hist


def moments_of(labels, rec, size, P):
    x, y, z = voxel_of(rec["index"], size)
    mom = np.zeros(P, MOMENTS)
    mom["lo"], mom["hi"] = size, -1
    for k in range(P):
        sel = labels == k
        if not sel.any():
            continue
        c = [x[sel].astype(np.uint64), y[sel].astype(np.uint64), z[sel].astype(np.uint64)]
        mom[k]["count"] = sel.sum()
        mom[k]["sum"] = [v.sum() for v in c]
        mom[k]["sum2"] = [(c[0] * c[0]).sum(), (c[1] * c[1]).sum(), (c[2] * c[2]).sum(), (c[0] * c[1]).sum(),
                          (c[0] * c[2]).sum(), (c[1] * c[2]).sum()]
        mom[k]["lo"] = [int(v.min()) for v in c]
        mom[k]["hi"] = [int(v.max()) for v in c]
    return mom


def assign(rec, size, planes, cos2, band):
    """(labels i16, moments) of the records for planes = P x (n0, n1, n2, d)."""
    planes = np.asarray(planes, f32).reshape(-1, 4)
    x, y, z = (c.astype(f32) for c in voxel_of(rec["index"], size))
    labels = np.full(len(rec), -1, np.int16)
    best = np.full(len(rec), np.inf, f32)
    for k, p in enumerate(planes):
        with np.errstate(all="ignore"):
            e = np.abs(_dot(p[:3], x, y, z) - p[3])
            take = _aligned(p[:3], rec["g"], cos2) & (e <= f32(band)) & ((labels < 0) | (e < best))
        labels[take], best[take] = k, e[take]
    return labels, moments_of(labels, rec, size, len(planes))


def assign_loop(rec, size, planes, cos2, band):
    planes = np.asarray(planes, f32).reshape(-1, 4)
    labels = np.full(len(rec), -1, np.int16)
    mom = np.zeros(len(planes), MOMENTS)
    mom["lo"], mom["hi"] = size, -1
    with np.errstate(all="ignore"):
        for i, r in enumerate(rec):
            g = [f32(c) for c in r["g"]]
            v = [int(c) for c in voxel_of(r["index"], size)]
            x, y, z = (f32(c) for c in v)
            gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
            label, best = -1, None
            for k, p in enumerate(planes):
                a = (p[0] * g[0] + p[1] * g[1]) + p[2] * g[2]
                if not (a > 0 and a * a >= f32(cos2) * gg):
                    continue
                e = abs(((p[0] * x + p[1] * y) + p[2] * z) - p[3])
                if e <= f32(band) and (label < 0 or e < best):
                    label, best = k, e
            labels[i] = label
            if label < 0:
                continue
            m = mom[label]
            m["count"] += 1
            for j in range(3):
                m["sum"][j] += v[j]
                m["lo"][j], m["hi"][j] = min(m["lo"][j], v[j]), max(m["hi"][j], v[j])
            for j, (p, q) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
                m["sum2"][j] += v[p] * v[q]
    return labels, mom


RECURRING = [0, 1, 0, 0, 1, 1, 0, -1]


def recurring_labels():
    """(records, size, planes, cos2, band): 64 records, one wave of the assign kernel, whose labels are RECURRING eight
    times over.  A label that comes back after another one is a run of its own: its sums must not cross the gap."""
    size = (16, 16, 16)
    rec = np.zeros(64, VOXEL)
    for i in range(64):
        z = {0: 3, 1: 11, -1: 7}[RECURRING[i % 8]]
        rec[i] = ((z * size[1] + (7 * i) % 16) * size[0] + i % 16, (0.0, 0.0, 1.0))
    return rec, size, np.array([(0, 0, 1, 3), (0, 0, 1, 11)], f32), f32(0.25), 0.5


# ---- the host steps between the stages, Python floats ---------------------------------------------------------------

def cell_centre(b, K):
    """The unit vector through the centre of bin b of the cube map."""
    face, iv, iu = b // (K * K), (b // K) % K, b % K
    m = face // 2
    c = [0.0, 0.0, 0.0]
    c[m] = -1.0 if face % 2 else 1.0
    c[(m + 1) % 3] = (iu + 0.5) / (K / 2.0) - 1.0
    c[(m + 2) % 3] = (iv + 0.5) / (K / 2.0) - 1.0
    norm = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    return [c[0] / norm, c[1] / norm, c[2] / norm]


def directions(bins, K, min_votes, separation_deg):
    """Greedy: bins by count descending, ties to the lower bin; a bin of at least min_votes becomes a direction unless
    its dot with a chosen one exceeds cos(separation).  [(bin, votes, n)], at most MAX_DIRS."""
    flat = [int(v) for v in np.asarray(bins).reshape(-1)]
    limit = math.cos(separation_deg * math.pi / 180.0)
    chosen = []
    for b in sorted(range(len(flat)), key=lambda b: (-flat[b], b)):
        if flat[b] < min_votes or len(chosen) == MAX_DIRS:
            break
        n = cell_centre(b, K)
        if any((n[0] * c[2][0] + n[1] * c[2][1]) + n[2] * c[2][2] > limit for c in chosen):
            continue
        chosen.append((b, flat[b], n))
    return chosen


def offset_frame(n, size, bin_vox):
    """(lo, S, inv_bin, shift) of a direction: lo the minimum of n . corner over the eight corners of the box's voxel
    cubes, S = floor((hi - lo) / bin) + 1 slots, slot = floor(n . b * inv_bin + shift)."""
    lo, hi = math.inf, -math.inf
    for k in range(8):
        b = [(size[j] - 0.5) if (k >> j) & 1 else -0.5 for j in range(3)]
        s = (n[0] * b[0] + n[1] * b[1]) + n[2] * b[2]
        lo, hi = min(lo, s), max(hi, s)
    S = int(math.floor((hi - lo) / bin_vox)) + 1
    inv_bin = 1.0 / bin_vox
    return lo, S, inv_bin, -lo * inv_bin


def offset_peaks(row, min_votes, peak_gap):
    """Greedy over the slots of one direction: [(slot, votes)], no two within peak_gap slots of each other."""
    row = [int(v) for v in row]
    chosen = []
    for s in sorted(range(len(row)), key=lambda s: (-row[s], s)):
        if row[s] < min_votes:
            break
        if all(abs(s - c[0]) > peak_gap for c in chosen):
            chosen.append((s, row[s]))
    return chosen


def seeds(dirs, hists, frames, bin_vox, min_votes, peak_gap):
    """The seed planes [(votes, direction, slot, n, d)] ordered by votes, ties by (direction, slot), at most MAX_PLANES."""
    out = []
    for k, (d, row, fr) in enumerate(zip(dirs, hists, frames)):
        for slot, votes in offset_peaks(row, min_votes, peak_gap):
            out.append((votes, k, slot, d[2], fr[0] + (slot + 0.5) * bin_vox))
    out.sort(key=lambda p: (-p[0], p[1], p[2]))
    return out[:MAX_PLANES]


def fit(mom, seed_n, seed_d):
    """dict(n, d, centroid, thickness, axes, eigenvalues) of a plane from its integer moments; fewer than 3 members
    keep the seed.  Centroid, covariance and Jacobi frame are those of the object shapes."""
    if int(mom["count"]) < 3:
        return dict(n=list(seed_n), d=seed_d, centroid=None, thickness=0.0, axes=None, eigenvalues=None, fitted=False)
    m = np.zeros((), sr.MOMENTS)
    m["solid"], m["sum"], m["sum2"] = mom["count"], mom["sum"], mom["sum2"]
    fr = sr.frame(m)
    axes = [[float(v) for v in fr["axes"][3 * k:3 * k + 3]] for k in range(3)]
    c = [float(v) for v in fr["centroid"]]
    n = axes[2]
    if (n[0] * seed_n[0] + n[1] * seed_n[1]) + n[2] * seed_n[2] < 0:
        n = [-n[0], -n[1], -n[2]]
    eig = [float(v) for v in fr["eigenvalues"]]
    return dict(n=n, d=(n[0] * c[0] + n[1] * c[1]) + n[2] * c[2], centroid=c, thickness=math.sqrt(max(eig[2], 0.0)),
                axes=axes[:2], eigenvalues=eig, fitted=True)


def find_planes(tsdf, weights, box=None, K=15, angle=20.0, separation=None, bin_vox=1.0, band=2.0, min_votes=50,
                peak_gap=2, refine=1, max_planes=MAX_PLANES, stages=None):
    """The whole finder on the restatement's own stages (or on `stages`, an object with the same four functions, e.g.
    the device): the list of fitted planes ordered by count, with labels and records."""
    st = stages or _Host
    lo, size = _box(tsdf, box)
    c = math.cos(angle * math.pi / 180.0)
    cos2 = c * c
    rec = st.records(tsdf, weights, box)
    if min_votes is None:  # the session's policy
        min_votes = max(50, len(rec) // 200)
    dirs = directions(st.direction_bins(rec, K), K, min_votes, angle if separation is None else separation)
    if not dirs:
        return [], rec, np.full(len(rec), -1, np.int16)
    frames = [offset_frame(d[2], size, bin_vox) for d in dirs]
    S = max(f[1] for f in frames)
    if S > MAX_SLOTS:
        raise ValueError("more than %d offset slots: a wider bin is needed" % MAX_SLOTS)
    hist = st.offset_hist(rec, size, [d[2] for d in dirs], [f[3] for f in frames], cos2, frames[0][2], S)
    planes = [(p[3], p[4]) for p in seeds(dirs, [hist[k][:f[1]] for k, f in enumerate(frames)], frames, bin_vox, min_votes,
                                          peak_gap)[:max_planes]]
    if not planes:
        return [], rec, np.full(len(rec), -1, np.int16)
    fits = None
    for _ in range(refine + 1):
        labels, mom = st.assign(rec, size, [list(n) + [d] for n, d in planes], cos2, band)
        fits = [fit(mom[k], *planes[k]) for k in range(len(planes))]
        planes = [(f["n"], f["d"]) for f in fits]
    for k, f in enumerate(fits):
        f.update(count=int(mom[k]["count"]), lo=[int(v) for v in mom[k]["lo"]], hi=[int(v) for v in mom[k]["hi"]], label=k)
    order = sorted(range(len(fits)), key=lambda k: (-fits[k]["count"], k))
    return [fits[k] for k in order if fits[k]["count"] > 0], rec, labels


class _Host:
    records = staticmethod(lambda tsdf, weights, box: records(tsdf, weights, box)[0])
    direction_bins = staticmethod(direction_bins)
    offset_hist = staticmethod(offset_hist)
    assign = staticmethod(assign)


def kinds(normals, heights, up, floor_angle=30.0, kind_angle=10.0):
    """(floor index or None, [kind]) of planes with world unit normals and centroid heights along `up`: the floor is,
    among the planes within floor_angle of up, the lowest one, ties to the lowest index; the others are named relative
    to the floor's normal (to up without a floor): level, ceiling, wall, slope."""
    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    norm = math.sqrt(dot(up, up))
    up = [up[0] / norm, up[1] / norm, up[2] / norm]
    cos_floor = math.cos(floor_angle * math.pi / 180.0)
    cos_kind, sin_kind = math.cos(kind_angle * math.pi / 180.0), math.sin(kind_angle * math.pi / 180.0)
    floor = None
    for k, n in enumerate(normals):
        if dot(n, up) >= cos_floor and (floor is None or heights[k] < heights[floor]):
            floor = k
    ref = up if floor is None else normals[floor]
    out = []
    for k, n in enumerate(normals):
        c = dot(n, ref)
        if k == floor:
            out.append("floor")
        elif c >= cos_kind:
            out.append("level")
        elif c <= -cos_kind:
            out.append("ceiling")
        elif abs(c) <= sin_kind:
            out.append("wall")
        else:
            out.append("slope")
    return floor, out


# ---- fixtures ------------------------------------------------------------------------------------------------------

def plane_volume(shape, planes, spheres=(), trunc=3.0, noise=0.0, seed=0):
    """(tsdf, weights) of shape (nx, ny, nz): free space is the intersection of the half-spaces n . p > d of `planes`
    ((n, d), n any length) minus the balls `spheres` ((centre, radius)); tsdf = clip(sd / trunc, -1, 1) (+ Gaussian
    noise), weights 1 down to `trunc` voxels behind the surface and 0 deeper: the interior is unobserved."""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    sd = np.full((nz, ny, nx), np.inf)
    for n, d in planes:
        n = np.asarray(n, np.float64) / np.linalg.norm(n)
        sd = np.minimum(sd, n[0] * x + n[1] * y + n[2] * z - d)
    for c, r in spheres:
        sd = np.minimum(sd, np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r)
    tsdf = np.clip(sd / trunc, -1.0, 1.0)
    if noise:
        tsdf = tsdf + np.random.default_rng(seed).normal(0.0, noise, tsdf.shape)
    return tsdf.astype(f32), (sd > -trunc).astype(f32)


ROOM_PLANES = [((0.0, 1.0, 0.0), 6.0), ((0.05, -0.1, -1.0), -40.0), ((1.0, 0.2, 0.1), 8.0)]  # (n, d), n unnormalised
ROOM_SPHERE = ((28.0, 26.0, 20.0), 6.0)


def room(noise=0.0):
    """The analytic 48^3 room: three planes and a sphere of radius 6, interior unobserved."""
    return plane_volume((48, 48, 48), ROOM_PLANES, [ROOM_SPHERE], noise=noise, seed=7)


def random_volume(shape, seed, specials=True):
    """Random tsdf with random weights that include 0, negative values and NaN; with specials also NaN, -0.0 and
    infinities in the tsdf."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(-1, 1, (nz, ny, nx)).astype(f32)
    weights = rng.choice(np.array([0.0, -1.0, np.nan, 1.0, 2.0, 5.0], f32), (nz, ny, nx), p=[0.1, 0.03, 0.02, 0.5, 0.25, 0.1])
    if specials:
        pick = rng.uniform(size=tsdf.shape)
        tsdf[pick < 0.02] = np.nan
        tsdf[(pick >= 0.02) & (pick < 0.05)] = -0.0
        tsdf[(pick >= 0.05) & (pick < 0.06)] = np.inf
        tsdf[(pick >= 0.06) & (pick < 0.07)] = -np.inf
    return tsdf, weights.astype(f32)


def volume(shape, content, seed=0):
    """(tsdf, weights) of shape (nx, ny, nz) by name."""
    nx, ny, nz = shape
    mid = [(v - 1) / 2.0 for v in shape]
    if content == "tilted":
        n = (0.3, 1.0, -0.45)
        return plane_volume(shape, [(n, float(np.dot(np.asarray(n) / np.linalg.norm(n), mid)))], trunc=2.0)
    if content == "axis":
        return plane_volume(shape, [((0.0, 0.0, 1.0), mid[2] - 0.25), ((1.0, 0.0, 0.0), min(2.5, mid[0]))], trunc=2.0)
    if content == "random":
        return random_volume(shape, seed + nx * 7 + ny * 3 + nz)
    if content == "infinite":
        tsdf, weights = random_volume(shape, seed + 99, specials=False)
        tsdf[::2, ::3, ::2] = np.inf
        return tsdf, np.ones_like(weights)
    if content == "zero_gradient":  # solid slabs one voxel thick between equal free values: every difference is 0
        tsdf = np.full((nz, ny, nx), 0.5, f32)
        tsdf[:, :, 1::4] = -0.0
        return tsdf, np.ones((nz, ny, nx), f32)
    if content == "unseen":
        return random_volume(shape, seed + 5, specials=False)[0], np.zeros((nz, ny, nx), f32)
    raise ValueError(content)
