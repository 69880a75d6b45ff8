"""Merging a volume restated (include/emf_hip.h "Merging a volume"): the device stage twice -- vectorised
numpy in float32, one operation per line, and a plain loop per voxel.  The geometry (tsdf, weights, the emf_absorb_t
record) is the absorption's, called as tests/absorb_reference.py states it; the FUSED voxels and the source voxel nearest
to each sample are those of tests/transfer_color_reference.py (values_of / _value_loop, built on the same sample-point,
outside and blend helpers), and the colour of a coloured merge is its absorb_color.  What is stated here is what a merge
adds: the (fg, bg) count pair of every FUSED voxel and the emf_merge_counts_t record.  No GPU, no library: the tests
compare emf_hip_mergeVolume and emf_hip_mergeVolumeColor with these, as bytes.  At the end the host steps of
Fusion.merge_objects: the union of the two bands in numpy and in Python floats, the resize arithmetic, the shift and
the foreground mask from the counts.

A count volume is a (nz, ny, nx, 2) float32 array, (fg, bg) interleaved: the layout of emf_hip_updateFgBgProbs.  A
destination is ar.dst_vol(...) with fgbg=; a source ar.src_vol(...) with fgbg= and a mask (fg=): a merge refuses a
source without one."""
from __future__ import annotations

import numpy as np

from tests import absorb_reference as ar
from tests import transfer_color_reference as tc

f32 = np.float32

MERGE_COUNTS = np.dtype([("foreground", "<u8"), ("gained", "<u8")])
assert MERGE_COUNTS.itemsize == 16

# the kinds of count pair a sweep has to reach (test_merge_reference_cpu.py checks that it does)
KINDS = ("fresh", "summed", "rounded_sum", "gained_fresh", "gained_summed", "stays_foreground", "stays_background", "equal_pair",
         "zero_pair")


def counts(foreground=0, gained=0):
    out = np.zeros((), MERGE_COUNTS)
    out["foreground"], out["gained"] = foreground, gained
    return out


# ---- the device stage, vectorised ----------------------------------------------------------------------------------

def merge(dst, src, pose, box=None, kinds=None):
    """(tsdf, weights, record, fgbg, counts) of the destination after emf_hip_mergeVolume over box = (lo, size), both
    (x, y, z).  kinds: a dict that collects how many voxels of each of KINDS the call met."""
    assert src["fg"] is not None, "a merge refuses a source without a mask"
    td, wd, rec = ar.absorb(dst, src, pose, box)
    fgbg = dst["fgbg"].copy()
    x, y, z, rx, ry, rz = tc.values_of(dst, src, pose, box, seed=False)
    assert len(x) == rec["fused"], (len(x), rec)
    S = src["fgbg"][rz, ry, rx]
    D = fgbg[z, y, x]
    sf, sb, df, db = S[:, 0], S[:, 1], D[:, 0], D[:, 1]
    with np.errstate(all="ignore"):
        fresh = ~(dst["weights"][z, y, x] > 0)
        af = df + sf
        ab = db + sb
        nf = np.where(fresh, sf, af)
        nb = np.where(fresh, sb, ab)
        foreground = nf > nb
        gained = foreground & (fresh | ~(df > db))
    fgbg[z, y, x, 0], fgbg[z, y, x, 1] = nf, nb
    if kinds is not None:
        exact = (df.astype(np.float64) + sf.astype(np.float64) == af) & (db.astype(np.float64) + sb.astype(np.float64) == ab)
        found = dict(fresh=fresh, summed=~fresh, rounded_sum=~fresh & ~exact, gained_fresh=gained & fresh, gained_summed=gained & ~fresh,
                     stays_foreground=foreground & ~gained, stays_background=~fresh & ~foreground & ~(df > db), equal_pair=nf == nb,
                     zero_pair=(sf == 0) & (sb == 0))
        for name in KINDS:
            kinds[name] = kinds.get(name, 0) + int(found[name].sum())
    return td, wd, rec, fgbg, counts(int(foreground.sum()), int(gained.sum()))


def merge_color(dst, src, pose, box=None):
    """(tsdf, weights, record, fgbg, counts, color, colour record) after emf_hip_mergeVolumeColor: the colour of the
    absorption, unchanged."""
    td, wd, rec, fgbg, cnt = merge(dst, src, pose, box)
    ct, cw, crec, color, moved = tc.absorb_color(dst, src, pose, box)
    assert ct.tobytes() == td.tobytes() and cw.tobytes() == wd.tobytes() and crec.tobytes() == rec.tobytes()
    return td, wd, rec, fgbg, cnt, color, moved


# ---- the device stage, voxel by voxel --------------------------------------------------------------------------------

def merge_loop(dst, src, pose, box=None):
    """The same by a plain loop over the box; every float step an np.float32 scalar operation."""
    assert src["fg"] is not None
    td, wd, rec = ar.absorb_loop(dst, src, pose, box)
    fgbg = dst["fgbg"].copy()
    nz, ny, nx = dst["tsdf"].shape
    nd, ns = (nx, ny, nz), src["tsdf"].shape[::-1]
    Rm, tm = ar.pose_of(*pose)
    R, t = [f32(v) for v in Rm], [f32(v) for v in tm]
    voxd, voxs = f32(dst["voxel_size"]), f32(src["voxel_size"])
    ratio = ar.ratio_of(src, dst)
    lo, size = ar.whole(dst) if box is None else box
    n_fg = n_gained = n_fused = 0
    with np.errstate(all="ignore"):
        for z in range(lo[2], lo[2] + max(size[2], 0)):
            for y in range(lo[1], lo[1] + max(size[1], 0)):
                for x in range(lo[0], lo[0] + max(size[0], 0)):
                    v = (x, y, z)
                    near = tc._value_loop(v, dst, src, nd, ns, voxd, voxs, R, t, ratio, False)
                    if near is None:
                        continue
                    n_fused += 1
                    sf, sb = (f32(c) for c in ar.at(src["fgbg"], near))
                    df, db = (f32(c) for c in fgbg[z, y, x])  # read once, before either is written
                    if not f32(ar.at(dst["weights"], v)) > 0:
                        nf, nb, fresh = sf, sb, True
                    else:
                        nf, nb, fresh = df + sf, db + sb, False
                    if nf > nb:
                        n_fg += 1
                        if fresh or not df > db:
                            n_gained += 1
                    fgbg[z, y, x] = (nf, nb)
    assert n_fused == rec["fused"]
    return td, wd, rec, fgbg, counts(n_fg, n_gained)


def check_identities(rec, cnt):
    """visited = outside + unknown + masked + saturated + fused (ar.check_identities) and gained <= foreground <= fused."""
    ar.check_identities(rec)
    assert int(cnt["gained"]) <= int(cnt["foreground"]) <= int(rec["fused"]), (cnt, rec)


# ---- count volumes and the sweep -------------------------------------------------------------------------------------

BIG = 2.0 ** 24  # the first float32 whose successor is 2 away: BIG + an odd count rounds


def count_volume(shape, seed):
    """A (nz, ny, nx, 2) f32 count volume for shape = (nx, ny, nz), integer-valued: about an eighth each of (0, 0), fg == bg,
    fg one above bg, fg one below bg and (2^24, 2^24 - 1) -- a pair whose sum with an odd count is no float32 -- the rest
    random pairs below 9."""
    nx, ny, nz = shape
    rng = np.random.default_rng([0xF6, seed, nx, ny, nz])
    c = rng.integers(0, 9, (nz, ny, nx, 2)).astype(f32)
    kind = rng.integers(0, 8, (nz, ny, nx))
    c[kind == 0] = 0
    c[..., 1][kind == 1] = c[..., 0][kind == 1]
    c[..., 0][kind == 2] = c[..., 1][kind == 2] + 1
    c[..., 1][kind == 3] = c[..., 0][kind == 3] + 1
    c[kind == 4] = (BIG, BIG - 1)
    return c


def with_counts(k, dst, src):
    """Case k of a sweep with count volumes attached.  A source without a mask gets the one its own counts give,
    fg > bg -- what a session derives an object's mask from."""
    dst = dict(dst, fgbg=count_volume(dst["tsdf"].shape[::-1], 1 + k % 2))
    src = dict(src, fgbg=count_volume(src["tsdf"].shape[::-1], 3 + k % 3))
    if src["fg"] is None:
        src["fg"] = np.ascontiguousarray(src["fgbg"][..., 0] > src["fgbg"][..., 1], np.uint8)
    return dst, src


def cases(dshape, content, boxes=ar.BOXES):
    """absorb_reference.cases with count volumes (and a mask on every source): (name, dst, src, pose, box)."""
    for k, (name, dst, src, pose, box) in enumerate(ar.cases(dshape, content, boxes)):
        dst, src = with_counts(k, dst, src)
        yield name, dst, src, pose, box


def color_cases(dshape, content, boxes=ar.BOXES):
    """transfer_color_reference.absorb_cases with count volumes."""
    for k, (name, dst, src, pose, box) in enumerate(tc.absorb_cases(dshape, content, boxes)):
        dst, src = with_counts(k, dst, src)
        yield name, dst, src, pose, box


def planted_case():
    """absorb_reference.planted_case with count volumes and the mask of the source's counts: (dst, src, poses)."""
    dst, src, poses = ar.planted_case()
    dst, src = with_counts(0, dst, src)
    return dst, src, poses


# ---- the host stage of a session's merge: the growth, float64 in a fixed order, rounded once --------------------------
# A bound v on axis j of a volume of N voxels is c_j = (v_j - (N_j - 1) / 2) * voxelSize; the source's eight corners go
# through (R, t) = the destination's volume frame <- the source's as x_i = ((R_i0 c_0 + R_i1 c_1) + R_i2 c_2) + t_i; the
# union with the destination's own two bounds is rounded to float32 once.  hi[0] < 0: no solid voxel, nothing to add.

def union_np(d_bounds, d_res, d_voxel, s_bounds, s_res, s_voxel, R, t):
    """(lo, hi) float32, or None where neither object has a solid voxel; numpy float64, one operation per line."""
    has_d, has_s = d_bounds[1][0] >= 0, s_bounds[1][0] >= 0
    if not has_d and not has_s:
        return None
    R, t = np.asarray(R, f32).reshape(3, 3).astype(np.float64), np.asarray(t, f32).reshape(3).astype(np.float64)

    def coord(v, n, voxel):
        half = (np.asarray(n, np.float64) - 1.0) / 2.0
        off = np.asarray(v, np.float64) - half
        return off * np.float64(f32(voxel))
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    if has_d:
        lo, hi = coord(d_bounds[0], d_res, d_voxel), coord(d_bounds[1], d_res, d_voxel)
    if has_s:
        c = np.stack([coord(s_bounds[0], s_res, s_voxel), coord(s_bounds[1], s_res, s_voxel)])
        for k in range(8):
            p = np.array([c[k & 1, 0], c[(k >> 1) & 1, 1], c[(k >> 2) & 1, 2]])
            x = R[:, 0] * p[0]
            x = x + R[:, 1] * p[1]
            x = x + R[:, 2] * p[2]
            x = x + t
            lo, hi = np.minimum(lo, x), np.maximum(hi, x)
    return lo.astype(f32), hi.astype(f32)


def union_py(d_bounds, d_res, d_voxel, s_bounds, s_res, s_voxel, R, t):
    """The same in plain Python floats."""
    from tests.contacts_reference import to_f32
    has_d, has_s = int(d_bounds[1][0]) >= 0, int(s_bounds[1][0]) >= 0
    if not has_d and not has_s:
        return None
    R, t = [float(v) for v in np.asarray(R, f32).reshape(9)], [float(v) for v in np.asarray(t, f32).reshape(3)]

    def coord(v, n, voxel):
        return (float(int(v)) - (float(int(n)) - 1.0) / 2.0) * float(f32(voxel))
    lo = [coord(d_bounds[0][j], d_res[j], d_voxel) if has_d else float("inf") for j in range(3)]
    hi = [coord(d_bounds[1][j], d_res[j], d_voxel) if has_d else float("-inf") for j in range(3)]
    if has_s:
        c = [[coord(s_bounds[b][j], s_res[j], s_voxel) for j in range(3)] for b in (0, 1)]
        for k in range(8):
            p = [c[k & 1][0], c[(k >> 1) & 1][1], c[(k >> 2) & 1][2]]
            for i in range(3):
                x = R[3 * i] * p[0]
                x = x + R[3 * i + 1] * p[1]
                x = x + R[3 * i + 2] * p[2]
                x = x + t[i]
                lo[i], hi[i] = min(lo[i], x), max(hi[i], x)
    return np.array([to_f32(v) for v in lo], f32), np.array([to_f32(v) for v in hi], f32)


def grow(res, voxel, lo, hi, vol_pad=2.0, max_res=256):
    """What the destination's resize makes of the union (lo, hi): (n, offset, centre) -- the new cubic resolution, the
    voxel offset of the old content (new(v) = old(v + offset), 0 outside) and the shift of the volume's centre in metres
    of the old volume frame -- or None where the box is contained or n would pass max_res: the volume stays.  Float32
    steps, as ObjTSDF::resize takes them."""
    res, voxel, lo, hi = np.asarray(res), f32(voxel), np.asarray(lo, f32), np.asarray(hi, f32)
    half = (res.astype(f32) - f32(1)) * f32(0.5) * voxel
    if not ((lo < -half) | (hi > half)).any():
        return None
    size = f32(vol_pad) * (hi - lo).max() / voxel
    n = (int(np.ceil(size)) + 1) // 2 * 2
    if n < 2 or n > max_res:
        return None
    centre = (lo + hi) / f32(2)
    pix = np.rint(centre / voxel).astype(np.int64)
    offset = pix - np.array([int((n - r) / 2) for r in res])  # C++ integer division: towards zero
    return n, tuple(int(v) for v in offset), pix.astype(f32) * voxel


def shifted(volume, n, offset):
    """A (nz, ny, nx[, c]) volume moved into a cube of n voxels: new(v) = old(v + offset), 0 outside (emf_hip_copyValues)."""
    out = np.zeros((n, n, n) + volume.shape[3:], volume.dtype)
    nz, ny, nx = volume.shape[:3]
    ox, oy, oz = offset
    x0, x1 = max(0, -ox), min(n, nx - ox)
    y0, y1 = max(0, -oy), min(n, ny - oy)
    z0, z1 = max(0, -oz), min(n, nz - oz)
    if x0 < x1 and y0 < y1 and z0 < z1:
        out[z0:z1, y0:y1, x0:x1] = volume[z0 + oz:z1 + oz, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def fg_mask_of(fgbg):
    """An object's foreground mask from its counts: fg / (fg + bg) > 0.5 as 255 (ObjTSDF::computeFgProbs)."""
    with np.errstate(all="ignore"):
        p = fgbg[..., 0] / (fgbg[..., 0] + fgbg[..., 1])
        return np.where(p > f32(0.5), 255, 0).astype(np.uint8)


# ---- the host stage of the automatic merge: the quotient, the pairs, the sums -----------------------------------------
# records: {(a, b): (surface, touching)} of the contact probe over all ordered object pairs.  overlap(a -> b) = touching /
# surface as a float64 quotient, 0 for an empty surface.  An unordered pair a < b qualifies when max(overlap(a -> b),
# overlap(b -> a)) >= min_overlap and both surfaces hold at least min_surface voxels; qualifying pairs go in descending
# maximum, ties to the smaller pair of ids; an object takes part once; the smaller id is the destination.

def overlap_np(surface, touching):
    surface, touching = np.asarray(surface, np.uint64), np.asarray(touching, np.uint64)
    with np.errstate(all="ignore"):
        return np.where(surface > 0, touching.astype(np.float64) / surface.astype(np.float64), 0.0)


def overlap_py(surface, touching):
    return float(int(touching)) / float(int(surface)) if int(surface) else 0.0


def merge_pairs_np(records, min_overlap=0.5, min_surface=64):
    """[(dst, src, overlap(dst -> src), overlap(src -> dst))] in the order the merges run; numpy, a lexicographic sort."""
    keys = sorted({(min(a, b), max(a, b)) for a, b in records})
    if not keys:
        return []
    ab = np.array([records.get((a, b), (0, 0)) for a, b in keys], np.uint64).reshape(-1, 2)
    ba = np.array([records.get((b, a), (0, 0)) for a, b in keys], np.uint64).reshape(-1, 2)
    has = np.array([(a, b) in records and (b, a) in records for a, b in keys])
    o_ab, o_ba = overlap_np(ab[:, 0], ab[:, 1]), overlap_np(ba[:, 0], ba[:, 1])
    best = np.maximum(o_ab, o_ba)
    ok = has & (best >= min_overlap) & (np.minimum(ab[:, 0], ba[:, 0]) >= np.uint64(min_surface))
    ids = np.array(keys, np.int64)
    order = np.lexsort((ids[:, 1], ids[:, 0], -best))  # the last key is the primary one
    taken, out = np.zeros(int(ids.max()) + 1, bool), []
    for k in order:
        a, b = ids[k]
        if ok[k] and not taken[a] and not taken[b]:
            taken[a] = taken[b] = True
            out.append((int(a), int(b), float(o_ab[k]), float(o_ba[k])))
    return out


def merge_pairs_py(records, min_overlap=0.5, min_surface=64):
    """The same in plain Python."""
    found = []
    for (a, b), (surface, touching) in records.items():
        if a < b and (b, a) in records:
            back = records[(b, a)]
            o_ab, o_ba = overlap_py(surface, touching), overlap_py(*back)
            if max(o_ab, o_ba) >= min_overlap and min(int(surface), int(back[0])) >= min_surface:
                found.append((-max(o_ab, o_ba), a, b, o_ab, o_ba))
    taken, out = set(), []
    for _, a, b, o_ab, o_ba in sorted(found):
        if a not in taken and b not in taken:
            taken |= {a, b}
            out.append((a, b, o_ab, o_ba))
    return out


def bookkeeping_np(dst, src):
    """(exists, not exists, class scores) of the destination after a merge: the sums of both; scores element-wise, the
    shorter list padded with zeros.  dst, src: (exists, not exists, scores)."""
    n = max(len(dst[2]), len(src[2]))
    scores = np.zeros(n, np.float64)
    scores[:len(dst[2])] += np.asarray(dst[2], np.float64)
    scores[:len(src[2])] += np.asarray(src[2], np.float64)
    return int(dst[0]) + int(src[0]), int(dst[1]) + int(src[1]), scores


def bookkeeping_py(dst, src):
    n = max(len(dst[2]), len(src[2]))
    a, b = list(dst[2]) + [0.0] * (n - len(dst[2])), list(src[2]) + [0.0] * (n - len(src[2]))
    return dst[0] + src[0], dst[1] + src[1], [float(x) + float(y) for x, y in zip(a, b)]
