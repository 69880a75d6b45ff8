"""Lifting a volume restated (include/emf_hip.h "Lifting a volume"): the two device stages, each twice --
vectorised numpy in float32, one operation per line, and a plain loop per voxel.  The sample point, the blend, the volumes,
the poses and the boxes are those of tests/absorb_reference.py; the case sweep is its sweep with the truncation ratios turned.  No GPU, no library: the tests compare
emf_hip_seedVolume and emf_hip_releaseVolume with these, as bytes."""
from __future__ import annotations

import numpy as np

from tests import absorb_reference as ar
from tests.contacts_reference import lerp, sample_points

f32 = np.float32

SEED = np.dtype([("visited", "<u8"), ("kept", "<u8"), ("outside", "<u8"), ("unknown", "<u8"), ("masked", "<u8"), ("saturated", "<u8"),
                 ("seeded", "<u8"), ("solid", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)])
RELEASE = np.dtype([("visited", "<u8"), ("empty", "<u8"), ("free_space", "<u8"), ("outside", "<u8"), ("unclaimed", "<u8"),
                    ("released", "<u8"), ("solid", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)])
assert SEED.itemsize == 88 and RELEASE.itemsize == 80
SEED_COUNTS = ("visited", "kept", "outside", "unknown", "masked", "saturated", "seeded", "solid")
RELEASE_COUNTS = ("visited", "empty", "free_space", "outside", "unclaimed", "released", "solid")


def claim_of(fg, res=None, voxel_size=0.01):
    """A claimant as the statements take it: a (nz, ny, nx) u8 mask, or None with res = (nx, ny, nz): the whole cube."""
    fg = None if fg is None else np.ascontiguousarray(fg, np.uint8)
    return dict(fg=fg, res=tuple(int(v) for v in (fg.shape[::-1] if fg is not None else res)), voxel_size=f32(voxel_size))


def neutral(dtype, res):
    out = np.zeros((), dtype)
    out["lo"], out["hi"] = res, (-1, -1, -1)
    return out


def _box_voxels(lo, size):
    z, y, x = np.meshgrid(*[np.arange(lo[j], lo[j] + size[j]) for j in (2, 1, 0)], indexing="ij")
    return x.reshape(-1), y.reshape(-1), z.reshape(-1)


# ---- the device stages, vectorised ---------------------------------------------------------------------------------

def seed(dst, src, pose, box=None):
    """(tsdf, weights, record) of the destination after the seed over box = (lo, size), both (x, y, z)."""
    td, wd = dst["tsdf"].copy(), dst["weights"].copy()
    tb, wb, fb = src["tsdf"], src["weights"], src["fg"]
    nz, ny, nx = td.shape
    res_d, res_s = (nx, ny, nz), tb.shape[::-1]
    R, t = ar.pose_of(*pose)
    lo, size = ar.whole(dst) if box is None else box
    out = neutral(SEED, res_d)
    if min(size) <= 0:
        return td, wd, out
    x, y, z = _box_voxels(lo, size)
    out["visited"] = len(x)
    ratio, max_weight = ar.ratio_of(src, dst), f32(dst["max_weight"])
    with np.errstate(all="ignore"):
        kept = wd[z, y, x] > 0  # before anything of the source is read
        out["kept"] = int(kept.sum())
        x, y, z = x[~kept], y[~kept], z[~kept]
        q = sample_points((x, y, z), res_d, dst["voxel_size"], R, t, res_s, src["voxel_size"])
        outside = ar.outside_of(q, res_s)
        out["outside"] = int(outside.sum())
        keep = ~outside
        x, y, z = x[keep], y[keep], z[keep]
        q = [c[keep] for c in q]
        l = [c.astype(np.int64) for c in q]
        f = [q[j] - l[j].astype(f32) for j in range(3)]
        g = [f32(1) - c for c in f]
        cw = [wb[l[2] + dz, l[1] + dy, l[0] + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        ct = [tb[l[2] + dz, l[1] + dy, l[0] + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        seen = np.ones(len(x), bool)
        for w in cw:
            seen &= w > 0
        a0, a1 = lerp(g[0], f[0], ct[0], ct[1]), lerp(g[0], f[0], ct[2], ct[3])
        a2, a3 = lerp(g[0], f[0], ct[4], ct[5]), lerp(g[0], f[0], ct[6], ct[7])
        b0, b1 = lerp(g[1], f[1], a0, a1), lerp(g[1], f[1], a2, a3)
        s = lerp(g[2], f[2], b0, b1)
        unknown = ~seen | np.isnan(s)
        masked = np.zeros(len(x), bool)
        if fb is not None:
            r = [np.where(unknown, 0, np.rint(c).astype(np.int64)) for c in q]
            masked = ~unknown & (fb[r[2], r[1], r[0]] == 0)
        u = s * ratio
        saturated = ~unknown & ~masked & (~(np.abs(s) < f32(1)) | ~(np.abs(u) < f32(1)))
        seeded = ~unknown & ~masked & ~saturated
        out["unknown"], out["masked"], out["saturated"] = int(unknown.sum()), int(masked.sum()), int(saturated.sum())
        out["seeded"] = int(seeded.sum())
        if not seeded.any():
            return td, wd, out
        x, y, z, u = x[seeded], y[seeded], z[seeded], u[seeded]
        wo = cw[0][seeded]
        for w in cw[1:]:
            wo = np.minimum(wo, w[seeded])
        out["solid"] = int((~(u > 0)).sum())
        out["lo"] = [int(c.min()) for c in (x, y, z)]
        out["hi"] = [int(c.max()) for c in (x, y, z)]
        td[z, y, x], wd[z, y, x] = u.astype(f32), np.minimum(wo, max_weight).astype(f32)
    return td, wd, out


def release(dst, claim, pose, box=None):
    """(tsdf, weights, record) of the destination after the release over box; claim: claim_of(...)."""
    td, wd = dst["tsdf"].copy(), dst["weights"].copy()
    cb = claim["fg"]
    nz, ny, nx = td.shape
    res_d, res_c = (nx, ny, nz), claim["res"]
    R, t = ar.pose_of(*pose)
    lo, size = ar.whole(dst) if box is None else box
    out = neutral(RELEASE, res_d)
    if min(size) <= 0:
        return td, wd, out
    x, y, z = _box_voxels(lo, size)
    out["visited"] = len(x)
    with np.errstate(all="ignore"):
        pw, pt = wd[z, y, x], td[z, y, x]
        empty = ~(pw > 0)
        free = ~empty & ~(np.abs(pt) < f32(1))
        out["empty"], out["free_space"] = int(empty.sum()), int(free.sum())
        band = ~empty & ~free
        x, y, z, pt = x[band], y[band], z[band], pt[band]
        q = sample_points((x, y, z), res_d, dst["voxel_size"], R, t, res_c, claim["voxel_size"])
        outside = ar.outside_of(q, res_c)
        out["outside"] = int(outside.sum())
        unclaimed = np.zeros(len(x), bool)
        if cb is not None:
            r = [np.where(outside, 0, np.rint(c).astype(np.int64)) for c in q]
            unclaimed = ~outside & (cb[r[2], r[1], r[0]] == 0)
        out["unclaimed"] = int(unclaimed.sum())
        released = ~outside & ~unclaimed
        out["released"] = int(released.sum())
        if not released.any():
            return td, wd, out
        x, y, z, pt = x[released], y[released], z[released], pt[released]
        out["solid"] = int((~(pt > 0)).sum())
        out["lo"] = [int(c.min()) for c in (x, y, z)]
        out["hi"] = [int(c.max()) for c in (x, y, z)]
        td[z, y, x], wd[z, y, x] = f32(0), f32(0)
    return td, wd, out


# ---- the device stages, voxel by voxel -------------------------------------------------------------------------------

def _record(dtype, names, c, blo, bhi):
    out = np.zeros((), dtype)
    for k in names:
        out[k] = c[k]
    out["lo"], out["hi"] = blo, bhi
    return out


def seed_loop(dst, src, pose, box=None):
    """The same by a plain loop over the box; every float step an np.float32 scalar operation."""
    td, wd = dst["tsdf"].copy(), dst["weights"].copy()
    tb, wb, fb = src["tsdf"], src["weights"], src["fg"]
    nz, ny, nx = td.shape
    nd, ns = (nx, ny, nz), tb.shape[::-1]
    Rm, tm = ar.pose_of(*pose)
    R, t = [f32(v) for v in Rm], [f32(v) for v in tm]
    voxd, voxs = f32(dst["voxel_size"]), f32(src["voxel_size"])
    ratio, max_weight = ar.ratio_of(src, dst), f32(dst["max_weight"])
    lo, size = ar.whole(dst) if box is None else box
    c = dict.fromkeys(SEED_COUNTS, 0)
    blo, bhi = list(nd), [-1, -1, -1]
    with np.errstate(all="ignore"):
        for z in range(lo[2], lo[2] + max(size[2], 0)):
            for y in range(lo[1], lo[1] + max(size[1], 0)):
                for x in range(lo[0], lo[0] + max(size[0], 0)):
                    v = (x, y, z)
                    c["visited"] += 1
                    if f32(ar.at(wd, v)) > 0:
                        c["kept"] += 1
                        continue
                    q, outside = ar.sample_loop(v, nd, voxd, R, t, ns, voxs)
                    if outside:
                        c["outside"] += 1
                        continue
                    l = [int(q[j]) for j in range(3)]
                    f = [q[j] - f32(l[j]) for j in range(3)]
                    corners = [(l[0] + dx, l[1] + dy, l[2] + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
                    vals = [f32(ar.at(tb, k)) for k in corners]
                    for j in range(3):  # x pairs, then y, then z
                        vals = [(f32(1) - f[j]) * vals[2 * k] + f[j] * vals[2 * k + 1] for k in range(len(vals) // 2)]
                    s = vals[0]
                    ws = [f32(ar.at(wb, k)) for k in corners]
                    if not all(w > 0 for w in ws) or np.isnan(s):
                        c["unknown"] += 1
                        continue
                    if fb is not None and ar.at(fb, [int(np.rint(q[j])) for j in range(3)]) == 0:
                        c["masked"] += 1
                        continue
                    u = s * ratio
                    if not abs(s) < f32(1) or not abs(u) < f32(1):
                        c["saturated"] += 1
                        continue
                    c["seeded"] += 1
                    c["solid"] += not u > 0
                    for j in range(3):
                        blo[j], bhi[j] = min(blo[j], v[j]), max(bhi[j], v[j])
                    td[z, y, x], wd[z, y, x] = u, min(min(ws), max_weight)
    return td, wd, _record(SEED, SEED_COUNTS, c, blo, bhi)


def release_loop(dst, claim, pose, box=None):
    td, wd = dst["tsdf"].copy(), dst["weights"].copy()
    cb = claim["fg"]
    nz, ny, nx = td.shape
    nd, nc = (nx, ny, nz), claim["res"]
    Rm, tm = ar.pose_of(*pose)
    R, t = [f32(v) for v in Rm], [f32(v) for v in tm]
    voxd, voxc = f32(dst["voxel_size"]), f32(claim["voxel_size"])
    lo, size = ar.whole(dst) if box is None else box
    c = dict.fromkeys(RELEASE_COUNTS, 0)
    blo, bhi = list(nd), [-1, -1, -1]
    with np.errstate(all="ignore"):
        for z in range(lo[2], lo[2] + max(size[2], 0)):
            for y in range(lo[1], lo[1] + max(size[1], 0)):
                for x in range(lo[0], lo[0] + max(size[0], 0)):
                    v = (x, y, z)
                    c["visited"] += 1
                    pw, pt = f32(ar.at(wd, v)), f32(ar.at(td, v))
                    if not pw > 0:
                        c["empty"] += 1
                        continue
                    if not abs(pt) < f32(1):
                        c["free_space"] += 1
                        continue
                    q, outside = ar.sample_loop(v, nd, voxd, R, t, nc, voxc)
                    if outside:
                        c["outside"] += 1
                        continue
                    if cb is not None and ar.at(cb, [int(np.rint(q[j])) for j in range(3)]) == 0:
                        c["unclaimed"] += 1
                        continue
                    c["released"] += 1
                    c["solid"] += not pt > 0
                    for j in range(3):
                        blo[j], bhi[j] = min(blo[j], v[j]), max(bhi[j], v[j])
                    td[z, y, x], wd[z, y, x] = f32(0), f32(0)
    return td, wd, _record(RELEASE, RELEASE_COUNTS, c, blo, bhi)


def check_identities(rec):
    for r in np.atleast_1d(rec):
        if r.dtype == SEED:
            assert r["visited"] == r["kept"] + r["outside"] + r["unknown"] + r["masked"] + r["saturated"] + r["seeded"], r
            moved = r["seeded"]
        else:
            assert r["visited"] == r["empty"] + r["free_space"] + r["outside"] + r["unclaimed"] + r["released"], r
            moved = r["released"]
        assert r["solid"] <= moved, r
        assert (moved > 0) == bool((r["hi"] >= 0).all()) == bool((r["hi"] >= r["lo"]).all()), r


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------------------------

SHAPES, BOXES, MAX_WEIGHT, DST_CONTENTS, TRUNC_RATIOS = ar.SHAPES, ar.BOXES, ar.MAX_WEIGHT, ar.DST_CONTENTS, ar.TRUNC_RATIOS


def seed_cases(dshape, content, boxes=BOXES):
    """The sweep of absorb_reference.cases -- per destination shape and source content: with and without the source's
    mask, a source on the destination's lattice, a finer one (voxel ratio 0.8) and a coarser one (ratio 2), the six poses;
    the destinations unobserved / random (weights 0, negative, NaN, at maxWeight; tsdf +-1, NaN, -0.0) / fully observed /
    half observed and the boxes whole / one voxel / cutting tiles / empty in turn -- with the truncation ratios 1, 0.5 and
    2 turning so that every pose meets each of them (ratio 0.5: s saturated where u is not; ratio 2: the opposite).
    Yields (name, dst, src, pose, box)."""
    from tests import shape_reference as sr
    k = 0
    for masked in (True, False):
        sources = [(dshape, content, 0.01), ((40, 24, 20), content if content in ("random", "all_solid") else "half_shell", 0.008),
                   ((33, 17, 9), "gated_block" if content != "all_solid" else content, 0.02)]
        for b, (sshape, scontent, svoxel) in enumerate(sources):
            st, sw, sf = sr.volume(sshape, scontent)
            for p, (R, t) in enumerate(ar.poses(svoxel)):
                dcontent = DST_CONTENTS[(k + b) % 4]
                dt, dw, _ = sr.volume(dshape, dcontent)
                ratio = TRUNC_RATIOS[(p + k // 6) % 3]
                kind = boxes[(k + p // 2) % len(boxes)]
                yield (f"{'fg' if masked else 'nofg'}-src{b}-pose{p}-{dcontent}-trunc{ratio}-{kind}",
                       ar.dst_vol(dt, dw, 0.01, 0.04, MAX_WEIGHT), ar.src_vol(st, sw, sf if masked else None, svoxel, 0.04 * ratio),
                       ar.pose_of(R, t), ar.box_of(kind, dshape))
                k += 1


def release_cases(dshape, content, boxes=BOXES):
    """(name, dst, claim, pose, box): the same sweep with the source's mask as the claim -- NULL where the sweep runs
    without the mask, and all zero in every fifth case."""
    for k, (name, dst, src, pose, box) in enumerate(seed_cases(dshape, content, boxes)):
        fg, res = src["fg"], src["tsdf"].shape[::-1]
        if k % 5 == 4:
            fg, name = np.zeros(src["tsdf"].shape, np.uint8), name + "-zero"
        yield name, dst, claim_of(fg, res, src["voxel_size"]), pose, box


def planted_cases():
    """absorb_reference.planted_case -- a smooth wall through a fully observed source, saturated on both sides, with NaN
    and -0.0 tsdf and a zero, a negative and a NaN weight planted at single corners, into a destination with every kind of
    weight -- under each truncation ratio: at 0.5 a saturated s has an unsaturated u, at 2 the opposite.  Yields
    (name, ratio, dst, src, pose)."""
    dst, src, poses = ar.planted_case()
    for ratio in TRUNC_RATIOS:
        for p, pose in enumerate(poses):
            yield f"planted-trunc{ratio}-pose{p}", ratio, dst, dict(src, truncdist=f32(0.04 * ratio)), pose
