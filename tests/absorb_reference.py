"""Absorbing a volume restated (include/emf_hip.h "Absorbing a volume"): the device stage twice --
vectorised numpy in float32, one operation per line, and a plain loop per voxel -- and the float64 pose helper in numpy
and in Python floats.  No GPU, no library: the tests compare emf_hip_absorbVolume and emf_fusion_absorb_pose with these,
as bytes."""
from __future__ import annotations

import numpy as np

from tests.contacts_reference import lerp, sample_points, to_f32

f32 = np.float32

ABSORB = np.dtype([("visited", "<u8"), ("outside", "<u8"), ("unknown", "<u8"), ("masked", "<u8"), ("saturated", "<u8"),
                   ("fused", "<u8"), ("fresh", "<u8"), ("solid", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)])
assert ABSORB.itemsize == 88
COUNTS = ("visited", "outside", "unknown", "masked", "saturated", "fused", "fresh", "solid")


def dst_vol(tsdf, weights, voxel_size=0.01, truncdist=0.04, max_weight=64.0):
    """A destination as the statements take it: (nz, ny, nx) arrays, never written (the statements return new arrays)."""
    return dict(tsdf=np.ascontiguousarray(tsdf, f32), weights=np.ascontiguousarray(weights, f32), voxel_size=f32(voxel_size),
                truncdist=f32(truncdist), max_weight=f32(max_weight))


def src_vol(tsdf, weights, fg=None, voxel_size=0.01, truncdist=0.04):
    return dict(tsdf=np.ascontiguousarray(tsdf, f32), weights=np.ascontiguousarray(weights, f32),
                fg=None if fg is None else np.ascontiguousarray(fg, np.uint8), voxel_size=f32(voxel_size), truncdist=f32(truncdist))


def pose_of(R=None, t=(0, 0, 0)):
    return (np.eye(3, dtype=f32).reshape(9) if R is None else np.asarray(R, f32).reshape(9)), np.asarray(t, f32).reshape(3)


def whole(dst):
    nz, ny, nx = dst["tsdf"].shape
    return (0, 0, 0), (nx, ny, nz)


def neutral(res):
    out = np.zeros((), ABSORB)
    out["lo"], out["hi"] = res, (-1, -1, -1)
    return out


def ratio_of(src, dst):
    with np.errstate(all="ignore"):
        return f32(src["truncdist"]) / f32(dst["truncdist"])


# ---- the device stage, vectorised ----------------------------------------------------------------------------------

def outside_of(q, res):
    """The pad-1 outside rule, a NaN first, of sample points q = (qx, qy, qz) in a volume of res (x, y, z)."""
    with np.errstate(all="ignore"):
        outside = np.zeros(len(q[0]), bool)
        for j in range(3):
            up = q[j] + f32(1)
            outside |= np.isnan(q[j]) | (q[j] < 0) | (up >= f32(res[j]))
    return outside


def absorb(dst, src, pose, box=None):
    """(tsdf, weights, record) of the destination after the pass over box = (lo, size), both (x, y, z)."""
    td, wd = dst["tsdf"].copy(), dst["weights"].copy()
    tb, wb, fb = src["tsdf"], src["weights"], src["fg"]
    nz, ny, nx = td.shape
    res_d, res_s = (nx, ny, nz), tb.shape[::-1]
    R, t = pose_of(*pose)
    lo, size = whole(dst) if box is None else box
    out = neutral(res_d)
    if min(size) <= 0:
        return td, wd, out
    z, y, x = np.meshgrid(*[np.arange(lo[j], lo[j] + size[j]) for j in (2, 1, 0)], indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    out["visited"] = len(x)
    q = sample_points((x, y, z), res_d, dst["voxel_size"], R, t, res_s, src["voxel_size"])
    ratio, max_weight = ratio_of(src, dst), f32(dst["max_weight"])
    with np.errstate(all="ignore"):
        outside = outside_of(q, res_s)
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
        saturated = ~unknown & ~masked & ~(np.abs(s) < f32(1))
        fused = ~unknown & ~masked & ~saturated
        out["unknown"], out["masked"], out["saturated"] = int(unknown.sum()), int(masked.sum()), int(saturated.sum())
        out["fused"] = int(fused.sum())
        if not fused.any():
            return td, wd, out
        x, y, z, s = x[fused], y[fused], z[fused], s[fused]
        scaled = s * ratio
        u = np.minimum(np.maximum(scaled, f32(-1)), f32(1))
        wo = cw[0][fused]
        for w in cw[1:]:
            wo = np.minimum(wo, w[fused])
        pw, pt = wd[z, y, x], td[z, y, x]
        fresh = ~(pw > 0)
        m0 = pw * pt
        m1 = wo * u
        num = m0 + m1
        den = pw + wo
        nt = np.where(fresh, u, num / den)
        nw = np.where(fresh, np.minimum(wo, max_weight), np.minimum(den, max_weight))
        out["fresh"], out["solid"] = int(fresh.sum()), int((~(nt > 0)).sum())
        out["lo"] = [int(c.min()) for c in (x, y, z)]
        out["hi"] = [int(c.max()) for c in (x, y, z)]
        td[z, y, x], wd[z, y, x] = nt.astype(f32), nw.astype(f32)
    return td, wd, out


# ---- the device stage, voxel by voxel --------------------------------------------------------------------------------

def at(arr, v):
    return arr[v[2], v[1], v[0]]


def sample_loop(v, nd, voxd, R, t, ns, voxs):
    """The sample point q of destination voxel v and whether it lies outside; np.float32 scalars, one operation a step."""
    pd = [(f32(v[j]) - f32(nd[j] - 1) / f32(2)) * voxd for j in range(3)]
    q = []
    for i in range(3):
        s = R[3 * i] * pd[0] + R[3 * i + 1] * pd[1]
        s = s + R[3 * i + 2] * pd[2]
        s = s + t[i]
        q.append(s / voxs + f32(ns[i] - 1) / f32(2))
    return q, any(np.isnan(q[j]) or q[j] < 0 or q[j] + f32(1) >= f32(ns[j]) for j in range(3))


def absorb_loop(dst, src, pose, box=None):
    """The same by a plain loop over the box; every float step an np.float32 scalar operation."""
    td, wd = dst["tsdf"].copy(), dst["weights"].copy()
    tb, wb, fb = src["tsdf"], src["weights"], src["fg"]
    nz, ny, nx = td.shape
    nd, ns = (nx, ny, nz), tb.shape[::-1]
    Rm, tm = pose_of(*pose)
    R, t = [f32(v) for v in Rm], [f32(v) for v in tm]
    voxd, voxs = f32(dst["voxel_size"]), f32(src["voxel_size"])
    ratio, max_weight = ratio_of(src, dst), f32(dst["max_weight"])
    lo, size = whole(dst) if box is None else box
    c = dict.fromkeys(COUNTS, 0)
    blo, bhi = list(nd), [-1, -1, -1]

    with np.errstate(all="ignore"):
        for z in range(lo[2], lo[2] + max(size[2], 0)):
            for y in range(lo[1], lo[1] + max(size[1], 0)):
                for x in range(lo[0], lo[0] + max(size[0], 0)):
                    v = (x, y, z)
                    c["visited"] += 1
                    q, outside = sample_loop(v, nd, voxd, R, t, ns, voxs)
                    if outside:
                        c["outside"] += 1
                        continue
                    l = [int(q[j]) for j in range(3)]
                    f = [q[j] - f32(l[j]) for j in range(3)]
                    corners = [(l[0] + dx, l[1] + dy, l[2] + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
                    vals = [f32(at(tb, k)) for k in corners]
                    for j in range(3):  # x pairs, then y, then z
                        vals = [(f32(1) - f[j]) * vals[2 * k] + f[j] * vals[2 * k + 1] for k in range(len(vals) // 2)]
                    s = vals[0]
                    ws = [f32(at(wb, k)) for k in corners]
                    if not all(w > 0 for w in ws) or np.isnan(s):
                        c["unknown"] += 1
                        continue
                    if fb is not None and at(fb, [int(np.rint(q[j])) for j in range(3)]) == 0:
                        c["masked"] += 1
                        continue
                    if not abs(s) < f32(1):
                        c["saturated"] += 1
                        continue
                    u = min(max(s * ratio, f32(-1)), f32(1))
                    wo = min(ws)
                    pw, pt = f32(at(wd, v)), f32(at(td, v))
                    if not pw > 0:
                        nt, nw = u, min(wo, max_weight)
                        c["fresh"] += 1
                    else:
                        nt = (pw * pt + wo * u) / (pw + wo)
                        nw = min(pw + wo, max_weight)
                    c["fused"] += 1
                    c["solid"] += not nt > 0
                    for j in range(3):
                        blo[j], bhi[j] = min(blo[j], v[j]), max(bhi[j], v[j])
                    td[z, y, x], wd[z, y, x] = nt, nw
    out = np.zeros((), ABSORB)
    for k in COUNTS:
        out[k] = c[k]
    out["lo"], out["hi"] = blo, bhi
    return td, wd, out


def check_identities(rec):
    for r in np.atleast_1d(rec):
        assert r["visited"] == r["outside"] + r["unknown"] + r["masked"] + r["saturated"] + r["fused"], r
        assert r["fresh"] <= r["fused"] and r["solid"] <= r["fused"], r
        assert (r["fused"] > 0) == bool((r["hi"] >= 0).all()) == bool((r["hi"] >= r["lo"]).all()), r


# ---- the host stage: the pose, float64 in a fixed order, rounded once ------------------------------------------------
# (R, t) takes the DESTINATION's volume frame into the SOURCE's: with the poses (world <- model) of the destination d and
# the source s,  R_ij = float((Rs_0i * Rd_0j + Rs_1i * Rd_1j) + Rs_2i * Rd_2j),  e_k = td_k - ts_k,
# t_i = float((Rs_0i * e_0 + Rs_1i * e_1) + Rs_2i * e_2): contact_pose with the destination as a and the source as b.

def absorb_pose_np(Rd, td, Rs, ts):
    A, B = np.asarray(Rd, f32).reshape(9).astype(np.float64), np.asarray(Rs, f32).reshape(9).astype(np.float64)
    e = np.asarray(td, f32).reshape(3).astype(np.float64) - np.asarray(ts, f32).reshape(3).astype(np.float64)
    R, t = np.zeros(9, f32), np.zeros(3, f32)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                s = B[i] * A[j]
                s = s + B[3 + i] * A[3 + j]
                s = s + B[6 + i] * A[6 + j]
                R[3 * i + j] = f32(s)
            s = B[i] * e[0]
            s = s + B[3 + i] * e[1]
            s = s + B[6 + i] * e[2]
            t[i] = f32(s)
    return R, t


def absorb_pose_py(Rd, td, Rs, ts):
    A, B = [float(v) for v in np.asarray(Rd, f32).reshape(9)], [float(v) for v in np.asarray(Rs, f32).reshape(9)]
    td, ts = np.asarray(td, f32).reshape(3), np.asarray(ts, f32).reshape(3)
    e = [float(td[k]) - float(ts[k]) for k in range(3)]
    R, t = [0.0] * 9, [0.0] * 3
    for i in range(3):
        for j in range(3):
            s = B[i] * A[j]
            s = s + B[3 + i] * A[3 + j]
            s = s + B[6 + i] * A[6 + j]
            R[3 * i + j] = to_f32(s)
        s = B[i] * e[0]
        s = s + B[3 + i] * e[1]
        s = s + B[6 + i] * e[2]
        t[i] = to_f32(s)
    return np.array(R, f32), np.array(t, f32)


# ---- the physical fixture: an analytic sphere band -----------------------------------------------------------------

def sphere_band(shape, voxel, radius, trunc):
    """A sphere about the volume's centre as a truncated band: weights 1 where |sdf| <= 2 * trunc."""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = [(n - 1) / 2 for n in shape]
    d = np.sqrt(((x - c[0]) * voxel) ** 2 + ((y - c[1]) * voxel) ** 2 + ((z - c[2]) * voxel) ** 2) - radius
    return np.clip(d / trunc, -1, 1).astype(f32), (np.abs(d) <= 2 * trunc).astype(f32), d


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------------------------

SHAPES = [(1, 1, 1), (5, 3, 2), (33, 17, 9), (64, 8, 8), (40, 24, 20)]  # (nx, ny, nz), destination and source
DST_CONTENTS = ("unobserved", "random", "all_solid", "half_shell")  # weights 0 | 0, negative, NaN, at maxWeight | 3 | 4 and 0
MAX_WEIGHT = 64.0  # the largest weight of shape_reference's "random" content: such a voxel is at maxWeight
TRUNC_RATIOS = (1.0, 0.5, 2.0)
BOXES = ("whole", "one", "cut", "empty")


def poses(voxel_s):
    """The six poses of tests/test_gpu_contacts.py poses(): identity, two fractional translations, the 20 degree
    rotation, everything outside, a NaN in t."""
    from tests.contacts_reference import rot_z
    return [(None, (0, 0, 0)), (None, (0.37 * voxel_s, -0.21 * voxel_s, 0.5 * voxel_s)), (None, (-1.5 * voxel_s, 2.25 * voxel_s, 0)),
            (rot_z(20.0), (0.3 * voxel_s, 0, -voxel_s)), (None, (100.0, 0, 0)), (None, (0, np.nan, 0))]


def box_of(kind, res):
    """whole; one voxel; a box that starts and ends inside tiles of 32 x 8 x 8 (where the volume is large enough to have
    more than one); empty."""
    res = np.asarray(res)
    if kind == "whole":
        return (0, 0, 0), tuple(int(v) for v in res)
    if kind == "one":
        return tuple(int(v) for v in res // 2), (1, 1, 1)
    if kind == "cut":
        lo = np.minimum((3, 2, 1), res - 1)
        return tuple(int(v) for v in lo), tuple(int(v) for v in np.minimum(res - lo, (34, 9, 10)))
    return (0, 0, 0), (int(res[0]), 0, int(res[2]))


def cases(dshape, content, boxes=BOXES):
    """For one destination shape and one source content of shape_reference.CONTENTS: with and without the source's
    mask, three sources -- the destination's own lattice, a finer one (voxel ratio 0.8) and a coarser one (ratio 2) --
    under the six poses; the truncation ratio, the destination's content and the box take turns.  Yields
    (name, dst, src, pose, box)."""
    from tests import shape_reference as sr
    k = 0
    for masked in (True, False):
        sources = [(dshape, content, 0.01), ((40, 24, 20), content if content in ("random", "all_solid") else "half_shell", 0.008),
                   ((33, 17, 9), "gated_block" if content != "all_solid" else content, 0.02)]
        for b, (sshape, scontent, svoxel) in enumerate(sources):
            st, sw, sf = sr.volume(sshape, scontent)
            for p, (R, t) in enumerate(poses(svoxel)):
                dcontent = DST_CONTENTS[(k + b) % 4]
                dt, dw, _ = sr.volume(dshape, dcontent)
                strunc = 0.04 * TRUNC_RATIOS[(k // 2) % 3]
                kind = boxes[(k + p // 2) % len(boxes)]
                yield (f"{'fg' if masked else 'nofg'}-src{b}-pose{p}-{dcontent}-{kind}", dst_vol(dt, dw, 0.01, 0.04, MAX_WEIGHT),
                       src_vol(st, sw, sf if masked else None, svoxel, strunc), pose_of(R, t), box_of(kind, dshape))
                k += 1


def planted_case():
    """A smooth wall through a fully observed source with NaN and -0.0 tsdf and a zero, a negative and a NaN weight planted
    at single corners; the destination holds every kind of weight.  Returns (dst, src, poses)."""
    from tests import shape_reference as sr
    shape = (33, 17, 9)
    nz, ny, nx = shape[::-1]
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    tsdf = np.clip((x - 14.3) / 6.0, -1, 1).astype(f32)
    weights = np.full(tsdf.shape, 2.0, f32)
    rng = np.random.default_rng(29)
    for k in range(40):
        at = (rng.integers(nz), rng.integers(ny), rng.integers(8, 21))
        if k % 4 == 0:
            tsdf[at] = (np.nan, -0.0, 0.0)[(k // 4) % 3]
        else:
            weights[at] = (0.0, -1.0, np.nan)[k % 4 - 1]
    dt, dw, _ = sr.volume(shape, "random")
    return dst_vol(dt, dw, 0.01, 0.04, MAX_WEIGHT), src_vol(tsdf, weights, None, 0.01, 0.04), \
        [pose_of(None, (0, 0, 0)), pose_of(None, (0.0031, 0.0047, 0.0013))]
