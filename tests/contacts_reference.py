"""Object contacts restated (include/emf_hip.h "Object contacts"): the device stage twice -- vectorised
numpy in float32, one operation per line, and a plain loop per voxel -- and the host stage in numpy float64 and in
Python floats.  No GPU, no library: the tests compare emf_hip_contactProbe and the emf_fusion_contact_* entries with
these, as bytes."""
from __future__ import annotations

import math
import struct

import numpy as np

from tests.shape_reference import float_keys, key_floats, solid_mask

f32 = np.float32

PAIR = np.dtype([("a", "<i4"), ("b", "<i4"), ("R", "<f4", 9), ("t", "<f4", 3), ("touch", "<f4"), ("reserved", "<i4")])
CONTACT = np.dtype([("surface", "<u8"), ("outside", "<u8"), ("unknown", "<u8"), ("masked", "<u8"), ("sampled", "<u8"),
                    ("inside", "<u8"), ("touching", "<u8"), ("normals", "<u8"), ("sum", "<u8", 3), ("gsum", "<i8", 3),
                    ("lo", "<i4", 3), ("hi", "<i4", 3), ("min_s", "<f4"), ("reserved", "<i4")])
SIDE = np.dtype([("res", "<i4", 3), ("voxel_size", "<f4"), ("truncdist", "<f4"), ("R", "<f4", 9), ("t", "<f4", 3)])
SUMMARY = np.dtype([("state", "<i4"), ("saturated", "<i4"), ("direction", "<i4"), ("has_normal", "<i4"), ("distance_m", "<f8"),
                    ("point", "<f8", 3), ("normal", "<f8", 3), ("corners", "<f8", 24)])
assert PAIR.itemsize == 64 and CONTACT.itemsize == 144 and SIDE.itemsize == 68 and SUMMARY.itemsize == 264
UNSEEN, APART, TOUCHING, PENETRATING = 0, 1, 2, 3
COUNTS = ("surface", "outside", "unknown", "masked", "sampled", "inside", "touching", "normals")


def vol(tsdf, weights, fg=None, voxel_size=0.01):
    """One model as the statements take it: (nz, ny, nx) arrays, fg None = no gate."""
    return dict(tsdf=np.ascontiguousarray(tsdf, f32), weights=np.ascontiguousarray(weights, f32),
                fg=None if fg is None else np.ascontiguousarray(fg, np.uint8), voxel_size=f32(voxel_size))


def pair(a, b, R=None, t=(0, 0, 0), touch=0.0):
    out = np.zeros((), PAIR)
    out["a"], out["b"] = a, b
    out["R"] = np.eye(3, dtype=f32).reshape(9) if R is None else np.asarray(R, f32).reshape(9)
    out["t"] = np.asarray(t, f32).reshape(3)
    out["touch"] = f32(touch)
    return out


def rot_z(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], f32)


# ---- the device stage, vectorised ----------------------------------------------------------------------------------

def surface_mask(tsdf, weights, fg=None):
    """surface(v): solid and at least one face neighbour inside the volume free."""
    solid = solid_mask(tsdf, weights, fg)
    with np.errstate(invalid="ignore"):
        free = (weights > 0) & (tsdf > 0)
    near = np.zeros(tsdf.shape, bool)
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        near[lo] |= free[hi]
        near[hi] |= free[lo]
    return solid & near


def sample_points(xyz, res_a, voxel_a, R, t, res_b, voxel_b):
    """q of the voxels xyz (3 int arrays): every line a single float32 operation, rows summed left to right."""
    with np.errstate(all="ignore"):
        pa = []
        for j in range(3):
            half = f32(res_a[j] - 1) / f32(2)
            d = xyz[j].astype(f32) - half
            pa.append(d * voxel_a)
        q = []
        for i in range(3):
            m0 = R[3 * i] * pa[0]
            m1 = R[3 * i + 1] * pa[1]
            m2 = R[3 * i + 2] * pa[2]
            s = m0 + m1
            s = s + m2
            pb = s + t[i]
            half = f32(res_b[i] - 1) / f32(2)
            d = pb / voxel_b
            q.append(d + half)
    return q


def lerp(g, f, c0, c1):
    m0 = g * c0
    m1 = f * c1
    return m0 + m1


def probe(va, vb, pr):
    """The record of one ordered pair (a 0-d array of CONTACT), vectorised."""
    ta, wa = va["tsdf"], va["weights"]
    tb, wb, fb = vb["tsdf"], vb["weights"], vb["fg"]
    nz, ny, nx = ta.shape
    res_a, res_b = (nx, ny, nz), tb.shape[::-1]
    R, t, touch = pr["R"].astype(f32), pr["t"].astype(f32), f32(pr["touch"])
    out = np.zeros((), CONTACT)
    out["lo"], out["hi"], out["min_s"] = res_a, (-1, -1, -1), np.inf
    z, y, x = np.nonzero(surface_mask(ta, wa, va["fg"]))
    out["surface"] = len(x)
    if len(x) == 0:
        return out
    q = sample_points((x, y, z), res_a, va["voxel_size"], R, t, res_b, vb["voxel_size"])
    with np.errstate(all="ignore"):
        outside = np.zeros(len(x), bool)
        for j in range(3):
            up = q[j] + f32(1)
            outside |= np.isnan(q[j]) | (q[j] < 0) | (up >= f32(res_b[j]))
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
            r = [np.rint(c).astype(np.int64) for c in q]
            r = [np.where(unknown, 0, c) for c in r]
            masked = ~unknown & (fb[r[2], r[1], r[0]] == 0)
        sampled = ~unknown & ~masked
        out["unknown"], out["masked"], out["sampled"] = int(unknown.sum()), int(masked.sum()), int(sampled.sum())
        if not sampled.any():
            return out
        out["min_s"] = key_floats(float_keys(s[sampled]).min())
        out["inside"] = int((sampled & (s < 0)).sum())
        touching = sampled & (s <= touch)
        n = int(touching.sum())
        out["touching"] = n
        if n == 0:
            return out
        x, y, z = x[touching], y[touching], z[touching]
        out["sum"] = [int(c.astype(object).sum()) for c in (x, y, z)]
        out["lo"] = [int(c.min()) for c in (x, y, z)]
        out["hi"] = [int(c.max()) for c in (x, y, z)]
        inner = (x > 0) & (x + 1 < nx) & (y > 0) & (y + 1 < ny) & (z > 0) & (z + 1 < nz)
        x, y, z = x[inner], y[inner], z[inner]
        steps = ((0, 0, 1), (0, 1, 0), (1, 0, 0))  # (dz, dy, dx) of e_0, e_1, e_2
        ok = np.ones(len(x), bool)
        grads = []
        for dz, dy, dx in steps:
            ok &= (wa[z + dz, y + dy, x + dx] > 0) & (wa[z - dz, y - dy, x - dx] > 0)
            grads.append(ta[z + dz, y + dy, x + dx] - ta[z - dz, y - dy, x - dx])
        for gj in grads:
            ok &= np.isfinite(gj)
        out["normals"] = int(ok.sum())
        gs = []
        for gj in grads:
            scaled = gj[ok] * f32(4096)
            clipped = np.minimum(np.maximum(scaled, f32(-8192)), f32(8192))
            gs.append(int(np.rint(clipped).astype(np.int64).sum()))
        out["gsum"] = gs
    return out


# ---- the device stage, voxel by voxel --------------------------------------------------------------------------------

def probe_loop(va, vb, pr):
    """The same record by a plain loop over a's voxels; every float step an np.float32 scalar operation."""
    ta, wa, fa = va["tsdf"], va["weights"], va["fg"]
    tb, wb, fb = vb["tsdf"], vb["weights"], vb["fg"]
    nz, ny, nx = ta.shape
    na, nb = (nx, ny, nz), tb.shape[::-1]
    R, t, touch = [f32(v) for v in pr["R"]], [f32(v) for v in pr["t"]], f32(pr["touch"])
    voxa, voxb = f32(va["voxel_size"]), f32(vb["voxel_size"])
    c = dict.fromkeys(COUNTS, 0)
    ssum, gsum, lo, hi = [0, 0, 0], [0, 0, 0], list(na), [-1, -1, -1]
    best = None

    def at(arr, v):
        return arr[v[2], v[1], v[0]]

    def neighbours(v):
        for axis in range(3):
            for step in (-1, 1):
                q = list(v)
                q[axis] += step
                if 0 <= q[axis] < na[axis]:
                    yield q

    with np.errstate(all="ignore"):
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    v = (x, y, z)
                    if not at(wa, v) > 0 or (fa is not None and at(fa, v) == 0) or at(ta, v) > 0:
                        continue
                    if not any(at(wa, n) > 0 and at(ta, n) > 0 for n in neighbours(v)):
                        continue
                    c["surface"] += 1
                    pa = [(f32(v[j]) - f32(na[j] - 1) / f32(2)) * voxa for j in range(3)]
                    q = []
                    for i in range(3):
                        s = R[3 * i] * pa[0] + R[3 * i + 1] * pa[1]
                        s = s + R[3 * i + 2] * pa[2]
                        s = s + t[i]
                        q.append(s / voxb + f32(nb[i] - 1) / f32(2))
                    if any(np.isnan(q[j]) or q[j] < 0 or q[j] + f32(1) >= f32(nb[j]) for j in range(3)):
                        c["outside"] += 1
                        continue
                    l = [int(q[j]) for j in range(3)]
                    f = [q[j] - f32(l[j]) for j in range(3)]
                    corners = [(l[0] + dx, l[1] + dy, l[2] + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
                    vals = [f32(at(tb, k)) for k in corners]
                    for j in range(3):  # x pairs, then y, then z
                        vals = [(f32(1) - f[j]) * vals[2 * k] + f[j] * vals[2 * k + 1] for k in range(len(vals) // 2)]
                    s = vals[0]
                    if not all(at(wb, k) > 0 for k in corners) or np.isnan(s):
                        c["unknown"] += 1
                        continue
                    if fb is not None and at(fb, [int(np.rint(q[j])) for j in range(3)]) == 0:
                        c["masked"] += 1
                        continue
                    c["sampled"] += 1
                    key = int(float_keys(s).reshape(-1)[0])
                    best = key if best is None else min(best, key)
                    c["inside"] += bool(s < 0)
                    if not s <= touch:
                        continue
                    c["touching"] += 1
                    for j in range(3):
                        ssum[j] += v[j]
                        lo[j], hi[j] = min(lo[j], v[j]), max(hi[j], v[j])
                    around = list(neighbours(v))
                    if len(around) < 6 or not all(at(wa, n) > 0 for n in around):
                        continue
                    g = [f32(at(ta, around[2 * j + 1])) - f32(at(ta, around[2 * j])) for j in range(3)]
                    if not all(np.isfinite(gj) for gj in g):
                        continue
                    c["normals"] += 1
                    for j in range(3):
                        gsum[j] += int(np.rint(min(max(g[j] * f32(4096), f32(-8192)), f32(8192))))
    out = np.zeros((), CONTACT)
    for k in COUNTS:
        out[k] = c[k]
    out["sum"], out["gsum"], out["lo"], out["hi"] = ssum, gsum, lo, hi
    out["min_s"] = np.inf if best is None else key_floats(np.uint32(best))
    return out


def expected(volumes, pairs, statement=probe):
    """The records of a pair list over a list of vol()s."""
    out = np.zeros(len(pairs), CONTACT)
    for k, pr in enumerate(pairs):
        out[k] = statement(volumes[int(pr["a"])], volumes[int(pr["b"])], pr)
    return out


def check_identities(rec):
    for r in np.atleast_1d(rec):
        assert r["surface"] == r["outside"] + r["unknown"] + r["masked"] + r["sampled"], r
        assert r["inside"] <= r["sampled"] and r["touching"] <= r["sampled"] and r["normals"] <= r["touching"], r
        assert r["reserved"] == 0 and (r["sampled"] > 0) == bool(np.isfinite(r["min_s"])), r


# ---- the host stage: numpy float64 ------------------------------------------------------------------------------------

def side(res, voxel_size, truncdist, R=None, t=(0, 0, 0)):
    out = np.zeros((), SIDE)
    out["res"], out["voxel_size"], out["truncdist"] = res, voxel_size, truncdist
    out["R"] = np.eye(3, dtype=f32).reshape(9) if R is None else np.asarray(R, f32).reshape(9)
    out["t"] = np.asarray(t, f32).reshape(3)
    return out


def contact_pose_np(Ra, ta, Rb, tb):
    A, B = np.asarray(Ra, f32).reshape(9).astype(np.float64), np.asarray(Rb, f32).reshape(9).astype(np.float64)
    d = np.asarray(ta, f32).astype(np.float64) - np.asarray(tb, f32).astype(np.float64)
    R, t = np.zeros(9, f32), np.zeros(3, f32)
    for i in range(3):
        for j in range(3):
            s = B[i] * A[j]
            s = s + B[3 + i] * A[3 + j]
            s = s + B[6 + i] * A[6 + j]
            R[3 * i + j] = f32(s)
        s = B[i] * d[0]
        s = s + B[3 + i] * d[1]
        s = s + B[6 + i] * d[2]
        t[i] = f32(s)
    return R, t


def contact_touch_np(touch_m, truncdist_b):
    with np.errstate(all="ignore"):
        return f32(np.float64(touch_m) / np.float64(f32(truncdist_b)))


def _to_world_np(vox, sd):
    R, t = sd["R"].astype(np.float64), sd["t"].astype(np.float64)
    half = (sd["res"].astype(np.float64) - 1.0) / 2.0
    c = np.asarray(vox, np.float64) - half
    o = c * np.float64(sd["voxel_size"])
    return _rotate_np(o, R) + t


def _rotate_np(p, R):
    w = np.zeros(3)
    for i in range(3):
        s = R[3 * i] * p[0]
        s = s + R[3 * i + 1] * p[1]
        s = s + R[3 * i + 2] * p[2]
        w[i] = s
    return w


def contact_summary_np(ab, ba, sa, sb):
    out = np.zeros((), SUMMARY)
    recs = [ab] + ([] if ba is None else [ba])
    tot = {k: sum(int(r[k]) for r in recs) for k in ("inside", "touching", "sampled")}
    out["state"] = PENETRATING if tot["inside"] else TOUCHING if tot["touching"] else APART if tot["sampled"] else UNSEEN
    with np.errstate(all="ignore"):
        d = np.float64(ab["min_s"]) * np.float64(sb["truncdist"])
        deciding = ab["min_s"]
        if ba is not None:
            dba = np.float64(ba["min_s"]) * np.float64(sa["truncdist"])
            if dba < d:
                d, deciding = dba, ba["min_s"]
    out["distance_m"], out["saturated"], out["direction"] = d, int(deciding == f32(1)), -1
    if ab["touching"] > 0 and (ba is None or ab["touching"] >= ba["touching"]):
        rec, sd, out["direction"] = ab, sa, 0
    elif ba is not None and ba["touching"] > 0:
        rec, sd, out["direction"] = ba, sb, 1
    else:
        return out
    m = rec["sum"].astype(np.float64) / np.float64(rec["touching"])
    out["point"] = _to_world_np(m, sd)
    g = rec["gsum"].astype(np.float64)
    sq = g[0] * g[0]
    sq = sq + g[1] * g[1]
    sq = sq + g[2] * g[2]
    length = np.sqrt(sq)
    if rec["normals"] > 0 and length > 0:
        out["normal"], out["has_normal"] = _rotate_np(g / length, sd["R"].astype(np.float64)), 1
    out["corners"] = np.concatenate([_to_world_np([(rec["hi"] if (c >> j) & 1 else rec["lo"])[j] for j in range(3)], sd)
                                     for c in range(8)])
    return out


# ---- the host stage: Python floats ------------------------------------------------------------------------------------

def to_f32(v: float) -> float:
    """A Python float rounded to float32 once (ties to even), as a Python float."""
    if math.isnan(v) or math.isinf(v):
        return v
    try:
        return struct.unpack("<f", struct.pack("<f", v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


def contact_pose_py(Ra, ta, Rb, tb):
    A, B = [float(v) for v in np.asarray(Ra, f32).reshape(9)], [float(v) for v in np.asarray(Rb, f32).reshape(9)]
    d = [float(f32(ta[k])) - float(f32(tb[k])) for k in range(3)]
    R, t = [0.0] * 9, [0.0] * 3
    for i in range(3):
        for j in range(3):
            s = B[i] * A[j]
            s = s + B[3 + i] * A[3 + j]
            s = s + B[6 + i] * A[6 + j]
            R[3 * i + j] = to_f32(s)
        s = B[i] * d[0]
        s = s + B[3 + i] * d[1]
        s = s + B[6 + i] * d[2]
        t[i] = to_f32(s)
    return np.array(R, f32), np.array(t, f32)


def contact_touch_py(touch_m, truncdist_b):
    den = float(f32(truncdist_b))
    if den == 0.0:
        return f32(contact_touch_np(touch_m, truncdist_b))  # Python raises where IEEE gives inf or NaN
    return f32(to_f32(float(touch_m) / den))


def contact_summary_py(ab, ba, sa, sb):
    out = np.zeros((), SUMMARY)
    recs = [ab] + ([] if ba is None else [ba])
    inside, touching, sampled = (sum(int(r[k]) for r in recs) for k in ("inside", "touching", "sampled"))
    out["state"] = PENETRATING if inside else TOUCHING if touching else APART if sampled else UNSEEN
    d, deciding = float(ab["min_s"]) * float(sb["truncdist"]), float(ab["min_s"])
    if ba is not None:
        dba = float(ba["min_s"]) * float(sa["truncdist"])
        if dba < d:
            d, deciding = dba, float(ba["min_s"])
    out["distance_m"], out["saturated"], out["direction"] = d, int(deciding == 1.0), -1
    if int(ab["touching"]) > 0 and (ba is None or int(ab["touching"]) >= int(ba["touching"])):
        rec, sd, out["direction"] = ab, sa, 0
    elif ba is not None and int(ba["touching"]) > 0:
        rec, sd, out["direction"] = ba, sb, 1
    else:
        return out
    R, t = [float(v) for v in sd["R"]], [float(v) for v in sd["t"]]
    half = [(float(int(sd["res"][j])) - 1.0) / 2.0 for j in range(3)]
    vs = float(sd["voxel_size"])

    def rotate(p):
        w = []
        for i in range(3):
            s = R[3 * i] * p[0]
            s = s + R[3 * i + 1] * p[1]
            s = s + R[3 * i + 2] * p[2]
            w.append(s)
        return w

    def to_world(vox):
        o = []
        for j in range(3):
            c = vox[j] - half[j]
            o.append(c * vs)
        w = rotate(o)
        return [w[i] + t[i] for i in range(3)]

    n = float(int(rec["touching"]))
    out["point"] = to_world([float(int(rec["sum"][j])) / n for j in range(3)])
    g = [float(int(rec["gsum"][j])) for j in range(3)]
    sq = g[0] * g[0]
    sq = sq + g[1] * g[1]
    sq = sq + g[2] * g[2]
    length = math.sqrt(sq)
    if int(rec["normals"]) > 0 and length > 0.0:
        out["normal"], out["has_normal"] = rotate([g[j] / length for j in range(3)]), 1
    corners = []
    for c in range(8):
        corners += to_world([float(int((rec["hi"] if (c >> j) & 1 else rec["lo"])[j])) for j in range(3)])
    out["corners"] = corners
    return out


# ---- the physical fixture: two analytic sphere bands -------------------------------------------------------------------

SPHERE_RADIUS, SPHERE_TRUNC, SPHERE_TOUCH = 0.07, 0.04, 0.25
SPHERE_PROBE = ((24, 24, 24), 0.01)      # (nx, ny, nz), voxel size
SPHERE_FIELD = ((32, 20, 24), 0.0125)
SPHERE_DX = (0.60, 0.19, 0.16, 0.14, 0.12, 0.06)
SPHERE_STATES = (UNSEEN, APART, APART, TOUCHING, PENETRATING, PENETRATING)


def sphere_band(shape, voxel):
    """A sphere about the volume's centre as a truncated band: weights 1 where sdf >= -trunc."""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = [(n - 1) / 2 for n in shape]
    d = np.sqrt(((x - c[0]) * voxel) ** 2 + ((y - c[1]) * voxel) ** 2 + ((z - c[2]) * voxel) ** 2) - SPHERE_RADIUS
    tsdf = np.clip(d / SPHERE_TRUNC, -1, 1).astype(f32)
    weights = (d >= -SPHERE_TRUNC).astype(f32)
    return vol(tsdf, weights, None, voxel)


def sphere_pair(dx):
    return pair(0, 1, rot_z(20.0), (dx, 0.01, -0.005), SPHERE_TOUCH)


def sphere_gap(dx):
    """The true gap between the two spheres' surfaces, metres (negative: the depth of the overlap)."""
    return math.sqrt(dx * dx + 0.01 ** 2 + 0.005 ** 2) - 2 * SPHERE_RADIUS
