"""Colour with the band restated (include/emf_hip.h "Absorbing a volume" and "Lifting a volume"): the
colour rules of emf_hip_absorbVolumeColor, emf_hip_seedVolumeColor and emf_hip_releaseVolumeColor twice -- vectorised numpy
with unsigned 64-bit integers for the quotient, and a plain loop per voxel in Python integers.  The geometry (tsdf, weights,
the geometry record) is that of tests/absorb_reference.py and tests/lift_reference.py, called as they are; the classes that
decide which voxels carry colour are restated here on their sample-point, outside and blend helpers and checked against
their records.  No GPU, no library: the tests compare the colour entries with these, as bytes.

A colour volume is a (nz, ny, nx, 4) uint16 array: R, G, B, Wc in 8.8 fixed point.  A destination is ar.dst_vol(...) with
color=; a source ar.src_vol(...) with color= (or None: every source entry is (0, 0, 0, 0))."""
from __future__ import annotations

import numpy as np

from tests import absorb_reference as ar
from tests import lift_reference as lr
from tests.contacts_reference import lerp, sample_points

f32 = np.float32
u64 = np.uint64

COLOR_MOVED = np.dtype([("colored", "<u8"), ("uncolored", "<u8")])
assert COLOR_MOVED.itemsize == 16

# the kinds of voxel a sweep has to reach (test_transfer_color_reference_cpu.py checks that it does)
ABSORB_KINDS = ("fresh_colored", "fresh_uncolored_cleared", "blend", "unweighted_not_fresh", "uncolored_not_fresh", "capped",
                "wide_product")
SEED_KINDS = ("colored", "uncolored")
RELEASE_KINDS = ("cleared", "already_zero")


def capq_of(max_weight):
    """The weight cap in 8.8 fixed point, made once on the host from the destination's maxWeight (float32 steps)."""
    scaled = f32(max_weight) * f32(256)
    if scaled >= f32(65535):
        return 65535
    return max(int(np.rint(scaled)), 1)  # lrintf: ties to even


def moved(colored=0, uncolored=0):
    out = np.zeros((), COLOR_MOVED)
    out["colored"], out["uncolored"] = colored, uncolored
    return out


# ---- which voxels carry colour: the classes of the geometry passes, vectorised ---------------------------------------

def _box_voxels(lo, size):
    z, y, x = np.meshgrid(*[np.arange(lo[j], lo[j] + size[j]) for j in (2, 1, 0)], indexing="ij")
    return x.reshape(-1), y.reshape(-1), z.reshape(-1)


def values_of(dst, src, pose, box, seed):
    """The destination voxels (x, y, z) of the box whose sample is a VALUE inside the band -- the FUSED voxels of an
    absorption, the SEEDED voxels of a seed (seed=True: KEPT voxels leave first and u = s * ratio has to lie in the band
    too) -- and the source voxel (rx, ry, rz) nearest to each sample, ties to even."""
    wd, tb, wb, fb = dst["weights"], src["tsdf"], src["weights"], src["fg"]
    nz, ny, nx = wd.shape
    res_d, res_s = (nx, ny, nz), tb.shape[::-1]
    R, t = ar.pose_of(*pose)
    lo, size = ar.whole(dst) if box is None else box
    none = tuple(np.zeros(0, np.int64) for _ in range(6))
    if min(size) <= 0:
        return none
    x, y, z = _box_voxels(lo, size)
    with np.errstate(all="ignore"):
        if seed:
            kept = wd[z, y, x] > 0
            x, y, z = x[~kept], y[~kept], z[~kept]
        q = sample_points((x, y, z), res_d, dst["voxel_size"], R, t, res_s, src["voxel_size"])
        keep = ~ar.outside_of(q, res_s)
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
        value = seen & ~np.isnan(s)
        r = [np.where(value, np.rint(c), 0).astype(np.int64) for c in q]
        if fb is not None:
            value &= fb[r[2], r[1], r[0]] != 0
        value &= np.abs(s) < f32(1)
        if seed:
            u = s * ar.ratio_of(src, dst)
            value &= np.abs(u) < f32(1)
    return x[value], y[value], z[value], r[0][value], r[1][value], r[2][value]


def released_of(dst, claim, pose, box):
    """The RELEASED voxels (x, y, z) of the box."""
    td, wd, cb = dst["tsdf"], dst["weights"], claim["fg"]
    nz, ny, nx = td.shape
    R, t = ar.pose_of(*pose)
    lo, size = ar.whole(dst) if box is None else box
    if min(size) <= 0:
        return tuple(np.zeros(0, np.int64) for _ in range(3))
    x, y, z = _box_voxels(lo, size)
    with np.errstate(all="ignore"):
        band = (wd[z, y, x] > 0) & (np.abs(td[z, y, x]) < f32(1))
        x, y, z = x[band], y[band], z[band]
        q = sample_points((x, y, z), (nx, ny, nz), dst["voxel_size"], R, t, claim["res"], claim["voxel_size"])
        released = ~ar.outside_of(q, claim["res"])
        if cb is not None:
            r = [np.where(released, np.rint(c), 0).astype(np.int64) for c in q]
            released &= cb[r[2], r[1], r[0]] != 0
    return x[released], y[released], z[released]


def source_entries(src, rx, ry, rz):
    """The source entries at the nearest voxels as (n, 4) u64; zeros without a source colour volume."""
    if src.get("color") is None:
        return np.zeros((len(rx), 4), u64)
    return src["color"][rz, ry, rx].astype(u64)


# ---- the colour rules, vectorised ------------------------------------------------------------------------------------

def absorb_color(dst, src, pose, box=None, kinds=None):
    """(tsdf, weights, record, color, colour record) of the destination after emf_hip_absorbVolumeColor.  kinds: a dict
    that collects how many voxels of each of ABSORB_KINDS the call met."""
    td, wd, rec = ar.absorb(dst, src, pose, box)
    color = dst["color"].copy()
    x, y, z, rx, ry, rz = values_of(dst, src, pose, box, seed=False)
    assert len(x) == rec["fused"], (len(x), rec)
    capq = u64(capq_of(dst["max_weight"]))
    S = source_entries(src, rx, ry, rz)
    D = color[z, y, x].astype(u64)
    with np.errstate(invalid="ignore"):
        fresh = ~(dst["weights"][z, y, x] > 0)
    colored = S[:, 3] > 0
    De = np.where(fresh, u64(0), D[:, 3])
    Sw = S[:, 3]
    den = np.where(colored, De + Sw, u64(1))  # an uncoloured entry divides nothing
    N = D.copy()
    for k in range(3):
        num = De * D[:, k] + Sw * S[:, k] + den // u64(2)  # below 2^34: exact in 64 bits
        N[:, k] = num // den
    N[:, 3] = np.minimum(De + Sw, capq)
    N[~colored] = np.where(fresh[~colored, None], u64(0), D[~colored])
    assert (N <= 65535).all()
    color[z, y, x] = N.astype(np.uint16)
    if kinds is not None:
        found = dict(fresh_colored=fresh & colored, fresh_uncolored_cleared=fresh & ~colored & D.any(axis=1),
                     blend=colored & (De > 0), unweighted_not_fresh=colored & ~fresh & (De == 0), uncolored_not_fresh=~colored & ~fresh,
                     capped=colored & (De + Sw > capq),
                     wide_product=colored & ((De[:, None] * D[:, :3] + Sw[:, None] * S[:, :3]).max(axis=1, initial=0) >= 2 ** 32))
        for name in ABSORB_KINDS:
            kinds[name] = kinds.get(name, 0) + int(found[name].sum())
    return td, wd, rec, color, moved(colored=int(colored.sum()), uncolored=int((~colored).sum()))


def seed_color(dst, src, pose, box=None, kinds=None):
    """(tsdf, weights, record, color, colour record) after emf_hip_seedVolumeColor."""
    td, wd, rec = lr.seed(dst, src, pose, box)
    color = dst["color"].copy()
    x, y, z, rx, ry, rz = values_of(dst, src, pose, box, seed=True)
    assert len(x) == rec["seeded"], (len(x), rec)
    S = source_entries(src, rx, ry, rz)
    colored = S[:, 3] > 0
    S[:, 3] = np.minimum(S[:, 3], u64(capq_of(dst["max_weight"])))
    S[~colored] = 0
    color[z, y, x] = S.astype(np.uint16)
    if kinds is not None:
        kinds["colored"] = kinds.get("colored", 0) + int(colored.sum())
        kinds["uncolored"] = kinds.get("uncolored", 0) + int((~colored).sum())
    return td, wd, rec, color, moved(colored=int(colored.sum()), uncolored=int((~colored).sum()))


def release_color(dst, claim, pose, box=None, kinds=None):
    """(tsdf, weights, record, color, colour record) after emf_hip_releaseVolumeColor."""
    td, wd, rec = lr.release(dst, claim, pose, box)
    color = dst["color"].copy()
    x, y, z = released_of(dst, claim, pose, box)
    assert len(x) == rec["released"], (len(x), rec)
    held = color[z, y, x].any(axis=1) if len(x) else np.zeros(0, bool)
    color[z, y, x] = 0
    if kinds is not None:
        kinds["cleared"] = kinds.get("cleared", 0) + int(held.sum())
        kinds["already_zero"] = kinds.get("already_zero", 0) + int((~held).sum())
    return td, wd, rec, color, moved(colored=int(held.sum()), uncolored=int((~held).sum()))


# ---- the colour rules, voxel by voxel --------------------------------------------------------------------------------

def _value_loop(v, dst, src, nd, ns, voxd, voxs, R, t, ratio, seed):
    """The nearest source voxel of destination voxel v if its sample is a VALUE inside the band, else None: the lines of
    absorb_reference.absorb_loop / lift_reference.seed_loop up to the class decision."""
    tb, wb, fb = src["tsdf"], src["weights"], src["fg"]
    if seed and f32(ar.at(dst["weights"], v)) > 0:
        return None
    q, outside = ar.sample_loop(v, nd, voxd, R, t, ns, voxs)
    if outside:
        return None
    l = [int(q[j]) for j in range(3)]
    f = [q[j] - f32(l[j]) for j in range(3)]
    corners = [(l[0] + dx, l[1] + dy, l[2] + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    vals = [f32(ar.at(tb, k)) for k in corners]
    for j in range(3):  # x pairs, then y, then z
        vals = [(f32(1) - f[j]) * vals[2 * k] + f[j] * vals[2 * k + 1] for k in range(len(vals) // 2)]
    s = vals[0]
    if not all(f32(ar.at(wb, k)) > 0 for k in corners) or np.isnan(s):
        return None
    near = [int(np.rint(q[j])) for j in range(3)]
    if fb is not None and ar.at(fb, near) == 0:
        return None
    if not abs(s) < f32(1):
        return None
    if seed and not abs(s * ratio) < f32(1):
        return None
    return near


def _transfer_color_loop(dst, src, pose, box, seed):
    color = dst["color"].copy()
    nz, ny, nx = dst["tsdf"].shape
    nd, ns = (nx, ny, nz), src["tsdf"].shape[::-1]
    Rm, tm = ar.pose_of(*pose)
    R, t = [f32(v) for v in Rm], [f32(v) for v in tm]
    voxd, voxs = f32(dst["voxel_size"]), f32(src["voxel_size"])
    ratio, capq = ar.ratio_of(src, dst), capq_of(dst["max_weight"])
    lo, size = ar.whole(dst) if box is None else box
    n_col = n_uncol = 0
    with np.errstate(all="ignore"):
        for z in range(lo[2], lo[2] + max(size[2], 0)):
            for y in range(lo[1], lo[1] + max(size[1], 0)):
                for x in range(lo[0], lo[0] + max(size[0], 0)):
                    v = (x, y, z)
                    near = _value_loop(v, dst, src, nd, ns, voxd, voxs, R, t, ratio, seed)
                    if near is None:
                        continue
                    S = [0, 0, 0, 0] if src.get("color") is None else [int(c) for c in ar.at(src["color"], near)]
                    D = [int(c) for c in color[z, y, x]]  # read once, before any channel is written
                    if seed:
                        N = S[:3] + [min(S[3], capq)] if S[3] > 0 else [0, 0, 0, 0]
                    else:
                        fresh = not f32(ar.at(dst["weights"], v)) > 0
                        De = 0 if fresh else D[3]
                        if S[3] == 0:
                            N = [0, 0, 0, 0] if fresh else D
                        else:
                            den = De + S[3]
                            N = [(De * D[k] + S[3] * S[k] + den // 2) // den for k in range(3)] + [min(den, capq)]
                    n_col += S[3] > 0
                    n_uncol += S[3] == 0
                    color[z, y, x] = N
    return color, moved(colored=n_col, uncolored=n_uncol)


def absorb_color_loop(dst, src, pose, box=None):
    """(color, colour record) by a plain loop over the box, every colour step in Python integers."""
    return _transfer_color_loop(dst, src, pose, box, seed=False)


def seed_color_loop(dst, src, pose, box=None):
    return _transfer_color_loop(dst, src, pose, box, seed=True)


def release_color_loop(dst, claim, pose, box=None):
    color = dst["color"].copy()
    td, wd, cb = dst["tsdf"], dst["weights"], claim["fg"]
    nz, ny, nx = td.shape
    nd, nc = (nx, ny, nz), claim["res"]
    Rm, tm = ar.pose_of(*pose)
    R, t = [f32(v) for v in Rm], [f32(v) for v in tm]
    voxd, voxc = f32(dst["voxel_size"]), f32(claim["voxel_size"])
    lo, size = ar.whole(dst) if box is None else box
    n_col = n_uncol = 0
    with np.errstate(all="ignore"):
        for z in range(lo[2], lo[2] + max(size[2], 0)):
            for y in range(lo[1], lo[1] + max(size[1], 0)):
                for x in range(lo[0], lo[0] + max(size[0], 0)):
                    v = (x, y, z)
                    if not f32(ar.at(wd, v)) > 0 or not abs(f32(ar.at(td, v))) < f32(1):
                        continue
                    q, outside = ar.sample_loop(v, nd, voxd, R, t, nc, voxc)
                    if outside or (cb is not None and ar.at(cb, [int(np.rint(q[j])) for j in range(3)]) == 0):
                        continue
                    if any(int(c) != 0 for c in color[z, y, x]):
                        n_col += 1
                    else:
                        n_uncol += 1
                    color[z, y, x] = (0, 0, 0, 0)
    return color, moved(colored=n_col, uncolored=n_uncol)


def check_identities(rec, crec, which):
    """colored + uncolored == fused | seeded | released."""
    assert int(crec["colored"]) + int(crec["uncolored"]) == int(rec[which]), (crec, rec)


# ---- colour contents and the sweep -----------------------------------------------------------------------------------

COLOR_CONTENTS = ("weighted", "hostile", "constant")


def color_volume(shape, content, seed, capq=capq_of(ar.MAX_WEIGHT)):
    """A (nz, ny, nx, 4) u16 colour volume for shape = (nx, ny, nz).
    weighted: about a third of the entries with Wc == 0 -- half of those all zero, half with channels left behind -- the
              rest with weights from 1 up to capq (capq itself included);
    hostile:  the full u16 range in all four values -- products beyond 32 bits, weight sums beyond any cap;
    constant: one colour everywhere, random weights."""
    nx, ny, nz = shape
    rng = np.random.default_rng([0xC0, COLOR_CONTENTS.index(content), seed, nx, ny, nz])
    c = rng.integers(0, 65536, (nz, ny, nx, 4), dtype=np.uint16)
    if content == "hostile":
        edge = rng.random((nz, ny, nx, 4))
        c[edge < 0.15] = 65535
        c[edge > 0.9] = 0
        return c
    if content == "constant":
        c[..., :3] = (0x1234, 0xFFFF, 0x0001)
        c[..., 3] = rng.integers(0, capq + 1, (nz, ny, nx))
        return c
    kind = rng.random((nz, ny, nx))
    c[..., 3] = rng.integers(1, capq + 1, (nz, ny, nx))
    c[..., 3][kind > 0.9] = capq
    c[..., 3][kind < 1 / 3] = 0
    c[kind < 1 / 6] = 0
    return c


def with_color(k, dst, other=None):
    """Case k of a sweep with colour volumes attached: the destination's content turns weighted / hostile / weighted; a
    source's hostile / weighted / weighted / none."""
    shape = dst["tsdf"].shape[::-1]
    dst = dict(dst, color=color_volume(shape, ("weighted", "hostile", "weighted")[k % 3], 1))
    if other is None:
        return dst
    sshape = other["tsdf"].shape[::-1]
    content = ("hostile", "weighted", "weighted", None)[k % 4]
    return dst, dict(other, color=None if content is None else color_volume(sshape, content, 2))


def absorb_cases(dshape, content, boxes=ar.BOXES):
    """absorb_reference.cases with colour: (name, dst, src, pose, box)."""
    for k, (name, dst, src, pose, box) in enumerate(ar.cases(dshape, content, boxes)):
        dst, src = with_color(k, dst, src)
        yield f"{name}-c{k % 3}{k % 4}", dst, src, pose, box


def seed_cases(dshape, content, boxes=lr.BOXES):
    for k, (name, dst, src, pose, box) in enumerate(lr.seed_cases(dshape, content, boxes)):
        dst, src = with_color(k, dst, src)
        yield f"{name}-c{k % 3}{k % 4}", dst, src, pose, box


def release_cases(dshape, content, boxes=lr.BOXES):
    for k, (name, dst, claim, pose, box) in enumerate(lr.release_cases(dshape, content, boxes)):
        yield f"{name}-c{k % 3}", with_color(k, dst), claim, pose, box


def planted_cases():
    """lift_reference.planted_cases (the planted wall under the truncation ratios 1, 0.5 and 2) with colour."""
    for k, (name, ratio, dst, src, pose) in enumerate(lr.planted_cases()):
        dst, src = with_color(k, dst, src)
        yield name, ratio, dst, src, pose
