"""Inputs on which the reference's own kernels are recorded (tests/golden/reference_v1.npz) and
compared live with the oracle (tests/test_oracle_pinned.py): the edges where a restatement of the
reference goes wrong without the mainstream inputs noticing.

A case is (kind, inputs, check).  ``inputs()`` builds named numpy arrays from nothing but numpy,
tests/scenes.py and closed-form volumes, so every test regenerates the same bytes (the recorded
input digests pin that).  ``RUN[kind](B, inp)`` drives a backend ``B`` that has the function names
of oracle/binding.py -- the oracle, or oracle/ref_binding.py -- and returns named outputs.
``check(inp, out)`` asserts, on the reference's outputs alone, that the edge the case is named
after is really exercised, so an input that misses its edge cannot pass vacuously.

Layouts as in oracle/emf_oracle.h.  ``small`` cases are recorded as whole arrays, the others as
digests only.
"""
from __future__ import annotations

import hashlib

import numpy as np

from tests.scenes import Pose, camera_path, intrinsics, rel_CO, rel_OC, render_depth, rot

f32 = np.float32
SPHERES = [((0.25, 0.05, 1.3), 0.22), ((-0.3, -0.1, 1.6), 0.18)]
BG_POSE = Pose(t=[0, 0, 1.28])


def canonical(a: np.ndarray) -> np.ndarray:
    """Equality as assert_parity(exact=True) defines it: every NaN is one value, -0 equals +0."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a + a.dtype.type(0)  # -0 -> +0
        a[np.isnan(a)] = np.nan  # one payload, one sign
    return a


def digest(a: np.ndarray) -> str:
    a = canonical(a)
    h = hashlib.sha256()
    h.update(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def voxel_pixels(res, vox, R, t, K):
    """float64 projection of every voxel centre: (u, v, z) arrays of shape (Nz, Ny, Nx).  For the
    exercise counts only -- never compared with a kernel."""
    nx, ny, nz = [int(v) for v in res]
    ax = [(np.arange(n) - (n - 1) / 2.0) * float(vox) for n in (nx, ny, nz)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    pc = [R[i, 0] * xx + R[i, 1] * yy + R[i, 2] * zz + t[i] for i in range(3)]
    with np.errstate(all="ignore"):
        u = (K[0, 0] * pc[0] + K[0, 2] * pc[2]) / pc[2]
        v = (K[1, 1] * pc[1] + K[1, 2] * pc[2]) / pc[2]
    return u, v, pc[2]


def sampled(res, vox, R, t, K, image):
    """(valid, value): the pixel each voxel reads, away from half-pixel ties (margin 1e-3)."""
    u, v, z = voxel_pixels(res, vox, R, t, K)
    h, w = image.shape
    with np.errstate(all="ignore"):
        iu, iv = np.rint(u), np.rint(v)
        clear = (np.abs(np.abs(u - np.floor(u)) - 0.5) > 1e-3) & (np.abs(np.abs(v - np.floor(v)) - 0.5) > 1e-3)
        ok = (z > 0) & clear & (iu >= 0) & (iu < w) & (iv >= 0) & (iv < h)
    val = np.zeros(u.shape, image.dtype)
    val[ok] = image[iv[ok].astype(int), iu[ok].astype(int)]
    return ok, val


# ---- integrate ----------------------------------------------------------------------------------

def _pack_frames(frames, K, res, vox, trunc, maxw):
    inp = dict(K=np.asarray(K, f32).reshape(3, 3), res=np.asarray(res, np.int32),
               scalars=np.array([vox, trunc, maxw], f32))
    for i, (depth, assoc, R, t) in enumerate(frames):
        inp[f"depth{i}"] = np.ascontiguousarray(depth, f32)
        inp[f"assoc{i}"] = np.ascontiguousarray(assoc, f32)
        inp[f"R{i}"] = np.asarray(R, f32).reshape(3, 3)
        inp[f"t{i}"] = np.asarray(t, f32).reshape(3)
    return inp


def nframes(inp):
    return sum(1 for k in inp if k.startswith("depth"))


def run_integrate(B, inp):
    nx, ny, nz = [int(v) for v in inp["res"]]
    vox, trunc, maxw = [float(v) for v in inp["scalars"]]
    tsdf, wts = np.zeros((nz, ny, nx), f32), np.zeros((nz, ny, nx), f32)
    out = {}
    with np.errstate(all="ignore"):
        for i in range(nframes(inp)):
            B.update_tsdf(inp[f"depth{i}"], inp[f"assoc{i}"], tsdf, wts, inp[f"R{i}"], inp[f"t{i}"],
                          inp["K"], vox, trunc, maxw)
            out[f"tsdf{i}"], out[f"wts{i}"] = tsdf.copy(), wts.copy()
    return out


def _hostile(depth, seed):
    rng = np.random.default_rng(seed)
    m = rng.random(depth.shape)
    d = depth.copy()
    d[m < 0.02] = np.nan
    d[(m >= 0.02) & (m < 0.04)] = np.inf
    d[(m >= 0.04) & (m < 0.06)] = -1.0
    d[(m >= 0.06) & (m < 0.07)] = 0.0
    return d


def _hostile_frames(w, h, K, res, vox):
    frames = []
    for i in range(3):
        cam = camera_path(i)
        depth, _ = render_depth(w, h, K, cam, SPHERES, noise=0.002, dropout=0.01, seed=100 + i)
        assoc = np.ones((h, w), f32)
        if i >= 1:  # a NaN weight, a zero weight and a weight below one on the later frames
            assoc[::7, ::5] = np.nan
            assoc[3::11, :] = 0.0
            assoc[:, 2::9] = 0.25
        oc = rel_OC(cam, BG_POSE)
        frames.append((_hostile(depth, 40 + i), assoc, oc.R32, oc.t32))
    return frames


def in_hostile_64():
    w, h = 160, 120
    K = intrinsics(w, h)
    return _pack_frames(_hostile_frames(w, h, K, (64, 64, 64), 0.04), K, (64, 64, 64), 0.04, f32(0.4), 64.0)


def in_hostile_odd():
    w, h = 96, 72
    K = intrinsics(w, h)
    vox = f32(2.56 / 33)
    return _pack_frames(_hostile_frames(w, h, K, (33, 21, 17), vox), K, (33, 21, 17), vox, f32(10) * vox, 64.0)


def check_hostile(inp, out):
    vox = float(inp["scalars"][0])
    seen = {}
    for i in range(nframes(inp)):
        d, a = inp[f"depth{i}"], inp[f"assoc{i}"]
        prev_w = out[f"wts{i - 1}"] if i else np.zeros_like(out["wts0"])
        ok, dv = sampled(inp["res"], vox, inp[f"R{i}"], inp[f"t{i}"], inp["K"], d)
        _, av = sampled(inp["res"], vox, inp[f"R{i}"], inp[f"t{i}"], inp["K"], a)
        for name, sel in (("nan", np.isnan(dv)), ("inf", np.isposinf(dv)), ("neg", dv < 0), ("zero", dv == 0)):
            for state, wsel in (("unseen", prev_w == 0), ("seen", prev_w > 0)):
                seen[f"{name}/{state}"] = seen.get(f"{name}/{state}", 0) + int((ok & sel & wsel).sum())
        seen["nan assoc"] = seen.get("nan assoc", 0) + int((ok & np.isnan(av) & (dv > 0) & np.isfinite(dv)).sum())
        # what the reference does with them (recorded): a NaN depth is not "<= 0", its sdf fails
        # "sdf >= -truncdist", so an unseen voxel becomes -1 and a seen one is left alone
        nan_unseen = ok & np.isnan(dv) & (prev_w == 0)
        assert np.all(out[f"tsdf{i}"][nan_unseen] == -1) and np.all(out[f"wts{i}"][nan_unseen] == 0)
        # +inf depth: sdf = +inf, tsdf = +1 with weight one whatever the association says
        inf_unseen = ok & np.isposinf(dv) & (prev_w == 0)
        assert np.all(out[f"tsdf{i}"][inf_unseen] == 1) and np.all(out[f"wts{i}"][inf_unseen] == 1)
        # depth <= 0: an unseen voxel becomes 0
        neg_unseen = ok & (dv <= 0) & (prev_w == 0)
        assert np.all(out[f"tsdf{i}"][neg_unseen] == 0) and np.all(out[f"wts{i}"][neg_unseen] == 0)
    for key, n in seen.items():
        assert n >= 5, (key, seen)
    last = nframes(inp) - 1
    assert not np.isnan(out[f"tsdf{last}"]).any() and not np.isnan(out[f"wts{last}"]).any()
    return seen


HALF_K = np.array([[1, 0, 20.5], [0, 1, 20.5], [0, 0, 1]], f32)


def _half_frames(res, w, h, tz):
    """Identity rotation, unit voxels, translation that puts every voxel centre on integer camera
    coordinates: u = X / Z + 20.5 is an exact x.5 wherever Z divides X."""
    frames = []
    half = [(((n - 1) % 2) * 0.5) for n in res]  # (n - 1) / 2 is a half-integer for even n
    for i in range(3):
        yy, xx = np.mgrid[0:h, 0:w]
        depth = (((xx * 3 + yy * 5 + i * 7) % 11) + tz + 2 * i).astype(f32)
        t = [half[0] + i, half[1] - i, half[2] + (res[2] - 1) // 2 + tz + i]
        frames.append((depth, np.ones((h, w), f32), np.eye(3, dtype=f32), np.asarray(t, f32)))
    return frames


def in_halfpixel_64():
    return _pack_frames(_half_frames((64, 64, 64), 96, 72, 4), HALF_K, (64, 64, 64), 1.0, 10.0, 64.0)


def in_halfpixel_small():
    return _pack_frames(_half_frames((9, 9, 3), 48, 40, 2), HALF_K, (9, 9, 3), 1.0, 10.0, 64.0)


def check_halfpixel(inp, out, need=50):
    total = 0
    for i in range(nframes(inp)):
        u, v, z = voxel_pixels(inp["res"], 1.0, inp[f"R{i}"], inp[f"t{i}"], inp["K"])
        h, w = inp[f"depth{i}"].shape
        with np.errstate(all="ignore"):
            tie = (z > 0) & ((u - np.floor(u) == 0.5) | (v - np.floor(v) == 0.5))
            inside = (u > 0) & (u < w - 1) & (v > 0) & (v < h - 1)
            # ties where half-to-even and half-up pick another pixel: the even side below
            differs = tie & inside & (((u - np.floor(u) == 0.5) & (np.floor(u) % 2 == 0)) |
                                      ((v - np.floor(v) == 0.5) & (np.floor(v) % 2 == 0)))
        total += int((differs & (out[f"wts{i}"] > 0)).sum())
    assert total >= need, total
    return total


def in_edges_64():
    """sdf == +truncdist and == -truncdist exactly on the optical axis, a first touch whose weights
    sum to zero, a later one (w + a == 0 with a < 0), and the weight cap."""
    w, h, res, vox = 160, 120, (64, 64, 64), f32(0.125)
    K = np.array([[64, 0, 80], [0, 64, 60], [0, 0, 1]], f32)
    t = np.array([0.0625, 0.0625, 6.0625], f32)  # voxel x = y = 31 lies on the axis, Z = z / 8 + 2.125
    yy, xx = np.mgrid[0:h, 0:w]
    frames = []
    for i in range(3):
        depth = (4.0 + ((xx // 4 + yy // 3 + i) % 9) * 0.25).astype(f32)
        depth[60, 80] = 4.625  # Z(10) + 1.25 = Z(30) - 1.25
        assoc = np.ones((h, w), f32)
        if i == 0:
            assoc[:, :40] = 0.0    # first touch, 0 + 0: untouched
        if i == 1:
            assoc[:, 120:] = -1.0  # 1 + (-1) == 0: untouched
        frames.append((depth, assoc, np.eye(3, dtype=f32), t))
    return _pack_frames(frames, K, res, vox, f32(1.25), 2.5)


def check_edges(inp, out):
    z = np.arange(64, dtype=f32) * f32(0.125) + f32(2.125)
    sdf = f32(4.625) - z  # lambda == 1 and |pos_cam| == Z on the axis: exact
    hi, lo = int(np.flatnonzero(sdf == f32(1.25))[0]), int(np.flatnonzero(sdf == f32(-1.25))[0])
    assert (hi, lo) == (10, 30)
    t0, w0 = out["tsdf0"], out["wts0"]
    assert t0[hi, 31, 31] == 1 and w0[hi, 31, 31] == 1      # sdf == truncdist: tsdf 1, weight 1 (not assoc)
    assert t0[lo, 31, 31] == -1 and w0[lo, 31, 31] == 1     # sdf == -truncdist passes "sdf >= -truncdist"
    assert t0[lo + 1, 31, 31] == -1 and w0[lo + 1, 31, 31] == 0  # one voxel deeper: carved, no weight
    # association weight 0 on the first touch: inside the band the voxel stays untouched (0 + 0 is not
    # > 0); at sdf >= truncdist the weight is 1 whatever the association says
    ok, a0 = sampled(inp["res"], 0.125, inp["R0"], inp["t0"], inp["K"], inp["assoc0"])
    zero = ok & (a0 == 0)
    untouched = zero & (w0 == 0) & (t0 == 0)
    free = zero & (w0 == 1) & (t0 == 1)
    carved = zero & (w0 == 0) & (t0 == -1)
    assert untouched.sum() > 1000 and free.sum() > 1000 and carved.sum() > 50
    assert np.array_equal(zero, untouched | free | carved)
    # weight -1 on a voxel that holds weight 1: 1 + (-1) is not > 0, untouched; free space gets 1 + 1
    _, a1 = sampled(inp["res"], 0.125, inp["R1"], inp["t1"], inp["K"], inp["assoc1"])
    cancel = ok & (a1 == -1) & (w0 == 1)
    kept = cancel & (out["wts1"] == 1) & (out["tsdf1"] == t0)
    grown = cancel & (out["wts1"] == 2)
    assert kept.sum() > 1000 and grown.sum() > 1000 and np.array_equal(cancel, kept | grown)
    assert out["wts2"].max() == 2.5 and (out["wts2"] == 2.5).sum() > 1000
    return int(kept.sum())


# ---- raycast ------------------------------------------------------------------------------------

def sphere_volume(res, vox, centre, radius, trunc):
    """Closed-form truncated sphere: +1 far outside (seen), -1 deep inside (unseen), an unseen slab."""
    nx, ny, nz = res
    ax = [(np.arange(n, dtype=f32) - f32(n - 1) / f32(2)) * f32(vox) for n in (nx, ny, nz)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    d = np.sqrt((xx - f32(centre[0])) ** 2 + (yy - f32(centre[1])) ** 2 + (zz - f32(centre[2])) ** 2, dtype=f32)
    sdf = (d - f32(radius)).astype(f32)
    tsdf = np.clip(sdf / f32(trunc), -1, 1).astype(f32)
    wts = np.where(sdf > -f32(trunc), f32(3), f32(0)).astype(f32)
    wts[:, :, :3] = 0
    tsdf[:, :, :3] = 0
    return tsdf, wts


def forward_grads(tsdf):
    """The gradient volume as a closed form (forward differences, zero on the last planes)."""
    g = np.zeros(tsdf.shape + (3,), f32)
    g[:-1, :-1, :-1, 0] = tsdf[:-1, :-1, 1:] - tsdf[:-1, :-1, :-1]
    g[:-1, :-1, :-1, 1] = tsdf[:-1, 1:, :-1] - tsdf[:-1, :-1, :-1]
    g[:-1, :-1, :-1, 2] = tsdf[1:, :-1, :-1] - tsdf[:-1, :-1, :-1]
    return g


def look_from(pos, away=False, roll=0.0):
    """Camera at ``pos`` looking at the origin (or straight away from it), rolled about its axis."""
    z = -np.asarray(pos, np.float64)
    z /= np.linalg.norm(z)
    if away:
        z = -z
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return Pose(np.stack([x, np.cross(z, x), z], axis=1) @ rot([0, 0, 1], roll), pos)


RW, RH = 96, 72
ODD = dict(res=(33, 21, 17), vox=f32(0.05), centre=(0.1, -0.05, 0.0), radius=0.3)
EVEN = dict(res=(36, 20, 28), vox=f32(0.05), centre=(-0.1, 0.05, 0.1), radius=0.35)
AXIS_K = np.array([[80, 0, 48], [0, 80, 36], [0, 0, 1]], f32)  # integer principal point: dir.x == 0 on column 48


def _ray_inputs(vol, cam, K=None, ray0=None, unseen=False, zero_grad=False):
    trunc = f32(10) * vol["vox"]
    tsdf, wts = sphere_volume(vol["res"], vol["vox"], vol["centre"], vol["radius"], trunc)
    if unseen:
        wts[:] = 0
    grads = forward_grads(tsdf)
    if zero_grad:
        grads[:, : vol["res"][1] // 2] = 0  # the upper half of the volume: normal = 0 / 0 at the hit
    co = rel_CO(cam, Pose())
    return dict(tsdf=tsdf, wts=wts, grads=grads, ray0=np.zeros((RH, RW), f32) if ray0 is None else ray0,
                R=co.R32.reshape(3, 3), t=co.t32.reshape(3),
                K=np.asarray(intrinsics(RW, RH) if K is None else K, f32).reshape(3, 3),
                scalars=np.array([vol["vox"], trunc], f32))


def run_raycast(B, inp):
    h, w = inp["ray0"].shape
    vox, trunc = [float(v) for v in inp["scalars"]]
    with np.errstate(all="ignore"):
        ray, vert, nrm, mask = B.raycast_tsdf(inp["tsdf"], inp["grads"], inp["wts"], None, w, h, inp["R"],
                                              inp["t"], inp["K"], vox, trunc, raylengths=inp["ray0"])[:4]
    return dict(ray=ray, vert=vert, nrm=nrm, mask=(np.asarray(mask) != 0).astype(np.uint8))


def _prev_ray0():
    r = np.zeros((RH, RW), f32)
    r[:, : RW // 3] = 0.75   # in front of the surface: those hits vanish
    r[:, RW // 3: RW // 2] = 5.0  # behind everything: no effect
    r[: RH // 4] = 0.01      # before the volume is entered: "ray not intersecting"
    return r


RAY_CASES = {
    "ray_odd_oblique": lambda: _ray_inputs(ODD, look_from([0.35, -0.45, -1.1], roll=7)),
    "ray_even_oblique": lambda: _ray_inputs(EVEN, look_from([-0.5, 0.3, -1.2], roll=-11)),
    "ray_odd_inside": lambda: _ray_inputs(ODD, Pose(rot([0, 1, 0], -8), [0.0, 0.0, -0.38])),
    "ray_odd_axis": lambda: _ray_inputs(ODD, Pose(t=[0.0, 0.0, -1.0]), K=AXIS_K),
    "ray_even_axis": lambda: _ray_inputs(EVEN, Pose(t=[0.0, 0.0, -1.0]), K=AXIS_K),
    "ray_behind": lambda: _ray_inputs(ODD, look_from([0.35, -0.45, -1.1], away=True)),
    "ray_miss": lambda: _ray_inputs(ODD, Pose(look_from([0.35, -0.45, -1.1]).R @ rot([0, 1, 0], 90), [0.35, -0.45, -1.1])),
    "ray_unseen": lambda: _ray_inputs(ODD, Pose(t=[0.0, 0.0, -1.0]), unseen=True),
    "ray_prev": lambda: _ray_inputs(ODD, Pose(t=[0.02, 0.01, -1.0]), ray0=_prev_ray0()),
    "ray_zero_grad": lambda: _ray_inputs(ODD, Pose(t=[0.02, 0.01, -1.0]), zero_grad=True),
}


def check_ray(name, inp, out):
    hits = int(out["mask"].sum())
    if name in ("ray_miss", "ray_unseen"):
        assert hits == 0 and not out["ray"].any() and not out["vert"].any()
        return hits
    assert hits > 300, hits
    if name == "ray_behind":
        # recorded: entry and exit steps are both negative and ordered, so the reference marches the
        # line BEHIND the camera and reports the surface there with a negative raylength
        m = out["mask"] != 0
        assert np.all(out["ray"][m] < 0) and np.all(out["vert"][m][:, 2] < 0)
    if name.endswith("axis"):
        assert inp["K"][0, 2] == 48 and np.array_equal(inp["R"], np.eye(3, dtype=f32))  # unproj.x == 0 exactly
        # recorded: with dir.x == 0 the entry step is (bound - campos.x) / 0 = +inf, so the reference
        # never enters the volume on that column (nor on the row with dir.y == 0): a cross without hits
        m = out["mask"]
        assert m[:, 48].sum() == 0 and m[36, :].sum() == 0, "a ray with a zero component must miss"
        assert m[:, 47].sum() > 5 and m[:, 49].sum() > 5 and m[35, :].sum() > 5 and m[37, :].sum() > 5
    if name == "ray_prev":
        m = out["mask"]
        assert m[RH // 4:, : RW // 3].sum() == 0 and m[: RH // 4].sum() == 0 and m[RH // 4:, RW // 3:].sum() > 300
        keep = m == 0
        assert np.array_equal(out["ray"][keep], inp["ray0"][keep]), "a pixel without a hit keeps its raylength"
    if name == "ray_zero_grad":
        bad = np.isnan(out["nrm"]).all(axis=2)
        assert bad.sum() > 50 and np.all(out["mask"][bad] != 0) and (~bad & (out["mask"] != 0)).sum() > 50
    else:
        assert not np.isnan(out["nrm"]).any()
    if name == "ray_odd_inside":
        # the camera is inside the box: the entry step is negative, the march starts at one voxel
        assert np.all(np.abs(inp["t"]) < (np.array(ODD["res"]) - 1) // 2 * ODD["vox"])
    return hits


# ---- per-pixel lookups --------------------------------------------------------------------------

def in_lookup():
    """Points with z <= 0 and points put exactly on the cells where ``v + 1 >= N``
    (values) and ``v + 2 >= N`` (pose gradients) flip, in an odd/even/odd volume."""
    res, vox = (11, 8, 9), f32(0.25)
    rng = np.random.default_rng(5)
    vol3 = rng.standard_normal((res[2], res[1], res[0], 3)).astype(f32)
    w, h = 24, 12
    pts = rng.uniform(-1.4, 1.4, (h, w, 3)).astype(f32)
    pts[..., 2] += 3.0
    half = [(n - 1) / 2.0 for n in res]
    k = 0
    for axis in range(3):  # v = p / vox + (N - 1) / 2: land on N - 3, N - 2, N - 1 and 0 exactly
        for cell in (0.0, res[axis] - 3.0, res[axis] - 2.0, res[axis] - 1.0, res[axis] - 1.5, -0.25):
            p = np.zeros(3)
            p[axis] = (cell - half[axis]) * 0.25
            pts[0, k] = p + [0, 0, 3.0]
            k += 1
    # (no NaN point: the reference lets NaN through both range tests and indexes the volume with
    # (int)NaN -- out of bounds, undefined; nothing to pin)
    pts[1, :3] = [[0.1, 0.1, 0.0], [0.1, 0.1, -1.0], [0.1, 0.1, -0.0]]
    return dict(vol3=vol3, vol2=np.ascontiguousarray(vol3[..., :2]), vol1=np.ascontiguousarray(vol3[..., 0]),
                points=pts, R=np.eye(3, dtype=f32), t=np.array([0, 0, -3.0], f32), scalars=np.array([vox], f32))


def run_lookup(B, inp):
    vox = float(inp["scalars"][0])
    with np.errstate(all="ignore"):
        out = {f"vals{c}": B.get_volume_vals(inp[f"vol{c}"], inp["points"], inp["R"], inp["t"], vox) for c in (1, 2, 3)}
        out["pose_grads"] = B.compute_pose_gradients(inp["vol1"], forward_grads(inp["vol1"]), inp["points"], inp["R"],
                                                     inp["t"], vox)
    return out


def check_lookup(inp, out):
    v1, pg = out["vals1"], out["pose_grads"].reshape(inp["points"].shape[:2] + (6,))
    assert np.all(v1[1, :3] == 0) and np.all(pg[1, :3] == 0), "z <= 0 must be skipped"
    for axis in range(3):
        c = 6 * axis  # cells 0, N - 3, N - 2, N - 1, N - 1.5, -0.25 along this axis
        inside_v = [v1[0, c + k] != 0 for k in range(6)]
        assert inside_v == [True, True, True, False, True, False], ("values: outside from v + 1 >= N", axis, inside_v)
        inside_g = [bool(np.any(pg[0, c + k] != 0)) for k in range(6)]
        assert inside_g == [True, True, False, False, False, False], ("gradients: outside from v + 2 >= N", axis, inside_g)
    assert (v1 != 0).sum() > 50
    return int((v1 != 0).sum())


# ---- foreground / background counts -------------------------------------------------------------

def in_fgbg():
    res, vox, w, h = (30, 22, 18), f32(0.8 / 30), 96, 72
    K = intrinsics(w, h)
    pose = Pose(rot([0, 0, 1], 10), SPHERES[0][0])
    tsdf, wts = sphere_volume(res, vox, (0, 0, 0), 0.22, f32(10) * vox)
    wts[:, :, :3] = 0
    inp = dict(tsdf=tsdf, wts=wts, K=np.asarray(K, f32).reshape(3, 3), res=np.asarray(res, np.int32),
               scalars=np.array([vox], f32))
    rng = np.random.default_rng(8)
    for i in range(3):
        cam = camera_path(i)
        _, ids = render_depth(w, h, K, cam, SPHERES, noise=0.002, dropout=0.01, seed=100 + i)
        oc = rel_OC(cam, pose)
        inp[f"mask{i}"] = ((ids == 1).astype(np.uint8) * (1 if i % 2 else 255)).astype(np.uint8)
        inp[f"occl{i}"] = ((rng.random((h, w)) < 0.2) * (255 if i % 2 else 1)).astype(np.uint8)
        inp[f"R{i}"], inp[f"t{i}"] = oc.R32.reshape(3, 3), oc.t32.reshape(3)
    return inp


def in_fgbg_halfpixel():
    """The same rounding as the integrate (__float2int_rn) picks the mask pixel: unit voxels on
    integer camera coordinates again, mask and occlusion bytes drawn from {0, 1, 255}."""
    res, w, h = (16, 12, 6), 48, 40
    rng = np.random.default_rng(17)
    tsdf = rng.uniform(-0.9, 0.9, (res[2], res[1], res[0])).astype(f32)
    wts = (rng.random(tsdf.shape) < 0.9).astype(f32)
    inp = dict(tsdf=tsdf, wts=wts, K=HALF_K.copy(), res=np.asarray(res, np.int32), scalars=np.array([1.0], f32))
    for i in range(3):
        inp[f"mask{i}"] = rng.choice(np.array([0, 1, 255], np.uint8), (h, w))
        inp[f"occl{i}"] = rng.choice(np.array([0, 0, 0, 1, 255], np.uint8), (h, w))
        inp[f"R{i}"] = np.eye(3, dtype=f32)
        inp[f"t{i}"] = np.array([0.5 + i, 0.5 - i, 0.5 + 2 + 3 + i], f32)
    return inp


def check_fgbg_halfpixel(inp, out):
    ties = 0
    for i in range(3):
        u, v, z = voxel_pixels(inp["res"], 1.0, inp[f"R{i}"], inp[f"t{i}"], inp["K"])
        h, w = inp[f"mask{i}"].shape
        fu, fv = u - np.floor(u), v - np.floor(v)
        ties += int(((z > 0) & (u > 0) & (u < w - 1) & (v > 0) & (v < h - 1) & (inp["wts"] > 0) &
                     (((fu == 0.5) & (np.floor(u) % 2 == 0)) | ((fv == 0.5) & (np.floor(v) % 2 == 0)))).sum())
    assert ties >= 50, ties
    assert out["fgbg"].sum(-1).max() == 3
    return ties


def run_fgbg(B, inp):
    nx, ny, nz = [int(v) for v in inp["res"]]
    fgbg = np.zeros((nz, ny, nx, 2), f32)
    for i in range(3):
        B.update_fgbg_probs(inp[f"mask{i}"], inp[f"occl{i}"], inp["tsdf"], inp["wts"], fgbg, inp[f"R{i}"],
                            inp[f"t{i}"], inp["K"], float(inp["scalars"][0]))
    return dict(fgbg=fgbg)


def check_fgbg(inp, out):
    f = out["fgbg"]
    assert f[..., 0].max() == 3 and f[..., 1].max() == 3, "a mask byte of 255 counts as one, like a byte of 1"
    assert np.all(f == np.rint(f)) and f.min() == 0
    assert np.all(f[(inp["wts"] == 0) | (np.abs(inp["tsdf"]) >= 1)] == 0)
    total = f.sum(-1)
    assert ((total > 0) & (total < 3)).sum() > 100, "occluded pixels must leave some voxels with fewer counts"
    return int((total > 0).sum())


# ---- registry -----------------------------------------------------------------------------------

class Case:
    def __init__(self, kind, inputs, check, small):
        self.kind, self.inputs, self.check, self.small = kind, inputs, check, small


RUN = dict(integrate=run_integrate, raycast=run_raycast, lookup=run_lookup, fgbg=run_fgbg)

CASES = {
    "int_hostile_64": Case("integrate", in_hostile_64, check_hostile, False),
    "int_hostile_odd": Case("integrate", in_hostile_odd, check_hostile, True),
    "int_halfpixel_64": Case("integrate", in_halfpixel_64, check_halfpixel, False),
    "int_halfpixel_small": Case("integrate", in_halfpixel_small, lambda i, o: check_halfpixel(i, o, 20), True),
    "int_edges_64": Case("integrate", in_edges_64, check_edges, False),
    "lookup_edges": Case("lookup", in_lookup, check_lookup, True),
    "fgbg_bytes": Case("fgbg", in_fgbg, check_fgbg, True),
    "fgbg_halfpixel": Case("fgbg", in_fgbg_halfpixel, check_fgbg_halfpixel, True),
}
for _name, _fn in RAY_CASES.items():
    # (ray_even_axis is recorded as digests only: the file of whole arrays has a size limit)
    CASES[_name] = Case("raycast", _fn, (lambda n: lambda i, o: check_ray(n, i, o))(_name), _name != "ray_even_axis")
