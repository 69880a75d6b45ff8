"""The inputs and references of the life-cycle shape tests (tests/test_lifecycle_cases_cpu.py,
tests/test_gpu_lifecycle_shapes.py): images, volumes and values chosen by the branch of lifecycle.hip (and k_hide_label)
they steer, with plain numpy references that share no code with the kernels.  Nothing here touches the GPU.

Images are (h, w[, c]); volumes are (nz, ny, nx) and their resolutions (nx, ny, nz), like everywhere in the project."""
import numpy as np

from tests.scenes import rot

f32 = np.float32


# ---- references (also used by tests/test_gpu_lifecycle.py) -----------------------------------------------------------

def sorted_stats(points, mask, R, t):
    """The reference's way: compact, transform, sort each channel, take two columns."""
    valid = (mask != 0) & np.any(points != 0, axis=2)
    p = points[valid].astype(f32)
    n = len(p)
    if n == 0:
        return 0, np.zeros(3, f32), np.zeros(3, f32)
    R = np.asarray(R, f32).reshape(3, 3)
    q = np.empty_like(p)
    for i in range(3):  # (r0 x + r1 y) + r2 z, then + t: the product's operation order
        q[:, i] = f32(f32(f32(R[i, 0] * p[:, 0]) + f32(R[i, 1] * p[:, 1])) + f32(R[i, 2] * p[:, 2])) + f32(t[i])
    s = np.sort(q, axis=0)
    return n, s[int(f32(n) * f32(.1))], s[int(f32(n) * f32(.9))]


def f32_transform(R, t, p):
    return np.stack([f32(f32(f32(R[i, 0] * p[:, 0]) + f32(R[i, 1] * p[:, 1])) + f32(R[i, 2] * p[:, 2])) + t[i]
                     for i in range(3)], -1).astype(f32)


CORNERS = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)]  # dx, dy, dz
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def mesh_cloud(tsdf, weights, fg, voxel):
    """Vertex cloud of the reference's marching cubes (TSDF.cu:855-1152, ObjTSDF.cpp:247-268) in numpy:
    one vertex per sign-changing edge of every cube whose 8 voxels pass the mask, vertexInterp."""
    nz, ny, nx = tsdf.shape
    ok = weights > 0 if fg is None else (weights > 0) & (fg != 0)
    corner = CORNERS
    sub = lambda a, c: a[c[2]:nz - 1 + c[2], c[1]:ny - 1 + c[1], c[0]:nx - 1 + c[0]]
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in corner:
        valid &= sub(ok, c)
    zz, yy, xx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    half = [f32(n - 1) / f32(2) for n in (nx, ny, nz)]
    pos = lambda c: np.stack([(f32(1) * (xx + c[0]).astype(f32) - half[0]) * f32(voxel),
                              ((yy + c[1]).astype(f32) - half[1]) * f32(voxel),
                              ((zz + c[2]).astype(f32) - half[2]) * f32(voxel)], -1).astype(f32)
    out = []
    for a, b in EDGES:
        v1, v2 = sub(tsdf, corner[a]), sub(tsdf, corner[b])
        sel = valid & ((v1 < 0) != (v2 < 0))
        p1, p2, v1, v2 = pos(corner[a])[sel], pos(corner[b])[sel], v1[sel], v2[sel]
        mu = (-v1 / (v2 - v1)).astype(f32)
        p = (p1 + (mu[:, None] * (p2 - p1)).astype(f32)).astype(f32)
        use1 = (np.abs(v1).astype(np.float64) < 1e-5)
        use2 = ~use1 & (np.abs(v2).astype(np.float64) < 1e-5)
        use3 = ~use1 & ~use2 & (np.abs(v1 - v2).astype(np.float64) < 1e-5)
        p[use1 | use3] = p1[use1 | use3]
        p[use2] = p2[use2]
        out.append(p)
    return np.concatenate(out) if out else np.zeros((0, 3), f32)


def interp_branches(tsdf, weights, fg):
    """How many vertices of mesh_cloud take the first end of their edge, the second end, an interpolated position."""
    nz, ny, nx = tsdf.shape
    ok = weights > 0 if fg is None else (weights > 0) & (fg != 0)
    sub = lambda a, c: a[c[2]:nz - 1 + c[2], c[1]:ny - 1 + c[1], c[0]:nx - 1 + c[0]]
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in CORNERS:
        valid &= sub(ok, c)
    first = second = between = 0
    for a, b in EDGES:
        v1, v2 = sub(tsdf, CORNERS[a]), sub(tsdf, CORNERS[b])
        sel = valid & ((v1 < 0) != (v2 < 0))
        e1 = np.abs(v1[sel]).astype(np.float64) < 1e-5
        e2 = ~e1 & (np.abs(v2[sel]).astype(np.float64) < 1e-5)
        first, second, between = first + int(e1.sum()), second + int(e2.sum()), between + int((~e1 & ~e2).sum())
    return first, second, between


# ---- order statistics: values written as bit patterns ----------------------------------------------------------------
# With R = I and t = 0 the transformed coordinate is (1 * x + 0 * y) + 0 * z + 0, which is x itself for every finite x
# other than -0.  So a channel of the points image is the data of one selection, bit for bit.  Finite values only and
# no -0.0f: numpy's sort and the radix order disagree on -0 against +0 (the keys differ, the floats compare equal),
# and the reference's own sort is not pinned there.  No +0 either, so that no pixel is the invalid point (0, 0, 0).

def ranks(n):
    """computePercentiles' two columns of n sorted points (EMFusion.cu:90-91)."""
    return int(f32(n) * f32(.1)), int(f32(n) * f32(.9))


def order_key(v):
    """The order-preserving map float32 -> uint32 of a radix select, restated for the checks of the CPU file (which
    byte of the selected element decides what); the reference of the GPU tests is np.sort, not this."""
    u = np.ascontiguousarray(v, f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_value(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(f32)


def all_equal(n, rng, value=-0.3):
    return np.full(n, value, f32)


def low_byte_only(n, rng):
    """1.5 <= v < 1.5 + 256 ulp: the keys share their top 24 bits."""
    return (np.uint32(0x3FC00000) | rng.integers(0, 256, n).astype(np.uint32)).view(f32)


def _sign_boundary(n, rng, negatives):
    mag = rng.uniform(0.001, 3.0, n).astype(f32)
    if negatives > 0:
        mag[0] = 2e-38            # the last negative and the first positive are as close to zero as normal numbers get
    if negatives < n:
        mag[negatives] = 2e-38
    mag[:negatives] *= f32(-1)
    return mag


def sign_last_negative(n, rng):
    """rank + 1 negatives: the p10 element is the last negative value."""
    return _sign_boundary(n, rng, ranks(n)[0] + 1)


def sign_first_positive(n, rng):
    """rank negatives: the p10 element is the first positive value."""
    return _sign_boundary(n, rng, ranks(n)[0])


TIE_MIN = 2100  # the smallest n at which two runs of 1000 fit round the two ranks with other values on every side


def tie_run(n, rng):
    """Two runs of max(1000, n / 4) equal values, one round each rank, the neighbours of each run one ulp away."""
    assert n >= TIE_MIN
    r10, r90 = ranks(n)
    L = max(1000, n // 4)
    a0 = max(1, r10 - L // 2)
    b0 = min(n - 1 - L, r90 - L // 2)
    va, vb = f32(-0.75), f32(1.25)
    below = rng.uniform(-5, -0.8, a0).astype(f32)
    below[0] = np.nextafter(va, f32(-9))
    mid = rng.uniform(-0.7, 1.2, b0 - (a0 + L)).astype(f32)
    mid[mid == 0] = 0.5
    mid[0], mid[1] = np.nextafter(va, f32(9)), np.nextafter(vb, f32(-9))
    above = rng.uniform(1.3, 5, n - (b0 + L)).astype(f32)
    above[0] = np.nextafter(vb, f32(9))
    return np.concatenate([below, np.full(L, va), mid, np.full(L, vb), above]).astype(f32)


def _round_keys(n, rng, key_a, key_b):
    """n values whose sorted order has the element of key key_a at the p10 rank and that of key_b at the p90 rank.
    The others lie 1 .. 2^8, 2^16 or 2^22 key steps away from one of the two, a third each: some share three, two
    and one key bytes with a selected element, so every pass has something to separate."""
    r10, r90 = ranks(n)
    assert r10 < r90 and key_b - key_a > (1 << 23)

    def offsets(m):
        return rng.integers(1, 1 << rng.choice([8, 16, 22], m), m, dtype=np.int64, endpoint=True)

    mid = r90 - r10 - 1
    keys = np.concatenate([key_a - offsets(r10), [key_a], key_a + offsets(mid // 2), key_b - offsets(mid - mid // 2),
                           [key_b], key_b + offsets(n - 1 - r90)])
    return key_value(keys.astype(np.uint32))


def byte_ff(n, rng):
    """The selected keys are 0xBFFFFFFF and 0xC0FFFFFF (positive floats): 0xFF in each of the three low bytes."""
    return _round_keys(n, rng, 0xBFFFFFFF, 0xC0FFFFFF)


def byte_00(n, rng):
    """The selected keys are 0x40000000 and 0x41000000 (negative floats): 0x00 in each of the three low bytes."""
    return _round_keys(n, rng, 0x40000000, 0x41000000)


def denormal_and_huge(n, rng):
    kind = rng.integers(0, 3, n)
    sign = np.where(rng.integers(0, 2, n) == 1, f32(-1), f32(1))
    den = rng.integers(1, 0x800000, n).astype(np.uint32).view(f32)
    v = np.where(kind == 0, den, np.where(kind == 1, rng.uniform(0.5e30, 2e30, n), rng.uniform(0.01, 10, n)))
    return (v.astype(f32) * sign).astype(f32)


CHANNELS = dict(all_equal=all_equal, low_byte_only=low_byte_only, sign_last_negative=sign_last_negative,
                sign_first_positive=sign_first_positive, tie_run=tie_run, byte_ff=byte_ff, byte_00=byte_00,
                denormal_and_huge=denormal_and_huge)

# (w, h, the cases of the x, y and z channel, padding columns of the points image and of the mask).  The three
# channels of a call hold different cases, so the 6 selections of a call diverge.
ORDER_CASES = [
    (64, 48, ("all_equal", "low_byte_only", "sign_last_negative"), (0, 0)),
    (64, 48, ("sign_first_positive", "tie_run", "byte_ff"), (0, 0)),
    (64, 48, ("byte_00", "denormal_and_huge", "all_equal"), (0, 0)),
    (1, 1, ("sign_last_negative", "sign_first_positive", "all_equal"), (1, 2)),  # tie_run needs TIE_MIN points:
    (5, 3, ("sign_last_negative", "sign_first_positive", "low_byte_only"), (2, 1)),    # absent below 2100 pixels
    (257, 3, ("sign_first_positive", "sign_last_negative", "low_byte_only"), (4, 3)),
    (161, 77, ("tie_run", "sign_last_negative", "sign_first_positive"), (3, 7)),
    (640, 480, ("tie_run", "byte_ff", "denormal_and_huge"), (0, 0)),
]
COUNTS = [2, 9, 10, 11, 19, 20]


def order_id(case):
    w, h, chans, pad = case
    return f"{w}x{h}-" + "-".join(chans)


def order_case(case):
    """(points (h, w, 3) float32, mask (h, w) uint8 of ones) of one entry of ORDER_CASES."""
    w, h, chans, _ = case
    n = w * h
    cols = []
    for i, name in enumerate(chans):
        rng = np.random.default_rng([w, h, i, sum(name.encode())])
        cols.append(rng.permutation(CHANNELS[name](n, rng)))
    return np.stack(cols, -1).reshape(h, w, 3).astype(f32), np.ones((h, w), np.uint8)


def counts_case(n, w=64, h=48):
    """n valid masked points with distinct coordinates among w * h pixels of other values; three pixels more are
    inside the mask but hold the invalid point (0, 0, 0)."""
    rng = np.random.default_rng([n, w, h])
    points = np.stack([rng.permutation(np.linspace(lo, hi, w * h)) for lo, hi in ((-2, 1), (0.5, 4), (-9, -3))],
                      -1).reshape(h, w, 3).astype(f32)
    mask = np.zeros(h * w, np.uint8)
    where = rng.permutation(h * w)[:n + 3]
    mask[where] = rng.choice([1, 7, 255], n + 3)
    points.reshape(-1, 3)[where[n:]] = 0
    return points, mask.reshape(h, w)


def cloud_image(w, h, seed, keep=0.6):
    """Random camera-frame points in front of a camera with a random mask; some pixels hold the invalid point."""
    rng = np.random.default_rng([seed, w, h])
    points = (rng.uniform(-0.35, 0.35, (h, w, 3)) + [0.05, -0.02, 1.2]).astype(f32)
    points[rng.uniform(size=(h, w)) < 0.05] = 0
    mask = (rng.uniform(size=(h, w)) < keep).astype(np.uint8) * rng.choice([1, 255], (h, w)).astype(np.uint8)
    return points, mask


ROTATED = (161, 77, rot([0.3, 1, 0.1], 25).astype(f32), np.array([0.4, -2.0, 0.3], f32))


# ---- object extent: volumes whose vertex cloud joins the points ------------------------------------------------------

EXTENT_RES = [(33, 31, 35), (30, 22, 18), (2, 2, 2), (2, 9, 3)]
# (name, resolution, with the foreground mask, image size)
EXTENT_CASES = [(f"{'x'.join(map(str, r))}-{'fg' if fg else 'plain'}", r, fg, (64, 48) if r[0] > 2 else (5, 3))
                for r in EXTENT_RES for fg in (False, True)]
EXTENT_CASES += [("empty_image_mask", (30, 22, 18), True, (64, 48)), ("no_crossing", (30, 22, 18), False, (64, 48))]
EXTENT_VOXEL = 0.02


def extent_volume(res):
    """(tsdf, weights, fg): a tilted plane (a sphere for (30, 22, 18)) in units of a 3-voxel truncation distance; near
    the surface some values are exactly 0 and some within 1e-5 of 0; a random tenth of the voxels has weight 0, another
    tenth is outside the foreground mask."""
    nx, ny, nz = res
    rng = np.random.default_rng([nx, ny, nz])
    if res == (2, 2, 2):  # by hand: every edge kind on the one cube
        t = np.array([[[-0.5, 0.0], [0.4, -5e-6]], [[5e-6, 0.7], [-0.2, 0.3]]], f32)
        return t, np.full(t.shape, 3, f32), np.array([[[1, 255], [128, 2]], [[255, 255], [7, 255]]], np.uint8)
    z, y, x = np.meshgrid(np.arange(nz) - (nz - 1) / 2, np.arange(ny) - (ny - 1) / 2, np.arange(nx) - (nx - 1) / 2,
                          indexing="ij")
    if res == (30, 22, 18):
        d = np.sqrt((x - 1.3) ** 2 + (y + 0.4) ** 2 + (z - 0.2) ** 2) - 6.7
    else:
        d = 0.5 * x + 0.3 * y + 0.8 * z + 0.21
    t = np.clip(d / 3, -1, 1).astype(f32)
    small = t.size < 100  # too few cubes to lose some at random: the first and the last y plane take the zeros
    near = np.flatnonzero((np.abs(t) < 0.5).reshape(-1) & (~small | ((y > y.min()) & (y < y.max())).reshape(-1)))
    k = max(2, len(near) // 30)
    pick = rng.permutation(near)[:2 * k]
    t.reshape(-1)[pick[:k]] = 0
    t.reshape(-1)[pick[k:]] = np.where(np.arange(k) % 2 == 1, f32(5e-6), f32(-5e-6))
    w = rng.uniform(1, 64, t.shape).astype(f32)
    lose = np.flatnonzero((y == y.max()).reshape(-1)) if small else np.arange(t.size)
    w.reshape(-1)[rng.permutation(lose)[:t.size // 10]] = 0
    fg = rng.choice([1, 128, 255], t.shape).astype(np.uint8)
    lose = np.flatnonzero((y == y.min()).reshape(-1)) if small else np.arange(t.size)
    fg.reshape(-1)[rng.permutation(lose)[:t.size // 10]] = 0
    return t, w, fg


def extent_case(case):
    name, res, with_fg, (w, h) = case
    t, wt, fg = extent_volume(res)
    points, mask = cloud_image(w, h, seed=sum(res))
    if name == "empty_image_mask":
        mask[:] = 0
    if name == "no_crossing":
        t = np.abs(t) + f32(0.01)
    R = rot([1, 0.2, -0.4], 40).astype(f32)
    tr = (-(R.astype(np.float64) @ [0.05, -0.02, 1.2])).astype(f32)  # the points land round the volume's centre
    return dict(points=points, mask=mask, R=R, t=tr, tsdf=t, weights=wt, fg=fg if with_fg else None, voxel=EXTENT_VOXEL)


def extent_reference(c):
    """(count, p10, p90): mesh_cloud plus the transformed masked points, sorted."""
    valid = (c["mask"] != 0) & np.any(c["points"] != 0, axis=2)
    allp = np.concatenate([f32_transform(c["R"], c["t"], c["points"][valid]),
                           mesh_cloud(c["tsdf"], c["weights"], c["fg"], c["voxel"])])
    s = np.sort(allp, axis=0)
    n = len(allp)
    return n, s[int(f32(n) * f32(.1))], s[int(f32(n) * f32(.9))]


# ---- association mass --------------------------------------------------------------------------------------------------
# Weights are k / 4096 with integer k in [0, 4096]: every partial sum of at most 2^20 of them is a multiple of 2^-12
# below 2^20, which a double holds exactly, so the sum does not depend on the order it is taken in.

MASS_BLOCKS, MASS_LANES = 240, 256  # workgroups of k_mask_mass (each a band of ceil(h / 240) rows), lanes along a row
MASS_SIZES = [(300, 7), (257, 241), (64, 480), (33, 481), (1, 1), (640, 480)]
MASS_PADS = (2, 5, 1)  # padding columns of the object mask, the match mask, the weights


def mass_bands(h):
    """(rows per band, bands that hold a row, rows of the last of them)."""
    rows = -(-h // MASS_BLOCKS)
    used = -(-h // rows)
    return rows, used, h - (used - 1) * rows


def mass_case(w, h):
    """(object mask, match mask, k): the weights are k / 4096.  The last row and the last column hold inside pixels
    of the object mask itself."""
    rng = np.random.default_rng([w, h, 77])
    seg = (rng.uniform(size=(h, w)) < 0.3).astype(np.uint8)
    seg[-1, :] |= (rng.uniform(size=w) < 0.5).astype(np.uint8)
    seg[:, -1] |= (rng.uniform(size=h) < 0.5).astype(np.uint8)
    seg[-1, -1] = seg[0, -1] = seg[-1, 0] = 1
    match = (rng.uniform(size=(h, w)) < 0.15).astype(np.uint8) * rng.choice([7, 255], (h, w)).astype(np.uint8)
    k = rng.integers(0, 4097, (h, w))
    return seg, match, k


def weights_of(k):
    return (k.astype(np.float64) / 4096).astype(f32)


def mass_reference(seg, match, k):
    """(count, sum) in integer arithmetic."""
    inside = (seg != 0) if match is None else ((seg != 0) | (match != 0))
    return int(inside.sum()), np.float64(int(k[inside].astype(np.int64).sum())) / np.float64(4096)


BATCH = dict(w=257, h=241, n=33, nall=35, thresh=0.25, with_match=(0, 5, 31, 32), tie=3, light=4, invisible=7,
             ex_low=32)


def batched_case():
    """33 objects (a second chunk of one) at 257 x 241: hit masks, k, match masks (None but for 4 objects, of both
    chunks), and the verdict inputs.  Object 3's weights are all 1/4 = the threshold: thr * count == sum, a tie, kept.
    Object 4 is the same with one pixel a step lighter: deleted."""
    b = BATCH
    w, h, n = b["w"], b["h"], b["n"]
    rng = np.random.default_rng(33)
    segs, ks, matches = [], [], []
    for i in range(n):
        seg = (rng.uniform(size=(h, w)) < 0.1 + 0.02 * i).astype(np.uint8)
        seg[-1, -1] = 1
        k = rng.integers(0, 4097, (h, w))
        if i in (b["tie"], b["light"]):
            k[:] = 1024
        if i == b["light"]:
            k[-1, -1] = 1023
        if i % 5 == 1:
            k = k // 8  # light objects among the others
        segs.append(seg)
        ks.append(k)
        matches.append((rng.uniform(size=(h, w)) < 0.1).astype(np.uint8) * 255 if i in b["with_match"] else None)
    visible = np.ones(n, np.int32)
    visible[b["invisible"]] = 0
    ex_low = np.zeros(n, np.uint8)
    ex_low[b["ex_low"]] = 1
    list_pos = rng.permutation(b["nall"])[:n]
    return dict(segs=segs, ks=ks, matches=matches, visible=visible, ex_low=ex_low, list_pos=list_pos)


def batched_reference(c):
    """(counts, sums, verdicts by list position, padded to a multiple of 4) -- cleanUpObjs' rule (EMFusion.cpp:936-951):
    deleted if its existence is low, or it is invisible, or float(thr * float(count)) > sum."""
    b = BATCH
    ref = [mass_reference(s, m, k) for s, m, k in zip(c["segs"], c["matches"], c["ks"])]
    verdict = np.zeros((b["nall"] + 3) // 4 * 4, f32)
    for i, (cnt, total) in enumerate(ref):
        light = np.float64(f32(b["thresh"]) * f32(cnt)) > total
        verdict[c["list_pos"][i]] = 1 if (c["ex_low"][i] or not c["visible"][i] or light) else 0
    return np.array([r[0] for r in ref], np.uint32), np.array([r[1] for r in ref], np.float64), verdict


# ---- overlap, carving, hiding ------------------------------------------------------------------------------------------

IMAGE_SIZES = [(1, 1), (5, 3), (257, 3), (161, 77), (640, 480)]
OVERLAP_KINDS = ["mixed", "one_region", "empty_mask"]


def overlap_case(w, h, kind):
    """(mask, model segmentation): ids 1, 2, 254, 255 and mask values 1, 200, 255."""
    rng = np.random.default_rng([w, h, 5])
    model = rng.choice([0, 1, 2, 254, 255], (h, w), p=[0.3, 0.2, 0.2, 0.1, 0.2]).astype(np.uint8)
    seg = rng.choice([0, 1, 200, 255], (h, w), p=[0.55, 0.15, 0.15, 0.15]).astype(np.uint8)
    model[-1, -1], seg[-1, -1] = 255, 200
    if kind == "one_region":  # every pixel id 255 and inside the mask: all of the image on one LDS counter
        model[:] = 255
        seg[seg == 0] = 1
    elif kind == "empty_mask":
        seg[:] = 0
    return seg, model


def overlap_reference(seg, model):
    """(mask pixels, intersection[256], area[256]) by counting; entry 0 (the background) is not counted."""
    inter = np.bincount(model[seg != 0].reshape(-1), minlength=256)
    area = np.bincount(model.reshape(-1), minlength=256)
    inter[0] = area[0] = 0
    return int((seg != 0).sum()), inter.astype(np.uint32), area.astype(np.uint32)


CARVE_KINDS = ["mixed", "everything", "nothing", "empty_mask"]


def carve_case(w, h, kind, obj_id):
    """(mask, model segmentation, match mask)."""
    rng = np.random.default_rng([w, h, obj_id, 2])
    other = 255 if obj_id == 1 else 1
    seg = rng.choice([0, 3, 255], (h, w), p=[0.4, 0.3, 0.3]).astype(np.uint8)
    model = rng.choice([0, obj_id, other, 2], (h, w)).astype(np.uint8)
    match = (rng.uniform(size=(h, w)) < 0.2).astype(np.uint8) * rng.choice([1, 255], (h, w)).astype(np.uint8)
    seg[-1, -1], model[-1, -1] = 3, obj_id
    if kind == "everything":
        seg[seg == 0] = 1
        model[:] = obj_id
    elif kind == "nothing":
        seg[seg == 0] = 1
        model[model == obj_id] = other
        match[:] = 0
    elif kind == "empty_mask":
        seg[:] = 0
    return seg, model, match


def carve_reference(seg, model, match, obj_id):
    """(carved mask, pixels before, pixels after)."""
    taken = (model == obj_id) if match is None else ((model == obj_id) | (match != 0))
    want = np.where(taken, 0, seg).astype(np.uint8)
    return want, int((seg != 0).sum()), int((want != 0).sum())


HIDE = dict(w=161, h=77, label=7, absent=9, pads=(1, 2, 3, 4, 5))


def hide_case():
    """segmentation, vertices, normals, background vertices, background normals; NaN normals inside and outside the
    label, NaN in the background's images too."""
    w, h = HIDE["w"], HIDE["h"]
    rng = np.random.default_rng(12)
    seg = rng.choice([0, 1, 2, 7, 255], (h, w)).astype(np.uint8)
    seg[0, 0] = seg[-1, -1] = 7
    imgs = [rng.standard_normal((h, w, 3)).astype(f32) for _ in range(4)]
    for im in imgs[1:]:
        im[rng.uniform(size=(h, w)) < 0.2] = np.nan
    return [seg] + imgs


def hide_reference(seg, vert, nrm, bg_vert, bg_nrm, label):
    """EMFusion::render's ignore_person (EMFusion.cpp:139-150): compare, setTo(0), two masked copies."""
    hit = seg == label
    return (np.where(hit, 0, seg).astype(np.uint8), np.where(hit[..., None], bg_vert, vert),
            np.where(hit[..., None], bg_nrm, nrm))
