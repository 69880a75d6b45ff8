"""Restatement of include/emf_hip.h "Object shapes"  for the tests.

Volumes are (nz, ny, nx) arrays, a voxel is v = (x, y, z).  What is measured is the OBSERVED SOLID BAND of a model, not
its body: a TSDF observes a band around the surface, the interior has weight 0.

  solid(v)     weights[v] > 0 and (no mask or mask[v] != 0) and not (tsdf[v] > 0)
  observed(v)  weights[v] > 0
  faces        per solid voxel and face neighbour n inside the volume: FREE if weights[n] > 0 and tsdf[n] > 0,
               UNKNOWN if not (weights[n] > 0)

moments() states the integer record from boolean masks, integer index grids and shifted slices; moments_loop() is a
plain Python loop over the voxels.  extents() does every float32 operation explicitly, in the header's order, and takes
minimum and maximum on the order-preserving u32 keys.  frame() uses Python ints for the 128-bit numerator and Python
floats (IEEE float64, one operation per expression) for the cyclic Jacobi; box() is the float64 box of the header,
element by element (no matrix product of a library)."""
import math

import numpy as np

MOMENTS = np.dtype([("solid", "<u8"), ("observed", "<u8"), ("sum", "<u8", 3), ("sum2", "<u8", 6), ("faces_free", "<u8"),
                    ("faces_unknown", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)])
AXES = np.dtype([("A", "<f4", 9), ("c", "<f4", 3)])
EXTENTS = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3)])
FRAME = np.dtype([("valid", "<i4"), ("reserved", "<i4"), ("centroid", "<f8", 3), ("covariance", "<f8", 6),
                  ("eigenvalues", "<f8", 3), ("axes", "<f8", 9), ("f32", AXES)])
BOX = np.dtype([("center_vox", "<f8", 3), ("half_vox", "<f8", 3), ("completeness", "<f8"), ("center_obj", "<f8", 3),
                ("half_m", "<f8", 3), ("corners_obj", "<f8", 24), ("center_world", "<f8", 3), ("axes_world", "<f8", 9),
                ("corners_world", "<f8", 24)])
SWEEPS = 8  # EMF_SHAPE_JACOBI_SWEEPS
PAIRS2 = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]  # the order of sum2 and of the covariance

SHAPES = [(1, 1, 1), (5, 3, 2), (7, 9, 11), (16, 16, 16), (33, 17, 9), (64, 8, 8), (40, 24, 20)]  # (nx, ny, nz)
CONTENTS = ["unobserved", "all_solid", "half_shell", "random", "gated_block", "corner"]


# ---- the definition ------------------------------------------------------------------------------------------------

def solid_mask(tsdf, weights, fg=None):
    with np.errstate(invalid="ignore"):
        s = (weights > 0) & ~(tsdf > 0)
    return s if fg is None else s & (fg != 0)


def observed_mask(weights):
    with np.errstate(invalid="ignore"):
        return weights > 0


def moments(tsdf, weights, fg=None):
    """The MOMENTS record of one volume (a 0-d array of the dtype)."""
    nz, ny, nx = tsdf.shape
    solid = solid_mask(tsdf, weights, fg)
    obs = observed_mask(weights)
    with np.errstate(invalid="ignore"):
        free = obs & (tsdf > 0)
    unknown = ~obs
    z, y, x = np.nonzero(solid)
    x, y, z = x.astype(object), y.astype(object), z.astype(object)  # Python ints: no width to overflow
    out = np.zeros((), MOMENTS)
    out["solid"] = len(x)
    out["observed"] = int(obs.sum())
    c = (x, y, z)
    out["sum"] = [int(sum(c[j])) for j in range(3)]
    out["sum2"] = [int(sum(c[j] * c[k])) for j, k in PAIRS2]
    ff = fu = 0
    for axis in range(3):  # shifted slices: the neighbour one step down and one step up this axis
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        ff += int((solid[lo] & free[hi]).sum()) + int((solid[hi] & free[lo]).sum())
        fu += int((solid[lo] & unknown[hi]).sum()) + int((solid[hi] & unknown[lo]).sum())
    out["faces_free"], out["faces_unknown"] = ff, fu
    if len(x):
        out["lo"] = [int(min(c[j])) for j in range(3)]
        out["hi"] = [int(max(c[j])) for j in range(3)]
    else:
        out["lo"], out["hi"] = (nx, ny, nz), (-1, -1, -1)
    return out


def moments_loop(tsdf, weights, fg=None):
    """The same record by a plain loop over the voxels and their six neighbours."""
    nz, ny, nx = tsdf.shape
    n = (nx, ny, nz)
    solid = observed = ff = fu = 0
    s, s2 = [0, 0, 0], [0] * 6
    lo, hi = [nx, ny, nz], [-1, -1, -1]
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                w, t = float(weights[z, y, x]), float(tsdf[z, y, x])
                if not w > 0:
                    continue
                observed += 1
                if (fg is not None and fg[z, y, x] == 0) or t > 0:
                    continue
                solid += 1
                v = (x, y, z)
                for j in range(3):
                    s[j] += v[j]
                    lo[j], hi[j] = min(lo[j], v[j]), max(hi[j], v[j])
                for i, (j, k) in enumerate(PAIRS2):
                    s2[i] += v[j] * v[k]
                for axis in range(3):
                    for step in (-1, 1):
                        q = list(v)
                        q[axis] += step
                        if not 0 <= q[axis] < n[axis]:
                            continue
                        wn, tn = float(weights[q[2], q[1], q[0]]), float(tsdf[q[2], q[1], q[0]])
                        if wn > 0:
                            ff += tn > 0
                        else:
                            fu += 1
    out = np.zeros((), MOMENTS)
    out["solid"], out["observed"], out["sum"], out["sum2"] = solid, observed, s, s2
    out["faces_free"], out["faces_unknown"], out["lo"], out["hi"] = ff, fu, lo, hi
    return out


def float_keys(e):
    """The order-preserving map of f32 bits to u32."""
    b = np.ascontiguousarray(e, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b ^ np.uint32(0x80000000))


def key_floats(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def projections(tsdf, weights, fg, axes):
    """e_k of every solid voxel, (n, 3) f32: every line a single float32 operation, rows summed left to right."""
    z, y, x = np.nonzero(solid_mask(tsdf, weights, fg))
    A = np.asarray(axes["A"], np.float32).reshape(3, 3)
    c = np.asarray(axes["c"], np.float32)
    p = [x.astype(np.float32) - c[0], y.astype(np.float32) - c[1], z.astype(np.float32) - c[2]]
    e = np.empty((len(x), 3), np.float32)
    with np.errstate(all="ignore"):
        for k in range(3):
            a0, a1, a2 = A[k, 0] * p[0], A[k, 1] * p[1], A[k, 2] * p[2]
            e[:, k] = (a0 + a1) + a2
    return e


def extents(tsdf, weights, fg, axes):
    """The EXTENTS record of one volume along `axes` (an AXES record)."""
    e = projections(tsdf, weights, fg, axes)
    out = np.zeros((), EXTENTS)
    if len(e) == 0:
        out["lo"], out["hi"] = np.inf, -np.inf
        return out
    keys = float_keys(e)
    out["lo"] = key_floats(keys.min(axis=0))
    out["hi"] = key_floats(keys.max(axis=0))
    return out


# ---- the frame -----------------------------------------------------------------------------------------------------

def covariance(mom):
    """(m, C): centroid and covariance in the order of PAIRS2, Python floats."""
    n = int(mom["solid"])
    s = [int(v) for v in mom["sum"]]
    s2 = [int(v) for v in mom["sum2"]]
    m = [float(s[j]) / float(n) for j in range(3)]
    den = float(n) * float(n)
    C = [float(n * s2[i] - s[j] * s[k]) / den for i, (j, k) in enumerate(PAIRS2)]  # int -> float rounds once, to even
    return m, C


def jacobi_sweep(S, V):
    """One sweep over (0,1), (0,2), (1,2), in place on the 3 x 3 lists S and V."""
    for p, q in ((0, 1), (0, 2), (1, 2)):
        apq = S[p][q]
        if apq == 0.0:
            continue
        theta = (S[q][q] - S[p][p]) / (2.0 * apq)
        t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
        if theta < 0.0:
            t = -t
        c = 1.0 / math.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        S[p][p] = S[p][p] - h
        S[q][q] = S[q][q] + h
        S[p][q] = S[q][p] = 0.0
        r = 3 - p - q
        srp, srq = S[r][p], S[r][q]
        S[r][p] = S[p][r] = c * srp - s * srq
        S[r][q] = S[q][r] = s * srp + c * srq
        for i in range(3):
            vip, viq = V[i][p], V[i][q]
            V[i][p] = c * vip - s * viq
            V[i][q] = s * vip + c * viq


def jacobi(C, sweeps=SWEEPS):
    S = [[C[0], C[3], C[4]], [C[3], C[1], C[5]], [C[4], C[5], C[2]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(sweeps):
        jacobi_sweep(S, V)
    return S, V


def frame(mom, sweeps=SWEEPS):
    """The FRAME record of a MOMENTS record."""
    out = np.zeros((), FRAME)
    if int(mom["solid"]) == 0:
        return out
    m, C = covariance(mom)
    S, V = jacobi(C, sweeps)
    eig = [S[0][0], S[1][1], S[2][2]]
    order = sorted(range(3), key=lambda j: (-eig[j], j))  # descending, ties to the lower index
    axes = [[V[i][order[k]] for i in range(3)] for k in range(3)]
    for k in (0, 1):
        big = 0
        for i in (1, 2):
            if abs(axes[k][i]) > abs(axes[k][big]):
                big = i
        if axes[k][big] < 0.0:
            axes[k] = [-v for v in axes[k]]
    a, b = axes[0], axes[1]
    axes[2] = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    out["valid"] = 1
    out["centroid"], out["covariance"] = m, C
    out["eigenvalues"] = [eig[j] for j in order]
    out["axes"] = [v for row in axes for v in row]
    out["f32"]["A"] = np.asarray(out["axes"], np.float64).astype(np.float32)
    out["f32"]["c"] = np.asarray(m, np.float64).astype(np.float32)
    return out


def sweeps_to_settle(mom, limit=64):
    """The smallest count of sweeps after which another sweep changes no bit of S or V."""
    _, C = covariance(mom)
    S, V = jacobi(C, 0)
    for k in range(limit):
        before = repr((S, V))
        jacobi_sweep(S, V)
        if repr((S, V)) == before:
            return k
    return limit


def box(mom, fr, ext, res, voxel_size, R, t):
    """The BOX record: float64, one operation per expression, sums left to right.  R (9,), t (3,): the model's pose,
    f32 taken to float64."""
    out = np.zeros((), BOX)
    A = [float(v) for v in fr["axes"]]
    m = [float(v) for v in fr["centroid"]]
    lo, hi = [float(v) for v in ext["lo"]], [float(v) for v in ext["hi"]]
    R, t = [float(np.float32(v)) for v in np.ravel(R)], [float(np.float32(v)) for v in np.ravel(t)]
    vs = float(np.float32(voxel_size))
    with np.errstate(all="ignore"):
        mid = [np.float64(lo[k]) + np.float64(hi[k]) for k in range(3)]
        mid = [float(v / 2.0) for v in mid]
        center = []
        for j in range(3):
            s = A[j] * mid[0]
            s = s + A[3 + j] * mid[1]
            s = s + A[6 + j] * mid[2]
            center.append(m[j] + s)
        half = []
        for k in range(3):
            w = abs(A[3 * k]) + abs(A[3 * k + 1])
            w = w + abs(A[3 * k + 2])
            half.append(float((np.float64(hi[k]) - np.float64(lo[k])) / 2.0 + w / 2.0))
        ff, fu = float(int(mom["faces_free"])), float(int(mom["faces_unknown"]))
        comp = ff / (ff + fu) if ff + fu != 0.0 else float("nan")
        cobj = [float(np.float64(center[j] - (float(int(res[j])) - 1.0) / 2.0) * vs) for j in range(3)]
        hm = [float(np.float64(half[k]) * vs) for k in range(3)]

        def to_world(p):
            w = []
            for i in range(3):
                s = np.float64(R[3 * i]) * p[0]
                s = s + np.float64(R[3 * i + 1]) * p[1]
                s = s + np.float64(R[3 * i + 2]) * p[2]
                w.append(float(s + t[i]))
            return w

        corners, wcorners = [], []
        for i in range(8):
            h = [np.float64(hm[k] if (i >> k) & 1 else -hm[k]) for k in range(3)]
            p = []
            for j in range(3):
                s = np.float64(cobj[j]) + h[0] * A[j]
                s = s + h[1] * A[3 + j]
                s = s + h[2] * A[6 + j]
                p.append(float(s))
            corners += p
            wcorners += to_world(p)
        waxes = []
        for k in range(3):
            for i in range(3):
                s = np.float64(R[3 * i]) * A[3 * k]
                s = s + np.float64(R[3 * i + 1]) * A[3 * k + 1]
                s = s + np.float64(R[3 * i + 2]) * A[3 * k + 2]
                waxes.append(float(s))
    out["center_vox"], out["half_vox"], out["completeness"] = center, half, comp
    out["center_obj"], out["half_m"], out["corners_obj"] = cobj, hm, corners
    out["center_world"], out["axes_world"], out["corners_world"] = to_world(cobj), waxes, wcorners
    return out


# ---- fixtures ------------------------------------------------------------------------------------------------------

def volume(shape, content):
    """(tsdf f32, weights f32, fg u8) as (nz, ny, nx) arrays for shape = (nx, ny, nz).  fg is the mask that belongs to
    the content ("gated_block") or a seeded random one; the tests run every case with it and without."""
    nx, ny, nz = shape
    rng = np.random.default_rng([0x5B, CONTENTS.index(content), *shape])
    dims = (nz, ny, nx)
    fg = rng.choice(np.array([0, 1, 1, 2, 255], np.uint8), dims)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if content == "unobserved":
        tsdf = rng.uniform(-1, 1, dims).astype(np.float32)
        weights = np.zeros(dims, np.float32)
    elif content == "all_solid":
        tsdf = np.full(dims, -0.5, np.float32)
        weights = np.full(dims, 3.0, np.float32)
    elif content == "half_shell":  # a sphere's shell seen from one side: weights positive on a half-space only
        c = np.array([(nx - 1) / 2 + 0.3, (ny - 1) / 2 - 0.2, (nz - 1) / 2 + 0.1])
        r = max(min(shape) / 3, 0.6)
        d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r
        tsdf = np.clip(d / 2.0, -1, 1).astype(np.float32)
        seen = (np.abs(d) < 2.0) & (x + 0.5 * y <= c[0] + 0.5 * c[1])
        weights = np.where(seen, 4.0, 0.0).astype(np.float32)
    elif content == "random":  # random signs with NaN and -0.0 tsdf and with zero, negative and NaN weights
        tsdf = rng.choice(np.array([-1.0, -0.25, -0.0, 0.0, 0.5, 1.0, np.nan], np.float32), dims)
        weights = rng.choice(np.array([0.0, 0.0, -1.0, np.nan, 1.0, 2.5, 64.0], np.float32), dims)
    elif content == "gated_block":  # a solid block in free space, the mask gates half of it
        tsdf = np.full(dims, 0.75, np.float32)
        weights = np.ones(dims, np.float32)
        inside = (x >= nx // 4) & (x <= nx - 1 - nx // 4) & (y >= ny // 4) & (z >= nz // 4)
        tsdf[inside] = -0.75
        fg = np.where(inside & ((x + y + z) % 2 == 0), 1, 0).astype(np.uint8)
    elif content == "corner":  # a single solid voxel in the far corner, unknown around it
        tsdf = np.zeros(dims, np.float32)
        weights = np.zeros(dims, np.float32)
        weights[-1, -1, -1] = 1.0
        fg = np.zeros(dims, np.uint8)
        fg[-1, -1, -1] = 7
    else:
        raise ValueError(content)
    return np.ascontiguousarray(tsdf), np.ascontiguousarray(weights), np.ascontiguousarray(fg)


def cases():
    """Every shape x content x (with mask, without)."""
    for shape in SHAPES:
        for content in CONTENTS:
            tsdf, weights, fg = volume(shape, content)
            for masked in (True, False):
                yield f"{shape}-{content}-{'fg' if masked else 'nofg'}", tsdf, weights, fg if masked else None


def skew_axes(shape):
    """A frame that is no frame of the volume: a rotation about a skew axis with a centre off the lattice, as AXES."""
    a = np.array([0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(0.7) * K + (1 - math.cos(0.7)) * (K @ K)
    out = np.zeros((), AXES)
    out["A"] = R.astype(np.float32).reshape(-1)
    out["c"] = [(shape[0] - 1) / 3, (shape[1] - 1) / 2 + 0.25, (shape[2] - 1) / 1.5]
    return out


def axes_for(mom, shape):
    """The axes the extents pass of a model gets: its frame's, or the skew ones for a model without a solid voxel."""
    fr = frame(mom)
    return fr["f32"].copy() if int(fr["valid"]) else skew_axes(shape)
