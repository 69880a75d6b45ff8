"""Restatement of include/emf_hip.h "Voxel rays"  for the tests.

The query runs over a box of class bytes in (z, y, x) order; what lies outside the box does not exist.

The walk.  A ray goes from voxel a to voxel b (x, y, z).  d_k = |b_k - a_k|, s_k = sign(b_k - a_k).  It makes exactly
n = d_x + d_y + d_z face steps v_1 .. v_n, v_n = b.  With i_k the steps already made along axis k, the next step goes
along the axis that still has steps left and has the smallest crossing parameter (2 i_k + 1) / (2 d_k), compared by
cross-multiplication in integers; ties go to the lower axis index.  The walk is NOT symmetric in a and b.
Stated twice: walk_steps is that rule, step by step; walk_sorted sorts all crossings by (parameter as an exact
fraction, axis).

What stops a ray.  a is never tested.  v passes if it lies in the box, (1 << class[v]) & pass_mask != 0 (a class byte
above 2 is in no mask) and, where d2 is given with min_d2 > 0, d2[v] >= min_d2.  The first voxel that does not pass ends
the ray.  Records: RESULT (stop, steps, counted, status, weighted) and GROUP (counted, weighted, reached, blocked, left,
invalid) as in the header.  Everything is an integer, so the tests compare bytes.

The view targets are float64 in the operation order of include/emf_fusion.h emf_fusion_view_ray_targets, element by
element (no matrix product of a library), and the shortcut greedy is that of emf_fusion_plan_shortcut."""
import numpy as np

from tests import plan_reference as pl

FREE, OCCUPIED, UNKNOWN = 0, 1, 2
FAR = 0x7fffffff
NONE = -1
MAX_DELTA = 4095
REACHED, BLOCKED, LEFT, OUTSIDE, INVALID = 0, 1, 2, 3, 4
RESULT = np.dtype([("stop", "<i4"), ("steps", "<i4"), ("counted", "<u4"), ("status", "<u4"), ("weighted", "<u8")])
GROUP = np.dtype([("counted", "<u8"), ("weighted", "<u8"), ("reached", "<u4"), ("blocked", "<u4"), ("left", "<u4"),
                  ("invalid", "<u4")])

SHAPES = [(1, 1, 1), (1, 1, 65), (3, 5, 2), (8, 8, 32), (9, 17, 65), (19, 21, 70), (1, 2, 2048)]  # (nz, ny, nx)
CONTENTS = pl.CONTENTS + ["sparse"]
COUNTS = [0, 1, 63, 64, 65, 129, 257]  # 129: a third wave with one ray (tests/test_rays_reference_cpu.py has the run edges)
GROUPS = [1, 3, 64, 100]


def class_field(shape, content):
    """u8 (nz, ny, nx): the contents of the plan's restatement, and "sparse": a few per cent occupied, some unknown,
    some bytes of 3 in free space."""
    if content != "sparse":
        return pl.class_field(shape, content)
    rng = np.random.default_rng([0x5A, *shape])
    return rng.choice(np.array([FREE] * 45 + [OCCUPIED] * 2 + [UNKNOWN] * 2 + [3], np.uint8), shape)


def walk_steps(a, b):
    """The voxels v_1 .. v_n of the ray a -> b, (n, 3) i64, by the step rule."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    d = [abs(b[k] - a[k]) for k in range(3)]
    s = [(b[k] > a[k]) - (b[k] < a[k]) for k in range(3)]
    i, v, out = [0, 0, 0], list(a), []
    for _ in range(sum(d)):
        best = -1
        for k in range(3):
            if i[k] >= d[k]:
                continue
            # strictly smaller wins: at a tie the lower axis, which came first, stays
            if best < 0 or (2 * i[k] + 1) * d[best] < (2 * i[best] + 1) * d[k]:
                best = k
        i[best] += 1
        v[best] += s[best]
        out.append(tuple(v))
    return np.array(out, np.int64).reshape(-1, 3)


def walk_sorted(a, b):
    """The same voxels from all crossings sorted by (parameter as an exact fraction, axis)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    d, s = np.abs(b - a), np.sign(b - a)
    # (2 i + 1) / (2 d_k) on the common denominator 2 * (product of the non-zero d): all integers, below 2^51
    prod = int(np.prod(np.where(d > 0, d, 1), dtype=object))
    key, axis = [], []
    for k in range(3):
        if d[k]:
            key.append((2 * np.arange(int(d[k]), dtype=np.int64) + 1) * (prod // int(d[k])))
            axis.append(np.full(int(d[k]), k, np.int64))
    if not key:
        return np.zeros((0, 3), np.int64)
    key, axis = np.concatenate(key), np.concatenate(axis)
    order = np.lexsort((axis, key))
    moves = np.zeros((len(order), 3), np.int64)
    moves[np.arange(len(order)), axis[order]] = s[axis[order]]
    return a + np.cumsum(moves, axis=0)


def cast_one(classes, a, b, d2=None, min_d2=0, pass_mask=1, count_mask=0):
    """(stop, steps, counted, status, weighted) of one ray."""
    nz, ny, nx = classes.shape
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    size = np.array([nx, ny, nz], np.int64)
    if ((a < 0) | (a >= size)).any():
        return NONE, 0, 0, OUTSIDE, 0
    if (np.abs(b - a) > MAX_DELTA).any():
        return NONE, 0, 0, INVALID, 0
    v = walk_sorted(a, b)
    n = len(v)
    if n == 0:
        return NONE, 0, 0, REACHED, 0
    inside = ((v >= 0) & (v < size)).all(axis=1)
    w = np.where(inside[:, None], v, 0)
    c = classes[w[:, 2], w[:, 1], w[:, 0]].astype(np.int64)
    bit = np.where(c <= 2, 1 << np.minimum(c, 2), 0)
    ok = inside & ((bit & pass_mask) != 0)
    if d2 is not None and min_d2 > 0:
        ok &= d2[w[:, 2], w[:, 1], w[:, 0]].astype(np.int64) >= min_d2
    steps = n if ok.all() else int(np.argmin(ok))
    counts = (bit[:steps] & count_mask) != 0
    r2 = ((v[:steps] - a) ** 2).sum(axis=1)
    counted, weighted = int(counts.sum()), int(r2[counts].sum())
    if steps == n:
        return NONE, steps, counted, REACHED, weighted
    if not inside[steps]:
        return NONE, steps, counted, LEFT, weighted
    x, y, z = (int(q) for q in v[steps])
    return (z * ny + y) * nx + x, steps, counted, BLOCKED, weighted


def cast(classes, rays_from, rays_to, d2=None, min_d2=0, pass_mask=1, count_mask=0):
    """RESULT records of n rays."""
    f, t = np.asarray(rays_from, np.int64).reshape(-1, 3), np.asarray(rays_to, np.int64).reshape(-1, 3)
    out = np.zeros(len(f), RESULT)
    for k in range(len(f)):
        out[k] = cast_one(classes, f[k], t[k], d2, min_d2, pass_mask, count_mask)
    return out


def group_records(results, group):
    """GROUP records of runs of `group` consecutive rays; the last run may be short."""
    n = len(results)
    out = np.zeros(-(-n // group), GROUP)
    for g in range(len(out)):
        r = results[g * group:(g + 1) * group]
        st = r["status"]
        out[g] = (int(r["counted"].astype(np.uint64).sum()), int(r["weighted"].sum()), int((st == REACHED).sum()),
                  int((st == BLOCKED).sum()), int((st == LEFT).sum()), int((st >= OUTSIDE).sum()))
    return out


def ray_list(shape, classes, pass_mask=1, n_random=300):
    """(from, to), (n, 3) i32 each: rays built by kind, then random ones.  The first two are the full first row, so that
    every group of two or more rays that starts at ray 0 holds both."""
    nz, ny, nx = shape
    cx, cy, cz = c = (nx // 2, ny // 2, nz // 2)
    rays = [((0, 0, 0), (nx - 1, 0, 0))] * 2                      # the full row, twice
    rays.append((c, c))                                           # zero length
    for k, n in enumerate((nx, ny, nz)):                          # each axis in both directions
        for end in (0, n - 1):
            b = list(c)
            b[k] = end
            rays.append((c, tuple(b)))
    m = min(nx, ny, nz) - 1                                       # the full-tie diagonals
    rays += [((0, 0, 0), (m, m, m)), ((m, m, m), (0, 0, 0)), ((nx - 1, 0, nz - 1), (nx - 1 - m, m, nz - 1 - m))]
    mxy, myz, mxz = min(nx, ny) - 1, min(ny, nz) - 1, min(nx, nz) - 1  # two equal
    rays += [((0, 0, 0), (mxy, mxy, 0)), ((0, 0, 0), (0, myz, myz)), ((0, 0, 0), (mxz, 0, mxz)),
             ((0, 0, 0), (mxy, mxy, nz - 1)), ((nx - 1, ny - 1, nz - 1), (nx - 1 - mxy, ny - 1 - mxy, 0)),
             ((0, 0, 0), (nx - 1, myz, myz))]
    rays += [((-1, 0, 0), c), ((nx, cy, cz), c), ((cx, cy, nz), c), ((cx, -7, cz), (cx, -7, cz)),  # origin outside
             ((2 ** 31 - 1, 0, 0), (-2 ** 31, 0, 0))]
    for k, n in enumerate((nx, ny, nz)):                          # target outside on each face
        for end in (-3, n + 2):
            b = list(c)
            b[k] = end
            rays.append((c, tuple(b)))
    rays += [(c, (nx + 5, ny + 3, nz + 1)), (c, (-4, -4, -4)), ((0, 0, 0), (4095, 0, 0)), ((0, 0, 0), (4095, 4095, 4095))]
    rays += [((0, 0, 0), (4096, 0, 0)), (c, (cx, cy - 4096, cz)), (c, (cx, cy, cz + 4096)),   # one d_k above the limit
             ((nx - 1, 0, 0), (-2 ** 31, 2 ** 31 - 1, 0))]
    # blocked at the first step, and a target on a blocking voxel: the first blocking voxels with a neighbour in the box
    c64 = classes.astype(np.int64)
    blocks = np.argwhere((c64 > 2) | (((1 << np.minimum(c64, 2)) & pass_mask) == 0))[:, ::-1]
    for b in blocks[:: max(len(blocks) // 6, 1)][:6]:
        for k, n in enumerate((nx, ny, nz)):
            for s in (-1, 1):
                a = b.copy()
                a[k] -= s
                if 0 <= a[k] < n:
                    far = b.copy()
                    far[k] += 2 * s
                    rays += [(tuple(a), tuple(far)), (tuple(a), tuple(b))]
        rays += [((0, 0, 0), tuple(b)), (c, tuple(b)), ((nx - 1, ny - 1, nz - 1), tuple(b))]
    rng = np.random.default_rng([0xA7, *shape])
    size = np.array([nx, ny, nz])
    f = rng.integers(0, size, (n_random, 3))
    t = rng.integers(-2, size + 2, (n_random, 3))
    short = rng.random(n_random) < 0.5                            # half of them short: near their origin
    t = np.where(short[:, None], f + rng.integers(-9, 10, (n_random, 3)), t)
    fr = np.array([r[0] for r in rays], np.int64).reshape(-1, 3)
    to = np.array([r[1] for r in rays], np.int64).reshape(-1, 3)
    return np.concatenate([fr, f]).astype(np.int32), np.concatenate([to, t]).astype(np.int32)


def view_targets(R, t, K4, grid, range_m, bg_R, bg_t, res, voxel, lo=(0, 0, 0)):
    """(origin (3,) i32, targets (gh, gw, 3) i32, scaled (gh, gw, 3) f64 = dir * (range / voxel) before the rounding):
    float64, every line a single operation, sums left to right."""
    gw, gh = int(grid[0]), int(grid[1])
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    B = np.asarray(bg_R, np.float32).reshape(3, 3).astype(np.float64)
    bt = np.asarray(bg_t, np.float32).reshape(3).astype(np.float64)
    fx, fy, cx, cy = (np.float64(v) for v in K4)
    voxel = np.float64(np.float32(voxel))
    scale = np.float64(range_m) / voxel
    d = [t[j] - bt[j] for j in range(3)]
    origin = np.zeros(3, np.float64)
    for i in range(3):
        q = d[0] * B[0, i]
        q = q + d[1] * B[1, i]
        q = q + d[2] * B[2, i]
        origin[i] = np.rint(q / voxel + (np.float64(res[i]) - 1.0) / 2.0) - np.float64(lo[i])
    origin = np.clip(origin, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    M = np.zeros((3, 3), np.float64)
    for i in range(3):
        for k in range(3):
            m = B[0, i] * R[0, k]
            m = m + B[1, i] * R[1, k]
            m = m + B[2, i] * R[2, k]
            M[i, k] = m
    x = ((np.arange(gw, dtype=np.float64) - cx) / fx)[None, :] + np.zeros((gh, 1))
    y = ((np.arange(gh, dtype=np.float64) - cy) / fy)[:, None] + np.zeros((1, gw))
    s = x * x
    s = s + y * y
    s = s + 1.0
    m = np.sqrt(s)
    c = [x / m, y / m, 1.0 / m]
    scaled = np.zeros((gh, gw, 3), np.float64)
    for a in range(3):
        v = M[a, 0] * c[0]
        v = v + M[a, 1] * c[1]
        v = v + M[a, 2] * c[2]
        scaled[:, :, a] = v * scale
    targets = np.clip(origin.astype(np.float64) + np.rint(scaled), -2.0 ** 31, 2.0 ** 31 - 1)
    return origin.astype(np.int32), targets.astype(np.int64).astype(np.int32), scaled


def shortcut_greedy(k, window, visible):
    """The ascending path indices from 0 to k: from i the largest j in i + 2 .. min(i + window, k) with visible(i, j),
    else i + 1.  Empty for a path without voxels (k < 0)."""
    if k < 0:
        return []
    way, i = [0], 0
    while i < k:
        nxt = i + 1
        for j in range(min(i + window, k), i + 1, -1):
            if visible(i, j):
                nxt = j
                break
        way.append(nxt)
        i = nxt
    return way


def path_visibility(classes, path_vox, window, d2=None, min_d2=0, mask=1):
    """{(i, j): REACHED?} of the rays p_i -> p_j, 2 <= j - i <= window, over a path of box voxels (k + 1, 3)."""
    k = len(path_vox) - 1
    pairs = [(i, j) for i in range(k + 1) for j in range(i + 2, min(i + window, k) + 1)]
    if not pairs:
        return {}
    p = np.asarray(path_vox, np.int64)
    rec = cast(classes, p[[i for i, _ in pairs]], p[[j for _, j in pairs]], d2, min_d2, mask, 0)
    return {pair: bool(s == REACHED) for pair, s in zip(pairs, rec["status"])}
