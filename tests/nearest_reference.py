"""Restatement of the nearest-site index of include/emf_hip.h "Distance field"  for the tests:
nearest[v] is the linear index (z * ny + y) * nx + x of the site nearest to v, the smallest one among equally near
sites, and NONE exactly where d2 is FAR.  Two forms: all pairs (small boxes) and three separable numpy passes that
break every pass's ties toward the smaller coordinate -- np.argmin takes the first minimum.  Plus the tie-heavy
contents the kernels' tie rule has to survive, and the outward scan of the line kernel in a few lines, once as it
has to be for the index (while d * d <= best, the lower side on equality) and once with the stop that is only good
enough for d2 (d * d < best)."""
import numpy as np

from tests import distance_reference as dr

FAR, NONE = dr.FAR, -1
_BIG = 1 << 30  # "no site" inside the passes: _BIG + 2047^2 stays below 2^31
_BLOCK = 1 << 24  # elements of one (n, n, columns) block

TIE_CONTENTS = ["checker", "octa", "two_planes", "row_ends"]
# the smallest shapes at which the ties steer the kernels: rows of 65, 129, 600 (the tie crosses the chunk carry of
# pass x; 601 puts it exactly in the middle of a long row), lines beyond a 64- and a 32-column bundle, an axis of 1
TIE_SHAPES = {
    "checker": [(9, 17, 65), (6, 9, 1), (2, 3, 600), (1, 7, 33)],
    "octa": [(9, 9, 9), (11, 11, 11), (65, 65, 65), (5, 7, 129)],
    "two_planes": [(9, 5, 70), (601, 2, 3), (1101, 2, 20), (1, 4, 5)],
    "row_ends": [(3, 4, 65), (2, 3, 129), (2, 2, 600), (1, 2, 601)],
}


def tie_field(shape, content):
    """bool (nz, ny, nx): the sites of a tie-heavy content."""
    nz, ny, nx = shape
    s = np.zeros(shape, bool)
    if content == "checker":  # every second voxel along each axis
        s[::2, ::2, ::2] = True
    elif content == "octa":  # six sites at the face centres: the centre voxel of an odd cube has all six equally near
        cz, cy, cx = nz // 2, ny // 2, nx // 2
        for z, y, x in ((0, cy, cx), (nz - 1, cy, cx), (cz, 0, cx), (cz, ny - 1, cx), (cz, cy, 0), (cz, cy, nx - 1)):
            s[z, y, x] = True
    elif content == "two_planes":  # with an odd nz the middle plane is equally far from both
        s[0] = True
        s[-1] = True
    else:
        assert content == "row_ends"
        s[:, :, 0] = True
        s[:, :, -1] = True
    return s


def linear_index(shape):
    return np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)


def _capped(d2, nearest, cap):
    d2 = dr.apply_cap(d2, cap)
    return d2, np.where(d2 == FAR, NONE, nearest).astype(np.int32)


def nearest_brute(sites, cap=0):
    """(d2, nearest) from all pairs, argmin over the sites in ascending linear order; small boxes only."""
    assert sites.size <= dr.BRUTE_LIMIT
    if not sites.any():
        return np.full(sites.shape, FAR, np.int32), np.full(sites.shape, NONE, np.int32)
    v = np.stack(np.indices(sites.shape), -1).reshape(-1, 3).astype(np.int64)
    lin = np.flatnonzero(sites.reshape(-1))  # ascending
    s = v[lin]
    d2, near = [], []
    for k in range(0, len(v), 256):
        d = ((v[k:k + 256, None, :] - s[None, :, :]) ** 2).sum(-1)
        a = d.argmin(axis=1)  # the first minimum: the smallest linear index
        d2.append(d[np.arange(len(a)), a])
        near.append(lin[a])
    return _capped(np.concatenate(d2).reshape(sites.shape), np.concatenate(near).reshape(sites.shape), cap)


def _pass(g, idx, axis):
    """out[i] = min_j g[j] + (i - j)^2 along `axis`, the index array taken at the first (smallest) minimising j."""
    n = g.shape[axis]
    gm, im = np.moveaxis(g, axis, 0).reshape(n, -1), np.moveaxis(idx, axis, 0).reshape(n, -1)
    og, oi = np.empty_like(gm), np.empty_like(im)
    i = np.arange(n, dtype=np.int64)
    sq = ((i[:, None] - i[None, :]) ** 2)[:, :, None]  # (i, j, 1)
    step = max(_BLOCK // (n * n), 1)
    for c in range(0, gm.shape[1], step):
        cost = gm[None, :, c:c + step] + sq  # (i, j, columns)
        j = cost.argmin(axis=1)  # (i, columns)
        og[:, c:c + step] = np.take_along_axis(cost, j[:, None, :], axis=1)[:, 0, :]
        oi[:, c:c + step] = np.take_along_axis(im[:, c:c + step], j, axis=0)
    moved = np.moveaxis(g, axis, 0).shape
    return np.moveaxis(og.reshape(moved), 0, axis), np.moveaxis(oi.reshape(moved), 0, axis)


def nearest_separable(sites, cap=0):
    """(d2, nearest) from three passes, x then y then z, each breaking its ties toward the smaller coordinate."""
    g = np.where(sites, 0, _BIG).astype(np.int64)
    idx = linear_index(sites.shape)
    for axis in (2, 1, 0):
        g, idx = _pass(g, idx, axis)
    none = g >= _BIG
    return _capped(np.where(none, FAR, g), np.where(none, NONE, idx), cap)


def check_against_d2(sites, d2, nearest, cap=0):
    """What holds for any right answer: NONE exactly where FAR, the indexed voxel is a site, and the squared distance
    to it is d2, which is scipy's."""
    want = dr.d2_scipy(sites, cap)
    assert d2.tobytes() == want.tobytes()
    assert ((nearest == NONE) == (want == FAR)).all()
    has = nearest != NONE
    assert sites.reshape(-1)[nearest[has]].all()
    nz, ny, nx = sites.shape
    n = nearest[has].astype(np.int64)
    z, y, x = np.nonzero(has)
    assert ((n // (ny * nx) - z) ** 2 + (n // nx % ny - y) ** 2 + (n % nx - x) ** 2 == want[has]).all()
    assert (nearest[sites] == linear_index(sites.shape)[sites]).all()


def scan_lines(g, idx, axis, early_stop):
    """The outward scan of the line kernel over one axis, element by element: best starts at the element's own value,
    d = 1, 2, ... looks at i - d, then i + d.  early_stop: while d * d < best and strict improvements only -- enough
    for the minimum, not for the index; otherwise while d * d <= best with the lower side winning on equality."""
    n = g.shape[axis]
    gm, im = np.moveaxis(g, axis, 0).reshape(n, -1), np.moveaxis(idx, axis, 0).reshape(n, -1)
    og, oi = gm.copy(), im.copy()
    for c in range(gm.shape[1]):
        for i in range(n):
            best, j, d = int(gm[i, c]), i, 1
            while (d * d < best) if early_stop else (d * d <= best):
                lo, hi = i - d, i + d
                if lo < 0 and hi >= n:
                    break
                if lo >= 0:
                    v = int(gm[lo, c]) + d * d
                    if v < best or (v == best and not early_stop):
                        best, j = v, lo
                if hi < n:
                    v = int(gm[hi, c]) + d * d
                    if v < best:
                        best, j = v, hi
                d += 1
            og[i, c], oi[i, c] = best, im[j, c]
    moved = np.moveaxis(g, axis, 0).shape
    return np.moveaxis(og.reshape(moved), 0, axis), np.moveaxis(oi.reshape(moved), 0, axis)


def nearest_by_scan(sites, early_stop):
    """(d2, nearest) with pass x from the separable form and passes y and z from scan_lines; tiny boxes only."""
    g = np.where(sites, 0, _BIG).astype(np.int64)
    g, idx = _pass(g, linear_index(sites.shape), 2)
    for axis in (1, 0):
        g, idx = scan_lines(g, idx, axis, early_stop)
    none = g >= _BIG
    return _capped(np.where(none, FAR, g), np.where(none, NONE, idx), 0)
