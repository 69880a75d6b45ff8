"""Restatement of include/emf_hip.h "Distance field"  for the tests: the occupancy classes and the
stamping of objects in float32 numpy, operation by operation in the order of csrc/common.hpp (mul, to_voxel, rint), and
the squared distance transform from scipy's exact feature transform (nearest-site INDICES, so the squared distance is
an integer; ties between sites do not matter, the squared distance is unique) or, for small volumes, from all pairs."""
import numpy as np

FREE, OCCUPIED, UNKNOWN = 0, 1, 2
FAR = 0x7fffffff
BRUTE_LIMIT = 5000  # voxels: all pairs is quadratic

SHAPES = [(8, 8, 32), (16, 16, 64), (9, 17, 65), (10, 12, 40),
          (2, 3, 600), (2, 600, 3), (600, 3, 2),  # one line longer than a wave, a 64-column bundle's 512
          (1, 7, 33), (5, 1, 70), (6, 9, 1),      # an axis of 1
          (2, 1100, 20), (1100, 2, 20),           # the 16-column bundles
          (1, 2048, 5), (2048, 1, 5), (2, 1, 2048)]  # the longest line of every pass
CONTENTS = ["none", "origin", "far_corner", "plane_z0", "plane_xlast", "p01", "p50", "all"]


def site_field(shape, content, seed=0):
    """bool (nz, ny, nx): where the sites of a named content are."""
    nz, ny, nx = shape
    s = np.zeros(shape, bool)
    rng = np.random.default_rng([seed, nz, ny, nx])
    if content == "origin":
        s[0, 0, 0] = True
    elif content == "far_corner":
        s[-1, -1, -1] = True
    elif content == "plane_z0":
        s[0] = True
    elif content == "plane_xlast":
        s[:, :, -1] = True
    elif content == "p01":
        s = rng.random(shape) < 0.01
    elif content == "p50":
        s = rng.random(shape) < 0.5
    elif content == "all":
        s[:] = True
    else:
        assert content == "none"
    return s


def classes_with_sites(sites, site_mask, seed=0):
    """u8 classes whose sites under site_mask are exactly `sites`: a site takes a class of the mask, every other
    voxel a class outside it (site_mask 7 has no class left for them: those get the invalid class 3)."""
    rng = np.random.default_rng([seed, site_mask])
    inside = [c for c in range(3) if (site_mask >> c) & 1]
    outside = [c for c in range(3) if not (site_mask >> c) & 1] or [3]
    return np.where(sites, rng.choice(inside, sites.shape), rng.choice(outside, sites.shape)).astype(np.uint8)


def sites_of(classes, site_mask):
    c = classes.astype(np.int64)
    return (c < 3) & (((site_mask >> np.minimum(c, 3)) & 1) != 0)


def apply_cap(d2, cap):
    d2 = d2.astype(np.int64)
    if cap > 0:
        d2 = np.where(d2 > cap * cap, FAR, d2)
    return d2.astype(np.int32)


def d2_scipy(sites, cap=0):
    """Exact squared distance to the nearest site, FAR without one or beyond the cap: (nz, ny, nx) i32."""
    from scipy import ndimage
    if not sites.any():
        return np.full(sites.shape, FAR, np.int32)
    idx = ndimage.distance_transform_edt(~sites, return_distances=False, return_indices=True)
    diff = idx.astype(np.int64) - np.indices(sites.shape)
    return apply_cap((diff * diff).sum(axis=0), cap)


def d2_brute(sites, cap=0):
    """The same from all pairs; small volumes only."""
    assert sites.size <= BRUTE_LIMIT
    if not sites.any():
        return np.full(sites.shape, FAR, np.int32)
    v = np.stack(np.indices(sites.shape), -1).reshape(-1, 3).astype(np.int64)
    s = v[sites.reshape(-1)]
    d = np.concatenate([((v[k:k + 256, None, :] - s[None, :, :]) ** 2).sum(-1).min(axis=1) for k in range(0, len(v), 256)])
    return apply_cap(d.reshape(sites.shape), cap)


def distance_transform(classes, site_mask=2, cap=0):
    return d2_scipy(sites_of(classes, site_mask), cap)


def metres_of(d2, voxel_size):
    """sqrtf(float(d2)) * voxel_size in float32 (both operations correctly rounded), +inf where FAR."""
    with np.errstate(invalid="ignore"):
        m = np.sqrt(d2.astype(np.float32)) * np.float32(voxel_size)
    return np.where(d2 == FAR, np.float32(np.inf), m).astype(np.float32)


def signed_metres(outside, inside):
    """+d_outside where the voxel is not a site, -d_inside where it is (float32 metres of the two transforms)."""
    return np.where(outside > 0, outside, -inside).astype(np.float32)


def crop(a, box):
    if box is None:
        return a
    (x, y, z), (sx, sy, sz) = box
    return a[z:z + sz, y:y + sy, x:x + sx]


def classes_of(tsdf, weights, box=None):
    """FREE: weights > 0 and tsdf > 0; OCCUPIED: weights > 0 and not (tsdf > 0); UNKNOWN: not (weights > 0)."""
    t, w = crop(tsdf, box), crop(weights, box)
    with np.errstate(invalid="ignore"):
        seen, pos = w > 0, t > 0
    return np.where(seen, np.where(pos, FREE, OCCUPIED), UNKNOWN).astype(np.uint8)


def half_extent(n):
    return np.float32(n - 1) / np.float32(2)


def object_solid(res, voxel_size, box, obj):
    """bool (bz, by, bx): the voxels of the box of a background (res = (nx, ny, nz)) that one object
    (tsdf, weights, fg_mask or None, voxel_size, R, t) turns OCCUPIED."""
    tsdf, weights, fg, vo, R, t = obj
    (x0, y0, z0), (sx, sy, sz) = box if box is not None else ((0, 0, 0), res)
    f = np.float32
    R = np.asarray(R, f).reshape(3, 3)
    t = np.asarray(t, f).reshape(3)
    vb, vo = f(voxel_size), f(vo)
    z, y, x = np.meshgrid(np.arange(z0, z0 + sz), np.arange(y0, y0 + sy), np.arange(x0, x0 + sx), indexing="ij")
    pb = [(c.astype(f) - half_extent(n)) * vb for c, n in zip((x, y, z), res)]
    oz, oy, ox = tsdf.shape
    inside = np.ones(x.shape, bool)
    idx = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a, n in zip(range(3), (ox, oy, oz)):
            po = (R[a, 0] * pb[0] + R[a, 1] * pb[1]) + R[a, 2] * pb[2] + t[a]
            q = po / vo + half_extent(n)
            r = np.rint(q)
            ok = ~np.isnan(q) & (r >= 0) & (r <= n - 1)
            inside &= ok
            idx.append(np.where(ok, r, 0).astype(np.int64))
        ix, iy, iz = idx
        solid = inside & (weights[iz, iy, ix] > 0) & ~(tsdf[iz, iy, ix] > 0)
    if fg is not None:
        solid &= fg[iz, iy, ix] != 0
    return solid


def stamp(classes, res, voxel_size, box, objects):
    out = classes.copy()
    for obj in objects:
        out[object_solid(res, voxel_size, box, obj)] = OCCUPIED
    return out
