"""numpy binding of the reference's own kernels built for the host (oracle/_ref/libemf_ref.so).

TEST INFRASTRUCTURE ONLY: what pins oracle/emf_oracle.c.  The library is made by
oracle/build_ref.py from a checkout of the reference; it is never committed and never loaded by
emfusion_amd/.  Functions carry the names, argument order and array layouts of oracle/binding.py
wherever the oracle has a function of the same shape, so one test body can drive either.

Where the oracle folds in a host-side step of the reference, the same step is done here in plain
numpy and said so: the zero fill of TSDF::updateGradients, ObjTSDF::raycast's masked weights copy,
getMesh's ``weights > 0 [& fg]`` mask, renderGPU's image.setTo(0).
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import build_ref

HERE = Path(__file__).resolve().parent
PATH = HERE / "_ref" / "libemf_ref.so"
_lib = None


def available() -> bool:
    """The library is there (whether it loads is for lib() to say)."""
    return PATH.is_file()


def reference_present() -> bool:
    return build_ref.reference_present()


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = C.CDLL(str(PATH))
        _lib.ref_abi_version.restype = C.c_int
        assert _lib.ref_abi_version() == 1
        _lib.ref_marchingCubes.restype = C.c_int
    return _lib


def _c(a, dtype=np.float32):
    return np.ascontiguousarray(a, dtype=dtype)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _farr(v, n):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
    assert a.size == n
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def _res(vol):
    nz, ny, nx = vol.shape[:3]
    return (C.c_int * 3)(nx, ny, nz)


def compute_points(depth, K):
    depth = _c(depth)
    h, w = depth.shape
    pts = np.full((h, w, 3), 7.0, np.float32)  # the reference zero-fills, then writes every pixel
    lib().ref_computePoints(_p(depth), _p(pts), w, h, _farr(K, 9))
    return pts


def update_tsdf(depth, assoc, tsdf, weights, R_OC, t_OC, K, voxel_size, truncdist, max_weight):
    depth, assoc = _c(depth), _c(assoc)
    assert tsdf.flags.c_contiguous and weights.flags.c_contiguous
    assert tsdf.dtype == np.float32 and weights.dtype == np.float32
    h, w = depth.shape
    lib().ref_updateTSDF(_p(depth), _p(assoc), w, h, _p(tsdf), _p(weights), _farr(R_OC, 9),
                         _farr(t_OC, 3), _farr(K, 9), _res(tsdf), C.c_float(voxel_size),
                         C.c_float(truncdist), C.c_float(max_weight))


def compute_tsdf_grads(tsdf):
    tsdf = _c(tsdf)
    grads = np.zeros(tsdf.shape + (3,), np.float32)  # TSDF::updateGradients: setTo(0), then the kernel
    lib().ref_computeTSDFGrads(_p(tsdf), _p(grads), _res(tsdf))
    return grads


def raycast_tsdf(tsdf, grads, weights, fg_mask, w, h, R_CO, t_CO, K, voxel_size, truncdist,
                 raylengths=None):
    """``grads=None``: the gradient volume is computed by the reference's own kernel first.
    ``fg_mask``: ObjTSDF::raycast's raycastWeights = weights where the mask is set, else 0."""
    tsdf, weights = _c(tsdf), _c(weights)
    grads = compute_tsdf_grads(tsdf) if grads is None else _c(grads)
    if fg_mask is not None:
        weights = np.where(_c(fg_mask, np.uint8) != 0, weights, np.float32(0)).astype(np.float32)
    ray = np.zeros((h, w), np.float32) if raylengths is None else _c(raylengths).copy()
    vert = np.zeros((h, w, 3), np.float32)
    nrm = np.zeros((h, w, 3), np.float32)
    mask = np.zeros((h, w), np.uint8)
    lib().ref_raycastTSDF(_p(tsdf), _p(grads), _p(weights), _p(ray), _p(vert), _p(nrm), _p(mask), w,
                          h, _farr(R_CO, 9), _farr(t_CO, 3), _farr(K, 9), _res(tsdf),
                          C.c_float(voxel_size), C.c_float(truncdist))
    return ray, vert, nrm, mask


def get_volume_vals(vol, points, R_CO, t_CO, voxel_size):
    vol, points = _c(vol), _c(points)
    ch = 1 if vol.ndim == 3 else vol.shape[3]
    h, w = points.shape[:2]
    vals = np.full((h, w) if ch == 1 else (h, w, ch), 9.0, np.float32)  # the callee zero-fills
    lib().ref_getVolumeVals(_p(vol), ch, _p(points), w, h, _farr(R_CO, 9), _farr(t_CO, 3), _res(vol),
                            C.c_float(voxel_size), _p(vals))
    return vals


def update_fgbg_probs(mask, occluded, tsdf, weights, fgbg, R_OC, t_OC, K, voxel_size):
    mask, occluded = _c(mask, np.uint8), _c(occluded, np.uint8)
    tsdf, weights = _c(tsdf), _c(weights)
    assert fgbg.flags.c_contiguous and fgbg.dtype == np.float32
    h, w = mask.shape
    lib().ref_updateFgBgProbs(_p(mask), _p(occluded), w, h, _p(tsdf), _p(weights), _p(fgbg),
                              _farr(R_OC, 9), _farr(t_OC, 3), _farr(K, 9), _res(tsdf),
                              C.c_float(voxel_size))


def compute_pose_gradients(tsdf, grads_vol, points, R_CO, t_CO, voxel_size):
    """The reference takes only the gradient volume; ``grads_vol=None`` computes it from ``tsdf``."""
    tsdf, points = _c(tsdf), _c(points)
    gv = compute_tsdf_grads(tsdf) if grads_vol is None else _c(grads_vol)
    h, w = points.shape[:2]
    out = np.full((h * w, 6), 9.0, np.float32)  # the callee zero-fills
    lib().ref_computePoseGradients(_p(gv), _p(points), w, h, _farr(R_CO, 9), _farr(t_CO, 3),
                                   _res(tsdf), C.c_float(voxel_size), _p(out))
    return out


def compute_ab(grads6, tsdf_vals):
    """Per-pixel products: As (n, 36) = g g^T, bs (n, 6) = tsdf * g."""
    g, tv = _c(grads6), _c(tsdf_vals).reshape(-1)
    n = tv.size
    assert g.shape == (n, 6)
    As, bs = np.full((n, 36), 9.0, np.float32), np.full((n, 6), 9.0, np.float32)
    lib().ref_computeAb(_p(g), _p(tv), n, _p(As), _p(bs))
    return As, bs


def mult_singleton_col(col, m):
    """m (n, c) scaled row-wise by col (n,)."""
    col, m = _c(col).reshape(-1), _c(m)
    n, c = m.shape
    assert col.size == n
    out = np.full((n, c), 9.0, np.float32)
    lib().ref_multSingletonCol(_p(col), _p(m), n, c, _p(out))
    return out


def copy_values(src, dst, offset):
    """dst[z - oz, y - oy, x - ox] = src[z, y, x] where that lies inside dst; offset = (ox, oy, oz)."""
    src = _c(src)
    assert dst.flags.c_contiguous and dst.dtype == np.float32
    ch = 1 if src.ndim == 3 else src.shape[3]
    lib().ref_copyValues(_p(src), _p(dst), ch, _i3(offset), _res(src), _res(dst))


def marching_cubes(tsdf, weights, voxel_size, fg=None, grads=None):
    """(vertices (n, 3), normals (n, 3), triangles (m, 4)); mask = weights > 0 [& fg != 0] as
    TSDF::getMesh / ObjTSDF::getMesh build it."""
    t, w = _c(tsdf), _c(weights)
    g = compute_tsdf_grads(t) if grads is None else _c(grads)
    mask = (w > 0).astype(np.uint8)
    if fg is not None:
        mask &= (_c(fg, np.uint8) != 0).astype(np.uint8)
    nt = C.c_int()
    nv = lib().ref_marchingCubes(_p(t), _p(g), _p(mask), _res(t), C.c_float(voxel_size), C.byref(nt))
    v, n = np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32)
    tri = np.empty((nt.value // 4, 4), np.int32)
    lib().ref_marchingCubesFetch(_p(v), _p(n), _p(tri))
    return v, n, tri


def render_phong(points, normals, seg, color_map, light=(0.0, 0.0, 0.0)):
    p, n = _c(points), _c(normals)
    s, cm = _c(seg, np.uint8), _c(color_map, np.uint8)
    h, w = s.shape
    assert cm.size == 768
    out = np.zeros((h, w, 3), np.uint8)  # image.setTo(0); the kernel skips pixels without a point
    lib().ref_renderPhong(_p(p), _p(n), _p(s), _p(cm), _farr(light, 3), w, h, _p(out))
    return out
