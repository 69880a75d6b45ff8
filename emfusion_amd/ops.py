"""Thin wrappers that hand device arrays (emfusion_amd.devmem.DeviceArray) to the emf_hip_* C ABI.

Harness-side plumbing only: all arithmetic happens inside libemf_hip.so.  Every wrapper enqueues
on the null stream unless ``stream`` (a raw hipStream_t integer of the product's HIP runtime) is
given, and never synchronises.

Layout conventions (see include/emf_hip.h): images are (H, W) or (H, W, C) arrays, rows possibly
padded (pitch); volumes are contiguous arrays of shape (Nz, Ny, Nx) or (Nz, Ny, Nx, C);
``res`` is (Nx, Ny, Nz).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import EmfImage, check
from .devmem import DeviceArray, DeviceView, synchronize

_L = _lib.load()


def _stream(stream: Optional[int]) -> C.c_void_p:
    return C.c_void_p(stream or 0)


def _f(values, n: int):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1))
    assert a.size == n, f"expected {n} floats, got {a.size}"
    return (C.c_float * n)(*a.tolist())


def _res(t: DeviceArray):
    nz, ny, nx = t.shape[0], t.shape[1], t.shape[2]
    return (C.c_int32 * 3)(nx, ny, nz)


def _ptr(t: Optional[DeviceArray]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.ptr)


def _vol(t: DeviceArray, dtype, channels: int = 1) -> DeviceArray:
    assert isinstance(t, DeviceArray) and t.dtype == np.dtype(dtype) and not t.padded, \
        "volume must be a contiguous device array"
    assert len(t.shape) == (3 if channels == 1 else 4), f"volume rank for {channels} channel(s)"
    if channels > 1:
        assert t.shape[3] == channels
    return t


def image_view(t: DeviceArray) -> EmfImage:
    """emf_image_t over an (H, W[, C]) device array; rows may be padded."""
    assert isinstance(t, DeviceArray) and len(t.shape) in (2, 3)
    return EmfImage(t.ptr, t.pitch, t.shape[1], t.shape[0])


def _views(ts: Sequence[DeviceArray]):
    arr = (EmfImage * max(len(ts), 1))()
    for i, t in enumerate(ts):
        arr[i] = image_view(t)
    return arr


def compute_points(depth, K, points, stream=None):
    check("emf_hip_computePoints",
          _L.emf_hip_computePoints(C.byref(image_view(depth)), C.byref(image_view(points)),
                                   _f(K, 9), _stream(stream)))
    return points


def brick_shape(vol_shape):
    """Shape (2, Bz, By, Bx) of the brick flag buffer of a (Nz, Ny, Nx) volume: [0] raw flags,
    [1] dilated flags."""
    return (2,) + tuple((n + 3) // 4 for n in vol_shape[:3])


def reset_brick_flags(tsdf_like, flags, stream=None):
    check("emf_hip_resetBrickFlags",
          _L.emf_hip_resetBrickFlags(_ptr(flags), _res(tsdf_like), _stream(stream)))
    return flags


def compute_inv_lambda(K, inv_lambda, stream=None):
    """inv_lambda: f32 H x W DeviceArray, written with the per-pixel 1 / lambda table."""
    check("emf_hip_computeInvLambda",
          _L.emf_hip_computeInvLambda(_f(K, 9), C.byref(image_view(inv_lambda)), _stream(stream)))


def _opt_view(img):
    return C.byref(image_view(img)) if img is not None else None


def update_tsdf(depth, assoc, tsdf, weights, R_OC, t_OC, K, voxel_size, truncdist, max_weight,
                brick_flags=None, stream=None, inv_lambda=None):
    _vol(tsdf, np.float32)
    _vol(weights, np.float32)
    if brick_flags is not None:
        assert brick_flags.dtype == np.dtype(np.uint8) and brick_flags.shape == brick_shape(tsdf.shape)
    check("emf_hip_updateTSDF",
          _L.emf_hip_updateTSDF(C.byref(image_view(depth)), C.byref(image_view(assoc)), _ptr(tsdf),
                                _ptr(weights), _ptr(brick_flags), _f(R_OC, 9), _f(t_OC, 3), _f(K, 9), _res(tsdf),
                                voxel_size, truncdist, max_weight, _opt_view(inv_lambda),
                                _stream(stream)))


def compute_tsdf_grads(tsdf, grads, stream=None):
    _vol(tsdf, np.float32)
    _vol(grads, np.float32, 3)
    check("emf_hip_computeTSDFGrads",
          _L.emf_hip_computeTSDFGrads(_ptr(tsdf), _ptr(grads), _res(tsdf), _stream(stream)))


def raycast_tsdf(tsdf, grads, weights, fg_mask, raylengths, vertices, normals, mask, R_CO, t_CO, K,
                 voxel_size, truncdist, stats=None, brick_flags=None, stream=None, rcp_voxel=0.0):
    _vol(tsdf, np.float32)
    _vol(weights, np.float32)
    if grads is not None:
        _vol(grads, np.float32, 3)
    if fg_mask is not None:
        _vol(fg_mask, np.uint8)
    if stats is not None:
        assert stats.dtype == np.dtype(np.uint64) and stats.shape[0] >= 4
    check("emf_hip_raycastTSDF",
          _L.emf_hip_raycastTSDF(_ptr(tsdf), _ptr(grads), _ptr(weights), _ptr(fg_mask),
                                 _ptr(brick_flags), C.byref(image_view(raylengths)), C.byref(image_view(vertices)),
                                 C.byref(image_view(normals)), C.byref(image_view(mask)),
                                 _f(R_CO, 9), _f(t_CO, 3), _f(K, 9), _res(tsdf), voxel_size,
                                 truncdist, float(rcp_voxel), _ptr(stats), _stream(stream)))


def get_volume_vals(vol, points, R_CO, t_CO, voxel_size, vals, stream=None):
    channels = 1 if len(vol.shape) == 3 else vol.shape[3]
    _vol(vol, np.float32, channels)
    check("emf_hip_getVolumeVals",
          _L.emf_hip_getVolumeVals(_ptr(vol), channels, C.byref(image_view(points)), _f(R_CO, 9),
                                   _f(t_CO, 3), _res(vol), voxel_size, C.byref(image_view(vals)),
                                   _stream(stream)))
    return vals


def update_fgbg_probs(mask, occluded, tsdf, weights, fgbg, R_OC, t_OC, K, voxel_size, stream=None):
    _vol(tsdf, np.float32)
    _vol(weights, np.float32)
    _vol(fgbg, np.float32, 2)
    check("emf_hip_updateFgBgProbs",
          _L.emf_hip_updateFgBgProbs(C.byref(image_view(mask)), C.byref(image_view(occluded)),
                                     _ptr(tsdf), _ptr(weights), _ptr(fgbg), _f(R_OC, 9),
                                     _f(t_OC, 3), _f(K, 9), _res(tsdf), voxel_size,
                                     _stream(stream)))


def compute_fg_probs(fgbg, fg_probs, fg_vol_mask, stream=None):
    _vol(fgbg, np.float32, 2)
    _vol(fg_probs, np.float32)
    _vol(fg_vol_mask, np.uint8)
    check("emf_hip_computeFgProbs",
          _L.emf_hip_computeFgProbs(_ptr(fgbg), _ptr(fg_probs), _ptr(fg_vol_mask), _res(fg_probs),
                                    _stream(stream)))


def mask_raycast_weights(weights, fg_vol_mask, out, stream=None):
    _vol(weights, np.float32)
    _vol(fg_vol_mask, np.uint8)
    _vol(out, np.float32)
    check("emf_hip_maskRaycastWeights",
          _L.emf_hip_maskRaycastWeights(_ptr(weights), _ptr(fg_vol_mask), _ptr(out), _res(weights),
                                        _stream(stream)))


def compute_association(tsdf, fg_probs, points, R_CO, t_CO, voxel_size, truncdist, sigma, alpha,
                        uni_prior, out, stream=None):
    _vol(tsdf, np.float32)
    if fg_probs is not None:
        _vol(fg_probs, np.float32)
    check("emf_hip_computeAssociation",
          _L.emf_hip_computeAssociation(_ptr(tsdf), _ptr(fg_probs), C.byref(image_view(points)),
                                        _f(R_CO, 9), _f(t_CO, 3), _res(tsdf), voxel_size,
                                        truncdist, sigma, alpha, uni_prior,
                                        C.byref(image_view(out)), _stream(stream)))
    return out


def normalize_association(maps, extra_sum=None, norm=None, nsum=None, stream=None):
    views = _views(maps)
    nsum = len(maps) if nsum is None else int(nsum)
    ex = C.byref(image_view(extra_sum)) if extra_sum is not None else None
    nr = C.byref(image_view(norm)) if norm is not None else None
    check("emf_hip_normalizeAssociation",
          _L.emf_hip_normalizeAssociation(views, len(maps), nsum, ex, nr, _stream(stream)))


def normalize_association_table(models_dev, nmodels, width, height, norm=None, stream=None):
    """normalize_association(nsum = all) over the `assoc` maps of a device model table, one launch."""
    check("emf_hip_normalizeAssociationTable",
          _L.emf_hip_normalizeAssociationTable(_ptr(models_dev), int(nmodels), int(width), int(height), _ptr(norm),
                                               _stream(stream)))


def sum_association(maps, out, stream=None):
    views = _views(maps)
    check("emf_hip_sumAssociation",
          _L.emf_hip_sumAssociation(views, len(maps), C.byref(image_view(out)), _stream(stream)))
    return out


def _frame_refs(*images):
    """The composite entries' ten frame images (background raycast, outputs) as the ABI's image pointers."""
    assert len(images) == 10
    return [C.byref(image_view(t)) for t in images]


def composite_visibility(ids, obj_ray, obj_vert, obj_norm, obj_seg, bg_ray, bg_vert, bg_norm, bg_mask,
                         ray, vert, norm, seg, diff, no_obj, boundary, vis_counts, thresh, visible, mirror=None,
                         stream=None):
    """emf_hip_compositeVisibility: vis_counts must hold zeros and holds zeros again afterwards; the numbers go
    to `mirror` (int32 device array of len(ids)) and into `visible` (int32, len(ids) + 1)."""
    n = len(ids)
    ids_arr = (C.c_int32 * max(n, 1))(*[int(i) for i in ids])
    check("emf_hip_compositeVisibility",
          _L.emf_hip_compositeVisibility(n, ids_arr, _views(obj_ray), _views(obj_vert),
                                         _views(obj_norm), _views(obj_seg),
                                         *_frame_refs(bg_ray, bg_vert, bg_norm, bg_mask, ray, vert, norm, seg, diff, no_obj),
                                         boundary, _ptr(vis_counts), int(thresh), _ptr(visible),
                                         _ptr(mirror) if mirror is not None else None, _stream(stream)))


def composite_raycast(ids, obj_ray, obj_vert, obj_norm, obj_seg, bg_ray, bg_vert, bg_norm, bg_mask,
                      ray, vert, norm, seg, diff, no_obj, boundary, vis_counts, stream=None):
    n = len(ids)
    ids_arr = (C.c_int32 * max(n, 1))(*[int(i) for i in ids])
    if n:
        assert vis_counts.dtype == np.dtype(np.int32) and vis_counts.shape[0] >= n
    check("emf_hip_compositeRaycast",
          _L.emf_hip_compositeRaycast(n, ids_arr, _views(obj_ray), _views(obj_vert),
                                      _views(obj_norm), _views(obj_seg),
                                      *_frame_refs(bg_ray, bg_vert, bg_norm, bg_mask, ray, vert, norm, seg, diff, no_obj),
                                      boundary, _ptr(vis_counts if n else None), _stream(stream)))


def occluded_mask(obj_seg, seg, obj_id, occluded, stream=None):
    check("emf_hip_occludedMask",
          _L.emf_hip_occludedMask(C.byref(image_view(obj_seg)), C.byref(image_view(seg)),
                                  int(obj_id), C.byref(image_view(occluded)), _stream(stream)))
    return occluded


def stream_copy(dst, src, stream=None):
    """dst <- src with the plain copy kernel (both DeviceArrays of equal byte size)."""
    assert dst.nbytes == src.nbytes
    check("emf_hip_streamCopy", _L.emf_hip_streamCopy(_ptr(dst), _ptr(src), dst.nbytes, _stream(stream)))


def l1_gather_probe(buf, footprint_bytes, lines, iterations, workgroups, sink, stream=None):
    """emf_hip_l1GatherProbe: the vector L1's gather rate on a resident footprint (bench.py's calibration)."""
    check("emf_hip_l1GatherProbe", _L.emf_hip_l1GatherProbe(_ptr(buf), int(footprint_bytes), int(lines), int(iterations),
                                                            int(workgroups), _ptr(sink), _stream(stream)))


def device_info():
    name = C.create_string_buffer(256)
    arch = C.create_string_buffer(256)
    cus = C.c_int(0)
    check("emf_hip_device_info", _L.emf_hip_device_info(name, 256, arch, 256, C.byref(cus)))
    return name.value.decode(), arch.value.decode(), cus.value


# ---- level 3: batched, model-table driven launches ----------------------------------------------

def make_model(tsdf, weights, assoc, raylengths, vertices, normals, hit_mask, voxel_size,
               truncdist, max_weight, sigma, alpha, uni_prior, model_id=0, grads=None,
               fg_probs=None, fg_mask=None, brick_flags=None, rcp_voxel=0.0, sign_maps=None, relevant_tiles=None,
               unseen_tiles=None) -> "_lib.EmfModel":
    """Fill an emf_model_t from device arrays (images must be unpadded)."""
    f32 = np.float32
    m = _lib.EmfModel()
    m.tsdf, m.weights = tsdf.ptr, weights.ptr
    m.grads = grads.ptr if grads is not None else None
    m.fgProbs = fg_probs.ptr if fg_probs is not None else None
    m.fgVolMask = fg_mask.ptr if fg_mask is not None else None
    m.brickFlags = brick_flags.ptr if brick_flags is not None else None
    m.signMaps = sign_maps.ptr if sign_maps is not None else None
    m.relevantTiles = relevant_tiles.ptr if relevant_tiles is not None else None
    m.unseenTiles = unseen_tiles.ptr if unseen_tiles is not None else None
    for name, im in (("assoc", assoc), ("raylengths", raylengths), ("vertices", vertices),
                     ("normals", normals), ("hitMask", hit_mask)):
        assert not im.padded
        setattr(m, name, im.ptr)
    nz, ny, nx = tsdf.shape
    m.res[:] = [nx, ny, nz]
    m.id = model_id
    m.voxelSize, m.truncdist, m.maxWeight = voxel_size, truncdist, max_weight
    m.assocC1 = float(-f32(truncdist) / f32(sigma))
    m.assocC2 = float(f32(1) / (f32(2) * f32(sigma)))
    m.alpha = alpha
    m.assocC3 = float((f32(1) - f32(alpha)) * f32(uni_prior))
    m.rcpVoxel = rcp_voxel  # 0, or ops.voxel_reciprocal(voxel_size)
    return m


def upload_models(models) -> DeviceArray:
    arr = (_lib.EmfModel * len(models))(*models)
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    return DeviceArray.from_numpy(raw)


def _poses(poses):
    arr = (_lib.EmfPose * max(len(poses), 1))()
    for i, (R, t) in enumerate(poses):
        arr[i].R[:] = np.asarray(R, np.float32).reshape(-1).tolist()
        arr[i].t[:] = np.asarray(t, np.float32).reshape(-1).tolist()
    return arr


def estep_batched(models_dev, poses_co, points, normalize=True, norm=None, obj_sum=None,
                  stream=None):
    check("emf_hip_estepBatched",
          _L.emf_hip_estepBatched(_ptr(models_dev), _poses(poses_co), len(poses_co),
                                  C.byref(image_view(points)), int(normalize),
                                  C.byref(image_view(norm)) if norm is not None else None,
                                  C.byref(image_view(obj_sum)) if obj_sum is not None else None,
                                  _stream(stream)))


def estep_batched_from_depth(models_dev, poses_co, depth, K, points, normalize=True, norm=None, obj_sum=None,
                             stream=None):
    """compute_points + estep_batched in one launch; `points` is written."""
    check("emf_hip_estepBatchedFromDepth",
          _L.emf_hip_estepBatchedFromDepth(_ptr(models_dev), _poses(poses_co), len(poses_co),
                                           C.byref(image_view(depth)), _f(K, 9), C.byref(image_view(points)),
                                           int(normalize),
                                           C.byref(image_view(norm)) if norm is not None else None,
                                           C.byref(image_view(obj_sum)) if obj_sum is not None else None,
                                           _stream(stream)))


def voxel_reciprocal(voxel_size) -> float:
    """1 / voxel_size if the device check finds it usable in place of x / voxel_size, else 0."""
    r = C.c_float(0.0)
    check("emf_hip_voxelReciprocal", _L.emf_hip_voxelReciprocal(float(voxel_size), C.byref(r)))
    return float(r.value)


def voxel_reciprocal_exhaustive(voxel_size) -> int:
    """Test aid: the number of floats x, 1e-30 <= |x| <= 1e30, on which the reciprocal form and the division differ,
    counted over all 2^32 bit patterns (2.3 ms of the whole chip; nothing is cached)."""
    n = C.c_ulonglong(0)
    check("emf_hip_voxelReciprocalExhaustive", _L.emf_hip_voxelReciprocalExhaustive(float(voxel_size), C.byref(n)))
    return int(n.value)


def raycast_batched(models_dev, poses_co, res_list, width, height, K, stats=None,
                    use_brick_flags=False, stream=None, bg_band=(0, 0), far_bounds=None, voxel_sizes=None, lanes=1,
                    objects_only=False):
    """bg_band = (row0, rows): march only that row band of table slot 0 (multi-GPU background split).
    far_bounds: raycast_far_bounds()'s array for the same table, poses and image (same results, shorter marches).
    lanes: 1 / 2 / 4 lanes per background ray.  objects_only: the table (chunk) holds no background in slot 0."""
    res = (C.c_int32 * (3 * len(poses_co)))(*[int(v) for r in res_list for v in r])
    vox = None if voxel_sizes is None else _f(voxel_sizes, len(poses_co))
    if objects_only:
        check("emf_hip_raycastBatchedObjects",
              _L.emf_hip_raycastBatchedObjects(_ptr(models_dev), _poses(poses_co), res, len(poses_co), width, height,
                                               _f(K, 9), int(use_brick_flags), _ptr(far_bounds), vox, _ptr(stats),
                                               _stream(stream)))
        return
    check("emf_hip_raycastBatchedLanes",
          _L.emf_hip_raycastBatchedLanes(_ptr(models_dev), _poses(poses_co), res, len(poses_co), width,
                                         height, _f(K, 9), int(use_brick_flags), int(bg_band[0]),
                                         int(bg_band[1]), _ptr(far_bounds), vox, int(lanes), _ptr(stats),
                                         _stream(stream)))


def sign_map_bytes(res) -> int:
    return int(_L.emf_hip_signMapBytes((C.c_int32 * 3)(*[int(v) for v in res])))


def rebuild_sign_maps(tsdf, sign_maps, stream=None):
    nz, ny, nx = tsdf.shape
    check("emf_hip_rebuildSignMaps",
          _L.emf_hip_rebuildSignMaps(_ptr(tsdf), (C.c_int32 * 3)(nx, ny, nz), _ptr(sign_maps), _stream(stream)))


def unseen_tile_bytes(res) -> int:
    return int(_L.emf_hip_unseenTileBytes((C.c_int32 * 3)(*[int(v) for v in res])))


def rebuild_unseen_tiles(tsdf, weights, unseen_tiles, stream=None):
    nz, ny, nx = tsdf.shape
    check("emf_hip_rebuildUnseenTiles",
          _L.emf_hip_rebuildUnseenTiles(_ptr(tsdf), _ptr(weights), (C.c_int32 * 3)(nx, ny, nz), _ptr(unseen_tiles),
                                        _stream(stream)))


def roll_volume(tsdf, weights, shift, color=None, sign_maps=None, unseen_tiles=None, out=None, stream=None):
    """emf_hip_rollVolume: dst(v) = src(v + shift) inside the volume, 0 elsewhere, bit for bit, for (Nz, Ny, Nx) f32
    tsdf / weights and an optional (Nz, Ny, Nx, 4) u16 colour volume; shift = (x, y, z) voxels.  On the tile-granular
    path (resolution and shift multiples of 32 x 8 x 8) sign_maps / unseen_tiles -- the SOURCE's maps, both or
    neither -- are moved along.  out: (tsdf, weights[, color]) destination arrays, allocated when None.
    Returns (tsdf, weights, color or None, sign_maps or None, unseen_tiles or None): the maps are None where the
    launch did not write them (the caller rebuilds them)."""
    nz, ny, nx = tsdf.shape
    res = (C.c_int32 * 3)(nx, ny, nz)
    sh = (C.c_int32 * 3)(*[int(v) for v in shift])
    if out is None:
        out = (DeviceArray(tsdf.shape, np.float32), DeviceArray(weights.shape, np.float32)) + \
              (() if color is None else (DeviceArray(color.shape, np.uint16),))
    d_color = out[2] if color is not None else None
    tiled = bool(_L.emf_hip_rollVolumeIsTiled(res, sh))
    d_sign = d_unseen = None
    if tiled and sign_maps is not None and unseen_tiles is not None:
        d_sign = DeviceArray((sign_map_bytes((nx, ny, nz)),), np.uint8)
        d_unseen = DeviceArray((unseen_tile_bytes((nx, ny, nz)),), np.uint8)
    check("emf_hip_rollVolume",
          _L.emf_hip_rollVolume(_ptr(tsdf), _ptr(weights), _ptr(color), _ptr(sign_maps) if d_sign is not None else None,
                                _ptr(unseen_tiles) if d_sign is not None else None, _ptr(out[0]), _ptr(out[1]),
                                _ptr(d_color), _ptr(d_sign), _ptr(d_unseen), res, sh, _stream(stream)))
    return out[0], out[1], d_color, d_sign, d_unseen


TILE = (32, 8, 8)
TILE_UNIT = 8192  # bytes of one arena unit: a tile's tsdf or weights; its colour is two


def _tile_res(tsdf):
    nz, ny, nx = tsdf.shape
    return (C.c_int32 * 3)(nx, ny, nz), (nx // TILE[0], ny // TILE[1], nz // TILE[2])


def spill_tiles(tsdf, weights, box_lo, box_size, color=None, count_only=False, arena_units=None, stream=None):
    """emf_hip_spillTiles over the tile box [box_lo, box_lo + box_size) (x, y, z, in tiles) of (Nz, Ny, Nx) f32 tsdf /
    weights and an optional (Nz, Ny, Nx, 4) u16 colour volume.  Returns dict(classes (n, 3) u8, words (n, 4) u32,
    lits (n, 3) u32, units, arena): numpy arrays, candidates x fastest inside the box; arena is the DeviceArray
    ((capacity, 8192) u8) whose first `units` rows hold the literals, None with count_only.  arena_units overrides the
    capacity (the box's worst case by default).  Synchronises (the totals are read back)."""
    res, _ = _tile_res(tsdf)
    n = int(box_size[0]) * int(box_size[1]) * int(box_size[2]) if min(int(v) for v in box_size) >= 0 else 0
    classes, words = DeviceArray.zeros((max(n, 1), 3), np.uint8), DeviceArray.zeros((max(n, 1), 4), np.uint32)
    lits, totals = DeviceArray.zeros((max(n, 1), 3), np.uint32), DeviceArray.zeros((1,), np.uint32)
    scratch = DeviceArray((max(int(_L.emf_hip_spillScratchBytes(max(n, 0))) // 4, 1),), np.uint32)
    arena = None
    if not count_only:
        cap = n * (2 if color is None else 4) if arena_units is None else int(arena_units)
        arena = DeviceArray((max(cap, 1), TILE_UNIT), np.uint8)
    check("emf_hip_spillTiles",
          _L.emf_hip_spillTiles(_ptr(tsdf), _ptr(weights), _ptr(color), res, (C.c_int32 * 3)(*[int(v) for v in box_lo]),
                                (C.c_int32 * 3)(*[int(v) for v in box_size]), _ptr(scratch), _ptr(classes), _ptr(words),
                                _ptr(lits), _ptr(totals), _ptr(arena), 0 if arena is None else cap, _stream(stream)))
    return dict(classes=classes.numpy()[:n], words=words.numpy()[:n], lits=lits.numpy()[:n],
                units=int(totals.numpy()[0]), arena=arena)


def fill_tiles(tsdf, weights, coords, classes, words, lits, arena=None, arena_units=None, color=None, sign_maps=None,
               unseen_tiles=None, stream=None):
    """emf_hip_fillTiles: write the listed tiles -- coords (n, 3) i32 tile coordinates (x, y, z) with classes (n, 3) u8,
    words (n, 4) u32, lits (n, 3) u32 as spill_tiles returns them (numpy) and its arena (DeviceArray) -- into the
    device volumes tsdf / weights[/ color] in place, and their entries into sign_maps / unseen_tiles (both or
    neither).  Tiles not listed are not touched.  Synchronises: the four lists are uploaded for the call and released
    when it returns."""
    res, _ = _tile_res(tsdf)
    coords = np.ascontiguousarray(np.asarray(coords, np.int32).reshape(-1, 3))
    n = coords.shape[0]
    classes = np.ascontiguousarray(np.asarray(classes, np.uint8).reshape(-1, 3))
    words = np.ascontiguousarray(np.asarray(words, np.uint32).reshape(-1, 4))
    lits = np.ascontiguousarray(np.asarray(lits, np.uint32).reshape(-1, 3))
    assert classes.shape[0] == n and words.shape[0] == n and lits.shape[0] == n
    d = [DeviceArray.from_numpy(a) if n else None for a in (coords, classes, words, lits)]
    if arena_units is None:
        arena_units = 0 if arena is None else arena.nbytes // TILE_UNIT
    check("emf_hip_fillTiles",
          _L.emf_hip_fillTiles(_ptr(tsdf), _ptr(weights), _ptr(color), _ptr(sign_maps), _ptr(unseen_tiles), res, _ptr(d[0]),
                               _ptr(d[1]), classes.ctypes.data_as(C.c_void_p) if n else None, _ptr(d[2]), _ptr(d[3]),
                               _ptr(arena), int(arena_units), n, _stream(stream)))
    synchronize()


def raycast_far_bounds(models_dev, poses_co, res_list, width, height, K, bounds=None, stream=None, scan_mask=0xffffffff):
    """emf_hip_raycastFarBounds -> float32 (nmodels, cellsY, cellsX) device array."""
    n = len(poses_co)
    res = (C.c_int32 * (3 * n))(*[int(v) for r in res_list for v in r])
    if bounds is None:
        cy, cx = 2 * ((height + 15) // 16), 2 * ((width + 15) // 16)
        assert int(_L.emf_hip_raycastFarBoundBytes(n, width, height)) == 4 * n * cy * cx
        bounds = DeviceArray.zeros((n, cy, cx), np.float32)
    check("emf_hip_raycastFarBounds",
          _L.emf_hip_raycastFarBounds(_ptr(models_dev), _poses(poses_co), res, n, width, height, _f(K, 9), int(scan_mask),
                                      _ptr(bounds), _stream(stream)))
    return bounds


def relevant_tile_words(res) -> int:
    return int(_L.emf_hip_relevantTileBytes((C.c_int32 * 3)(*[int(v) for v in res]))) // 4


def update_relevant_tiles(models_dev, res_list, stream=None):
    n = len(res_list)
    res = (C.c_int32 * (3 * n))(*[int(v) for r in res_list for v in r])
    check("emf_hip_updateRelevantTiles", _L.emf_hip_updateRelevantTiles(_ptr(models_dev), res, n, _stream(stream)))


def integrate_batched(models_dev, poses_oc, res_list, visible, depth, K, stats=None, stream=None,
                      inv_lambda=None):
    res = (C.c_int32 * (3 * len(poses_oc)))(*[int(v) for r in res_list for v in r])
    check("emf_hip_integrateBatched",
          _L.emf_hip_integrateBatched(_ptr(models_dev), _poses(poses_oc), res, len(poses_oc),
                                      _ptr(visible), C.byref(image_view(depth)),
                                      _opt_view(inv_lambda), _f(K, 9), 1, _ptr(stats),
                                      _stream(stream)))


def integrate_color_batched(models_dev, colors, poses_oc, res_list, visible, depth, rgb, K, stats=None, stream=None,
                            inv_lambda=None):
    """emf_hip_integrateColorBatched: colors = one (Nz, Ny, Nx, 4) u16 device array (or None: skipped) per model;
    rgb an (H, W, 3) u8 device image.  The colour volumes are updated in place."""
    res = (C.c_int32 * (3 * len(poses_oc)))(*[int(v) for r in res_list for v in r])
    ptrs = DeviceArray.from_numpy(np.array([0 if c is None else c.ptr for c in colors], np.uint64))
    check("emf_hip_integrateColorBatched",
          _L.emf_hip_integrateColorBatched(_ptr(models_dev), _ptr(ptrs), _poses(poses_oc), res, len(poses_oc),
                                           _ptr(visible), C.byref(image_view(depth)), _opt_view(inv_lambda),
                                           C.byref(image_view(rgb)), _f(K, 9), _ptr(stats), _stream(stream)))
    from .devmem import synchronize
    synchronize()  # `ptrs` is released on return


def copy_color_values(src: DeviceArray, dst: DeviceArray, offset, stream=None):
    """dst(v) = src(v + offset) inside src, else 0, for colour volumes (Nz, Ny, Nx, 4) u16."""
    sres = (C.c_int32 * 3)(src.shape[2], src.shape[1], src.shape[0])
    dres = (C.c_int32 * 3)(dst.shape[2], dst.shape[1], dst.shape[0])
    check("emf_hip_copyColorValues",
          _L.emf_hip_copyColorValues(_ptr(src), _ptr(dst), (C.c_int32 * 3)(*[int(v) for v in offset]), sres, dres,
                                     _stream(stream)))


def integrate_batched_culled(models_dev, poses_oc, res_list, visible, depth, K, launch_boxes=0, survivors=None,
                             stats=None, stream=None, inv_lambda=None, scratch=None):
    """emf_hip_integrateBatchedCulled; returns the scratch buffer (reusable)."""
    res = (C.c_int32 * (3 * len(poses_oc)))(*[int(v) for r in res_list for v in r])
    if scratch is None:
        scratch = DeviceArray.zeros((int(_L.emf_hip_integrateCullScratchBytes(res, len(poses_oc))) // 4,), np.uint32)
    check("emf_hip_integrateBatchedCulled",
          _L.emf_hip_integrateBatchedCulled(_ptr(models_dev), _poses(poses_oc), res, len(poses_oc), _ptr(visible),
                                            C.byref(image_view(depth)), _opt_view(inv_lambda), _f(K, 9),
                                            _ptr(scratch), int(launch_boxes), _ptr(survivors), _ptr(stats),
                                            _stream(stream)))
    return scratch


def integrate_dirty_map_bytes(res) -> int:
    return int(_L.emf_hip_integrateDirtyMapBytes((C.c_int32 * 3)(*[int(v) for v in res])))


def integrate_prepare_out(outs, res_list, scratch, stream=None):
    """emf_hip_integratePrepareOut: clear the survivor counter and the dirtyNext maps of outs ahead of time."""
    from ._lib import EmfVolumeOut
    res = (C.c_int32 * (3 * len(res_list)))(*[int(v) for r in res_list for v in r])
    table = (EmfVolumeOut * len(outs))()
    for o, (t, w, dp, dn) in zip(table, outs):
        o.tsdf, o.weights, o.dirtyPrev, o.dirtyNext = t.ptr, w.ptr, dp.ptr, dn.ptr
    check("emf_hip_integratePrepareOut",
          _L.emf_hip_integratePrepareOut(C.cast(table, C.c_void_p), res, len(outs), _ptr(scratch), _stream(stream)))


def integrate_batched_culled_out(models_dev, poses_oc, res_list, visible, depth, K, outs, launch_boxes=0,
                                 stats=None, stream=None, inv_lambda=None, scratch=None, prepared=False):
    """emf_hip_integrateBatchedCulledOut: model m is read from the table and written to outs[m] =
    (tsdf_back, weights_back, dirty_prev, dirty_next) device arrays; returns the scratch buffer."""
    from ._lib import EmfVolumeOut
    res = (C.c_int32 * (3 * len(poses_oc)))(*[int(v) for r in res_list for v in r])
    if scratch is None:
        scratch = DeviceArray.zeros((int(_L.emf_hip_integrateCullScratchBytes(res, len(poses_oc))) // 4,), np.uint32)
    table = (EmfVolumeOut * len(outs))()
    for o, (t, w, dp, dn) in zip(table, outs):
        o.tsdf, o.weights, o.dirtyPrev, o.dirtyNext = t.ptr, w.ptr, dp.ptr, dn.ptr
    check("emf_hip_integrateBatchedCulledOut",
          _L.emf_hip_integrateBatchedCulledOut(_ptr(models_dev), _poses(poses_oc), res, len(poses_oc), _ptr(visible),
                                               C.byref(image_view(depth)), _opt_view(inv_lambda), _f(K, 9),
                                               C.cast(table, C.c_void_p), int(prepared), _ptr(scratch), int(launch_boxes), None,
                                               _ptr(stats), _stream(stream)))
    return scratch


def visibility_flags(vis_counts, nmodels, thresh, visible, stream=None):
    check("emf_hip_visibilityFlags",
          _L.emf_hip_visibilityFlags(_ptr(vis_counts), nmodels, thresh, _ptr(visible), None,
                                     _stream(stream)))


# ---- cross-GPU compositing ------------------------------------------------------------------------

def pack_hit_keys(list_pos, obj_ray, obj_seg, keys, width, height, stream=None):
    n = len(list_pos)
    pos = (C.c_int32 * max(n, 1))(*[int(p) for p in list_pos])
    assert keys.dtype == np.dtype(np.uint64)
    check("emf_hip_packHitKeys",
          _L.emf_hip_packHitKeys(n, pos, _views(obj_ray), _views(obj_seg), _ptr(keys), width,
                                 height, _stream(stream)))
    return keys


def composite_from_keys(keys, ids_all, list_pos, obj_ray, obj_vert, obj_norm, bg_ray, bg_vert,
                        bg_norm, bg_mask, ray, vert, norm, seg, diff, no_obj, boundary, vis_counts,
                        stream=None):
    nall, n = len(ids_all), len(list_pos)
    ids = (C.c_int32 * max(nall, 1))(*[int(i) for i in ids_all])
    pos = (C.c_int32 * max(n, 1))(*[int(p) for p in list_pos])
    check("emf_hip_compositeFromKeys",
          _L.emf_hip_compositeFromKeys(_ptr(keys), nall, ids, n, pos, _views(obj_ray),
                                       _views(obj_vert), _views(obj_norm),
                                       *_frame_refs(bg_ray, bg_vert, bg_norm, bg_mask, ray, vert, norm, seg, diff, no_obj),
                                       boundary, _ptr(vis_counts if nall else None),
                                       _stream(stream)))


def visibility_flags_indexed(vis_counts, count_index, thresh, visible, stream=None):
    n = len(count_index)
    idx = (C.c_int32 * max(n, 1))(*[int(i) for i in count_index])
    check("emf_hip_visibilityFlagsIndexed",
          _L.emf_hip_visibilityFlagsIndexed(_ptr(vis_counts), n, idx, thresh, _ptr(visible),
                                            _stream(stream)))


# ---- direct peer-write exchanges (include/emf_hip.h; `group` is an _lib.EmfPeer) ------------------------

def peer_buffer_bytes(world, slot_bytes) -> int:
    return int(_L.emf_hip_peerBufferBytes(int(world), int(slot_bytes)))


def peer_raycast_slot_bytes(width, height) -> int:
    return int(_L.emf_hip_peerRaycastSlotBytes(int(width), int(height)))


def _at(t, byte_offset=0) -> C.c_void_p:
    """Device address `byte_offset` bytes into a device array (or a raw address)."""
    return C.c_void_p((t.ptr if isinstance(t, DeviceArray) else int(t)) + int(byte_offset))


def peer_scatter(group, src, nbytes, dst_offset, seq, src_offset=0, stream=None):
    check("emf_hip_peerScatter",
          _L.emf_hip_peerScatter(C.byref(group), _at(src, src_offset), int(nbytes), int(dst_offset), int(seq),
                                 _stream(stream)))


def peer_signal_wait(group, seq, timeout_ms=0, stream=None):
    check("emf_hip_peerSignalWait", _L.emf_hip_peerSignalWait(C.byref(group), int(seq), int(timeout_ms), _stream(stream)))


def peer_reduce_sum_f32(group, seq, count, out, wait=False, stream=None):
    """out := sum over the slots in rank order; wait: the peerWait* form, which signals and waits itself."""
    name = "emf_hip_peerWaitReduceSumF32" if wait else "emf_hip_peerReduceSumF32"
    check(name, getattr(_L, name)(C.byref(group), int(seq), int(count), _at(out), _stream(stream)))


def peer_reduce_min_u64(group, seq, count, out, wait=False, stream=None):
    name = "emf_hip_peerWaitReduceMinU64" if wait else "emf_hip_peerReduceMinU64"
    check(name, getattr(_L, name)(C.byref(group), int(seq), int(count), _at(out), _stream(stream)))


def peer_copy_from_slot(group, seq, sender, src_offset, dst, nbytes, dst_offset=0, stream=None):
    check("emf_hip_peerCopyFromSlot",
          _L.emf_hip_peerCopyFromSlot(C.byref(group), int(seq), int(sender), int(src_offset), _at(dst, dst_offset),
                                      int(nbytes), _stream(stream)))


def peer_wait_copy_from_slots(group, seq, parts, stream=None):
    """parts: (sender, slot offset, destination array, destination offset, bytes) each, copied in one launch behind the wait."""
    n = len(parts)
    senders = (C.c_int32 * max(n, 1))(*[int(p[0]) for p in parts])
    offsets = (C.c_size_t * max(n, 1))(*[int(p[1]) for p in parts])
    dsts = (C.c_void_p * max(n, 1))(*[_at(p[2], p[3]).value for p in parts])
    sizes = (C.c_size_t * max(n, 1))(*[int(p[4]) for p in parts])
    check("emf_hip_peerWaitCopyFromSlots",
          _L.emf_hip_peerWaitCopyFromSlots(C.byref(group), int(seq), n, senders, offsets, dsts, sizes, _stream(stream)))


def estep_batched_peer(models_dev, poses_co, points, group, seq, depth=None, K=None, stream=None):
    """estep_batched(normalize=False) whose per-pixel sum of the object maps goes into this rank's slot on every peer."""
    check("emf_hip_estepBatchedPeer",
          _L.emf_hip_estepBatchedPeer(_ptr(models_dev), _poses(poses_co), len(poses_co),
                                      C.byref(image_view(depth)) if depth is not None else None,
                                      _f(K, 9) if K is not None else None, C.byref(image_view(points)), C.byref(group),
                                      int(seq), _stream(stream)))


def peer_normalize_association(group, seq, maps, obj_sum=None, norm=None, stream=None):
    check("emf_hip_peerNormalizeAssociation",
          _L.emf_hip_peerNormalizeAssociation(C.byref(group), int(seq), _views(maps), len(maps),
                                              C.byref(image_view(obj_sum)) if obj_sum is not None else None,
                                              C.byref(image_view(norm)) if norm is not None else None, _stream(stream)))


def pack_hit_keys_peer(list_pos, obj_ray, obj_seg, bg_ray, bg_mask, band_row0, band_rows, group, seq, stream=None):
    n = len(list_pos)
    pos = (C.c_int32 * max(n, 1))(*[int(p) for p in list_pos])
    check("emf_hip_packHitKeysPeer",
          _L.emf_hip_packHitKeysPeer(n, pos, _views(obj_ray), _views(obj_seg), C.byref(image_view(bg_ray)),
                                     C.byref(image_view(bg_mask)), int(band_row0), int(band_rows), C.byref(group), int(seq),
                                     _stream(stream)))


def composite_from_keys_peer(group, seq, band_rows_per_rank, ids_all, list_pos, obj_ray, obj_vert, obj_norm, bg_ray,
                             bg_vert, bg_norm, bg_mask, ray, vert, norm, seg, diff, no_obj, boundary, vis_counts,
                             stream=None):
    nall, n = len(ids_all), len(list_pos)
    ids = (C.c_int32 * max(nall, 1))(*[int(i) for i in ids_all])
    pos = (C.c_int32 * max(n, 1))(*[int(p) for p in list_pos])
    check("emf_hip_compositeFromKeysPeer",
          _L.emf_hip_compositeFromKeysPeer(C.byref(group), int(seq), int(band_rows_per_rank), nall, ids, n, pos,
                                           _views(obj_ray), _views(obj_vert), _views(obj_norm),
                                           *_frame_refs(bg_ray, bg_vert, bg_norm, bg_mask, ray, vert, norm, seg, diff, no_obj),
                                           int(boundary), _ptr(vis_counts), _stream(stream)))


def visibility_flags_mirror(vis_counts, nall, count_index, thresh, visible, mirror=None, stream=None):
    n = len(count_index)
    idx = (C.c_int32 * max(n, 1))(*[int(i) for i in count_index])
    check("emf_hip_visibilityFlagsMirror",
          _L.emf_hip_visibilityFlagsMirror(_ptr(vis_counts), int(nall), n, idx, int(thresh), _ptr(visible), _ptr(mirror),
                                           _stream(stream)))


# ---- tracking (SURVEY f-1) ----------------------------------------------------------------------

def compute_pose_gradients(tsdf, grads, points, R_CO, t_CO, voxel_size, out, stream=None):
    """out: float32 DeviceArray (H * W, 6); grads: gradient volume or None (on the fly)."""
    _vol(tsdf, np.float32)
    check("emf_hip_computePoseGradients",
          _L.emf_hip_computePoseGradients(_ptr(tsdf), _ptr(grads), C.byref(image_view(points)),
                                          _f(R_CO, 9), _f(t_CO, 3), _res(tsdf), voxel_size,
                                          _ptr(out), _stream(stream)))


def track_scratch_bytes(width, height) -> int:
    return int(_L.emf_hip_trackScratchBytes(int(width), int(height)))


def track_prepare(states_dev, poses_co, nu_init=2.0, stream=None):
    """states_dev: uint8 DeviceArray of len(poses_co) * sizeof(EmfTrackState) bytes."""
    check("emf_hip_trackPrepare",
          _L.emf_hip_trackPrepare(_ptr(states_dev), _poses(poses_co), len(poses_co), nu_init,
                                  _stream(stream)))


def track_iterate(models_dev, states_dev, nmodels, points, params, scratch, scratch_per_model,
                  iterations=1, stream=None):
    check("emf_hip_trackIterate",
          _L.emf_hip_trackIterate(_ptr(models_dev), _ptr(states_dev), nmodels,
                                  C.byref(image_view(points)), C.byref(params), _ptr(scratch),
                                  scratch_per_model, iterations, _stream(stream)))


def track_step(models_dev, states_dev, nmodels, points, params, scratch, scratch_per_model, launch,
               iterations, watch=None, seq=0, stream=None, final_states=None):
    """One launch of the LM step kernel (emf_hip_trackStep); watch: address of host-pinned uint32s or None;
    final_states: address of nmodels EmfTrackState the device can write (a done model's state, ahead of its word) or None."""
    check("emf_hip_trackStep",
          _L.emf_hip_trackStep(_ptr(models_dev), _ptr(states_dev), nmodels, C.byref(image_view(points)),
                               C.byref(params), _ptr(scratch), scratch_per_model, launch, iterations,
                               watch, seq, final_states, _stream(stream)))


def track_weight_images(models_dev, states_dev, nmodels, points, params, scratch, scratch_per_model,
                        huber=None, track=None, stream=None):
    """Huber and combined tracking weights of a finished stage at its final pose (emf_hip_trackWeightImages);
    huber / track: device arrays of nmodels x H x W floats or None."""
    check("emf_hip_trackWeightImages",
          _L.emf_hip_trackWeightImages(_ptr(models_dev), _ptr(states_dev), nmodels, C.byref(image_view(points)),
                                       C.byref(params), _ptr(scratch), scratch_per_model,
                                       _ptr(huber) if huber is not None else None,
                                       _ptr(track) if track is not None else None, _stream(stream)))


def read_track_states(states_dev, nmodels):
    """Synchronise and return the device LM states as a list of EmfTrackState."""
    raw = states_dev.numpy().tobytes()
    n = C.sizeof(_lib.EmfTrackState)
    return [_lib.EmfTrackState.from_buffer_copy(raw[i * n:(i + 1) * n]) for i in range(nmodels)]


# ---- depth pre-processing (SURVEY f-2) -----------------------------------------------------------

def preprocess_depth(raw, out, ksz=7, sigma_depth=0.04, sigma_spatial=4.5, stream=None):
    check("emf_hip_preprocessDepth",
          _L.emf_hip_preprocessDepth(C.byref(image_view(raw)), C.byref(image_view(out)), int(ksz),
                                     sigma_depth, sigma_spatial, _stream(stream)))


# ---- object creation / matching from masks (SURVEY f-3) ------------------------------------------

def _stats_buffers(buffers):
    """(scratch, out) of the point statistics: fresh and zeroed, or the caller's pair (any contents)."""
    if buffers is not None:
        return buffers
    return (DeviceArray.zeros((int(_L.emf_hip_pointStatsScratchBytes()) // 4,), np.uint32),
            DeviceArray.zeros((7,), np.float32))


def masked_point_stats(points, mask, R, t, stream=None, buffers=None):
    """(count, p10[3], p90[3]) of the valid masked points after x' = R x + t (synchronises).  buffers: None, or
    the (scratch uint32[emf_hip_pointStatsScratchBytes / 4], out float32[7]) device arrays to use."""
    scratch, out = _stats_buffers(buffers)
    check("emf_hip_maskedPointStats",
          _L.emf_hip_maskedPointStats(C.byref(image_view(points)), C.byref(image_view(mask)), _f(R, 9),
                                      _f(t, 3), _ptr(scratch), _ptr(out), _stream(stream)))
    raw = out.numpy()
    return int(raw.view(np.uint32)[0]), raw[1:4].copy(), raw[4:7].copy()


def mask_overlap(seg, model_seg, stream=None):
    """(mask pixels, intersection[256], area[256]) against every id of the model segmentation."""
    counts = DeviceArray.zeros((513,), np.uint32)
    check("emf_hip_maskOverlap",
          _L.emf_hip_maskOverlap(C.byref(image_view(seg)), C.byref(image_view(model_seg)),
                                 _ptr(counts), _stream(stream)))
    c = counts.numpy()
    return int(c[0]), c[1:257].copy(), c[257:513].copy()


def mask_association_mass(obj_seg, match_mask, assoc, stream=None, out=None):
    """(count, sum) of cleanUpObjs' association test; match_mask may be None (synchronises).  out: None, or the
    float64[emf_hip_maskAssociationMassBytes / 8] device array to use (any contents)."""
    if out is None:
        out = DeviceArray.zeros((int(_L.emf_hip_maskAssociationMassBytes()) // 8,), np.float64)
    check("emf_hip_maskAssociationMass",
          _L.emf_hip_maskAssociationMass(C.byref(image_view(obj_seg)), _opt_view(match_mask),
                                         C.byref(image_view(assoc)), _ptr(out), _stream(stream)))
    raw = out.numpy()
    return int(raw.view(np.uint32)[2]), float(raw[0])


def carve_mask(seg, model_seg, obj_id, match_mask=None, stream=None):
    """seg &= !((model_seg == obj_id) | match_mask) in place; returns (pixels before, after)."""
    counts = DeviceArray.zeros((2,), np.uint32)
    check("emf_hip_carveMask",
          _L.emf_hip_carveMask(C.byref(image_view(seg)), C.byref(image_view(model_seg)), int(obj_id),
                               _opt_view(match_mask), _ptr(counts), _stream(stream)))
    c = counts.numpy()
    return int(c[0]), int(c[1])


def object_extent_stats(points, mask, R, t, tsdf, weights, fg_mask, voxel_size, stream=None, buffers=None):
    """updateObj's statistics: masked points (R x + t) plus the object's iso-surface vertex cloud.  buffers: as in
    masked_point_stats."""
    scratch, out = _stats_buffers(buffers)
    check("emf_hip_objectExtentStats",
          _L.emf_hip_objectExtentStats(C.byref(image_view(points)), C.byref(image_view(mask)), _f(R, 9),
                                       _f(t, 3), _ptr(tsdf), _ptr(weights), _ptr(fg_mask), _res(tsdf),
                                       voxel_size, _ptr(scratch), _ptr(out), _stream(stream)))
    raw = out.numpy()
    return int(raw.view(np.uint32)[0]), raw[1:4].copy(), raw[4:7].copy()


def hide_label(segmentation, label, vertices, normals, bg_vertices, bg_normals, stream=None):
    """ignore_person in EMFusion::render: pixels of `label` become 0 and show the background's vertex / normal."""
    check("emf_hip_hideLabel",
          _L.emf_hip_hideLabel(C.byref(image_view(segmentation)), int(label), C.byref(image_view(vertices)),
                               C.byref(image_view(normals)), C.byref(image_view(bg_vertices)),
                               C.byref(image_view(bg_normals)), _stream(stream)))


def render_phong(vertices, normals, segmentation, color_map, image, light=(0.0, 0.0, 0.0), stream=None):
    """renderGPU: Phong-shaded RGB image (H, W, 3) u8 of the composited raycast; color_map (256, 3) u8 host."""
    cm = np.ascontiguousarray(color_map, np.uint8)
    assert cm.size == 768
    check("emf_hip_renderPhong",
          _L.emf_hip_renderPhong(C.byref(image_view(vertices)), C.byref(image_view(normals)),
                                 C.byref(image_view(segmentation)), cm.ctypes.data, _f(light, 3),
                                 C.byref(image_view(image)), _stream(stream)))
    return image


def upload_poses(poses) -> DeviceArray:
    """emf_pose_t[n] on the device from [(R, t), ...] (the pose array of render_view)."""
    arr = _poses(poses)
    return DeviceArray.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8)[:len(poses) * C.sizeof(_lib.EmfPose)].copy())


def hide_mask(labels) -> np.ndarray:
    """The 32-byte label mask of render_view: bit s (byte s // 8, bit s % 8) hides label s."""
    m = np.zeros(32, np.uint8)
    for s in labels:
        assert 1 <= int(s) <= 255, f"label {s}"
        m[int(s) >> 3] |= np.uint8(1 << (int(s) & 7))
    return m


def render_view(models_dev, poses_vo, ids, width, height, K, rgb, raylengths=None, segmentation=None, vertices=None,
                normals=None, color_map=None, light=(0.0, 0.0, 0.0), hide=(), stats=None, stream=None):
    """emf_hip_renderView: the whole table (slot 0 = background) seen from a viewer in one launch -- raycast, composite
    (zeroed diff), hide, Phong.  poses_vo: viewer -> volume per slot, [(R, t), ...] or upload_poses()'s array.
    ids: the labels of slots 1.. .  rgb (H, W, 3) u8 is required; the other outputs may be None."""
    if not isinstance(poses_vo, DeviceArray):
        poses_vo = upload_poses(poses_vo)
    n = poses_vo.nbytes // C.sizeof(_lib.EmfPose)
    ids_arr = (C.c_int32 * max(n - 1, 1))(*[int(i) for i in ids]) if n > 1 else None
    assert n <= 1 or len(ids) == n - 1, "one label per object slot"
    cm = np.ascontiguousarray(np.zeros((256, 3), np.uint8) if color_map is None else color_map, np.uint8)
    assert cm.size == 768
    hm = hide_mask(hide)

    def view(t):
        return None if t is None else C.byref(image_view(t))

    check("emf_hip_renderView",
          _L.emf_hip_renderView(_ptr(models_dev), _ptr(poses_vo), ids_arr, n, int(width), int(height), _f(K, 9),
                                _f(light, 3), cm.ctypes.data, hm.ctypes.data, view(rgb), view(raylengths),
                                view(segmentation), view(vertices), view(normals), _ptr(stats), _stream(stream)))
    return rgb


def sample_color(models_dev, colors, poses_vo, ids, vertices, segmentation, color_map, out, stream=None):
    """emf_hip_sampleColor: per pixel of a view (vertices (H, W, 3) f32 in the viewer frame, segmentation (H, W) u8, as
    render_view writes them) the colour of the nearest voxel of the model the label names, label colour where nobody
    coloured it.  colors: one colour volume (or None) per table slot, or None for label colours only; poses_vo as
    render_view; out (H, W, 3) u8."""
    if not isinstance(poses_vo, DeviceArray):
        poses_vo = upload_poses(poses_vo)
    n = poses_vo.nbytes // C.sizeof(_lib.EmfPose)
    ids_arr = (C.c_int32 * max(n - 1, 1))(*[int(i) for i in ids]) if n > 1 else None
    ptrs = None
    if colors is not None:
        assert len(colors) == n
        ptrs = DeviceArray.from_numpy(np.array([0 if c is None else c.ptr for c in colors], np.uint64))
    cm = np.ascontiguousarray(color_map, np.uint8)
    assert cm.size == 768
    check("emf_hip_sampleColor",
          _L.emf_hip_sampleColor(_ptr(models_dev), _ptr(ptrs), _ptr(poses_vo), ids_arr, n, C.byref(image_view(vertices)),
                                 C.byref(image_view(segmentation)), cm.ctypes.data, C.byref(image_view(out)),
                                 _stream(stream)))
    from .devmem import synchronize
    synchronize()  # `ptrs` is released on return
    return out


def render_phong_color(vertices, normals, colors, image, light=(0.0, 0.0, 0.0), stream=None):
    """emf_hip_renderPhongColor: render_phong with each pixel's diffuse colour read from `colors` (H, W, 3) u8."""
    check("emf_hip_renderPhongColor",
          _L.emf_hip_renderPhongColor(C.byref(image_view(vertices)), C.byref(image_view(normals)),
                                      C.byref(image_view(colors)), _f(light, 3), C.byref(image_view(image)),
                                      _stream(stream)))
    return image


class _T(tuple):
    """The arguments only the ...Batched form of a mesh entry takes, at their place among the others."""

    def __new__(cls, *args):
        return super().__new__(cls, args)


def _mesh_entry(name, batched, *args):
    """check() of the mesh entry `name` for one mesh or, `batched`, of `name`Batched for a table of meshes."""
    if batched:
        name += "Batched"
    flat = []
    for a in args:
        if isinstance(a, _T):
            flat.extend(a if batched else ())
        else:
            flat.append(a)
    check(name, getattr(_L, name)(*flat))


def _kept_arrays(knv, knt, cols):
    """Device arrays for knv vertices and knt triangles coming out of a pass, one spare element each: (vertices,
    normals, triangles -- None where knt is, the pass rewrites them in place --, colours or None as `cols` is)."""
    kv = DeviceArray.zeros((max(knv, 1), 3), np.float32)
    kn = DeviceArray.zeros((max(knv, 1), 3), np.float32)
    kt = None if knt is None else DeviceArray.zeros((max(knt, 1), 4), np.int32)
    kc = None if cols is None else DeviceArray.zeros((max(knv, 1), 3), np.uint8)
    return kv, kn, kt, kc


def _weld(keys, nv, nt, verts, norms, tris, cols, soup_bases=None, n=1, stream=None):
    """emf_hip_meshWeldCount / ...Emit on device soup arrays: (welded vertices, normals, triangles, colours or None as
    device arrays, welded counts (n,) u32, welded bases (n + 1,) u64 on the host and on the device)."""
    scratch = DeviceArray.zeros((max(int(_L.emf_hip_meshWeldScratchBytes(nv)) // 4, 4),), np.uint32)
    wcounts = DeviceArray.zeros((max(n, 1),), np.uint32)
    wbases = DeviceArray.zeros((n + 1,), np.uint64)
    batched = soup_bases is not None
    _mesh_entry("emf_hip_meshWeldCount", batched, _ptr(keys), nv, _T(_ptr(soup_bases), n), _ptr(scratch), _ptr(wcounts),
                _T(_ptr(wbases)), _stream(stream))
    check("emf_hip_meshWeldStatus", _L.emf_hip_meshWeldStatus(_ptr(scratch), nv, _stream(stream)))
    cnt = wcounts.numpy()
    nw = int(cnt.sum())
    wv, wn, _, wc = _kept_arrays(nw, None, cols)
    if nv:
        _mesh_entry("emf_hip_meshWeldEmit", batched, _ptr(scratch), nv, nt, _T(_ptr(soup_bases), _ptr(wbases), n),
                    _ptr(verts), _ptr(norms), _ptr(cols), _ptr(tris), _ptr(wv), _ptr(wn), _ptr(wc), _ptr(tris),
                    _stream(stream))
    from .devmem import synchronize
    synchronize()  # the scratch is released on return
    return wv, wn, tris, wc, cnt, wbases.numpy(), wbases


def _on_device(a, dtype):
    return a if isinstance(a, DeviceArray) else DeviceArray.from_numpy(np.ascontiguousarray(a, dtype))


def _table_bases(tri_bases, vertex_bases):
    """Host bases of a table of meshes -> (n, device soup bases 2 (n + 1) u64 with the triangle bases in the odd
    entries, device welded bases (n + 1) u64), or (1, None, None) for one mesh."""
    if tri_bases is None and vertex_bases is None:
        return 1, None, None
    tb, vb = np.asarray(tri_bases, np.uint64), np.asarray(vertex_bases, np.uint64)
    if tb.ndim != 1 or tb.shape != vb.shape or len(tb) < 2:
        raise ValueError("tri_bases and vertex_bases: n + 1 entries each")
    inter = np.zeros((len(tb), 2), np.uint64)
    inter[:, 1] = tb
    return len(tb) - 1, DeviceArray.from_numpy(inter), DeviceArray.from_numpy(vb)


def _label(tris, nv, nt, soup_bases=None, wbases=None, n=1, outputs=True, stream=None):
    """emf_hip_meshComponentsLabel / ...Batched on a device index buffer: (scratch, labels, sizes) as device arrays
    (labels and sizes None without `outputs`)."""
    nbytes = int(_L.emf_hip_meshComponentsScratchBytes(nv, nt))
    if nbytes == 0:
        raise ValueError(f"mesh components: {nv} vertices / {nt} triangles are beyond the limits")
    scratch = DeviceArray.zeros((nbytes // 4,), np.uint32)
    labels = DeviceArray.zeros((max(nv, 1),), np.int32) if outputs else None
    sizes = DeviceArray.zeros((max(nv, 1),), np.uint32) if outputs else None
    _mesh_entry("emf_hip_meshComponentsLabel", soup_bases is not None, _ptr(tris), nv, nt,
                _T(_ptr(soup_bases), _ptr(wbases), n), _ptr(scratch), _ptr(labels), _ptr(sizes), _stream(stream))
    return scratch, labels, sizes


def _per_model(value, n, dtype):
    a = np.asarray(value)
    return np.ascontiguousarray(np.broadcast_to(a, (n,)) if a.ndim == 0 else a.reshape(n), dtype)


def _filter(nv, nt, verts, norms, tris, cols, min_triangles, largest_only, soup_bases=None, wbases=None, n=1,
            stream=None):
    """Label, filter-count, status and emit on device welded arrays: (kept vertices, normals, triangles, colours or
    None as device arrays, kept counts (n, 2) u32, kept bases (n + 1, 2) u64, dict(components=, kept_components=))."""
    scratch, _, _ = _label(tris, nv, nt, soup_bases, wbases, n, outputs=False, stream=stream)
    mins = _per_model(min_triangles, n, np.uint32)
    largest = _per_model(largest_only, n, np.uint8)
    kcounts = DeviceArray.zeros((n, 2), np.uint32)
    kbases = DeviceArray.zeros((n + 1, 2), np.uint64)
    comps = DeviceArray.zeros((n,), np.uint32)
    kcomps = DeviceArray.zeros((n,), np.uint32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    batched = soup_bases is not None
    table = _T(_ptr(soup_bases), _ptr(wbases), n)
    _mesh_entry("emf_hip_meshComponentsFilterCount", batched, _ptr(tris), nv, nt, table, _ptr(scratch), hp(mins),
                hp(largest), _ptr(kcounts), _T(_ptr(kbases)), _ptr(comps), _ptr(kcomps), _stream(stream))
    check("emf_hip_meshComponentsStatus", _L.emf_hip_meshComponentsStatus(_ptr(scratch), nv, nt, _stream(stream)))
    cnt = kcounts.numpy()
    if soup_bases is None:
        bs = np.array([[0, 0], cnt[0]], np.uint64)
    else:
        bs = kbases.numpy()
    knv, knt = int(bs[n, 0]), int(bs[n, 1])
    kv, kn, kt, kc = _kept_arrays(knv, knt, cols)
    if nv:
        _mesh_entry("emf_hip_meshComponentsEmit", batched, _ptr(scratch), nv, nt, table, _ptr(verts), _ptr(norms),
                    _ptr(cols), _ptr(tris), _ptr(kv), _ptr(kn), _ptr(kc), _ptr(kt), _stream(stream))
    from .devmem import synchronize
    synchronize()  # the scratch is released on return
    return kv, kn, kt, kc, cnt, bs, dict(components=comps.numpy(), kept_components=kcomps.numpy())


def mesh_components(triangles, n_vertices, tri_bases=None, vertex_bases=None, stream=None):
    """emf_hip_meshComponentsLabel: connected components of an indexed mesh, by index (include/emf_hip.h "Mesh
    components").  triangles: (m, 4) i32 records (3, i0, i1, i2), numpy or device; n_vertices: the vertices they index.
    A table of meshes: tri_bases / vertex_bases, n + 1 host entries each, the triangles' indices model-local.
    Returns (labels (n_vertices,) i32 -- the smallest model-local index of the vertex's component --, sizes
    (n_vertices,) u32 -- that component's triangles)."""
    nv = int(n_vertices)
    nt = int(triangles.shape[0])
    n, sb, wb = _table_bases(tri_bases, vertex_bases)
    if nv == 0 and nt == 0:
        return np.zeros((0,), np.int32), np.zeros((0,), np.uint32)
    tris = _on_device(triangles, np.int32) if nt else None
    scratch, labels, sizes = _label(tris, nv, nt, sb, wb, n, stream=stream)
    check("emf_hip_meshComponentsStatus", _L.emf_hip_meshComponentsStatus(_ptr(scratch), nv, nt, _stream(stream)))
    return labels.numpy()[:nv], sizes.numpy()[:nv]


def filter_mesh(vertices, normals, triangles, colors=None, min_triangles=0, largest_only=False, tri_bases=None,
                vertex_bases=None, stats=False, stream=None):
    """emf_hip_meshComponentsFilterCount / ...Emit on an indexed mesh (numpy or device arrays): the components with
    fewer than min_triangles triangles removed and, with largest_only, every component but the largest (a tie to the
    smaller label).  Returns (vertices, normals, triangles[, colours]) as numpy arrays -- kept vertices in order, bits
    unchanged, kept triangles in order, re-indexed.  A table of meshes (tri_bases / vertex_bases, n + 1 host entries
    each; min_triangles / largest_only scalars or one per mesh): a list of such tuples.  stats: also a dict
    (components, kept_components, one per mesh)."""
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    n, sb, wb = _table_bases(tri_bases, vertex_bases)
    if nv == 0:
        empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32)) + \
                (() if colors is None else (np.zeros((0, 3), np.uint8),))
        out = empty if sb is None else [empty] * n
        zero = dict(components=np.zeros((n,), np.uint32), kept_components=np.zeros((n,), np.uint32))
        return (out, zero) if stats else out
    verts, norms = _on_device(vertices, np.float32), _on_device(normals, np.float32)
    tris = _on_device(triangles, np.int32) if nt else None
    cols = None if colors is None else _on_device(colors, np.uint8)
    kv, kn, kt, kc, cnt, bs, st = _filter(nv, nt, verts, norms, tris, cols, min_triangles, largest_only, sb, wb, n,
                                          stream=stream)
    out = _slices(kv, kn, kt, kc, bs[:, 0], cnt[:, 0], bs[:, 1], cnt[:, 1], n)
    out = out[0] if sb is None else out
    return (out, st) if stats else out


def _simplify(nv, nt, verts, norms, tris, cols, cells, origin=(0.0, 0.0, 0.0), soup_bases=None, wbases=None, n=1,
              stream=None):
    """emf_hip_meshSimplifyCount / ...Status / ...Emit on device arrays: (vertices, normals, triangles, colours or None
    as device arrays, kept counts (n, 2) u32, kept bases (n + 1, 2) u64, clusters (n,) u32).  An EMF_E_ARG refusal (a
    triangle index out of range) is raised after the emit, with the arrays in the error's `partial`."""
    nbytes = int(_L.emf_hip_meshSimplifyScratchBytes(nv, nt))
    if nbytes == 0:
        raise ValueError(f"mesh simplify: {nv} vertices / {nt} triangles are beyond the limits")
    scratch = DeviceArray.zeros((nbytes // 4,), np.uint32)
    cell = _per_model(cells, n, np.float32)
    org = np.ascontiguousarray(origin, np.float32).reshape(3)
    kcounts = DeviceArray.zeros((n, 2), np.uint32)
    kbases = DeviceArray.zeros((n + 1, 2), np.uint64)
    clusters = DeviceArray.zeros((n,), np.uint32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    check("emf_hip_meshSimplifyCount",
          _L.emf_hip_meshSimplifyCount(_ptr(verts), _ptr(norms), _ptr(cols), _ptr(tris), nv, nt, _ptr(soup_bases),
                                       _ptr(wbases), n, hp(cell), hp(org), _ptr(scratch), _ptr(kcounts), _ptr(kbases),
                                       _ptr(clusters), _stream(stream)))
    refused = None
    try:
        check("emf_hip_meshSimplifyStatus", _L.emf_hip_meshSimplifyStatus(_ptr(scratch), nv, nt, _stream(stream)))
    except _lib.EmfHipError as e:
        if e.code != -4:  # EMF_E_LIMIT: the outputs are meaningless
            raise
        refused = e      # EMF_E_ARG: the offending triangles are dropped, the rest stands
    cnt, bs = kcounts.numpy(), kbases.numpy()
    knv, knt = int(bs[n, 0]), int(bs[n, 1])
    kv, kn, kt, kc = _kept_arrays(knv, knt, cols)
    if nv:
        check("emf_hip_meshSimplifyEmit",
              _L.emf_hip_meshSimplifyEmit(_ptr(scratch), nv, nt, _ptr(soup_bases), _ptr(wbases), n, _ptr(verts),
                                          _ptr(norms), _ptr(cols), _ptr(tris), _ptr(kv), _ptr(kn), _ptr(kc), _ptr(kt),
                                          _stream(stream)))
    from .devmem import synchronize
    synchronize()  # the scratch is released on return
    out = (kv, kn, kt, kc, cnt, bs, clusters.numpy())
    if refused is not None:
        refused.partial = out
        raise refused
    return out


def simplify_mesh(vertices, normals, triangles, colors=None, cell=0.0, origin=(0.0, 0.0, 0.0), tri_bases=None,
                  vertex_bases=None, stats=False, stream=None):
    """emf_hip_meshSimplifyCount / ...Emit on an indexed mesh (numpy or device arrays): vertex clustering by cubic cells
    of `cell` metres counted from `origin` (include/emf_hip.h "Simplified meshes").  Returns (vertices, normals,
    triangles[, colours]) as numpy arrays: one vertex per cluster that a kept triangle references, in order of first
    occurrence, the triangles with three distinct clusters in input order, re-indexed.  cell <= 0 passes the mesh
    through.  A table of meshes (tri_bases / vertex_bases, n + 1 host entries each; cell a scalar or one per mesh): a
    list of such tuples.  stats: also a dict (vertices_in, triangles_in, vertices_out, triangles_out, clusters, one
    entry per mesh).  A refusal raises EmfHipError; for a triangle index out of range (EMF_E_ARG) its `partial` holds
    what would have been returned, without the offending triangles."""
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    n, sb, wb = _table_bases(tri_bases, vertex_bases)
    if sb is None:
        vin, tin = np.array([nv], np.uint32), np.array([nt], np.uint32)
    else:
        vin = np.diff(np.asarray(vertex_bases, np.int64)).astype(np.uint32)
        tin = np.diff(np.asarray(tri_bases, np.int64)).astype(np.uint32)
    if nv == 0 and nt == 0:
        empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32)) + \
                (() if colors is None else (np.zeros((0, 3), np.uint8),))
        out = empty if sb is None else [empty] * n
        zero = np.zeros((n,), np.uint32)
        st = dict(vertices_in=vin, triangles_in=tin, vertices_out=zero, triangles_out=zero, clusters=zero)
        return (out, st) if stats else out
    verts, norms = _on_device(vertices, np.float32), _on_device(normals, np.float32)
    tris = _on_device(triangles, np.int32) if nt else None
    cols = None if colors is None else _on_device(colors, np.uint8)

    def result(dev):
        kv, kn, kt, kc, cnt, bs, clusters = dev
        out = _slices(kv, kn, kt, kc, bs[:, 0], cnt[:, 0], bs[:, 1], cnt[:, 1], n)
        out = out[0] if sb is None else out
        st = dict(vertices_in=vin, triangles_in=tin, vertices_out=cnt[:, 0].copy(), triangles_out=cnt[:, 1].copy(),
                  clusters=clusters)
        return (out, st) if stats else out

    try:
        return result(_simplify(nv, nt, verts, norms, tris, cols, cell, origin, sb, wb, n, stream=stream))
    except _lib.EmfHipError as e:
        if getattr(e, "partial", None) is not None:
            e.partial = result(e.partial)
        raise


def _slices(verts, norms, tris, cols, vbase, vcnt, tbase, tcnt, n):
    hv, hn, ht = verts.numpy(), norms.numpy(), tris.numpy()
    hc = None if cols is None else cols.numpy()
    out = []
    for k in range(n):
        v0, t0, cv, ct = int(vbase[k]), int(tbase[k]), int(vcnt[k]), int(tcnt[k])
        out.append((hv[v0:v0 + cv], hn[v0:v0 + cv], ht[t0:t0 + ct]) + ((hc[v0:v0 + cv],) if hc is not None else ()))
    return out


def mesh_edge_keys(tsdf, weights, fg_mask=None, stream=None):
    """emf_hip_meshEdgeKeys: the u64 grid-edge key of every soup vertex of extract_mesh(tsdf, weights, ...), in its
    vertex order: 3 * ((z * Ny + y) * Nx + x) + axis of the edge's lower voxel (include/emf_hip.h "Welded meshes")."""
    res = _res(tsdf)
    scratch = DeviceArray.zeros((max(int(_L.emf_hip_meshScratchBytes(res)) // 4, 2),), np.uint32)
    counts = DeviceArray.zeros((2,), np.uint32)
    check("emf_hip_meshCount",
          _L.emf_hip_meshCount(_ptr(tsdf), _ptr(weights), _ptr(fg_mask), res, _ptr(scratch), _ptr(counts),
                               _stream(stream)))
    nv = int(counts.numpy()[0])
    keys = DeviceArray.zeros((max(nv, 1),), np.uint64)
    if nv:
        check("emf_hip_meshEdgeKeys",
              _L.emf_hip_meshEdgeKeys(_ptr(tsdf), _ptr(weights), _ptr(fg_mask), res, _ptr(scratch), _ptr(keys),
                                      _stream(stream)))
    return keys.numpy()[:nv]


def extract_mesh(tsdf, weights, voxel_size, fg_mask=None, grads=None, stream=None, color=None, weld=False,
                 min_triangles=0, largest_only=False, simplify=0.0):
    """TSDF::getMesh / ObjTSDF::getMesh: (vertices (n, 3) f32, normals (n, 3) f32, triangles (m, 4) i32)
    as numpy arrays; two launches to count, one read-back, one launch to emit.  color: the volume's colour volume
    ((Nz, Ny, Nx, 4) u16): a fourth array, the vertex colours (n, 3) u8 (emf_hip_meshColors).  weld: the welded mesh
    instead of the soup (emf_hip_meshEdgeKeys / meshWeldCount / meshWeldEmit): one vertex per grid edge, the first
    copy's bits, triangles re-indexed.  min_triangles / largest_only (with weld): the welded mesh filtered by
    connected component (filter_mesh) on the device; off (0, False) launches nothing more.  simplify (with weld): the
    welded, filtered mesh clustered by cells of that many metres (simplify_mesh, origin 0); 0 launches nothing more."""
    if (int(min_triangles) > 1 or largest_only) and not weld:
        raise ValueError("extract_mesh: the component filter works on the welded mesh (weld=True)")
    if float(simplify) > 0 and not weld:
        raise ValueError("extract_mesh: simplification works on the welded mesh (weld=True)")
    res = _res(tsdf)
    scratch = DeviceArray.zeros((max(int(_L.emf_hip_meshScratchBytes(res)) // 4, 2),), np.uint32)
    counts = DeviceArray.zeros((2,), np.uint32)
    check("emf_hip_meshCount",
          _L.emf_hip_meshCount(_ptr(tsdf), _ptr(weights), _ptr(fg_mask), res, _ptr(scratch), _ptr(counts),
                               _stream(stream)))
    nv, nt = (int(v) for v in counts.numpy())
    verts = DeviceArray.zeros((max(nv, 1), 3), np.float32)
    norms = DeviceArray.zeros((max(nv, 1), 3), np.float32)
    tris = DeviceArray.zeros((max(nt, 1), 4), np.int32)
    if nv:
        check("emf_hip_meshEmit",
              _L.emf_hip_meshEmit(_ptr(tsdf), _ptr(grads), _ptr(weights), _ptr(fg_mask), res, voxel_size,
                                  _ptr(scratch), _ptr(verts), _ptr(norms), _ptr(tris), _stream(stream)))
    cols = None
    if color is not None:
        cols = DeviceArray.zeros((max(nv, 1), 3), np.uint8)
        if nv:
            check("emf_hip_meshColors",
                  _L.emf_hip_meshColors(_ptr(tsdf), _ptr(weights), _ptr(fg_mask), _ptr(color), res, _ptr(scratch),
                                        _ptr(cols), _stream(stream)))
    if weld:
        keys = DeviceArray.zeros((max(nv, 1),), np.uint64)
        if nv:
            check("emf_hip_meshEdgeKeys",
                  _L.emf_hip_meshEdgeKeys(_ptr(tsdf), _ptr(weights), _ptr(fg_mask), res, _ptr(scratch), _ptr(keys),
                                          _stream(stream)))
        verts, norms, tris, cols, cnt, _, _ = _weld(keys, nv, nt, verts, norms, tris, cols, stream=stream)
        nv = int(cnt[0])
        if int(min_triangles) > 1 or largest_only:
            verts, norms, tris, cols, kcnt, _, _ = _filter(nv, nt, verts, norms, tris if nt else None, cols, min_triangles,
                                                           largest_only, stream=stream)
            nv, nt = int(kcnt[0, 0]), int(kcnt[0, 1])
        if float(simplify) > 0 and nv:
            verts, norms, tris, cols, kcnt, _, _ = _simplify(nv, nt, verts, norms, tris if nt else None, cols, simplify,
                                                             stream=stream)
            nv, nt = int(kcnt[0, 0]), int(kcnt[0, 1])
    if color is not None:
        return verts.numpy()[:nv], norms.numpy()[:nv], tris.numpy()[:nt], cols.numpy()[:nv]
    return verts.numpy()[:nv], norms.numpy()[:nv], tris.numpy()[:nt]


def mesh_tile_table(coords, classes, words, at, neighbours=None):
    """The emf_mesh_tile_t table of n tiles as a ctypes array: coords (n, 3) i32 lattice tile coordinates (x, y, z),
    classes (n, 3) u8, words (n, 4) u32, at (n, 3) u64 (class 2: arena unit, class 3: element offset).  neighbours:
    (n, 7) i32, or None to look them up by coordinate."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    n = coords.shape[0]
    classes = np.asarray(classes, np.uint8).reshape(n, 3)
    words = np.asarray(words, np.uint32).reshape(n, 4)
    at = np.asarray(at, np.uint64).reshape(n, 3)
    if neighbours is None:
        index = {tuple(int(v) for v in c): i for i, c in enumerate(coords)}
        neighbours = np.full((n, 7), -1, np.int32)
        for i, c in enumerate(coords):
            for k in range(1, 8):
                key = (int(c[0]) + (k & 1), int(c[1]) + ((k >> 1) & 1), int(c[2]) + (k >> 2))
                neighbours[i, k - 1] = index.get(key, -1)
    neighbours = np.asarray(neighbours, np.int32).reshape(n, 7)
    table = (_lib.EmfMeshTile * max(n, 1))()
    for i in range(n):
        e = table[i]
        e.coord[:] = [int(v) for v in coords[i]]
        e.cls[:] = [int(v) for v in classes[i]]
        e.words[:] = [int(v) for v in words[i]]
        e.nbr[:] = [int(v) for v in neighbours[i]]
        e.at[:] = [int(v) for v in at[i]]
    return table


def mesh_tiles(tiles, voxel_size, half, weld=False, colors=False, min_triangles=0, keys=False, stream=None,
               simplify=0.0):
    """emf_hip_meshTilesCount / ...Emit[/ ...Colors / ...EdgeKeys] (include/emf_hip.h "Meshing a set of tiles"): the
    mesh of the dense volume that holds exactly the listed tiles.  tiles: dict(coords (n, 3) lattice tile coordinates
    (x, y, z), sorted ascending in (z, y, x); classes (n, 3) u8; words (n, 4) u32; at (n, 3): the arena unit of a
    class-2 array, the element offset of a class-3 one; arena: (units, 8192) u8 numpy or None; volume: None or
    dict(tsdf, weights[, color]) -- numpy (Nz, Ny, Nx) volumes that class 3 reads in place; neighbours: optional
    (n, 7) i32 instead of the lookup by coordinate).  half: the three floats a lattice voxel is shifted by.  Returns
    (vertices (n, 3) f32, normals (n, 3) f32, triangles (m, 4) i32[, colours (n, 3) u8][, keys (n,) u64]) as numpy
    arrays with global indices; weld / min_triangles / simplify as in extract_mesh (the keys are then not returned)."""
    if int(min_triangles) > 1 and not weld:
        raise ValueError("mesh_tiles: the component filter works on the welded mesh (weld=True)")
    if float(simplify) > 0 and not weld:
        raise ValueError("mesh_tiles: simplification works on the welded mesh (weld=True)")
    table = mesh_tile_table(tiles["coords"], tiles["classes"], tiles["words"], tiles["at"], tiles.get("neighbours"))
    n = int(np.asarray(tiles["coords"]).reshape(-1, 3).shape[0])
    src = _lib.EmfMeshTilesSource()
    arena = tiles.get("arena")
    d_arena = None
    if arena is not None and np.asarray(arena).size:
        d_arena = DeviceArray.from_numpy(np.ascontiguousarray(arena, np.uint8).reshape(-1, TILE_UNIT))
        src.arena, src.arena_units = d_arena.ptr, d_arena.nbytes // TILE_UNIT
    vol = tiles.get("volume")
    d_vol = []
    if vol is not None:
        nz, ny, nx = vol["tsdf"].shape
        d_vol = [DeviceArray.from_numpy(np.ascontiguousarray(vol["tsdf"], np.float32)),
                 DeviceArray.from_numpy(np.ascontiguousarray(vol["weights"], np.float32))]
        src.tsdf, src.weights = d_vol[0].ptr, d_vol[1].ptr
        if vol.get("color") is not None:
            d_vol.append(DeviceArray.from_numpy(np.ascontiguousarray(vol["color"], np.uint16)))
            src.color = d_vol[2].ptr
        src.volume_elements, src.row_stride, src.plane_stride = nz * ny * nx, nx, nx * ny
    d_table = DeviceArray.from_numpy(np.frombuffer(table, np.uint8).copy()) if n else None
    scratch = DeviceArray.zeros((max(int(_L.emf_hip_meshTilesScratchBytes(n)) // 4, 2),), np.uint32)
    counts = DeviceArray.zeros((2,), np.uint32)
    check("emf_hip_meshTilesCount",
          _L.emf_hip_meshTilesCount(_ptr(d_table), C.cast(table, C.c_void_p), n, C.byref(src), _ptr(scratch),
                                    _ptr(counts), _stream(stream)))
    nv, nt = (int(v) for v in counts.numpy())
    verts = DeviceArray.zeros((max(nv, 1), 3), np.float32)
    norms = DeviceArray.zeros((max(nv, 1), 3), np.float32)
    tris = DeviceArray.zeros((max(nt, 1), 4), np.int32)
    if nv:
        check("emf_hip_meshTilesEmit",
              _L.emf_hip_meshTilesEmit(_ptr(d_table), n, C.byref(src), _f(half, 3), voxel_size, _ptr(scratch), _ptr(verts),
                                       _ptr(norms), _ptr(tris), _stream(stream)))
    cols = None
    if colors:
        cols = DeviceArray.zeros((max(nv, 1), 3), np.uint8)
        if nv:
            check("emf_hip_meshTilesColors",
                  _L.emf_hip_meshTilesColors(_ptr(d_table), n, C.byref(src), _ptr(scratch), _ptr(cols), _stream(stream)))
    d_keys = None
    if weld or keys:
        d_keys = DeviceArray.zeros((max(nv, 1),), np.uint64)
        if nv:
            check("emf_hip_meshTilesEdgeKeys",
                  _L.emf_hip_meshTilesEdgeKeys(_ptr(d_table), n, C.byref(src), _ptr(scratch), _ptr(d_keys),
                                               _stream(stream)))
    if weld:
        verts, norms, tris, cols, cnt, _, _ = _weld(d_keys, nv, nt, verts, norms, tris, cols, stream=stream)
        nv = int(cnt[0])
        if int(min_triangles) > 1:
            verts, norms, tris, cols, kcnt, _, _ = _filter(nv, nt, verts, norms, tris if nt else None, cols, min_triangles,
                                                           False, stream=stream)
            nv, nt = int(kcnt[0, 0]), int(kcnt[0, 1])
        if float(simplify) > 0 and nv:
            verts, norms, tris, cols, kcnt, _, _ = _simplify(nv, nt, verts, norms, tris if nt else None, cols, simplify,
                                                             stream=stream)
            nv, nt = int(kcnt[0, 0]), int(kcnt[0, 1])
    synchronize()  # the uploads are released on return
    out = (verts.numpy()[:nv], norms.numpy()[:nv], tris.numpy()[:nt])
    if colors:
        out += (cols.numpy()[:nv],)
    if keys and not weld:
        out += (d_keys.numpy()[:nv],)
    return out


def mesh_table(volumes):
    """The device model table (only what meshing reads) and the host resolutions of extract_meshes' volumes."""
    n = len(volumes)
    models = []
    res = (C.c_int32 * (3 * max(n, 1)))()
    for k, v in enumerate(volumes):
        tsdf = v["tsdf"]
        m = _lib.EmfModel()
        m.tsdf, m.weights = tsdf.ptr, v["weights"].ptr
        m.grads = v["grads"].ptr if v.get("grads") is not None else None
        m.fgVolMask = v["fg_mask"].ptr if v.get("fg_mask") is not None else None
        nz, ny, nx = tsdf.shape[:3]
        m.res[:] = [nx, ny, nz]
        m.voxelSize = float(v["voxel_size"])
        res[3 * k:3 * k + 3] = [nx, ny, nz]
        models.append(m)
    return (upload_models(models) if n else None), res


def extract_meshes(volumes, stream=None, weld=False, min_triangles=0, largest_only=False, simplify=0.0):
    """emf_hip_meshCountBatched / emf_hip_meshEmitBatched: the meshes of a table of volumes in one pass (one count
    launch, one read-back of the counts, one emit launch).  volumes: [dict(tsdf=, weights=, voxel_size=, fg_mask=None,
    grads=None), ...] of device arrays, at most EMF_MAX_MODELS.  Returns [(vertices (n, 3) f32, normals (n, 3) f32,
    triangles (m, 4) i32), ...] in table order, each what extract_mesh gives for that volume alone -- with weld, what
    extract_mesh(..., weld=True) gives (emf_hip_meshEdgeKeysBatched / meshWeldCountBatched / meshWeldEmitBatched).
    min_triangles / largest_only (with weld; scalars or one value per volume): each slice filtered by connected component
    as extract_mesh(..., weld=True, min_triangles=, largest_only=) filters that volume alone.  simplify (with weld; a
    scalar or one cell per volume, 0 = that volume as it is): each slice clustered as extract_mesh(..., simplify=)
    clusters that volume alone."""
    n = len(volumes)
    filtered = bool(np.any(np.asarray(min_triangles) > 1) or np.any(largest_only))
    if filtered and not weld:
        raise ValueError("extract_meshes: the component filter works on the welded meshes (weld=True)")
    simplified = bool(np.any(np.asarray(simplify, np.float32) > 0))
    if simplified and not weld:
        raise ValueError("extract_meshes: simplification works on the welded meshes (weld=True)")
    table, res = mesh_table(volumes)
    scratch_bytes = int(_L.emf_hip_meshScratchBytesBatched(res, n))
    scratch = DeviceArray.zeros((max(scratch_bytes // 4, 2),), np.uint32)
    counts = DeviceArray.zeros((max(n, 1), 2), np.uint32)
    bases = DeviceArray.zeros((n + 1, 2), np.uint64)
    check("emf_hip_meshCountBatched",
          _L.emf_hip_meshCountBatched(_ptr(table), res, n, _ptr(scratch), _ptr(counts), _ptr(bases), _stream(stream)))
    cnt, bs = counts.numpy(), bases.numpy()
    nv, nt = int(bs[n, 0]), int(bs[n, 1])
    verts = DeviceArray.zeros((max(nv, 1), 3), np.float32)
    norms = DeviceArray.zeros((max(nv, 1), 3), np.float32)
    tris = DeviceArray.zeros((max(nt, 1), 4), np.int32)
    if nv:
        check("emf_hip_meshEmitBatched",
              _L.emf_hip_meshEmitBatched(_ptr(table), res, n, _ptr(scratch), _ptr(verts), _ptr(norms), _ptr(tris),
                                         _stream(stream)))
    cols = None
    if any(v.get("color") is not None for v in volumes):  # emf_hip_meshColorsBatched: 4-tuples, colours last
        ptrs = DeviceArray.from_numpy(np.array([0 if v.get("color") is None else v["color"].ptr for v in volumes],
                                               np.uint64))
        cols = DeviceArray.zeros((max(nv, 1), 3), np.uint8)
        if nv:
            check("emf_hip_meshColorsBatched",
                  _L.emf_hip_meshColorsBatched(_ptr(table), _ptr(ptrs), res, n, _ptr(scratch), _ptr(cols),
                                               _stream(stream)))
    vbase, vcnt, tbase, tcnt = bs[:, 0], cnt[:, 0], bs[:, 1], cnt[:, 1]
    if weld:
        keys = DeviceArray.zeros((max(nv, 1),), np.uint64)
        if nv:
            check("emf_hip_meshEdgeKeysBatched",
                  _L.emf_hip_meshEdgeKeysBatched(_ptr(table), res, n, _ptr(scratch), _ptr(keys), _stream(stream)))
        verts, norms, tris, cols, vcnt, vbase, wbases = _weld(keys, nv, nt, verts, norms, tris, cols, soup_bases=bases,
                                                              n=n, stream=stream)
        if filtered and n:
            nw = int(vbase[n])
            verts, norms, tris, cols, kcnt, kbs, _ = _filter(nw, nt, verts, norms, tris if nt else None, cols,
                                                             min_triangles, largest_only, bases, wbases, n, stream=stream)
            vbase, vcnt, tbase, tcnt = kbs[:, 0], kcnt[:, 0], kbs[:, 1], kcnt[:, 1]
            if simplified:  # the filtered table's bases, in the layout the entries take
                bases = DeviceArray.from_numpy(np.ascontiguousarray(kbs))
                wbases = DeviceArray.from_numpy(np.ascontiguousarray(vbase))
        if simplified and n and int(vbase[n]):
            nt = int(tbase[n])
            verts, norms, tris, cols, kcnt, kbs, _ = _simplify(int(vbase[n]), nt, verts, norms, tris if nt else None, cols,
                                                               simplify, soup_bases=bases, wbases=wbases, n=n,
                                                               stream=stream)
            vbase, vcnt, tbase, tcnt = kbs[:, 0], kcnt[:, 0], kbs[:, 1], kcnt[:, 1]
    return _slices(verts, norms, tris, cols, vbase, vcnt, tbase, tcnt, n)


def mask_association_masses(hit_masks, assocs, match_masks=None, verdict=None, stream=None, seed_byte=0):
    """emf_hip_maskAssociationMassBatched: cleanUpObjs' (count, sum) for n objects in one pass over a model table.
    hit_masks / assocs: n unpadded device images (u8 / f32 W x H), the objects' raycast masks and association weights,
    placed at table slots 1 .. n behind an empty slot 0 (as in the product's table); match_masks: None or n entries,
    each a device image or None.  seed_byte: what every byte of the scratch and the answers holds before the call.
    verdict: None, or dict(nall=, list_pos=[n ints], visible=[n 0/1], ex_low=[n 0/1],
    assoc_thresh=) for the delete verdicts by list position.  Returns (counts (n,) uint32, sums (n,) float64,
    verdicts (round_up(nall, 4),) float32 or None); synchronises."""
    n = len(hit_masks)
    assert len(assocs) == n and (match_masks is None or len(match_masks) == n)
    h, w = hit_masks[0].shape[:2] if n else (1, 1)
    models = [_lib.EmfModel()]
    for hm, a in zip(hit_masks, assocs):
        assert not hm.padded and not a.padded and hm.shape[:2] == (h, w) and a.shape[:2] == (h, w)
        m = _lib.EmfModel()
        m.hitMask, m.assoc = hm.ptr, a.ptr
        models.append(m)
    table = upload_models(models)
    imgs = (EmfImage * max(n, 1))()
    for k in range(n):
        mm = None if match_masks is None else match_masks[k]
        if mm is not None:
            imgs[k] = image_view(mm)
    scratch = DeviceArray.zeros((max(int(_L.emf_hip_maskAssociationMassScratchBytes(n)) // 8, 2),), np.float64)
    out = DeviceArray.zeros((max(n, 1), 2), np.float64)
    if seed_byte:
        scratch.fill_bytes_(seed_byte)
        out.fill_bytes_(seed_byte)
    vd, nall, lp, vis, ex, thr = None, 0, None, None, None, 0.0
    if verdict is not None:
        nall = int(verdict["nall"])
        vd = DeviceArray.full(((nall + 3) // 4 * 4 or 4,), 7.0, np.float32)  # all of it must be overwritten
        lp = (C.c_int32 * max(n, 1))(*[int(p) for p in verdict["list_pos"]])
        slots = np.zeros(n + 1, np.int32)
        slots[1:] = np.asarray(verdict["visible"], np.int32)
        vis = DeviceArray.from_numpy(slots)
        ex = (C.c_uint8 * max(n, 1))(*[int(bool(e)) for e in verdict.get("ex_low", [0] * n)])
        thr = float(verdict["assoc_thresh"])
    check("emf_hip_maskAssociationMassBatched",
          _L.emf_hip_maskAssociationMassBatched(_ptr(table), 1, n, w, h, imgs if match_masks is not None else None,
                                                _ptr(scratch), _ptr(out), _ptr(vd), nall, lp, _ptr(vis), ex, thr,
                                                _stream(stream)))
    raw = out.numpy()[:n]
    counts = raw[:, 1].copy().view(np.uint32)[::2] if n else np.zeros(0, np.uint32)
    return counts, raw[:, 0].copy(), (None if vd is None else vd.numpy()[:(nall + 3) // 4 * 4])


def copy_values(src, dst, offset, stream=None):
    """dst(v) = src(v + offset) inside src, else 0 (kernel_copyValues); volumes (Nz, Ny, Nx[, C])."""
    ch = 1 if len(src.shape) == 3 else src.shape[3]
    check("emf_hip_copyValues",
          _L.emf_hip_copyValues(_ptr(src), _ptr(dst), ch, (C.c_int32 * 3)(*[int(v) for v in offset]),
                                _res(src), _res(dst), _stream(stream)))


# ---- packed buffers (include/emf_hip.h "Packed buffers") --------------------------------------------------------------

PACK_CHUNK = 1024
PACK_ARENA_CHUNKS = 65536  # 64 MiB of literals per gather / upload


def _pad8(b: bytes) -> bytes:
    return b + bytes(-len(b) % 8)


def pack_arrays(buf: DeviceArray, stream=None) -> dict:
    """emf_hip_packClassify + emf_hip_packRank over a contiguous device array: dict(nbytes=, nchunks=, classes=,
    words=, ranks=, uniform=, literal_chunks= (device arrays of nchunks entries), nuniform=, nliteral=).
    Synchronises (the totals are read back)."""
    assert isinstance(buf, DeviceArray) and not buf.padded
    nbytes = buf.nbytes
    nchunks = (nbytes + PACK_CHUNK - 1) // PACK_CHUNK
    p = dict(nbytes=nbytes, nchunks=nchunks,
             classes=DeviceArray((max(nchunks, 1),), np.uint8), words=DeviceArray((max(nchunks, 1),), np.uint32))
    check("emf_hip_packClassify",
          _L.emf_hip_packClassify(_ptr(buf), nbytes, _ptr(p["classes"]), _ptr(p["words"]), _stream(stream)))
    _pack_rank(p, p["words"], stream)
    return p


def _pack_rank(p: dict, words: Optional[DeviceArray], stream=None):
    n = max(p["nchunks"], 1)
    scratch = DeviceArray((max(int(_L.emf_hip_packScratchBytes(p["nbytes"])) // 8, 1),), np.uint64)
    p["ranks"], p["literal_chunks"] = DeviceArray((n,), np.uint32), DeviceArray((n,), np.uint32)
    p["uniform"] = DeviceArray((n,), np.uint32) if words is not None else None
    totals = DeviceArray.zeros((2,), np.uint32)
    check("emf_hip_packRank",
          _L.emf_hip_packRank(_ptr(p["classes"]), _ptr(words), p["nbytes"], _ptr(scratch), _ptr(p["ranks"]),
                              _ptr(p["uniform"]), _ptr(p["literal_chunks"]), _ptr(totals), _stream(stream)))
    p["nuniform"], p["nliteral"] = (int(v) for v in totals.numpy())


def pack_gather(buf: DeviceArray, packed: dict, first: int, count: int, arena: Optional[DeviceArray] = None,
                stream=None) -> np.ndarray:
    """emf_hip_packGather: the literal chunks of ranks [first, first + count) as a (count, 1024) u8 host array."""
    assert 0 <= first and 0 <= count and first + count <= packed["nliteral"]
    if arena is None:
        arena = DeviceArray((max(count, 1), PACK_CHUNK), np.uint8)
    assert arena.nbytes >= count * PACK_CHUNK
    check("emf_hip_packGather",
          _L.emf_hip_packGather(_ptr(buf), packed["nbytes"], _ptr(packed["literal_chunks"]), first, count, _ptr(arena),
                                _stream(stream)))
    return DeviceView(arena.ptr, (count, PACK_CHUNK), np.uint8).numpy()


def pack_buffer(buf: DeviceArray, arena_chunks: int = PACK_ARENA_CHUNKS, splits: Optional[Sequence[int]] = None,
                stream=None) -> bytes:
    """The packed record (include/emf_hip.h) of a contiguous device array whose size is a multiple of 4 bytes.  The
    literals move through a device arena of at most arena_chunks chunks; ``splits`` (counts that sum to the number of
    literals) overrides how the rank ranges are cut."""
    p = pack_arrays(buf, stream)
    nu, nl = p["nuniform"], p["nliteral"]
    parts = [np.array([p["nbytes"]], "<u8").tobytes() + np.array([p["nchunks"], nu, nl, 0], "<u4").tobytes(),
             _pad8(p["classes"].numpy().tobytes()),
             _pad8(DeviceView(p["uniform"].ptr, (nu,), np.uint32).numpy().tobytes())]
    if splits is None:
        splits = [min(arena_chunks, nl - f) for f in range(0, nl, arena_chunks)]
    assert sum(splits) == nl and all(s >= 0 for s in splits)
    arena = DeviceArray((max(max(splits, default=0), 1), PACK_CHUNK), np.uint8)
    first = 0
    for count in splits:
        parts.append(pack_gather(buf, p, first, count, arena, stream).tobytes())
        first += count
    return b"".join(parts)


def unpack_buffer(record: bytes, dst: DeviceArray, arena_chunks: int = PACK_ARENA_CHUNKS, stream=None) -> DeviceArray:
    """Writes the buffer a packed record describes into dst (same byte size; whatever dst held is overwritten, nothing
    past it is touched).  Raises ValueError for a record that is inconsistent with itself or with dst."""
    assert isinstance(dst, DeviceArray) and not dst.padded
    mv = memoryview(record)
    if len(mv) < 24:
        raise ValueError("packed record: shorter than its header")
    nbytes = int(np.frombuffer(mv[:8], "<u8")[0])
    nchunks, nu, nl, zero = (int(v) for v in np.frombuffer(mv[8:24], "<u4"))
    if nbytes != dst.nbytes or nbytes % 4 or nchunks != (nbytes + PACK_CHUNK - 1) // PACK_CHUNK or zero:
        raise ValueError(f"packed record: header ({nbytes} bytes, {nchunks} chunks) does not describe a buffer of "
                         f"{dst.nbytes} bytes")
    o_cls, o_uni = 24, 24 + (nchunks + 7) // 8 * 8
    o_lit = o_uni + (4 * nu + 7) // 8 * 8
    if len(mv) != o_lit + nl * PACK_CHUNK:
        raise ValueError(f"packed record: {len(mv)} bytes, its header says {o_lit + nl * PACK_CHUNK}")
    cls = np.frombuffer(mv[o_cls:o_cls + nchunks], np.uint8)
    if int((cls == 1).sum()) != nu or int((cls == 2).sum()) != nl or int((cls > 2).sum()):
        raise ValueError("packed record: class array and counts disagree")
    p = dict(nbytes=nbytes, nchunks=nchunks, classes=DeviceArray.from_numpy(cls))
    _pack_rank(p, None, stream)
    assert (p["nuniform"], p["nliteral"]) == (nu, nl)
    uniform = DeviceArray.from_numpy(np.frombuffer(mv[o_uni:o_uni + 4 * nu], "<u4")) if nu else None
    check("emf_hip_unpackFill",
          _L.emf_hip_unpackFill(_ptr(dst), nbytes, _ptr(p["classes"]), _ptr(p["ranks"]), _ptr(uniform), nu,
                                _stream(stream)))
    for first in range(0, nl, arena_chunks):
        count = min(arena_chunks, nl - first)
        arena = DeviceArray.from_numpy(np.frombuffer(mv[o_lit + first * PACK_CHUNK:o_lit + (first + count) * PACK_CHUNK],
                                                     np.uint8))
        check("emf_hip_unpackLiterals",
              _L.emf_hip_unpackLiterals(_ptr(dst), nbytes, _ptr(p["literal_chunks"]), first, count, _ptr(arena),
                                        _stream(stream)))
        synchronize()  # the arena is freed when the loop moves on
    return dst


# ---- motion masks (include/emf_hip.h "Motion masks") ---------------------------------------------------------------

class MotionBuffers:
    """The scratch and the outputs of emf_hip_motionMasks for one frame size, reusable from call to call."""

    def __init__(self, width: int, height: int, max_masks: int = _lib.MOTION_MAX_MASKS):
        nbytes = int(_L.emf_hip_motionMasksScratchBytes(int(width), int(height), int(max_masks)))
        if nbytes == 0:
            raise ValueError(f"motion masks: {width} x {height} with {max_masks} masks is beyond the limits")
        self.width, self.height, self.max_masks = int(width), int(height), int(max_masks)
        self.scratch = DeviceArray.zeros(((nbytes + 3) // 4,), np.uint32)
        self.labels = DeviceArray.zeros((height, width), np.int32)
        self.masks = DeviceArray.zeros((max_masks, height, width), np.uint8)
        self.info = DeviceArray.zeros((max_masks, 6), np.int32)
        self.count = DeviceArray.zeros((1,), np.int32)


def motion_params(band=None, continuity=None, erode=None, min_pixels=None, max_masks=None) -> _lib.EmfMotionParams:
    """emf_motion_params_t with the documented defaults for whatever is None."""
    p = _lib.EmfMotionParams.defaults()
    for name, value in (("band", band), ("continuity", continuity), ("erode", erode), ("min_pixels", min_pixels),
                        ("max_masks", max_masks)):
        if value is not None:
            setattr(p, name, value)
    return p


def motion_info_dicts(info: np.ndarray, count: int):
    """Rows {label, area, x0, y0, x1, y1} of an info array as a list of dicts."""
    keys = ("label", "area", "x0", "y0", "x1", "y1")
    return [dict(zip(keys, (int(v) for v in row))) for row in np.asarray(info).reshape(-1, 6)[:count]]


def motion_masks(points, bg_raylengths, band=None, continuity=None, erode=None, min_pixels=None, max_masks=None,
                 buffers: Optional[MotionBuffers] = None, stream=None):
    """emf_hip_motionMasks: instance proposals from a points image (H, W, 3) f32 and the background's ray-length
    image (H, W) f32, numpy or dense device arrays.  Returns dict(labels (H, W) i32, masks (max_masks, H, W) u8,
    info (max_masks, 6) i32 rows {label, area, x0, y0, x1, y1}, count, proposals: the first `count` rows as dicts).
    `buffers` (MotionBuffers of the same size) are reused when given."""
    pts = _on_device(points, np.float32)
    bg = _on_device(bg_raylengths, np.float32)
    h, w = bg.shape
    assert pts.shape == (h, w, 3) and not pts.padded and not bg.padded, "dense (H, W, 3) points and (H, W) ray lengths"
    p = motion_params(band, continuity, erode, min_pixels, max_masks)
    if buffers is None:
        buffers = MotionBuffers(w, h, min(max(int(p.max_masks), 1), _lib.MOTION_MAX_MASKS))
    assert (buffers.width, buffers.height) == (w, h) and buffers.max_masks >= p.max_masks
    check("emf_hip_motionMasks",
          _L.emf_hip_motionMasks(_ptr(pts), _ptr(bg), w, h, C.byref(p), _ptr(buffers.scratch), _ptr(buffers.labels),
                                 _ptr(buffers.masks), _ptr(buffers.info), _ptr(buffers.count), _stream(stream)))
    count = int(buffers.count.numpy()[0])  # waits for the device: the inputs and the scratch may go after this
    info = buffers.info.numpy()[:p.max_masks]
    masks = buffers.masks.numpy().reshape(-1)[:p.max_masks * h * w].reshape(p.max_masks, h, w)
    return dict(labels=buffers.labels.numpy(), masks=masks, info=info, count=count,
                proposals=motion_info_dicts(info, count))


# ---- distance field (include/emf_hip.h "Distance field") -----------------------------------------

OCC_FREE, OCC_OCCUPIED, OCC_UNKNOWN = _lib.OCC_FREE, _lib.OCC_OCCUPIED, _lib.OCC_UNKNOWN
DF_FAR, DF_NONE = _lib.DF_FAR, _lib.DF_NONE


def _i3(values):
    return (C.c_int32 * 3)(*[int(v) for v in values])


def _box(res, box):
    """box None: the whole volume; else (lo, size), both (x, y, z) in voxels."""
    if box is None:
        return (0, 0, 0), tuple(int(v) for v in res)
    lo, size = box
    return tuple(int(v) for v in lo), tuple(int(v) for v in size)


def occupancy_objects(objects, res, voxel_size):
    """The emf_occ_object_t table of `objects` -- a sequence of (tsdf, weights, fg_mask or None, voxel_size, R, t)
    with (Nz, Ny, Nx) device volumes and (R, t) = object frame <- background volume frame -- each with the covering
    sub-box of a background of resolution res (x, y, z) and voxel size voxel_size (emf_hip_occupancyObjectBox)."""
    table = (_lib.EmfOccObject * max(len(objects), 1))()
    bres = _i3(res)
    for k, (tsdf, weights, fg_mask, vs, R, t) in enumerate(objects):
        o = table[k]
        _vol(tsdf, np.float32)
        assert weights.shape == tsdf.shape and (fg_mask is None or fg_mask.shape == tsdf.shape)
        o.tsdf, o.weights, o.fgVolMask = tsdf.ptr, weights.ptr, None if fg_mask is None else fg_mask.ptr
        o.res = _i3((tsdf.shape[2], tsdf.shape[1], tsdf.shape[0]))
        o.voxelSize = float(vs)
        o.R, o.t = _f(R, 9), _f(t, 3)
        check("emf_hip_occupancyObjectBox", _L.emf_hip_occupancyObjectBox(C.byref(o), bres, float(voxel_size)))
    return table


def stamp_objects(classes, res, voxel_size, objects, box=None, stream=None):
    """emf_hip_occupancyStampObjects on a (bz, by, bx) u8 class volume of the box `box` of a background of resolution
    res (x, y, z): OCCUPIED wherever an object is solid, nothing else written.  objects: see occupancy_objects, or a
    ready table of it (then with its length as (table, n))."""
    lo, size = _box(res, box)
    assert classes.dtype == np.uint8 and classes.shape == (size[2], size[1], size[0]) and not classes.padded
    table, n = objects if isinstance(objects, tuple) else (occupancy_objects(objects, res, voxel_size), len(objects))
    check("emf_hip_occupancyStampObjects",
          _L.emf_hip_occupancyStampObjects(_ptr(classes), _i3(res), float(voxel_size), _i3(lo), _i3(size),
                                           C.cast(table, C.c_void_p), int(n), _stream(stream)))
    return classes


def occupancy_classes(tsdf, weights, box=None, objects=None, voxel_size=None, out=None, stream=None):
    """emf_hip_occupancyClasses (+ emf_hip_occupancyStampObjects with `objects`): the (bz, by, bx) u8 classes --
    OCC_FREE / OCC_OCCUPIED / OCC_UNKNOWN -- of the box (lo, size), both (x, y, z), of (Nz, Ny, Nx) f32 tsdf / weights;
    box None: the whole volume.  objects: see occupancy_objects; they need the background's voxel_size."""
    _vol(tsdf, np.float32)
    assert weights.shape == tsdf.shape and weights.dtype == np.float32
    res = (tsdf.shape[2], tsdf.shape[1], tsdf.shape[0])
    lo, size = _box(res, box)
    shape = tuple(max(int(v), 0) for v in (size[2], size[1], size[0]))
    if out is None:
        out = DeviceArray(shape, np.uint8)
    assert out.dtype == np.uint8 and out.shape == shape and not out.padded
    check("emf_hip_occupancyClasses",
          _L.emf_hip_occupancyClasses(_ptr(tsdf), _ptr(weights), _i3(res), _i3(lo), _i3(size), _ptr(out), _stream(stream)))
    if objects:
        assert voxel_size is not None, "stamping objects needs the background's voxel_size"
        stamp_objects(out, res, voxel_size, objects, box=(lo, size), stream=stream)
    return out


def occupancy_tiles(tiles, box, stream=None):
    """emf_hip_occupancyTiles (include/emf_hip.h "Occupancy of a set of tiles"): the (bz, by, bx) u8
    classes of the box (lo, size), both (x, y, z) in LATTICE voxels -- lo may be negative, nothing needs to be aligned
    -- of the dense volume that holds exactly the listed tiles: OCC_UNKNOWN wherever no tile is listed.  tiles: the dict
    of mesh_tiles (its neighbours, if any, are not looked at).  Returns a numpy array."""
    coords = np.asarray(tiles["coords"]).reshape(-1, 3)
    n = int(coords.shape[0])
    table = mesh_tile_table(coords, tiles["classes"], tiles["words"], tiles["at"], np.full((n, 7), -1, np.int32))
    src = _lib.EmfMeshTilesSource()
    keep = []  # the uploads live until the synchronize below
    arena = tiles.get("arena")
    if arena is not None and np.asarray(arena).size:
        keep.append(DeviceArray.from_numpy(np.ascontiguousarray(arena, np.uint8).reshape(-1, TILE_UNIT)))
        src.arena, src.arena_units = keep[-1].ptr, keep[-1].nbytes // TILE_UNIT
    vol = tiles.get("volume")
    if vol is not None:
        nz, ny, nx = vol["tsdf"].shape
        keep.append(DeviceArray.from_numpy(np.ascontiguousarray(vol["tsdf"], np.float32)))
        keep.append(DeviceArray.from_numpy(np.ascontiguousarray(vol["weights"], np.float32)))
        src.tsdf, src.weights = keep[-2].ptr, keep[-1].ptr
        if vol.get("color") is not None:
            keep.append(DeviceArray.from_numpy(np.ascontiguousarray(vol["color"], np.uint16)))
            src.color = keep[-1].ptr
        src.volume_elements, src.row_stride, src.plane_stride = nz * ny * nx, nx, nx * ny
    d_table = DeviceArray.from_numpy(np.frombuffer(table, np.uint8).copy()) if n else None
    lo, size = box
    shape = tuple(max(int(v), 0) for v in (size[2], size[1], size[0]))
    out = DeviceArray(shape, np.uint8)
    check("emf_hip_occupancyTiles",
          _L.emf_hip_occupancyTiles(_ptr(d_table), C.cast(table, C.c_void_p), n, C.byref(src), _i3(lo), _i3(size), _ptr(out),
                                    _stream(stream)))
    synchronize()  # the uploads are released on return
    return out.numpy()


def distance_transform(classes, site_mask=2, cap=0, voxel_size=None, out=None, stream=None, nearest=False):
    """emf_hip_distanceTransform of a (nz, ny, nx) u8 class volume: d2 (nz, ny, nx) i32, the exact squared distance in
    voxels to the nearest voxel whose class bit is set in site_mask (1 FREE, 2 OCCUPIED, 4 UNKNOWN), DF_FAR where there
    is none or, with cap > 0 (voxels), beyond cap.  With voxel_size also metres (nz, ny, nx) f32, +inf where DF_FAR:
    returns d2, or (d2, metres).  out: (d2[, metres]) to reuse.
    nearest=True (emf_hip_distanceTransformNearest): also nearest (nz, ny, nx) i32, the linear index
    (z * ny + y) * nx + x of the nearest site -- the smallest one among equally near sites -- and DF_NONE exactly where
    d2 is DF_FAR: returns (d2, nearest) or (d2, metres, nearest); out then is (d2[, metres], nearest)."""
    assert classes.dtype == np.uint8 and len(classes.shape) == 3 and not classes.padded
    d2 = out[0] if out is not None else DeviceArray(classes.shape, np.int32)
    metres = None
    if voxel_size is not None:
        metres = out[1] if out is not None else DeviceArray(classes.shape, np.float32)
    assert d2.shape == classes.shape and d2.dtype == np.int32 and (metres is None or metres.shape == classes.shape)
    size, vs = _i3(classes.shape[::-1]), 0.0 if voxel_size is None else float(voxel_size)
    if not nearest:
        check("emf_hip_distanceTransform",
              _L.emf_hip_distanceTransform(_ptr(classes), size, int(site_mask), int(cap), _ptr(d2), _ptr(metres), vs,
                                           _stream(stream)))
        return d2 if metres is None else (d2, metres)
    index = out[-1] if out is not None else DeviceArray(classes.shape, np.int32)
    assert index.shape == classes.shape and index.dtype == np.int32 and not index.padded and index is not d2
    scratch = DeviceArray((max(int(_L.emf_hip_nearestSiteScratchBytes(size)), 16),), np.uint8)
    check("emf_hip_distanceTransformNearest",
          _L.emf_hip_distanceTransformNearest(_ptr(classes), size, int(site_mask), int(cap), _ptr(d2), _ptr(metres),
                                              _ptr(index), _ptr(scratch), vs, _stream(stream)))
    return (d2, index) if metres is None else (d2, metres, index)


def distance_query(voxels, classes=None, d2=None, nearest=None, stream=None):
    """emf_hip_distanceQuery: a gather of n voxels -- an (n, 3) list of (x, y, z) -- from the (nz, ny, nx) device arrays
    of a box, any of classes u8, d2 i32 and nearest i32 (at least one).  Returns a dict of numpy arrays with the keys of
    the arrays passed: "classes" (n,) u8, "d2" (n,) i32, "nearest" (n,) i32.  A voxel outside the box reads as 255,
    DF_FAR and DF_NONE."""
    given = {k: a for k, a in (("classes", classes), ("d2", d2), ("nearest", nearest)) if a is not None}
    assert given, "distance_query: no array to read"
    shape = next(iter(given.values())).shape
    for k, a in given.items():
        assert a.dtype == (np.uint8 if k == "classes" else np.int32) and a.shape == shape and len(shape) == 3 and not a.padded
    d_vox, n = _voxel_list(voxels, "distance_query")
    outs = {k: DeviceArray((n,), a.dtype) for k, a in given.items()}
    check("emf_hip_distanceQuery",
          _L.emf_hip_distanceQuery(_ptr(classes), _ptr(d2), _ptr(nearest), _i3(shape[::-1]), _ptr(d_vox), n,
                                   _ptr(outs.get("classes")), _ptr(outs.get("d2")), _ptr(outs.get("nearest")),
                                   _stream(stream)))
    return {k: o.numpy() for k, o in outs.items()}


def distance_field(tsdf, weights, voxel_size, box=None, objects=None, site_mask=2, cap=0, metres=True, stream=None):
    """occupancy_classes then distance_transform: (classes, d2, metres or None) of the box."""
    classes = occupancy_classes(tsdf, weights, box=box, objects=objects, voxel_size=voxel_size, stream=stream)
    r = distance_transform(classes, site_mask=site_mask, cap=cap, voxel_size=voxel_size if metres else None, stream=stream)
    return (classes, r[0], r[1]) if metres else (classes, r, None)


# ---- frontiers (include/emf_hip.h "Frontiers") ---------------------------------------------------

FRONTIER_KEPT, FRONTIER_CLUSTERS, FRONTIER_VOXELS = _lib.FRONTIER_KEPT, _lib.FRONTIER_CLUSTERS, _lib.FRONTIER_VOXELS
FRONTIER_CLUSTER_DTYPE = np.dtype(_lib.FRONTIER_CLUSTER_DTYPE)
assert FRONTIER_CLUSTER_DTYPE.itemsize == C.sizeof(_lib.EmfFrontierCluster) == 72


def frontier_labels(classes, d2=None, min_d2=0, out=None, stream=None):
    """emf_hip_frontierLabel of a (nz, ny, nx) u8 class volume: labels (nz, ny, nx) i32, the smallest linear index of
    the voxel's 26-connected cluster of frontier voxels (FREE with an UNKNOWN face neighbour inside the volume and,
    with d2 (nz, ny, nx) i32 and min_d2 > 0, d2 >= min_d2), -1 elsewhere.  labels.counters: u32 x 3 on the device,
    [FRONTIER_CLUSTERS] and [FRONTIER_VOXELS] written, [FRONTIER_KEPT] zero.  out: a labels array to reuse."""
    assert classes.dtype == np.uint8 and len(classes.shape) == 3 and not classes.padded
    assert d2 is None or (d2.dtype == np.int32 and d2.shape == classes.shape and not d2.padded)
    labels = out if out is not None else DeviceArray(classes.shape, np.int32)
    assert labels.shape == classes.shape and labels.dtype == np.int32 and not labels.padded
    if getattr(labels, "counters", None) is None:
        labels.counters = DeviceArray((3,), np.uint32)
    check("emf_hip_frontierLabel",
          _L.emf_hip_frontierLabel(_ptr(classes), _i3(classes.shape[::-1]), _ptr(d2), int(min_d2), _ptr(labels),
                                   _ptr(labels.counters), _stream(stream)))
    return labels


def frontier_clusters(labels, min_voxels=1, capacity=None, records=None, stream=None):
    """emf_hip_frontierClusters of what frontier_labels returned: (records, counts) -- records a numpy array of
    FRONTIER_CLUSTER_DTYPE, the clusters of at least min_voxels voxels in ascending label order, at most capacity of
    them (None: all); counts the three counters as a tuple (kept, clusters, voxels), always the full numbers.  Waits
    once for the number of clusters, which sizes the scratch, and once for the result.  records: a device array of
    capacity FRONTIER_CLUSTER_DTYPE entries to write into (then returned as it is instead of a numpy array)."""
    assert labels.dtype == np.int32 and len(labels.shape) == 3 and not labels.padded
    counters = labels.counters
    size = _i3(labels.shape[::-1])
    n_clusters = int(counters.numpy()[FRONTIER_CLUSTERS])
    cap = n_clusters if capacity is None else int(capacity)
    own = records is None
    if own:
        records = DeviceArray((max(cap, 0),), FRONTIER_CLUSTER_DTYPE)
    else:
        assert records.dtype == FRONTIER_CLUSTER_DTYPE and records.shape == (cap,)
    scratch = DeviceArray((max(int(_L.emf_hip_frontierScratchBytes(size, n_clusters)), 16),), np.uint8)
    check("emf_hip_frontierClusters",
          _L.emf_hip_frontierClusters(_ptr(labels), size, int(min_voxels), n_clusters, _ptr(scratch),
                                      _ptr(records) if cap > 0 else None, cap, _ptr(counters), _stream(stream)))
    counts = tuple(int(v) for v in counters.numpy())
    if not own:
        return records, counts
    return records.numpy()[:min(counts[FRONTIER_KEPT], max(cap, 0))], counts


def frontiers(classes, d2=None, min_d2=0, min_voxels=1, capacity=None, stream=None):
    """frontier_labels then frontier_clusters: (labels, records, (kept, clusters, voxels))."""
    labels = frontier_labels(classes, d2=d2, min_d2=min_d2, stream=stream)
    records, counts = frontier_clusters(labels, min_voxels=min_voxels, capacity=capacity, stream=stream)
    return labels, records, counts


# ---- planning (include/emf_hip.h "Planning") -----------------------------------------------------

PLAN_UNREACHED, PLAN_BLOCKED = _lib.PLAN_UNREACHED, _lib.PLAN_BLOCKED
PLAN_CONVERGED, PLAN_ROUNDS, PLAN_FINITE, PLAN_SEEDS = _lib.PLAN_CONVERGED, _lib.PLAN_ROUNDS, _lib.PLAN_FINITE, _lib.PLAN_SEEDS


def _voxel_list(points, what):
    """An (n, 3) list of (x, y, z) voxels as a device array of i32."""
    v = np.ascontiguousarray(np.asarray(points, np.int32).reshape(-1, 3))
    assert len(v) >= 1, f"{what}: an empty list"
    return DeviceArray.from_numpy(v.reshape(-1)), len(v)


def plan_cost(classes, seeds, d2=None, min_d2=0, traverse_mask=1, seed_radius=0, max_cost=0, max_rounds=0, out=None,
              stream=None):
    """emf_hip_planCost of a (nz, ny, nx) u8 class volume: the cost-to-go field (nz, ny, nx) u32 from the seeds -- an
    (n, 3) list of (x, y, z) voxels -- through the traversable voxels: those whose class is in traverse_mask (bit
    1 << class) and, with d2 (nz, ny, nx) i32 and min_d2 > 0, d2 >= min_d2, plus whatever is not occupied within
    seed_radius voxels of a used seed.  26-connected moves of weight 3 / 4 / 5; 0 at a used seed, PLAN_UNREACHED where
    no seed reaches or the cost exceeds max_cost (> 0), PLAN_BLOCKED off the traversable set.  cost.counters: u32 x 4 on
    the device, [converged, rounds enqueued, voxels with a finite cost, seeds used].  Waits on the stream, once per
    batch of rounds.  out: a cost array to reuse."""
    assert classes.dtype == np.uint8 and len(classes.shape) == 3 and not classes.padded
    assert d2 is None or (d2.dtype == np.int32 and d2.shape == classes.shape and not d2.padded)
    cost = out if out is not None else DeviceArray(classes.shape, np.uint32)
    assert cost.shape == classes.shape and cost.dtype == np.uint32 and not cost.padded
    if getattr(cost, "counters", None) is None:
        cost.counters = DeviceArray((4,), np.uint32)
    size = _i3(classes.shape[::-1])
    d_seeds, n_seeds = _voxel_list(seeds, "plan_cost")
    scratch = DeviceArray((max(int(_L.emf_hip_planScratchBytes(size)), 16),), np.uint8)
    check("emf_hip_planCost",
          _L.emf_hip_planCost(_ptr(classes), size, _ptr(d2), int(min_d2), int(traverse_mask), _ptr(d_seeds),
                              n_seeds, int(seed_radius), int(max_cost), int(max_rounds), _ptr(cost),
                              _ptr(scratch), _ptr(cost.counters), _stream(stream)))
    return cost


def plan_paths(cost, goals, capacity=None, paths=None, lengths=None, goal_cost=None, stream=None):
    """emf_hip_planPaths over what plan_cost returned: (paths, lengths, goal_cost) as numpy arrays -- paths (n, capacity)
    i32 linear indices (z * ny + y) * nx + x, the goal first, each step to the neighbour the cost came from (ties: the
    smallest index), valid up to min(length, capacity); lengths (n,) i32, 0 for a goal that is unreached, blocked or
    out of the box; goal_cost (n,) u32.  capacity None: the longest path (one more call after the lengths are known).
    paths / lengths / goal_cost: device arrays to write into, returned as they are."""
    assert cost.dtype == np.uint32 and len(cost.shape) == 3 and not cost.padded
    size = _i3(cost.shape[::-1])
    d_goals, n = _voxel_list(goals, "plan_paths")
    own = paths is None and lengths is None and goal_cost is None
    lengths = lengths if lengths is not None else DeviceArray((n,), np.int32)
    goal_cost = goal_cost if goal_cost is not None else DeviceArray((n,), np.uint32)

    def run(cap, sink):
        check("emf_hip_planPaths",
              _L.emf_hip_planPaths(_ptr(cost), size, _ptr(d_goals), n, cap, _ptr(sink) if cap > 0 else None, _ptr(lengths),
                                   _ptr(goal_cost), _stream(stream)))

    if capacity is None:
        assert paths is None
        run(0, None)
        capacity = int(np.abs(lengths.numpy()).max(initial=0))
    capacity = int(capacity)
    if paths is None:
        paths = DeviceArray((n, max(capacity, 1)), np.int32)
        if capacity == 0:
            paths = None
    run(capacity, paths)
    if not own:
        return paths, lengths, goal_cost
    host = paths.numpy()[:, :capacity] if paths is not None else np.zeros((n, 0), np.int32)
    return host, lengths.numpy(), goal_cost.numpy()


def plan(classes, seeds, goals, capacity=None, **kwargs):
    """plan_cost then plan_paths: (cost, paths, lengths, goal_cost)."""
    stream = kwargs.get("stream")
    cost = plan_cost(classes, seeds, **kwargs)
    paths, lengths, goal_cost = plan_paths(cost, goals, capacity=capacity, stream=stream)
    return cost, paths, lengths, goal_cost


# ---- voxel rays (include/emf_hip.h "Voxel rays") -------------------------------------------------

RAY_MAX_DELTA = _lib.RAY_MAX_DELTA
RAY_REACHED, RAY_BLOCKED, RAY_LEFT, RAY_OUTSIDE, RAY_INVALID = (_lib.RAY_REACHED, _lib.RAY_BLOCKED, _lib.RAY_LEFT,
                                                                _lib.RAY_OUTSIDE, _lib.RAY_INVALID)
RAY_RESULT_DTYPE = np.dtype(_lib.RAY_RESULT_DTYPE)
RAY_GROUP_DTYPE = np.dtype(_lib.RAY_GROUP_DTYPE)
assert RAY_RESULT_DTYPE.itemsize == 24 and RAY_GROUP_DTYPE.itemsize == 32


def _ray_ends(points, what):
    """(n, 3) voxels (x, y, z) as a device array of 3 * n i32: a device array goes through as it is."""
    if isinstance(points, DeviceArray):
        assert points.dtype == np.int32 and not points.padded and int(np.prod(points.shape)) % 3 == 0, what
        return points, int(np.prod(points.shape)) // 3
    v = np.ascontiguousarray(np.asarray(points, np.int32).reshape(-1, 3))
    return DeviceArray.from_numpy(v.reshape(-1)), len(v)


def cast_voxel_rays(classes, rays_from, rays_to, d2=None, min_d2=0, pass_mask=1, count_mask=0, group=0, out=None,
                    stream=None):
    """emf_hip_castVoxelRays over a (nz, ny, nx) u8 class volume: n rays from rays_from to rays_to -- (n, 3) lists of
    (x, y, z) voxels, numpy or device i32 -- each an integer walk of |dx| + |dy| + |dz| face steps (the next step along
    the axis with the smallest crossing parameter (2 i + 1) / (2 d), ties x before y before z; NOT symmetric in its
    ends) that ends at the first voxel that is outside the volume, whose class bit is not in pass_mask or, with d2
    (nz, ny, nx) i32 and min_d2 > 0, whose d2 < min_d2.  The origin is never tested.  Returns the records, a numpy
    array of RAY_RESULT_DTYPE (stop: linear index of the blocking voxel or DF_NONE; steps; counted: passed voxels whose
    class bit is in count_mask; status RAY_*; weighted: the sum of |v - origin|^2 over the counted voxels), and with
    group > 0 the pair (records, groups): one RAY_GROUP_DTYPE record per run of `group` consecutive rays, the last one
    may be short.  out: (results, groups) device arrays of at least n and ceil(n / group) records to write into, either
    may be None (results None with groups: only the groups are computed); they are returned as they are."""
    assert classes.dtype == np.uint8 and len(classes.shape) == 3 and not classes.padded
    assert d2 is None or (d2.dtype == np.int32 and d2.shape == classes.shape and not d2.padded)
    d_from, n = _ray_ends(rays_from, "cast_voxel_rays: rays_from")
    d_to, n_to = _ray_ends(rays_to, "cast_voxel_rays: rays_to")
    assert n == n_to, "cast_voxel_rays: as many origins as targets"
    group = int(group)
    n_groups = -(-n // group) if group > 0 else 0
    if out is None:
        results = DeviceArray((n,), RAY_RESULT_DTYPE)
        groups = DeviceArray((n_groups,), RAY_GROUP_DTYPE) if group > 0 else None
    else:
        results, groups = out
        assert results is None or (results.dtype == RAY_RESULT_DTYPE and results.shape[0] >= n)
        assert groups is None or (groups.dtype == RAY_GROUP_DTYPE and groups.shape[0] >= n_groups)
    check("emf_hip_castVoxelRays",
          _L.emf_hip_castVoxelRays(_ptr(classes), _i3(classes.shape[::-1]), _ptr(d2), int(min_d2), int(pass_mask),
                                   int(count_mask), _ptr(d_from), _ptr(d_to), n, _ptr(results), group, _ptr(groups),
                                   _stream(stream)))
    if out is not None:
        return results, groups
    return (results.numpy(), groups.numpy()) if group > 0 else results.numpy()


# ---- object shapes (include/emf_hip.h "Object shapes") -------------------------------------------

SHAPE_MOMENTS_DTYPE = np.dtype(_lib.SHAPE_MOMENTS_DTYPE)
SHAPE_AXES_DTYPE = np.dtype(_lib.SHAPE_AXES_DTYPE)
SHAPE_EXTENTS_DTYPE = np.dtype(_lib.SHAPE_EXTENTS_DTYPE)
assert SHAPE_MOMENTS_DTYPE.itemsize == C.sizeof(_lib.EmfShapeMoments) == 128
assert SHAPE_AXES_DTYPE.itemsize == C.sizeof(_lib.EmfShapeAxes) == 48
assert SHAPE_EXTENTS_DTYPE.itemsize == C.sizeof(_lib.EmfShapeExtents) == 24


def shape_table(volumes, first=0):
    """The device model table of shape_moments / shape_extents -- only what they read: tsdf, weights, fg_mask,
    unseen_tiles (optional, as rebuild_unseen_tiles leaves it) and the resolution -- with `first` empty slots in front,
    and the host resolutions of the volumes."""
    n = len(volumes)
    models = [_lib.EmfModel() for _ in range(first)]
    res = (C.c_int32 * (3 * max(n, 1)))()
    for k, v in enumerate(volumes):
        tsdf = _vol(v["tsdf"], np.float32)
        m = _lib.EmfModel()
        m.tsdf, m.weights = tsdf.ptr, _vol(v["weights"], np.float32).ptr
        assert v["weights"].shape == tsdf.shape
        if v.get("fg_mask") is not None:
            assert v["fg_mask"].shape == tsdf.shape
            m.fgVolMask = _vol(v["fg_mask"], np.uint8).ptr
        if v.get("unseen_tiles") is not None:
            m.unseenTiles = v["unseen_tiles"].ptr
        nz, ny, nx = tsdf.shape
        m.res[:] = [nx, ny, nz]
        res[3 * k:3 * k + 3] = [nx, ny, nz]
        models.append(m)
    return (upload_models(models) if models else None), res


def shape_moments(volumes, first=0, out=None, stream=None):
    """emf_hip_shapeMoments: the integer moments of the OBSERVED SOLID BAND of every volume of a table in one launch --
    a TSDF observes a band around the surface, so this is not the body and no volume in cubic metres.  volumes:
    [dict(tsdf=, weights=, fg_mask=None, unseen_tiles=None), ...] of device arrays, as extract_meshes takes them; they
    occupy the table slots [first, first + n), first + n <= EMF_MAX_MODELS.  A voxel is solid where weights > 0, the
    mask (if any) is non-zero and not tsdf > 0.  Returns a numpy array of n SHAPE_MOMENTS_DTYPE records (solid,
    observed, sum, sum2 = xx yy zz xy xz yz, faces_free, faces_unknown, lo, hi), or with out= (a device array of at
    least n such records) that array."""
    n = len(volumes)
    table, res = shape_table(volumes, first)
    records = DeviceArray((max(n, 1),), SHAPE_MOMENTS_DTYPE) if out is None else out
    assert records.dtype == SHAPE_MOMENTS_DTYPE and records.shape[0] >= n
    check("emf_hip_shapeMoments", _L.emf_hip_shapeMoments(_ptr(table), res, int(first), n, _ptr(records), _stream(stream)))
    return records.numpy()[:n] if out is None else out


def shape_extents(volumes, frames, first=0, out=None, stream=None):
    """emf_hip_shapeExtents: minimum and maximum, over the solid voxels v of every volume of a table, of
    e_k = A_k0 p_0 + A_k1 p_1 + A_k2 p_2 with p = float(v) - c, each a single float32 operation, in one launch.
    frames: n SHAPE_AXES_DTYPE records (A: three row vectors, c: the centre, voxel coordinates), numpy or device.
    Returns a numpy array of n SHAPE_EXTENTS_DTYPE records (+inf / -inf for a volume without a solid voxel), or with
    out= (a device array of at least n such records) that array."""
    n = len(volumes)
    table, res = shape_table(volumes, first)
    if not isinstance(frames, DeviceArray):
        frames = DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(frames, SHAPE_AXES_DTYPE).reshape(-1)))
    assert frames.dtype == SHAPE_AXES_DTYPE and frames.shape[0] >= n
    records = DeviceArray((max(n, 1),), SHAPE_EXTENTS_DTYPE) if out is None else out
    assert records.dtype == SHAPE_EXTENTS_DTYPE and records.shape[0] >= n
    check("emf_hip_shapeExtents",
          _L.emf_hip_shapeExtents(_ptr(table), res, int(first), n, _ptr(frames), _ptr(records), _stream(stream)))
    return records.numpy()[:n] if out is None else out


# ---- object contacts (include/emf_hip.h "Object contacts") ---------------------------------------

CONTACT_PAIR_DTYPE = np.dtype(_lib.CONTACT_PAIR_DTYPE)
CONTACT_DTYPE = np.dtype(_lib.CONTACT_DTYPE)
assert CONTACT_PAIR_DTYPE.itemsize == 64 and CONTACT_DTYPE.itemsize == 144


def contact_table(volumes):
    """The device model table of contact_probe -- shape_table's plus the voxel size of every volume
    (dict(tsdf=, weights=, voxel_size=, fg_mask=None, unseen_tiles=None)) -- and the host resolutions."""
    models, n = [], len(volumes)
    res = (C.c_int32 * (3 * max(n, 1)))()
    for k, v in enumerate(volumes):
        tsdf = _vol(v["tsdf"], np.float32)
        m = _lib.EmfModel()
        m.tsdf, m.weights = tsdf.ptr, _vol(v["weights"], np.float32).ptr
        assert v["weights"].shape == tsdf.shape
        if v.get("fg_mask") is not None:
            assert v["fg_mask"].shape == tsdf.shape
            m.fgVolMask = _vol(v["fg_mask"], np.uint8).ptr
        if v.get("unseen_tiles") is not None:
            m.unseenTiles = v["unseen_tiles"].ptr
        nz, ny, nx = tsdf.shape
        m.res[:] = [nx, ny, nz]
        m.voxelSize = float(np.float32(v["voxel_size"]))
        res[3 * k:3 * k + 3] = [nx, ny, nz]
        models.append(m)
    return (upload_models(models) if models else None), res


def contact_pairs(pairs):
    """A list of (a, b, R, t, touch) -- or an array of CONTACT_PAIR_DTYPE -- as a contiguous array of CONTACT_PAIR_DTYPE."""
    if isinstance(pairs, np.ndarray) and pairs.dtype == CONTACT_PAIR_DTYPE:
        return np.ascontiguousarray(pairs.reshape(-1))
    out = np.zeros(len(pairs), CONTACT_PAIR_DTYPE)
    for k, (a, b, R, t, touch) in enumerate(pairs):
        out[k]["a"], out[k]["b"] = int(a), int(b)
        out[k]["R"] = np.asarray(R, np.float32).reshape(9)
        out[k]["t"] = np.asarray(t, np.float32).reshape(3)
        out[k]["touch"] = np.float32(touch)
    return out


def contact_probe(volumes, pairs, out=None, stream=None, lib=None):
    """emf_hip_contactProbe: for every ordered pair (probe a, field b) of `pairs` -- (a, b, R, t, touch) with a, b indices
    into `volumes`, R, t taking a's frame into b's and touch in units of b's stored tsdf -- the surface voxels of a are
    taken into b's volume and b's tsdf is sampled there trilinearly, in one launch for the whole list.  Returns a numpy
    array of CONTACT_DTYPE records, one per pair in the list's order (surface = outside + unknown + masked + sampled;
    inside, touching, normals; sum, gsum, lo, hi of the touching voxels; min_s), or with out= (a device array of at
    least that many records) that array.  IT MEASURES WHAT THE VOLUMES SAY: min_s == 1 means "at least one truncation
    distance apart", a penetration deeper than the fused band reads unknown, and a clearance reads up to one probe voxel
    large.  A list grouped by probe is the fast one; any order gives the same bytes.  lib: another build of the kernel
    library (_lib.load_variant)."""
    L = _L if lib is None else lib
    table, res = contact_table(volumes)
    host = contact_pairs(pairs)
    n = len(host)
    d_pairs = DeviceArray.from_numpy(host if n else np.zeros(1, CONTACT_PAIR_DTYPE))
    records = DeviceArray((max(n, 1),), CONTACT_DTYPE) if out is None else out
    assert records.dtype == CONTACT_DTYPE and records.shape[0] >= n
    check("emf_hip_contactProbe",
          L.emf_hip_contactProbe(_ptr(table), res, len(volumes), _ptr(d_pairs), C.c_void_p(host.ctypes.data), n, _ptr(records),
                                 _stream(stream)))
    return records.numpy()[:n] if out is None else out


# ---- absorbing a volume (include/emf_hip.h "Absorbing a volume") -----------------------------------

ABSORB_DTYPE = np.dtype(_lib.ABSORB_DTYPE)
COLOR_MOVED_DTYPE = np.dtype(_lib.COLOR_MOVED_DTYPE)
assert ABSORB_DTYPE.itemsize == 88 and C.sizeof(_lib.EmfAbsorbSource) == 56 and COLOR_MOVED_DTYPE.itemsize == 16


def absorb_box(dst_res, dst_voxel_size, src_res, src_voxel_size, pose):
    """The covering box (lo, size), both (x, y, z), of a whole source in a destination of resolution dst_res (x, y, z):
    emf_hip_occupancyObjectBox of the source's corners through the inverse of pose = (R, t), source frame <-
    destination frame.  A source that misses the destination gives a size of 0."""
    o = _lib.EmfOccObject()
    o.res = _i3(src_res)
    o.voxelSize = float(src_voxel_size)
    o.R, o.t = _f(pose[0], 9), _f(pose[1], 3)
    check("emf_hip_occupancyObjectBox", _L.emf_hip_occupancyObjectBox(C.byref(o), _i3(dst_res), float(dst_voxel_size)))
    return tuple(o.lo), tuple(o.size)


def _transfer_call(dst, other_res, other_voxel_size, pose, box, out, dtype):
    """What the passes over a box of `dst` share: the destination's arguments (tsdf, weights, res, voxel size), the box
    (lo, size) -- None: the covering box of the whole other volume (absorb_box) -- and the record array."""
    tsdf, weights = _vol(dst["tsdf"], np.float32), _vol(dst["weights"], np.float32)
    assert weights.shape == tsdf.shape
    res = (tsdf.shape[2], tsdf.shape[1], tsdf.shape[0])
    if box is None:
        box = absorb_box(res, dst["voxel_size"], other_res, other_voxel_size, pose)
    lo, size = _box(res, box)
    record = DeviceArray((1,), dtype) if out is None else out
    assert record.dtype == dtype and record.shape[0] >= 1
    return (_ptr(tsdf), _ptr(weights), _i3(res), float(np.float32(dst["voxel_size"]))), (_i3(lo), _i3(size)), record


def _transfer_color(dst, color_out):
    """The colour arguments of a pass into a destination with a colour volume (dst["color"], (Nz, Ny, Nx, 4) u16): its
    pointer and the colour record array; (None, None) for a destination without one -- the plain entry."""
    if dst.get("color") is None:
        assert color_out is None, "a colour record without a colour volume"
        return None, None
    color = _vol(dst["color"], np.uint16, 4)
    assert color.shape[:3] == dst["tsdf"].shape
    crec = DeviceArray((1,), COLOR_MOVED_DTYPE) if color_out is None else color_out
    assert crec.dtype == COLOR_MOVED_DTYPE and crec.shape[0] >= 1
    return color, crec


def _transfer_result(record, out, crec, color_out):
    """The record of a plain pass; (record, colour record) of a colour pass; numpy records, or the arrays given."""
    rec = record.numpy()[0] if out is None else out
    if crec is None:
        return rec
    return rec, (crec.numpy()[0] if color_out is None else color_out)


def _transfer_volume(entry, dtype, dst, src, pose, box, out, lib, stream, color_out=None, counts=None):
    """absorb_volume, seed_volume and merge_volume: emf_hip_<entry> of a whole source into dst; emf_hip_<entry>Color where
    dst has a colour volume.  counts (merge_volume alone): (counts_out,) -- the call takes dst["fgbg"] and src["fgbg"],
    (Nz, Ny, Nx, 2) f32, behind the weights and the source, and the count record behind the record."""
    stsdf, sweights = _vol(src["tsdf"], np.float32), _vol(src["weights"], np.float32)
    assert sweights.shape == stsdf.shape
    s = _lib.EmfAbsorbSource()
    s.tsdf, s.weights = stsdf.ptr, sweights.ptr
    if src.get("fg_mask") is not None:
        assert src["fg_mask"].shape == stsdf.shape
        s.fgVolMask = _vol(src["fg_mask"], np.uint8).ptr
    if src.get("unseen_tiles") is not None:
        s.unseenTiles = src["unseen_tiles"].ptr
    s.res = _i3((stsdf.shape[2], stsdf.shape[1], stsdf.shape[0]))
    s.voxelSize, s.truncdist = float(np.float32(src["voxel_size"])), float(np.float32(src["truncdist"]))
    d, b, record = _transfer_call(dst, tuple(s.res), src["voxel_size"], pose, box, out, dtype)
    color, crec = _transfer_color(dst, color_out)
    arrays, source, records = [d[0], d[1]], [C.byref(s)], [_ptr(record)]
    cnt = None
    if counts is not None:
        dfgbg, sfgbg = _vol(dst["fgbg"], np.float32, 2), _vol(src["fgbg"], np.float32, 2)
        assert dfgbg.shape[:3] == dst["tsdf"].shape and sfgbg.shape[:3] == stsdf.shape
        cnt = DeviceArray((1,), MERGE_COUNTS_DTYPE) if counts[0] is None else counts[0]
        assert cnt.dtype == MERGE_COUNTS_DTYPE and cnt.shape[0] >= 1
        arrays.append(_ptr(dfgbg)), source.append(_ptr(sfgbg)), records.append(_ptr(cnt))
    if color is not None:
        scolor = src.get("color")
        if scolor is not None:
            assert _vol(scolor, np.uint16, 4).shape[:3] == stsdf.shape
        arrays.append(_ptr(color)), source.append(_ptr(scolor)), records.append(_ptr(crec))
        entry += "Color"
    check("emf_hip_" + entry,
          getattr(_L if lib is None else lib, "emf_hip_" + entry)(
              *arrays, d[2], d[3], float(np.float32(dst["truncdist"])), float(np.float32(dst["max_weight"])), *source, _f(pose[0], 9),
              _f(pose[1], 3), *b, *records, _stream(stream)))
    result = _transfer_result(record, out, crec, color_out)
    if counts is None:
        return result
    cnt = cnt.numpy()[0] if counts[0] is None else cnt
    return (result, cnt) if crec is None else (result[0], cnt, result[1])


def absorb_volume(dst, src, pose, box=None, out=None, lib=None, stream=None, color_out=None):
    """emf_hip_absorbVolume: the signed-distance band of `src` resampled through pose = (R, t) (f32, source frame <-
    destination frame) into `dst` and fused there, in place, by dst's running average.
    dst: dict(tsdf=, weights=, voxel_size=, truncdist=, max_weight=), (Nz, Ny, Nx) f32 device arrays of any shape from
    (1, 1, 1); src: dict(tsdf=, weights=, voxel_size=, truncdist=, fg_mask=None, unseen_tiles=None), only read.
    box: (lo, size) in destination voxels, (x, y, z); None: the covering box of the whole source (absorb_box).
    Returns the record (a 0-d numpy array of ABSORB_DTYPE: visited = outside + unknown + masked + saturated + fused;
    fresh, solid; lo, hi of the fused voxels), or with out= (a device array of at least one record) that array.
    IT CARRIES THE BAND, NOT THE FREE SPACE AROUND IT: saturated source samples are left alone.  lib: another build of
    the kernel library (_lib.load_variant).
    COLOUR: with dst["color"] (an (Nz, Ny, Nx, 4) u16 device colour volume) the call is
    emf_hip_absorbVolumeColor -- the same tsdf, weights and record, and the colour entry of every fused voxel blended
    with the entry of src["color"] (or None: no source colour) at the nearest source voxel -- and returns the pair
    (record, colour record), the second of COLOR_MOVED_DTYPE (colored + uncolored == fused), or with color_out= (a device
    array of at least one such record) that array in its place.  Without dst["color"] the call is what it was."""
    return _transfer_volume("absorbVolume", ABSORB_DTYPE, dst, src, pose, box, out, lib, stream, color_out)


# ---- merging a volume (include/emf_hip.h "Merging a volume") ---------------------------------------

MERGE_COUNTS_DTYPE = np.dtype(_lib.MERGE_COUNTS_DTYPE)
assert MERGE_COUNTS_DTYPE.itemsize == 16


def merge_volume(dst, src, pose, box=None, out=None, lib=None, stream=None, counts_out=None, color_out=None):
    """emf_hip_mergeVolume: absorb_volume into an OBJECT -- dst and src as there, each with fgbg= as well, a (Nz, Ny, Nx, 2)
    f32 device volume of interleaved (fg, bg) counts, and src["fg_mask"] required.  tsdf, weights and the record are
    absorb_volume's byte for byte; the count pair of every fused voxel becomes the source's pair at the nearest source
    voxel where the voxel had no observation, and the sum of both otherwise.  Returns (record, counts), counts a 0-d numpy
    array of MERGE_COUNTS_DTYPE (foreground: fused voxels whose new pair has fg > bg; gained: those of them that did not
    before), or with out= / counts_out= (device arrays of at least one record) those arrays in their places.
    With dst["color"]: emf_hip_mergeVolumeColor -- the colour entries as absorb_volume carries them -- and the triple
    (record, counts, colour record); color_out= as there."""
    return _transfer_volume("mergeVolume", ABSORB_DTYPE, dst, src, pose, box, out, lib, stream, color_out, counts=(counts_out,))


# ---- lifting a volume (include/emf_hip.h "Lifting a volume") ---------------------------------------

SEED_DTYPE = np.dtype(_lib.SEED_DTYPE)
RELEASE_DTYPE = np.dtype(_lib.RELEASE_DTYPE)
assert SEED_DTYPE.itemsize == 88 and RELEASE_DTYPE.itemsize == 80


def seed_volume(dst, src, pose, box=None, out=None, lib=None, stream=None, color_out=None):
    """emf_hip_seedVolume: `dst` takes the signed-distance band of `src`, resampled through pose = (R, t) (f32, source
    frame <- destination frame), ONLY WHERE IT HAS NO OBSERVATION OF ITS OWN (weights not > 0), in place, and only values
    inside its own band: no clamped +-1 is written.  dst, src, box and out as in absorb_volume (box None: the covering
    box of the whole source).  Returns the record (a 0-d numpy array of SEED_DTYPE: visited = kept + outside + unknown +
    masked + saturated + seeded; solid; lo, hi of the seeded voxels), or with out= that array.
    With dst["color"]: emf_hip_seedVolumeColor -- every seeded voxel takes the entry of src["color"] (or None) at the
    nearest source voxel, its weight capped, or (0, 0, 0, 0) -- and the pair (record, colour record) as absorb_volume."""
    return _transfer_volume("seedVolume", SEED_DTYPE, dst, src, pose, box, out, lib, stream, color_out)


def release_volume(dst, claim, pose, box=None, out=None, lib=None, stream=None, color_out=None):
    """emf_hip_releaseVolume: `dst` gives up, in place, the band voxels (weights > 0, |tsdf| < 1) that the claimant holds:
    tsdf and weights become +0.0.  dst: dict(tsdf=, weights=, voxel_size=); claim: dict(fg_mask=, voxel_size=) with a
    (Nz, Ny, Nx) u8 device volume, or dict(fg_mask=None, res=(nx, ny, nz), voxel_size=): everything inside the
    claimant's cube; pose = (R, t), claimant frame <- destination frame.  box: (lo, size) in destination voxels, None: the
    covering box of the claimant's cube (absorb_box).  Returns the record (RELEASE_DTYPE: visited = empty + free_space +
    outside + unclaimed + released; solid; lo, hi of the released voxels), or with out= that array.
    With dst["color"]: emf_hip_releaseVolumeColor -- the colour entry of every released voxel becomes (0, 0, 0, 0) -- and
    the pair (record, colour record) as absorb_volume (colored: the entries that held something)."""
    L = _L if lib is None else lib
    mask = claim.get("fg_mask")
    if mask is not None:
        mask = _vol(mask, np.uint8)
        cres = (mask.shape[2], mask.shape[1], mask.shape[0])
        assert claim.get("res") is None or tuple(int(v) for v in claim["res"]) == cres
    else:
        cres = tuple(int(v) for v in claim["res"])
    d, b, record = _transfer_call(dst, cres, claim["voxel_size"], pose, box, out, RELEASE_DTYPE)
    color, crec = _transfer_color(dst, color_out)
    if color is None:
        check("emf_hip_releaseVolume",
              L.emf_hip_releaseVolume(*d, _ptr(mask), _i3(cres), float(np.float32(claim["voxel_size"])), _f(pose[0], 9),
                                      _f(pose[1], 3), *b, _ptr(record), _stream(stream)))
    else:
        check("emf_hip_releaseVolumeColor",
              L.emf_hip_releaseVolumeColor(d[0], d[1], _ptr(color), d[2], d[3], _ptr(mask), _i3(cres),
                                           float(np.float32(claim["voxel_size"])), _f(pose[0], 9), _f(pose[1], 3), *b, _ptr(record),
                                           _ptr(crec), _stream(stream)))
    return _transfer_result(record, out, crec, color_out)


# ---- ground map (include/emf_hip.h "Ground map") -------------------------------------------------

GROUND_CELL_DTYPE = np.dtype(_lib.GROUND_CELL_DTYPE)
GROUND_MAX_BINS = _lib.GROUND_MAX_BINS
GroundFrame = _lib.EmfGroundFrame
assert GROUND_CELL_DTYPE.itemsize == 8 and C.sizeof(GroundFrame) == 60


def ground_frame(G, map_size, bins):
    """The emf_ground_frame_t of a 3 x 4 map G (box voxel -> u in cells, v in cells, h in bins; rounded to f32 here
    unless it is f32 already), map_size = (W, H) and `bins` height bins.  A GroundFrame passes through."""
    if isinstance(G, GroundFrame):
        return G
    f = GroundFrame()
    f.G = _f(G, 12)
    f.map[:] = [int(map_size[0]), int(map_size[1])]
    f.bins = int(bins)
    return f


def _ground_words(bins):
    return (int(bins) + 63) // 64


def ground_columns(classes, frame, out=None, stream=None):
    """emf_hip_groundColumns: the two bit planes (occ, fre), each (H, W, words) u64 with words = (bins + 63) // 64, of a
    (nz, ny, nx) u8 class volume under `frame` (a GroundFrame, see ground_frame).  Bit h & 63 of word h >> 6 of cell
    (v, u) is set in occ where an OCCUPIED voxel falls into slot (u, v, h), in fre where a FREE one does; every voxel
    counts.  The planes are zeroed by the call.  out: (occ, fre) to reuse."""
    assert classes.dtype == np.uint8 and len(classes.shape) == 3 and not classes.padded
    assert isinstance(frame, GroundFrame)
    shape = (max(frame.map[1], 1), max(frame.map[0], 1), max(_ground_words(frame.bins), 1))
    occ, fre = out if out is not None else (DeviceArray(shape, np.uint64), DeviceArray(shape, np.uint64))
    for p in (occ, fre):
        assert p.dtype == np.uint64 and not p.padded and p.shape == shape
    check("emf_hip_groundColumns",
          _L.emf_hip_groundColumns(_ptr(classes), _i3(classes.shape[::-1]), frame, _ptr(occ), _ptr(fre), _stream(stream)))
    return occ, fre


def ground_cells(occ, fre, bins, robot_bins, out=None, stream=None):
    """emf_hip_groundCells: the (H, W) GROUND_CELL_DTYPE records (floor, top, clear, levels) of the (H, W, words) planes
    of ground_columns for a robot of robot_bins >= 1 bins.  out: a records array to reuse."""
    assert occ.dtype == np.uint64 and fre.dtype == np.uint64 and occ.shape == fre.shape and len(occ.shape) == 3
    H, W = occ.shape[0], occ.shape[1]
    cells = DeviceArray((H, W), GROUND_CELL_DTYPE) if out is None else out
    assert cells.dtype == GROUND_CELL_DTYPE and cells.shape == (H, W) and not cells.padded
    check("emf_hip_groundCells",
          _L.emf_hip_groundCells(_ptr(occ), _ptr(fre), (C.c_int32 * 2)(W, H), int(bins), int(robot_bins), _ptr(cells),
                                 _stream(stream)))
    return cells


def ground_classes(cells, max_step, out=None, stream=None):
    """emf_hip_groundClasses: the (1, H, W) u8 classes of (H, W) ground cells for a largest step of max_step >= 0 bins:
    FREE where a robot can stand, OCCUPIED at steps and where there is matter but no floor, UNKNOWN elsewhere.  A valid
    input of distance_transform, frontier_labels, plan_cost and cast_voxel_rays."""
    assert cells.dtype == GROUND_CELL_DTYPE and len(cells.shape) == 2 and not cells.padded
    H, W = cells.shape
    classes2d = DeviceArray((1, H, W), np.uint8) if out is None else out
    assert classes2d.dtype == np.uint8 and classes2d.shape == (1, H, W) and not classes2d.padded
    check("emf_hip_groundClasses",
          _L.emf_hip_groundClasses(_ptr(cells), (C.c_int32 * 2)(W, H), int(max_step), _ptr(classes2d), _stream(stream)))
    return classes2d


def ground_map(classes, frame, robot_bins, max_step, stream=None):
    """ground_columns, ground_cells and ground_classes of a class volume: (cells, classes2d), both on the device."""
    occ, fre = ground_columns(classes, frame, stream=stream)
    cells = ground_cells(occ, fre, frame.bins, robot_bins, stream=stream)
    return cells, ground_classes(cells, max_step, stream=stream)


# ---- planes (include/emf_hip.h "Planes") ----------------------------------------------------------

PLANE_VOXEL_DTYPE = np.dtype(_lib.PLANE_VOXEL_DTYPE)
PLANE_MOMENTS_DTYPE = np.dtype(_lib.PLANE_MOMENTS_DTYPE)
PLANE_MAX_K, PLANE_MAX_DIRS, PLANE_MAX_SLOTS, PLANE_MAX_PLANES = (_lib.PLANE_MAX_K, _lib.PLANE_MAX_DIRS,
                                                                  _lib.PLANE_MAX_SLOTS, _lib.PLANE_MAX_PLANES)
assert PLANE_VOXEL_DTYPE.itemsize == 16 and PLANE_MOMENTS_DTYPE.itemsize == 104


def plane_surface_scratch_bytes(size) -> int:
    return int(_L.emf_hip_planeSurfaceScratchBytes(_i3(size)))


def plane_surface(tsdf, weights, box=None, capacity=None, unseen_tiles=None, records=None, counters=None, stream=None):
    """emf_hip_planeSurface: the surface voxels with a normal of the box (lo, size), both (x, y, z), of (Nz, Ny, Nx) f32
    tsdf / weights (box None: the whole volume) as PLANE_VOXEL_DTYPE records (index: linear index in the box, g: the
    central tsdf differences), in the fixed tile order of the header.  capacity None: one record per voxel of the box.
    unseen_tiles: the volume's map as rebuild_unseen_tiles leaves it, or None; the bytes are the same either way.
    Returns (records, counters), both on the device: counters = 4 x u32 (surface voxels, those with a normal, records
    written, 0).  The host does not wait: the entries below read the count from counters (the scratch stays alive as
    counters.scratch)."""
    _vol(tsdf, np.float32)
    assert weights.shape == tsdf.shape and weights.dtype == np.float32
    res = (tsdf.shape[2], tsdf.shape[1], tsdf.shape[0])
    lo, size = _box(res, box)
    if capacity is None:
        capacity = max(size[0], 0) * max(size[1], 0) * max(size[2], 0)
    capacity = int(capacity)
    if records is None and capacity > 0:
        records = DeviceArray((capacity,), PLANE_VOXEL_DTYPE)
    assert records is None or (records.dtype == PLANE_VOXEL_DTYPE and records.shape[0] >= capacity)
    if counters is None:
        counters = DeviceArray((4,), np.uint32)
    assert counters.dtype == np.uint32 and counters.shape == (4,)
    scratch = DeviceArray((max(plane_surface_scratch_bytes(size), 4),), np.uint8)
    check("emf_hip_planeSurface",
          _L.emf_hip_planeSurface(_ptr(tsdf), _ptr(weights), _i3(res), _i3(lo), _i3(size), _ptr(unseen_tiles), _ptr(records),
                                  capacity, _ptr(counters), _ptr(scratch), _stream(stream)))
    counters.scratch = scratch
    return records, counters


def plane_directions(records, counters, k=15, capacity=None, out=None, stream=None):
    """emf_hip_planeDirections: the (6, k, k) u32 cube-map histogram (face, v cell, u cell) of the records' gradients."""
    capacity = records.shape[0] if capacity is None else int(capacity)
    shape = (6, max(int(k), 1), max(int(k), 1))
    bins = DeviceArray(shape, np.uint32) if out is None else out
    assert bins.dtype == np.uint32 and bins.shape == shape and not bins.padded
    check("emf_hip_planeDirections",
          _L.emf_hip_planeDirections(_ptr(records), _ptr(counters), capacity, int(k), _ptr(bins), _stream(stream)))
    return bins


def plane_offsets(records, counters, size, dirs, shift, cos2, inv_bin, slots, capacity=None, out=None, stream=None):
    """emf_hip_planeOffsets: the (D, slots) u32 histogram of the offsets along the D unit directions dirs (D x 3 f32, box
    voxel coordinates) of the records of a box of shape size (x, y, z) that are aligned with them (cos2: the squared
    cosine of the gate); slot = floor(n . b * inv_bin + shift[k])."""
    capacity = records.shape[0] if capacity is None else int(capacity)
    dirs = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
    shift = np.ascontiguousarray(np.asarray(shift, np.float32).reshape(-1))
    D = dirs.shape[0]
    assert shift.shape[0] == D
    shape = (max(D, 1), max(int(slots), 1))
    hist = DeviceArray(shape, np.uint32) if out is None else out
    assert hist.dtype == np.uint32 and hist.shape == shape and not hist.padded
    fp = C.POINTER(C.c_float)
    check("emf_hip_planeOffsets",
          _L.emf_hip_planeOffsets(_ptr(records), _ptr(counters), capacity, _i3(size), dirs.ctypes.data_as(fp),
                                  shift.ctypes.data_as(fp), D, float(np.float32(cos2)), float(np.float32(inv_bin)), int(slots),
                                  _ptr(hist), _stream(stream)))
    return hist


def plane_assign(records, counters, size, planes, cos2, band, capacity=None, out=None, stream=None):
    """emf_hip_planeAssign: per record the index of the plane (planes: P x 4 f32 = n0, n1, n2, d in box voxels) of
    smallest |n . b - d| among those it is aligned with and within `band` voxels of, -1 for none, and per plane the
    integer moments of its members.  Returns (labels, moments) on the device: `capacity` i16 of which the first
    counters[2] are written, and P PLANE_MOMENTS_DTYPE records.  out: (labels, moments) to reuse."""
    capacity = records.shape[0] if capacity is None else int(capacity)
    planes = np.ascontiguousarray(np.asarray(planes, np.float32).reshape(-1, 4))
    P = planes.shape[0]
    labels, moments = out if out is not None else (DeviceArray((max(capacity, 1),), np.int16),
                                                   DeviceArray((max(P, 1),), PLANE_MOMENTS_DTYPE))
    assert labels.dtype == np.int16 and labels.shape[0] >= capacity
    assert moments.dtype == PLANE_MOMENTS_DTYPE and moments.shape[0] >= P
    check("emf_hip_planeAssign",
          _L.emf_hip_planeAssign(_ptr(records), _ptr(counters), capacity, _i3(size), planes.ctypes.data_as(C.POINTER(C.c_float)),
                                 P, float(np.float32(cos2)), float(np.float32(band)), _ptr(labels), _ptr(moments),
                                 _stream(stream)))
    return labels, moments


# ---- plane patches (include/emf_hip.h "Planes", stage 4) ------------------------------------------

PLANE_PATCH_DTYPE = np.dtype(_lib.PLANE_PATCH_DTYPE)
PLANE_MAX_REACH = _lib.PLANE_MAX_REACH
PATCH_KEPT, PATCH_PATCHES, PATCH_MEMBERS = _lib.PATCH_KEPT, _lib.PATCH_PATCHES, _lib.PATCH_MEMBERS
assert PLANE_PATCH_DTYPE.itemsize == 128


def plane_patch_label(records, labels, counters, size, reach=1, capacity=None, out=None, stream=None):
    """emf_hip_planePatchLabel: per record of plane_surface (labels: plane_assign's) the id of its PATCH -- the connected
    component of the records with its label whose box voxels lie within `reach` (1 or 2, Chebyshev) of each other, named
    by the smallest record index among its members -- or -1 where the label is < 0.  Returns (patch, patch_counters) on
    the device: `capacity` i32 of which the first counters[2] are written, and 3 x u32 (kept patches: 0 until
    plane_patches, all patches, records with a label >= 0).  out: (patch, patch_counters) to reuse.  The host does not
    wait."""
    capacity = records.shape[0] if capacity is None else int(capacity)
    patch, pc = out if out is not None else (DeviceArray((max(capacity, 1),), np.int32), DeviceArray((3,), np.uint32))
    assert patch.dtype == np.int32 and patch.shape[0] >= capacity
    assert pc.dtype == np.uint32 and pc.shape == (3,)
    check("emf_hip_planePatchLabel",
          _L.emf_hip_planePatchLabel(_ptr(records), _ptr(labels), _ptr(counters), capacity, _i3(size), int(reach), _ptr(patch),
                                     _ptr(pc), _stream(stream)))
    return patch, pc


def plane_patch_scratch_bytes(capacity, n_patches) -> int:
    return int(_L.emf_hip_planePatchScratchBytes(int(capacity), int(n_patches)))


def plane_patches(records, labels, patch, counters, size, axes, patch_counters, min_count=1, n_patches=None, capacity=None,
                  capacity_patches=None, out=None, stream=None):
    """emf_hip_planePatches: one PLANE_PATCH_DTYPE record per patch of at least min_count members, in ascending id order:
    id, plane, the integer moments and bounds of the members and the extents (ulo, uhi, vlo, vhi) of the members along
    the two in-plane axes of their plane (axes: P x 6 f32 = u0, u1, u2, v0, v1, v2, box voxels).  n_patches None: read
    from patch_counters here -- the one wait.  Returns the records on the device (capacity_patches of them, None:
    n_patches); patch_counters[PATCH_KEPT] says how many are kept."""
    capacity = records.shape[0] if capacity is None else int(capacity)
    axes = np.ascontiguousarray(np.asarray(axes, np.float32).reshape(-1, 6))
    if n_patches is None:
        n_patches = int(patch_counters.numpy()[PATCH_PATCHES])
    n_patches = int(n_patches)
    if capacity_patches is None:
        capacity_patches = n_patches
    capacity_patches = int(capacity_patches)
    if out is None:
        out = DeviceArray((max(capacity_patches, 1),), PLANE_PATCH_DTYPE)
    assert out.dtype == PLANE_PATCH_DTYPE and out.shape[0] >= capacity_patches
    scratch = DeviceArray((max(plane_patch_scratch_bytes(capacity, n_patches), 16),), np.uint8)
    check("emf_hip_planePatches",
          _L.emf_hip_planePatches(_ptr(records), _ptr(labels), _ptr(patch), _ptr(counters), capacity, _i3(size),
                                  axes.ctypes.data_as(C.POINTER(C.c_float)), axes.shape[0], int(min_count), n_patches,
                                  _ptr(scratch), _ptr(out), capacity_patches, _ptr(patch_counters), _stream(stream)))
    out.scratch = scratch
    return out
