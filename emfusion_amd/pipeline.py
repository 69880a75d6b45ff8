"""ctypes binding of libemf_fusion.so (include/emf_fusion.h): the C++ host classes
emf::EMFusion / TSDF / ObjTSDF, the RCCL communicator and the synthetic RGB-D stream.

Harness-side only (tests/, bench.py).  All per-frame work happens in C++/HIP; this module moves
pointers.  Fails loudly if the library is missing -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np

from . import devmem
from ._lib import EmfImage, PKG_DIR, REPO_ROOT

# EMF_FUSION_VARIANT=_dbg loads libemf_fusion_dbg.so (the host classes built with -DEMF_DEBUG_SWITCHES: test infrastructure)
LIB_PATH = PKG_DIR / ("libemf_fusion%s.so" % os.environ.get("EMF_FUSION_VARIANT", ""))
HEADER_PATH = REPO_ROOT / "include" / "emf_fusion.h"


def obstacle_offsets(nearest, box_size=None):
    """The vectors from every voxel to its nearest obstacle voxel: (offsets (bz, by, bx, 3) i32 -- (dx, dy, dz) in
    voxels, zero where there is none -- and valid (bz, by, bx) bool) from the `nearest` array of
    Fusion.distance_field(nearest=True), linear indices (z * by + y) * bx + x with -1 for "none".  box_size (x, y, z):
    checked against the array's shape when given.  For an exact Euclidean transform the offset is the exact gradient
    direction of the distance field."""
    nearest = np.asarray(nearest)
    bz, by, bx = nearest.shape
    if box_size is not None and tuple(int(v) for v in box_size) != (bx, by, bz):
        raise ValueError(f"obstacle_offsets: box_size {tuple(box_size)} against an array of shape {nearest.shape}")
    valid = nearest >= 0
    lin = np.where(valid, nearest, 0).astype(np.int64)
    z, y, x = np.indices(nearest.shape)
    off = np.stack([lin % bx - x, lin // bx % by - y, lin // (bx * by) - z], axis=-1)
    return np.where(valid[..., None], off, 0).astype(np.int32), valid


class FusionParams(C.Structure):
    """Mirror of emf_fusion_params_t."""

    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("K", C.c_float * 9),
                ("bg_res", C.c_int32 * 3), ("bg_voxel_size", C.c_float),
                ("bg_rel_truncdist", C.c_float), ("volume_pose_t", C.c_float * 3),
                ("obj_res", C.c_int32 * 3), ("obj_rel_truncdist", C.c_float),
                ("max_tsdf_weight", C.c_float), ("assoc_sigma", C.c_float), ("alpha", C.c_float),
                ("uni_prior", C.c_float), ("visibility_thresh", C.c_int32),
                ("boundary", C.c_int32), ("mask_frames", C.c_int32),
                ("materialize_gradients", C.c_int32), ("max_tracking_iter", C.c_int32)]


class FrameTimings(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("points", "estep", "raycast", "composite", "integrate",
                                         "masks", "total")]

    def as_dict(self) -> Dict[str, float]:
        return {n: float(getattr(self, n)) for n, _ in self._fields_}


class CheckpointStats(C.Structure):
    """Mirror of emf_checkpoint_stats_t."""
    _fields_ = [("raw_bytes", C.c_uint64), ("file_bytes", C.c_uint64), ("chunks", C.c_uint64 * 3),
                ("ms_classify", C.c_double), ("ms_gather", C.c_double), ("ms_copy", C.c_double), ("ms_file", C.c_double),
                ("ms_total", C.c_double), ("records", C.c_uint32), ("reserved", C.c_uint32)]


class KernelSummary(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("total_ms", C.c_double), ("units", C.c_double)]


KERNEL_KINDS = ("points", "assoc", "normalize", "raycast", "composite", "integrate", "grads", "fgbg",
                "track", "integrate_bg")

IMG = dict(points=0, bg_assoc=1, obj_assoc=2, assoc_norm=3, raylengths=4, vertices=5, normals=6,
           segmentation=7, bg_raylengths=8, obj_raylengths=9)
_IMG_DTYPE = {0: ("float32", 3), 1: ("float32", 1), 2: ("float32", 1), 3: ("float32", 1),
              4: ("float32", 1), 5: ("float32", 3), 6: ("float32", 3), 7: ("uint8", 1),
              8: ("float32", 1), 9: ("float32", 1)}
SHADING = dict(label=0, color=1)
BACKGROUND_STORE_BYTES = 1 << 30  # set_background_store's default budget: a cap, not a measurement
VOL = dict(tsdf=0, weights=1, fgprobs=2, fgmask=3, bricks=4, color=5, fgbg=6)

_lib = None


class FusionError(RuntimeError):
    def __init__(self, fn, code, msg):
        super().__init__(f"{fn} failed with {code}: {msg}")
        self.code = code


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", HEADER_PATH.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(emf_(?:fusion|comm|synth)_\w+)\s*\(", text)))


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR / 'csrc'}` "
                           "(or __graft_entry__.build()). There is no CPU fallback.")
    lib = C.CDLL(os.fspath(LIB_PATH))
    lib.emf_fusion_last_error_string.restype = C.c_char_p
    lib.emf_fusion_default_params.restype = None
    lib.emf_fusion_destroy.restype = None
    lib.emf_comm_destroy.restype = None
    lib.emf_synth_destroy.restype = None
    vp = C.c_void_p
    fp = C.POINTER(C.c_float)
    ip = C.POINTER(C.c_int32)
    img = C.POINTER(EmfImage)
    sigs = {
        "emf_fusion_default_params": [C.POINTER(FusionParams)],
        "emf_fusion_create": [C.POINTER(FusionParams), vp, C.POINTER(vp)],
        "emf_fusion_destroy": [vp],
        "emf_fusion_reset": [vp],
        "emf_fusion_trim_pool": [C.POINTER(C.c_uint64)],
        "emf_fusion_save_checkpoint": [vp, C.c_char_p, C.POINTER(CheckpointStats)],
        "emf_fusion_load_checkpoint": [vp, C.c_char_p],
        "emf_fusion_checkpoint_info": [C.c_char_p, C.c_char_p, C.c_size_t],
        "emf_fusion_create_from_checkpoint": [C.c_char_p, vp, C.c_void_p, C.POINTER(vp)],
        "emf_fusion_describe_switches": [C.c_char_p, C.c_size_t],
        "emf_fusion_process_rgbd": [vp, fp, C.c_int32, C.c_int32],
        "emf_fusion_use_preproc_masks": [vp, C.c_char_p],
        "emf_fusion_set_color": [vp, C.c_int],
        "emf_fusion_set_mesh_weld": [vp, C.c_int],
        "emf_fusion_set_mesh_filter": [vp, C.c_uint32, C.c_int],
        "emf_fusion_set_mesh_simplify": [vp, C.c_float],
        "emf_fusion_last_mesh_simplify": [vp, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32)],
        "emf_fusion_mesh_components": [vp, C.c_int, C.POINTER(C.c_uint32)],
        "emf_fusion_copy_mesh_components": [vp, C.c_void_p, C.c_void_p],
        "emf_fusion_last_mesh_filter": [vp, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32)],
        "emf_fusion_set_color_image": [vp, img],
        "emf_fusion_set_background_follow": [vp, C.c_int, C.c_void_p],
        "emf_fusion_roll_background": [vp, ip, C.c_int],
        "emf_fusion_set_background_store": [vp, C.c_int, C.c_uint64],
        "emf_fusion_background_store_info": [vp, C.c_void_p],
        "emf_fusion_background_origin": [vp, ip, fp, fp],
        "emf_fusion_retired_slabs": [vp, C.c_void_p, C.c_int, ip],
        "emf_fusion_retired_slab_mesh": [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
        "emf_fusion_world_mesh": [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
        "emf_fusion_world_mesh_info": [vp, C.c_void_p],
        "emf_fusion_set_world_mesh_output": [vp, C.c_int],
        "emf_fusion_set_query_extent": [vp, C.c_int],
        "emf_fusion_world_extent": [vp, ip, ip],
        "emf_fusion_follow_shift": [fp, ip, C.c_float, ip],
        "emf_fusion_distance_field": [vp, ip, ip, C.c_uint32, C.c_int32, ip, C.c_int32, C.c_int, ip, ip, fp, fp],
        "emf_fusion_copy_distance_field": [vp, C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_distance_field_objects": [vp, ip, fp, fp, C.c_int, ip],
        "emf_fusion_set_distance_output": [vp, C.c_int, C.c_float, C.c_int],
        "emf_fusion_distance_field_nearest": [vp, ip, ip, C.c_uint32, C.c_int32, ip, C.c_int32, C.c_int, ip, ip, fp, fp],
        "emf_fusion_copy_distance_nearest": [vp, C.c_void_p],
        "emf_fusion_query_distance": [vp, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, ip, ip],
        "emf_fusion_set_distance_nearest_output": [vp, C.c_int],
        "emf_fusion_frontiers": [vp, ip, ip, C.c_int32, C.c_int32, ip, C.c_int32, ip, ip, fp, fp, C.c_void_p],
        "emf_fusion_copy_frontiers": [vp, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_set_frontier_output": [vp, C.c_int, C.c_int32, C.c_float],
        "emf_fusion_plan": [vp, ip, ip, ip, C.c_int32, C.c_int32, C.c_int, C.c_int32, C.c_uint32, ip, C.c_int32, C.c_int32, ip,
                            C.c_int32, ip, ip, fp, fp, C.c_void_p, ip],
        "emf_fusion_copy_plan": [vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
        "emf_fusion_plan_cost_ptr": [vp, C.POINTER(C.c_void_p)],
        "emf_fusion_set_plan_output": [vp, C.c_int, C.c_float, C.c_int],
        "emf_fusion_cast_rays": [vp, ip, ip, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, ip, C.c_int32,
                                 C.c_int32, C.c_void_p, C.c_void_p, ip, ip, fp, fp],
        "emf_fusion_view_ray_targets": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, fp, fp, ip,
                                        C.c_float, ip, ip, C.c_void_p],
        "emf_fusion_view_gain": [vp, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double, ip, ip, ip,
                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ip, ip, fp, fp],
        "emf_fusion_plan_shortcut": [vp, C.c_int32, C.c_void_p, ip],
        "emf_fusion_copy_plan_shortcut": [vp, C.c_void_p, C.c_int32],
        "emf_fusion_set_plan_shortcut_output": [vp, C.c_int32],
        "emf_fusion_object_shapes": [vp, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_shape_frame": [C.c_void_p, C.c_void_p],
        "emf_fusion_shape_box": [C.c_void_p, C.c_void_p, C.c_void_p, ip, C.c_float, fp, fp, C.c_void_p],
        "emf_fusion_set_shape_output": [vp, C.c_int],
        "emf_fusion_object_contacts": [vp, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ip, ip],
        "emf_fusion_contact_pose": [fp, fp, fp, fp, fp, fp],
        "emf_fusion_contact_touch": [C.c_double, C.c_float, fp],
        "emf_fusion_contact_summary": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_set_contacts_output": [vp, C.c_int, C.c_double],
        "emf_fusion_absorb_pose": [fp, fp, fp, fp, fp, fp],
        "emf_fusion_set_absorb_objects": [vp, C.c_int],
        "emf_fusion_absorb_object": [vp, C.c_int32, C.c_void_p],
        "emf_fusion_absorbed": [vp, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
        "emf_fusion_absorbed_colors": [vp, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
        "emf_fusion_set_absorbed_output": [vp, C.c_int],
        "emf_fusion_merge_union": [ip, ip, ip, C.c_float, ip, ip, ip, C.c_float, fp, fp, fp, fp, ip],
        "emf_fusion_set_merge_objects": [vp, C.c_int, C.c_double, C.c_int64, C.c_double, C.c_int32],
        "emf_fusion_merge_objects": [vp, C.c_int32, C.c_int32, C.c_void_p],
        "emf_fusion_set_merged_output": [vp, C.c_int],
        "emf_fusion_object_bookkeeping": [vp, C.c_int32, ip, ip, C.POINTER(C.c_double), C.c_int32, ip],
        "emf_fusion_merged": [vp, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
        "emf_fusion_set_lift_objects": [vp, C.c_int],
        "emf_fusion_lift_object": [vp, C.c_int32, C.c_void_p],
        "emf_fusion_lifted": [vp, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
        "emf_fusion_lifted_colors": [vp, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
        "emf_fusion_set_lifted_output": [vp, C.c_int],
        "emf_fusion_planes": [vp, ip, ip, C.c_void_p, ip, ip, fp, fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                              C.POINTER(C.c_int32)],
        "emf_fusion_copy_plane_labels": [vp, C.c_void_p, C.c_void_p, C.c_int64],
        "emf_fusion_set_planes_output": [vp, C.c_int, C.c_double, C.c_int64, C.c_int],
        "emf_fusion_plane_directions": [C.c_void_p, C.c_int32, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int32)],
        "emf_fusion_plane_offsets": [C.c_void_p, ip, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_uint32, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
        "emf_fusion_plane_fit": [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p],
        "emf_fusion_plane_patches": [vp, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
        "emf_fusion_copy_plane_patch_ids": [vp, C.c_void_p, C.c_int64],
        "emf_fusion_plane_patch_rect": [C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_plane_support": [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int32)],
        "emf_fusion_set_plane_patches_output": [vp, C.c_int, C.c_int32, C.c_int64],
        "emf_fusion_ground_map": [vp, ip, ip, ip, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_double,
                                  C.c_double, C.c_int32, C.c_int32, ip, ip, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int64],
        "emf_fusion_copy_ground_map": [vp, C.c_void_p, C.c_void_p],
        "emf_fusion_ground_classes_ptr": [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)],
        "emf_fusion_ground_frame": [ip, ip, ip, C.c_float, fp, fp, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_double,
                                    C.c_double, C.c_void_p, C.c_void_p],
        "emf_fusion_set_ground_output": [vp, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                         C.c_double],
        "emf_fusion_process_rgbd_color": [vp, fp, C.c_void_p, C.c_int32, C.c_int32],
        "emf_fusion_colored_voxels": [vp, C.POINTER(C.c_uint64)],
        "emf_fusion_get_last_masks": [vp, C.c_void_p, C.c_size_t, ip],
        "emf_fusion_set_motion_masks": [vp, C.c_int, C.c_void_p],
        "emf_fusion_last_motion_masks": [vp, C.c_void_p, C.c_void_p, C.c_int, ip],
        "emf_io_read_depth_png": [C.c_char_p, C.c_float, fp, C.c_size_t, ip, ip],
        "emf_io_read_exr": [C.c_char_p, C.c_char_p, fp, C.c_size_t, ip, ip],
        "emf_io_read_color_png": [C.c_char_p, C.c_void_p, C.c_size_t, ip, ip],
        "emf_io_load_config": [C.c_char_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t],
        "emf_io_image_reader": [C.c_char_p, C.c_char_p, C.c_char_p, ip, ip],
        "emf_io_tum_associations": [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), ip],
        "emf_io_load_preproc_masks": [C.c_char_p, ip, ip, ip, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_size_t,
                                      C.POINTER(C.c_double), C.c_size_t, ip],
        "emf_fusion_create_from_config": [C.c_char_p, C.c_char_p, C.c_int, vp, C.c_void_p, C.POINTER(vp)],
        "emf_fusion_add_object": [vp, fp, C.c_float, ip],
        "emf_fusion_process_frame": [vp, img, fp, fp, C.c_int, ip, fp, fp, C.c_int, ip, img,
                                     C.c_int],
        "emf_fusion_set_tracking": [vp, C.c_int, C.c_int],
        "emf_fusion_set_preprocess": [vp, C.c_int],
        "emf_fusion_set_cleanup": [vp, C.c_int],
        "emf_fusion_enable_pose_log": [vp, C.c_int],
        "emf_fusion_setup_output": [vp, C.c_int, C.c_int],
        "emf_fusion_write_results": [vp, C.c_char_p, C.c_int],
        "emf_io_png_unfilter": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
        "emf_io_write_volume": [C.c_char_p, fp, ip, C.c_float],
        "emf_io_write_pose_file": [C.c_char_p, C.c_int, ip, fp, fp],
        "emf_fusion_last_deleted": [vp, ip, C.c_int, ip],
        "emf_fusion_create_object_from_mask": [vp, img, ip],
        "emf_fusion_match_mask": [vp, img, ip, fp],
        "emf_fusion_update_object": [vp, C.c_int, img, fp],
        "emf_fusion_set_depth_broadcast": [vp, C.c_int],
        "emf_fusion_queue_instance_scores": [vp, C.c_int, C.c_int, C.c_void_p],
        "emf_fusion_object_class": [vp, C.c_int, ip],
        "emf_fusion_set_ignore_person": [vp, C.c_int],
        "emf_fusion_object_info": [vp, C.c_int, ip, fp, fp, fp],
        "emf_fusion_render": [vp, C.c_void_p, C.c_void_p],
        "emf_fusion_render_view": [vp, fp, fp, fp, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_set_3d_view": [vp, fp, fp, fp, C.c_int32, C.c_int32],
        "emf_fusion_clear_3d_view": [vp],
        "emf_fusion_render_view_shaded": [vp, fp, fp, fp, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_set_3d_view_shading": [vp, C.c_int],
        "emf_fusion_extract_mesh": [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
        "emf_fusion_copy_mesh": [vp, C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_extract_meshes": [vp, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint32)],
        "emf_fusion_copy_meshes": [vp, C.c_void_p, C.c_void_p, C.c_void_p],
        "emf_fusion_copy_mesh_colors": [vp, C.c_void_p],
        "emf_fusion_copy_meshes_colors": [vp, C.c_void_p],
        "emf_io_write_mesh": [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
        "emf_io_write_mesh_colors": [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p],
        "emf_fusion_queue_new_object_masks": [vp, C.c_int, img],
        "emf_fusion_last_created": [vp, ip, C.c_int, ip],
        "emf_fusion_queue_instance_masks": [vp, C.c_int, img],
        "emf_fusion_last_mask_assignment": [vp, ip, C.c_int, ip],
        "emf_fusion_get_pose": [vp, C.c_int, fp, fp],
        "emf_fusion_track_result": [vp, C.c_int, ip, ip, ip, fp],
        "emf_fusion_stage_estep": [vp],
        "emf_fusion_stage_raycast": [vp],
        "emf_fusion_stage_integrate": [vp],
        "emf_fusion_synchronize": [vp],
        "emf_fusion_enable_timings": [vp, C.c_int],
        "emf_fusion_last_timings": [vp, C.POINTER(FrameTimings)],
        "emf_fusion_enable_raycast_stats": [vp, C.c_int],
        "emf_fusion_raycast_stats": [vp, C.POINTER(C.c_uint64)],
        "emf_fusion_kernel_timers_enable": [vp, C.c_uint64],
        "emf_fusion_kernel_timers_clear": [vp],
        "emf_fusion_kernel_timers_select": [vp, C.c_uint32],
        "emf_fusion_kernel_timers_stride": [vp, C.c_uint32],
        "emf_fusion_kernel_timers_collect": [vp, C.POINTER(KernelSummary), C.POINTER(C.c_uint64)],
        "emf_fusion_get_image": [vp, C.c_int, C.c_int, img],
        "emf_fusion_get_volume": [vp, C.c_int, C.c_int, C.POINTER(vp), ip],
        "emf_fusion_visible_objects": [vp, ip, C.c_int, C.POINTER(C.c_int)],
        "emf_fusion_object_ids": [vp, ip, C.c_int, C.POINTER(C.c_int)],
        "emf_fusion_frame_index": [vp],
        "emf_fusion_background_overlap": [vp],
        "emf_fusion_batched_chunks": [vp],
        "emf_fusion_upload_host_time": [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)],
        "emf_fusion_owns_object": [vp, C.c_int],
        "emf_comm_describe": [vp, C.c_char_p, C.c_size_t],
        "emf_comm_unique_id": [vp],
        "emf_comm_create": [vp, C.c_int, C.c_int, C.POINTER(vp)],
        "emf_comm_destroy": [vp],
        "emf_comm_create_local_group": [C.c_int, C.POINTER(vp)],
        "emf_comm_create_delayed": [vp, C.c_int, C.POINTER(vp)],
        "emf_comm_all_reduce_sum_f32": [vp, vp, C.c_size_t, vp],
        "emf_comm_all_reduce_min_u64": [vp, vp, C.c_size_t, vp],
        "emf_comm_broadcast": [vp, vp, C.c_size_t, C.c_int, vp],
        "emf_comm_gather_row_bands": [vp, vp, C.c_size_t, C.c_int, C.c_int, vp],
        "emf_comm_create_peer_local_group": [C.c_int, C.c_size_t, C.POINTER(vp)],
        "emf_comm_create_peer": [C.c_int, C.c_int, C.c_size_t, vp, vp, C.POINTER(vp)],
        "emf_comm_exchanges": [vp, C.POINTER(C.c_uint64)],
        "emf_comm_create_host_staged": [vp, C.POINTER(vp)],
        "emf_synth_create": [C.c_int, C.c_int, fp, C.c_int, C.c_uint64, C.c_float, C.c_float,
                             C.POINTER(vp)],
        "emf_synth_destroy": [vp],
        "emf_synth_render": [vp, C.c_int, vp, vp],
        "emf_synth_camera_pose": [vp, C.c_int, fp, fp],
        "emf_synth_sphere": [vp, C.c_int, C.c_int, fp, fp, fp],
    }
    for name, argtypes in sigs.items():
        getattr(lib, name).argtypes = argtypes
    lib._emf_sigs = sigs
    _lib = lib
    return lib


def _check(fn: str, rc: int):
    if rc != 0:
        raise FusionError(fn, rc, load().emf_fusion_last_error_string().decode(errors="replace"))


def _farr(v, n):
    a = np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1))
    assert a.size == n
    return (C.c_float * n)(*a.tolist())


def _metres_to_voxels(metres, voxel):
    """Metres rounded up to whole voxels, at most 4096 and 0 for "none" -- in float32, as write_results does."""
    return int(min(np.ceil(np.float32(metres) / np.float32(voxel)), np.float32(4096))) if metres > 0 else 0


class _BoxFrame:
    """The frame of a box of the background that the scene queries share: bg_R (3x3), bg_t (3) the
    background's pose, res its resolution and lo the box origin, both (x, y, z) voxels, voxel its voxel size."""

    def __init__(self, bg_R, bg_t, res, voxel, lo=(0, 0, 0)):
        self.R, self.t = np.ascontiguousarray(bg_R, np.float64), np.asarray(bg_t, np.float64)
        self.res, self.lo = np.array(list(res), np.float64), np.array(list(lo), np.int64)
        self.voxel = float(voxel)

    def world64(self, vox):
        """One box voxel (3,), fractional too -> its world point (3,) f64 with the operand order of QueryBox::worldPoint:
        p_j = (v_j + (lo_j - (res_j - 1) / 2)) * voxel, then ((R_i0 p_0 + R_i1 p_1) + R_i2 p_2) + t_i."""
        p = (np.asarray(vox, np.float64) + (self.lo - (self.res - 1) / 2.0)) * np.float64(self.voxel)
        return np.array([((self.R[i, 0] * p[0] + self.R[i, 1] * p[1]) + self.R[i, 2] * p[2]) + self.t[i] for i in range(3)])

    def world(self, vox):
        """Box voxels (n, 3), fractional ones too -> world points (n, 3) f32: in float64, rounded once."""
        p = (np.asarray(vox, np.float64) + (self.lo - (self.res - 1) / 2.0)) * np.float64(self.voxel)
        return (p @ self.R.T + self.t).astype(np.float32)

    def to_voxels(self, points):
        """World points -> box voxels (n, 3) i32, each rounded to its voxel: clipped to the int32 range, -1 in a
        coordinate that is not finite -- so a point that is no point lies outside every box."""
        with np.errstate(invalid="ignore"):
            q = (np.asarray(points, np.float64).reshape(-1, 3) - self.t) @ self.R
            v = np.rint(q / self.voxel + (self.res - 1) / 2.0) - self.lo
        return np.where(np.isfinite(v), np.clip(v, -2.0 ** 31, 2.0 ** 31 - 1), -1).astype(np.int64).astype(np.int32)

    @staticmethod
    def unravel(lin, size):
        """Linear indices (z * ny + y) * nx + x of a box of `size` (x, y, z) -> its voxels (n, 3) i64."""
        lin, nx, ny = np.asarray(lin, np.int64), int(size[0]), int(size[1])
        return np.stack([lin % nx, lin // nx % ny, lin // (nx * ny)], axis=1)


def _box_args(box, exclude):
    """(box_lo, box_size, exclude_ids, num_exclude) of the query entries; a box of None is the whole background."""
    lo = size = None
    if box is not None:
        lo, size = (C.c_int32 * 3)(*[int(v) for v in box[0]]), (C.c_int32 * 3)(*[int(v) for v in box[1]])
    return lo, size, (C.c_int32 * max(len(exclude), 1))(*[int(i) for i in exclude]), len(exclude)


def _box_outs():
    """The (lo_out, size_out, R, t) arrays the query entries describe their box in."""
    return (C.c_int32 * 3)(), (C.c_int32 * 3)(), (C.c_float * 9)(), (C.c_float * 3)()


def _read_box_outs(lo, sz, R, t):
    """((lo, size), (R 3x3, t 3)): the box and the pose of its voxel (0, 0, 0) -> world."""
    return (tuple(lo), tuple(sz)), (np.array(R, np.float32).reshape(3, 3), np.array(t, np.float32))


def ground_bins(robot_height, max_step, bin):
    """(R, S): the robot's height rounded up to whole bins and at least 1, the largest step rounded down -- in float32,
    as _metres_to_voxels; both roundings err on the careful side."""
    b = np.float32(bin)
    robot = max(int(min(np.ceil(np.float32(robot_height) / b), np.float32(4096))), 1)
    step = int(min(np.floor(np.float32(max_step) / b), np.float32(4096))) if max_step > 0 else 0
    return robot, step


def ground_frame(lo, size, res, voxel, bg_R, bg_t, up, cell, bin, reference, band):
    """The frame of a ground map (include/emf_hip.h "Ground map"), restated in numpy float64 with the
    operand order of emf_fusion_ground_frame, so that both give the same bits.  lo, size: the box, res: the background's
    resolution, all (x, y, z) voxels; voxel: its voxel size; bg_R, bg_t: its pose (f32); up: the world direction that is
    up; cell, bin: metres; reference: a world point; band = (lo, hi) metres relative to it along up.  Returns
    (G (3, 4) f32: box voxel -> (u cells, v cells, h bins), W, H, B, pose (12,) f64: R row-major with (u, v, h) as
    columns, then t; ground metres -> world).  Raises ValueError where the entry returns an error."""
    f8 = np.float64
    lo, size, res = (np.array([int(v) for v in a], f8) for a in (lo, size, res))
    vs = f8(np.float32(voxel))
    R = np.asarray(bg_R, np.float32).reshape(9).astype(f8)
    t = np.asarray(bg_t, np.float32).reshape(3).astype(f8)
    up, ref = np.asarray(up, f8).reshape(3), np.asarray(reference, f8).reshape(3)
    cell, bin, band_lo, band_hi = f8(cell), f8(bin), f8(band[0]), f8(band[1])
    if not (np.isfinite(up).all() and np.isfinite(ref).all()):
        raise ValueError("ground_frame: a non-finite up or reference")
    if not (cell > 0 and bin > 0 and np.isfinite(cell) and np.isfinite(bin)):
        raise ValueError("ground_frame: cell and bin must be positive metres")
    if not (np.isfinite(band_lo) and np.isfinite(band_hi) and band_hi > band_lo):
        raise ValueError("ground_frame: the height band is empty")
    s = up[0] * up[0]
    s = s + up[1] * up[1]
    s = s + up[2] * up[2]
    length = np.sqrt(s)
    if not (length > 0 and np.isfinite(length)):
        raise ValueError("ground_frame: up has no direction")
    h = up / length
    for column in (0, 2):
        a = R[column::3]
        d = a[0] * h[0]
        d = d + a[1] * h[1]
        d = d + a[2] * h[2]
        along = d * h
        w = a - along
        n2 = w[0] * w[0]
        n2 = n2 + w[1] * w[1]
        n2 = n2 + w[2] * w[2]
        if not n2 < 1e-6:
            break
    u = w / np.sqrt(n2)
    v = np.array([h[1] * u[2] - h[2] * u[1], h[2] * u[0] - h[0] * u[2], h[0] * u[1] - h[1] * u[0]], f8)
    E = np.stack([u, v, h])
    c = (f8(0.0) + (lo - (res - 1.0) / 2.0)) * vs  # QueryBox::worldPoint of box voxel (0, 0, 0)
    p0 = np.empty(3, f8)
    for i in range(3):
        q = R[3 * i] * c[0]
        q = q + R[3 * i + 1] * c[1]
        q = q + R[3 * i + 2] * c[2]
        p0[i] = q + t[i]
    M, g = np.empty((3, 3), f8), np.empty(3, f8)
    for j in range(3):
        for k in range(3):
            m = E[j, 0] * R[k]
            m = m + E[j, 1] * R[3 + k]
            m = m + E[j, 2] * R[6 + k]
            M[j, k] = m * vs
        q = E[j, 0] * p0[0]
        q = q + E[j, 1] * p0[1]
        q = q + E[j, 2] * p0[2]
        g[j] = q
    A, mn, dims = np.empty((3, 4), f8), np.empty(2, f8), []
    corners = np.array([[size[k] - 0.5 if (n >> k) & 1 else -0.5 for k in range(3)] for n in range(8)], f8)
    for j in range(2):
        A[j, :3] = M[j] / cell
        a = g[j] / cell
        q = A[j, 0] * corners[:, 0]
        q = q + A[j, 1] * corners[:, 1]
        q = q + A[j, 2] * corners[:, 2]
        q = q + a
        mn[j] = q.min()
        A[j, 3] = a - mn[j]
        n = np.floor(q.max() - mn[j]) + 1.0
        if not n <= _GROUND_MAX_AXIS:
            raise ValueError(f"ground_frame: the map has more than {_GROUND_MAX_AXIS} cells on an axis")
        dims.append(int(n))
    A[2, :3] = M[2] / bin
    z0 = h[0] * ref[0]
    z0 = z0 + h[1] * ref[1]
    z0 = z0 + h[2] * ref[2]
    z0 = z0 + band_lo
    above = g[2] - z0
    A[2, 3] = above / bin
    span = band_hi - band_lo
    bins = np.ceil(span / bin)
    if not bins >= 1:
        raise ValueError("ground_frame: the height band holds no bin")
    if not bins <= _GROUND_MAX_BINS:
        raise ValueError(f"ground_frame: more than {_GROUND_MAX_BINS} height bins")
    ou, ov = mn[0] * cell, mn[1] * cell
    pose = np.empty(12, f8)
    pose[0:9:3], pose[1:9:3], pose[2:9:3] = u, v, h
    o = u * ou
    o = o + v * ov
    o = o + h * z0
    pose[9:] = o
    return A.astype(np.float32), dims[0], dims[1], int(bins), pose


_GROUND_MAX_AXIS, _GROUND_MAX_BINS = 2048, 256


def ground_frame_aligned(G):
    """Is up along a box axis to within float rounding of the frame: in every row of G[:, :3] all entries but the
    largest are at most 2^-20 of it.  Only then cells and bins below two voxels leave no holes in the columns."""
    G = np.abs(np.asarray(G, np.float32).reshape(3, 4)[:, :3])
    return all(int((row > row.max() * np.float32(2.0 ** -20)).sum()) == 1 for row in G)


class _GroundFrame:
    """Ground coordinates of a ground map: pose (12,) f64 "ground metres -> world", cell and bin in metres."""

    def __init__(self, pose, cell, bin):
        pose = np.asarray(pose, np.float64)
        self.R, self.o = pose[:9].reshape(3, 3), pose[9:]
        self.cell, self.bin = np.float64(cell), np.float64(bin)

    def world(self, cu, cv, ch):
        """Ground metres -> world (n, 3) f64: ((o + u cu) + v cv) + h ch per component."""
        cu, cv, ch = (np.asarray(a, np.float64) for a in (cu, cv, ch))
        out = []
        for i in range(3):
            q = self.o[i] + self.R[i, 0] * cu
            q = q + self.R[i, 1] * cv
            q = q + self.R[i, 2] * ch
            out.append(q)
        return np.stack(np.broadcast_arrays(*out), axis=-1)

    def to_cells(self, points):
        """World points -> the (u, v) cells they lie over, (n, 2) i32; -1 in a coordinate that is not finite."""
        d = np.asarray(points, np.float64).reshape(-1, 3) - self.o
        with np.errstate(invalid="ignore"):
            c = np.stack([np.floor(((d[:, 0] * self.R[0, k] + d[:, 1] * self.R[1, k]) + d[:, 2] * self.R[2, k]) / self.cell)
                          for k in range(2)], axis=1)
        return np.where(np.isfinite(c), np.clip(c, -2.0 ** 31, 2.0 ** 31 - 1), -1).astype(np.int64).astype(np.int32)


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """Viewer -> world (R, t) of a camera at `eye` looking at `target`, in the OpenCV camera convention (+z forward,
    +y down, +x right): R's columns are the camera axes in world coordinates, t = eye.  `up` is the world direction
    that appears up in the image (default -y: the world is an OpenCV camera frame, like the first frame's)."""
    eye, target, up = (np.asarray(v, np.float64).reshape(3) for v in (eye, target, up))
    z = target - eye
    if not np.linalg.norm(z) > 0:
        raise ValueError("look_at: eye and target coincide")
    z = z / np.linalg.norm(z)
    x = np.cross(-up, z)  # image right = down x forward
    if not np.linalg.norm(x) > 1e-9:
        raise ValueError("look_at: the viewing direction is parallel to `up`")
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1).astype(np.float32), eye.astype(np.float32)


DEFAULT_3D_VIEW_SIZE = (1024, 768)


def view_ray_targets(R, t, K, grid, range_m, bg_R, bg_t, res, voxel, lo=(0, 0, 0)):
    """emf_fusion_view_ray_targets, on the host without a device: (origin (3,) i32, targets (gh, gw, 3)
    i32) of the view (R, t) viewer -> world with the intrinsics K = (fx, fy, cx, cy) of a grid = (gw, gh) image and rays
    of range_m metres, in the box at `lo` of a background of pose (bg_R, bg_t), resolution res and voxel size voxel."""
    gw, gh = int(grid[0]), int(grid[1])
    Rd, td = np.ascontiguousarray(R, np.float64).reshape(9), np.ascontiguousarray(t, np.float64).reshape(3)
    Kd = np.ascontiguousarray(K, np.float64).reshape(4)
    origin, targets = np.zeros(3, np.int32), np.zeros((gh, gw, 3), np.int32)
    _check("emf_fusion_view_ray_targets",
           load().emf_fusion_view_ray_targets(Rd.ctypes.data, td.ctypes.data, Kd.ctypes.data, gw, gh, float(range_m), _farr(bg_R, 9),
                                              _farr(bg_t, 3), (C.c_int32 * 3)(*[int(v) for v in res]), float(voxel),
                                              (C.c_int32 * 3)(*[int(v) for v in lo]),
                                              origin.ctypes.data_as(C.POINTER(C.c_int32)), targets.ctypes.data))
    return origin, targets


def _shape_dtypes():
    from . import _lib as hip
    return (np.dtype(hip.SHAPE_MOMENTS_DTYPE), np.dtype(hip.SHAPE_FRAME_DTYPE), np.dtype(hip.SHAPE_EXTENTS_DTYPE),
            np.dtype(hip.SHAPE_BOX_DTYPE))


def shape_frame(moments):
    """emf_fusion_shape_frame, on the host without a device: the frame of one record of
    SHAPE_MOMENTS_DTYPE (ops.shape_moments) as a 0-d array of SHAPE_FRAME_DTYPE -- valid, centroid (voxels), covariance
    (xx yy zz xy xz yz, voxels^2), eigenvalues (descending), axes (three row vectors, right-handed) and f32, the frame
    rounded once for ops.shape_extents.  Float64 in the fixed operation order of include/emf_hip.h "Object shapes".  The
    moments describe the OBSERVED SOLID BAND of a model, not its body.  Without a solid voxel valid is 0 and the rest
    zeros."""
    md, fd, _, _ = _shape_dtypes()
    m = np.ascontiguousarray(np.asarray(moments, md).reshape(()))
    out = np.zeros((), fd)
    _check("emf_fusion_shape_frame", load().emf_fusion_shape_frame(m.ctypes.data, out.ctypes.data))
    return out


def shape_box(moments, frame, extents, res, voxel_size, R, t):
    """emf_fusion_shape_box, on the host without a device: the box of a model (a 0-d array of SHAPE_BOX_DTYPE) from its
    moments, a frame with valid != 0, the extents along it, the model's resolution (nx, ny, nz), voxel size and pose
    (R, t: volume -> world).  Voxels, metres in the model's own frame (p = (v - (res - 1) / 2) * voxel_size) and the
    world frame; float64 in the order of the header."""
    md, fd, ed, bd = _shape_dtypes()
    m = np.ascontiguousarray(np.asarray(moments, md).reshape(()))
    f = np.ascontiguousarray(np.asarray(frame, fd).reshape(()))
    e = np.ascontiguousarray(np.asarray(extents, ed).reshape(()))
    out = np.zeros((), bd)
    _check("emf_fusion_shape_box",
           load().emf_fusion_shape_box(m.ctypes.data, f.ctypes.data, e.ctypes.data, (C.c_int32 * 3)(*[int(v) for v in res]),
                                       float(voxel_size), _farr(R, 9), _farr(t, 3), out.ctypes.data))
    return out


def _contact_dtypes():
    from . import _lib as hip
    return (np.dtype(hip.CONTACT_PAIR_DTYPE), np.dtype(hip.CONTACT_DTYPE), np.dtype(hip.CONTACT_SIDE_DTYPE),
            np.dtype(hip.CONTACT_SUMMARY_DTYPE))


def contact_pose(pose_a, pose_b):
    """emf_fusion_contact_pose, on the host without a device: what a contact pair (probe a, field b)
    carries -- (R, t) taking a's frame into b's, R = Rb^T Ra, t = Rb^T (ta - tb) -- from the two poses (R, t: model ->
    world, f32).  Float64 in the fixed operation order of include/emf_hip.h "Object contacts", rounded to f32 once."""
    (Ra, ta), (Rb, tb) = pose_a, pose_b
    R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
    _check("emf_fusion_contact_pose",
           load().emf_fusion_contact_pose(_farr(Ra, 9), _farr(ta, 3), _farr(Rb, 9), _farr(tb, 3),
                                          R.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float))))
    return R.reshape(3, 3), t


def contact_touch(touch_m, truncdist_b):
    """emf_fusion_contact_touch: a distance in metres in units of the field's stored tsdf, float(touch_m / truncdist_b)."""
    out = (C.c_float * 1)()
    _check("emf_fusion_contact_touch", load().emf_fusion_contact_touch(float(touch_m), float(np.float32(truncdist_b)), out))
    return np.float32(out[0])


def contact_summary(record_ab, record_ba, side_a, side_b):
    """emf_fusion_contact_summary, on the host without a device: the unordered pair {a, b} from the record a -> b of
    ops.contact_probe and, where b was a probe as well, b -> a (else None).  side_a, side_b: records of
    _lib.CONTACT_SIDE_DTYPE (res, voxel_size, truncdist, R, t: model -> world).  Returns a 0-d array of
    _lib.CONTACT_SUMMARY_DTYPE: state (0 unseen, 1 apart, 2 touching, 3 penetrating), saturated (the deciding min_s is 1:
    AT LEAST one truncation distance apart, not a distance), direction (0: a -> b, 1: b -> a, -1: no touching voxel),
    has_normal, distance_m, and the world point, normal (out of the probe of `direction`) and the eight corners of the
    contact region.  Float64 in the fixed operation order of include/emf_hip.h "Object contacts"."""
    _, cd, sd, ud = _contact_dtypes()
    ab = np.ascontiguousarray(np.asarray(record_ab, cd).reshape(()))
    ba = None if record_ba is None else np.ascontiguousarray(np.asarray(record_ba, cd).reshape(()))
    a, b = (np.ascontiguousarray(np.asarray(v, sd).reshape(())) for v in (side_a, side_b))
    out = np.zeros((), ud)
    _check("emf_fusion_contact_summary",
           load().emf_fusion_contact_summary(ab.ctypes.data, None if ba is None else ba.ctypes.data, a.ctypes.data, b.ctypes.data,
                                             out.ctypes.data))
    return out


def contact_line(a, b, record, side_a, side_b):
    """One line of contacts.txt (without the newline): the ids, the eight counts, then in %.9g min_s and the world
    contact point and normal of this record alone."""
    s = contact_summary(record, None, side_a, side_b)
    ints = [int(record[k]) for k in ("surface", "outside", "unknown", "masked", "sampled", "inside", "touching", "normals")]
    floats = [float(record["min_s"])] + [float(v) for v in s["point"]] + [float(v) for v in s["normal"]]
    return " ".join([str(int(a)), str(int(b))] + [str(v) for v in ints] + ["%.9g" % v for v in floats])


def _absorb_event_dtype():
    """emf_absorb_event_t (include/emf_fusion.h): 176 bytes."""
    from . import _lib as hip
    d = np.dtype([("id", "<i4"), ("frame", "<i4"), ("clipped", "<i4"), ("reserved", "<i4"), ("R", "<f4", 9), ("t", "<f4", 3),
                  ("lo", "<i4", 3), ("size", "<i4", 3), ("record", np.dtype(hip.ABSORB_DTYPE))])
    assert d.itemsize == 176
    return d


def absorb_pose(pose_bg, pose_obj):
    """emf_fusion_absorb_pose, on the host without a device: what an absorption carries -- (R, t) taking
    the DESTINATION's volume frame into the SOURCE's, R = Ro^T Rb, t = Ro^T (tb - to) -- from the poses (R, t: volume ->
    world, f32) of the background and the object.  Float64 in the fixed operation order of contact_pose(pose_bg,
    pose_obj), rounded to f32 once."""
    (Rb, tb), (Ro, to) = pose_bg, pose_obj
    R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
    _check("emf_fusion_absorb_pose",
           load().emf_fusion_absorb_pose(_farr(Rb, 9), _farr(tb, 3), _farr(Ro, 9), _farr(to, 3),
                                         R.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float))))
    return R.reshape(3, 3), t


def _color_fields(records):
    """The trailing fields of a line of a coloured session: colored and uncolored of each colour record."""
    return "".join(" %d %d" % (int(c["colored"]), int(c["uncolored"])) for c in records)


def absorbed_line(event, color=None):
    """One line of absorbed.txt (without the newline) from an event of Fusion.absorbed().  color: the event's record of
    Fusion.absorbed_colors() in a coloured session -- its two counts follow as trailing fields -- or None."""
    if color is not None:
        return absorbed_line(event) + _color_fields([color])
    r = event["record"]
    ints = [event["id"], event["frame"], int(event["clipped"]), *event["lo"], *event["size"]] + \
        [int(r[k]) for k in ("visited", "outside", "unknown", "masked", "saturated", "fused", "fresh", "solid")] + \
        [int(v) for v in r["lo"]] + [int(v) for v in r["hi"]]
    floats = [float(v) for v in np.asarray(event["R"], np.float32).reshape(9)] + [float(v) for v in event["t"]]
    return " ".join([str(int(v)) for v in ints] + ["%.9g" % v for v in floats])


def _lift_event_dtype():
    """emf_lift_event_t (include/emf_fusion.h): 304 bytes."""
    from . import _lib as hip
    d = np.dtype([("id", "<i4"), ("frame", "<i4"), ("clipped", "<i4"), ("reserved", "<i4"), ("seed_R", "<f4", 9), ("seed_t", "<f4", 3),
                  ("release_R", "<f4", 9), ("release_t", "<f4", 3), ("lo", "<i4", 3), ("size", "<i4", 3),
                  ("seed", np.dtype(hip.SEED_DTYPE)), ("release", np.dtype(hip.RELEASE_DTYPE))])
    assert d.itemsize == 304
    return d


def lifted_line(event, color=None):
    """One line of lifted.txt (without the newline) from an event of Fusion.lifted().  color: the event's pair (seed,
    release) of Fusion.lifted_colors() in a coloured session -- four trailing fields -- or None."""
    if color is not None:
        return lifted_line(event) + _color_fields(color)
    s, r = event["seed"], event["release"]
    ints = [event["id"], event["frame"], int(event["clipped"]), *event["lo"], *event["size"]] + \
        [int(s[k]) for k in ("visited", "kept", "outside", "unknown", "masked", "saturated", "seeded", "solid")] + \
        [int(v) for v in s["lo"]] + [int(v) for v in s["hi"]] + \
        [int(r[k]) for k in ("visited", "empty", "free_space", "outside", "unclaimed", "released", "solid")] + \
        [int(v) for v in r["lo"]] + [int(v) for v in r["hi"]]
    floats = []
    for k in ("seed_R", "seed_t", "release_R", "release_t"):
        floats += [float(v) for v in np.asarray(event[k], np.float32).reshape(-1)]
    return " ".join([str(int(v)) for v in ints] + ["%.9g" % v for v in floats])


def _merge_event_dtype():
    """emf_merge_event_t (include/emf_fusion.h): 336 bytes."""
    from . import _lib as hip
    d = np.dtype([("dst", "<i4"), ("src", "<i4"), ("frame", "<i4"), ("clipped", "<i4"), ("automatic", "<i4"), ("res_before", "<i4"),
                  ("res_after", "<i4"), ("reserved", "<i4"), ("dst_R", "<f4", 9), ("dst_t", "<f4", 3), ("src_R", "<f4", 9),
                  ("src_t", "<f4", 3), ("R", "<f4", 9), ("t", "<f4", 3), ("lo", "<i4", 3), ("size", "<i4", 3), ("overlap", "<f8", 2),
                  ("record", np.dtype(hip.ABSORB_DTYPE)), ("counts", np.dtype(hip.MERGE_COUNTS_DTYPE)),
                  ("color", np.dtype(hip.COLOR_MOVED_DTYPE))])
    assert d.itemsize == 336
    return d


def merge_union(dst_bounds, dst_res, dst_voxel_size, src_bounds, src_res, src_voxel_size, pose):
    """emf_fusion_merge_union, on the host without a device: the box (lo, hi) in metres of the
    destination's volume frame that holds the bands of both objects -- what merge_objects hands to the destination's
    resize.  *_bounds: (lo, hi), inclusive voxel bounds of an object's observed solid band (object_shapes() moments; hi[0] <
    0: no solid voxel); pose = (R, t), f32, the destination's volume frame <- the source's.  Float64 in a fixed operation
    order, rounded to f32 once.  None where neither object has a solid voxel."""
    def i3(v):
        return (C.c_int32 * 3)(*[int(x) for x in v])
    lo, hi, any_ = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_int32(0)
    p = C.POINTER(C.c_float)
    _check("emf_fusion_merge_union",
           load().emf_fusion_merge_union(i3(dst_bounds[0]), i3(dst_bounds[1]), i3(dst_res), float(np.float32(dst_voxel_size)),
                                         i3(src_bounds[0]), i3(src_bounds[1]), i3(src_res), float(np.float32(src_voxel_size)),
                                         _farr(pose[0], 9), _farr(pose[1], 3), lo.ctypes.data_as(p), hi.ctypes.data_as(p),
                                         C.byref(any_)))
    return (lo, hi) if any_.value else None


def merged_line(event):
    """One line of a merge log (without the newline) from an event of Fusion.merged(): dst src frame clipped automatic
    res_before res_after, the box (lo, size), the eight counts and the bounds of the fused voxels, foreground gained, colored
    uncolored, then the two overlaps, the destination's pose R (9) t (3), the source's, and the pose used R (9) t (3), all
    in %.9g."""
    r = event["record"]
    ints = [event["dst"], event["src"], event["frame"], int(event["clipped"]), int(event["automatic"]), event["res_before"],
            event["res_after"], *event["lo"], *event["size"]] + \
        [int(r[k]) for k in ("visited", "outside", "unknown", "masked", "saturated", "fused", "fresh", "solid")] + \
        [int(v) for v in r["lo"]] + [int(v) for v in r["hi"]] + \
        [int(event["counts"]["foreground"]), int(event["counts"]["gained"]), int(event["color"]["colored"]), int(event["color"]["uncolored"])]
    floats = [float(v) for v in event["overlap"]]
    for k in ("dst_R", "dst_t", "src_R", "src_t", "R", "t"):
        floats += [float(v) for v in np.asarray(event[k], np.float32).reshape(-1)]
    return " ".join([str(int(v)) for v in ints] + ["%.9g" % v for v in floats])


# include/emf_hip.h "Planes": emf_plane_params_t (56 bytes) and emf_plane_t (176)
PLANE_PARAMS_DTYPE = np.dtype([("K", "<i4"), ("refine", "<i4"), ("max_planes", "<i4"), ("peak_gap", "<i4"), ("angle_deg", "<f8"),
                               ("separation_deg", "<f8"), ("bin_vox", "<f8"), ("band_vox", "<f8"), ("min_votes", "<i8")])
PLANE_DTYPE = np.dtype([("n", "<f8", 3), ("d", "<f8"), ("centroid", "<f8", 3), ("thickness", "<f8"), ("axes", "<f8", 6),
                        ("eigenvalues", "<f8", 3), ("count", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("fitted", "<i4"),
                        ("label", "<i4")])
assert PLANE_PARAMS_DTYPE.itemsize == 56 and PLANE_DTYPE.itemsize == 176


def _dot3(a, b):
    """(a0 * b0 + a1 * b1) + a2 * b2 in float64, one operation after the other."""
    s = np.float64(a[0]) * np.float64(b[0])
    s = s + np.float64(a[1]) * np.float64(b[1])
    return s + np.float64(a[2]) * np.float64(b[2])


def plane_cell_centre(b, k):
    """The unit vector (3,) f64 through the centre of bin b of a cube map of k cells per face side."""
    face, iv, iu = b // (k * k), b // k % k, b % k
    m = face // 2
    half = np.float64(k) / np.float64(2.0)
    c = np.zeros(3, np.float64)
    c[m] = -1.0 if face % 2 else 1.0
    c[(m + 1) % 3] = (np.float64(iu) + np.float64(0.5)) / half - np.float64(1.0)
    c[(m + 2) % 3] = (np.float64(iv) + np.float64(0.5)) / half - np.float64(1.0)
    return c / np.sqrt(_dot3(c, c))


def plane_directions(bins, k, min_votes, separation):
    """emf_fusion_plane_directions restated in numpy float64 with its operand order (include/emf_hip.h "Planes"), so that
    both give the same bits; on the host without a device.  The directions of a (6, k, k) u32 cube-map histogram
    (ops.plane_directions): bins by count descending, ties to the lower bin; a bin of at least min_votes becomes a
    direction, the normalised centre of its cell, unless its dot with a chosen one exceeds cos(separation degrees); at
    most 16.  Returns (dirs (n, 3) f64, bins (n,) i32, votes (n,) u32)."""
    from ._lib import PLANE_MAX_DIRS
    b = np.asarray(bins, np.uint32).reshape(-1)
    assert b.size == 6 * int(k) * int(k)
    order = np.argsort(-b.astype(np.int64), kind="stable")
    limit = np.cos(np.float64(separation) * np.float64(np.pi) / np.float64(180.0))
    dirs, which = [], []
    for i in order:
        if b[i] < min_votes or len(dirs) == PLANE_MAX_DIRS:
            break
        n = plane_cell_centre(int(i), int(k))
        if any(_dot3(n, c) > limit for c in dirs):
            continue
        dirs.append(n)
        which.append(int(i))
    return (np.array(dirs, np.float64).reshape(-1, 3), np.array(which, np.int32),
            b[np.array(which, np.int64)].astype(np.uint32) if which else np.zeros(0, np.uint32))


def plane_offsets(n, size, bin=1.0, row=None, min_votes=1, peak_gap=2):
    """emf_fusion_plane_offsets restated in numpy float64 with its operand order; on the host without a device.  The
    offset frame of the unit direction n over a box of `size` (x, y, z) voxels -- lo, the minimum of n . corner over the
    corners of the voxel cubes, the number of slots of `bin` voxels, inv_bin and shift with slot = floor(n . b * inv_bin +
    shift) -- and, with a row of votes, its peaks [(slot, votes)]: slots by votes descending, ties to the lower slot, at
    least min_votes, no two within peak_gap slots.  Returns (lo, slots, inv_bin, shift, peaks)."""
    n = np.asarray(n, np.float64).reshape(3)
    lo, hi = np.float64(np.inf), np.float64(-np.inf)
    for c in range(8):
        b = [np.float64(size[j]) - np.float64(0.5) if (c >> j) & 1 else np.float64(-0.5) for j in range(3)]
        s = _dot3(n, b)
        lo, hi = min(lo, s), max(hi, s)
    slots = int(np.floor((hi - lo) / np.float64(bin))) + 1
    inv_bin = np.float64(1.0) / np.float64(bin)
    shift = -lo * inv_bin
    peaks = []
    if row is not None:
        r = np.asarray(row, np.uint32).reshape(-1)[:slots]
        for i in np.argsort(-r.astype(np.int64), kind="stable"):
            if r[i] < min_votes:
                break
            if all(abs(int(i) - p[0]) > peak_gap for p in peaks):
                peaks.append((int(i), int(r[i])))
    return float(lo), slots, float(inv_bin), float(shift), peaks


def plane_fit(moments, seed_n, seed_d):
    """emf_fusion_plane_fit restated in numpy float64; on the host without a device.  One plane (a 0-d array of
    PLANE_DTYPE, box voxel coordinates) from a record of PLANE_MOMENTS_DTYPE (ops.plane_assign) and its seed: centroid,
    covariance and Jacobi frame are shape_frame's, called, not restated; the normal is the axis of the smallest
    eigenvalue turned towards the seed, d = n . centroid, thickness the root of that eigenvalue.  Fewer than 3 members
    keep the seed (fitted == 0)."""
    from ._lib import PLANE_MOMENTS_DTYPE, SHAPE_MOMENTS_DTYPE
    m = np.asarray(moments, np.dtype(PLANE_MOMENTS_DTYPE)).reshape(())
    seed = np.asarray(seed_n, np.float64).reshape(3)
    out = np.zeros((), PLANE_DTYPE)
    out["count"], out["lo"], out["hi"] = m["count"], m["lo"], m["hi"]
    if int(m["count"]) < 3:
        out["n"], out["d"] = seed, np.float64(seed_d)
        return out
    sm = np.zeros((), np.dtype(SHAPE_MOMENTS_DTYPE))
    sm["solid"], sm["sum"], sm["sum2"] = m["count"], m["sum"], m["sum2"]
    fr = shape_frame(sm)
    a = fr["axes"][6:9]
    n = -a if _dot3(a, seed) < 0.0 else a.copy()
    out["n"], out["centroid"], out["eigenvalues"], out["axes"] = n, fr["centroid"], fr["eigenvalues"], fr["axes"][:6]
    out["d"] = _dot3(n, fr["centroid"])
    out["thickness"] = np.sqrt(max(np.float64(fr["eigenvalues"][2]), np.float64(0.0)))
    out["fitted"] = 1
    return out


# include/emf_hip.h "Planes", stage 4: emf_plane_patch_rect_t (320 bytes)
PLANE_PATCH_RECT_DTYPE = np.dtype([("fit", PLANE_DTYPE), ("center", "<f8", 3), ("half", "<f8", 2), ("corners", "<f8", 12),
                                   ("fill", "<f8")])
assert PLANE_PATCH_RECT_DTYPE.itemsize == 320


def plane_patch_rect(plane, patch):
    """emf_fusion_plane_patch_rect restated in numpy float64 with its operand order (include/emf_hip.h, the host steps
    behind stage 4), so that both give the same bits; on the host without a device.  From a plane (PLANE_DTYPE, box voxel
    coordinates) and one of its patches (ops.PLANE_PATCH_DTYPE): fit, the patch's own plane by plane_fit CALLED on its
    moments with the plane as the seed; the rectangle that holds the patch's members along the plane's two in-plane
    axes, widened by half a voxel on each side -- center, half (2), corners (4 x 3, flat), all IN the plane; and
    fill = count / (the rectangle's voxel columns), near 1 for a full rectangle and lower for an L shape or one with
    holes: A RATIO OF TWO ESTIMATES.  Returns a 0-d array of PLANE_PATCH_RECT_DTYPE."""
    from ._lib import PLANE_MOMENTS_DTYPE
    f8 = np.float64
    mom = np.zeros((), np.dtype(PLANE_MOMENTS_DTYPE))
    for key in ("count", "sum", "sum2", "lo", "hi"):
        mom[key] = patch[key]
    n, d = np.asarray(plane["n"], f8).reshape(3), f8(plane["d"])
    u, v = np.asarray(plane["axes"], f8).reshape(6)[:3], np.asarray(plane["axes"], f8).reshape(6)[3:]
    out = np.zeros((), PLANE_PATCH_RECT_DTYPE)
    out["fit"] = plane_fit(mom, n, d)
    out["fit"]["label"] = plane["label"]
    a0, a1 = f8(patch["ulo"]) - f8(0.5), f8(patch["uhi"]) + f8(0.5)
    b0, b1 = f8(patch["vlo"]) - f8(0.5), f8(patch["vhi"]) + f8(0.5)
    with np.errstate(all="ignore"):
        cu, hu = (a0 + a1) * f8(0.5), (a1 - a0) * f8(0.5)
        cv, hv = (b0 + b1) * f8(0.5), (b1 - b0) * f8(0.5)

        def point(eu, ev):
            p = np.zeros(3, f8)
            for j in range(3):
                s = d * n[j]
                t = u[j] * eu
                s = s + t
                t = v[j] * ev
                p[j] = s + t
            return p

        out["center"], out["half"] = point(cu, cv), (hu, hv)
        out["corners"] = np.concatenate([point(cu + su * hu, cv + sv * hv)
                                         for su, sv in ((f8(-1), f8(-1)), (f8(1), f8(-1)), (f8(1), f8(1)), (f8(-1), f8(1)))])
        wu = (f8(patch["uhi"]) - f8(patch["ulo"])) + f8(1.0)
        wv = (f8(patch["vhi"]) - f8(patch["vlo"])) + f8(1.0)
        area = (wu * wv) * np.abs(n).max()
        out["fill"] = f8(int(patch["count"])) / area
    return out


def plane_support_of(n, d, center, axes, half, box_center, box_axes, box_half, margin=0.0):
    """emf_fusion_plane_support restated in numpy float64 with its operand order; on the host without a device.  One
    oriented box (centre, three unit row axes, half sizes) against one patch (plane n . x = d, rectangle centre, two row
    axes, half sizes), world metres: (s, over) with s = (n . c - d) - sum_k |n . A_k| * h_k, the height of the box's lowest
    point above the plane, and over = the box centre lies, along the rectangle's axes about its centre, within
    half + margin."""
    f8 = np.float64
    n, c = np.asarray(n, f8).reshape(3), np.asarray(box_center, f8).reshape(3)
    A, h = np.asarray(box_axes, f8).reshape(3, 3), np.asarray(box_half, f8).reshape(3)
    axes, half, center = np.asarray(axes, f8).reshape(2, 3), np.asarray(half, f8).reshape(2), np.asarray(center, f8).reshape(3)
    s = _dot3(n, c) - f8(d)
    for k in range(3):
        s = s - np.abs(_dot3(n, A[k])) * h[k]
    q = [c[0] - center[0], c[1] - center[1], c[2] - center[2]]
    over = True
    for j in range(2):
        over = over and bool(np.abs(_dot3(q, axes[j])) <= half[j] + f8(margin))
    return float(s), over


def plane_support(patches, boxes, gap=0.05, margin=0.0):
    """Which patch each oriented box rests on; on the host without a device.  patches: the patch dicts of
    Fusion.planes(patches=True) in any order (normal, d, rect and kind are read); boxes: dicts with center (3,), axes
    (3 x 3 unit rows) and half (3,) in world metres, or None.  A box is OVER a patch iff its centre, along the
    rectangle's axes about the rectangle's centre, lies within half_m + margin: the rectangle, not the members, because
    the surface under a standing object is occluded and missing from the patch, and the rectangle spans the hole.  It
    RESTS ON the patch of smallest |s| (plane_support_of) among those it is over with |s| <= gap and whose kind is floor
    or level; ties go to the earlier patch.  gap 0.05 m IS POLICY, NOT A MEASUREMENT.  Returns per box (index into
    patches, s) or None."""
    out = []
    for box in boxes:
        best = None
        for k, p in enumerate(patches if box is not None else ()):
            if p["kind"] not in ("floor", "level"):
                continue
            s, over = plane_support_of(p["normal"], p["d"], p["rect"]["center"], p["rect"]["axes"], p["rect"]["half_m"],
                                       box["center"], box["axes"], box["half"], margin)
            if over and abs(s) <= gap and (best is None or abs(s) < abs(best[1])):
                best = (k, s)
        out.append(best)
    return out


def plane_kinds(normals, heights, up, floor_angle=30.0, kind_angle=10.0):
    """(floor, kinds) of planes with world unit normals and centroid heights along `up`.  The floor is, among the planes
    whose normal is within floor_angle degrees of up, the one whose centroid is lowest along up, ties to the lowest
    index, or None.  Relative to the floor's normal (to up without a floor): "floor", "level" (within kind_angle),
    "ceiling" (within kind_angle of the opposite), "wall" (perpendicular within kind_angle), "slope"."""
    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    up = [float(v) for v in up]
    norm = float(np.sqrt(dot(up, up)))
    up = [up[0] / norm, up[1] / norm, up[2] / norm]
    cos_floor = float(np.cos(floor_angle * np.pi / 180.0))
    cos_kind, sin_kind = float(np.cos(kind_angle * np.pi / 180.0)), float(np.sin(kind_angle * np.pi / 180.0))
    normals = [[float(v) for v in n] for n in normals]
    floor = None
    for k, n in enumerate(normals):
        if dot(n, up) >= cos_floor and (floor is None or heights[k] < heights[floor]):
            floor = k
    ref = up if floor is None else normals[floor]
    kinds = []
    for k, n in enumerate(normals):
        c = dot(n, ref)
        kinds.append("floor" if k == floor else "level" if c >= cos_kind else "ceiling" if c <= -cos_kind
                     else "wall" if abs(c) <= sin_kind else "slope")
    return floor, kinds


def default_3d_view(params: FusionParams):
    """The reference's 3D window (apps/EM-Fusion.cpp:118-131): viewer at (0, 0, -1) with the world's axes, 1024 x 768,
    the frame intrinsics scaled by 1024 / W and 768 / H.  Returns (R, t, K, size)."""
    w, h = DEFAULT_3D_VIEW_SIZE
    K = np.array(params.K, np.float32).reshape(3, 3)
    sx, sy = np.float32(w / params.width), np.float32(h / params.height)
    K[0, 0] *= sx
    K[0, 2] *= sx
    K[1, 1] *= sy
    K[1, 2] *= sy
    return np.eye(3, dtype=np.float32), np.array([0, 0, -1], np.float32), K, (w, h)


def default_params() -> FusionParams:
    p = FusionParams()
    load().emf_fusion_default_params(C.byref(p))
    return p


def make_params(width=640, height=480, bg_res=512, bg_voxel=0.01, obj_res=128,
                materialize_gradients=False, **overrides) -> FusionParams:
    """Reference defaults (config/default.cfg) with the BASELINE.json volume sizes."""
    p = default_params()
    p.width, p.height = width, height
    f = 525.0 * width / 640.0
    p.K[:] = [f, 0, width / 2 - 0.5, 0, f, height / 2 - 0.5, 0, 0, 1]
    p.bg_res[:] = [bg_res] * 3
    p.bg_voxel_size = bg_voxel
    p.volume_pose_t[:] = [0, 0, bg_res * bg_voxel / 2]
    p.obj_res[:] = [obj_res] * 3
    p.materialize_gradients = int(materialize_gradients)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


class Communicator:
    """RCCL communicator (one process per GPU).  The unique id travels over torch.distributed."""

    def __init__(self, unique_id: bytes, rank: int, world: int):
        self._h = C.c_void_p()
        buf = C.create_string_buffer(unique_id, 128)
        _check("emf_comm_create", load().emf_comm_create(buf, rank, world, C.byref(self._h)))
        self.rank, self.world = rank, world

    @classmethod
    def local_group(cls, world: int, transport: str = "host", max_bytes: int = 0):
        """`world` communicators of THIS process for `world` Fusion objects on `world` threads sharing one
        GPU (rehearsal of the multi-GPU code path).  transport "host": collectives staged through host
        memory; "peer": the direct peer-write exchanges (max_bytes = the slot size: W * H * 16 holds the raycast's fused exchange -- keys, background band, mask; with less the frame falls back to unfused exchanges)."""
        handles = (C.c_void_p * world)()
        if transport == "peer":
            _check("emf_comm_create_peer_local_group",
                   load().emf_comm_create_peer_local_group(world, int(max_bytes), handles))
        else:
            _check("emf_comm_create_local_group", load().emf_comm_create_local_group(world, handles))
        out = []
        for r in range(world):
            c = cls.__new__(cls)
            c._h, c.rank, c.world = C.c_void_p(handles[r]), r, world
            out.append(c)
        return out

    @classmethod
    def host_staged(cls, dist):
        """One process per rank, collectives staged through host memory and carried by the given
        torch.distributed module (gloo): rehearsal of the N-rank job on fewer than N GPUs."""
        import torch
        rank, world = dist.get_rank(), dist.get_world_size()

        def view(ptr, count, dtype):
            return torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dtype)), shape=(count,)))

        def guard(fn):
            def wrapped(*a):
                try:
                    fn(*a)
                    return 0
                except Exception as e:  # noqa: BLE001 - reported through the C++ exception
                    print("host-staged collective failed:", repr(e), flush=True)
                    return 1
            return wrapped

        def sum_f32(user, ptr, count):
            dist.all_reduce(view(ptr, count, C.c_float), op=dist.ReduceOp.SUM)

        def min_u64(user, ptr, count):
            t = view(ptr, count, C.c_int64)
            t ^= -(2 ** 63)          # unsigned order -> signed order
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            t ^= -(2 ** 63)

        def bcast(user, ptr, nbytes, root):
            dist.broadcast(view(ptr, nbytes, C.c_uint8), src=root)

        f_red = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
        f_bc = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)

        class Callbacks(C.Structure):
            _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("sum", f_red), ("min", f_red),
                        ("bcast", f_bc), ("user", C.c_void_p)]
        c = cls.__new__(cls)
        c._keep = (f_red(guard(sum_f32)), f_red(guard(min_u64)), f_bc(guard(bcast)))
        cb = Callbacks(rank, world, c._keep[0], c._keep[1], c._keep[2], None)
        c._h = C.c_void_p()
        _check("emf_comm_create_host_staged", load().emf_comm_create_host_staged(C.byref(cb), C.byref(c._h)))
        c.rank, c.world = rank, world
        return c

    @classmethod
    def peer(cls, dist, max_bytes: int):
        """One process per rank, direct peer-write exchanges: the ranks' receive buffers are mapped into each
        other with hipIpc*, the handles travel through the given torch.distributed module (gloo)."""
        import torch
        rank, world = dist.get_rank(), dist.get_world_size()

        def gather(user, mine, nbytes, allp):
            try:
                t = torch.from_numpy(np.ctypeslib.as_array(C.cast(mine, C.POINTER(C.c_uint8)), shape=(nbytes,)).copy())
                outs = [torch.empty_like(t) for _ in range(world)]
                dist.all_gather(outs, t)
                dst = np.ctypeslib.as_array(C.cast(allp, C.POINTER(C.c_uint8)), shape=(nbytes * world,))
                for r, o in enumerate(outs):
                    dst[r * nbytes:(r + 1) * nbytes] = o.numpy()
                return 0
            except Exception as e:  # noqa: BLE001 - reported through the C++ exception
                print("peer bootstrap all-gather failed:", repr(e), flush=True)
                return 1
        f_ag = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
        c = cls.__new__(cls)
        c._keep = (f_ag(gather),)
        c._h = C.c_void_p()
        _check("emf_comm_create_peer", load().emf_comm_create_peer(rank, world, int(max_bytes),
                                                                   C.cast(c._keep[0], C.c_void_p), None, C.byref(c._h)))
        c.rank, c.world = rank, world
        return c

    # the four exchanges on their own (device arrays of emfusion_amd.devmem, stream = devmem.Stream or None)
    def all_reduce_sum_f32(self, arr, stream=None):
        _check("emf_comm_all_reduce_sum_f32", load().emf_comm_all_reduce_sum_f32(
            self._h, C.c_void_p(arr.ptr), arr.nbytes // 4, stream.handle if stream else None))

    def all_reduce_min_u64(self, arr, stream=None):
        _check("emf_comm_all_reduce_min_u64", load().emf_comm_all_reduce_min_u64(
            self._h, C.c_void_p(arr.ptr), arr.nbytes // 8, stream.handle if stream else None))

    def broadcast(self, arr, root, stream=None):
        _check("emf_comm_broadcast", load().emf_comm_broadcast(
            self._h, C.c_void_p(arr.ptr), arr.nbytes, int(root), stream.handle if stream else None))

    def gather_row_bands(self, arr, band_rows, stream=None):
        _check("emf_comm_gather_row_bands", load().emf_comm_gather_row_bands(
            self._h, C.c_void_p(arr.ptr), arr.pitch, int(band_rows), arr.shape[0], stream.handle if stream else None))

    def delayed(self, microseconds: int) -> "Communicator":
        """Latency model around this communicator: every exchange (a grouped one counts once) first keeps its
        stream busy for `microseconds`.  Keep `self` alive as long as the result is used."""
        c = Communicator.__new__(Communicator)
        c._h = C.c_void_p()
        _check("emf_comm_create_delayed", load().emf_comm_create_delayed(self._h, int(microseconds), C.byref(c._h)))
        c.rank, c.world, c._inner = self.rank, self.world, self
        return c

    def describe(self) -> dict:
        """What the transport itself reports about this rank: ranks it sees, device ordinal, PCI bus id, version."""
        import json as _json
        buf = C.create_string_buffer(1024)
        _check("emf_comm_describe", load().emf_comm_describe(self._h, buf, len(buf)))
        return _json.loads(buf.value.decode())

    def exchanges(self) -> int:
        """Exchanges issued so far (a group counts once) through a delayed(), peer or local-group communicator (0 for the
        others)."""
        n = C.c_uint64(0)
        _check("emf_comm_exchanges", load().emf_comm_exchanges(self._h, C.byref(n)))
        return int(n.value)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check("emf_comm_unique_id", load().emf_comm_unique_id(buf))
        return buf.raw

    def close(self):
        if self._h:
            load().emf_comm_destroy(self._h)
            self._h = C.c_void_p()


class SyntheticStream:
    """Deterministic synthetic RGB-D stream (emf::SyntheticScene)."""

    def __init__(self, width, height, K, num_spheres, seed=0xE3F5, noise=0.002, dropout=0.01):
        self._h = C.c_void_p()
        self.width, self.height, self.n = width, height, num_spheres
        _check("emf_synth_create",
               load().emf_synth_create(width, height, _farr(K, 9), num_spheres, seed, noise,
                                       dropout, C.byref(self._h)))

    def render(self, frame: int):
        depth = np.empty((self.height, self.width), np.float32)
        ids = np.empty((self.height, self.width), np.uint8)
        _check("emf_synth_render",
               load().emf_synth_render(self._h, frame, depth.ctypes.data, ids.ctypes.data))
        return depth, ids

    def camera_pose(self, frame: int):
        R = (C.c_float * 9)()
        t = (C.c_float * 3)()
        _check("emf_synth_camera_pose", load().emf_synth_camera_pose(self._h, frame, R, t))
        return np.array(R, np.float32), np.array(t, np.float32)

    def sphere(self, k: int, frame: int):
        c = (C.c_float * 3)()
        r = C.c_float()
        v = C.c_float()
        _check("emf_synth_sphere",
               load().emf_synth_sphere(self._h, k, frame, c, C.byref(r), C.byref(v)))
        return np.array(c, np.float32), float(r.value), float(v.value)

    def close(self):
        if self._h:
            load().emf_synth_destroy(self._h)
            self._h = C.c_void_p()


class Fusion:
    """One emf::EMFusion instance (background + object volumes) on the current device."""

    def __init__(self, params: FusionParams, comm: Optional[Communicator] = None):
        self._h = C.c_void_p()
        self.params = params
        self._comm = comm
        _check("emf_fusion_create",
               load().emf_fusion_create(C.byref(params), comm._h if comm else None,
                                        C.byref(self._h)))

    @classmethod
    def from_config(cls, path=None, calibration=None, comm: Optional[Communicator] = None, materialize_gradients=False):
        """The instance `apps/emfusion_synth --configfile` builds: every key of one of the reference's configuration
        files (ignore_person, LM / Huber / bilateral / lifecycle thresholds included -- FusionParams holds a subset)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.params = FusionParams()
        self._comm = comm
        _check("emf_fusion_create_from_config",
               load().emf_fusion_create_from_config(os.fspath(path).encode() if path else None,
                                                    os.fspath(calibration).encode() if calibration else None,
                                                    int(materialize_gradients), comm._h if comm else None,
                                                    C.byref(self.params), C.byref(self._h)))
        return self

    def close(self):
        if self._h:
            load().emf_fusion_destroy(self._h)
            self._h = C.c_void_p()

    def reset(self):
        _check("emf_fusion_reset", load().emf_fusion_reset(self._h))

    def add_object(self, center, vol_size: float) -> int:
        out = C.c_int32()
        _check("emf_fusion_add_object",
               load().emf_fusion_add_object(self._h, _farr(center, 3), vol_size, C.byref(out)))
        return out.value

    def process_frame(self, depth_view: EmfImage, cam_R, cam_t, obj_poses=None, masks=None,
                      run_masks=False):
        """obj_poses: {id: (R9, t3)}; masks: {id: EmfImage (device u8 0/1)}."""
        obj_poses = obj_poses or {}
        masks = masks or {}
        n = len(obj_poses)
        ids = (C.c_int32 * max(n, 1))(*obj_poses.keys())
        Rs = (C.c_float * (9 * max(n, 1)))()
        ts = (C.c_float * (3 * max(n, 1)))()
        for i, (R, t) in enumerate(obj_poses.values()):
            Rs[9 * i:9 * i + 9] = np.asarray(R, np.float32).reshape(-1).tolist()
            ts[3 * i:3 * i + 3] = np.asarray(t, np.float32).reshape(-1).tolist()
        m = len(masks)
        mids = (C.c_int32 * max(m, 1))(*masks.keys())
        mviews = (EmfImage * max(m, 1))(*masks.values())
        _check("emf_fusion_process_frame",
               load().emf_fusion_process_frame(self._h, C.byref(depth_view), _farr(cam_R, 9),
                                               _farr(cam_t, 3), n, ids, Rs, ts, m, mids, mviews,
                                               int(run_masks)))

    def process_rgbd(self, depth: np.ndarray, rgb: Optional[np.ndarray] = None):
        """EMFusion::processFrame(const RGBD&): a host depth image in metres (uploaded, filtered, fused).  rgb: the
        frame's (H, W, 3) u8 colour image, fused into the colour volumes (needs enable_color())."""
        d = np.ascontiguousarray(depth, np.float32)
        if rgb is None:
            _check("emf_fusion_process_rgbd",
                   load().emf_fusion_process_rgbd(self._h, d.ctypes.data_as(C.POINTER(C.c_float)), d.shape[1], d.shape[0]))
            return
        c = np.ascontiguousarray(rgb, np.uint8)
        if c.shape != d.shape + (3,):
            raise ValueError(f"process_rgbd: rgb is {c.shape}, expected {d.shape + (3,)}")
        _check("emf_fusion_process_rgbd_color",
               load().emf_fusion_process_rgbd_color(self._h, d.ctypes.data_as(C.POINTER(C.c_float)), c.ctypes.data,
                                                    d.shape[1], d.shape[0]))

    def enable_color(self, on=True):
        """Per-voxel colour: every model keeps a colour volume (volume("color", id): (Nz, Ny, Nx, 4) u16 = R, G, B and
        the colour weight in 8.8 fixed point) that frames with a colour image fuse into.  Before the first frame or
        after reset() only; refused on the sharded and per-volume paths."""
        _check("emf_fusion_set_color", load().emf_fusion_set_color(self._h, int(on)))

    def set_mesh_weld(self, on=True):
        """Welded meshes: mesh(), meshes(), write_results' PLY files and the per-frame meshes become one vertex per grid
        edge (the first soup copy's bits) with the soup's triangles re-indexed, welded on the device.  An output form
        only: no pose, life-cycle decision or image changes."""
        _check("emf_fusion_set_mesh_weld", load().emf_fusion_set_mesh_weld(self._h, int(on)))

    def set_mesh_filter(self, min_triangles=0, largest_objects=False):
        """The component filter: wherever set_mesh_weld acts, every mesh loses its connected components of fewer than
        min_triangles triangles and, with largest_objects, every object mesh all components but its largest (the
        background keeps its pieces).  Done on the device behind the weld; an active filter implies the welded form.
        An output form only; not stored in a checkpoint.  Off: set_mesh_filter()."""
        _check("emf_fusion_set_mesh_filter",
               load().emf_fusion_set_mesh_filter(self._h, int(min_triangles), int(bool(largest_objects))))

    def mesh_components(self, obj_id: int = 0):
        """(labels (n,) i32, sizes (n,) u32) of model obj_id's welded, unfiltered mesh: per vertex the smallest welded
        index of its connected component and that component's triangles."""
        nv = C.c_uint32()
        _check("emf_fusion_mesh_components", load().emf_fusion_mesh_components(self._h, int(obj_id), C.byref(nv)))
        labels, sizes = np.empty((nv.value,), np.int32), np.empty((nv.value,), np.uint32)
        _check("emf_fusion_copy_mesh_components",
               load().emf_fusion_copy_mesh_components(self._h, labels.ctypes.data, sizes.ctypes.data))
        return labels, sizes

    def last_mesh_filter(self):
        """{id: dict(components, kept_components, triangles, kept_triangles)} of the last mesh() / meshes() (or
        write_results / per-frame export) under an active filter; empty without one."""
        cap = 257
        ids, stats, count = np.zeros((cap,), np.int32), np.zeros((cap, 4), np.uint32), C.c_int32()
        _check("emf_fusion_last_mesh_filter",
               load().emf_fusion_last_mesh_filter(self._h, ids.ctypes.data, stats.ctypes.data, cap, C.byref(count)))
        keys = ("components", "kept_components", "triangles", "kept_triangles")
        return {int(ids[k]): dict(zip(keys, (int(x) for x in stats[k]))) for k in range(min(count.value, cap))}

    def set_mesh_simplify(self, cell=0.0):
        """Simplified meshes: wherever set_mesh_weld and the filter act, and in world_mesh() and the slabs retired from
        then on, the vertices of a model's welded, filtered mesh that share a cubic cell of `cell` metres become one
        vertex (ops.simplify_mesh of that mesh, origin 0); collapsed triangles and unreferenced vertices are dropped.
        Done on the device behind the filter; a cell > 0 implies the welded form.  An output form only; not stored in a
        checkpoint.  Off: set_mesh_simplify()."""
        _check("emf_fusion_set_mesh_simplify", load().emf_fusion_set_mesh_simplify(self._h, float(cell)))

    def last_mesh_simplify(self):
        """{id: dict(vertices_in, triangles_in, vertices_out, triangles_out, clusters)} of the last mesh() / meshes() (or
        write_results / per-frame export) with set_mesh_simplify on; empty without it."""
        cap = 257
        ids, stats, count = np.zeros((cap,), np.int32), np.zeros((cap, 5), np.uint32), C.c_int32()
        _check("emf_fusion_last_mesh_simplify",
               load().emf_fusion_last_mesh_simplify(self._h, ids.ctypes.data, stats.ctypes.data, cap, C.byref(count)))
        keys = ("vertices_in", "triangles_in", "vertices_out", "triangles_out", "clusters")
        return {int(ids[k]): dict(zip(keys, (int(x) for x in stats[k]))) for k in range(min(count.value, cap))}

    def set_color_image(self, rgb_view: EmfImage):
        """The u8 x 3 device image (frame size) that goes with the next frame, and with that one only."""
        _check("emf_fusion_set_color_image", load().emf_fusion_set_color_image(self._h, C.byref(rgb_view)))

    def colored_voxels(self) -> int:
        """Voxels the colour pass has updated since the last call (synchronises)."""
        n = C.c_uint64(0)
        _check("emf_fusion_colored_voxels", load().emf_fusion_colored_voxels(self._h, C.byref(n)))
        return int(n.value)

    def use_preproc_masks(self, path):
        """EMFusion::usePreprocMasks: <path>/Mask%04d.plk on every mask frame of process_rgbd."""
        _check("emf_fusion_use_preproc_masks", load().emf_fusion_use_preproc_masks(self._h, os.fspath(path).encode()))

    def last_masks(self):
        """EMFusion::getLastMasks: (instances, (H, W, 3) u8 image or None before the first mask frame)."""
        n = C.c_int32(0)
        img = np.zeros((self.params.height, self.params.width, 3), np.uint8)
        _check("emf_fusion_get_last_masks", load().emf_fusion_get_last_masks(self._h, img.ctypes.data, img.nbytes, C.byref(n)))
        return n.value, img

    def set_motion_masks(self, on=True, band=None, continuity=None, erode=1, min_pixels=200, max_masks=8):
        """Motion masks: a mask frame that ran a raycast and was handed no masks proposes its own instance masks --
        connected regions of pixels measured in front of the background's raycast by more than `band` metres (None:
        the background's truncation distance), neighbours joined across ray-length steps of at most `continuity`
        metres (None: 0.05), after `erode` 3 x 3 erosion passes, at least `min_pixels` large, the `max_masks` largest
        -- and runs them through the object life cycle as queued instance masks would.  Queued or preprocessed masks
        take precedence on a frame that has them.  Off by default; nothing is kept between frames or in a checkpoint
        (a resumed session switches it on again).  Refused on the sharded path."""
        from ._lib import EmfMotionParams
        p = EmfMotionParams(-1.0 if band is None else float(band), 0.05 if continuity is None else float(continuity),
                            int(erode), int(min_pixels), int(max_masks))
        _check("emf_fusion_set_motion_masks", load().emf_fusion_set_motion_masks(self._h, int(bool(on)), C.addressof(p)))

    def set_background_follow(self, on=True, step=(64, 64, 64), look_ahead=0.0, keep_retired=True):
        """Follow the camera: at the end of every frame the background is rolled by whole voxels (multiples of `step`,
        each a positive multiple of the tile (32, 8, 8)) so that the point `look_ahead` metres in front of the camera
        stays within one step of its centre; with `keep_retired` what slides out is meshed first (retired_slabs()).
        Off by default; refused on the sharded path.  save_checkpoint() carries the switch and its parameters only once
        the background has rolled (a never-rolled session's file is the version 1 file byte for byte): a session saved
        before its first roll resumes with follow off, and the caller sets it again, as with the motion masks."""
        p = EmfFollowParams((C.c_int32 * 3)(*[int(v) for v in step]), float(look_ahead), int(bool(keep_retired)))
        _check("emf_fusion_set_background_follow",
               load().emf_fusion_set_background_follow(self._h, int(bool(on)), C.addressof(p)))

    def roll_background(self, shift, keep_retired=None):
        """Roll the background now by `shift` = (x, y, z) voxels: afterwards voxel v holds what v + shift held, zeros
        where that lay outside, and the background's pose is translated by R (shift * voxel_size).  keep_retired None:
        what leaves is meshed and kept (retired_slabs()) if the session's keep_retired says so, which it does by
        default, also with follow off; False: only re-centre, nothing is meshed or kept; True: retire."""
        keep = -1 if keep_retired is None else int(bool(keep_retired))
        _check("emf_fusion_roll_background",
               load().emf_fusion_roll_background(self._h, (C.c_int32 * 3)(*[int(v) for v in shift]), keep))

    def set_background_store(self, on=True, max_bytes=BACKGROUND_STORE_BYTES):
        """Remember what rolls out: the whole tiles (32 x 8 x 8) that a roll moves out of the background are kept on the
        host as the bytes they are and written back -- tsdf, weights, colour, sign and unseen-tile entries -- when a
        later roll moves them in again.  `max_bytes` caps the store (1 GiB by default: a cap, not a measurement); past
        it whole spills are dropped, the oldest first.  With the store on, a roll that is not tile-granular is refused.
        retired_slabs() stays the chronological log it is: a region that leaves twice is logged twice.  Turning the
        store off drops what it holds.  Off by default; refused on the sharded path.  save_checkpoint() of a session
        with the store on writes version 3, which carries the store."""
        _check("emf_fusion_set_background_store",
               load().emf_fusion_set_background_store(self._h, int(bool(on)), int(max_bytes)))

    def background_store_info(self):
        """dict(tiles_held, bytes_held, tiles_spilled, tiles_restored, tiles_evicted) of the background store."""
        out = (C.c_uint64 * 5)()
        _check("emf_fusion_background_store_info", load().emf_fusion_background_store_info(self._h, C.addressof(out)))
        return dict(zip(("tiles_held", "bytes_held", "tiles_spilled", "tiles_restored", "tiles_evicted"), (int(v) for v in out)))

    def background_origin(self):
        """The cumulative roll in voxels, on the lattice whose index (0, 0, 0) is voxel (0, 0, 0) at the initial pose."""
        o = (C.c_int32 * 3)()
        _check("emf_fusion_background_origin", load().emf_fusion_background_origin(self._h, o, None, None))
        return tuple(int(v) for v in o)

    def background_pose(self):
        """(R 3x3, t 3): the background's current pose, volume centre -> world."""
        o, R, t = (C.c_int32 * 3)(), (C.c_float * 9)(), (C.c_float * 3)()
        _check("emf_fusion_background_origin", load().emf_fusion_background_origin(self._h, o, R, t))
        return np.array(R, np.float32).reshape(3, 3), np.array(t, np.float32)

    def retired_slabs(self, colors=False):
        """What the rolls removed, in order: dicts {frame, origin (x, y, z), res (x, y, z), vertices (n, 3), normals
        (n, 3), triangles (m, 4)[, colors (n, 3) u8]}; vertices in the slab's own frame (its centre at 0).  frame: the one at whose
        end the roll happened, which for roll_background() is the last one processed."""
        n = C.c_int32(0)
        _check("emf_fusion_retired_slabs", load().emf_fusion_retired_slabs(self._h, None, 0, C.byref(n)))
        info = np.zeros((max(n.value, 1), 7), np.int32)
        _check("emf_fusion_retired_slabs", load().emf_fusion_retired_slabs(self._h, info.ctypes.data, n.value, C.byref(n)))
        out = []
        for k in range(n.value):
            nv, nt = C.c_uint32(), C.c_uint32()
            _check("emf_fusion_retired_slab_mesh",
                   load().emf_fusion_retired_slab_mesh(self._h, k, C.byref(nv), C.byref(nt)))
            v, nr = np.empty((nv.value, 3), np.float32), np.empty((nv.value, 3), np.float32)
            t = np.empty((nt.value, 4), np.int32)
            _check("emf_fusion_copy_mesh", load().emf_fusion_copy_mesh(self._h, v.ctypes.data, nr.ctypes.data, t.ctypes.data))
            slab = dict(frame=int(info[k, 0]), origin=tuple(int(x) for x in info[k, 1:4]),
                        res=tuple(int(x) for x in info[k, 4:7]), vertices=v, normals=nr, triangles=t)
            if colors:
                c = np.empty((nv.value, 3), np.uint8)
                if nv.value:
                    _check("emf_fusion_copy_mesh_colors", load().emf_fusion_copy_mesh_colors(self._h, c.ctypes.data))
                slab["colors"] = c
            out.append(slab)
        return out

    def world_mesh(self, weld=None, colors=False):
        """ONE mesh of what the session has mapped: the current background's observed tiles plus the
        tiles the background store holds, meshed as one lattice -- no duplicates, no seams.  (vertices (n, 3), normals
        (n, 3), triangles (m, 4)[, colours (n, 3) u8]) in the frame retired_slabs() are written in.  weld None: the
        session's switch; an active set_mesh_filter or set_mesh_simplify implies the weld, and the latter simplifies the
        mesh.  Changes nothing of the session."""
        nv, nt = C.c_uint32(), C.c_uint32()
        _check("emf_fusion_world_mesh",
               load().emf_fusion_world_mesh(self._h, -1 if weld is None else int(bool(weld)), C.byref(nv), C.byref(nt)))
        v, nr = np.empty((nv.value, 3), np.float32), np.empty((nv.value, 3), np.float32)
        t = np.empty((nt.value, 4), np.int32)
        _check("emf_fusion_copy_mesh", load().emf_fusion_copy_mesh(self._h, v.ctypes.data, nr.ctypes.data, t.ctypes.data))
        if not colors:
            return v, nr, t
        c = np.empty((nv.value, 3), np.uint8)
        if nv.value:
            _check("emf_fusion_copy_mesh_colors", load().emf_fusion_copy_mesh_colors(self._h, c.ctypes.data))
        return v, nr, t, c

    def world_mesh_info(self):
        """Of the last world_mesh(): dict(volume_tiles, stored_tiles, duplicate_tiles, stored_surface_cubes)."""
        out = np.zeros(4, np.uint64)
        _check("emf_fusion_world_mesh_info", load().emf_fusion_world_mesh_info(self._h, out.ctypes.data))
        return dict(volume_tiles=int(out[0]), stored_tiles=int(out[1]), duplicate_tiles=int(out[2]),
                    stored_surface_cubes=int(out[3]))

    def camera_box(self, size):
        """The box (lo, size), both (x, y, z) voxels, of `size` voxels (an int or three) centred on the background voxel
        under the camera and clipped to the volume; None if nothing of it lies inside."""
        size = (int(size),) * 3 if np.isscalar(size) else tuple(int(v) for v in size)
        res = np.array(list(self.params.bg_res), np.int64)
        centre = self._box_frame().to_voxels(self.pose(0)[1])[0].astype(np.int64)
        lo = np.maximum(centre - np.array(size) // 2, 0)
        hi = np.minimum(centre - np.array(size) // 2 + np.array(size), res)
        if (hi <= lo).any():
            return None
        return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo)

    def _box_frame(self, lo=(0, 0, 0)):
        """The frame of the box of the background at `lo`, at the background's current pose."""
        return _BoxFrame(*self.background_pose(), self.params.bg_res, self.params.bg_voxel_size, lo)

    def set_query_extent(self, extent):
        """The extent of the scene queries: "background" (the default) or "world".  With "world" the
        box of distance_field, frontiers, plan, cast_rays, view_gain and ground_map may leave the background -- it stays
        in voxels of the current background volume, so lo may be negative and lo + size may exceed the resolution --
        and is classified from the tiles world_mesh() reads: the observed tiles of the volume and every tile the
        background store holds; what lies in no tile is unknown.  Sticky, never in a checkpoint.  A world query is
        refused on the sharded path and when the background's resolution or origin is off the tile (32, 8, 8);
        planes() keeps to the background."""
        if extent not in ("world", "background"):
            raise ValueError(f'set_query_extent: "world" or "background", not {extent!r}')
        _check("emf_fusion_set_query_extent", load().emf_fusion_set_query_extent(self._h, int(extent == "world")))
        self._query_extent = extent

    def query_extent(self):
        return getattr(self, "_query_extent", "background")

    def world_extent(self):
        """(lo, size), both (x, y, z) in voxels of the current background volume: the bounding box of the background
        and every tile the background store holds -- ((0, 0, 0), the resolution) when nothing is stored."""
        lo, size = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        _check("emf_fusion_world_extent", load().emf_fusion_world_extent(self._h, lo, size))
        return tuple(lo), tuple(size)

    def _resolve_box(self, who, box, size):
        """The `box` argument of the query `who`: None, (lo, size), "camera" with `size` for camera_box(size), or
        "world" for world_extent() while the query extent is "world"."""
        if not isinstance(box, str):
            return box
        if box == "world":
            if self.query_extent() != "world":
                raise ValueError(f'{who}: box="world" needs set_query_extent("world")')
            return self.world_extent()
        if box != "camera" or size is None:
            raise ValueError(f'{who}: box="camera" needs a size')
        box = self.camera_box(size)
        if box is None:
            raise ValueError(f"{who}: the camera box lies outside the background")
        return box

    def distance_field(self, box=None, unknown_is_obstacle=False, cap=0.0, exclude=(), signed=False, metres=True,
                       size=None, nearest=False):
        """The distance field of the scene: how far is the nearest obstacle.  Over a box of the
        background -- None: all of it; ((x, y, z) lo, (x, y, z) size) in voxels; "camera" with `size`: centred on the
        voxel under the camera, clipped to the volume -- the occupancy classes (0 free, 1 occupied, 2 unknown) with
        every live object not in `exclude` stamped as occupied at its current pose, and the exact Euclidean distance to
        the nearest occupied voxel (or occupied or unknown, with unknown_is_obstacle).  cap (metres, rounded up to whole
        voxels; 0: none): farther voxels count as having no obstacle.  Returns a dict:
          classes (bz, by, bx) u8; d2 (bz, by, bx) i32, squared voxels, DF_FAR = 0x7fffffff for "none"; metres f32 with
          +inf for "none" (when asked); box (lo, size); pose (R 3x3, t 3) of voxel (0, 0, 0) of the box -> world, the
          background's pose composed with the box origin, so right after rolls too; voxel_size; objects [(id, R, t)]
          stamped, (R, t) = object volume <- background volume.
        signed=True: a second transform from the complement gives d2_inside / metres_inside, the distance from an
        obstacle voxel to the nearest voxel that is none, and `signed` (metres) = +outside, -inside.
        nearest=True: also nearest (bz, by, bx) i32, the linear index (z * by + y) * bx + x in the box of
        the nearest obstacle voxel -- the smallest index among equally near ones -- and -1 exactly where d2 is DF_FAR
        (obstacle_offsets turns it into vectors); with signed=True also nearest_inside, the same for the second
        transform.  The index stays on the device for query_distance."""
        box = self._resolve_box("distance_field", box, size)
        vs = float(self.params.bg_voxel_size)
        cap_voxels = _metres_to_voxels(cap, vs)
        sites = 2 | (4 if unknown_is_obstacle else 0)
        lo_arg, size_arg, ex, n_ex = _box_args(box, exclude)

        def run(mask, want_metres):
            outs = _box_outs()
            entry = "emf_fusion_distance_field_nearest" if nearest else "emf_fusion_distance_field"
            _check(entry, getattr(load(), entry)(self._h, lo_arg, size_arg, mask, cap_voxels, ex, n_ex, int(want_metres), *outs))
            shape = tuple(outs[1])[::-1]
            classes, d2 = np.empty(shape, np.uint8), np.empty(shape, np.int32)
            m = np.empty(shape, np.float32) if want_metres else None
            _check("emf_fusion_copy_distance_field",
                   load().emf_fusion_copy_distance_field(self._h, classes.ctypes.data, d2.ctypes.data,
                                                         m.ctypes.data if want_metres else None))
            index = np.empty(shape, np.int32) if nearest else None
            if nearest:
                _check("emf_fusion_copy_distance_nearest", load().emf_fusion_copy_distance_nearest(self._h, index.ctypes.data))
            return classes, d2, m, *_read_box_outs(*outs), index

        if signed:  # the complement first: the field that stays on the device for query_distance is the outside one
            _, d2_in, m_in, _, _, index_in = run(7 ^ sites, True)
        classes, d2, m, out_box, pose, index = run(sites, metres or signed)
        n = C.c_int32(0)
        _check("emf_fusion_distance_field_objects", load().emf_fusion_distance_field_objects(self._h, None, None, None, 0, C.byref(n)))
        ids, Rs, ts = (C.c_int32 * max(n.value, 1))(), (C.c_float * (9 * max(n.value, 1)))(), (C.c_float * (3 * max(n.value, 1)))()
        _check("emf_fusion_distance_field_objects", load().emf_fusion_distance_field_objects(self._h, ids, Rs, ts, n.value, C.byref(n)))
        objects = [(int(ids[k]), np.array(Rs[9 * k:9 * k + 9], np.float32).reshape(3, 3), np.array(ts[3 * k:3 * k + 3], np.float32))
                   for k in range(n.value)]
        out = dict(classes=classes, d2=d2, box=out_box, pose=pose, voxel_size=vs, objects=objects)
        if metres or signed:
            out["metres"] = m
        if nearest:
            out["nearest"] = index
        if signed:
            out.update(d2_inside=d2_in, metres_inside=m_in, signed=np.where(m > 0, m, -m_in).astype(np.float32))
            if nearest:
                out["nearest_inside"] = index_in
        return out

    def query_distance(self, points):
        """Point queries on the last distance_field(), answered from its arrays on the device: only the
        n points' records cross the bus.  points: (n, 3) world points, each rounded to its voxel exactly as plan()
        rounds world goals and never moved to another one.  Returns a dict of arrays, one entry per point:
          voxel (n, 3) i32, box coordinates (x, y, z); inside (n,) bool: the voxel lies in the field's box;
          class (n,) u8 (255 outside the box); d2 (n,) i32 (DF_FAR outside, beyond the cap or without an obstacle);
          metres (n,) f32 = sqrt(f32(d2)) * voxel size by the field's own formula, +inf for DF_FAR;
          nearest_voxel (n, 3) i32, the nearest obstacle voxel in box coordinates, (-1, -1, -1) where there is none;
          nearest_world (n, 3) f32, its centre in the world frame (float64 through the background's pose, rounded
          once), NaN where there is none; direction (n, 3) f32, the unit vector from the point's voxel toward it in the
          world frame, NaN where there is none or the voxel is the obstacle itself.
        Needs a last distance_field(nearest=True); box, pose and voxel size are the session's current ones."""
        vs = float(self.params.bg_voxel_size)
        c_lo, c_size = (C.c_int32 * 3)(), (C.c_int32 * 3)()  # the box of the last field
        _check("emf_fusion_query_distance", load().emf_fusion_query_distance(self._h, None, 0, None, None, None, c_lo, c_size))
        size = np.array(list(c_size), np.int64)
        frame = self._box_frame(c_lo)
        v = frame.to_voxels(points)
        n = len(v)
        cls, d2, near = np.full(n, 255, np.uint8), np.full(n, 0x7fffffff, np.int32), np.full(n, -1, np.int32)
        flat = np.ascontiguousarray(v.reshape(-1))
        _check("emf_fusion_query_distance",
               load().emf_fusion_query_distance(self._h, flat.ctypes.data, n, cls.ctypes.data, d2.ctypes.data,
                                                near.ctypes.data, None, None))
        inside = ((v >= 0) & (v < size)).all(axis=1)
        with np.errstate(invalid="ignore"):
            metres = np.sqrt(d2.astype(np.float32)) * np.float32(vs)
        metres = np.where(d2 == 0x7fffffff, np.float32(np.inf), metres).astype(np.float32)
        has = near >= 0
        lin = np.where(has, near, 0).astype(np.int64)
        site = frame.unravel(lin, size)
        nearest_voxel = np.where(has[:, None], site, -1).astype(np.int32)
        nearest_world = np.where(has[:, None], frame.world(site), np.nan).astype(np.float32)
        step = (site - v.astype(np.int64)).astype(np.float64) @ frame.R.T  # the rotation of the voxel offset
        norm = np.sqrt((step * step).sum(axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            direction = np.where((has & (norm > 0))[:, None], step / norm[:, None], np.nan).astype(np.float32)
        out = {"voxel": v, "inside": inside, "class": cls, "d2": d2, "metres": metres, "nearest_voxel": nearest_voxel,
               "nearest_world": nearest_world, "direction": direction}
        return out

    def frontiers(self, box=None, min_voxels=8, clearance=0.0, exclude=(), labels=False, size=None):
        """Exploration frontiers of the scene: where the known map ends.  Over a box of the background
        as for distance_field -- None, ((x, y, z) lo, (x, y, z) size) or "camera" with `size` -- and on the same
        occupancy classes (every live object not in `exclude` stamped as occupied): the free voxels with an unknown face
        neighbour inside the box, grouped into 26-connected clusters; clusters of fewer than min_voxels voxels are
        dropped.  clearance (metres, rounded up to whole voxels; 0: none): only frontier voxels at least that far from
        the nearest occupied voxel of the box, i.e. where a robot of that radius can stand.  Returns a dict:
          clusters: a list of dicts, largest first (ties: smallest label), each with label, count, lo and hi (the
          inclusive bounding box), sum (of the members' coordinates) and rep (the representative voxel, a member of the
          cluster nearest its centroid) -- integers, (x, y, z) in box coordinates -- and centroid_world, rep_world:
          float32 points in the world frame, computed from those integers in float64 and rounded once;
          box (lo, size); box_pose (R 3x3, t 3) of voxel (0, 0, 0) of the box -> world; voxel_size;
          kept, n_clusters, n_voxels: clusters kept, all clusters, frontier voxels;
          labels (bz, by, bx) i32 with labels=True: the label of the voxel's cluster, -1 off the frontier."""
        from ._lib import FRONTIER_CLUSTER_DTYPE
        box = self._resolve_box("frontiers", box, size)
        vs = float(self.params.bg_voxel_size)
        lo_arg, size_arg, ex, n_ex = _box_args(box, exclude)
        lo, sz, _, _ = outs = _box_outs()
        counters = np.zeros(3, np.uint32)
        _check("emf_fusion_frontiers",
               load().emf_fusion_frontiers(self._h, lo_arg, size_arg, int(min_voxels), _metres_to_voxels(clearance, vs), ex, n_ex,
                                           *outs, counters.ctypes.data))
        kept = int(counters[0])
        records = np.zeros(kept, np.dtype(FRONTIER_CLUSTER_DTYPE))
        volume = np.empty((sz[2], sz[1], sz[0]), np.int32) if labels else None
        _check("emf_fusion_copy_frontiers",
               load().emf_fusion_copy_frontiers(self._h, records.ctypes.data if kept else None, kept, None, None,
                                                volume.ctypes.data if labels else None))
        world = self._box_frame(lo).world  # the world points: from the integers, in float64, rounded once
        centroid = world(records["sum"].astype(np.float64) / np.maximum(records["count"], 1).astype(np.float64)[:, None])
        rep = world(records["rep"].astype(np.float64))
        clusters = [dict(label=int(r["label"]), count=int(r["count"]), lo=tuple(int(v) for v in r["lo"]),
                         hi=tuple(int(v) for v in r["hi"]), sum=tuple(int(v) for v in r["sum"]),
                         rep=tuple(int(v) for v in r["rep"]), centroid_world=centroid[k], rep_world=rep[k])
                    for k, r in enumerate(records)]
        out_box, box_pose = _read_box_outs(*outs)
        out = dict(clusters=clusters, centroid_world=centroid, rep_world=rep, box=out_box, box_pose=box_pose, voxel_size=vs, kept=kept,
                   n_clusters=int(counters[1]), n_voxels=int(counters[2]), records=records)
        if labels:
            out["labels"] = volume
        return out

    def cast_rays(self, origins, targets, box=None, size=None, clearance=0.0, through_unknown=False, count=("unknown",),
                  exclude=(), group=0):
        """Voxel rays over the scene: can I go, or look, straight from A to B.  Over a box of the
        background as for frontiers -- None, ((x, y, z) lo, (x, y, z) size) or "camera" with `size` -- and on the same
        occupancy classes (every live object not in `exclude` stamped as occupied): one ray per pair of origins[k],
        targets[k], (n, 3) world points each rounded to its voxel and never moved to another one.  A ray is an integer
        walk of |dx| + |dy| + |dz| face steps on the voxel lattice (include/emf_hip.h "Voxel rays") that ends at the
        first voxel that is not free -- or neither free nor unknown, with through_unknown --, that leaves the box or,
        with clearance (metres, rounded up to whole voxels), that is nearer than that to an occupied voxel of the box.
        The origin voxel is never tested.  The walk is NOT symmetric: A -> B and B -> A may visit different voxels.
        count: the classes counted along the way, of "free", "occupied", "unknown".  Returns a dict of arrays, one entry
        per ray: from_voxel, to_voxel (n, 3) i32 box coordinates; status (RAY_*); visible = status == RAY_REACHED; steps,
        the voxels entered and passed; stop_voxel (n, 3) i32, the blocking voxel, -1s where none; stop_world (n, 3) f32
        (float64, rounded once), NaN where none; counted, the passed voxels of a counted class; weighted u64, the sum of
        their squared voxel distances from the origin (a far voxel stands for more solid angle) -- scores, not volumes;
        and box, box_pose, voxel_size, clearance_voxels.  group > 0: also groups, one RAY_GROUP_DTYPE record of sums per
        run of `group` consecutive rays."""
        from ._lib import RAY_GROUP_DTYPE, RAY_RESULT_DTYPE
        box = self._resolve_box("cast_rays", box, size)
        vs = float(self.params.bg_voxel_size)
        names = {"free": 1, "occupied": 2, "unknown": 4}
        count_mask = 0
        for c in count:
            if c not in names:
                raise ValueError('cast_rays: count holds "free", "occupied" or "unknown"')
            count_mask |= names[c]
        clearance_voxels = _metres_to_voxels(clearance, vs)
        frame = self._box_frame(box[0] if box is not None else (0, 0, 0))
        a, b = frame.to_voxels(origins), frame.to_voxels(targets)
        if len(a) != len(b):
            raise ValueError("cast_rays: as many origins as targets")
        n, group = len(a), int(group)
        n_groups = -(-n // group) if group > 0 else 0
        results = np.zeros(n, np.dtype(RAY_RESULT_DTYPE))
        groups = np.zeros(n_groups, np.dtype(RAY_GROUP_DTYPE)) if group > 0 else None
        lo_arg, size_arg, ex, n_ex = _box_args(box, exclude)
        outs = _box_outs()
        flat_a, flat_b = np.ascontiguousarray(a.reshape(-1)), np.ascontiguousarray(b.reshape(-1))
        _check("emf_fusion_cast_rays",
               load().emf_fusion_cast_rays(self._h, lo_arg, size_arg, flat_a.ctypes.data, flat_b.ctypes.data, n,
                                           1 | (4 if through_unknown else 0), count_mask, clearance_voxels, ex, n_ex, group,
                                           results.ctypes.data, groups.ctypes.data if group > 0 else None, *outs))
        out_box, box_pose = _read_box_outs(*outs)
        out = self._ray_records(frame, out_box[1], results)
        out.update(from_voxel=a, to_voxel=b, box=out_box, box_pose=box_pose, voxel_size=vs, clearance_voxels=clearance_voxels)
        if group > 0:
            out["groups"] = groups
        return out

    @staticmethod
    def _ray_records(frame, size, results):
        """The per-ray entries of cast_rays / view_gain from the RAY_RESULT_DTYPE records of a box of `size`."""
        from ._lib import RAY_REACHED
        has = results["stop"] >= 0
        site = frame.unravel(np.where(has, results["stop"], 0), size)
        return dict(status=results["status"].copy(), visible=results["status"] == RAY_REACHED, steps=results["steps"].copy(),
                    stop_voxel=np.where(has[:, None], site, -1).astype(np.int32),
                    stop_world=np.where(has[:, None], frame.world(site), np.nan).astype(np.float32),
                    counted=results["counted"].copy(), weighted=results["weighted"].copy())

    def view_gain(self, views, grid=(32, 24), K=None, range_m=3.0, box=None, size=None, exclude=(), rays=False):
        """View scoring: which candidate pose would see the most unknown space.  views: a list of (R, t),
        viewer -> world in the OpenCV camera convention (as render_view / look_at).  Per view the rays of a grid = (gw, gh)
        image with the intrinsics K (3 x 3; None: the frame's, scaled to the grid as default_3d_view scales them), range_m
        metres long, from the voxel under the camera to integer targets computed on the host in float64
        (view_ray_targets); all views in one launch over a box of the background as for cast_rays.  A ray sees through
        free and unknown space and stops at the first occupied voxel; the unknown voxels it passes are counted.  The
        counts are SCORES, not volumes: rays share voxels near the origin, and a diagonal ray enters up to sqrt(3) times
        more voxels per metre than an axis-parallel one.  Returns a dict of arrays, one entry per view: origin_voxel
        (n, 3) i32; inside: the camera stands in the box (else zero counts); unknown, the unknown voxels passed; weighted
        u64, each weighted by its squared voxel distance from the camera; reached, blocked, left: rays by how they ended;
        and order: the views' indices by weighted, descending, ties to the lower index; box, box_pose, voxel_size.
        rays=True: also targets (n, gh, gw, 3) i32 and rays, the per-ray entries of cast_rays as (n * gh * gw,) arrays."""
        from ._lib import RAY_GROUP_DTYPE, RAY_RESULT_DTYPE
        box = self._resolve_box("view_gain", box, size)
        vs = float(self.params.bg_voxel_size)
        gw, gh = int(grid[0]), int(grid[1])
        if K is None:
            K = np.array(self.params.K, np.float32).reshape(3, 3)
            sx, sy = np.float32(gw / self.params.width), np.float32(gh / self.params.height)
            K[0, 0] *= sx
            K[0, 2] *= sx
            K[1, 1] *= sy
            K[1, 2] *= sy
        K = np.asarray(K, np.float64).reshape(3, 3)
        k4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
        n = len(views)
        Rs = np.ascontiguousarray(np.array([np.asarray(v[0], np.float64).reshape(9) for v in views], np.float64).reshape(n, 9))
        ts = np.ascontiguousarray(np.array([np.asarray(v[1], np.float64).reshape(3) for v in views], np.float64).reshape(n, 3))
        groups = np.zeros(n, np.dtype(RAY_GROUP_DTYPE))
        origins = np.zeros((n, 3), np.int32)
        targets = np.zeros((n, gh, gw, 3), np.int32) if rays else None
        results = np.zeros(n * gh * gw, np.dtype(RAY_RESULT_DTYPE)) if rays else None
        lo_arg, size_arg, ex, n_ex = _box_args(box, exclude)
        outs = _box_outs()
        _check("emf_fusion_view_gain",
               load().emf_fusion_view_gain(self._h, Rs.ctypes.data, ts.ctypes.data, n, gw, gh, k4.ctypes.data, float(range_m),
                                           lo_arg, size_arg, ex, n_ex, groups.ctypes.data, origins.ctypes.data,
                                           targets.ctypes.data if rays else None, results.ctypes.data if rays else None, *outs))
        out_box, box_pose = _read_box_outs(*outs)
        inside = ((origins >= 0) & (origins < np.array(out_box[1], np.int64))).all(axis=1)
        weighted = groups["weighted"].copy()
        order = np.array(sorted(range(n), key=lambda v: (-int(weighted[v]), v)), np.int64)
        out = dict(origin_voxel=origins, inside=inside, unknown=groups["counted"].copy(), weighted=weighted,
                   reached=groups["reached"].copy(), blocked=groups["blocked"].copy(), left=groups["left"].copy(), order=order,
                   groups=groups, box=out_box, box_pose=box_pose, voxel_size=vs, K=k4)
        if rays:
            frame = self._box_frame(out_box[0])
            out.update(targets=targets, rays=self._ray_records(frame, out_box[1], results), records=results)
        return out

    def plan(self, goals="frontiers", start=None, box=None, size=None, clearance=0.0, start_radius=None,
             through_unknown=False, max_cost=0.0, exclude=(), min_voxels=8, field=False, shortcut=0):
        """Path planning over the scene: can the robot get there, by which way, at what cost.  Over a
        box of the background as for frontiers -- None, ((x, y, z) lo, (x, y, z) size) or "camera" with `size` -- and on
        the same occupancy classes (every live object not in `exclude` stamped as occupied): the cost-to-go field from
        `start` (None: the voxel under the camera, or the nearest voxel of the background where the camera is outside; else (n, 3) world points, each rounded to its voxel) through the free
        voxels -- and the unknown ones with through_unknown -- at least `clearance` metres (rounded up to whole voxels)
        from the nearest occupied voxel of the box, plus whatever is not occupied within start_radius metres of a start
        (None: max(clearance, one voxel); rounded up to whole voxels): the robot stands there, and the sensor does not
        see its own near field.  Moves are 26-connected with the integer weights 3 / 4 / 5 for face / edge / corner
        steps; max_cost (metres of face steps, 0: none) stops the search at max(floor(3 * max_cost / voxel), 1).
        goals="frontiers": self.frontiers(box, min_voxels, clearance, exclude) and a plan to every kept cluster's
        representative; else (n, 3) world points, each rounded to its voxel and never moved to another one.  A start or
        goal with a coordinate that is not finite becomes a voxel outside the box: a goal without a path, a start that is ignored.
        Returns a dict:
          goals: one dict per goal -- with "frontiers" the cluster's record of frontiers() -- that gains voxel (box
          coordinates), reachable, cost (the chamfer cost; PLAN_UNREACHED / PLAN_BLOCKED without a path), length_m =
          (faces + sqrt 2 edges + sqrt 3 corners) * voxel in float64, steps (faces, edges, corners), path_vox (k, 3) i32
          box voxels from the goal to the start, path_world (k, 3) f32 (float64, rounded once).  With "frontiers" the
          reachable clusters come first, cheapest first, then the rest in the frontier order; `clusters` is the same list;
          start_voxels (box coordinates), start_radius_voxels, clearance_voxels; box (lo, size); box_pose; voxel_size;
          converged, rounds, n_finite, n_starts: the counters; frontiers: what frontiers() returned (with "frontiers");
          cost (bz, by, bx) u32 with field=True.
        shortcut=W > 0: every goal also gains waypoints -- ascending indices into its path, from 0 to the
        last one: from index i the farthest of the next W path voxels that a voxel ray from path[i] reaches through the
        plan's own traversable voxels (its classes and clearance, without the start bubble), else i + 1 --,
        waypoints_vox, waypoints_world and waypoints_length_m, the sum of the Euclidean voxel distances between
        consecutive waypoints times the voxel size, in float64.  The default 0 changes nothing and makes no new call."""
        from ._lib import PLAN_BLOCKED
        box = self._resolve_box("plan", box, size)
        vs = float(self.params.bg_voxel_size)
        clearance_voxels = _metres_to_voxels(clearance, vs)
        radius_voxels = max(clearance_voxels, 1) if start_radius is None else _metres_to_voxels(start_radius, vs)
        # at least 1: a positive cap below a third of a voxel must not turn into 0, which means "no cap"
        cost_cap = min(max(int(np.floor(3.0 * float(max_cost) / vs)), 1), PLAN_BLOCKED - 1) if max_cost > 0 else 0
        frame = self._box_frame(box[0] if box is not None else (0, 0, 0))
        found = None
        if isinstance(goals, str):
            if goals != "frontiers":
                raise ValueError('plan: goals is "frontiers" or an (n, 3) array of world points')
            found = self.frontiers(box=box, min_voxels=min_voxels, clearance=clearance, exclude=exclude)
            goal_voxels = np.array([c["rep"] for c in found["clusters"]], np.int32).reshape(-1, 3)
        else:
            goal_voxels = frame.to_voxels(goals)
        if start is None:  # the voxel under the camera; the nearest voxel of the background where it stands outside
            cam = frame.to_voxels(self.pose(0)[1]).astype(np.int64) + frame.lo
            start_voxels = (np.clip(cam, 0, frame.res.astype(np.int64) - 1) - frame.lo).astype(np.int32)
        else:
            start_voxels = frame.to_voxels(start)
        n_goals = len(goal_voxels)
        lo_arg, size_arg, ex, n_ex = _box_args(box, exclude)
        outs = _box_outs()
        sz = outs[1]
        counters, longest = np.zeros(4, np.uint32), C.c_int32(0)
        starts = np.ascontiguousarray(start_voxels.reshape(-1))
        flat_goals = np.ascontiguousarray(goal_voxels.reshape(-1)) if n_goals else np.zeros(3, np.int32)
        _check("emf_fusion_plan",
               load().emf_fusion_plan(self._h, lo_arg, size_arg, starts.ctypes.data_as(C.POINTER(C.c_int32)), len(start_voxels),
                                      radius_voxels, int(bool(through_unknown)), clearance_voxels, cost_cap,
                                      flat_goals.ctypes.data_as(C.POINTER(C.c_int32)), n_goals, -1, ex, n_ex, *outs,
                                      counters.ctypes.data, C.byref(longest)))
        cap = int(longest.value)
        goal_cost, lengths = np.zeros(n_goals, np.uint32), np.zeros(n_goals, np.int32)
        steps, paths = np.zeros((n_goals, 3), np.int32), np.full((n_goals, max(cap, 1)), -1, np.int32)
        volume = np.empty((sz[2], sz[1], sz[0]), np.uint32) if field else None
        _check("emf_fusion_copy_plan",
               load().emf_fusion_copy_plan(self._h, goal_cost.ctypes.data, lengths.ctypes.data, steps.ctypes.data,
                                           paths.ctypes.data, cap, None, volume.ctypes.data if field else None))
        records = []
        for g in range(n_goals):
            k = max(int(lengths[g]), 0)
            vox = frame.unravel(paths[g, :k], sz).astype(np.int32)
            r = dict(found["clusters"][g]) if found is not None else {}
            f, e, c = (int(v) for v in steps[g])
            r.update(voxel=tuple(int(v) for v in goal_voxels[g]), reachable=k > 0, cost=int(goal_cost[g]),
                     length_m=(f + np.sqrt(2.0) * e + np.sqrt(3.0) * c) * np.float64(vs), steps=(f, e, c), path_vox=vox,
                     path_world=frame.world(vox))
            records.append(r)
        if shortcut > 0:
            counts, most = np.zeros(max(n_goals, 1), np.int32), C.c_int32(0)
            _check("emf_fusion_plan_shortcut", load().emf_fusion_plan_shortcut(self._h, int(shortcut), counts.ctypes.data, C.byref(most)))
            ways = np.full((max(n_goals, 1), max(int(most.value), 1)), -1, np.int32)
            _check("emf_fusion_copy_plan_shortcut", load().emf_fusion_copy_plan_shortcut(self._h, ways.ctypes.data, ways.shape[1]))
            for g, r in enumerate(records):
                w = ways[g, :int(counts[g])].copy()
                vox = r["path_vox"][w]
                hops = np.diff(vox.astype(np.float64), axis=0)
                r.update(waypoints=w, waypoints_vox=vox, waypoints_world=r["path_world"][w],
                         waypoints_length_m=np.sqrt((hops * hops).sum(axis=1)).sum() * np.float64(vs))
        if found is not None:  # reachable first, cheapest first (stable: ties and the rest keep the frontier order)
            records = sorted(records, key=lambda r: (not r["reachable"], r["cost"] if r["reachable"] else 0))
        out_box, box_pose = _read_box_outs(*outs)
        out = dict(goals=records, start_voxels=start_voxels, start_radius_voxels=radius_voxels, clearance_voxels=clearance_voxels,
                   max_cost=cost_cap, box=out_box, box_pose=box_pose, voxel_size=vs,
                   converged=bool(counters[0]), rounds=int(counters[1]), n_finite=int(counters[2]), n_starts=int(counters[3]))
        if found is not None:
            out.update(clusters=records, frontiers=found)
        if field:
            out["cost"] = volume
        return out

    def object_shapes(self, ids=None, background=False):
        """Where in its volume each object is, how large it is, how it is oriented and how much of its surface has been
        seen, computed on the device from the volumes as they are: one launch for the integer moments of
        all asked models, the frames on the host, one launch for the extents along them.

        WHAT IS MEASURED IS THE OBSERVED SOLID BAND, NOT THE BODY.  A TSDF observes a band around the surface; the
        interior of an object has weight 0.  solid counts the voxels with weight > 0, a set foreground bit and tsdf <= 0
        (the rule by which the distance field calls an object solid), so neither a count nor a box here is a volume in
        cubic metres, and the box bounds what has been seen so far.

        ids: live object ids (default: all of them, in creation order); background=True puts the background (id 0) in
        front.  An id that does not exist raises.  Returns a list of dicts, per model: id, valid (False: no solid voxel;
        everything from centroid_vox on is None then), solid, observed, faces_free, faces_unknown (voxel faces of the
        band towards seen free space / towards space nobody has seen), completeness = faces_free / (faces_free +
        faces_unknown) (NaN without either), bounds_vox = (lo, hi) of the solid voxels, res, voxel_size, pose = (R, t)
        volume -> world as the call found it (Fusion.pose(id) for an object), centroid_vox, axes (3 x 3 rows, sorted by
        eigenvalue, right-handed), eigenvalues (voxels^2), extents_vox = (lo, hi) along the axes about the centroid
        (f32), box_center_vox, box_half_vox; box_center, box_half, box_corners (8 x 3) in the model's own frame in
        metres, p = (v - (res - 1) / 2) * voxel_size; box_center_world, box_axes_world, box_corners_world through the
        pose.  Float64, rounded once.  The raw records are under moments, frame, extents and box.  Changes nothing of
        the session; refused on the sharded path."""
        md, fd, ed, bd = _shape_dtypes()
        ids = self.object_ids() if ids is None else [int(i) for i in ids]
        n = len(ids) + (1 if background else 0)
        arr = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1)) if ids else np.zeros(1, np.int32)
        ids_out, res, vs, poses = (np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 3), np.int32),
                                   np.zeros(max(n, 1), np.float32), np.zeros((max(n, 1), 12), np.float32))
        mom, fr, ex, bx = np.zeros(max(n, 1), md), np.zeros(max(n, 1), fd), np.zeros(max(n, 1), ed), np.zeros(max(n, 1), bd)
        _check("emf_fusion_object_shapes",
               load().emf_fusion_object_shapes(self._h, arr.ctypes.data, len(ids), int(bool(background)), ids_out.ctypes.data,
                                               res.ctypes.data, vs.ctypes.data, poses.ctypes.data, mom.ctypes.data,
                                               fr.ctypes.data, ex.ctypes.data, bx.ctypes.data))
        out = []
        for k in range(n):
            m, f, e, b = mom[k], fr[k], ex[k], bx[k]
            valid = bool(f["valid"])
            r = dict(id=int(ids_out[k]), valid=valid, solid=int(m["solid"]), observed=int(m["observed"]),
                     faces_free=int(m["faces_free"]), faces_unknown=int(m["faces_unknown"]),
                     bounds_vox=(m["lo"].copy(), m["hi"].copy()), res=tuple(int(v) for v in res[k]), voxel_size=float(vs[k]),
                     pose=(poses[k, :9].reshape(3, 3).copy(), poses[k, 9:].copy()), moments=m.copy(), frame=f.copy(),
                     extents=e.copy(), box=b.copy())
            faces = r["faces_free"] + r["faces_unknown"]
            r["completeness"] = float(b["completeness"]) if valid else (r["faces_free"] / faces if faces else float("nan"))
            for key, value in (("centroid_vox", f["centroid"]), ("axes", f["axes"].reshape(3, 3)), ("eigenvalues", f["eigenvalues"]),
                               ("extents_vox", (e["lo"], e["hi"])), ("box_center_vox", b["center_vox"]),
                               ("box_half_vox", b["half_vox"]), ("box_center", b["center_obj"]), ("box_half", b["half_m"]),
                               ("box_corners", b["corners_obj"].reshape(8, 3)), ("box_center_world", b["center_world"]),
                               ("box_axes_world", b["axes_world"].reshape(3, 3)),
                               ("box_corners_world", b["corners_world"].reshape(8, 3))):
                r[key] = (tuple(v.copy() for v in value) if isinstance(value, tuple) else value.copy()) if valid else None
            out.append(r)
        return out

    def object_contacts(self, ids=None, background=True, touch=None):
        """Whether objects touch each other or the scene, how far apart their surfaces are and whether they interpenetrate
        (DESIGN.md 5.27), read on the device from the signed-distance volumes as they are: every surface voxel of a
        PROBE a is taken through the relative pose into a FIELD b's volume and b's tsdf is sampled there trilinearly --
        one launch for all ordered pairs, one wait.

        IT MEASURES WHAT THE VOLUMES SAY.  A tsdf is clamped to +-1, so a summary with saturated=True means "at least
        one truncation distance apart" and its distance_m is no distance.  Nothing is fused deeper than one truncation
        distance behind a surface, so a deeper penetration reads `unknown`, not a larger depth.  A surface voxel lies up
        to one voxel behind the probe's zero crossing, so clearances read up to one probe voxel large.

        ids: live object ids, each once (default: all of them, in creation order): the probes.  The fields are those
        objects and, with background=True, the background (id 0), so a-versus-background says whether an object rests
        on the scene; the background is never a probe.  touch: the `touching` threshold in metres; None means one voxel
        of the probe -- A POLICY, NOT A MEASUREMENT.  An id that does not exist raises.

        Returns dict(pairs=, summaries=, ids=, sides=).  pairs: one dict per ordered pair, grouped by probe: a, b (ids),
        R, t (b's frame <- a's), touch (in units of b's stored tsdf), the counts surface = outside + unknown + masked +
        sampled, inside, touching, normals, then min_s, sum, gsum, lo, hi and the raw `record` and `pair`.  summaries:
        one dict per unordered pair: a, b, state ("unseen", "apart", "touching", "penetrating"), distance_m, saturated,
        direction (0: a -> b, 1: b -> a, None), point, normal (world, out of the probe of `direction`; None without),
        corners (8 x 3, world) and the raw `summary`, with record_ab / record_ba the indices into pairs (None: b was no
        probe).  Changes nothing of the session; refused on the sharded path."""
        from ._lib import CONTACT_STATES
        pd, cd, sd, ud = _contact_dtypes()
        ids = self.object_ids() if ids is None else [int(i) for i in ids]
        n, bg = len(ids), 1 if background else 0
        m = n + bg
        n_pairs, n_sum = n * max(m - 1, 0), n * (n - 1) // 2 + (n if bg else 0)
        arr = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1)) if ids else np.zeros(1, np.int32)
        ids_out, sides = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), sd)
        pair_ids, pairs, recs = np.zeros((max(n_pairs, 1), 2), np.int32), np.zeros(max(n_pairs, 1), pd), np.zeros(max(n_pairs, 1), cd)
        sum_ids, sums = np.zeros((max(n_sum, 1), 4), np.int32), np.zeros(max(n_sum, 1), ud)
        got_pairs, got_sums = C.c_int32(0), C.c_int32(0)
        _check("emf_fusion_object_contacts",
               load().emf_fusion_object_contacts(self._h, arr.ctypes.data, n, bg, -1.0 if touch is None else float(touch),
                                                 ids_out.ctypes.data, sides.ctypes.data, pair_ids.ctypes.data, pairs.ctypes.data,
                                                 recs.ctypes.data, sum_ids.ctypes.data, sums.ctypes.data, C.byref(got_pairs),
                                                 C.byref(got_sums)))
        assert got_pairs.value == n_pairs and got_sums.value == n_sum, (got_pairs.value, n_pairs, got_sums.value, n_sum)
        out_pairs = []
        for k in range(n_pairs):
            r, p = recs[k], pairs[k]
            d = dict(a=int(pair_ids[k, 0]), b=int(pair_ids[k, 1]), R=p["R"].reshape(3, 3).copy(), t=p["t"].copy(),
                     touch=float(p["touch"]), min_s=float(r["min_s"]), sum=r["sum"].copy(), gsum=r["gsum"].copy(),
                     lo=r["lo"].copy(), hi=r["hi"].copy(), record=r.copy(), pair=p.copy())
            for key in ("surface", "outside", "unknown", "masked", "sampled", "inside", "touching", "normals"):
                d[key] = int(r[key])
            out_pairs.append(d)
        out_sums = []
        for k in range(n_sum):
            u = sums[k]
            direction = int(u["direction"])
            out_sums.append(dict(a=int(sum_ids[k, 0]), b=int(sum_ids[k, 1]), record_ab=int(sum_ids[k, 2]),
                                 record_ba=None if sum_ids[k, 3] < 0 else int(sum_ids[k, 3]),
                                 state=CONTACT_STATES[int(u["state"])], distance_m=float(u["distance_m"]),
                                 saturated=bool(u["saturated"]), direction=None if direction < 0 else direction,
                                 point=None if direction < 0 else u["point"].copy(),
                                 normal=u["normal"].copy() if u["has_normal"] else None,
                                 corners=None if direction < 0 else u["corners"].reshape(8, 3).copy(), summary=u.copy()))
        return dict(pairs=out_pairs, summaries=out_sums, ids=[int(v) for v in ids_out[:m]], sides=sides[:m].copy())

    @staticmethod
    def _absorb_event(e):
        return dict(id=int(e["id"]), frame=int(e["frame"]), clipped=bool(e["clipped"]), R=e["R"].reshape(3, 3).copy(),
                    t=e["t"].copy(), lo=tuple(int(v) for v in e["lo"]), size=tuple(int(v) for v in e["size"]),
                    record=e["record"].copy())

    def set_absorb_objects(self, on=True):
        """Absorb objects that leave view into the background.  Sticky, off by default.  On: an object
        that the frame's clean-up (set_cleanup) deletes BECAUSE IT IS NOT VISIBLE any more has the band of its signed-
        distance volume resampled through the relative pose into the background volume and fused there by the
        background's running average before it is erased, so that distance_field(), plan(), ground_map(), world_mesh(),
        the tile store and a checkpoint keep what was mapped.  Objects deleted as spurious (low existence, association
        mass below assocThresh) and a person under set_ignore_person are not absorbed.

        WHAT IT DOES NOT DO: it carries the band, not the free space around it (saturated samples are left alone);
        in a coloured session (enable_color) the colour entries of the fused voxels go with it and absorbed_colors() counts
        them, in a colourless one no call changes; an absorbed object that later moves leaves a ghost until free space carves it; what lies
        outside the background's cube is clipped and lost; objects are not merged with each other and none is seeded
        from the background.  Neither the switch nor the log (absorbed()) is written to a checkpoint: no checkpoint byte
        changes.  Off: no launch and no output byte changes.  Refused on the sharded path."""
        _check("emf_fusion_set_absorb_objects", load().emf_fusion_set_absorb_objects(self._h, int(bool(on))))

    def absorb_object(self, obj_id):
        """Absorb the LIVE object obj_id into the background now (see set_absorb_objects; the switch need not be on) and
        remove it from the session as a deletion would -- leaving it live would let two models explain one surface; with
        the pose log on its mesh is kept.  An explicit call absorbs what it names, a person under set_ignore_person too.
        Returns the event: dict(id, frame, clipped, R, t (object volume frame <-
        background volume frame), lo, size (the box of background voxels), record (ops.ABSORB_DTYPE)).  An unknown id, the
        background (0) and an object this rank does not own raise; refused on the sharded path."""
        e = np.zeros((), _absorb_event_dtype())
        _check("emf_fusion_absorb_object", load().emf_fusion_absorb_object(self._h, int(obj_id), e.ctypes.data))
        return self._absorb_event(e)

    def absorbed(self):
        """The session's log of absorbed objects, oldest first: a list of the events of absorb_object().  Session state
        only: reset() and a loaded checkpoint start it empty, and it is never written to a checkpoint."""
        n = C.c_int32(0)
        _check("emf_fusion_absorbed", load().emf_fusion_absorbed(self._h, None, 0, C.byref(n)))
        events = np.zeros(max(n.value, 1), _absorb_event_dtype())
        _check("emf_fusion_absorbed", load().emf_fusion_absorbed(self._h, events.ctypes.data, n.value, C.byref(n)))
        return [self._absorb_event(events[k]) for k in range(n.value)]

    def absorbed_colors(self):
        """The colour records of absorbed(), one per event in its order (numpy records of ops.COLOR_MOVED_DTYPE: colored +
        uncolored == the event's fused voxels): how many colour entries went into the background with the band
        (DESIGN.md 5.31).  Zeros for the events of a colourless session.  Session state like the log."""
        from . import _lib as hip
        n = C.c_int32(0)
        _check("emf_fusion_absorbed_colors", load().emf_fusion_absorbed_colors(self._h, None, 0, C.byref(n)))
        records = np.zeros(max(n.value, 1), np.dtype(hip.COLOR_MOVED_DTYPE))
        _check("emf_fusion_absorbed_colors", load().emf_fusion_absorbed_colors(self._h, records.ctypes.data, n.value, C.byref(n)))
        return [records[k].copy() for k in range(n.value)]

    @staticmethod
    def _lift_event(e):
        return dict(id=int(e["id"]), frame=int(e["frame"]), clipped=bool(e["clipped"]), seed_R=e["seed_R"].reshape(3, 3).copy(),
                    seed_t=e["seed_t"].copy(), release_R=e["release_R"].reshape(3, 3).copy(), release_t=e["release_t"].copy(),
                    lo=tuple(int(v) for v in e["lo"]), size=tuple(int(v) for v in e["size"]), seed=e["seed"].copy(),
                    release=e["release"].copy())

    def set_lift_objects(self, on=True):
        """Lift new objects out of the background, the other half of set_absorb_objects.  Sticky, off by
        default.  On: every object a frame creates from a mask is SEEDED, after the frame's integration and before its
        masks are integrated, with the band the background holds inside its cube -- only where the object has no
        observation of its own -- and after the masks the background RELEASES the band voxels the object holds as
        foreground (its fgmask), so that one surface has one explanation and no ghost stays when the object moves.  The
        frame's own mask classifies the seeded voxels: under it they are foreground at once; seeded table or floor inside
        the cube becomes background and is never raycast.

        In a coloured session (enable_color) the seeded voxels take the background's colour entries, the released voxels'
        entries are cleared and lifted_colors() counts both.  WHAT IT DOES NOT DO: a voxel
        behind the object along a mask ray inside the cube is claimed and released too (a hole in the table under a cup);
        an object discovered by motion masks sits where the background holds free space: the seed finds nothing there
        and the ghost at the OLD place is not addressed.  Neither the switch nor the log (lifted()) is written to a
        checkpoint: no checkpoint byte changes.  Off: no launch and no output byte changes.  Refused on the sharded
        path."""
        _check("emf_fusion_set_lift_objects", load().emf_fusion_set_lift_objects(self._h, int(bool(on))))

    def lift_object(self, obj_id):
        """Seed, then release, for the LIVE object obj_id now (see set_lift_objects; the switch need not be on); the
        object stays live.  ITS SEEDED VOXELS CARRY NO FOREGROUND COUNT UNTIL THE NEXT MASK FRAME: until then they are
        neither raycast nor released.  Returns the event: dict(id, frame, clipped, seed_R, seed_t (background volume frame
        <- object volume frame), release_R, release_t (the opposite), lo, size (the box of background voxels the release
        covered), seed (ops.SEED_DTYPE), release (ops.RELEASE_DTYPE)).  An unknown id, the background (0) and an object
        this rank does not own raise; refused on the sharded path."""
        e = np.zeros((), _lift_event_dtype())
        _check("emf_fusion_lift_object", load().emf_fusion_lift_object(self._h, int(obj_id), e.ctypes.data))
        return self._lift_event(e)

    def lifted(self):
        """The session's log of lifted objects, oldest first: a list of the events of lift_object().  Session state
        only: reset() and a loaded checkpoint start it empty, and it is never written to a checkpoint."""
        n = C.c_int32(0)
        _check("emf_fusion_lifted", load().emf_fusion_lifted(self._h, None, 0, C.byref(n)))
        events = np.zeros(max(n.value, 1), _lift_event_dtype())
        _check("emf_fusion_lifted", load().emf_fusion_lifted(self._h, events.ctypes.data, n.value, C.byref(n)))
        return [self._lift_event(events[k]) for k in range(n.value)]

    def lifted_colors(self):
        """The colour records of lifted(), one pair (seed, release) per event in its order (numpy records of
        ops.COLOR_MOVED_DTYPE: colored + uncolored == the seeded / the released voxels): the colour entries the new object
        took from the background and those the background gave up.  Zeros for a colourless session."""
        from . import _lib as hip
        n = C.c_int32(0)
        _check("emf_fusion_lifted_colors", load().emf_fusion_lifted_colors(self._h, None, 0, C.byref(n)))
        records = np.zeros(2 * max(n.value, 1), np.dtype(hip.COLOR_MOVED_DTYPE))
        _check("emf_fusion_lifted_colors", load().emf_fusion_lifted_colors(self._h, records.ctypes.data, n.value, C.byref(n)))
        return [(records[2 * k].copy(), records[2 * k + 1].copy()) for k in range(n.value)]

    @staticmethod
    def _merge_event(e):
        out = dict(dst=int(e["dst"]), src=int(e["src"]), frame=int(e["frame"]), clipped=bool(e["clipped"]),
                   automatic=bool(e["automatic"]), res_before=int(e["res_before"]), res_after=int(e["res_after"]),
                   lo=tuple(int(v) for v in e["lo"]), size=tuple(int(v) for v in e["size"]), overlap=e["overlap"].copy(),
                   record=e["record"].copy(), counts=e["counts"].copy(), color=e["color"].copy())
        for k in ("dst_R", "src_R", "R"):
            out[k] = e[k].reshape(3, 3).copy()
        for k in ("dst_t", "src_t", "t"):
            out[k] = e[k].copy()
        return out

    def set_merge_objects(self, on=True, min_overlap=0.5, min_surface=64, touch=None, max_res=256):
        """Merge DUPLICATE objects automatically.  Sticky, off by default; the parameters are kept either
        way (merge_objects grows up to max_res).  On: at the end of every mask frame, after the clean-up, with at least two
        live objects, one contact-probe launch over all ordered object pairs (object_contacts without the background);
        overlap(a -> b) = touching / surface of the record; a pair qualifies when max(overlap(a -> b), overlap(b -> a)) >=
        min_overlap and both surfaces hold at least min_surface voxels; qualifying pairs are merged in descending overlap,
        ties to the smaller pair of ids, the older object (smaller id) the destination, an object at most once per frame.
        THE DEFAULTS ARE POLICY, NOT MEASUREMENTS: min_overlap 0.5, min_surface 64, touch None = half a truncation
        distance (metres otherwise), max_res 256.
        IT FINDS DUPLICATES.  Two halves that merely abut reach no sensible overlap: merge them with merge_objects or by
        a rule of your own on object_contacts().  Neither the switch nor the log is written to a checkpoint.  Off: no
        launch, no output byte, no checkpoint byte changes.  Refused on the sharded path."""
        _check("emf_fusion_set_merge_objects",
               load().emf_fusion_set_merge_objects(self._h, int(bool(on)), float(min_overlap), int(min_surface),
                                                   -1.0 if touch is None else float(touch), int(max_res)))

    def merge_objects(self, dst, src):
        """Merge the LIVE object src into the LIVE object dst now, between frames: the repair for one
        physical thing that ended up with two volumes.  GROWS dst's cube until it holds src's band (the resize of the union
        of both bands, merge_union; set_merge_objects' max_res caps the grown resolution per axis -- 256, a policy value,
        not a measurement -- and beyond it dst is not grown and `clipped` says so), MERGES src's band into dst through the relative pose and
        dst's running average, the (fg, bg) counts of every fused voxel following the band (ops.merge_volume; with colour
        in a coloured session), and sums the existence counts and the class scores.  dst keeps its id and its tracking
        state; src is deleted and NEITHER ITS MESH NOR ITS exp_vols COPY IS KEPT: its geometry lives on in dst.

        WHAT IT DOES NOT DO: the poses are taken as they are -- the volumes are not registered first, a drifted duplicate
        merges blurred; it carries the band, not the free space around it.
        Returns the event: dict(dst, src, frame, clipped, automatic (False here), res_before, res_after, dst_R, dst_t, src_R, src_t
        (the poses used, dst's after the growth), R, t (src volume frame <- dst volume frame), lo, size (the box of dst's
        voxels), overlap, record (ops.ABSORB_DTYPE), counts (ops.MERGE_COUNTS_DTYPE), color (ops.COLOR_MOVED_DTYPE)).  Id
        0, an unknown id, dst == src and an object this rank does not own raise; refused on the sharded path."""
        e = np.zeros((), _merge_event_dtype())
        _check("emf_fusion_merge_objects", load().emf_fusion_merge_objects(self._h, int(dst), int(src), e.ctypes.data))
        return self._merge_event(e)

    def object_bookkeeping(self, obj_id):
        """(exists, not exists, class scores) of the live object obj_id: the frames it was matched and was not, and its
        accumulated class scores (a float64 array, empty before any score) -- what a merge sums."""
        ex, non, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        fn = load().emf_fusion_object_bookkeeping
        _check("emf_fusion_object_bookkeeping", fn(self._h, int(obj_id), C.byref(ex), C.byref(non), None, 0, C.byref(n)))
        scores = np.zeros(max(n.value, 1), np.float64)
        _check("emf_fusion_object_bookkeeping",
               fn(self._h, int(obj_id), C.byref(ex), C.byref(non), scores.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
        return ex.value, non.value, scores[:n.value]

    def merged(self):
        """The session's log of merges, oldest first: a list of the events of merge_objects().  Session state only:
        reset() and a loaded checkpoint start it empty, and it is never written to a checkpoint."""
        n = C.c_int32(0)
        _check("emf_fusion_merged", load().emf_fusion_merged(self._h, None, 0, C.byref(n)))
        events = np.zeros(max(n.value, 1), _merge_event_dtype())
        _check("emf_fusion_merged", load().emf_fusion_merged(self._h, events.ctypes.data, n.value, C.byref(n)))
        return [self._merge_event(events[k]) for k in range(n.value)]

    def planes(self, box=None, size=None, k=15, angle=20.0, separation=None, bin=None, band=None, min_votes=None, refine=1,
               up_hint=None, floor_angle=30.0, kind_angle=10.0, max_planes=64, labels=False, patches=False, patch_reach=1,
               patch_min_voxels=None):
        """What the scene is made of: the dominant planes -- floor, walls, table tops -- of a box of the
        background: None, ((x, y, z) lo, (x, y, z) size) or "camera" with `size`, as for distance_field.  On the device
        the surface voxels (solid with a free face neighbour) with their TSDF gradients vote for a direction on a cube
        map of k cells per face side, then for an offset along each chosen direction in slots of `bin` voxels; every
        surface voxel whose gradient is within `angle` degrees of a plane's normal and that lies within `band` voxels
        of it joins the nearest such plane, and the plane is refitted to its members by least squares from integer
        moments, `refine` + 1 times.  A PLANE IS THE PLANE OF THE SHELL'S VOXEL CENTRES: a solid voxel with a free
        neighbour lies less than one voxel behind the zero crossing, so the plane sits up to one voxel behind the
        surface, and nothing corrects that.  ALL NUMERIC DEFAULTS ARE POLICY, NOT MEASUREMENTS: k 15, angle 20 degrees,
        separation = angle, bin 1 voxel, band 2 voxels, min_votes max(50, records / 200), suppression of 2 slots.
        Returns a dict: planes, a list of dicts ordered by count -- normal (3,), point (3,) and d in the world frame
        (normal . x = d, the normal pointing into free space; float64, d rounded once), normal_voxel and d_voxel in box
        voxels, count, bounds (lo, hi) in box voxels, thickness_m, axes (2, 3) world and extents_m (the roots of the
        in-plane eigenvalues times the voxel size), area_m2 = count * voxel^2 / max |normal_voxel_j| (AN ESTIMATE from a
        shell one voxel thick), kind and label; box; counters (surface voxels, with a normal, records kept, 0);
        min_votes; floor (an index into planes or None) and, with labels=True, records (the surface voxels, PLANE_VOXEL_DTYPE)
        and labels (bz, by, bx) i16, the `label` of the plane a voxel belongs to, -1 for none.
        The floor is, among planes whose normal is within floor_angle of up_hint (None: minus the background's y axis,
        ground_map's own default), the one whose centroid is lowest along up_hint; the others are named relative to its
        normal: level, ceiling, wall (within kind_angle) or slope.  Waits 3 + refine times.  Changes nothing of the
        session; refused on the sharded path.

        patches=True (off: nothing new runs and the dict is as above): a plane is infinite -- two tables
        of one height are one plane -- so every plane is split on the device into its connected surfaces, the components
        of its members under a Chebyshev reach of patch_reach voxels (1 or 2), and patches of fewer than patch_min_voxels
        members are dropped.  THE REACH OF 1 AND patch_min_voxels = max(25, min_votes // 4) ARE POLICY, NOT MEASUREMENTS.
        Every plane gains patches, a list ordered by count descending, ties to the lower id, of dicts: id (the smallest
        record index of the members), count, bounds (lo, hi) in box voxels, point, normal and d in the world frame from
        the patch's OWN least-squares fit, thickness_m, rect -- center (3,), axes (2, 3: the plane's), half_m (2,) and
        corners (4, 3) in the world frame, the rectangle IN THE PLANE that holds the members along the plane's axes --,
        area_m2 (the plane's formula on the patch's count), fill = count / the rectangle's voxel columns (near 1 for a
        full rectangle, lower for an L shape or one with holes: A RATIO OF TWO ESTIMATES), kind (the plane's) and the raw
        records under record and rect_voxel.  The result gains patch_counters (kept patches, all patches, members) and,
        with labels=True, patch_ids (bz, by, bx) i32, the id of the patch a voxel belongs to, -1 for none (a dropped
        patch keeps its id here).  Two more waits."""
        from ._lib import PLANE_VOXEL_DTYPE
        box = self._resolve_box("planes", box, size)
        prm = np.zeros((), PLANE_PARAMS_DTYPE)
        prm["K"], prm["refine"], prm["max_planes"], prm["peak_gap"] = int(k), int(refine), int(max_planes), 2
        prm["angle_deg"], prm["separation_deg"] = float(angle), 0.0 if separation is None else float(separation)
        prm["bin_vox"], prm["band_vox"] = 1.0 if bin is None else float(bin), 2.0 if band is None else float(band)
        prm["min_votes"] = 0 if min_votes is None else int(min_votes)
        lo_arg, size_arg, _, _ = _box_args(box, ())
        lo_out, size_out, R, t = _box_outs()
        counters, votes, count = np.zeros(4, np.uint32), C.c_uint32(0), C.c_int32(0)
        recs = np.zeros(64, PLANE_DTYPE)
        _check("emf_fusion_planes",
               load().emf_fusion_planes(self._h, lo_arg, size_arg, prm.ctypes.data, lo_out, size_out, R, t, counters.ctypes.data,
                                        C.byref(votes), recs.ctypes.data, 64, C.byref(count)))
        (blo, bsize), _ = _read_box_outs(lo_out, size_out, R, t)
        vs = float(np.float32(self.params.bg_voxel_size))
        bg_R, bg_t = self.background_pose()
        frame = _BoxFrame(bg_R, bg_t, self.params.bg_res, vs, blo)
        Rd = bg_R.astype(np.float64)
        up = -Rd[:, 1] if up_hint is None else np.asarray(up_hint, np.float64).reshape(3)

        def rotate(v):
            return np.array([(Rd[i, 0] * v[0] + Rd[i, 1] * v[1]) + Rd[i, 2] * v[2] for i in range(3)])

        out = []
        for r in recs[:count.value]:
            n_vox = r["n"].copy()
            n = rotate(n_vox)
            m = r["centroid"] if r["fitted"] else n_vox * r["d"]  # a point of the plane
            point = frame.world64(m)
            out.append(dict(normal=n, point=point, d=float((n[0] * point[0] + n[1] * point[1]) + n[2] * point[2]),
                            normal_voxel=n_vox, d_voxel=float(r["d"]), count=int(r["count"]),
                            bounds=(tuple(int(v) for v in r["lo"]), tuple(int(v) for v in r["hi"])),
                            thickness_m=float(r["thickness"] * vs), axes=np.stack([rotate(r["axes"][:3]), rotate(r["axes"][3:])]),
                            extents_m=tuple(float(np.sqrt(max(e, 0.0)) * vs) for e in r["eigenvalues"][:2]),
                            area_m2=float(r["count"] * (vs * vs) / np.abs(n_vox).max()), label=int(r["label"])))
        heights = [float((p["point"][0] * up[0] + p["point"][1] * up[1]) + p["point"][2] * up[2]) for p in out]
        floor, kinds = plane_kinds([p["normal"] for p in out], heights, up, floor_angle, kind_angle)
        for p, kind in zip(out, kinds):
            p["kind"] = kind
        res = dict(planes=out, box=(blo, bsize), counters=tuple(int(v) for v in counters), min_votes=int(votes.value), floor=floor)
        if labels:
            n = int(counters[2])
            rec, lab = np.zeros(max(n, 1), np.dtype(PLANE_VOXEL_DTYPE)), np.full(max(n, 1), -1, np.int16)
            _check("emf_fusion_copy_plane_labels", load().emf_fusion_copy_plane_labels(self._h, rec.ctypes.data, lab.ctypes.data, n))
            volume = np.full(bsize[0] * bsize[1] * bsize[2], -1, np.int16)
            volume[rec["index"][:n]] = lab[:n]
            res["labels"] = volume.reshape(bsize[2], bsize[1], bsize[0])
            res["records"] = rec[:n]
        if patches:
            self._plane_patches(res, recs[:count.value], frame, rotate, vs, int(patch_reach),
                                max(25, res["min_votes"] // 4) if patch_min_voxels is None else int(patch_min_voxels), labels)
        return res

    def _plane_patches(self, res, recs, frame, rotate, vs, reach, min_count, labels):
        """planes(patches=True): the patches of the planes just found, into their dicts."""
        from ._lib import PLANE_PATCH_DTYPE
        dtype = np.dtype(PLANE_PATCH_DTYPE)
        counters, count = np.zeros(3, np.uint32), C.c_int32(0)
        found = np.zeros(1024, dtype)
        _check("emf_fusion_plane_patches",
               load().emf_fusion_plane_patches(self._h, reach, min_count, counters.ctypes.data, found.ctypes.data, len(found),
                                               C.byref(count)))
        if count.value > len(found):  # rare: once more with room for all (every buffer is initialised by the call)
            found = np.zeros(count.value, dtype)
            _check("emf_fusion_plane_patches",
                   load().emf_fusion_plane_patches(self._h, reach, min_count, counters.ctypes.data, found.ctypes.data,
                                                   count.value, C.byref(count)))
        found = found[:count.value]
        res["patch_counters"] = tuple(int(v) for v in counters)
        for p, r in zip(res["planes"], recs):
            mine = found[found["plane"] == r["label"]]
            p["patches"] = []
            for q in mine[np.argsort(-mine["count"].astype(np.int64), kind="stable")]:
                rect = np.zeros((), PLANE_PATCH_RECT_DTYPE)  # the C entry: plane_patch_rect gives the same bits, more slowly
                plane, one = np.ascontiguousarray(r).reshape(1), np.ascontiguousarray(q).reshape(1)  # alive across the call
                _check("emf_fusion_plane_patch_rect",
                       load().emf_fusion_plane_patch_rect(plane.ctypes.data, one.ctypes.data, rect.ctypes.data))
                f = rect["fit"]
                n = rotate(f["n"])
                point = frame.world64(f["centroid"] if f["fitted"] else f["n"] * f["d"])
                p["patches"].append(dict(
                    id=int(q["id"]), count=int(q["count"]), bounds=(tuple(int(v) for v in q["lo"]), tuple(int(v) for v in q["hi"])),
                    point=point, normal=n, d=float((n[0] * point[0] + n[1] * point[1]) + n[2] * point[2]),
                    thickness_m=float(f["thickness"] * vs),
                    rect=dict(center=frame.world64(rect["center"]), axes=p["axes"].copy(), half_m=rect["half"] * vs,
                              corners=np.stack([frame.world64(rect["corners"][3 * c:3 * c + 3]) for c in range(4)])),
                    area_m2=float(q["count"] * (vs * vs) / np.abs(r["n"]).max()), fill=float(rect["fill"]), kind=p["kind"],
                    record=q.copy(), rect_voxel=rect))
        if labels:
            n = int(res["counters"][2])
            ids = np.full(max(n, 1), -1, np.int32)
            _check("emf_fusion_copy_plane_patch_ids", load().emf_fusion_copy_plane_patch_ids(self._h, ids.ctypes.data, n))
            bsize = res["box"][1]
            volume = np.full(bsize[0] * bsize[1] * bsize[2], -1, np.int32)
            volume[res["records"]["index"]] = ids[:n]
            res["patch_ids"] = volume.reshape(bsize[2], bsize[1], bsize[0])

    def object_support(self, ids=None, gap=0.05, margin=0.0, **plane_args):
        """Which surface each object stands on: planes(patches=True, **plane_args) and object_shapes(ids),
        then plane_support of every object's oriented box against every patch.  THE BOX BOUNDS THE OBSERVED SOLID BAND,
        NOT THE BODY (object_shapes): an object seen only from above has a box that ends where the observation does,
        and the test is about that box.  gap 0.05 m IS POLICY, NOT A MEASUREMENT.  Returns a dict: per object id
        dict(plane (an index into planes), patch (its id), s (the height of the box's lowest point above the patch's
        plane, metres)) or None -- also for an object without a valid box --, under "objects"; and the planes() result
        under "planes"."""
        found = self.planes(patches=True, **plane_args)
        shapes = self.object_shapes(ids)
        flat = [(k, q) for k, p in enumerate(found["planes"]) for q in p["patches"]]
        boxes = [dict(center=s["box_center_world"], axes=s["box_axes_world"], half=s["box_half"]) if s["valid"] else None
                 for s in shapes]
        objects = {}
        for s, hit in zip(shapes, plane_support([q for _, q in flat], boxes, gap, margin)):
            objects[s["id"]] = None if hit is None else dict(plane=flat[hit[0]][0], patch=flat[hit[0]][1]["id"], s=hit[1])
        return dict(objects=objects, planes=found)

    def ground_map(self, box=None, size=None, up=None, cell=None, bin=None, band=(-1.5, 0.5), reference=None,
                   robot_height=0.3, max_step=0.05, exclude=(), up_hint=None):
        """Where can a robot drive: a 2-D traversability map with a floor height per cell, projected on
        the device from the occupancy classes of a box of the background -- None, ((x, y, z) lo, (x, y, z) size) or
        "camera" with `size`, as for distance_field -- with every live object not in `exclude` stamped as occupied.
        up: the world direction that is up (None: minus the background's y axis in the world frame, the OpenCV camera
        convention at the first pose; "floor": the normal of the floor that planes(box, size, up_hint=up_hint) finds,
        ValueError where it finds none).  cell, bin (metres; None: two voxels): the side of a ground cell and the height
        of a bin; below two voxels a slot can miss every voxel centre of a tilted lattice, so smaller values are refused
        unless up is along a box axis.  band = (lo, hi) metres relative to `reference` (a world point; None: the camera
        position) along up: the heights that are looked at.  Per cell the column of height bins is OCCUPIED where any
        occupied voxel falls into the bin, FREE where a free one and no occupied one does; the floor is the lowest
        occupied bin with ceil(robot_height / bin) free bins above it, and a cell whose floor differs from a
        neighbour's by more than floor(max_step / bin) bins is an obstacle.  THE NUMERIC DEFAULTS ARE POLICY, NOT
        MEASUREMENTS: a band from 1.5 m below to 0.5 m above the camera, a robot 0.3 m high that climbs 5 cm.
        Returns a dict: classes (H, W) u8 (0 free: a floor the robot can stand on; 1 occupied: a step, or matter
        without a floor; 2 unknown); floor, top, clear, levels (H, W) i16 (-1 / -1 / 0 / 0 without); height_m (H, W)
        f32, the top face of the floor bin relative to the reference along up, NaN without a floor; frame = (G (3, 4)
        f32, W, H, B); ground_pose (12,) f64 (R row-major with the ground axes as columns, then t; ground metres ->
        world); cell, bin, band, up, reference, robot_bins, max_step_bins, box; cells, the raw records; cell_world(u, v): the world
        points (n, 3) f32 of the cells' centres at their floor height, float64 rounded once, NaN without a floor.  The
        classes stay on the device for ground_plan().  Changes nothing of the session; refused on the sharded path."""
        from ._lib import GROUND_CELL_DTYPE
        box = self._resolve_box("ground_map", box, size)
        if isinstance(up, str):
            if up != "floor":
                raise ValueError('ground_map: up is a world direction, None or "floor"')
            found = self.planes(box=box, up_hint=up_hint)
            if found["floor"] is None:
                raise ValueError('ground_map: up="floor" and planes() finds no floor')
            up = found["planes"][found["floor"]]["normal"]
        vs = float(np.float32(self.params.bg_voxel_size))
        bg_R, bg_t = self.background_pose()
        up = -bg_R[:, 1].astype(np.float64) if up is None else np.asarray(up, np.float64).reshape(3)
        cell = 2.0 * vs if cell is None else float(cell)
        bin = 2.0 * vs if bin is None else float(bin)
        ref = np.ascontiguousarray(self.pose(0)[1] if reference is None else reference, np.float64).reshape(3)
        up = np.ascontiguousarray(up)
        robot_bins, step_bins = ground_bins(robot_height, max_step, bin)
        lo, sz = box if box is not None else ((0, 0, 0), tuple(self.params.bg_res))
        G, W, H, B, _ = ground_frame(lo, sz, self.params.bg_res, vs, bg_R, bg_t, up, cell, bin, ref, band)
        if (cell < 2.0 * vs or bin < 2.0 * vs) and not ground_frame_aligned(G):
            raise ValueError("ground_map: cells and bins below two voxels need an up along a box axis")
        lo_arg, size_arg, ex, n_ex = _box_args(box, exclude)
        lo_out, size_out = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        frame, pose = np.zeros(15, np.int32), np.zeros(12, np.float64)
        cells, classes = np.zeros((H, W), np.dtype(GROUND_CELL_DTYPE)), np.zeros((H, W), np.uint8)
        _check("emf_fusion_ground_map",
               load().emf_fusion_ground_map(self._h, lo_arg, size_arg, ex, n_ex, up.ctypes.data, cell, bin, ref.ctypes.data,
                                            float(band[0]), float(band[1]), robot_bins, step_bins, lo_out, size_out,
                                            frame.ctypes.data, pose.ctypes.data, cells.ctypes.data, classes.ctypes.data, H * W))
        G_out = frame[:12].view(np.float32).reshape(3, 4).copy()
        assert (int(frame[12]), int(frame[13])) == (W, H), "the frame on the host and the session's disagree"
        gf = _GroundFrame(pose, cell, bin)
        floor = cells["floor"].copy()
        has = floor >= 0
        top_face = (floor.astype(np.float64) + 1.0) * np.float64(bin)
        height = np.where(has, np.float64(band[0]) + top_face, np.nan).astype(np.float32)

        def cell_world(u, v):
            u, v = np.asarray(u, np.int64).reshape(-1), np.asarray(v, np.int64).reshape(-1)
            inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
            f = np.where(inside, floor[np.clip(v, 0, H - 1), np.clip(u, 0, W - 1)], -1)
            ch = np.where(f >= 0, (f.astype(np.float64) + 1.0) * np.float64(bin), np.nan)
            return gf.world((u.astype(np.float64) + 0.5) * np.float64(cell), (v.astype(np.float64) + 0.5) * np.float64(cell),
                            ch).astype(np.float32)

        return dict(classes=classes, floor=floor, top=cells["top"].copy(), clear=cells["clear"].copy(),
                    levels=cells["levels"].copy(), height_m=height, frame=(G_out, W, H, int(frame[14])), ground_pose=pose,
                    cell=cell, bin=bin, band=(float(band[0]), float(band[1])), robot_bins=robot_bins, max_step_bins=step_bins,
                    box=(tuple(lo_out), tuple(size_out)), cells=cells, cell_world=cell_world, up=up, reference=ref)

    def ground_plan(self, goals="frontiers", start=None, robot_radius=0.0, through_unknown=False, min_cells=8,
                    **ground_map_args):
        """Path planning on the ground: ground_map(**ground_map_args), then the existing 2-D entries
        on its (1, H, W) classes where they lie on the device -- the capped distance transform from the occupied cells
        for robot_radius (metres, rounded up to whole cells), the frontiers (clusters of at least min_cells cells) for
        goals="frontiers", the cost-to-go from `start` (None: the cell under the camera, clipped to the map; else (n, 3)
        world points) with a start bubble of max(radius, 1) cells, and the paths.  goals: "frontiers" or (n, 3) world
        points, each taken to the cell it lies over.  Returns what plan() returns with cells (u, v, 0) for voxels --
        goals (voxel, reachable, cost, length_m = (faces + sqrt 2 edges) * cell, steps, path_vox, path_world: the
        cells' centres at their floor height, NaN where a path crosses a cell without a floor), start_voxels,
        start_radius_voxels, clearance_voxels, converged, rounds, n_finite, n_starts, and with "frontiers" clusters and
        frontiers -- plus ground, the dict of ground_map()."""
        from . import ops
        from ._lib import FRONTIER_KEPT
        from .devmem import DeviceView
        if isinstance(goals, str) and goals != "frontiers":
            raise ValueError('ground_plan: goals is "frontiers" or an (n, 3) array of world points')
        gm = self.ground_map(**ground_map_args)
        H, W = gm["classes"].shape
        gf = _GroundFrame(gm["ground_pose"], gm["cell"], gm["bin"])
        ptr = C.c_void_p()
        _check("emf_fusion_ground_classes_ptr", load().emf_fusion_ground_classes_ptr(self._h, C.byref(ptr), None))
        classes = DeviceView(ptr.value, (1, H, W), np.uint8)
        radius = _metres_to_voxels(robot_radius, gm["cell"])
        cap = min(radius, 4095)
        d2 = ops.distance_transform(classes, site_mask=2, cap=cap) if radius > 0 else None
        min_d2 = cap * cap
        found = None
        if isinstance(goals, str):
            _, records, counts = ops.frontiers(classes, d2=d2, min_d2=min_d2, min_voxels=int(min_cells))
            order = sorted(range(len(records)), key=lambda k: (-int(records[k]["count"]), int(records[k]["label"])))
            records = records[order] if len(records) else records
            goal_cells = records["rep"].astype(np.int32).reshape(-1, 3)
            clusters = []
            for r in records:
                rep, mean = r["rep"], r["sum"].astype(np.float64) / max(int(r["count"]), 1)
                clusters.append(dict(label=int(r["label"]), count=int(r["count"]), lo=tuple(int(v) for v in r["lo"]),
                                     hi=tuple(int(v) for v in r["hi"]), sum=tuple(int(v) for v in r["sum"]),
                                     rep=tuple(int(v) for v in rep), rep_world=gm["cell_world"](rep[0], rep[1])[0],
                                     centroid_cells=mean[:2]))
            found = dict(clusters=clusters, kept=counts[FRONTIER_KEPT], n_clusters=counts[1], n_voxels=counts[2], records=records)
        else:
            uv = gf.to_cells(goals)
            goal_cells = np.concatenate([uv, np.zeros((len(uv), 1), np.int32)], axis=1)
        if start is None:
            uv = np.clip(gf.to_cells(self.pose(0)[1]).astype(np.int64), 0, np.array([W - 1, H - 1])).astype(np.int32)
        else:
            uv = gf.to_cells(start)
        start_cells = np.concatenate([uv, np.zeros((len(uv), 1), np.int32)], axis=1)
        seed_radius = max(radius, 1)
        cost = ops.plan_cost(classes, start_cells, d2=d2, min_d2=min_d2, traverse_mask=1 | (4 if through_unknown else 0),
                             seed_radius=seed_radius)
        n_goals = len(goal_cells)
        if n_goals:
            paths, lengths, goal_cost = ops.plan_paths(cost, goal_cells)
        else:
            paths, lengths, goal_cost = np.zeros((0, 0), np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32)
        counters = cost.counters.numpy()
        records = []
        for g in range(n_goals):
            k = max(int(lengths[g]), 0)
            lin = paths[g, :k].astype(np.int64)
            vox = np.stack([lin % W, lin // W, np.zeros_like(lin)], axis=1).astype(np.int32)
            hops = np.abs(np.diff(vox[:, :2].astype(np.int64), axis=0)).sum(axis=1)
            faces, edges = int((hops == 1).sum()), int((hops == 2).sum())
            r = dict(found["clusters"][g]) if found is not None else {}
            r.update(voxel=tuple(int(v) for v in goal_cells[g]), reachable=k > 0, cost=int(goal_cost[g]),
                     length_m=(faces + np.sqrt(2.0) * edges) * np.float64(gm["cell"]), steps=(faces, edges, 0), path_vox=vox,
                     path_world=gm["cell_world"](vox[:, 0], vox[:, 1]))
            records.append(r)
        if found is not None:  # reachable first, cheapest first, as plan() orders them
            records = sorted(records, key=lambda r: (not r["reachable"], r["cost"] if r["reachable"] else 0))
        out = dict(goals=records, start_voxels=start_cells, start_radius_voxels=seed_radius, clearance_voxels=radius,
                   converged=bool(counters[0]), rounds=int(counters[1]), n_finite=int(counters[2]), n_starts=int(counters[3]),
                   ground=gm)
        if found is not None:
            out.update(clusters=records, frontiers=found)
        return out

    def last_motion_masks(self):
        """The proposals of the last processed frame: ((H, W) i32 image of proposal ranks, -1 where none is, list of
        dicts {label, area, x0, y0, x1, y1} by rank).  Empty / all -1 if the frame proposed nothing."""
        from ._lib import MOTION_MAX_MASKS
        labels = np.empty((self.params.height, self.params.width), np.int32)
        info, n = np.zeros((MOTION_MAX_MASKS, 6), np.int32), C.c_int32(0)
        _check("emf_fusion_last_motion_masks",
               load().emf_fusion_last_motion_masks(self._h, labels.ctypes.data, info.ctypes.data, MOTION_MAX_MASKS, C.byref(n)))
        keys = ("label", "area", "x0", "y0", "x1", "y1")
        return labels, [dict(zip(keys, (int(v) for v in row))) for row in info[:n.value]]

    def set_tracking(self, camera=True, objects=True):
        """From the next frame on, track the camera / object poses instead of taking them as inputs."""
        _check("emf_fusion_set_tracking", load().emf_fusion_set_tracking(self._h, int(camera), int(objects)))

    def create_object_from_mask(self, mask_view: EmfImage) -> int:
        """EMFusion::initNewObjVolume on the current frame's points; -1 if no object is created."""
        i = C.c_int32(-1)
        _check("emf_fusion_create_object_from_mask",
               load().emf_fusion_create_object_from_mask(self._h, C.byref(mask_view), C.byref(i)))
        return i.value

    def queue_new_object_masks(self, mask_views):
        """Masks for in-frame object creation by the next process_frame (initOrMatchObjs)."""
        arr = (EmfImage * max(len(mask_views), 1))(*mask_views)
        _check("emf_fusion_queue_new_object_masks",
               load().emf_fusion_queue_new_object_masks(self._h, len(mask_views), arr))

    def queue_instance_masks(self, mask_views):
        """The instance masks of a Mask R-CNN frame for the next process_frame (initOrMatchObjs);
        the masks are modified in place by the carving step."""
        arr = (EmfImage * max(len(mask_views), 1))(*mask_views)
        _check("emf_fusion_queue_instance_masks",
               load().emf_fusion_queue_instance_masks(self._h, len(mask_views), arr))

    def last_mask_assignment(self):
        ids, n = (C.c_int32 * 64)(), C.c_int32(0)
        _check("emf_fusion_last_mask_assignment",
               load().emf_fusion_last_mask_assignment(self._h, ids, 64, C.byref(n)))
        return [ids[i] for i in range(min(n.value, 64))]

    def last_created(self):
        ids, n = (C.c_int32 * 64)(), C.c_int32(0)
        _check("emf_fusion_last_created", load().emf_fusion_last_created(self._h, ids, 64, C.byref(n)))
        return [ids[i] for i in range(min(n.value, 64))]

    def match_mask(self, mask_view: EmfImage):
        """EMFusion::matchSegmentation: (object id or -1, best IoU)."""
        i, iou = C.c_int32(-1), C.c_float(0.0)
        _check("emf_fusion_match_mask",
               load().emf_fusion_match_mask(self._h, C.byref(mask_view), C.byref(i), C.byref(iou)))
        return i.value, iou.value

    def update_object(self, obj_id: int, mask_view: EmfImage):
        """EMFusion::updateObj + ObjTSDF::resize; returns the centre shift (zeros: unchanged)."""
        off = (C.c_float * 3)()
        _check("emf_fusion_update_object",
               load().emf_fusion_update_object(self._h, int(obj_id), C.byref(mask_view), off))
        return np.array(list(off), np.float32)

    def queue_instance_scores(self, scores):
        """Class scores (n, num_classes) that go with the masks of queue_instance_masks."""
        s = np.ascontiguousarray(scores, np.float64)
        s = s.reshape(len(s), -1) if s.size else np.zeros((0, 81))
        _check("emf_fusion_queue_instance_scores",
               load().emf_fusion_queue_instance_scores(self._h, s.shape[0], s.shape[1], s.ctypes.data))

    def object_class(self, obj_id: int) -> int:
        c = C.c_int32()
        _check("emf_fusion_object_class", load().emf_fusion_object_class(self._h, int(obj_id), C.byref(c)))
        return c.value

    def object_info(self, obj_id: int) -> Dict[str, float]:
        """resolution, voxel size, truncation distance and existence probability of an object volume as it is now."""
        res = (C.c_int32 * 3)()
        vox, trunc, ex = C.c_float(), C.c_float(), C.c_float()
        _check("emf_fusion_object_info",
               load().emf_fusion_object_info(self._h, int(obj_id), res, C.byref(vox), C.byref(trunc), C.byref(ex)))
        return dict(res=tuple(res), voxel_size=vox.value, truncdist=trunc.value, existence=ex.value)

    def set_ignore_person(self, on=True):
        """Params.ignore_person: objects classified as person stay out of renderings and mesh files."""
        _check("emf_fusion_set_ignore_person", load().emf_fusion_set_ignore_person(self._h, int(on)))

    def set_depth_broadcast(self, root: int = 0):
        """Multi-GPU: every frame's depth image is broadcast from rank `root` first (-1: off)."""
        _check("emf_fusion_set_depth_broadcast", load().emf_fusion_set_depth_broadcast(self._h, int(root)))

    def render(self):
        """EMFusion::render: (image (H, W, 3) u8 RGB, colour map (256, 3) u8)."""
        rgb = np.empty((self.params.height, self.params.width, 3), np.uint8)
        cmap = np.empty((256, 3), np.uint8)
        _check("emf_fusion_render", load().emf_fusion_render(self._h, rgb.ctypes.data, cmap.ctypes.data))
        return rgb, cmap

    def _view_args(self, R, t, K, size):
        K = np.array(self.params.K, np.float32) if K is None else K
        w, h = (self.params.width, self.params.height) if size is None else (int(size[0]), int(size[1]))
        return _farr(R, 9), _farr(t, 3), _farr(K, 9), w, h

    def render_view(self, R, t, K=None, size=None, shading="label"):
        """EMFusion::renderView: the map seen from a free viewpoint -- viewer -> world (R, t) (OpenCV camera, see
        look_at), intrinsics K (default: the frame's), size (width, height) (default: the frame's).  shading: "label"
        (every model in its label colour) or "color" (the fused colour of the voxel under each pixel, label colour
        where nobody coloured it; needs enable_color()).  Returns (rgb (H, W, 3) u8, raylengths (H, W) f32,
        segmentation (H, W) u8)."""
        Rc, tc, Kc, w, h = self._view_args(R, t, K, size)
        rgb = np.empty((h, w, 3), np.uint8)
        ray = np.empty((h, w), np.float32)
        seg = np.empty((h, w), np.uint8)
        if shading == "label":
            _check("emf_fusion_render_view",
                   load().emf_fusion_render_view(self._h, Rc, tc, Kc, w, h, rgb.ctypes.data, ray.ctypes.data,
                                                 seg.ctypes.data))
        else:
            _check("emf_fusion_render_view_shaded",
                   load().emf_fusion_render_view_shaded(self._h, Rc, tc, Kc, w, h, SHADING[shading], rgb.ctypes.data,
                                                        ray.ctypes.data, seg.ctypes.data))
        return rgb, ray, seg

    def set_3d_view_shading(self, shading="label"):
        """The shading ("label" / "color", see render_view) of the view of set_3d_view."""
        _check("emf_fusion_set_3d_view_shading", load().emf_fusion_set_3d_view_shading(self._h, SHADING[shading]))

    def set_3d_view(self, R=None, t=None, K=None, size=None):
        """EMFusion::set3dView (the reference's --3d-vis): render() also renders this view, and with setup_output
        write_results writes mesh_vis_out/%04d.png.  All None: the reference window's default (default_3d_view)."""
        if R is None and t is None and K is None and size is None:
            R, t, K, size = default_3d_view(self.params)
        Rc, tc, Kc, w, h = self._view_args(R, t, K, size)
        _check("emf_fusion_set_3d_view", load().emf_fusion_set_3d_view(self._h, Rc, tc, Kc, w, h))

    def clear_3d_view(self):
        _check("emf_fusion_clear_3d_view", load().emf_fusion_clear_3d_view(self._h))

    def mesh(self, obj_id: int = 0, colors=False):
        """TSDF::getMesh / ObjTSDF::getMesh: (vertices (n, 3), normals (n, 3), triangles (m, 4)); colors=True: a fourth
        array, the vertex colours (n, 3) u8 of the same extraction (needs enable_color())."""
        nv, nt = C.c_uint32(), C.c_uint32()
        _check("emf_fusion_extract_mesh",
               load().emf_fusion_extract_mesh(self._h, int(obj_id), C.byref(nv), C.byref(nt)))
        v = np.empty((nv.value, 3), np.float32)
        n = np.empty((nv.value, 3), np.float32)
        t = np.empty((nt.value, 4), np.int32)
        _check("emf_fusion_copy_mesh",
               load().emf_fusion_copy_mesh(self._h, v.ctypes.data, n.ctypes.data, t.ctypes.data))
        if colors:
            c = np.empty((nv.value, 3), np.uint8)
            _check("emf_fusion_copy_mesh_colors", load().emf_fusion_copy_mesh_colors(self._h, c.ctypes.data))
            return v, n, t, c
        return v, n, t

    def mesh_colors(self, obj_id: int = 0):
        """Vertex colours (n, 3) u8 RGB of model obj_id's mesh, in mesh(obj_id)'s vertex order (needs enable_color())."""
        nv, nt = C.c_uint32(), C.c_uint32()
        _check("emf_fusion_extract_mesh",
               load().emf_fusion_extract_mesh(self._h, int(obj_id), C.byref(nv), C.byref(nt)))
        c = np.empty((nv.value, 3), np.uint8)
        _check("emf_fusion_copy_mesh_colors", load().emf_fusion_copy_mesh_colors(self._h, c.ctypes.data))
        return c

    def meshes(self, ids=None, colors=False):
        """EMFusion::extractMeshes: {id: (vertices (n, 3), normals (n, 3), triangles (m, 4))} of the listed models
        (0 = background; None: the background and every live object) in one pass over the model table -- the same
        arrays as mesh(id) for each.  colors=True: 4-tuples, with the vertex colours (n, 3) u8 last (enable_color())."""
        ids = [0] + self.object_ids() if ids is None else [int(i) for i in ids]
        if not ids:
            return {}
        n = len(ids)
        id_arr = (C.c_int32 * n)(*ids)
        counts = np.zeros((n, 2), np.uint32)
        _check("emf_fusion_extract_meshes",
               load().emf_fusion_extract_meshes(self._h, id_arr, n,
                                                counts.ctypes.data_as(C.POINTER(C.c_uint32))))
        nv, nt = int(counts[:, 0].sum()), int(counts[:, 1].sum())
        v = np.empty((nv, 3), np.float32)
        nrm = np.empty((nv, 3), np.float32)
        t = np.empty((nt, 4), np.int32)
        _check("emf_fusion_copy_meshes",
               load().emf_fusion_copy_meshes(self._h, v.ctypes.data, nrm.ctypes.data, t.ctypes.data))
        c = None
        if colors:
            c = np.empty((nv, 3), np.uint8)
            _check("emf_fusion_copy_meshes_colors", load().emf_fusion_copy_meshes_colors(self._h, c.ctypes.data))
        out, v0, t0 = {}, 0, 0
        for k, i in enumerate(ids):
            cv, ct = int(counts[k, 0]), int(counts[k, 1])
            out[i] = (v[v0:v0 + cv], nrm[v0:v0 + cv], t[t0:t0 + ct]) + ((c[v0:v0 + cv],) if colors else ())
            v0, t0 = v0 + cv, t0 + ct
        return out

    def enable_pose_log(self, on=True):
        _check("emf_fusion_enable_pose_log", load().emf_fusion_enable_pose_log(self._h, int(on)))

    def setup_output(self, exp_frame_meshes=False, exp_vols=False, exp_world_mesh=False, exp_distance_field=False,
                     distance_cap=0.0, distance_unknown_is_obstacle=False, exp_frontiers=False, frontier_min_voxels=8,
                     frontier_clearance=0.0, exp_plan=False, plan_clearance=0.0, plan_through_unknown=False,
                     exp_distance_nearest=False, exp_plan_shortcut=0, exp_object_shapes=False, exp_ground_map=False,
                     ground_up=None, ground_cell=None, ground_bin=None, ground_band=(-1.5, 0.5), ground_robot_height=0.3,
                     ground_max_step=0.05, exp_planes=False, planes_angle=20.0, planes_min_votes=None,
                     exp_plane_patches=False, plane_patch_reach=1, plane_patch_min=None, exp_object_contacts=False,
                     contact_touch=None, exp_absorbed=False, exp_lifted=False, exp_merged=False):
        """Reference EMFusion::setupOutput: log on; exp_vols keeps deleted objects' volumes too; exp_frame_meshes meshes
        the background and every shown object at the end of every frame for write_results' frame_meshes/ (refused on
        the sharded path); exp_world_mesh: write_results also writes world.ply, write_mesh of world_mesh();
        exp_distance_field: write_results also writes distance.bin (f32 metres to the nearest obstacle of the whole
        background, +inf beyond distance_cap metres or without an obstacle) and occupancy.bin (u8 classes);
        exp_frontiers: write_results also writes frontiers.txt, one line per frontier cluster of the whole background
        of at least frontier_min_voxels voxels, largest first (include/emf_fusion.h emf_fusion_set_frontier_output);
        exp_plan: write_results also writes plan.txt, the plan from the voxel under the last camera position to every
        frontier cluster of at least frontier_min_voxels voxels at plan_clearance metres
        (include/emf_fusion.h emf_fusion_set_plan_output);
        exp_distance_nearest (needs exp_distance_field): write_results also writes nearest.bin, i32 in the container of
        distance.bin: the linear index of the nearest obstacle voxel of the background, -1 where there is none;
        exp_plan_shortcut=W > 0 (needs exp_plan): plan.txt carries one extra "waypoints n i_0 .. i_(n-1)" line per
        reachable goal, plan(shortcut=W) of its path (include/emf_fusion.h emf_fusion_set_plan_shortcut_output);
        exp_object_shapes: write_results also writes shapes.txt, one line per live object in id order: the integers of
        object_shapes(), then the world-frame box in %.9g (include/emf_fusion.h emf_fusion_set_shape_output);
        exp_ground_map: write_results also writes ground.bin (the W * H class bytes, then the W * H records of four
        i16) and ground.txt (map size, bins, G and the ground pose) of ground_map() over the whole background with
        ground_up (None: minus the background's y axis), ground_cell, ground_bin (None: two voxels), ground_band,
        ground_robot_height and ground_max_step; the reference is the camera position
        (include/emf_fusion.h emf_fusion_set_ground_output); ground_up="floor": up is the normal of the floor that
        planes() finds in the whole background, and write_results fails where it finds none;
        exp_planes: write_results also writes planes.txt, one line per plane of planes(angle=planes_angle,
        min_votes=planes_min_votes) over the whole background ordered by count: kind count, then in %.9g the world
        normal, d, the point, the thickness in metres, then the bounds in voxels (include/emf_fusion.h
        emf_fusion_set_planes_output);
        exp_plane_patches (needs exp_planes): planes.txt gains, after each plane's line, one line per patch of
        planes(patches=True, patch_reach=plane_patch_reach, patch_min_voxels=plane_patch_min) of that plane: "patch" id
        count, then in %.9g the world point, the four corners and fill; and, with exp_object_shapes as well, after all
        planes one "support <object id> <plane> <patch id> <s>" line per object that rests on a patch
        (include/emf_fusion.h emf_fusion_set_plane_patches_output);
        exp_object_contacts: write_results also writes contacts.txt, after a comment line one line per ordered pair of
        object_contacts(touch=contact_touch) over the live objects in id order and the background with sampled > 0: the
        ids, the eight counts, then in %.9g min_s and the world contact point and normal of that record
        (include/emf_fusion.h emf_fusion_set_contacts_output);
        exp_absorbed: write_results also writes absorbed.txt, after a comment line one line per event of absorbed():
        absorbed_line() of it (include/emf_fusion.h emf_fusion_set_absorbed_output).
        exp_lifted: write_results also writes lifted.txt, after a comment line one line per event of lifted():
        lifted_line() of it (include/emf_fusion.h emf_fusion_set_lifted_output).
        exp_merged: write_results also writes merged.txt, after a comment line one line per event of merged():
        merged_line() of it (include/emf_fusion.h emf_fusion_set_merged_output)."""
        if contact_touch is not None and not exp_object_contacts:
            raise ValueError("setup_output: contact_touch is the threshold of contacts.txt and needs exp_object_contacts")
        if exp_plan_shortcut and not exp_plan:
            raise ValueError("setup_output: exp_plan_shortcut adds lines to plan.txt and needs exp_plan")
        if exp_distance_nearest and not exp_distance_field:
            raise ValueError("setup_output: exp_distance_nearest writes nearest.bin beside distance.bin and needs exp_distance_field")
        _check("emf_fusion_setup_output",
               load().emf_fusion_setup_output(self._h, int(exp_frame_meshes), int(exp_vols)))
        _check("emf_fusion_set_world_mesh_output",
               load().emf_fusion_set_world_mesh_output(self._h, int(bool(exp_world_mesh))))
        _check("emf_fusion_set_distance_output",
               load().emf_fusion_set_distance_output(self._h, int(bool(exp_distance_field)), float(distance_cap),
                                                     int(bool(distance_unknown_is_obstacle))))
        _check("emf_fusion_set_distance_nearest_output",
               load().emf_fusion_set_distance_nearest_output(self._h, int(bool(exp_distance_nearest))))
        _check("emf_fusion_set_frontier_output",
               load().emf_fusion_set_frontier_output(self._h, int(bool(exp_frontiers)), int(frontier_min_voxels),
                                                     float(frontier_clearance)))
        _check("emf_fusion_set_plan_output",
               load().emf_fusion_set_plan_output(self._h, int(bool(exp_plan)), float(plan_clearance),
                                                 int(bool(plan_through_unknown))))
        if exp_plan_shortcut:  # off: no new call
            _check("emf_fusion_set_plan_shortcut_output",
                   load().emf_fusion_set_plan_shortcut_output(self._h, int(exp_plan_shortcut)))
        if exp_object_shapes:  # off: no new call
            _check("emf_fusion_set_shape_output", load().emf_fusion_set_shape_output(self._h, 1))
        up_floor = isinstance(ground_up, str)
        if up_floor and ground_up != "floor":
            raise ValueError('setup_output: ground_up is a world direction, None or "floor"')
        if exp_planes or up_floor:  # off: no new call
            _check("emf_fusion_set_planes_output",
                   load().emf_fusion_set_planes_output(self._h, int(bool(exp_planes)), float(planes_angle),
                                                       0 if planes_min_votes is None else int(planes_min_votes), int(up_floor)))
        if exp_plane_patches:  # off: no new call
            if not exp_planes:
                raise ValueError("setup_output: exp_plane_patches adds lines to planes.txt and needs exp_planes")
            _check("emf_fusion_set_plane_patches_output",
                   load().emf_fusion_set_plane_patches_output(self._h, 1, int(plane_patch_reach),
                                                              0 if plane_patch_min is None else int(plane_patch_min)))
        if exp_object_contacts:  # off: no new call
            _check("emf_fusion_set_contacts_output",
                   load().emf_fusion_set_contacts_output(self._h, 1, -1.0 if contact_touch is None else float(contact_touch)))
        if exp_absorbed:  # off: no new call
            _check("emf_fusion_set_absorbed_output", load().emf_fusion_set_absorbed_output(self._h, 1))
        if exp_lifted:  # off: no new call
            _check("emf_fusion_set_lifted_output", load().emf_fusion_set_lifted_output(self._h, 1))
        if exp_merged:  # off: no new call
            _check("emf_fusion_set_merged_output", load().emf_fusion_set_merged_output(self._h, 1))
        if exp_ground_map:  # off: no new call
            up = None if ground_up is None or up_floor else np.ascontiguousarray(ground_up, np.float64).reshape(3)
            _check("emf_fusion_set_ground_output",
                   load().emf_fusion_set_ground_output(self._h, 1, None if up is None else up.ctypes.data,
                                                       0.0 if ground_cell is None else float(ground_cell),
                                                       0.0 if ground_bin is None else float(ground_bin), float(ground_band[0]),
                                                       float(ground_band[1]), float(ground_robot_height), float(ground_max_step)))

    def write_results(self, directory: str, volumes: bool = True):
        """poses-*.txt, mesh_bg.ply, mesh_<id>.ply always; tsdfs/*.bin with `volumes` (reference formats)."""
        _check("emf_fusion_write_results",
               load().emf_fusion_write_results(self._h, os.fspath(directory).encode(), int(volumes)))

    def set_cleanup(self, on=True):
        """Run the reference's cleanUpObjs at the end of every frame."""
        _check("emf_fusion_set_cleanup", load().emf_fusion_set_cleanup(self._h, int(on)))

    def last_deleted(self):
        ids, n = (C.c_int32 * 64)(), C.c_int32(0)
        _check("emf_fusion_last_deleted", load().emf_fusion_last_deleted(self._h, ids, 64, C.byref(n)))
        return [ids[i] for i in range(min(n.value, 64))]

    def set_preprocess(self, on=True):
        """Filter incoming depth maps as the reference's preprocessDepth does (bilateral + patches)."""
        _check("emf_fusion_set_preprocess", load().emf_fusion_set_preprocess(self._h, int(on)))

    def pose(self, obj_id: int = 0):
        """(R 3x3, t 3): camera -> world for id 0, object volume -> world otherwise."""
        R, t = (C.c_float * 9)(), (C.c_float * 3)()
        _check("emf_fusion_get_pose", load().emf_fusion_get_pose(self._h, int(obj_id), R, t))
        return np.array(R, np.float32).reshape(3, 3), np.array(t, np.float32)

    def track_result(self, obj_id: int = 0) -> Dict[str, float]:
        it, acc, conv, err = C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
        _check("emf_fusion_track_result",
               load().emf_fusion_track_result(self._h, int(obj_id), C.byref(it), C.byref(acc),
                                              C.byref(conv), C.byref(err)))
        return dict(iterations=it.value, accepted=acc.value, converged=bool(conv.value), error=err.value)

    def stage_estep(self):
        _check("emf_fusion_stage_estep", load().emf_fusion_stage_estep(self._h))

    def stage_raycast(self):
        _check("emf_fusion_stage_raycast", load().emf_fusion_stage_raycast(self._h))

    def stage_integrate(self):
        _check("emf_fusion_stage_integrate", load().emf_fusion_stage_integrate(self._h))

    def synchronize(self):
        _check("emf_fusion_synchronize", load().emf_fusion_synchronize(self._h))

    def enable_timings(self, on=True):
        _check("emf_fusion_enable_timings", load().emf_fusion_enable_timings(self._h, int(on)))

    def last_timings(self) -> Dict[str, float]:
        t = FrameTimings()
        _check("emf_fusion_last_timings", load().emf_fusion_last_timings(self._h, C.byref(t)))
        return t.as_dict()

    def enable_raycast_stats(self, on=True):
        _check("emf_fusion_enable_raycast_stats",
               load().emf_fusion_enable_raycast_stats(self._h, int(on)))

    def raycast_stats(self):
        c = (C.c_uint64 * 4)()
        _check("emf_fusion_raycast_stats", load().emf_fusion_raycast_stats(self._h, c))
        return tuple(int(v) for v in c)

    def kernel_timers_enable(self, max_launches: int):
        _check("emf_fusion_kernel_timers_enable",
               load().emf_fusion_kernel_timers_enable(self._h, int(max_launches)))

    def kernel_timers_select(self, kinds):
        """Bracket only these kernel kinds (names from KERNEL_KINDS) with event pairs."""
        mask = 0
        for k in kinds:
            mask |= 1 << KERNEL_KINDS.index(k)
        _check("emf_fusion_kernel_timers_select", load().emf_fusion_kernel_timers_select(self._h, mask))

    def kernel_timers_stride(self, every: int):
        """Bracket only every `every`-th launch of a kind with an event pair (1 = all)."""
        _check("emf_fusion_kernel_timers_stride", load().emf_fusion_kernel_timers_stride(self._h, int(every)))

    def kernel_timers_clear(self):
        _check("emf_fusion_kernel_timers_clear", load().emf_fusion_kernel_timers_clear(self._h))

    def kernel_timers_collect(self) -> Dict[str, Dict[str, float]]:
        """Synchronises, then returns {kind: {launches, total_ms, units}} (+ '_dropped')."""
        arr = (KernelSummary * len(KERNEL_KINDS))()
        dropped = C.c_uint64()
        _check("emf_fusion_kernel_timers_collect",
               load().emf_fusion_kernel_timers_collect(self._h, arr, C.byref(dropped)))
        out = {k: dict(launches=int(arr[i].launches), total_ms=float(arr[i].total_ms),
                       units=float(arr[i].units)) for i, k in enumerate(KERNEL_KINDS)}
        out["_dropped"] = int(dropped.value)
        return out

    def image_view(self, which: str, obj_id: int = 0) -> EmfImage:
        v = EmfImage()
        _check("emf_fusion_get_image",
               load().emf_fusion_get_image(self._h, IMG[which], obj_id, C.byref(v)))
        return v

    def image(self, which: str, obj_id: int = 0) -> np.ndarray:
        """Synchronise and copy an image of the last frame to the host."""
        self.synchronize()
        v = self.image_view(which, obj_id)
        dt, ch = _IMG_DTYPE[IMG[which]]
        out = np.empty((v.height, v.width, ch) if ch > 1 else (v.height, v.width), dt)
        assert v.pitch == v.width * ch * out.itemsize
        devmem.memcpy_d2h(out, v.data)
        return out

    def volume(self, which: str, obj_id: int = 0) -> np.ndarray:
        self.synchronize()
        ptr = C.c_void_p()
        res = (C.c_int32 * 3)()
        _check("emf_fusion_get_volume",
               load().emf_fusion_get_volume(self._h, VOL[which], obj_id, C.byref(ptr), res))
        if which == "color":
            out = np.empty((res[2], res[1], res[0], 4), np.uint16)
        elif which == "fgbg":
            out = np.empty((res[2], res[1], res[0], 2), np.float32)
        else:
            out = np.empty((res[2], res[1], res[0]), np.uint8 if which in ("fgmask", "bricks") else np.float32)
        devmem.memcpy_d2h(out, ptr.value)
        return out

    def save_checkpoint(self, path) -> dict:
        """emf_fusion_save_checkpoint: the session's primary state, volumes packed losslessly on the device, written to
        `path` (through path + ".tmp").  Returns raw_bytes / file_bytes, chunks per class and the milliseconds of the
        stages (classify, gather: device; copy, file, total: host).  The background-follow switch and its parameters
        are in the file only once the background has rolled (see set_background_follow); a session with the
        background store on writes version 3, which carries the store (see set_background_store)."""
        st = CheckpointStats()
        _check("emf_fusion_save_checkpoint", load().emf_fusion_save_checkpoint(self._h, os.fspath(path).encode(), C.byref(st)))
        return dict(raw_bytes=int(st.raw_bytes), file_bytes=int(st.file_bytes), records=int(st.records),
                    chunks=dict(zero=int(st.chunks[0]), uniform=int(st.chunks[1]), literal=int(st.chunks[2])),
                    ms=dict(classify=st.ms_classify, gather=st.ms_gather, copy=st.ms_copy, file=st.ms_file,
                            total=st.ms_total))

    def load_checkpoint(self, path):
        """emf_fusion_load_checkpoint: reset, then restore the session saved in `path`; FusionError (EMF_E_ARG) with
        the session untouched if the file does not fit this instance or is damaged."""
        _check("emf_fusion_load_checkpoint", load().emf_fusion_load_checkpoint(self._h, os.fspath(path).encode()))

    @classmethod
    def from_checkpoint(cls, path, comm: Optional["Communicator"] = None):
        """The instance built from the parameters a checkpoint was saved with, with the checkpoint loaded."""
        self = cls.__new__(cls)
        self.params = FusionParams()
        self._comm = comm
        self._h = C.c_void_p()
        _check("emf_fusion_create_from_checkpoint",
               load().emf_fusion_create_from_checkpoint(os.fspath(path).encode(), comm._h if comm else None,
                                                        C.byref(self.params), C.byref(self._h)))
        return self

    def background_overlap(self) -> bool:
        return load().emf_fusion_background_overlap(self._h) == 1

    def upload_host_time(self):
        """(seconds, frames): host time process_rgbd has spent handing depth maps to the device so far."""
        s, n = C.c_double(0), C.c_uint64(0)
        _check("emf_fusion_upload_host_time", load().emf_fusion_upload_host_time(self._h, C.byref(s), C.byref(n)))
        return float(s.value), int(n.value)

    def batched_chunks(self) -> int:
        """0: per-volume path; k >= 1: batched path with k launches per stage (one per <= 32 table slots)."""
        return int(load().emf_fusion_batched_chunks(self._h))

    def object_ids(self):
        """Live objects of the job in creation order."""
        ids = (C.c_int32 * 256)()
        n = C.c_int()
        _check("emf_fusion_object_ids", load().emf_fusion_object_ids(self._h, ids, 256, C.byref(n)))
        return [ids[i] for i in range(n.value)]

    def visible_objects(self):
        ids = (C.c_int32 * 256)()
        n = C.c_int()
        _check("emf_fusion_visible_objects",
               load().emf_fusion_visible_objects(self._h, ids, 256, C.byref(n)))
        return [ids[i] for i in range(n.value)]

    def frame_index(self) -> int:
        return load().emf_fusion_frame_index(self._h)

    def owns_object(self, obj_id: int) -> bool:
        return bool(load().emf_fusion_owns_object(self._h, obj_id))


def read_depth_png(path, scale=1.0 / 5000.0) -> np.ndarray:
    """core/Readers.cpp readPngGray through the C API: float32 (H, W) = raw * scale."""
    w, h = C.c_int32(), C.c_int32()
    _check("emf_io_read_depth_png", load().emf_io_read_depth_png(os.fspath(path).encode(), scale, None, 0, C.byref(w), C.byref(h)))
    out = np.empty((h.value, w.value), np.float32)
    _check("emf_io_read_depth_png", load().emf_io_read_depth_png(os.fspath(path).encode(), scale,
                                                               out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(w), C.byref(h)))
    return out


def read_color_png(path) -> np.ndarray:
    """core/Readers.cpp readPngColor through the C API: uint8 (H, W, 3) of an 8-bit RGB / RGBA PNG (alpha dropped)."""
    w, h = C.c_int32(), C.c_int32()
    _check("emf_io_read_color_png", load().emf_io_read_color_png(os.fspath(path).encode(), None, 0, C.byref(w), C.byref(h)))
    out = np.empty((h.value, w.value, 3), np.uint8)
    _check("emf_io_read_color_png", load().emf_io_read_color_png(os.fspath(path).encode(), out.ctypes.data, out.nbytes,
                                                               C.byref(w), C.byref(h)))
    return out


def load_config(path=None, calibration=None):
    """The reference's configuration file (config/*.cfg, apps/EM-Fusion.cpp:268-371) and / or a Co-Fusion
    calibration.txt applied to the reference defaults (core/Config.cpp): (FusionParams for Fusion(...), {key: value
    string or list of strings} of every configurable field)."""
    prm = FusionParams()
    buf = C.create_string_buffer(1 << 14)
    _check("emf_io_load_config",
           load().emf_io_load_config(os.fspath(path).encode() if path else None,
                                     os.fspath(calibration).encode() if calibration else None,
                                     C.byref(prm), buf, len(buf)))
    fields: Dict[str, object] = {}
    for line in buf.value.decode().splitlines():
        k, v = [t.strip() for t in line.split("=", 1)]
        if k.startswith("Params.MaskRCNNParams."):
            fields.setdefault(k, []).append(v)
        else:
            fields[k] = v
    return prm, fields


def read_exr(path, channel=None) -> np.ndarray:
    """core/Readers.cpp readExr through the C API: one channel of a scan-line OpenEXR file as float32 (H, W)."""
    w, h = C.c_int32(), C.c_int32()
    ch = channel.encode() if channel else None
    _check("emf_io_read_exr", load().emf_io_read_exr(os.fspath(path).encode(), ch, None, 0, C.byref(w), C.byref(h)))
    out = np.empty((h.value, w.value), np.float32)
    _check("emf_io_read_exr", load().emf_io_read_exr(os.fspath(path).encode(), ch, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                     out.size, C.byref(w), C.byref(h)))
    return out


def image_reader(base, colordir="colour", depthdir="depth"):
    """(number of frames, first index) of a Co-Fusion style dataset, as the C++ emf::ImageReader sees it."""
    n, first = C.c_int32(), C.c_int32()
    _check("emf_io_image_reader", load().emf_io_image_reader((os.fspath(base) + os.sep).encode(), colordir.encode(),
                                                            depthdir.encode(), C.byref(n), C.byref(first)))
    return n.value, first.value


def tum_associations(path):
    """[(depth file name, time stamp)] of a TUM associations.txt, as the C++ TUMRGBDReader parses it."""
    n, out = C.c_int32(), []
    _check("emf_io_tum_associations", load().emf_io_tum_associations(os.fspath(path).encode(), -1, None, 0, None, C.byref(n)))
    for i in range(n.value):
        name, stamp = C.create_string_buffer(512), C.c_double()
        _check("emf_io_tum_associations", load().emf_io_tum_associations(os.fspath(path).encode(), i, name, 512, C.byref(stamp), C.byref(n)))
        out.append((name.value.decode(), stamp.value))
    return out


def load_preproc_masks(path):
    """core/Readers.cpp loadPreprocessedMasks through the C API: (boxes (N, 4), masks (N, H, W) u8, scores (N, S))."""
    n, w, h, ns = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    f = load().emf_io_load_preproc_masks
    _check("emf_io_load_preproc_masks", f(os.fspath(path).encode(), C.byref(n), C.byref(w), C.byref(h), None, 0, None, 0, None, 0, C.byref(ns)))
    masks = np.zeros((n.value, h.value, w.value), np.uint8)
    boxes = np.zeros((n.value, 4), np.float64)
    scores = np.zeros((n.value, ns.value), np.float64)
    _check("emf_io_load_preproc_masks", f(os.fspath(path).encode(), C.byref(n), C.byref(w), C.byref(h), masks.ctypes.data, masks.nbytes,
                                          boxes.ctypes.data_as(C.POINTER(C.c_double)), boxes.size, scores.ctypes.data_as(C.POINTER(C.c_double)),
                                          scores.size, C.byref(ns)))
    return boxes, masks, scores


def trim_pool() -> int:
    """Really free the device buffers the host classes keep pooled (waits for the device); bytes freed."""
    n = C.c_uint64(0)
    _check("emf_fusion_trim_pool", load().emf_fusion_trim_pool(C.byref(n)))
    return int(n.value)


class EmfFollowParams(C.Structure):
    """Mirror of emf_follow_params_t (include/emf_fusion.h)."""

    _fields_ = [("step", C.c_int32 * 3), ("look_ahead", C.c_float), ("keep_retired", C.c_int32)]


def follow_shift(q, step=(64, 64, 64), voxel=0.01):
    """The follow policy (emf_fusion_follow_shift; no device): per axis trunc(q_i / (step_i * voxel)) * step_i for the
    followed point q in the background's frame, in single precision.  FusionError (EMF_E_ARG) for a step component that
    is not a positive multiple of the tile (32, 8, 8)."""
    out = (C.c_int32 * 3)()
    _check("emf_fusion_follow_shift",
           load().emf_fusion_follow_shift(_farr(q, 3), (C.c_int32 * 3)(*[int(v) for v in step]), float(voxel), out))
    return tuple(int(v) for v in out)


def checkpoint_info(path) -> dict:
    """emf_fusion_checkpoint_info: what a checkpoint file holds (no device needed); FusionError if it is not a
    complete checkpoint."""
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    _check("emf_fusion_checkpoint_info", load().emf_fusion_checkpoint_info(os.fspath(path).encode(), buf, cap))
    return json.loads(buf.value.decode())


def describe_switches() -> dict:
    """The run-time switches of the host classes as the loaded library parses them from the current environment:
    {NAME: {"kind", "type", "rule", "default", "read", "value", "path", "doc", "field"}} (csrc/core/Switches.hpp).
    Needs no GPU.  Raises FusionError (EMF_E_ARG) where a value is refused, as a Fusion constructed now would."""
    buf = C.create_string_buffer(1 << 14)
    _check("emf_fusion_describe_switches", load().emf_fusion_describe_switches(buf, len(buf)))
    return {row.pop("name"): row for row in json.loads(buf.value.decode())["switches"]}


def write_volume(filename, volume: np.ndarray, voxel_size: float):
    """Reference volume dump (EMFusion::writeVolume): volume is float32 (Nz, Ny, Nx)."""
    v = np.ascontiguousarray(volume, np.float32)
    nz, ny, nx = v.shape
    _check("emf_io_write_volume",
           load().emf_io_write_volume(os.fspath(filename).encode(), v.ctypes.data_as(C.POINTER(C.c_float)),
                                      (C.c_int32 * 3)(nx, ny, nz), float(voxel_size)))


def write_mesh(filename, vertices, normals, triangles, colors=None):
    """ASCII PLY of the reference (EMFusion::writeMesh); colors ((n, 3) u8): red / green / blue behind the normals."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 4)
    assert len(v) == len(n)
    if colors is not None:
        c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        assert len(c) == len(v)
        _check("emf_io_write_mesh_colors",
               load().emf_io_write_mesh_colors(os.fspath(filename).encode(), len(v), v.ctypes.data, n.ctypes.data,
                                               c.ctypes.data, len(t), t.ctypes.data))
        return
    _check("emf_io_write_mesh",
           load().emf_io_write_mesh(os.fspath(filename).encode(), len(v), v.ctypes.data, n.ctypes.data,
                                    len(t), t.ctypes.data))


def write_pose_file(filename, poses: Dict[int, tuple]):
    """TUM-style pose file from {frame: (R 3x3, t 3)} (EMFusion::writePoseFile)."""
    frames = sorted(poses)
    R = np.ascontiguousarray([np.asarray(poses[f][0], np.float32).reshape(9) for f in frames], np.float32)
    t = np.ascontiguousarray([np.asarray(poses[f][1], np.float32).reshape(3) for f in frames], np.float32)
    _check("emf_io_write_pose_file",
           load().emf_io_write_pose_file(os.fspath(filename).encode(), len(frames),
                                         (C.c_int32 * max(len(frames), 1))(*frames),
                                         R.ctypes.data_as(C.POINTER(C.c_float)),
                                         t.ctypes.data_as(C.POINTER(C.c_float))))
