"""CPU side of the per-voxel colour feature: the numpy restatement the colour kernel is pinned to is itself pinned
to the oracle's updateTSDF, and the new entries are declared, exported and typed."""
import ctypes as C
import re

import numpy as np

from tests import color_scene as cs


def test_restatement_matches_the_oracle_bit_for_bit(oracle):
    """tests/color_reference.py restates updateTSDF and the colour rule; its tsdf and weight volumes equal
    orc_updateTSDF's bit for bit over 6 frames fed back into each other (background 64^3 at 0.04 m + one 32^3
    object, 160 x 120, association maps with zeros, ones and fractions) -- which ties the pixel, the depth gate and
    the signed distance the colour rule reuses to the oracle, and through it to the reference's kernel."""
    ids_seen = set()
    for f, (_, _, ids, _) in enumerate(cs.frames()):
        bg, obj = cs.assoc_maps(ids, f)
        for a in (bg, obj):
            ids_seen |= {"zero"} if (a == 0).any() else set()
            ids_seen |= {"one"} if (a == 1).any() else set()
            ids_seen |= {"frac"} if ((a > 0) & (a < 1)).any() else set()
    assert ids_seen == {"zero", "one", "frac"}
    state = cs.run_reference([cs.BG, cs.OBJ], oracle=oracle)
    for name, s in zip(("background", "object"), state):
        assert (s["ow"] > 0).sum() > 1000, name
        assert np.array_equal(s["t"].view(np.uint32), s["ot"].view(np.uint32)), f"{name}: tsdf differs from the oracle"
        assert np.array_equal(s["w"].view(np.uint32), s["ow"].view(np.uint32)), f"{name}: weights differ from the oracle"
    # the colour rule is exercised by the same run: the non-vacuity bounds the GPU tests rely on
    assert (state[0]["c"][..., 3] > 0).sum() >= 1000
    assert (state[1]["c"][..., 3] > 0).sum() >= 100


def test_restatement_colour_rule_on_a_single_voxel():
    """One voxel, by hand: the first colour lands unblended (the colour weight starts at 0 although the TSDF weight
    may not), the second is the weighted mean in 8.8 fixed point, and the weight saturates at maxWeight."""
    from tests import color_reference as ref
    F = np.float32
    K = np.array([[100, 0, 1.5], [0, 100, 1.5], [0, 0, 1]], F)
    depth = np.full((4, 4), 1.0, F)
    tsdf, wts = np.zeros((2, 2, 2), F), np.zeros((2, 2, 2), F)
    col = np.zeros((2, 2, 2, 4), np.uint16)
    rgb = np.zeros((4, 4, 3), np.uint8)
    rgb[...] = (200, 100, 7)
    R, t = np.eye(3, dtype=F), np.array([0, 0, 1.0], F)
    assert ref.update(depth, np.full((4, 4), 0.5, F), tsdf, wts, R, t, K, 0.01, 0.05, 1.0, rgb, col) == 8
    assert (col[..., :3] == np.array([200, 100, 7]) * 256).all() and (col[..., 3] == 128).all()
    rgb[...] = (100, 100, 8)
    ref.update(depth, np.full((4, 4), 1.0, F), tsdf, wts, R, t, K, 0.01, 0.05, 1.0, rgb, col)
    want = np.rint((F(0.5) * F(200) + F(100)) / F(1.5) * F(256))
    assert (col[..., 0] == want).all() and (col[..., 1] == 100 * 256).all()
    assert (col[..., 3] == 256).all()  # min(0.5 + 1, maxWeight = 1)
    before = col.copy()
    ref.update(depth, np.zeros((4, 4), F), tsdf, wts, R, t, K, 0.01, 0.05, 1.0, rgb, col)  # assoc 0: untouched
    assert np.array_equal(col, before)


NEW_HIP = ["emf_hip_integrateColorBatched", "emf_hip_copyColorValues", "emf_hip_meshColors", "emf_hip_meshColorsBatched"]
NEW_FUSION = ["emf_fusion_set_color", "emf_fusion_set_color_image", "emf_fusion_process_rgbd_color",
              "emf_fusion_colored_voxels", "emf_fusion_copy_mesh_colors", "emf_fusion_copy_meshes_colors"]


def test_new_entries_are_declared_exported_and_typed():
    from emfusion_amd import _lib, pipeline
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in NEW_HIP:
        assert name in declared, f"{name} is not declared in include/emf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    fdecl = pipeline.declared_symbols()
    flib = pipeline.load()
    for name in NEW_FUSION:
        assert name in fdecl, f"{name} is not declared in include/emf_fusion.h"
        assert hasattr(flib, name), f"{name} is not exported"
        assert name in flib._emf_sigs, f"{name} has no ctypes signature"
    text = pipeline.HEADER_PATH.read_text()
    assert re.search(r"EMF_VOL_COLOR\s*=\s*5\b", text)
    assert pipeline.VOL["color"] == 5
    # the limits of the boundary: same ABI version, same struct sizes
    assert lib.emf_hip_abi_version() == 8
    assert C.sizeof(_lib.EmfModel) == 168


def test_colour_entries_reject_bad_arguments_before_any_launch():
    from emfusion_amd import _lib
    lib = _lib.load()
    res = (C.c_int32 * 3)(8, 8, 8)
    K = (C.c_float * 9)(*([0.0] * 9))
    img = _lib.EmfImage(C.c_void_p(256), 32, 8, 8)
    rgb = _lib.EmfImage(C.c_void_p(256), 24, 8, 8)
    pose = _lib.EmfPose()
    f = lib.emf_hip_integrateColorBatched
    assert f(None, C.c_void_p(16), C.byref(pose), res, 1, None, C.byref(img), None, C.byref(rgb), K, None, None) == -1
    assert f(C.c_void_p(16), C.c_void_p(16), C.byref(pose), res, 33, None, C.byref(img), None, C.byref(rgb), K, None,
             None) == -5
    narrow = _lib.EmfImage(C.c_void_p(256), 8, 8, 8)  # pitch smaller than a row of u8 x 3
    assert f(C.c_void_p(16), C.c_void_p(16), C.byref(pose), res, 1, None, C.byref(img), None, C.byref(narrow), K, None,
             None) == -3
    other = _lib.EmfImage(C.c_void_p(256), 48, 16, 8)
    assert f(C.c_void_p(16), C.c_void_p(16), C.byref(pose), res, 1, None, C.byref(img), None, C.byref(other), K, None,
             None) == -2
    bad = (C.c_int32 * 3)(8, 1, 8)
    assert lib.emf_hip_copyColorValues(C.c_void_p(16), C.c_void_p(16), res, bad, res, None) == -2
    assert lib.emf_hip_copyColorValues(None, C.c_void_p(16), res, res, res, None) == -1
