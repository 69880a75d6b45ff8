"""The distance-field restatement (tests/distance_reference.py) against itself -- all pairs equals the scipy form --
and the argument checks of the emf_hip_occupancy* / emf_hip_distanceTransform entries, which reject before any launch
and so need no device (include/emf_hip.h "Distance field")."""
import ctypes as C

import numpy as np
import pytest

from emfusion_amd import _lib
from tests import distance_reference as dr

E_ARG, E_LIMIT = -4, -5
P = C.c_void_p(4096)  # a non-NULL, aligned pointer that is never dereferenced


def i3(*v):
    return (C.c_int32 * 3)(*v)


@pytest.mark.parametrize("content", dr.CONTENTS)
def test_all_pairs_equals_the_scipy_form(content):
    sites = dr.site_field((10, 12, 40), content, seed=3)
    for cap in (0, 1, 5):
        assert dr.d2_brute(sites, cap).tobytes() == dr.d2_scipy(sites, cap).tobytes(), (content, cap)


def test_reference_values_by_hand():
    sites = np.zeros((3, 4, 5), bool)
    sites[1, 2, 3] = True
    d2 = dr.d2_scipy(sites)
    assert d2[1, 2, 3] == 0 and d2[0, 0, 0] == 1 + 4 + 9 and d2[2, 3, 4] == 3
    assert dr.d2_scipy(sites, cap=1)[0, 0, 0] == dr.FAR and dr.d2_scipy(sites, cap=1)[1, 2, 4] == 1
    assert (dr.d2_scipy(np.zeros((2, 2, 2), bool)) == dr.FAR).all()
    m = dr.metres_of(np.array([0, 2, dr.FAR], np.int32), 0.04)
    assert m[0] == 0 and m[1] == np.float32(np.sqrt(np.float32(2))) * np.float32(0.04) and np.isposinf(m[2])
    c = dr.classes_of(np.array([[[0.5, -0.0, np.nan, 0.5, 0.5, 0.5]]], np.float32),
                      np.array([[[1.0, 1.0, 1.0, 0.0, -1.0, np.nan]]], np.float32))
    assert c.reshape(-1).tolist() == [dr.FREE, dr.OCCUPIED, dr.OCCUPIED, dr.UNKNOWN, dr.UNKNOWN, dr.UNKNOWN]
    for mask in range(1, 8):
        s = dr.site_field((4, 5, 6), "p50", seed=mask)
        assert (dr.sites_of(dr.classes_with_sites(s, mask), mask) == s).all()


def test_classes_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    res, lo, size = i3(16, 16, 16), i3(0, 0, 0), i3(16, 16, 16)
    f = lib.emf_hip_occupancyClasses
    assert f(None, P, res, lo, size, P, None) == E_ARG
    assert f(P, None, res, lo, size, P, None) == E_ARG
    assert f(P, P, res, lo, size, None, None) == E_ARG
    assert f(P, P, None, lo, size, P, None) == E_ARG
    assert f(P, P, res, None, size, P, None) == E_ARG
    assert f(P, P, res, lo, None, P, None) == E_ARG
    assert f(P, P, res, i3(1, 0, 0), size, P, None) == E_ARG  # leaves the volume
    assert f(P, P, res, i3(0, -1, 0), i3(4, 4, 4), P, None) == E_ARG
    assert f(P, P, res, i3(0, 0, 13), i3(4, 4, 4), P, None) == E_ARG
    assert b"leaves the volume" in lib.emf_hip_last_error_string()
    assert f(P, P, res, lo, i3(16, 0, 16), P, None) == E_ARG
    big = i3(4096, 16, 16)
    assert f(P, P, big, lo, i3(2049, 4, 4), P, None) == E_LIMIT
    assert f(P, P, i3(2048, 2048, 2048), lo, i3(2048, 2048, 512), P, None) == E_LIMIT  # 2^31 voxels
    assert b"2^31 - 1" in lib.emf_hip_last_error_string()


def test_stamp_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    res, lo, size = i3(16, 16, 16), i3(0, 0, 0), i3(16, 16, 16)
    obj = _lib.EmfOccObject(4096, 4096, None, i3(8, 8, 8), 0.01, (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1),
                            (C.c_float * 3)(0, 0, 0), i3(0, 0, 0), i3(16, 16, 16))
    f = lib.emf_hip_occupancyStampObjects
    assert f(None, res, 0.01, lo, size, C.byref(obj), 1, None) == E_ARG
    assert f(P, res, 0.01, lo, size, None, 1, None) == E_ARG
    assert f(P, res, 0.01, lo, size, C.byref(obj), -1, None) == E_ARG
    assert f(P, res, 0.0, lo, size, C.byref(obj), 1, None) == E_ARG
    assert f(P, res, 0.01, i3(8, 8, 8), i3(9, 8, 8), C.byref(obj), 1, None) == E_ARG
    assert f(P, i3(4096, 16, 16), 0.01, lo, i3(2049, 1, 1), C.byref(obj), 1, None) == E_LIMIT
    assert f(P, res, 0.01, lo, i3(0, 8, 8), C.byref(obj), 1, None) == E_ARG
    bad = _lib.EmfOccObject.from_buffer_copy(obj)
    bad.weights = None
    assert f(P, res, 0.01, lo, size, C.byref(bad), 1, None) == E_ARG
    bad = _lib.EmfOccObject.from_buffer_copy(obj)
    bad.voxelSize = -1.0
    assert f(P, res, 0.01, lo, size, C.byref(bad), 1, None) == E_ARG
    assert f(P, res, 0.01, lo, size, None, 0, None) == 0  # an empty list launches nothing


def test_object_box_covers_the_object_and_needs_no_device():
    lib = _lib.load()
    assert C.sizeof(_lib.EmfOccObject) == 112
    obj = _lib.EmfOccObject(4096, 4096, None, i3(24, 24, 24), 0.02, (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1),
                            (C.c_float * 3)(0, 0, 0), i3(0, 0, 0), i3(0, 0, 0))
    assert lib.emf_hip_occupancyObjectBox(C.byref(obj), i3(48, 48, 48), 0.02) == 0
    # object voxels 0 .. 23 sit on background voxels 12 .. 35; half a voxel either side, then one of margin
    assert list(obj.lo) == [10, 10, 10] and list(obj.size) == [28, 28, 28]
    obj.t = (C.c_float * 3)(1.0, 0, 0)  # p_o = p_b + 1 m: the object lies 50 voxels below the volume
    assert lib.emf_hip_occupancyObjectBox(C.byref(obj), i3(48, 48, 48), 0.02) == 0
    assert 0 in list(obj.size)
    obj.R = (C.c_float * 9)(*([0.0] * 9))  # singular: everywhere
    assert lib.emf_hip_occupancyObjectBox(C.byref(obj), i3(48, 40, 32), 0.02) == 0
    assert list(obj.lo) == [0, 0, 0] and list(obj.size) == [48, 40, 32]
    assert lib.emf_hip_occupancyObjectBox(None, i3(48, 48, 48), 0.02) == E_ARG
    assert lib.emf_hip_occupancyObjectBox(C.byref(obj), i3(48, 48, 48), 0.0) == E_ARG


def test_transform_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    size = i3(16, 16, 16)
    f = lib.emf_hip_distanceTransform
    assert f(None, size, 2, 0, P, None, 0.0, None) == E_ARG
    assert f(P, size, 2, 0, None, None, 0.0, None) == E_ARG
    assert f(P, None, 2, 0, P, None, 0.0, None) == E_ARG
    assert f(P, i3(16, 0, 16), 2, 0, P, None, 0.0, None) == E_ARG
    assert f(P, i3(16, 16, -3), 2, 0, P, None, 0.0, None) == E_ARG
    assert f(P, i3(2049, 1, 1), 2, 0, P, None, 0.0, None) == E_LIMIT
    assert f(P, i3(1, 1, 2049), 2, 0, P, None, 0.0, None) == E_LIMIT
    assert f(P, i3(2048, 2048, 512), 2, 0, P, None, 0.0, None) == E_LIMIT
    assert f(P, size, 0, 0, P, None, 0.0, None) == E_ARG
    assert f(P, size, 8, 0, P, None, 0.0, None) == E_ARG
    assert b"site_mask" in lib.emf_hip_last_error_string()
    assert f(P, size, 2, -1, P, None, 0.0, None) == E_ARG
    assert f(P, size, 2, 0, P, P, 0.0, None) == E_ARG  # metres need a voxel size
    assert f(P, size, 2, 0, P, P, float("nan"), None) == E_ARG
