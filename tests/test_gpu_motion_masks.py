"""emf_hip_motionMasks against its restatement (tests/motion_reference.py): labels, mask planes, info records and the
count, equal byte for byte, at sizes that are ragged against every tile, one pixel, one narrow strip and several
workgroups; plus the argument checks and the zeroing of unused planes."""
import ctypes as C

import numpy as np
import pytest

from tests import motion_reference as mr

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (67, 45), (1, 1), (5, 300), (160, 120))  # width x height

_CASES = {}


def cases(w, h):
    """The inputs of one size, built once and shared by the three erosion depths (never modified)."""
    if (w, h) not in _CASES:
        _CASES[(w, h)] = mr.cases(h, w)
        for _, p, b, _ in _CASES[(w, h)]:
            p.setflags(write=False)
            b.setflags(write=False)
    return _CASES[(w, h)]


def assert_equal(got, ref, what):
    assert got["count"] == ref["count"], what
    for key in ("labels", "masks", "info"):
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, (what, key)
        assert got[key].tobytes() == ref[key].tobytes(), (what, key)


@pytest.mark.parametrize("erode", (0, 1, 2))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_equal_the_restatement(dev, size, erode):
    from emfusion_amd import ops
    w, h = size
    buffers = ops.MotionBuffers(w, h)  # one set of buffers for all cases: whatever a call leaves behind must not matter
    proposals = 0
    for name, points, bg, params in cases(w, h):
        ref = mr.motion_masks(points, bg, erode=erode, **params)
        got = ops.motion_masks(points, bg, erode=erode, buffers=buffers, **params)
        assert_equal(got, ref, f"{name} {w}x{h} erode={erode}")
        assert got["proposals"] == mr.proposals(ref)
        proposals += ref["count"]
    if min(w, h) > 5 and erode < 2:
        assert proposals > 0  # the comparison is not one of empty results


def test_unused_planes_are_zeroed_when_fewer_proposals_follow_more(dev):
    from emfusion_amd import ops
    w, h = 67, 45
    buffers = ops.MotionBuffers(w, h, 16)
    many = mr.scene(mr.blob_grid(h, w))
    few = mr.scene(mr.two_blobs_with_bridge(h, w))
    first = ops.motion_masks(*many, erode=0, min_pixels=1, max_masks=16, buffers=buffers)
    assert first["count"] == 16 and all(plane.any() for plane in first["masks"])
    second = ops.motion_masks(*few, erode=1, min_pixels=1, max_masks=16, buffers=buffers)
    assert second["count"] == 2
    assert not second["masks"][2:].any() and not second["info"][2:].any()
    assert_equal(second, mr.motion_masks(*few, erode=1, min_pixels=1, max_masks=16), "after a fuller call")
    none = ops.motion_masks(few[0], np.zeros((h, w), np.float32), erode=1, min_pixels=1, max_masks=16, buffers=buffers)
    assert none["count"] == 0 and not none["masks"].any() and not none["info"].any() and (none["labels"] == -1).all()


def test_rejected_arguments(dev):
    from emfusion_amd import _lib, ops
    from emfusion_amd.devmem import DeviceArray
    lib = _lib.load()
    EMF_E_ARG = -4
    w, h = 16, 8
    b = ops.MotionBuffers(w, h, 16)
    pts = DeviceArray.zeros((h, w, 3), np.float32)
    bg = DeviceArray.zeros((h, w), np.float32)
    b.count.copy_from(np.array([77], np.int32))

    def call(motion=None, null=None):
        p = motion if motion is not None else ops.motion_params(max_masks=16)
        args = dict(points=pts.ptr, bg=bg.ptr, params=C.addressof(p), scratch=b.scratch.ptr, labels=b.labels.ptr,
                    masks=b.masks.ptr, info=b.info.ptr, count=b.count.ptr)
        if null:
            args[null] = None
        return lib.emf_hip_motionMasks(args["points"], args["bg"], w, h, args["params"], args["scratch"], args["labels"],
                                       args["masks"], args["info"], args["count"], None)

    for name in ("points", "bg", "params", "scratch", "labels", "masks", "info", "count"):
        assert call(null=name) == EMF_E_ARG, name
        assert b"NULL" in lib.emf_hip_last_error_string()
    for bad in (dict(erode=4), dict(erode=-1), dict(max_masks=0), dict(max_masks=17), dict(max_masks=-3),
                dict(min_pixels=-1), dict(band=-0.5), dict(band=float("nan")), dict(continuity=-1.0)):
        assert call(ops.motion_params(**bad)) == EMF_E_ARG, bad
    assert lib.emf_hip_motionMasksScratchBytes(w, h, 0) == 0 and lib.emf_hip_motionMasksScratchBytes(w, h, 17) == 0
    assert lib.emf_hip_motionMasksScratchBytes(0, h, 8) == 0 and lib.emf_hip_motionMasksScratchBytes(1 << 16, 1 << 15, 8) == 0
    assert 0 < lib.emf_hip_motionMasksScratchBytes(640, 480, 8) < 19 * 640 * 480 + 1024
    with pytest.raises(_lib.EmfHipError) as err:
        ops.motion_masks(np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), erode=7, buffers=b)
    assert err.value.code == EMF_E_ARG
    assert int(b.count.numpy()[0]) == 77  # nothing was enqueued by any of the rejected calls
    assert call() == 0 and int(b.count.numpy()[0]) == 0
