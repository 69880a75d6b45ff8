"""The free-viewpoint view without a device: emf_hip_renderView's argument checks (rejected before any launch), the
viewer placement helpers of pipeline.py, and the apps' --3d-vis refusal without --out."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from emfusion_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def _img(ptr, pitch, w, h):
    return _lib.EmfImage(C.c_void_p(ptr), pitch, w, h)


def test_render_view_arguments_are_rejected_before_any_launch():
    lib = _lib.load()
    W, H = 8, 4
    K = (C.c_float * 9)(*([1.0] * 9))
    light = (C.c_float * 3)()
    cmap = (C.c_uint8 * 768)()
    hide = (C.c_uint8 * 32)()
    ids = (C.c_int32 * 4)(1, 2, 3, 4)
    rgb = _img(256, 3 * W, W, H)
    tab, poses = C.c_void_p(4096), C.c_void_p(8192)

    def call(models=tab, poses_=poses, ids_=ids, n=2, w=W, h=H, k=K, li=light, cm=cmap, rgb_=C.byref(rgb), ray=None,
             seg=None, vert=None, nrm=None):
        return lib.emf_hip_renderView(models, poses_, ids_, n, w, h, k, li, cm, hide, rgb_, ray, seg, vert, nrm, None,
                                      None)

    assert call(models=None) == -1  # EMF_E_NULL
    assert b"models_dev is NULL" in lib.emf_hip_last_error_string()
    assert call(poses_=None) == -1
    assert call(ids_=None) == -1  # objects need their labels
    assert call(k=None) == -1
    assert call(cm=None) == -1
    assert call(rgb_=None) == -1
    assert call(rgb_=C.byref(_img(0, 3 * W, W, H))) == -1  # NULL data
    assert call(n=0) == -5  # EMF_E_LIMIT
    assert call(n=257) == -5
    assert call(w=0) == -2  # EMF_E_SHAPE
    assert call(h=-3) == -2
    assert call(rgb_=C.byref(_img(256, 3 * W + 3, W + 1, H))) == -2  # not the view's size
    assert call(rgb_=C.byref(_img(256, 3 * W - 1, W, H))) == -3  # EMF_E_PITCH: row does not fit
    assert call(ray=C.byref(_img(256, 4 * W - 4, W, H))) == -3
    assert call(ray=C.byref(_img(256, 4 * W + 2, W, H))) == -3  # f32 rows must stay 4-byte aligned
    assert call(vert=C.byref(_img(256, 12 * W, W, H + 1))) == -2
    assert call(seg=C.byref(_img(256, W - 1, W, H))) == -3
    assert call(nrm=C.byref(_img(0, 12 * W, W, H))) == -1
    # one model (the background alone) needs no labels
    assert call(ids_=None, n=1, w=0) == -2  # (reaches the size check: the NULL ids were accepted)


def test_look_at_is_a_proper_rotation_pointing_at_the_target():
    from emfusion_amd import pipeline
    rng = np.random.default_rng(7)
    for _ in range(50):
        eye, target = rng.normal(size=3) * 2, rng.normal(size=3)
        R, t = pipeline.look_at(eye, target)
        R64 = R.astype(np.float64)
        assert np.allclose(R64.T @ R64, np.eye(3), atol=1e-6)
        assert abs(np.linalg.det(R64) - 1) < 1e-6
        d = (target - eye) / np.linalg.norm(target - eye)
        assert np.allclose(R64[:, 2], d, atol=1e-6)  # +z looks at the target
        assert np.allclose(t, eye, atol=1e-6)
        # a point round-trips viewer -> world -> viewer, and the target sits on the optical axis
        p = rng.normal(size=3)
        assert np.allclose(R64.T @ (R64 @ p + t - t), p, atol=1e-5)
        q = R64.T @ (target - t)
        assert q[2] > 0 and np.allclose(q[:2], 0, atol=1e-5)
        # +y of the image points "down" (-up = +y of the world) as far as the direction allows
        assert R64[1, 1] >= -1e-6
    R, t = pipeline.look_at((0, 0, -1), (0, 0, 0))
    assert np.allclose(R, np.eye(3), atol=1e-7) and np.allclose(t, (0, 0, -1))
    with pytest.raises(ValueError):
        pipeline.look_at((0, 0, 0), (0, 0, 0))
    with pytest.raises(ValueError):
        pipeline.look_at((0, 0, 0), (0, 1, 0))  # straight along `up`


def test_default_3d_view_is_the_reference_window():
    from emfusion_amd import pipeline
    prm = pipeline.make_params(640, 480, 64, 0.04, 32)
    R, t, K, size = pipeline.default_3d_view(prm)
    assert size == (1024, 768)
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, [0, 0, -1])
    K0 = np.array(prm.K, np.float32).reshape(3, 3)
    assert np.isclose(K[0, 0], K0[0, 0] * 1.6) and np.isclose(K[1, 1], K0[1, 1] * 1.6)
    assert np.isclose(K[0, 2], K0[0, 2] * 1.6) and np.isclose(K[1, 2], K0[1, 2] * 1.6)


def test_synth_app_refuses_3d_vis_without_out():
    app = ROOT / "apps" / "emfusion_synth"
    if not app.exists():
        pytest.fail(f"{app} is missing: run __graft_entry__.build() first")
    r = subprocess.run([str(app), "--3d-vis", "--frames", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--out" in r.stderr and "--3d-vis" in r.stderr
    r = subprocess.run([str(app), "--3d-vis-eye", "1", "0", "0", "--out", "/nonexistent"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode != 0 and "--3d-vis" in r.stderr


def test_run_tum_refuses_3d_vis_without_out():
    r = subprocess.run([sys.executable, str(ROOT / "apps" / "run_tum.py"), "/nonexistent", "--3d-vis"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "needs --out" in r.stderr
