"""The scene of the colour tests: the smoke scene (background 64^3 at 0.04 m, one 32^3 object, 160 x 120) seen by a
slowly moving camera, with seeded RGB noise images and association maps that hold zeros, ones and fractions."""
from __future__ import annotations

import numpy as np

from tests.scenes import Pose, camera_path, intrinsics, rel_OC, render_depth

F = np.float32
W, H = 160, 120
NFRAMES = 6
MAXW = 64.0
SPHERE = ((0.1, 0.05, 1.2), 0.2)
BG = dict(res=(64, 64, 64), vox=0.04, trunc=float(F(3) * F(0.04)), pose=Pose(t=[0, 0, 1.28]))
OBJ_SIZE = 0.5
OBJ = dict(res=(32, 32, 32), vox=OBJ_SIZE / 32, trunc=float(F(0.0625)), pose=Pose(t=SPHERE[0]))


def rgb_noise(frame, w=W, h=H, seed=0xC0105):
    return np.random.default_rng(seed + frame).integers(0, 256, (h, w, 3), dtype=np.uint8)


def assoc_maps(ids, frame, seed=77):
    """(background map, object map): the object owns most of its silhouette outright, a seeded third of it by a
    fraction; the background owns the rest, except a stripe nobody owns (weight 0 in both)."""
    rng = np.random.default_rng(seed + frame)
    h, w = ids.shape
    frac = rng.choice(np.array([0.25, 0.5, 0.8125, 1.0, 1.0, 1.0], F), size=(h, w)).astype(F)
    obj = np.where(ids == 1, frac, F(0)).astype(F)
    bg = (F(1) - obj).astype(F)
    bg[:, 5:12] = 0
    obj[:, 5:12] = 0
    return bg, obj


def frames(n=NFRAMES, w=W, h=H, moving=True):
    """[(camera pose, depth, sphere ids, rgb)]"""
    K = intrinsics(w, h)
    out = []
    for f in range(n):
        cam = camera_path(f) if moving else Pose()
        depth, ids = render_depth(w, h, K, cam, [SPHERE], noise=0.002, dropout=0.01, seed=100 + f)
        out.append((cam, depth, ids, rgb_noise(f, w, h)))
    return out


def run_reference(models, n=NFRAMES, oracle=None):
    """The restatement over the scene's frames for models = [BG, OBJ]-like dicts; returns per model
    (tsdf, weights, color) after the sequence.  With `oracle`, its updateTSDF runs beside it on its own volumes (fed
    back frame after frame) and both pairs of volumes are returned for comparison."""
    from tests import color_reference as ref
    K = intrinsics(W, H)
    state = []
    for m in models:
        nx, ny, nz = m["res"]
        state.append(dict(t=np.zeros((nz, ny, nx), F), w=np.zeros((nz, ny, nx), F),
                          c=np.zeros((nz, ny, nx, 4), np.uint16),
                          ot=np.zeros((nz, ny, nx), F), ow=np.zeros((nz, ny, nx), F), n=0, frac=0))
    for f, (cam, depth, ids, rgb) in enumerate(frames(n)):
        maps = assoc_maps(ids, f)
        for m, s, a in zip(models, state, maps):
            oc = rel_OC(cam, m["pose"])
            s["n"] += ref.update(depth, a, s["t"], s["w"], oc.R32, oc.t32, K, m["vox"], m["trunc"], MAXW, rgb, s["c"])
            if oracle is not None:
                oracle.update_tsdf(depth, a, s["ot"], s["ow"], oc.R32, oc.t32, K, m["vox"], m["trunc"], MAXW)
    return state
