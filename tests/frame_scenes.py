"""Scenes of the per-frame kernel tests at a given image size: what tests/test_gpu_batched.py (`Model`, `frame`, `scene`)
and tests/test_gpu_tracking.py (`world`, `DeviceTracker`) build at their fixed 160 x 120, here with the size as an argument.
tests/scenes.intrinsics scales with the size, so the same spheres and the same camera path stay in view.

Everything a size needs from the oracle is computed once and kept (`batched_scene`, `tracking_world`, `oracle_track`):
the tests share it and leave it unchanged."""
import ctypes as C

import numpy as np

from tests.oracle_tracking import OracleTracker, orthonormalise
from tests.parity_util import dev_full, to_dev
from tests.scenes import Pose, camera_path, intrinsics, rel_CO, rel_OC, render_depth, rot

SPHERES = [((0.25, 0.05, 1.3), 0.22), ((-0.3, -0.1, 1.6), 0.18)]
SIGMA, ALPHA, PRIOR, MAXW = 0.02, 0.8, 1.0, 64.0


def frame(size, i):
    """Frame i of the camera path at size = (W, H): camera pose, noisy depth with drop-outs, sphere ids."""
    w, h = size
    cam = camera_path(i)
    depth, ids = render_depth(w, h, intrinsics(w, h), cam, SPHERES, noise=0.002, dropout=0.01, seed=100 + i)
    return cam, depth, ids


# ---- the model table of tests/test_gpu_batched.py -------------------------------------------------

class Model:
    """One volume with its device buffers and output images of size (W, H), integrated identically on oracle and device."""

    def __init__(self, ops, oracle, size, res, vox, pose, is_obj, mid):
        self.ops, self.oracle = ops, oracle
        self.W, self.H = size
        self.K = intrinsics(*size)
        self.res, self.vox, self.pose, self.id = res, np.float32(vox), pose, mid
        shape = (res[2], res[1], res[0])
        self.tsdf, self.wts = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        self.d_tsdf, self.d_wts = to_dev(self.tsdf), to_dev(self.wts)
        self.d_flags = dev_full(ops.brick_shape(shape), 0, np.uint8)
        ops.reset_brick_flags(self.d_tsdf, self.d_flags)
        self.is_obj = is_obj
        self.vmask = None
        if is_obj:
            self.fgbg = np.zeros(shape + (2,), np.float32)
        H, W = self.H, self.W
        self.d_assoc = dev_full((H, W), 1.0)
        self.d_ray, self.d_vert, self.d_nrm = dev_full((H, W), 0.0), dev_full((H, W, 3), 0.0), dev_full((H, W, 3), 0.0)
        self.d_hit = dev_full((H, W), 0, np.uint8)
        self.d_sign = None  # sign maps and relevant-tile list: set by the tests of the far bounds
        self.d_rel = None

    @property
    def trunc(self):
        return np.float32(10) * self.vox

    @property
    def images(self):
        return [self.d_ray, self.d_vert, self.d_nrm, self.d_hit]

    def poison(self):
        """What a raycast that skips a pixel leaves behind."""
        H, W = self.H, self.W
        self.d_ray.copy_from(np.full((H, W), 5, np.float32))
        self.d_vert.copy_from(np.full((H, W, 3), 5, np.float32))
        self.d_nrm.copy_from(np.full((H, W, 3), 5, np.float32))
        self.d_hit.copy_from(np.full((H, W), 5, np.uint8))

    def clear(self):
        """What the per-volume raycast starts from: it reads the ray lengths (another volume's hit bounds its search,
        TSDF.cu:496-500) and leaves pixels without a hit untouched, as the reference does."""
        for im in self.images:
            im.copy_from(np.zeros(im.shape, im.dtype))

    def integrate(self, cam, depth):
        oc = rel_OC(cam, self.pose)
        assoc = np.ones((self.H, self.W), np.float32)
        self.oracle.update_tsdf(depth, assoc, self.tsdf, self.wts, oc.R32, oc.t32, self.K, self.vox, self.trunc, MAXW)
        self.ops.update_tsdf(to_dev(depth), to_dev(assoc), self.d_tsdf, self.d_wts, oc.R32, oc.t32, self.K, self.vox,
                             self.trunc, MAXW, brick_flags=self.d_flags)

    def finish_fg(self, cam, ids):
        oc = rel_OC(cam, self.pose)
        self.oracle.update_fgbg_probs((ids == self.id).astype(np.uint8), np.zeros((self.H, self.W), np.uint8), self.tsdf,
                                      self.wts, self.fgbg, oc.R32, oc.t32, self.K, self.vox)
        self.probs, self.vmask = self.oracle.compute_fg_probs(self.fgbg)
        self.d_probs, self.d_vmask = to_dev(self.probs), to_dev(self.vmask)

    def table_entry(self):
        return self.ops.make_model(
            self.d_tsdf, self.d_wts, self.d_assoc, self.d_ray, self.d_vert, self.d_nrm, self.d_hit, float(self.vox),
            float(self.trunc), MAXW, SIGMA, ALPHA, PRIOR, model_id=self.id, fg_probs=self.d_probs if self.is_obj else None,
            fg_mask=self.d_vmask if self.is_obj else None, brick_flags=self.d_flags,
            rcp_voxel=self.ops.voxel_reciprocal(self.vox), sign_maps=self.d_sign, relevant_tiles=self.d_rel)


class BatchedScene:
    """The three-model scene of tests/test_gpu_batched.py after four frames, the camera of frame 4, and the oracle's
    raycast of every model from there (ray, vertex, normal, mask, samples per ray)."""

    def __init__(self, ops, oracle, dev, size):
        self.size = size
        self.K = intrinsics(*size)
        self.models = [Model(ops, oracle, size, (64, 64, 64), 0.04, Pose(t=[0, 0, 1.28]), False, 0),
                       Model(ops, oracle, size, (32, 32, 32), 0.025, Pose(t=SPHERES[0][0]), True, 1),
                       Model(ops, oracle, size, (40, 32, 24), 0.025, Pose(rot([0, 1, 0], 7), SPHERES[1][0]), True, 2)]
        for i in range(4):
            cam, depth, ids = frame(size, i)
            for m in self.models:
                m.integrate(cam, depth)
                if m.is_obj:
                    m.finish_fg(cam, ids)
        dev.synchronize()
        cam = camera_path(4)
        self.poses = [(rel_CO(cam, m.pose).R32, rel_CO(cam, m.pose).t32) for m in self.models]
        self.want = [oracle.raycast_tsdf(m.tsdf, None, m.wts, m.vmask, size[0], size[1], R, t, self.K, m.vox, m.trunc,
                                         count_steps=True) for m, (R, t) in zip(self.models, self.poses)]

    def hits(self, k):
        return int(self.want[k][3].sum())

    def samples(self, which):
        return sum(int(self.want[k][4].sum()) for k in which)


_batched = {}


def batched_scene(ops, oracle, dev, size):
    if size not in _batched:
        _batched[size] = BatchedScene(ops, oracle, dev, size)
    return _batched[size]


# ---- the tracker's world of tests/test_gpu_tracking.py --------------------------------------------

BG = dict(n=(64, 64, 64), vox=0.04, pose=Pose(t=[0, 0, 1.28]))
OBJ = dict(n=(32, 32, 32), vox=0.02, pose=Pose(t=SPHERES[0][0]))


def _integrate(oracle, size, vol, frames):
    w, h = size
    n = vol["n"]
    tsdf, wts = np.zeros((n[2], n[1], n[0]), np.float32), np.zeros((n[2], n[1], n[0]), np.float32)
    for i in frames:
        cam, depth, _ = frame(size, i)
        oc = rel_OC(cam, vol["pose"])
        oracle.update_tsdf(depth, np.ones((h, w), np.float32), tsdf, wts, oc.R32, oc.t32, intrinsics(w, h), vol["vox"],
                           10 * vol["vox"], 64.0)
    return tsdf, wts


_worlds = {}


def tracking_world(oracle, size):
    """Background and object volumes after four frames, the points of frame 5, association weights and a start pose
    that is off by ~1.5 cm and ~0.6 degrees."""
    if size in _worlds:
        return _worlds[size]
    w, h = size
    vols = []
    for v in (BG, OBJ):
        tsdf, wts = _integrate(oracle, size, v, range(4))
        vols.append(dict(v, tsdf=tsdf, wts=wts))
    cam, depth, _ = frame(size, 5)
    points = oracle.compute_points(depth, intrinsics(w, h))
    rng = np.random.default_rng(3)
    assoc = [np.ones((h, w), np.float32), rng.uniform(0.2, 1.0, (h, w)).astype(np.float32)]
    guess = cam * Pose(rot([0.2, 1.0, 0.3], 0.6), [0.012, -0.006, 0.008])
    _worlds[size] = dict(size=size, weights="integrated", vols=vols, cam=cam, guess=guess, points=points, assoc=assoc)
    return _worlds[size]


def ramped(world):
    """The same world with integration weights that grow along x: their maximum over the image moves with the pose
    (tests/test_gpu_tracking.py, _ramped)."""
    vols = []
    for v in world["vols"]:
        nx = v["wts"].shape[2]
        ramp = (1.0 + np.arange(nx, dtype=np.float32) / nx)[None, None, :]
        vols.append(dict(v, wts=(v["wts"] * ramp).astype(np.float32)))
    return dict(world, weights="ramped", vols=vols)


def start_pose(world, k):
    co = rel_CO(world["guess"], world["vols"][k]["pose"])
    return orthonormalise(co.R32.reshape(3, 3)).reshape(-1), co.t32


class DeviceTracker:
    """The device LM loop over the models `which` of a world (a model may be listed several times: the copies share one
    table entry -- k_track_step writes states and scratch only, nothing through the table's image pointers).
    pad_cols: row padding of the uploaded points image (the pitched addressing of the kernels)."""

    def __init__(self, ops, world, which, pad_cols=0):
        from emfusion_amd import _lib
        w, h = world["size"]
        self.ops, self.n = ops, len(which)
        self.keep, entries = {}, {}
        for k in set(which):
            v = world["vols"][k]
            d = dict(tsdf=to_dev(v["tsdf"]), wts=to_dev(v["wts"]), assoc=to_dev(world["assoc"][k]), ray=dev_full((h, w), 0.0),
                     vert=dev_full((h, w, 3), 0.0), nrm=dev_full((h, w, 3), 0.0), hit=dev_full((h, w), 0, np.uint8))
            self.keep[k] = d
            entries[k] = ops.make_model(d["tsdf"], d["wts"], d["assoc"], d["ray"], d["vert"], d["nrm"], d["hit"],
                                        float(np.float32(v["vox"])), float(np.float32(10 * v["vox"])), 64.0, 0.02, 0.8, 1.0,
                                        model_id=k)
        self.table = ops.upload_models([entries[k] for k in which])
        self.states = dev_full((self.n * C.sizeof(_lib.EmfTrackState),), 0, np.uint8)
        self.per_model = ops.track_scratch_bytes(w, h)
        self.scratch = dev_full((self.n * self.per_model,), 0, np.uint8)
        self.points = to_dev(world["points"], pad_cols=pad_cols)
        self.params = _lib.EmfTrackParams.defaults()
        ops.track_prepare(self.states, [start_pose(world, k) for k in which])

    def iterate(self, iterations=1):
        self.ops.track_iterate(self.table, self.states, self.n, self.points, self.params, self.scratch, self.per_model,
                               iterations)
        return self.ops.read_track_states(self.states, self.n)


def oracle_tracker(oracle, world, k):
    v = world["vols"][k]
    t = OracleTracker(oracle, v["tsdf"], v["wts"], v["vox"])
    t.prepare(*start_pose(world, k))
    return t


_tracks = {}


def oracle_track(oracle, world, k, iterations):
    """The oracle's LM loop on model k: a snapshot (history, R, t, mu, accepted) after every iteration, [0] = the start."""
    key = (world["size"], world["weights"], k, iterations)
    if key not in _tracks:
        ot = oracle_tracker(oracle, world, k)
        snaps = []
        for i in range(iterations + 1):
            if i:
                ot.iterate(world["points"], world["assoc"][k])
            snaps.append(dict(history=list(ot.history), R=ot.R.copy(), t=ot.t.copy(), mu=float(ot.mu), accepted=ot.accepted))
        _tracks[key] = snaps
    return _tracks[key]
