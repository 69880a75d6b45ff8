"""Checkpoint and resume of a session (Fusion.save_checkpoint / load_checkpoint, emfusion_amd/csrc/core/Checkpoint.cpp).

The acceptance test is CONTINUATION: n frames uninterrupted against k frames, save, close, a new Fusion, load, the rest
-- every volume, every image tests/long_sequence.py's snapshot_digests lists, the per-frame visible sets, the object
table, the frame index and all poses must be the same bytes.  The scene is the small one of the colour and life-cycle
tests: background 64^3 at 4 cm, 32^3 objects, 160 x 120."""
import functools
import inspect
import os
import shutil
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

from tests import checkpoint_format as CF
from tests import pack_reference as PR
from tests.parity_util import to_dev
from tests.scenes import camera_path, intrinsics, render_depth

pytestmark = pytest.mark.gpu

W, H = 160, 120
MASK_EVERY = 4
N, CUT = 10, 6
SPHERES = {1: ((0.10, 0.05, 1.20), 0.20, 0.50), 2: ((-0.38, 0.00, 1.35), 0.17, 0.45)}  # centre, radius, volume edge
FAR = np.array([0.0, 0.0, -30.0], np.float32)
EYE = np.eye(3, dtype=np.float32).reshape(-1)
IMAGES = ("raylengths", "segmentation", "assoc_norm", "bg_assoc", "bg_raylengths", "vertices", "normals")
_frames, _runs = {}, {}
ROOT = Path(__file__).resolve().parent.parent
CHILD = "EMF_CHECKPOINT_TEST_CHILD"  # set in the child processes of own_process()


def own_process(fn):
    """Runs the test in a pytest process of its own and passes if that one does.  The module creates some forty
    instances (also on rank threads), each with its four streams; HIP maps a process's streams onto a few hardware
    queues by their creation history, and modules that run later in the same interpreter keep two ranks spinning on
    each other's flags on one GPU (tests/test_gpu_sharded_lifecycle.py, peer transport) -- with this module's history
    in front of them their streams land on one queue and the bounded wait expires.  As tests/test_gpu_peer_exchange.py,
    test_gpu_exchange_latency.py, test_gpu_dynamic_objects.py and test_gpu_stream_history.py do for the same reason,
    everything that opens an instance runs in a child; the caller's process keeps the history it had."""
    params = list(inspect.signature(fn).parameters.values())
    wants_request = any(p.name == "request" for p in params)

    @functools.wraps(fn)
    def wrapper(*args, request, **kw):
        if os.environ.get(CHILD):
            return fn(*args, **({"request": request} if wants_request else {}), **kw)
        p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", request.node.nodeid],
                           cwd=ROOT, env=dict(os.environ, **{CHILD: "1"}), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and " passed" in p.stdout, p.stdout[-6000:] + p.stderr[-2000:]

    if not wants_request:
        params.append(inspect.Parameter("request", inspect.Parameter.KEYWORD_ONLY))
    wrapper.__signature__ = inspect.Signature(params)
    return wrapper


def frame(f, hidden=(), size=(W, H)):
    """(depth, sphere ids, camera R9, t3) of frame f; spheres listed in `hidden` are not in the scene."""
    key = (f, tuple(hidden), size)
    if key not in _frames:
        w, h = size
        sph = [(SPHERES[k][0], SPHERES[k][1] if k not in hidden else 1e-6) for k in (1, 2)]
        cam = camera_path(f)
        depth, ids = render_depth(w, h, intrinsics(w, h), cam, sph, noise=0.002, dropout=0.01, seed=300 + f)
        _frames[key] = (depth, ids.astype(np.uint8), cam.R32, cam.t32)
    return _frames[key]


def rgb_noise(f):
    return np.random.default_rng(0xC0105 + f).integers(0, 256, (H, W, 3), dtype=np.uint8)


def new_fusion(env=None, size=(W, H), bg_res=64, bg_voxel=0.04, comm=None):
    from emfusion_amd import pipeline
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        prm = pipeline.make_params(size[0], size[1], bg_res, bg_voxel, 32, visibility_thresh=100, boundary=5,
                                   mask_frames=MASK_EVERY)
        return pipeline.Fusion(prm, comm)
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)


def mask_of(ids, k):
    return (ids == k).astype(np.uint8)


class Scenario:
    """A stream whose inputs are a function of the frame number and of what the Fusion itself reports, so that a
    process that resumes at frame k needs nothing but the checkpoint.  switches(): what a caller sets at start, and
    again after a resume; populate(): what only a session that starts at frame 0 does."""
    env = None
    color = False
    pose_log = False
    size = (W, H)

    def switches(self, fus):
        if self.pose_log:
            fus.enable_pose_log(True)

    def populate(self, fus):
        for k in (1, 2):
            assert fus.add_object(np.array(SPHERES[k][0], np.float32), SPHERES[k][2]) == k

    def hidden(self, f):
        return ()

    def step(self, fus, f):
        from emfusion_amd.ops import image_view
        depth, ids, R, t = frame(f, self.hidden(f), self.size)
        keep = [to_dev(depth)]
        poses, masks, run_masks = self.inputs(fus, f, ids, keep)
        if self.color:
            keep.append(to_dev(rgb_noise(f)))
            fus.set_color_image(image_view(keep[-1]))
        views = {}
        for i, m in masks.items():
            keep.append(to_dev(m))
            views[i] = image_view(keep[-1])
        fus.process_frame(image_view(keep[0]), R, t, poses, views, run_masks)
        fus.synchronize()
        return self.record(fus, f)

    def inputs(self, fus, f, ids, keep):
        live = fus.object_ids()
        poses = {k: (EYE, FAR if k in self.hidden(f) else np.array(SPHERES[k][0], np.float32)) for k in live}
        masks = {}
        if f % MASK_EVERY == 0:
            masks = {k: mask_of(ids, k) for k in live if int(mask_of(ids, k).sum()) > 100}
        return poses, masks, bool(masks)

    def record(self, fus, f):
        return dict(visible=sorted(fus.visible_objects()), ids=fus.object_ids(), created=fus.last_created(),
                    deleted=fus.last_deleted())


class Supplied(Scenario):
    """Supplied poses; object 2 leaves the scene in frames 2-5 (gated out of the integration when the run is cut at
    frame 6) and is back from frame 6 on; masks on frames 0, 4 and -- after the cut -- 8."""

    def hidden(self, f):
        return (2,) if 2 <= f <= 5 else ()


class Tracked(Scenario):
    """Camera and object tracking from frame 1 on; the tracking outcome of every model is part of the record."""

    def step(self, fus, f):
        if f >= 1:  # frame 0 defines the world frame
            fus.set_tracking(camera=True, objects=True)
        return super().step(fus, f)

    def record(self, fus, f):
        r = super().record(fus, f)
        r["track"] = {i: fus.track_result(i) for i in [0] + fus.object_ids()} if f >= 1 else {}
        r["poses"] = {i: tuple(np.asarray(x).tobytes() for x in fus.pose(i)) for i in [0] + fus.object_ids()}
        return r


class Resized(Scenario):
    """Object 1 is created from a small patch of sphere 1 on frame 0 and, before frame 3, outgrows its volume under
    the full mask: ObjTSDF::resize leaves a resolution that is no multiple of 4 (no tile launches, no sign maps).
    At 320 x 240: the points under the mask must outnumber the surface vertices of the small volume for the
    percentile box to leave it."""
    pose_log = True
    size = (320, 240)
    PATCH = 12  # (half the patch edge in pixels: the resize then leaves 74^3)

    def populate(self, fus):
        pass

    def inputs(self, fus, f, ids, keep):
        from emfusion_amd.ops import image_view
        full = mask_of(ids, 1)
        if f == 0:
            ys, xs = np.nonzero(full)
            cy, cx = int(ys.mean()), int(xs.mean())
            patch = np.zeros_like(full)
            patch[cy - self.PATCH:cy + self.PATCH, cx - self.PATCH:cx + self.PATCH] = 1
            keep.append(to_dev(patch & full))
            fus.queue_new_object_masks([image_view(keep[-1])])
            return {}, {}, True
        if f == 3:  # under the full mask of the frame just processed
            keep.append(to_dev(mask_of(frame(2, (), self.size)[1], 1)))
            shift = fus.update_object(1, image_view(keep[-1]))
            assert np.any(shift != 0), "the scenario must outgrow the volume"
            res = fus.object_info(1)["res"]
            assert res[0] > 32 and res[0] % 4 == 2, res
        R1, t1 = fus.pose(1)
        return {1: (np.asarray(R1, np.float32).reshape(-1), t1)}, {1: full}, True


class CleanedUp(Scenario):
    """Clean-up on: objects 1 and 2 are created from masks on frame 0, object 2 is reported far away on frame 3 and
    deleted there (its last mesh is kept: the pose log is on); on frame 7 -- after the cut -- sphere 2's mask spawns a
    new object, which must get id 3 in both runs."""
    pose_log = True

    def switches(self, fus):
        super().switches(fus)
        fus.set_cleanup(True)

    def populate(self, fus):
        pass

    def inputs(self, fus, f, ids, keep):
        from emfusion_amd.ops import image_view
        if f == 0 or f == 7:
            new = [k for k in (1, 2) if f == 0 or k == 2]
            for k in new:
                keep.append(to_dev(mask_of(ids, k)))
            fus.queue_new_object_masks([image_view(m) for m in keep[-len(new):]])
        live = fus.object_ids()
        poses = {i: (EYE, fus.pose(i)[1]) for i in live}
        if f == 3:
            poses[2] = (EYE, FAR)
        sphere_of = {1: 1, 2: 2, 3: 2}
        return poses, {i: mask_of(ids, sphere_of[i]) for i in live}, True


class Coloured(Supplied):
    color = True


class PerVolume(Supplied):
    env = {"EMF_PER_VOLUME": "1"}


class NoOverlap(Supplied):
    env = {"EMF_BG_OVERLAP": "0"}


def snapshot(fus, color=False):
    """Every volume, every image of long_sequence.snapshot_digests, the object table, the frame index, all poses."""
    ids = fus.object_ids()
    out = {"ids": ids, "frame_index": fus.frame_index(), "visible": sorted(fus.visible_objects())}
    for i in [0] + ids:
        kinds = ("tsdf", "weights") + (("fgbg", "fgprobs", "fgmask") if i else ()) + (("color",) if color else ())
        for which in kinds:
            v = fus.volume(which, i)
            out[f"{i} {which}"] = (v.shape, v.tobytes())
        out[f"{i} pose"] = tuple(np.asarray(x).tobytes() for x in fus.pose(i))
        if i:
            out[f"{i} info"] = repr(sorted(fus.object_info(i).items()))
            out[f"{i} assoc"] = fus.image("obj_assoc", i).tobytes()
            out[f"{i} raylengths"] = fus.image("obj_raylengths", i).tobytes()
    for im in IMAGES:
        out[im] = fus.image(im).tobytes()
    return out


def start(sc):
    fus = new_fusion(sc.env, sc.size)
    if sc.color:
        fus.enable_color(True)
    sc.switches(fus)
    sc.populate(fus)
    return fus


def results(fus, directory):
    fus.write_results(directory, volumes=False)
    return {p.name: p.read_bytes() for p in sorted(directory.iterdir()) if p.is_file()}


def uninterrupted(cls, tmp_path_factory):
    """The reference run of a scenario: computed once per module and left unchanged."""
    if cls not in _runs:
        sc = cls()
        fus = start(sc)
        rec = [sc.step(fus, f) for f in range(N)]
        out = dict(frames=rec, final=snapshot(fus, sc.color))
        if sc.pose_log:
            out["files"] = results(fus, tmp_path_factory.mktemp("whole"))
        fus.close()
        _runs[cls] = out
    return _runs[cls]


def same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k] == want[k], (what, k)


@pytest.mark.parametrize("cls", [Supplied, Tracked, Resized, CleanedUp, Coloured, PerVolume, NoOverlap])
@own_process
def test_a_resumed_session_continues_with_the_same_bytes(dev, tmp_path, tmp_path_factory, cls):
    from emfusion_amd import pipeline
    want = uninterrupted(cls, tmp_path_factory)
    sc = cls()
    fus = start(sc)
    rec = [sc.step(fus, f) for f in range(CUT)]
    saved = tmp_path / "saved" / "session.ckpt"
    saved.parent.mkdir()
    stats = fus.save_checkpoint(saved)
    before = snapshot(fus, sc.color)
    fus.close()
    assert not saved.with_name(saved.name + ".tmp").exists()
    assert stats["file_bytes"] == saved.stat().st_size and stats["raw_bytes"] > stats["file_bytes"]
    # saved on one path, loaded on another
    moved = tmp_path / "elsewhere.ckpt"
    shutil.move(saved, moved)
    info = pipeline.checkpoint_info(moved)
    assert info["frame_index"] == CUT and [o["id"] for o in info["objects"]] == before["ids"] and info["color"] is sc.color

    fus = new_fusion(sc.env, sc.size)
    sc.switches(fus)
    fus.load_checkpoint(moved)
    restored = snapshot_volumes(fus, sc.color)
    same(restored, {k: v for k, v in before.items() if k in restored}, "restored")
    rec += [sc.step(fus, f) for f in range(CUT, N)]
    assert rec == want["frames"]
    same(snapshot(fus, sc.color), want["final"], cls.__name__)
    if cls is CleanedUp:
        assert [r["deleted"] for r in rec][3] == [2] and rec[7]["created"] == [3] and rec[-1]["ids"] == [1, 3]
    if cls is Supplied:
        assert all(2 not in r["visible"] for r in rec[3:6]) and 2 in rec[-1]["visible"]
    if sc.pose_log:
        got = results(fus, tmp_path / "resumed")
        same(got, want["files"], "result files")
        assert "poses-1-corrected.txt" in got and "mesh_1.ply" in got
        if cls is CleanedUp:
            assert len(got["mesh_2.ply"]) > 1000  # the mesh kept of the object deleted before the cut
    fus.close()


def snapshot_volumes(fus, color):
    """What a restored session holds before its next frame: volumes, poses, object table (the images are the next
    frame's to make)."""
    s = snapshot(fus, color)
    return {k: v for k, v in s.items() if k in ("ids", "frame_index", "visible") or k.split()[-1] in
            ("tsdf", "weights", "fgbg", "fgprobs", "fgmask", "color", "pose", "info")}


@own_process
def test_saving_in_the_middle_changes_nothing(dev, tmp_path, tmp_path_factory):
    want = uninterrupted(Supplied, tmp_path_factory)
    sc = Supplied()
    fus = start(sc)
    rec = []
    for f in range(N):
        if f in (0, 3, CUT):
            fus.save_checkpoint(tmp_path / "mid.ckpt")
        rec.append(sc.step(fus, f))
    assert rec == want["frames"]
    same(snapshot(fus), want["final"], "after saves")
    fus.close()


@own_process
def test_loading_into_a_used_instance_gives_the_same_continuation(dev, tmp_path, tmp_path_factory):
    want = uninterrupted(Supplied, tmp_path_factory)
    sc = Supplied()
    fus = start(sc)
    for f in range(CUT):
        sc.step(fus, f)
    fus.save_checkpoint(tmp_path / "s.ckpt")
    fus.close()
    # another session's frames first: three objects, five frames of the clean-up stream
    other = CleanedUp()
    fus = start(other)
    for f in range(5):
        other.step(fus, f)
    fus.add_object(np.array([0.3, 0.3, 1.0], np.float32), 0.3)
    fus.set_cleanup(False)
    fus.enable_pose_log(False)
    fus.load_checkpoint(tmp_path / "s.ckpt")
    rec = [sc.step(fus, f) for f in range(CUT, N)]
    assert rec == want["frames"][CUT:]
    same(snapshot(fus), want["final"], "used instance")
    fus.close()


@own_process
def test_records_equal_the_restatement_and_the_file_is_smaller(dev, tmp_path):
    sc = Coloured()
    fus = start(sc)
    for f in range(3):
        sc.step(fus, f)
    vols = {(i, w): fus.volume(name, i) for i in (0, 1, 2)
            for w, name in ((CF.VOL_TSDF, "tsdf"), (CF.VOL_WEIGHTS, "weights"), (CF.VOL_FGBG, "fgbg"), (CF.VOL_COLOR, "color"))
            if i or name != "fgbg"}
    want = {k: PR.pack(v) for k, v in vols.items()}
    raw = sum(v.nbytes for v in vols.values())
    # most of the 64^3 background is never seen: by the reference's own class counts the records are smaller than
    # the buffers (a zero chunk costs one byte, a uniform one five, a literal one 1025, a record 24 + padding)
    counts = np.sum([PR.class_counts(r) for r in want.values()], axis=0)
    assert counts[0] > 0 and counts[0] + 5 * counts[1] + 1025 * counts[2] + 40 * len(want) < raw
    assert sum(len(r) for r in want.values()) < raw
    stats = fus.save_checkpoint(tmp_path / "c.ckpt")
    data = (tmp_path / "c.ckpt").read_bytes()
    got = CF.records(data)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    assert len(data) < raw and stats["raw_bytes"] == raw and stats["file_bytes"] == len(data)
    assert [stats["chunks"][k] for k in ("zero", "uniform", "literal")] == counts.tolist() and stats["records"] == len(want)
    assert all(stats["ms"][k] >= 0 for k in ("classify", "gather", "copy", "file", "total"))
    # the order of the records: background first, then the objects in creation order
    order = [(i, w) for tag, i, w, _, _ in CF.split(data)[1] if tag == b"PACK"]
    assert order == [(0, 0), (0, 1), (0, 5)] + [(i, w) for i in (1, 2) for w in (0, 1, 6, 5)]
    fus.close()


# ---- refusals ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def saved_session(dev, tmp_path_factory):
    if not os.environ.get(CHILD):
        return None  # (the tests that use it run in children, see own_process)
    sc = Supplied()
    fus = start(sc)
    for f in range(3):
        sc.step(fus, f)
    path = tmp_path_factory.mktemp("refusals") / "good.ckpt"
    fus.save_checkpoint(path)
    fus.close()
    return path


def plain_frames(fus, frames, size):
    """Frames of the scene at `size` through an instance with one object of its own; the snapshot after the last."""
    from emfusion_amd.ops import image_view
    if fus.frame_index() == 0 and not fus.object_ids():
        fus.add_object(np.array(SPHERES[1][0], np.float32), 0.5)
    for f in frames:
        depth, ids, R, t = frame(f, (), size)
        d, m = to_dev(depth), to_dev(mask_of(ids, 1))
        fus.process_frame(image_view(d), R, t, {1: (EYE, np.array(SPHERES[1][0], np.float32))}, {1: image_view(m)}, f == 0)
        fus.synchronize()
    return snapshot(fus)


@pytest.mark.parametrize("what", ["frame_size", "bg_res", "truncated"])
@own_process
def test_refused_files_leave_the_session_as_it_was(dev, tmp_path, saved_session, what):
    from emfusion_amd import pipeline
    size = (176, 120) if what == "frame_size" else (W, H)
    kw = dict(bg_res=32, bg_voxel=0.08) if what == "bg_res" else {}
    path = saved_session
    if what == "truncated":
        path = tmp_path / "cut.ckpt"
        path.write_bytes(saved_session.read_bytes()[:-4000])
    fus, twin = new_fusion(size=size, **kw), new_fusion(size=size, **kw)
    plain_frames(fus, (0, 1), size)
    with pytest.raises(pipeline.FusionError) as e:
        fus.load_checkpoint(path)
    assert e.value.code == -4 and fus.frame_index() == 2 and fus.object_ids() == [1]
    plain_frames(twin, (0, 1), size)
    same(plain_frames(fus, (2,), size), plain_frames(twin, (2,), size), what)
    fus.close()
    twin.close()


@own_process
def test_refused_on_the_sharded_path(dev, tmp_path, saved_session):
    """World 2 (local group, one thread per rank): save and load raise on every rank, and the job's next frame equals
    that of a twin job nobody asked."""
    from emfusion_amd import pipeline

    def job(ask):
        comms = pipeline.Communicator.local_group(2)
        out, errors = [None, None], []
        ready = threading.Barrier(2)

        def rank_main(r):
            try:
                fus = new_fusion(comm=comms[r])
                ids = [fus.add_object(np.array(SPHERES[k][0], np.float32), SPHERES[k][2]) for k in (1, 2)]
                mine = [i for i in ids if fus.owns_object(i)]
                ready.wait(timeout=60)
                refused = 0
                from emfusion_amd.ops import image_view
                for f in range(3):
                    if f == 2 and ask:
                        for call in (lambda: fus.load_checkpoint(saved_session),
                                     lambda: fus.save_checkpoint(tmp_path / f"rank{r}.ckpt")):
                            try:
                                call()
                            except pipeline.FusionError as e:
                                refused += e.code == -4
                    depth, ids_img, R, t = frame(f)
                    d = to_dev(depth)
                    fus.process_frame(image_view(d), R, t, {i: (EYE, np.array(SPHERES[i][0], np.float32)) for i in mine},
                                      {}, False)
                    fus.synchronize()
                out[r] = dict(refused=refused, seg=fus.image("segmentation").tobytes(), bg=fus.volume("tsdf", 0).tobytes(),
                              ray=fus.image("raylengths").tobytes(), frame_index=fus.frame_index(), ids=fus.object_ids(),
                              objs={i: fus.volume("tsdf", i).tobytes() for i in mine})
                fus.close()
            except Exception as e:  # noqa: BLE001 - reported by the main thread
                errors.append((r, repr(e)))

        threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
        assert not any(th.is_alive() for th in threads), "a rank hangs"
        assert not errors, errors
        for c in comms:
            c.close()
        return out

    asked, twin = job(True), job(False)
    for r in range(2):
        assert asked[r].pop("refused") == 2 and twin[r].pop("refused") == 0
        assert not (tmp_path / f"rank{r}.ckpt").exists()
        same(asked[r], twin[r], f"rank {r}")
