"""Per-frame meshes (setup_output(exp_frame_meshes=True), the reference's --export-frame-meshes): every frame ends by
meshing the background and every shown object in one pass; write_results writes frame_meshes/bg/%04d.ply and
frame_meshes/<id>/%04d.ply, each byte-identical to what write_results would have written as mesh_*.ply after that
frame.  The export changes nothing of the frame path."""
import hashlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FW, FH = 160, 120


def _setup(nobj=2, first=None):
    """Fusion over the synthetic stream; objects k < `first` exist from the start, the others are added later."""
    from emfusion_amd import pipeline
    prm = pipeline.make_params(FW, FH, 64, 0.04, 32, visibility_thresh=100, boundary=5)
    synth = pipeline.SyntheticStream(FW, FH, np.array(prm.K, np.float32), nobj)
    fus = pipeline.Fusion(prm)
    n0 = nobj if first is None else first
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(n0)]
    return synth, fus, ids


def _frame(fus, synth, ids, f, mask_frame):
    from emfusion_amd.ops import image_view
    depth, sid = synth.render(f)
    R, t = synth.camera_pose(f)
    poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(k, f)[0]) for k, i in enumerate(ids)}
    masks = {i: to_dev((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if mask_frame else {}
    fus.process_frame(image_view(to_dev(depth)), R, t, poses, {i: image_view(m) for i, m in masks.items()},
                      mask_frame)


def _files(d):
    d = Path(d)
    return {str(p.relative_to(d)): hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(d.rglob("*"))
            if p.is_file()}


def _run(tmp, frames=6, add_at=None, export=True):
    """Frames with the export on; write_results(tmp/k) after every frame k.  Object 2 is added before frame
    `add_at` when given.  Returns the fusion (open), the ids and the frame each id was added at."""
    synth, fus, ids = _setup(2, first=1 if add_at is not None else None)
    born = {i: 0 for i in ids}
    fus.setup_output(export, False)
    for f in range(frames):
        if f == add_at:
            ids.append(fus.add_object(*[synth.sphere(1, f)[i] for i in (0, 2)]))
            born[ids[-1]] = f
        _frame(fus, synth, ids, f, f in (0, 3) or f == add_at)
        fus.synchronize()
        fus.write_results(str(tmp / str(f)), volumes=False)
    return synth, fus, ids, born


def _check_frames(tmp, frames, born):
    last = tmp / str(frames - 1) / "frame_meshes"
    assert sorted(p.name for p in last.iterdir()) == sorted(["bg"] + [str(i) for i in born])
    assert sorted(p.name for p in (last / "bg").iterdir()) == [f"{f:04d}.ply" for f in range(frames)]
    for i, b in born.items():
        assert sorted(p.name for p in (last / str(i)).iterdir()) == [f"{f:04d}.ply" for f in range(b, frames)]
    for f in range(frames):
        snap = tmp / str(f)
        assert (last / "bg" / f"{f:04d}.ply").read_bytes() == (snap / "mesh_bg.ply").read_bytes(), f
        for i, b in born.items():
            if f >= b:
                assert (last / str(i) / f"{f:04d}.ply").read_bytes() == (snap / f"mesh_{i}.ply").read_bytes(), (f, i)
    # earlier snapshots hold the frames up to theirs, the same bytes
    for f in range(frames):
        snap = _files(tmp / str(f) / "frame_meshes")
        assert sorted(snap) == sorted(k for k in _files(last) if int(k[-8:-4]) <= f)
        assert all(_files(last)[k] == v for k, v in snap.items())


def test_frame_meshes_equal_the_meshes_written_after_each_frame(dev, tmp_path):
    synth, fus, ids, born = _run(tmp_path, frames=6)
    try:
        _check_frames(tmp_path, 6, born)
        assert len(open(tmp_path / "5" / "frame_meshes" / "bg" / "0005.ply").read()) > 1000
        got = fus.meshes()
        assert sorted(got) == [0] + ids
        for i in [0] + ids:
            want = fus.mesh(i)
            for g, w in zip(got[i], want):
                assert g.shape == w.shape and g.tobytes() == w.tobytes(), i
        sub = fus.meshes([ids[-1], 0])
        assert list(sub) == [ids[-1], 0] and sub[0][0].tobytes() == got[0][0].tobytes()
    finally:
        fus.close()
        synth.close()


def test_object_added_mid_run_starts_at_its_frame(dev, tmp_path):
    synth, fus, ids, born = _run(tmp_path, frames=6, add_at=3)
    try:
        assert born == {1: 0, 2: 3}
        _check_frames(tmp_path, 6, born)
    finally:
        fus.close()
        synth.close()


def test_deleted_object_keeps_its_earlier_frames(dev, tmp_path):
    """test_gpu_lifecycle's clean-up scenario: object 2 is reported behind the camera in frame 3 and deleted there."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    Wf, Hf = 320, 240
    prm = pipeline.make_params(Wf, Hf, 128, 0.04, 32, visibility_thresh=400, boundary=10)
    synth = pipeline.SyntheticStream(Wf, Hf, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    fus.set_cleanup(True)
    fus.setup_output(True, False)
    centers, keep = {}, []
    try:
        for f in range(5):
            depth, sid = synth.render(f)
            R, t = synth.camera_pose(f)
            d = to_dev(depth)
            masks = {i: to_dev((sid == i).astype(np.uint8)) for i in centers}
            keep += [d, masks]
            poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), c) for i, c in centers.items()}
            if f == 3:
                poses[2] = (poses[2][0], np.array([0, 0, -30], np.float32))
            if f == 0:
                new = [to_dev((sid == k).astype(np.uint8)) for k in (1, 2)]
                keep.append(new)
                fus.queue_new_object_masks([image_view(m) for m in new])
            fus.process_frame(image_view(d), R, t, poses, {i: image_view(m) for i, m in masks.items()}, True)
            fus.synchronize()
            if f == 0:
                centers = {k: fus.pose(k)[1] for k in (1, 2)}
            if f == 3:
                assert fus.last_deleted() == [2]
                del centers[2]
        fus.write_results(str(tmp_path), volumes=False)
        fm = tmp_path / "frame_meshes"
        assert sorted(p.name for p in (fm / "1").iterdir()) == [f"{f:04d}.ply" for f in range(5)]
        assert sorted(p.name for p in (fm / "2").iterdir()) == [f"{f:04d}.ply" for f in range(3)]
        # the deleted object's last mesh is its last frame's (cleanUpObjs keeps it, EMFusion.cpp:966)
        assert (fm / "2" / "0002.ply").read_bytes() == (tmp_path / "mesh_2.ply").read_bytes()
        assert (fm / "1" / "0004.ply").read_bytes() == (tmp_path / "mesh_1.ply").read_bytes()
    finally:
        fus.close()
        synth.close()


def test_ignore_person_objects_have_no_frame_meshes(dev, tmp_path):
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    Wf, Hf = 320, 240
    prm = pipeline.make_params(Wf, Hf, 128, 0.04, 32, visibility_thresh=400, boundary=10)
    synth = pipeline.SyntheticStream(Wf, Hf, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    fus.set_ignore_person(True)
    fus.setup_output(True, False)
    person = np.zeros(81); person[1] = 0.9; person[57] = 0.1      # COCO: 1 = person, 57 = chair
    chair = np.zeros(81); chair[57] = 0.6; chair[1] = 0.3
    centers, keep = {}, []
    try:
        for f in range(3):
            depth, sid = synth.render(f)
            R, t = synth.camera_pose(f)
            d = to_dev(depth)
            inst = [to_dev((sid == k).astype(np.uint8)) for k in (1, 2)]
            keep += [d, inst]
            fus.queue_instance_masks([image_view(m) for m in inst])
            fus.queue_instance_scores([chair, person])
            poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), c) for i, c in centers.items()}
            fus.process_frame(image_view(d), R, t, poses, {}, False)
            fus.synchronize()
            if f == 0:
                centers = {k: fus.pose(k)[1] for k in (1, 2)}
        assert fus.object_class(1) == 57 and fus.object_class(2) == 1
        fus.write_results(str(tmp_path), volumes=False)
        fm = tmp_path / "frame_meshes"
        assert sorted(p.name for p in fm.iterdir()) == ["1", "bg"]
        assert len(list((fm / "1").iterdir())) == 3 and not (tmp_path / "mesh_2.ply").exists()
    finally:
        fus.close()
        synth.close()


def _state(fus, ids):
    from emfusion_amd.pipeline import IMG

    def dg(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {"pose": [dg(np.concatenate([x.reshape(-1) for x in fus.pose(i)])) for i in [0] + ids]}
    for name in IMG:
        for i in ([0] if name not in ("obj_assoc", "obj_raylengths") else ids):
            out[f"img {name} {i}"] = dg(fus.image(name, i))
    for i in [0] + ids:
        for v in ("tsdf", "weights"):
            out[f"vol {v} {i}"] = dg(fus.volume(v, i))
    return out


def test_export_changes_nothing_of_the_frame_path(dev, tmp_path):
    runs = {}
    for export in (True, False):
        synth, fus, ids = _setup(2)
        fus.setup_output(export, False)
        try:
            for f in range(6):
                _frame(fus, synth, ids, f, f in (0, 3))
            fus.synchronize()
            out = tmp_path / str(export)
            fus.write_results(str(out), volumes=False)
            runs[export] = (_state(fus, ids), {k: v for k, v in _files(out).items()
                                               if not k.startswith("frame_meshes")})
        finally:
            fus.close()
            synth.close()
    assert runs[True][0] == runs[False][0]
    assert runs[True][1] == runs[False][1]  # poses, meshes and the debug-image log (output/, assoc_weights/, ...)
    assert (tmp_path / "True" / "frame_meshes").is_dir() and not (tmp_path / "False" / "frame_meshes").exists()


def test_per_volume_path_writes_the_frame_meshes(dev, tmp_path):
    os.environ["EMF_PER_VOLUME"] = "1"
    try:
        synth, fus, ids, born = _run(tmp_path, frames=4)
    finally:
        os.environ.pop("EMF_PER_VOLUME", None)
    try:
        _check_frames(tmp_path, 4, born)
    finally:
        fus.close()
        synth.close()


def test_sharded_path_refuses_the_export_and_the_next_frame_runs(dev):
    from emfusion_amd import pipeline
    os.environ["EMF_FORCE_SHARDED"] = "1"
    try:
        comm = pipeline.Communicator(pipeline.Communicator.unique_id(), 0, 1)
        prm = pipeline.make_params(FW, FH, 64, 0.04, 32, visibility_thresh=100, boundary=5)
        synth = pipeline.SyntheticStream(FW, FH, np.array(prm.K, np.float32), 1)
        fus = pipeline.Fusion(prm, comm)
        ids = [fus.add_object(*[synth.sphere(0, 0)[i] for i in (0, 2)])]
        try:
            _frame(fus, synth, ids, 0, True)
            with pytest.raises(pipeline.FusionError) as e:
                fus.setup_output(True, False)
            assert e.value.code == -4  # EMF_E_ARG
            _frame(fus, synth, ids, 1, False)
            fus.synchronize()
            assert fus.frame_index() == 2
        finally:
            fus.close()
            synth.close()
            comm.close()
    finally:
        os.environ.pop("EMF_FORCE_SHARDED", None)


def test_synth_app_exports_frame_meshes(dev, tmp_path):
    app = ROOT / "apps" / "emfusion_synth"
    r = subprocess.run([str(app), "--frames", "3", "--objects", "2", "--bg-res", "128", "--obj-res", "32", "--width",
                        "160", "--height", "120", "--export-frame-meshes", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fm = tmp_path / "frame_meshes"
    assert sorted(p.name for p in (fm / "bg").iterdir()) == [f"{f:04d}.ply" for f in range(3)]
    assert (fm / "bg" / "0002.ply").read_bytes() == (tmp_path / "mesh_bg.ply").read_bytes()
    r = subprocess.run([str(app), "--frames", "2", "--export-frame-meshes"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--out" in r.stderr


def test_run_tum_exports_frame_meshes(dev, tmp_path):
    from tests import tum_staging as T
    seq_dir, masks, _ = T.stage(tmp_path)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "apps" / "run_tum.py"), seq_dir, "--masks", str(masks),
                        "--out", str(out), "--bg-res", "64", "--bg-voxel", "0.04", "--obj-res", "32",
                        "--visibility-thresh", "100", "--mask-frames", "2", "--export-frame-meshes"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    fm = out / "frame_meshes"
    assert sorted(p.name for p in (fm / "bg").iterdir()) == [f"{f:04d}.ply" for f in range(T.N)]
    assert (fm / "bg" / f"{T.N - 1:04d}.ply").read_bytes() == (out / "mesh_bg.ply").read_bytes()
    for d in fm.iterdir():
        if d.name != "bg":
            assert (out / f"mesh_{d.name}.ply").exists()
