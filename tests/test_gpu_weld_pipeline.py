"""Welded meshes through the pipeline (Fusion.set_mesh_weld, EMFusion::setMeshWeld): mesh(), meshes(), the PLY files of
write_results and the per-frame meshes equal the numpy restatement's weld (tests/weld_reference.py) of the same calls
with the switch off, nothing else changes with the switch, and both apps take --weld-meshes.  The kernels themselves:
tests/test_gpu_mesh_weld.py."""
import hashlib
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.parity_util import to_dev
from tests.weld_reference import edge_keys, weld

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


FW, FH = 160, 120


def _setup(color=False):
    """The frame-mesh tests' scene: a 64^3 background and two 32^3 objects over the synthetic stream."""
    from emfusion_amd import pipeline
    prm = pipeline.make_params(FW, FH, 64, 0.04, 32, visibility_thresh=100, boundary=5)
    synth = pipeline.SyntheticStream(FW, FH, np.array(prm.K, np.float32), 2)
    fus = pipeline.Fusion(prm)
    if color:
        fus.enable_color()
    ids = [fus.add_object(*[synth.sphere(k, 0)[i] for i in (0, 2)]) for k in range(2)]
    return synth, fus, ids


def _frame(fus, synth, ids, f, mask_frame, color=False):
    from emfusion_amd.ops import image_view
    depth, sid = synth.render(f)
    R, t = synth.camera_pose(f)
    poses = {i: (np.eye(3, dtype=np.float32).reshape(-1), synth.sphere(k, f)[0]) for k, i in enumerate(ids)}
    masks = {i: to_dev((sid == k + 1).astype(np.uint8)) for k, i in enumerate(ids)} if mask_frame else {}
    keep = [to_dev(depth)]
    if color:
        keep.append(to_dev(np.random.default_rng(0xC0105 + f).integers(0, 256, (FH, FW, 3), dtype=np.uint8)))
        fus.set_color_image(image_view(keep[1]))
    fus.process_frame(image_view(keep[0]), R, t, poses, {i: image_view(m) for i, m in masks.items()}, mask_frame)
    fus.synchronize()


def _fusion_keys(fus, i):
    return edge_keys(fus.volume("tsdf", i), fus.volume("weights", i), None if i == 0 else fus.volume("fgmask", i))


def _ply_bytes(tmp, mesh):
    from emfusion_amd import pipeline
    p = tmp / "expected.ply"
    pipeline.write_mesh(p, *mesh[:3], colors=mesh[3] if len(mesh) > 3 else None)
    return p.read_bytes()


@pytest.mark.parametrize("color", [False, True])
def test_fusion_switch_welds_meshes_files_and_frame_meshes(dev, tmp_path, color):
    synth, fus, ids = _setup(color)
    try:
        fus.setup_output(True, False)
        fus.set_mesh_weld(True)
        for f in range(3):
            _frame(fus, synth, ids, f, f == 0, color)
        welded_all = fus.meshes(colors=color)
        welded_one = {i: fus.mesh(i, colors=color) for i in [0] + ids}
        fus.write_results(str(tmp_path / "on"), volumes=False)
        fus.set_mesh_weld(False)
        soup_all = fus.meshes(colors=color)
        for i in [0] + ids:
            soup = fus.mesh(i, colors=color)
            same(soup_all[i], soup, i)
            keys = _fusion_keys(fus, i)
            assert len(keys) == len(soup[0]) > 100
            want = weld(*soup[:3], keys, *soup[3:])
            same(welded_one[i], want, i)
            same(welded_all[i], want, i)
            assert len(want[0]) < len(soup[0])
            if color:
                assert want[3].any()
            name = "mesh_bg.ply" if i == 0 else f"mesh_{i}.ply"
            frame = tmp_path / "on" / "frame_meshes" / ("bg" if i == 0 else str(i)) / "0002.ply"
            expected = _ply_bytes(tmp_path, want)
            assert (tmp_path / "on" / name).read_bytes() == expected, i
            assert frame.read_bytes() == expected, i
    finally:
        fus.close()
        synth.close()


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _files(d):
    return {str(p.relative_to(d)): hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(Path(d).rglob("*"))
            if p.is_file()}


def _cleanup_run(tmp, weld_on):
    """The frame-mesh tests' clean-up scenario: object 2 is reported behind the camera in frame 3 and deleted there."""
    from emfusion_amd import pipeline
    from emfusion_amd.ops import image_view
    Wf, Hf = 320, 240
    prm = pipeline.make_params(Wf, Hf, 128, 0.04, 32, visibility_thresh=400, boundary=10)
    synth = pipeline.SyntheticStream(Wf, Hf, np.array(prm.K, np.float32), 2, seed=0xE3F5)
    fus = pipeline.Fusion(prm, None)
    fus.set_cleanup(True)
    fus.set_mesh_weld(weld_on)
    fus.setup_output(True, False)
    centers, keep, log = {}, [], []
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
                del centers[2]
            live = fus.object_ids()
            log.append((live, fus.last_deleted(), [_digest(np.concatenate([x.reshape(-1) for x in fus.pose(i)]))
                                                  for i in [0] + live],
                        [_digest(fus.volume(v, i)) for i in [0] + live for v in ("tsdf", "weights")]))
        fus.write_results(str(tmp), volumes=False)
        return log, _files(tmp)
    finally:
        fus.close()
        synth.close()


def test_switch_changes_no_decision_and_no_image(dev, tmp_path):
    off_log, off_files = _cleanup_run(tmp_path / "off", False)
    on_log, on_files = _cleanup_run(tmp_path / "on", True)
    assert off_log[3][1] == [2] and off_log[4][0] == [1]      # the scenario happened
    assert on_log == off_log                                   # poses, object_ids(), last_deleted(), volumes
    assert sorted(on_files) == sorted(off_files)
    ply = {k for k in on_files if k.endswith(".ply")}
    assert {k for k in on_files if on_files[k] != off_files[k]} <= ply   # poses-*.txt and every image log: same bytes
    assert any(k.endswith(".png") for k in on_files)
    assert on_files["mesh_bg.ply"] != off_files["mesh_bg.ply"] and on_files["mesh_1.ply"] != off_files["mesh_1.ply"]
    # the deleted object's last mesh is the soup the life cycle took (EMFusion::setMeshWeld)
    assert on_files["mesh_2.ply"] == off_files["mesh_2.ply"]


def _ply_counts(path):
    lines = path.read_text().split("\n")
    end = lines.index("end_header")
    nv = int([ln for ln in lines[:end] if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines[:end] if ln.startswith("element face")][0].split()[-1])
    tri = np.array([ln.split() for ln in lines[end + 1 + nv:end + 1 + nv + nf]], np.int64)
    return nv, nf, tri


def _assert_welded(path):
    """A soup has more vertices than triangles (every cube brings its own: 3 for 1 triangle ... 12 for 5); a welded
    surface has about half as many."""
    nv, nf, tri = _ply_counts(path)
    assert nf > 200 and nv < nf and tri[:, 1:].max() == nv - 1 and tri[:, 1:].min() == 0
    assert len(np.unique(tri[:, 1:])) == nv


def test_synth_app_welds_what_it_writes(dev, tmp_path):
    app = ROOT / "apps" / "emfusion_synth"
    r = subprocess.run([str(app), "--frames", "3", "--objects", "2", "--bg-res", "128", "--obj-res", "32", "--width",
                        "160", "--height", "120", "--export-frame-meshes", "--weld-meshes", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _assert_welded(tmp_path / "mesh_bg.ply")
    assert (tmp_path / "frame_meshes" / "bg" / "0002.ply").read_bytes() == (tmp_path / "mesh_bg.ply").read_bytes()


def test_run_tum_welds_what_it_writes(dev, tmp_path):
    from tests import tum_staging as T
    seq_dir, masks, _ = T.stage(tmp_path)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "apps" / "run_tum.py"), seq_dir, "--masks", str(masks),
                        "--out", str(out), "--bg-res", "64", "--bg-voxel", "0.04", "--obj-res", "32",
                        "--visibility-thresh", "100", "--mask-frames", "2", "--export-frame-meshes", "--weld-meshes"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    _assert_welded(out / "mesh_bg.ply")
    assert (out / "frame_meshes" / "bg" / f"{T.N - 1:04d}.ply").read_bytes() == (out / "mesh_bg.ply").read_bytes()
