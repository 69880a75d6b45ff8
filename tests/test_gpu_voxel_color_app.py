"""--color end to end: apps/emfusion_synth --sequence on a staged TUM-layout scene with RGB PNGs writes PLYs whose colours
are Fusion.mesh_colors of the same run driven from Python, colour volumes in the dump, and unchanged files otherwise; the
refusals (synthetic stream, sharded job, per-volume path) say why."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.test_color_io import encode_png

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
APP = ROOT / "apps" / "emfusion_synth"


def _stage_with_colour(tmp_path):
    from tests import tum_staging as T
    seq, masks, _ = T.stage(tmp_path)
    (Path(seq) / "rgb").mkdir()
    rng = np.random.default_rng(0xC0105)
    images = []
    for f in range(T.N):
        # smooth colours (so that neighbouring voxels agree and a mesh shows them) + noise; RGBA on odd frames
        yy, xx = np.mgrid[0:T.H, 0:T.W]
        img = np.stack([xx * 255 // (T.W - 1), yy * 255 // (T.H - 1), (xx + yy + 10 * f) % 256], -1).astype(np.int64)
        img = np.clip(img + rng.integers(-8, 9, img.shape), 0, 255).astype(np.uint8)
        images.append(img)
        out = img if f % 2 == 0 else np.concatenate([img, np.full((T.H, T.W, 1), 200, np.uint8)], -1)
        (Path(seq) / "rgb" / f"{f:04d}.png").write_bytes(encode_png(out, filters=np.arange(T.H) % 5))
    return T, seq, masks, images


def _ply(path):
    lines = path.read_text().split("\n")
    end = lines.index("end_header")
    nv = int([ln for ln in lines[:end] if ln.startswith("element vertex")][0].split()[-1])
    has_colour = "property uchar red" in lines[:end]
    rows = [ln.split() for ln in lines[end + 1:end + 1 + nv]]
    return nv, has_colour, rows


def _python_run(T, seq, masks, color):
    """apps/run_tum.py's loop, kept open so that the meshes can be asked for."""
    from emfusion_amd import pipeline, readers
    from emfusion_amd.devmem import DeviceArray
    from emfusion_amd.ops import image_view
    reader = readers.TUMReader(seq)
    prm = pipeline.make_params(T.W, T.H, 64, 0.04, 32, visibility_thresh=100, boundary=int(round(20 * T.W / 640.0)),
                               mask_frames=T.MASK_EVERY)
    fus = pipeline.Fusion(prm, None)
    if color:
        fus.enable_color()
    fus.set_preprocess(True)
    fus.set_cleanup(True)
    fus.setup_output(False, True)
    eye, zero = np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)
    for f in range(len(reader)):
        depth = np.ascontiguousarray(reader.depth(f), np.float32)
        keep = [DeviceArray.from_numpy(depth)]
        if f % prm.mask_frames == 0:
            _, ms, scores = readers.load_preprocessed_masks(Path(masks) / f"Mask{f:04d}.plk")
            dm = [DeviceArray.from_numpy(m) for m in ms]
            keep += dm
            fus.queue_instance_masks([image_view(m) for m in dm])
            fus.queue_instance_scores(scores)
        if color:
            keep.append(DeviceArray.from_numpy(reader.color(f)))
            fus.set_color_image(image_view(keep[-1]))
        if f == 1:
            fus.set_tracking(camera=True, objects=True)
        fus.process_frame(image_view(keep[0]), eye, zero, {}, {}, False)
        fus.synchronize()
    return fus


def test_sequence_with_colour_writes_coloured_plys(dev, tmp_path):
    T, seq, masks, images = _stage_with_colour(tmp_path)
    outs = {}
    for name, extra in (("plain", []), ("colour", ["--color"])):
        outs[name] = tmp_path / ("out_" + name)
        p = subprocess.run([str(APP), "--sequence", seq, "--masks", masks, "--out", str(outs[name]), "--volumes", *extra,
                            *T.SMALL], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    # colour changes nothing else: poses, volumes and the geometry columns of the PLYs
    for f in sorted(outs["plain"].glob("poses-*.txt")):
        assert (outs["colour"] / f.name).read_bytes() == f.read_bytes(), f.name
    for f in sorted((outs["plain"] / "tsdfs").glob("*.bin")):
        assert (outs["colour"] / "tsdfs" / f.name).read_bytes() == f.read_bytes(), f.name
    assert not list((outs["plain"] / "tsdfs").glob("*color*"))
    plys = sorted(f.name for f in outs["plain"].glob("mesh_*.ply"))
    assert "mesh_bg.ply" in plys and len(plys) >= 2 and plys == sorted(f.name for f in outs["colour"].glob("mesh_*.ply"))
    fus = _python_run(T, seq, masks, True)
    try:
        live, checked = [0] + fus.object_ids(), 0
        for name in plys:
            nv0, c0, rows0 = _ply(outs["plain"] / name)
            nv1, c1, rows1 = _ply(outs["colour"] / name)
            assert not c0 and c1 and nv0 == nv1 and nv1 > 100, name
            assert [r[:6] for r in rows1] == rows0, name
            who = 0 if name == "mesh_bg.ply" else int(name[5:-4])
            if who not in live:
                continue  # an object the clean-up deleted: its last mesh is in the file, the model is gone
            checked += 1
            want = fus.mesh_colors(who)
            got = np.array([r[6:9] for r in rows1], np.int64)
            assert got.shape == want.shape and np.array_equal(got, want), name
            assert len(np.unique(got, axis=0)) > 20, name  # a textured model, not a constant
            # ... and the colour volume of the dump is the run's
            dump = (outs["colour"] / "tsdfs" / ("bg_color.bin" if who == 0 else f"color_{who}.bin")).read_bytes()
            vol = fus.volume("color", who)
            assert np.frombuffer(dump[:12], np.int32).tolist() == list(vol.shape[2::-1])
            assert int(np.frombuffer(dump[12:20], np.uint64)[0]) == 8
            assert dump[24:] == vol.tobytes(), name
        assert checked >= 2  # the background and at least one live object
        assert (fus.volume("color", 0)[..., 3] > 0).sum() > 1000
    finally:
        fus.close()


def test_color_is_refused_where_it_cannot_work(dev, tmp_path):
    p = subprocess.run([str(APP), "--frames", "2", "--color"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "the synthetic stream has none" in p.stderr
    from emfusion_amd import pipeline
    prm = pipeline.make_params(160, 120, 64, 0.04, 32)
    for env, what in (("EMF_FORCE_SHARDED", "sharded path"), ("EMF_PER_VOLUME", "per-volume path")):
        os.environ[env] = "1"
        comm = None
        try:
            if env == "EMF_FORCE_SHARDED":
                comm = pipeline.Communicator(pipeline.Communicator.unique_id(), 0, 1)
            fus = pipeline.Fusion(prm, comm)
            with pytest.raises(pipeline.FusionError, match="not supported on the " + what) as e:
                fus.enable_color()
            assert e.value.code != 0
            fus.close()
        finally:
            os.environ.pop(env, None)
            if comm is not None:
                comm.close()


def test_python_driver_takes_color(dev, tmp_path):
    T, seq, masks, _ = _stage_with_colour(tmp_path)
    out = tmp_path / "out_py"
    q = subprocess.run([sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", masks, "--out", str(out),
                        "--color", *T.SMALL], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert q.returncode == 0, q.stdout[-1500:] + q.stderr[-1500:]
    nv, has_colour, rows = _ply(out / "mesh_bg.ply")
    assert has_colour and nv > 100 and len({tuple(r[6:9]) for r in rows}) > 20
