"""bench.py's plain line and --dump-outputs: a plain run times the frames and nothing else, and what its last timed frame
computed is written as float32 .npy files within 64 MB -- the same files with the same values from run to run, so that
two builds of the project can be compared output for output."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_module", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _FakeFusion:
    """The read-backs dump_outputs uses, on volumes and images of the given sizes (values: their flat indices)."""

    def __init__(self, w, h, bg_res, obj_res):
        self.w, self.h, self.bg_res, self.obj_res = w, h, bg_res, obj_res

    def image(self, which, obj_id=0):
        ch = 3 if which in ("vertices", "normals") else 1
        a = np.arange(self.w * self.h * ch, dtype=np.float32).reshape((self.h, self.w, ch) if ch > 1 else (self.h, self.w))
        return (a % 251).astype(np.uint8) if which == "segmentation" else a + obj_id

    def volume(self, which, obj_id=0):
        n = self.bg_res if obj_id == 0 else self.obj_res
        return np.arange(n ** 3, dtype=np.float32).reshape(n, n, n) + obj_id

    def visible_objects(self):
        return [2, 1]


@pytest.mark.parametrize("objects", [0, 4, 64])
def test_dump_stays_within_its_budget_and_is_reproducible(bench, tmp_path, objects):
    ids = list(range(1, objects + 1))
    fus = _FakeFusion(640, 480, 128, 96)
    bench.dump_outputs(fus, ids, tmp_path / "a")
    bench.dump_outputs(fus, ids, tmp_path / "b")
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert len(files) == 9 + 5 * objects and "bg_tsdf.npy" in files and "visible_objects.npy" in files
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= bench.DUMP_BYTES + 256 * len(files)  # + headers
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "visible_objects.npy"), [1, 2])
    tsdf, wts = np.load(tmp_path / "a" / "bg_tsdf.npy"), np.load(tmp_path / "a" / "bg_weights.npy")
    assert 0 < tsdf.size <= bench.DUMP_VOLUME_SAMPLE and np.array_equal(tsdf, wts)  # same voxels of every volume
    assert np.all(np.diff(tsdf) >= 0) and tsdf[-1] > tsdf[0]  # ascending indices spread over the volume
    if objects <= 4:  # the headline's outputs fit whole: images keep their shapes
        assert np.load(tmp_path / "a" / "vertices.npy").shape == (480, 640, 3)


def _run(args, cwd):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--bg-res", "128",
           "--bg-voxel", "0.04", "--obj-res", "32", "--objects-per-gpu", "2", "--width", "320", "--height", "240"] + args
    p = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_its_outputs(dev, tmp_path):
    d = _run(["--dump-outputs", str(tmp_path / "a")], tmp_path)
    assert d["metric"] == "frames/sec (integrate+raycast+EM-assoc)" and d["unit"] == "frames/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["steps"] == 5 and d["warmup"] == 2
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1.0
    for key in ("roofline", "kernels", "hbm_copy_GBs", "cpu_baseline", "target_config", "steady_state", "entry_point",
                "strong_scaling"):
        assert key not in d, key  # --full's
    d2 = _run(["--dump-outputs", str(tmp_path / "b")], tmp_path)
    assert d2["config"]["visible_objects_last_frame"] == d["config"]["visible_objects_last_frame"] > 0
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and len(files) == 9 + 5 * 2
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64 << 20
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.shape == b.shape, f
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=f)
    assert (np.load(tmp_path / "a" / "bg_weights.npy") > 0).any()  # the sample reaches integrated voxels
