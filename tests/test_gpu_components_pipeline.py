"""The component filter through the pipeline (Fusion.set_mesh_filter, EMFusion::setMeshFilter): mesh(), meshes(), the
PLY files of write_results and the per-frame meshes equal the restatement's filter (tests/components_reference.py) of
what the same calls return with the filter off and the weld on; mesh_components() and last_mesh_filter() agree with it;
nothing but mesh files changes with the switch; both apps take the two flags.  The kernels themselves:
tests/test_gpu_mesh_components.py.
The scenarios on a Fusion run in tests/components_pipeline_probe.py, a process of their own like the apps (its header
says why); every assertion on them is made there and this file checks that they held."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.components_pipeline_probe import MIN_TRIANGLES
from tests.components_reference import components

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _probe(what, tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "components_pipeline_probe.py"), what, str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "PROBE_RESULT ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]


@pytest.mark.parametrize("color", [False, True])
def test_fusion_switch_filters_meshes_files_and_frame_meshes(dev, tmp_path, color):
    _probe("switch_color" if color else "switch", tmp_path)


def test_filter_changes_no_decision_and_no_image(dev, tmp_path):
    _probe("cleanup", tmp_path)


def _read_ply(path):
    lines = path.read_text().split("\n")
    end = lines.index("end_header")
    nv = int([ln for ln in lines[:end] if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines[:end] if ln.startswith("element face")][0].split()[-1])
    tri = np.array([ln.split() for ln in lines[end + 1 + nv:end + 1 + nv + nf]], np.int64).reshape(nf, 4)
    return nv, tri.astype(np.int32)


def _assert_filtered(path, largest):
    """A filtered file by itself: indexed (fewer vertices than triangles), every vertex used, no component below the
    threshold and, for an object, one component."""
    nv, tri = _read_ply(path)
    assert len(tri) > 200 and nv < len(tri) and tri[:, 1:].min() == 0 and tri[:, 1:].max() == nv - 1
    assert len(np.unique(tri[:, 1:])) == nv
    labels, sizes = components(tri, nv)
    assert sizes.min() >= MIN_TRIANGLES
    if largest:
        assert not labels.any()


def test_synth_app_filters_what_it_writes(dev, tmp_path):
    app = ROOT / "apps" / "emfusion_synth"
    r = subprocess.run([str(app), "--frames", "3", "--objects", "2", "--bg-res", "128", "--obj-res", "32", "--width",
                        "160", "--height", "120", "--export-frame-meshes", "--mesh-min-triangles", str(MIN_TRIANGLES),
                        "--mesh-largest-object", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _assert_filtered(tmp_path / "mesh_bg.ply", False)
    _assert_filtered(tmp_path / "mesh_1.ply", True)
    assert (tmp_path / "frame_meshes" / "bg" / "0002.ply").read_bytes() == (tmp_path / "mesh_bg.ply").read_bytes()


def test_run_tum_filters_what_it_writes(dev, tmp_path):
    from tests import tum_staging as T
    seq_dir, masks, _ = T.stage(tmp_path)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(ROOT / "apps" / "run_tum.py"), seq_dir, "--masks", str(masks),
                        "--out", str(out), "--bg-res", "64", "--bg-voxel", "0.04", "--obj-res", "32",
                        "--visibility-thresh", "100", "--mask-frames", "2", "--export-frame-meshes",
                        "--mesh-min-triangles", str(MIN_TRIANGLES), "--mesh-largest-object"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    _assert_filtered(out / "mesh_bg.ply", False)
    assert (out / "frame_meshes" / "bg" / f"{T.N - 1:04d}.ply").read_bytes() == (out / "mesh_bg.ply").read_bytes()
