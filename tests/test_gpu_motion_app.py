"""apps/emfusion_synth --autonomous --motion-masks: the reference's main loop with nothing but depth going in -- no
mask file, no generator masks.  The spheres enter the scene after the first frames, are proposed by the motion masks,
created, tracked and written out as objects."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
APP = ROOT / "apps" / "emfusion_synth"
SMALL = ["--frames", "30", "--objects", "2", "--bg-res", "128", "--obj-res", "32", "--width", "320", "--height", "240"]


def run(*args):
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    return subprocess.run([str(APP), *args], cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_autonomous_run_discovers_objects_from_depth_alone(dev, tmp_path):
    p = run("--autonomous", "--motion-masks", *SMALL, "--mask-frames", "3", "--motion-band", "0.15", "--out", str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "objects spawned from motion masks" in p.stdout, p.stdout
    poses = sorted(q.name for q in tmp_path.glob("poses-[0-9]*.txt") if "corrected" not in q.name)
    meshes = sorted(q.name for q in tmp_path.glob("mesh_[0-9]*.ply"))
    assert poses and meshes, (sorted(q.name for q in tmp_path.iterdir()), p.stdout)
    assert (tmp_path / "poses-cam.txt").exists() and (tmp_path / "mesh_bg.ply").exists()
    assert (tmp_path / meshes[0]).stat().st_size > 1000


def test_motion_masks_and_mask_files_exclude_each_other(tmp_path):
    p = run("--motion-masks", "--masks", str(tmp_path), "--sequence", str(tmp_path), "--out", str(tmp_path))
    assert p.returncode != 0
    assert "usage:" in p.stderr and "--motion-masks" in p.stderr and "--masks" in p.stderr
