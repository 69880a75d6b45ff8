"""Simplified meshes through the pipeline (Fusion.set_mesh_simplify, EMFusion::setMeshSimplify): mesh(), meshes(), the
PLY files of write_results, the per-frame meshes, world_mesh() and the retired slabs equal ops.simplify_mesh of what the
same calls return with the switch off and the weld on; last_mesh_simplify() agrees with the arrays; nothing but mesh
files changes with the switch, a checkpoint included; both apps take --mesh-simplify.  The kernels themselves:
tests/test_gpu_mesh_simplify.py.
The scenarios on a Fusion with objects run in tests/simplify_pipeline_probe.py, a process of their own like the apps;
every assertion on them is made there and this file checks that they held."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.simplify_pipeline_probe import CELL
from tests.simplify_reference import simplify

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


def _probe(what, tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "simplify_pipeline_probe.py"), what, str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "PROBE_RESULT ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]


@pytest.mark.parametrize("color", [False, True])
def test_fusion_switch_simplifies_meshes_files_and_frame_meshes(dev, tmp_path, color):
    _probe("switch_color" if color else "switch", tmp_path)


def test_switch_changes_no_decision_no_image_and_no_checkpoint(dev, tmp_path):
    _probe("cleanup", tmp_path)


def test_world_mesh_and_retired_slabs_are_simplified(dev):
    """--follow-camera --follow-store as a session: the out-and-back walk's roll of frame 6.  world_mesh() with the
    switch on equals ops.simplify_mesh of the welded world mesh with it off; the slabs retired under the switch equal
    ops.simplify_mesh of the welded slabs of a session without it."""
    from emfusion_amd import ops
    from tests import store_reference as sr
    from tests.test_gpu_background_store import frames, new_session
    cell = np.float32(0.09)
    got = {}
    for on in (False, True):
        fus = new_session(touch=lambda f: f.set_mesh_simplify(cell) if on else f.set_mesh_weld(True))
        frames(fus, 0, 7, explicit={6: sr.ROLLS[6]})
        got[on] = dict(slabs=fus.retired_slabs(), world=fus.world_mesh(), info=fus.world_mesh_info())
        if not on:
            fus.set_mesh_simplify(cell)
            got["switched"] = fus.world_mesh()
            fus.set_mesh_simplify(0.0)
            same(fus.world_mesh(), got[on]["world"], "back to 0")
            fus.set_mesh_weld(False)
            same(fus.world_mesh(weld=True), got[on]["world"], "weld=True")
            soup = fus.world_mesh()                                                   # the soup again
            assert len(soup[0]) > len(got[on]["world"][0]) and len(soup[2]) == len(got[on]["world"][2])
        fus.close()
    welded = got[False]["world"]
    assert len(welded[2]) > 1000 and got[False]["info"]["stored_tiles"] > 0
    want = ops.simplify_mesh(*welded, cell=cell)
    same(want, simplify(*welded, cell=cell))
    assert 0 < len(want[0]) < len(welded[0]) / 2
    same(got[True]["world"], want, "world mesh")
    same(got["switched"], want, "switched on later")
    assert got[True]["info"] == got[False]["info"]
    assert len(got[True]["slabs"]) == len(got[False]["slabs"]) > 0
    for a, b in zip(got[True]["slabs"], got[False]["slabs"]):
        assert (a["frame"], a["origin"], a["res"]) == (b["frame"], b["origin"], b["res"])
        if len(b["vertices"]):
            same((a["vertices"], a["normals"], a["triangles"]),
                 ops.simplify_mesh(b["vertices"], b["normals"], b["triangles"], cell=cell), a["origin"])
        else:
            assert len(a["vertices"]) == 0 and len(a["triangles"]) == 0


def _read_ply(path):
    """(vertices (n, 3) as written, triangles (m, 4)) of an ASCII PLY of the project."""
    lines = path.read_text().split("\n")
    end = lines.index("end_header")
    nv = int([ln for ln in lines[:end] if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines[:end] if ln.startswith("element face")][0].split()[-1])
    tri = np.array([ln.split() for ln in lines[end + 1 + nv:end + 1 + nv + nf]], np.int64).reshape(nf, 4)
    return nv, tri.astype(np.int32)


def _assert_simplified(path, plain):
    """A simplified file by itself: indexed, every vertex used, no collapsed triangle, and a fraction of the plain one."""
    nv, tri = _read_ply(path)
    pv, ptri = _read_ply(plain)
    assert 0 < nv < pv / 2 and 0 < len(tri) < len(ptri) / 2, (nv, pv, len(tri), len(ptri))
    assert tri[:, 1:].min() == 0 and tri[:, 1:].max() == nv - 1 and len(np.unique(tri[:, 1:])) == nv
    assert np.all((tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 3]) & (tri[:, 1] != tri[:, 3]))


def test_synth_app_writes_what_the_python_path_writes(dev, tmp_path):
    """emfusion_synth --mesh-simplify against --weld-meshes: the written files are ops.simplify_mesh of the welded
    files' meshes (the switch scenario holds Fusion to the same), and the last frame's mesh is the result file."""
    app = ROOT / "apps" / "emfusion_synth"
    base = [str(app), "--frames", "3", "--objects", "2", "--bg-res", "128", "--obj-res", "32", "--width", "160",
            "--height", "120", "--export-frame-meshes"]
    for name, extra in (("plain", ["--weld-meshes"]), ("simple", ["--mesh-simplify", str(CELL)])):
        (tmp_path / name).mkdir()
        r = subprocess.run(base + extra + ["--out", str(tmp_path / name)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    for f in ("mesh_bg.ply", "mesh_1.ply", "mesh_2.ply"):
        _assert_simplified(tmp_path / "simple" / f, tmp_path / "plain" / f)
    assert (tmp_path / "simple" / "frame_meshes" / "bg" / "0002.ply").read_bytes() == \
        (tmp_path / "simple" / "mesh_bg.ply").read_bytes()
    others = [p.relative_to(tmp_path / "plain") for p in (tmp_path / "plain").rglob("*") if p.is_file() and p.suffix != ".ply"]
    assert others and all((tmp_path / "simple" / p).read_bytes() == (tmp_path / "plain" / p).read_bytes() for p in others)


def test_both_apps_write_the_same_simplified_files(dev, tmp_path):
    """apps/run_tum.py (the Python path: the readers, the C handle API, Fusion.set_mesh_simplify) and
    apps/emfusion_synth --sequence (EMFusion::setMeshSimplify from C++) on the staged TUM sequence, both with
    --mesh-simplify: every mesh file and every other result file the same bytes; against --weld-meshes the meshes are a
    fraction and nothing else differs."""
    from tests import tum_staging as T
    seq, masks, _ = T.stage(tmp_path)
    py = [sys.executable, str(ROOT / "apps" / "run_tum.py"), seq]
    cpp = [str(ROOT / "apps" / "emfusion_synth"), "--sequence", seq]
    common = ["--masks", str(masks), *T.SMALL, "--export-frame-meshes"]
    runs = (("plain", py, ["--weld-meshes"]), ("py", py, ["--mesh-simplify", "0.1"]), ("cpp", cpp, ["--mesh-simplify", "0.1"]))
    for name, head, extra in runs:
        r = subprocess.run(head + common + extra + ["--out", str(tmp_path / name)], cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    files = {name: {str(p.relative_to(tmp_path / name)): p for p in sorted((tmp_path / name).rglob("*")) if p.is_file()}
             for name, _, _ in runs}
    ply = [k for k in files["py"] if k.endswith(".ply")]
    assert "mesh_bg.ply" in ply and "mesh_1.ply" in ply and any(k.startswith("frame_meshes/") for k in ply)
    assert sorted(files["py"]) == sorted(files["plain"])
    assert sorted(k for k in files["cpp"] if k.endswith(".ply")) == sorted(ply)
    for k in ply:
        assert files["cpp"][k].read_bytes() == files["py"][k].read_bytes(), k
    for k in files["py"]:
        if not k.endswith(".ply"):
            assert files["py"][k].read_bytes() == files["plain"][k].read_bytes(), k
    _assert_simplified(files["py"]["mesh_bg.ply"], files["plain"]["mesh_bg.ply"])
    last = f"frame_meshes/bg/{T.N - 1:04d}.ply"
    assert files["py"][last].read_bytes() == files["py"]["mesh_bg.ply"].read_bytes()
