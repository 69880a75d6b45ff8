"""--checkpoint / --checkpoint-every / --resume of the two apps on the staged TUM-layout sequence of the driver tests:
N frames in one go against k frames with a checkpoint, then the rest in a fresh process that resumes from it.  Pose
files and tsdfs/ dumps must be the same bytes.  The child processes run one after another, each under a time limit."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
APP = ROOT / "apps" / "emfusion_synth"
CUT = 4  # of the sequence's 6 frames; frame 4 is a mask frame, in the resumed process


def run(cmd):
    p = subprocess.run([str(c) for c in cmd], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def outputs(out: Path):
    files = {p.name: p.read_bytes() for p in sorted(out.glob("poses-*.txt"))}
    files.update({"tsdfs/" + p.name: p.read_bytes() for p in sorted((out / "tsdfs").iterdir())})
    assert "poses-cam.txt" in files and "tsdfs/bg_tsdf.bin" in files
    return files


@pytest.mark.parametrize("app", ["emfusion_synth", "run_tum"])
def test_a_resumed_process_writes_the_results_of_an_uninterrupted_one(tmp_path, dev, app):
    from emfusion_amd import pipeline
    from tests import tum_staging as T
    if app == "emfusion_synth" and not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    seq, masks, _ = T.stage(tmp_path)
    base = ([APP, "--sequence", seq] if app == "emfusion_synth" else [sys.executable, ROOT / "apps" / "run_tum.py", seq])
    base += ["--masks", masks, "--volumes", *T.SMALL]
    whole, first, rest = tmp_path / "whole", tmp_path / "first", tmp_path / "rest"
    ckpt = tmp_path / "session.ckpt"
    run(base + ["--out", whole])
    said = run(base + ["--out", first, "--frames", CUT, "--checkpoint", ckpt, "--checkpoint-every", CUT])
    assert "checkpoint after frame 3" in said
    info = pipeline.checkpoint_info(ckpt)
    assert info["frame_index"] == CUT and info["params"]["bg_res"] == [64, 64, 64] and info["logged_frames"] == CUT
    # the resumed process takes its sizes from the file, not from the command line
    resume = [c for c in base if c not in T.SMALL] if app == "run_tum" else base
    run(resume + ["--out", rest, "--resume", ckpt])
    want, got = outputs(whole), outputs(rest)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    assert len(want["poses-cam.txt"].splitlines()) == T.N
