"""Fusion.planes on a live session: the 64^3 background with one object the frontier pipeline test
uses.  planes() equals tests/planes_reference.py applied to Fusion.volume("tsdf", 0) / "weights" byte for byte -- the
counters, the records, the labels and every plane's float64 bits -- over the whole background and over a camera box;
with up_hint towards the camera the wall in front of it is the floor; ground_map(up="floor") equals ground_map(up=that
normal) byte for byte; planes.txt appears only with the switch, from Python and from apps/emfusion_synth, and no other
result byte changes; the sharded path refuses; a checkpoint written after the calls equals one written without them
and nothing of the session changes."""
import math

import numpy as np
import pytest

from tests import planes_reference as pr
from tests.test_gpu_frontier_pipeline import BG, VOX, new_session, params
from tests.test_gpu_ground_pipeline import WALL

pytestmark = pytest.mark.gpu
TO_CAMERA = (0.0, 0.0, -1.0)


@pytest.fixture(scope="module")
def session(dev):
    fus, oid = new_session()
    yield fus, oid
    fus.close()


def check(fus, got, **kw):
    """got = fus.planes(labels=True, **kw) against the restatement on the volumes the session reports."""
    tsdf, weights = fus.volume("tsdf", 0), fus.volume("weights", 0)
    lo, size = got["box"]
    planes, rec, labels = pr.find_planes(tsdf, weights, (lo, size), K=kw.get("k", 15), angle=kw.get("angle", 20.0),
                                         separation=kw.get("separation"), bin_vox=kw.get("bin") or 1.0,
                                         band=2.0 if kw.get("band") is None else kw["band"], min_votes=kw.get("min_votes"),
                                         refine=kw.get("refine", 1), max_planes=kw.get("max_planes", 64))
    counts = pr.records(tsdf, weights, (lo, size))[1]
    assert got["counters"] == (counts[0], counts[1], counts[1], 0) and counts[1] == len(rec) < 65536
    assert got["min_votes"] == (kw["min_votes"] if kw.get("min_votes") else max(50, len(rec) // 200))
    assert got["records"].tobytes() == rec.tobytes()
    volume = np.full(size[0] * size[1] * size[2], -1, np.int16)
    volume[rec["index"]] = labels
    assert got["labels"].dtype == np.int16 and got["labels"].shape == (size[2], size[1], size[0])
    assert got["labels"].tobytes() == volume.tobytes()
    assert len(got["planes"]) == len(planes)
    bg_R, bg_t = fus.background_pose()
    vs = float(np.float32(VOX))
    for g, w in zip(got["planes"], planes):
        assert g["normal_voxel"].tobytes() == np.array(w["n"]).tobytes() and g["d_voxel"] == w["d"], (g, w)
        assert g["count"] == w["count"] and g["bounds"] == (tuple(w["lo"]), tuple(w["hi"])) and g["label"] == w["label"]
        assert g["thickness_m"] == w["thickness"] * vs
        # the world frame: the normal through the background's rotation, the centroid through the box's world mapping
        n = bg_R.astype(np.float64) @ np.array(w["n"])
        assert np.abs(g["normal"] - n).max() < 1e-15 and abs(np.linalg.norm(g["normal"]) - 1.0) < 1e-9
        if w["fitted"]:  # QueryBox::worldPoint in Python floats, as bits
            R, t = [[float(v) for v in row] for row in bg_R], [float(v) for v in bg_t]
            p = [(w["centroid"][j] + (float(lo[j]) - (float(BG) - 1.0) / 2.0)) * vs for j in range(3)]
            want_point = [((R[i][0] * p[0] + R[i][1] * p[1]) + R[i][2] * p[2]) + t[i] for i in range(3)]
            assert g["point"].tobytes() == np.array(want_point, np.float64).tobytes()
        assert abs(g["d"] - float(np.dot(g["normal"], g["point"]))) < 1e-12
        assert g["area_m2"] == w["count"] * (vs * vs) / np.abs(w["n"]).max()
    return planes


def test_planes_equal_the_restatement(session):
    fus, _ = session
    got = fus.planes(labels=True)
    planes = check(fus, got)
    assert len(planes) >= 1 and planes[0]["count"] > 500
    # the synthetic wall z = 2.2 + 0.15 x - 0.1 y is among them, its normal within the seed's bound of the truth
    truth = np.array((0.15, -0.1, -1.0)) / np.linalg.norm((0.15, -0.1, -1.0))
    angles = [math.degrees(math.acos(min(1.0, float(np.dot(truth, p["normal"]))))) for p in got["planes"]]
    print("planes:", [(p["count"], np.round(p["normal"], 4).tolist(), round(p["d"], 4), p["kind"]) for p in got["planes"]], angles)
    assert min(angles) < math.degrees(math.atan(math.sqrt(2.0) / 15))
    for kw in (dict(k=16, angle=30.0, min_votes=20, refine=0), dict(k=31, bin=2.0, band=1.0, separation=40.0, refine=2, max_planes=2)):
        check(fus, fus.planes(labels=True, **kw), **kw)


def test_a_camera_box(session):
    fus, _ = session
    got = fus.planes(box="camera", size=(40, 33, 128), labels=True, min_votes=20)
    assert got["box"] == fus.camera_box((40, 33, 128)) and got["box"][1] != (BG, BG, BG)
    assert len(check(fus, got, min_votes=20)) >= 1


def test_the_wall_is_the_floor_when_up_points_at_the_camera(session):
    fus, _ = session
    got = fus.planes(up_hint=TO_CAMERA)
    assert got["floor"] is not None
    floor = got["planes"][got["floor"]]
    assert floor["kind"] == "floor" and float(np.dot(floor["normal"], TO_CAMERA)) > math.cos(math.radians(30.0))
    assert [p["kind"] for p in got["planes"]].count("floor") == 1
    # floor and kinds are those of the restatement, for this hint, the default one and one that no plane faces
    bg_R, _ = fus.background_pose()
    for hint in (TO_CAMERA, None, (1.0, 0.0, 0.0)):
        res = fus.planes(up_hint=hint)
        up = list(-bg_R[:, 1].astype(np.float64)) if hint is None else list(hint)
        heights = [float(np.dot(p["point"], up)) for p in res["planes"]]
        want = pr.kinds([list(p["normal"]) for p in res["planes"]], heights, up)
        assert (res["floor"], [p["kind"] for p in res["planes"]]) == want, hint
    assert res["floor"] is None
    wall = dict(WALL)
    del wall["up"]
    a = fus.ground_map(up="floor", up_hint=TO_CAMERA, **wall)
    b = fus.ground_map(up=floor["normal"], **wall)
    assert a["up"].tobytes() == np.asarray(floor["normal"], np.float64).tobytes()
    for key in ("classes", "cells", "height_m", "ground_pose"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["frame"][0].tobytes() == b["frame"][0].tobytes() and a["frame"][1:] == b["frame"][1:]
    assert (a["floor"] >= 0).sum() > 100
    with pytest.raises(ValueError, match="finds no floor"):
        fus.ground_map(up="floor", up_hint=(1.0, 0.0, 0.0), **wall)
    with pytest.raises(ValueError, match='None or "floor"'):
        fus.ground_map(up="ceiling", **wall)


def test_bad_arguments_are_refused(session):
    from emfusion_amd import pipeline
    fus, _ = session
    for kw in (dict(k=0), dict(k=32), dict(angle=0.0), dict(angle=91.0), dict(bin=0.0), dict(band=-1.0), dict(refine=-1),
               dict(max_planes=0), dict(max_planes=65), dict(box=((0, 0, 0), (65, 8, 8))), dict(bin=0.01)):
        with pytest.raises(pipeline.FusionError) as err:
            fus.planes(**kw)
        assert err.value.code in (-4, -5), kw


def test_nothing_of_the_session_changes(session):
    fus, oid = session
    before = [fus.volume(k, i).tobytes() for i in (0, oid) for k in ("tsdf", "weights")]
    df = fus.distance_field(metres=False)
    fus.planes(labels=True)
    fus.planes(box="camera", size=32, up_hint=TO_CAMERA)
    assert [fus.volume(k, i).tobytes() for i in (0, oid) for k in ("tsdf", "weights")] == before
    again = fus.distance_field(metres=False)
    assert again["classes"].tobytes() == df["classes"].tobytes() and again["d2"].tobytes() == df["d2"].tobytes()


def test_a_checkpoint_after_the_calls_equals_one_without_them(dev, tmp_path):
    files = []
    for ask in (False, True):
        fus, oid = new_session()
        if ask:
            fus.planes(labels=True)
            fus.ground_map(up="floor", up_hint=TO_CAMERA, band=WALL["band"])
        fus.save_checkpoint(tmp_path / f"{ask}.ckpt")
        fus.close()
        files.append((tmp_path / f"{ask}.ckpt").read_bytes())
    assert files[0] == files[1] and len(files[0]) > 1000


def read_planes(path):
    lines = path.read_text().splitlines()
    assert lines[0].startswith("# kind count normal_world(3) d point_world(3) thickness_m lo(3) hi(3)")
    rows = [line.split() for line in lines[1:]]
    assert all(len(r) == 16 for r in rows)
    return rows


def check_planes_file(rows, got):
    """The lines of planes.txt against what planes() returns: %.9g of the float64 values, integers exactly."""
    assert len(rows) == len(got["planes"]) >= 1
    for r, p in zip(rows, got["planes"]):
        assert r[0] == p["kind"] and int(r[1]) == p["count"]
        want = list(p["normal"]) + [p["d"]] + list(p["point"]) + [p["thickness_m"]]
        assert r[2:10] == ["%.9g" % v for v in want], (r, want)
        assert [int(v) for v in r[10:]] == list(p["bounds"][0]) + list(p["bounds"][1])


def test_write_results_writes_planes_txt_only_with_the_switch(dev, tmp_path):
    from tests.test_gpu_ground_pipeline import digest
    out = {}
    for name, kw in (("off", {}), ("on", dict(exp_planes=True)), ("votes", dict(exp_planes=True, planes_angle=30.0, planes_min_votes=20))):
        fus, _ = new_session()
        fus.setup_output(False, False, **kw)
        fus.write_results(tmp_path / name, volumes=False)
        if kw:
            args = dict(angle=kw["planes_angle"], min_votes=kw["planes_min_votes"]) if "planes_angle" in kw else {}
            check_planes_file(read_planes(tmp_path / name / "planes.txt"), fus.planes(**args))
        fus.close()
        out[name] = digest(tmp_path / name)
    for name in ("on", "votes"):
        assert set(out[name]) - set(out["off"]) == {"planes.txt"} and set(out["off"]) <= set(out[name])
        assert all(out[name][k] == v for k, v in out["off"].items()) and len(out["off"]) >= 3


def test_ground_up_floor_in_the_results(dev, tmp_path):
    """setup_output(ground_up="floor"): with the default hint the scene of this session holds no floor in view, so
    write_results fails with the message; nothing but the string is accepted."""
    from emfusion_amd import pipeline
    fus, _ = new_session()
    with pytest.raises(ValueError, match='None or "floor"'):
        fus.setup_output(False, False, exp_ground_map=True, ground_up="wall")
    has_floor = fus.planes()["floor"] is not None
    fus.setup_output(False, False, exp_ground_map=True, ground_up="floor", ground_band=WALL["band"])
    if has_floor:
        fus.write_results(tmp_path / "floor", volumes=False)
        want = fus.ground_map(up="floor", band=WALL["band"])
        raw = (tmp_path / "floor" / "ground.bin").read_bytes()
        assert raw[:want["classes"].size] == want["classes"].tobytes()
    else:
        with pytest.raises(pipeline.FusionError, match="the plane search finds no floor"):
            fus.write_results(tmp_path / "floor", volumes=False)
    fus.close()


def test_the_app_writes_planes_txt_and_nothing_else_changes(dev, tmp_path):
    """apps/emfusion_synth on its synthetic stream: with --planes the results gain planes.txt and no other byte changes;
    the parameters alone, or an angle outside (0, 90], are a usage error; --ground-up floor is accepted."""
    import subprocess
    from tests.test_gpu_frontier_pipeline import APP, ROOT
    from tests.test_gpu_ground_pipeline import digest
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    small = [str(APP), "--frames", "4", "--objects", "1", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    outs = {}
    for name, extra in (("plain", []), ("planes", ["--planes", "--planes-angle", "25", "--planes-min-votes", "30"])):
        p = subprocess.run([*small, "--out", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name] = digest(tmp_path / name)
    assert set(outs["planes"]) - set(outs["plain"]) == {"planes.txt"}
    assert all(outs["planes"][k] == v for k, v in outs["plain"].items()) and len(outs["plain"]) > 3
    rows = read_planes(tmp_path / "planes" / "planes.txt")
    assert len(rows) >= 1 and int(rows[0][1]) > 500 and {r[0] for r in rows} <= {"floor", "level", "ceiling", "wall", "slope"}
    assert all(abs(sum(float(v) ** 2 for v in r[2:5]) - 1.0) < 1e-6 for r in rows)
    for bad in (["--planes-angle", "25"], ["--planes", "--planes-angle", "0"], ["--planes-min-votes", "3"]):
        p = subprocess.run([*small, "--out", str(tmp_path / "bad"), *bad], cwd=ROOT, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--planes" in p.stderr
    p = subprocess.run([*small, "--out", str(tmp_path / "floor"), "--ground-map", "--ground-up", "floor", "--ground-band", "-3.0,0.2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and (tmp_path / "floor" / "ground.txt").exists() or "finds no floor" in p.stdout + p.stderr, p.stderr[-800:]


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        with pytest.raises(pipeline.FusionError, match="the plane search is not supported on the sharded path") as err:
            fus.planes()
        ready.wait(timeout=JOIN_S)
        fus.close()
        return err.value.code

    assert list(run_ranks(2, body)) == [-4, -4]
