"""Fusion.object_shapes on a live session: the 64^3 background of the other *_pipeline tests with two
sphere objects and a few frames.  Every record equals tests/shape_reference.py applied to Fusion.volume("tsdf" /
"weights" / "fgmask", id): integers and extents as bytes, frame, box and world corners as the restatement's float64
exactly; an unknown id raises; background=True adds slot 0; the session and its next frame are those of a twin that
never asked; shapes.txt appears with the switch and only with it, in write_results and in both apps; a sharded session
refuses."""
import subprocess
import sys

import numpy as np
import pytest

from tests import shape_reference as sr
from tests.test_gpu_frontier_pipeline import APP, H, ROOT, W, listing, params

pytestmark = pytest.mark.gpu


def feed(fus, synth, oids, f):
    from emfusion_amd import devmem, ops
    depth, sid = synth.render(f)
    R, t = synth.camera_pose(f)
    masks = {oid: devmem.DeviceArray.from_numpy((sid == k + 1).astype(np.uint8)) for k, oid in enumerate(oids)} if f == 0 else {}
    d_depth = devmem.DeviceArray.from_numpy(depth)
    poses = {oid: (np.eye(3, dtype=np.float32), synth.sphere(k, f)[0]) for k, oid in enumerate(oids)}
    fus.process_frame(ops.image_view(d_depth), R, t, poses, {i: ops.image_view(m) for i, m in masks.items()}, f == 0)
    fus.synchronize()


def open_session(frames=3):
    """Two moving spheres in front of the synthetic background, each with a volume of its own."""
    from emfusion_amd import pipeline
    prm = params()
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), 2)
    fus = pipeline.Fusion(prm)
    oids = []
    for k in range(2):
        c, _, vs = synth.sphere(k, 0)
        oids.append(fus.add_object(c, vs))
    for f in range(frames):
        feed(fus, synth, oids, f)
    return fus, oids, synth


@pytest.fixture(scope="module")
def session(dev):
    fus, oids, synth = open_session()
    synth.close()
    yield fus, oids
    fus.close()


def snapshot(fus, oids):
    out = [fus.volume("tsdf", 0), fus.volume("weights", 0), *fus.pose(0), *fus.background_pose()]
    for oid in oids:
        out += [fus.volume("tsdf", oid), fus.volume("weights", oid), fus.volume("fgmask", oid), *fus.pose(oid)]
    return out


def check_record(fus, got, oid):
    """One record of object_shapes() against the restatement on the volumes the session hands out."""
    tsdf, weights = fus.volume("tsdf", oid), fus.volume("weights", oid)
    fg = fus.volume("fgmask", oid) if oid else None
    res = tsdf.shape[::-1]
    mom = sr.moments(tsdf, weights, fg)
    assert got["id"] == oid and got["res"] == res
    assert got["moments"].dtype == sr.MOMENTS and got["moments"].tobytes() == mom.tobytes(), (oid, got["moments"], mom)
    assert (got["solid"], got["observed"], got["faces_free"], got["faces_unknown"]) == \
        (int(mom["solid"]), int(mom["observed"]), int(mom["faces_free"]), int(mom["faces_unknown"]))
    assert (got["bounds_vox"][0] == mom["lo"]).all() and (got["bounds_vox"][1] == mom["hi"]).all()
    fr = sr.frame(mom)
    assert got["frame"].tobytes() == fr.tobytes() and got["valid"] == bool(fr["valid"])
    if not got["valid"]:
        assert got["centroid_vox"] is None and got["box_corners_world"] is None
        return mom
    ext = sr.extents(tsdf, weights, fg, fr["f32"])
    assert got["extents"].tobytes() == ext.tobytes(), (oid, got["extents"], ext)
    R, t = fus.pose(oid) if oid else fus.background_pose()
    assert got["pose"][0].tobytes() == R.tobytes() and got["pose"][1].tobytes() == t.tobytes()
    vs = fus.object_info(oid)["voxel_size"] if oid else got["voxel_size"]
    assert got["voxel_size"] == vs
    box = sr.box(mom, fr, ext, res, vs, R, t)
    assert got["box"].tobytes() == box.tobytes(), (oid, got["box"], box)
    for key, want in (("centroid_vox", fr["centroid"]), ("axes", fr["axes"].reshape(3, 3)), ("eigenvalues", fr["eigenvalues"]),
                      ("box_center_vox", box["center_vox"]), ("box_half_vox", box["half_vox"]), ("box_center", box["center_obj"]),
                      ("box_half", box["half_m"]), ("box_corners", box["corners_obj"].reshape(8, 3)),
                      ("box_center_world", box["center_world"]), ("box_axes_world", box["axes_world"].reshape(3, 3)),
                      ("box_corners_world", box["corners_world"].reshape(8, 3))):
        assert got[key].dtype == np.float64 and got[key].tobytes() == np.ascontiguousarray(want).tobytes(), key
    assert got["extents_vox"][0].tobytes() == ext["lo"].tobytes() and got["extents_vox"][1].tobytes() == ext["hi"].tobytes()
    assert got["completeness"] == float(box["completeness"]) or np.isnan(box["completeness"])
    return mom


def test_object_shapes_equal_the_reference(session):
    fus, oids = session
    before = snapshot(fus, oids)
    got = fus.object_shapes()
    assert [r["id"] for r in got] == oids == fus.object_ids()
    for r, oid in zip(got, oids):
        mom = check_record(fus, r, oid)
        # the spheres have been seen from one side: a band, some of it against free space, some against the unseen
        assert r["valid"] and 0 < r["solid"] < r["observed"] and r["faces_free"] > 0 and r["faces_unknown"] > 0
        assert 0.0 < r["completeness"] < 1.0 and int(mom["solid"]) < np.prod(r["res"]) // 4
        # the box holds the sphere's visible cap: it lies inside the object's volume and has a positive size
        assert (r["box_half"] > 0).all() and (np.abs(r["box_center"]) < 0.5 * r["voxel_size"] * np.array(r["res"])).all()
    again = fus.object_shapes(ids=oids[::-1])
    assert [r["id"] for r in again] == oids[::-1]
    assert all(a["moments"].tobytes() == b["moments"].tobytes() and a["box"].tobytes() == b["box"].tobytes()
               for a, b in zip(again[::-1], got))
    one = fus.object_shapes(ids=[oids[1]])
    assert len(one) == 1 and one[0]["box"].tobytes() == got[1]["box"].tobytes()
    assert fus.object_shapes(ids=[]) == []
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, snapshot(fus, oids)))  # nothing of the session changed


def test_background_adds_slot_zero(session):
    fus, oids = session
    got = fus.object_shapes(background=True)
    assert [r["id"] for r in got] == [0] + oids
    mom = check_record(fus, got[0], 0)
    assert int(mom["solid"]) > 0 and got[0]["res"] == (64, 64, 64)
    for r, oid in zip(got[1:], oids):
        check_record(fus, r, oid)
    only = fus.object_shapes(ids=[], background=True)
    assert len(only) == 1 and only[0]["moments"].tobytes() == got[0]["moments"].tobytes()


def test_an_unknown_id_raises(session):
    from emfusion_amd import pipeline
    fus, oids = session
    for bad in ([max(oids) + 7], [oids[0], 0], [-1]):
        with pytest.raises(pipeline.FusionError) as err:
            fus.object_shapes(ids=bad)
        assert err.value.code == -4, bad


def test_an_empty_object_is_a_record_without_a_frame(dev):
    """An object volume behind the camera, which no frame fuses anything into: valid False, the neutral integer record."""
    from emfusion_amd import devmem, ops, pipeline
    prm = params()
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), 1)
    fus = pipeline.Fusion(prm)
    try:
        c, _, vs = synth.sphere(0, 0)
        seen = fus.add_object(c, vs)
        behind = np.array([0.0, 0.0, -3.0], np.float32)
        empty = fus.add_object(behind, vs)
        for f in range(2):
            depth, sid = synth.render(f)
            R, t = synth.camera_pose(f)
            masks = {seen: devmem.DeviceArray.from_numpy((sid == 1).astype(np.uint8))} if f == 0 else {}
            d_depth = devmem.DeviceArray.from_numpy(depth)
            poses = {seen: (np.eye(3, dtype=np.float32), synth.sphere(0, f)[0]), empty: (np.eye(3, dtype=np.float32), behind)}
            fus.process_frame(ops.image_view(d_depth), R, t, poses, {i: ops.image_view(m) for i, m in masks.items()}, f == 0)
            fus.synchronize()
        assert not (fus.volume("weights", empty) > 0).any()
        first, r = fus.object_shapes(ids=[seen, empty])
        check_record(fus, first, seen)
        check_record(fus, r, empty)
        assert first["valid"] and not r["valid"] and r["solid"] == 0 and r["observed"] == 0 and r["box_center_world"] is None
        assert tuple(r["bounds_vox"][0]) == r["res"] and tuple(r["bounds_vox"][1]) == (-1, -1, -1)
        assert np.isnan(r["completeness"]) and np.isposinf(r["extents"]["lo"]).all() and np.isneginf(r["extents"]["hi"]).all()
    finally:
        synth.close()
        fus.close()


def test_the_next_frame_is_that_of_a_session_that_never_asked(dev):
    out = []
    for ask in (False, True):
        fus, oids, synth = open_session()
        if ask:
            fus.object_shapes(background=True)
            fus.object_shapes(ids=oids[:1])
        feed(fus, synth, oids, 3)
        synth.close()
        out.append(snapshot(fus, oids) + [fus.image("segmentation"), fus.image("bg_raylengths")])
        fus.close()
    assert len(out[0]) == len(out[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(*out))


def read_shapes(path):
    lines = path.read_text().splitlines()
    assert lines[0].startswith("# id valid solid observed faces_free faces_unknown") and "not the body" in lines[0]
    rows = [line.split() for line in lines[1:]]
    assert all(len(r) == 12 + 15 for r in rows)
    return [([int(v) for v in r[:12]], [float(v) for v in r[12:]]) for r in rows]


def test_write_results_writes_the_file_only_with_the_switch(dev, tmp_path):
    out = {}
    for on in (False, True):
        fus, oids, synth = open_session()
        synth.close()
        fus.setup_output(False, False, exp_object_shapes=on)
        fus.write_results(tmp_path / str(on), volumes=False)
        if on:
            shapes = fus.object_shapes()
        fus.close()
        out[on] = listing(tmp_path / str(on))
    assert set(out[True]) - set(out[False]) == {"shapes.txt"} and set(out[False]) <= set(out[True])
    assert all(out[True][k] == v for k, v in out[False].items())  # every other file byte for byte
    rows = read_shapes(tmp_path / "True" / "shapes.txt")
    assert [r[0][0] for r in rows] == sorted(s["id"] for s in shapes)
    for (ints, floats), s in zip(rows, sorted(shapes, key=lambda s: s["id"])):
        assert ints == [s["id"], int(s["valid"]), s["solid"], s["observed"], s["faces_free"], s["faces_unknown"],
                        *s["bounds_vox"][0].tolist(), *s["bounds_vox"][1].tolist()]
        want = [*s["box_center_world"], *s["box_half"], *s["box_axes_world"].reshape(-1)]
        assert floats == [float("%.9g" % v) for v in want]


def test_the_apps_write_the_file_only_with_the_switch(dev, tmp_path):
    from tests import tum_staging as T
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    seq, masks, _ = T.stage(tmp_path)
    small = ["--frames", "4", "--objects", "2", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    apps = {"synth": [str(APP), *small],
            "tum": [sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", str(masks), *T.SMALL]}
    for app, cmd in apps.items():
        outs = {}
        for name, extra in (("plain", []), ("shapes", ["--object-shapes"])):
            p = subprocess.run([*cmd, "--out", str(tmp_path / app / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
            outs[name] = listing(tmp_path / app / name)
        assert set(outs["shapes"]) - set(outs["plain"]) == {"shapes.txt"} and len(outs["plain"]) > 2, app
        assert all(outs["shapes"][k] == v for k, v in outs["plain"].items()), app
        rows = read_shapes(tmp_path / app / "shapes" / "shapes.txt")
        ids = [r[0][0] for r in rows]
        assert ids == sorted(ids) and len(set(ids)) == len(ids), app
        assert (any(r[0][1] == 1 and r[0][2] > 0 for r in rows) if app == "synth" else all(r[0][2] >= r[0][1] for r in rows)), app


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.object_shapes(), lambda: fus.object_shapes(ids=[], background=True)):
            with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4] * 2, [-4] * 2]
