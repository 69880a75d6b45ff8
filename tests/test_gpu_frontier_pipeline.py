"""Fusion.frontiers on a live session: a 64^3 background with one object for a few frames.  The
clusters equal tests/frontier_reference.py applied to the classes of tests/distance_reference.py on Fusion.volume(...)
and to the classes Fusion.distance_field() reports for the same box, byte for byte; boxes, the clearance, exclude, a
roll, the label volume, the world points, the outputs of write_results and of apps/emfusion_synth, and the refusal on
a sharded session."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import distance_reference as dr
from tests import frontier_reference as fr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
APP = ROOT / "apps" / "emfusion_synth"
W, H, BG, VOX, OBJ = 160, 120, 64, 0.04, 32


def params():
    from emfusion_amd import pipeline
    return pipeline.make_params(W, H, BG, VOX, OBJ, visibility_thresh=100, boundary=5)


def feed(fus, synth, oid, f):
    from emfusion_amd import devmem, ops
    depth, sid = synth.render(f)
    R, t = synth.camera_pose(f)
    masks = {oid: devmem.DeviceArray.from_numpy((sid == 1).astype(np.uint8))} if f == 0 else {}
    d_depth = devmem.DeviceArray.from_numpy(depth)
    fus.process_frame(ops.image_view(d_depth), R, t, {oid: (np.eye(3, dtype=np.float32), synth.sphere(0, f)[0])},
                      {i: ops.image_view(m) for i, m in masks.items()}, f == 0)
    fus.synchronize()


def open_session(frames=3):
    """The scene of the entry point's smoke run: one moving sphere in front of the synthetic background."""
    from emfusion_amd import pipeline
    prm = params()
    synth = pipeline.SyntheticStream(W, H, np.array(prm.K, np.float32), 1)
    fus = pipeline.Fusion(prm)
    c, _, vs = synth.sphere(0, 0)
    oid = fus.add_object(c, vs)
    for f in range(frames):
        feed(fus, synth, oid, f)
    return fus, oid, synth


def new_session(frames=3):
    fus, oid, synth = open_session(frames)
    synth.close()
    return fus, oid


@pytest.fixture(scope="module")
def session(dev):
    fus, oid = new_session()
    yield fus, oid
    fus.close()


def clearance_voxels(metres):
    return int(np.ceil(np.float32(metres) / np.float32(VOX))) if metres > 0 else 0


def check(fus, got, min_voxels=8, clearance=0.0, exclude=()):
    """got against the restatement on the classes of the same box: those Fusion.distance_field() reports and those
    tests/distance_reference.py forms from Fusion.volume(...).  Returns (classes, labels, kept in session order)."""
    df = fus.distance_field(box=got["box"], exclude=exclude, metres=False)
    tsdf, wts = fus.volume("tsdf", 0), fus.volume("weights", 0)
    objs = [(fus.volume("tsdf", i), fus.volume("weights", i), fus.volume("fgmask", i), fus.object_info(i)["voxel_size"], R, t)
            for i, R, t in df["objects"]]
    classes = dr.stamp(dr.classes_of(tsdf, wts, got["box"]), tsdf.shape[::-1], got["voxel_size"], got["box"], objs)
    assert df["classes"].tobytes() == classes.tobytes() and df["box"] == got["box"]
    cv = clearance_voxels(clearance)
    d2 = dr.distance_transform(classes, 1 << dr.OCCUPIED, cv) if cv else None
    labels, kept, counts = fr.frontiers(classes, d2, cv * cv, min_voxels)
    want = fr.session_order(kept)
    assert (got["kept"], got["n_clusters"], got["n_voxels"]) == counts
    assert got["records"].tobytes() == want.tobytes()
    assert [c["label"] for c in got["clusters"]] == want["label"].tolist()
    for c, r in zip(got["clusters"], want):
        assert (c["count"], c["lo"], c["hi"], c["sum"], c["rep"]) == \
            (int(r["count"]), tuple(r["lo"].tolist()), tuple(r["hi"].tolist()), tuple(r["sum"].tolist()), tuple(r["rep"].tolist()))
        assert labels[c["rep"][2], c["rep"][1], c["rep"][0]] == c["label"]  # a voxel of the cluster, one to go to
    counts_sorted = [c["count"] for c in got["clusters"]]
    assert counts_sorted == sorted(counts_sorted, reverse=True) and all(c >= min_voxels for c in counts_sorted)
    if "labels" in got:
        assert got["labels"].dtype == np.int32 and got["labels"].tobytes() == labels.tobytes()
    # the world points: the numpy float64 formula, within one float32 ulp (the integers they come from are exact;
    # only the last rounding may differ where the order of the float64 operations does)
    R, t = fus.background_pose()
    centroid, rep = fr.world_points(want, got["box"][0], (BG, BG, BG), np.float32(VOX), R, t)
    for a, b in ((got["centroid_world"], centroid), (got["rep_world"], rep)):
        assert a.dtype == np.float32 and a.shape == b.shape == (len(want), 3)
        assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))).all()
    for k, c in enumerate(got["clusters"]):
        assert c["rep_world"].tobytes() == got["rep_world"][k].tobytes() and c["centroid_world"].tobytes() == got["centroid_world"][k].tobytes()
    return classes, labels, want


def box_pose(fus, lo):
    """The background's pose composed with the box origin, in float64."""
    R, t = fus.background_pose()
    corner = (np.array(lo, np.float64) - (BG - 1) / 2.0) * float(np.float32(VOX))
    return R, t.astype(np.float64) + R.astype(np.float64) @ corner


def test_whole_background_equals_the_reference(session):
    fus, oid = session
    before = (fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.pose(0), fus.pose(oid), fus.background_pose())
    got = fus.frontiers(labels=True)
    assert got["box"] == ((0, 0, 0), (BG, BG, BG)) and got["labels"].shape == (BG, BG, BG) and got["voxel_size"] == float(np.float32(VOX))
    classes, labels, want = check(fus, got)
    assert got["n_voxels"] > 500 and got["kept"] >= 1 and got["n_clusters"] >= got["kept"]  # the scene does have a frontier
    assert (classes[labels >= 0] == dr.FREE).all()
    Rp, tp = got["box_pose"]
    wR, wt = box_pose(fus, (0, 0, 0))
    assert Rp.tobytes() == wR.tobytes() and np.abs(tp - wt).max() < 1e-5
    # every kept cluster's representative, taken through the reported box pose, is its rep_world
    for c in got["clusters"]:
        p = Rp.astype(np.float64) @ (np.array(c["rep"], np.float64) * float(np.float32(VOX))) + tp.astype(np.float64)
        assert np.abs(p - c["rep_world"]).max() < 1e-4
    # min_voxels: 1 keeps every cluster
    every = fus.frontiers(min_voxels=1)
    check(fus, every, min_voxels=1)
    assert every["kept"] == every["n_clusters"] == got["n_clusters"] and every["n_voxels"] == got["n_voxels"]
    # nothing of the session changed, and a second call gives the same
    after = (fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.pose(0), fus.pose(oid), fus.background_pose())
    for a, b in zip(before, after):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) if isinstance(a, tuple) else a.tobytes() == b.tobytes()
    again = fus.frontiers(labels=True)
    assert again["records"].tobytes() == got["records"].tobytes() and again["labels"].tobytes() == got["labels"].tobytes()


def test_boxes(session):
    fus, _ = session
    got = fus.frontiers(box=((3, 5, 7), (33, 20, 11)), min_voxels=2, labels=True)
    assert got["box"] == ((3, 5, 7), (33, 20, 11)) and got["labels"].shape == (11, 20, 33)
    check(fus, got, min_voxels=2)
    wR, wt = box_pose(fus, (3, 5, 7))
    assert np.abs(got["box_pose"][1] - wt).max() < 1e-5
    got = fus.frontiers(box="camera", size=24, min_voxels=1, labels=True)
    assert got["box"] == fus.camera_box(24) and min(got["box"][1]) < 24  # cut at the volume's near face
    check(fus, got, min_voxels=1)
    from emfusion_amd import pipeline
    with pytest.raises(pipeline.FusionError) as err:
        fus.frontiers(box=((40, 0, 0), (25, 8, 8)))
    assert err.value.code == -4
    with pytest.raises(pipeline.FusionError) as err:
        fus.frontiers(min_voxels=0)
    assert err.value.code == -4
    with pytest.raises(ValueError):
        fus.frontiers(box="camera")


def test_clearance_of_two_voxels(session):
    fus, _ = session
    plain = fus.frontiers(min_voxels=1)
    got = fus.frontiers(min_voxels=1, clearance=0.07, labels=True)  # rounded up to two voxels
    assert clearance_voxels(0.07) == 2
    check(fus, got, min_voxels=1, clearance=0.07)
    assert 0 < got["n_voxels"] < plain["n_voxels"]  # the gate does drop the frontier next to the surface
    # the distance field of the session is not touched by it
    df = fus.distance_field()
    fus.frontiers(clearance=0.07)
    again = np.empty_like(df["d2"])
    from emfusion_amd.pipeline import _check, load
    _check("emf_fusion_copy_distance_field", load().emf_fusion_copy_distance_field(fus._h, None, again.ctypes.data, None))
    assert again.tobytes() == df["d2"].tobytes()


def test_exclude_removes_the_objects_voxels(session):
    fus, oid = session
    got = fus.frontiers(min_voxels=1, exclude=[oid], labels=True)
    classes, _, _ = check(fus, got, min_voxels=1, exclude=[oid])
    assert classes.tobytes() == dr.classes_of(fus.volume("tsdf", 0), fus.volume("weights", 0)).tobytes()


def test_follows_a_roll(dev):
    fus, oid = new_session()
    before = fus.frontiers(min_voxels=1, labels=True)
    shift = (8, 0, -8)
    fus.roll_background(shift, keep_retired=False)
    got = fus.frontiers(min_voxels=1, labels=True)
    check(fus, got, min_voxels=1)
    wR, wt = box_pose(fus, (0, 0, 0))
    assert np.abs(got["box_pose"][1] - wt).max() < 1e-5
    moved = got["box_pose"][1].astype(np.float64) - before["box_pose"][1].astype(np.float64)
    assert np.abs(moved - got["box_pose"][0].astype(np.float64) @ (np.array(shift) * float(np.float32(VOX)))).max() < 1e-5
    # voxel v now holds what v + shift held: away from the faces of the box and from the slabs that rolled in as
    # unknown, a frontier voxel is a frontier voxel still
    inner_before = before["labels"][2:55, 1:63, 9:62] >= 0
    inner_after = got["labels"][10:63, 1:63, 1:54] >= 0
    assert inner_before.any() and (inner_before == inner_after).all()
    fus.close()


def test_the_next_frame_is_that_of_a_session_that_never_asked(dev):
    out = []
    for ask in (False, True):
        fus, oid, synth = open_session()
        if ask:
            fus.frontiers(min_voxels=1, clearance=0.07, labels=True)
            fus.frontiers(box="camera", size=24)
        feed(fus, synth, oid, 3)
        synth.close()
        out.append([fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.volume("weights", oid),
                    *fus.pose(0), *fus.pose(oid), *fus.background_pose()])
        fus.close()
    assert len(out[0]) == len(out[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(*out))


def listing(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(Path(root).rglob("*")) if p.is_file()}


def read_frontiers(path):
    lines = Path(path).read_text().splitlines()
    assert lines[0].startswith("# count rep_x rep_y rep_z centroid_x centroid_y centroid_z lo_x")
    rows = [line.split() for line in lines[1:]]
    assert all(len(r) == 13 for r in rows)
    return ([int(r[0]) for r in rows], np.array([[np.float32(v) for v in r[1:4]] for r in rows], np.float32).reshape(-1, 3),
            np.array([[np.float32(v) for v in r[4:7]] for r in rows], np.float32).reshape(-1, 3), [[int(v) for v in r[7:]] for r in rows])


def one_ulp(a, b):
    return (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))).all()


def test_write_results_writes_the_file_only_with_the_switch(dev, tmp_path):
    out = {}
    for on in (False, True):
        fus, _ = new_session()
        if on:
            fus.setup_output(False, False, exp_frontiers=True, frontier_min_voxels=3, frontier_clearance=0.07)
        else:
            fus.setup_output(False, False)
        fus.write_results(tmp_path / str(on), volumes=False)
        if on:
            got = fus.frontiers(min_voxels=3, clearance=0.07)
            check(fus, got, min_voxels=3, clearance=0.07)
        fus.close()
        out[on] = listing(tmp_path / str(on))
    assert set(out[True]) - set(out[False]) == {"frontiers.txt"} and set(out[False]) <= set(out[True])
    assert all(out[True][k] == v for k, v in out[False].items())
    counts, rep, centroid, boxes = read_frontiers(tmp_path / "True" / "frontiers.txt")
    assert counts == [c["count"] for c in got["clusters"]] and len(counts) == got["kept"] >= 1
    assert boxes == [list(c["lo"]) + list(c["hi"]) for c in got["clusters"]]
    assert one_ulp(rep, got["rep_world"]) and one_ulp(centroid, got["centroid_world"])


def test_the_app_writes_the_file_and_nothing_else_changes(dev, tmp_path):
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    small = ["--frames", "4", "--objects", "1", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    outs = {}
    for name, extra in (("plain", []), ("frontiers", ["--frontiers", "--frontier-min-voxels", "4", "--frontier-clearance", "0.05"])):
        p = subprocess.run([str(APP), *small, "--out", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name] = listing(tmp_path / name)
    assert set(outs["frontiers"]) - set(outs["plain"]) == {"frontiers.txt"}
    assert all(outs["frontiers"][k] == v for k, v in outs["plain"].items()) and len(outs["plain"]) > 3
    counts, rep, centroid, boxes = read_frontiers(tmp_path / "frontiers" / "frontiers.txt")
    assert len(counts) >= 1 and counts == sorted(counts, reverse=True) and min(counts) >= 4
    assert all(0 <= b[i] <= b[i + 3] < 64 for b in boxes for i in range(3))
    assert np.isfinite(rep).all() and np.isfinite(centroid).all()


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
            fus.frontiers()
        code = err.value.code
        ready.wait(timeout=JOIN_S)
        fus.close()
        return code

    assert list(run_ranks(2, body)) == [-4, -4]
