"""Fusion.distance_field(nearest=True) and Fusion.query_distance on a live session, on the small scenes
of tests/test_gpu_distance_pipeline.py: the index equals tests/nearest_reference.py on the classes the call returns,
byte for byte; nearest=False is what it was; point queries equal a host lookup in the copied arrays; nearest.bin of
write_results and of both apps; the refusals."""
import subprocess
import sys

import numpy as np
import pytest

from tests import distance_reference as dr
from tests import nearest_reference as nr
from tests.test_gpu_distance_pipeline import APP, BG, ROOT, VOX, check, listing, new_session, params, read_volume_file

pytestmark = pytest.mark.gpu
QUERY_BOX = ((3, 5, 2), (58, 50, 50))  # most of the volume: obstacles, and free space farther than the cap from any


@pytest.fixture(scope="module")
def session(dev):
    fus, oid = new_session()
    yield fus, oid
    fus.close()


def check_nearest(fus, got, site_mask=2, cap_voxels=0, key="nearest"):
    """The plain checks of the distance pipeline, then the index against the reference on the returned classes."""
    if key == "nearest":
        check(fus, got, site_mask, cap_voxels)
    d2, near = nr.nearest_separable(dr.sites_of(got["classes"], site_mask), cap_voxels)
    assert got[key].dtype == np.int32 and got[key].shape == got["classes"].shape
    assert got[key].tobytes() == near.tobytes(), (key, int((got[key] != near).sum()))
    return d2, near


def test_whole_background_a_box_and_the_camera_box(session):
    fus, _ = session
    plain = fus.distance_field()
    got = fus.distance_field(nearest=True)
    assert got["box"] == ((0, 0, 0), (BG, BG, BG))
    d2, near = check_nearest(fus, got)
    assert (near >= 0).all() and (near[d2 == 0] == nr.linear_index(d2.shape)[d2 == 0]).all()
    # nearest=False: today's keys and bytes, before and after a call that computed the index
    again = fus.distance_field()
    for other in (plain, again):
        assert set(other) == {"classes", "d2", "metres", "box", "pose", "voxel_size", "objects"}
        for k in ("classes", "d2", "metres"):
            assert other[k].tobytes() == got[k].tobytes()
    assert set(got) == set(plain) | {"nearest"}
    got = fus.distance_field(box=((3, 5, 7), (33, 20, 11)), unknown_is_obstacle=True, cap=0.2, metres=False, nearest=True)
    assert "metres" not in got
    d2, near = check_nearest(fus, got, site_mask=6, cap_voxels=5)
    assert ((near == -1) == (d2 == dr.FAR)).all() and (near >= 0).any() and near.max() < 33 * 20 * 11  # box indices
    got = fus.distance_field(box="camera", size=24, nearest=True)
    assert min(got["box"][1]) < 24  # cut at the volume's near face
    check_nearest(fus, got)


def test_signed(session):
    fus, _ = session
    plain = fus.distance_field(signed=True)
    got = fus.distance_field(signed=True, nearest=True)
    assert set(got) == set(plain) | {"nearest", "nearest_inside"}
    for k in ("classes", "d2", "metres", "d2_inside", "metres_inside", "signed"):
        assert got[k].tobytes() == plain[k].tobytes(), k
    check_nearest(fus, got)
    d2_in, _ = check_nearest(fus, got, site_mask=7 ^ 2, key="nearest_inside")
    assert got["d2_inside"].tobytes() == d2_in.tobytes()


def test_obstacle_offsets(session):
    from emfusion_amd import pipeline
    fus, _ = session
    got = fus.distance_field(box=QUERY_BOX, unknown_is_obstacle=True, cap=0.2, nearest=True)
    off, valid = pipeline.obstacle_offsets(got["nearest"], got["box"][1])
    assert off.shape == (50, 50, 58, 3) and off.dtype == np.int32 and valid.dtype == bool
    assert (valid == (got["d2"] != dr.FAR)).all() and not off[~valid].any() and valid.any() and not valid.all()
    assert ((off.astype(np.int64) ** 2).sum(-1)[valid] == got["d2"][valid]).all()  # the vector has the field's length
    z, y, x = np.nonzero(valid)
    o = off[valid]
    assert (got["classes"][z + o[:, 2], y + o[:, 1], x + o[:, 0]] != dr.FREE).all()  # and ends on an obstacle
    with pytest.raises(ValueError):
        pipeline.obstacle_offsets(got["nearest"], (58, 50, 51))


def world_of(fus, box_lo, vox):
    """Box voxels -> world in float64."""
    R, t = fus.background_pose()
    p = (np.asarray(vox, np.float64) + np.array(box_lo, np.float64) - (BG - 1) / 2.0) * float(np.float32(VOX))
    return p @ R.astype(np.float64).T + t.astype(np.float64)


def test_query_distance_equals_the_host_lookup(session):
    fus, _ = session
    box = QUERY_BOX
    got = fus.distance_field(box=box, unknown_is_obstacle=True, cap=0.2, nearest=True)  # 5 voxels
    assert (got["d2"] == dr.FAR).any()
    size = np.array(box[1])
    rng = np.random.default_rng(2105)
    on_obstacle = np.argwhere(got["d2"] == 0)[:5][:, ::-1]
    far = np.argwhere(got["d2"] == dr.FAR)[:5][:, ::-1]
    vox = np.concatenate([rng.integers(0, size, (40, 3)), on_obstacle, far, [[0, 0, 0], size - 1, [-1, 0, 0], [0, 50, 0],
                          [58, 19, 10], [5, 5, -4], [200, 3, 3]]]).astype(np.int64)
    # off the voxel centres by less than half a voxel: the point rounds to its voxel and is never moved
    jitter = rng.uniform(-0.45, 0.45, vox.shape)
    points = world_of(fus, box[0], vox + jitter)
    q = fus.query_distance(points)
    n = len(vox)
    assert q["voxel"].dtype == np.int32 and q["voxel"].tobytes() == vox.astype(np.int32).tobytes()
    inside = ((vox >= 0) & (vox < size)).all(axis=1)
    assert q["inside"].tolist() == inside.tolist() and inside.sum() == n - 5

    def lookup(a, outside):
        out = np.full(n, outside, a.dtype)
        v = vox[inside]
        out[inside] = a[v[:, 2], v[:, 1], v[:, 0]]
        return out

    want2, want_near = lookup(got["d2"], dr.FAR), lookup(got["nearest"], -1)
    assert q["class"].dtype == np.uint8 and q["class"].tobytes() == lookup(got["classes"], 255).tobytes()
    assert q["d2"].dtype == np.int32 and q["d2"].tobytes() == want2.tobytes()
    assert q["metres"].dtype == np.float32 and q["metres"].tobytes() == dr.metres_of(want2, got["voxel_size"]).tobytes()
    assert q["metres"][inside].tobytes() == lookup(got["metres"], np.float32(np.inf))[inside].tobytes()
    has = want_near >= 0
    assert has.any() and (~has).sum() >= 10 and ((want_near == -1) == (want2 == dr.FAR)).all()
    lin = np.where(has, want_near, 0).astype(np.int64)
    site = np.stack([lin % 58, lin // 58 % 50, lin // (58 * 50)], 1)
    assert q["nearest_voxel"].dtype == np.int32 and q["nearest_voxel"].shape == (n, 3)
    assert q["nearest_voxel"].tobytes() == np.where(has[:, None], site, -1).astype(np.int32).tobytes()
    assert np.isnan(q["nearest_world"][~has]).all() and np.isnan(q["direction"][~has]).all()
    assert np.abs(q["nearest_world"][has] - world_of(fus, box[0], site[has])).max() < 1e-6
    moving = has & (want2 > 0)
    assert np.isnan(q["direction"][has & (want2 == 0)]).all() and (has & (want2 == 0)).sum() >= 5
    step = world_of(fus, box[0], site[moving]) - world_of(fus, box[0], vox[moving])
    unit = step / np.linalg.norm(step, axis=1)[:, None]
    assert q["direction"].dtype == np.float32 and np.abs(q["direction"][moving] - unit).max() < 1e-5
    assert np.abs(np.linalg.norm(step, axis=1) - np.sqrt(want2[moving]) * float(np.float32(VOX))).max() < 1e-6
    # one point, and a field that was not recomputed in between
    one = fus.query_distance(points[3])
    assert one["d2"].tolist() == [int(want2[3])] and one["nearest_voxel"].shape == (1, 3)


def test_query_needs_the_index(session):
    from emfusion_amd import pipeline
    fus, _ = session
    fus.distance_field()  # nearest=False
    with pytest.raises(pipeline.FusionError, match="without the nearest-site index") as err:
        fus.query_distance(np.zeros((2, 3)))
    assert err.value.code == -4
    fus.distance_field(nearest=True)
    assert fus.query_distance(np.zeros((2, 3)))["d2"].shape == (2,)  # and the session stays usable


def test_query_before_any_field_is_refused(dev):
    from emfusion_amd import pipeline
    fus = pipeline.Fusion(params())
    with pytest.raises(pipeline.FusionError, match="no distance field has been computed"):
        fus.query_distance(np.zeros((1, 3)))
    fus.close()


def test_write_results_writes_nearest_bin_only_with_the_switch(dev, tmp_path):
    out = {}
    for name in ("field", "nearest"):
        fus, _ = new_session()
        fus.setup_output(False, False, exp_distance_field=True, distance_cap=0.4, exp_distance_nearest=name == "nearest")
        fus.write_results(tmp_path / name, volumes=False)
        if name == "nearest":
            got = fus.distance_field(cap=0.4, nearest=True)
            with pytest.raises(ValueError):
                fus.setup_output(False, False, exp_distance_nearest=True)
        fus.close()
        out[name] = listing(tmp_path / name)
    assert set(out["nearest"]) - set(out["field"]) == {"nearest.bin"} and set(out["field"]) <= set(out["nearest"])
    assert all(out["nearest"][k] == v for k, v in out["field"].items())
    near, voxel = read_volume_file(tmp_path / "nearest" / "nearest.bin", np.int32)  # checks the element size of the header
    assert voxel == np.float32(VOX) and near.shape == (BG, BG, BG)
    assert near.tobytes() == got["nearest"].tobytes() and (near == -1).any() and (near >= 0).any()


def test_the_apps_write_nearest_bin_and_nothing_else_changes(dev, tmp_path):
    """Both apps: --distance-field --distance-nearest adds exactly nearest.bin, which is the reference's index of the
    run's own occupancy.bin and, on the staged sequence, the Fusion.distance_field(nearest=True) of a session fed the
    same frames in this process; --distance-nearest alone is a usage error before any device is touched."""
    from tests import tum_staging as T
    from tests.test_gpu_voxel_color_app import _python_run
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    seq, masks, _ = T.stage(tmp_path)
    small = ["--frames", "4", "--objects", "1", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    apps = {"synth": [str(APP), *small],
            "tum": [sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", str(masks), *T.SMALL]}
    field = ["--distance-field", "--distance-cap", "0.5"]
    files = {}
    for app, cmd in apps.items():
        p = subprocess.run([*cmd, "--out", str(tmp_path / app / "alone"), "--distance-nearest"], cwd=ROOT, capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 2 and "usage" in p.stderr and "--distance-field" in p.stderr, (app, p.returncode, p.stderr[-500:])
        assert not (tmp_path / app / "alone" / "nearest.bin").exists()
        outs = {}
        for name, extra in (("field", field), ("nearest", field + ["--distance-nearest"])):
            p = subprocess.run([*cmd, "--out", str(tmp_path / app / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
            outs[name] = listing(tmp_path / app / name)
        assert set(outs["nearest"]) - set(outs["field"]) == {"nearest.bin"}, app
        assert all(outs["nearest"][k] == v for k, v in outs["field"].items()) and len(outs["field"]) > 3
        near, voxel = read_volume_file(tmp_path / app / "nearest" / "nearest.bin", np.int32)
        classes, _ = read_volume_file(tmp_path / app / "nearest" / "occupancy.bin", np.uint8)
        cap = int(np.ceil(np.float32(0.5) / np.float32(voxel)))
        assert near.tobytes() == nr.nearest_separable(dr.sites_of(classes, 2), cap)[1].tobytes(), app
        assert (near >= 0).any()
        files[app] = near
    fus = _python_run(T, seq, masks, False)  # the apps' loop on the same frames, kept open
    try:
        got = fus.distance_field(cap=0.5, nearest=True)
        assert files["tum"].tobytes() == got["nearest"].tobytes()
    finally:
        fus.close()


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.distance_field(nearest=True), lambda: fus.query_distance(np.zeros((1, 3)))):
            with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4, -4], [-4, -4]]
