"""Fusion.plan on a live session: the 64^3 background with one object the frontier pipeline test uses.
The cost field and the paths equal tests/plan_reference.py applied to the classes Fusion.distance_field() reports for
the same box and exclude list, with the same start voxels, radius and clearance, byte for byte; the metric length and
the world points equal the float64 formula; explicit goals, the camera box, through_unknown, the outputs of
write_results and of both apps, and the refusal on a sharded session."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import distance_reference as dr
from tests import plan_reference as pl
from tests.test_gpu_frontier_pipeline import APP, BG, ROOT, VOX, listing, new_session, one_ulp, params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session(dev):
    fus, oid = new_session()
    yield fus, oid
    fus.close()


def voxels_of(metres):
    return int(np.ceil(np.float32(metres) / np.float32(VOX))) if metres > 0 else 0


def world_of(fus, box_lo, vox):
    """Box voxels in the world frame: the float64 formula of the frontiers' world points, rounded once."""
    R, t = fus.background_pose()
    p = (np.asarray(vox, np.float64) + np.asarray(box_lo, np.float64) - (BG - 1) / 2.0) * np.float64(np.float32(VOX))
    return (p @ R.astype(np.float64).T + t.astype(np.float64)).astype(np.float32)


def check(fus, got, clearance=0.0, through_unknown=False, exclude=(), radius=None, max_cost=0):
    """got against the restatement on the classes Fusion.distance_field() reports for the same box.  Returns
    (classes, cost)."""
    df = fus.distance_field(box=got["box"], exclude=exclude, metres=False)
    classes = df["classes"]
    cv = voxels_of(clearance)
    assert got["clearance_voxels"] == cv and got["start_radius_voxels"] == (max(cv, 1) if radius is None else radius)
    d2 = dr.distance_transform(classes, 1 << dr.OCCUPIED, cv) if cv else None
    seeds = got["start_voxels"]
    cost, (finite, used) = pl.cost_field(classes, seeds, d2=d2, min_d2=cv * cv, mask=5 if through_unknown else 1,
                                         radius=got["start_radius_voxels"], max_cost=max_cost)
    assert got["converged"] and got["rounds"] >= 1 and (got["n_finite"], got["n_starts"]) == (finite, used)
    if "cost" in got:
        assert got["cost"].dtype == np.uint32 and got["cost"].tobytes() == cost.tobytes()
    goals = [g["voxel"] for g in got["goals"]]
    nz, ny, nx = cost.shape
    if goals:
        _, lengths, goal_cost = pl.paths(cost, goals, 0)
        paths, _, _ = pl.paths(cost, goals, int(lengths.max(initial=0)))
    vs = np.float64(np.float32(VOX))
    for k, g in enumerate(got["goals"]):
        assert g["reachable"] == bool(lengths[k] > 0) and g["cost"] == int(goal_cost[k])
        lin = paths[k, :lengths[k]].astype(np.int64)
        vox = np.stack([lin % nx, lin // nx % ny, lin // (nx * ny)], axis=1).astype(np.int32)
        assert g["path_vox"].dtype == np.int32 and g["path_vox"].tobytes() == vox.tobytes()
        f, e, c = pl.step_counts(lin, cost.shape) if len(lin) else (0, 0, 0)
        assert g["steps"] == (f, e, c) and 3 * f + 4 * e + 5 * c == (g["cost"] if g["reachable"] else 0)
        assert g["length_m"] == (f + np.sqrt(2.0) * e + np.sqrt(3.0) * c) * vs
        assert g["path_world"].dtype == np.float32 and g["path_world"].tobytes() == world_of(fus, got["box"][0], vox).tobytes()
        if g["reachable"]:
            assert tuple(vox[0]) == g["voxel"] and cost[vox[-1][2], vox[-1][1], vox[-1][0]] == 0
    return classes, cost


def test_plan_to_the_frontiers_equals_the_reference(session):
    fus, oid = session
    before = (fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.pose(0), fus.pose(oid), fus.background_pose())
    got = fus.plan(field=True)
    assert got["box"] == ((0, 0, 0), (BG, BG, BG)) and got["cost"].shape == (BG, BG, BG)
    classes, cost = check(fus, got)
    # the start is the voxel under the camera, and the field is 0 there
    cam = fus.camera_box(1)[0]
    assert tuple(got["start_voxels"][0]) == cam and got["cost"][cam[2], cam[1], cam[0]] == 0 and got["n_starts"] == 1
    # the goals are the kept clusters' representatives: reachable first, cheapest first, the rest in frontier order
    fr = fus.frontiers()
    assert sorted(g["label"] for g in got["clusters"]) == sorted(c["label"] for c in fr["clusters"]) and len(fr["clusters"]) >= 2
    assert all(g["voxel"] == g["rep"] for g in got["clusters"]) and got["clusters"] is got["goals"]
    order = {c["label"]: k for k, c in enumerate(fr["clusters"])}
    keys = [(not g["reachable"], g["cost"] if g["reachable"] else 0, order[g["label"]]) for g in got["clusters"]]
    assert keys == sorted(keys) and any(g["reachable"] for g in got["clusters"])
    for g in got["clusters"]:  # with the same clearance a representative is in T by construction
        assert cost[g["rep"][2], g["rep"][1], g["rep"][0]] != pl.BLOCKED
    # nothing of the session changed, and a second call gives the same
    after = (fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.pose(0), fus.pose(oid), fus.background_pose())
    for a, b in zip(before, after):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) if isinstance(a, tuple) else a.tobytes() == b.tobytes()
    again = fus.plan(field=True)
    assert again["cost"].tobytes() == got["cost"].tobytes()
    # the device pointer of the field: the same bytes, and usable by the kernel-level entries as it is
    import ctypes as C
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceView
    from emfusion_amd.pipeline import _check, load
    ptr = C.c_void_p()
    _check("emf_fusion_plan_cost_ptr", load().emf_fusion_plan_cost_ptr(fus._h, C.byref(ptr)))
    field = DeviceView(ptr.value, (BG, BG, BG), np.uint32)
    assert field.numpy().tobytes() == got["cost"].tobytes()
    g = next(g for g in got["goals"] if g["reachable"])
    walk, lengths, goal_cost = ops.plan_paths(field, [g["voxel"]])
    assert goal_cost[0] == g["cost"] and lengths[0] == len(g["path_vox"])
    lin = walk[0, :lengths[0]].astype(np.int64)
    assert np.stack([lin % BG, lin // BG % BG, lin // (BG * BG)], axis=1).astype(np.int32).tobytes() == g["path_vox"].tobytes()
    assert [(g["label"], g["cost"], g["path_vox"].tobytes()) for g in again["goals"]] == \
        [(g["label"], g["cost"], g["path_vox"].tobytes()) for g in got["goals"]]


def test_clearance_radius_and_exclude(session):
    fus, oid = session
    plain = fus.plan(field=True)
    got = fus.plan(field=True, clearance=0.07, min_voxels=1)  # rounded up to two voxels
    assert voxels_of(0.07) == 2
    check(fus, got, clearance=0.07)
    assert 0 < got["n_finite"] < plain["n_finite"]  # the gate does keep the paths off the surface
    got = fus.plan(field=True, clearance=0.07, start_radius=0.2, exclude=[oid], min_voxels=3)
    check(fus, got, clearance=0.07, exclude=[oid], radius=5)
    got = fus.plan(field=True, start_radius=0.0)
    check(fus, got, radius=0)


def test_through_unknown_reaches_at_least_as_much(session):
    fus, _ = session
    plain = fus.plan(field=True, min_voxels=1)
    got = fus.plan(field=True, through_unknown=True, min_voxels=1)
    check(fus, got, through_unknown=True)
    assert got["n_finite"] > plain["n_finite"]
    finite = plain["cost"] < pl.BLOCKED
    assert (got["cost"][finite] <= plain["cost"][finite]).all()
    reach = {g["label"]: g for g in got["goals"]}
    for g in plain["goals"]:
        if g["reachable"]:
            assert reach[g["label"]]["reachable"] and reach[g["label"]]["cost"] <= g["cost"]


def test_explicit_goals_start_and_the_camera_box(session):
    fus, _ = session
    whole = fus.plan(field=True)
    # explicit world-point goals: a reachable voxel, a blocked one, one outside the background; never snapped
    cost = whole["cost"]
    reachable = np.argwhere((cost < pl.BLOCKED) & (cost > 60))[0][::-1]
    blocked = np.argwhere(cost == pl.BLOCKED)[0][::-1]
    pts = world_of(fus, (0, 0, 0), np.array([reachable, blocked, (-3, 5, 5)]))
    got = fus.plan(goals=pts + np.float32(0.3 * VOX), field=True)  # off the voxel centres: rounded to the same voxels
    assert [g["voxel"] for g in got["goals"]] == [tuple(int(v) for v in reachable), tuple(int(v) for v in blocked), (-3, 5, 5)]
    assert [g["reachable"] for g in got["goals"]] == [True, False, False] and "clusters" not in got
    assert got["goals"][1]["cost"] == got["goals"][2]["cost"] == pl.BLOCKED and len(got["goals"][1]["path_vox"]) == 0
    check(fus, got)
    # an explicit start: two world points, one of them outside the background (ignored)
    starts = world_of(fus, (0, 0, 0), np.array([reachable, (70, 0, 0)]))
    got = fus.plan(goals=pts[:1], start=starts, field=True, max_cost=1.0)
    assert got["n_starts"] == 1 and got["max_cost"] == int(np.floor(3.0 / float(np.float32(VOX))))
    check(fus, got, max_cost=got["max_cost"])
    assert got["goals"][0]["cost"] == 0 and len(got["goals"][0]["path_vox"]) == 1
    # a cap below a third of a voxel is the smallest cap, 1, not "no cap"
    got = fus.plan(goals=pts[:1], field=True, max_cost=0.001)
    assert got["max_cost"] == 1 and got["n_finite"] == 1
    check(fus, got, max_cost=1)
    # the camera box: box coordinates throughout
    got = fus.plan(box="camera", size=24, min_voxels=1, field=True)
    assert got["box"] == fus.camera_box(24) and got["cost"].shape == got["box"][1][::-1]
    check(fus, got)
    cam = np.array(fus.camera_box(1)[0]) - np.array(got["box"][0])
    assert tuple(got["start_voxels"][0]) == tuple(cam) and got["cost"][cam[2], cam[1], cam[0]] == 0
    from emfusion_amd import pipeline
    with pytest.raises(pipeline.FusionError) as err:
        fus.plan(box=((40, 0, 0), (25, 8, 8)))
    assert err.value.code == -4
    with pytest.raises(ValueError):
        fus.plan(box="camera")
    with pytest.raises(ValueError):
        fus.plan(goals="nearest")


def test_earlier_queries_are_unchanged_after_a_plan(session):
    fus, _ = session
    from emfusion_amd.pipeline import _check, load
    df = fus.distance_field()
    fr = fus.frontiers(labels=True, min_voxels=1)
    kept = fr["kept"]
    lib = load()
    fus.plan(goals=world_of(fus, (0, 0, 0), np.array([[31, 32, 5]])), clearance=0.07, through_unknown=True)
    d2, classes = np.empty_like(df["d2"]), np.empty_like(df["classes"])
    _check("emf_fusion_copy_distance_field", lib.emf_fusion_copy_distance_field(fus._h, classes.ctypes.data, d2.ctypes.data, None))
    assert d2.tobytes() == df["d2"].tobytes() and classes.tobytes() == df["classes"].tobytes()
    records, labels = np.zeros(kept, fr["records"].dtype), np.empty_like(fr["labels"])
    _check("emf_fusion_copy_frontiers", lib.emf_fusion_copy_frontiers(fus._h, records.ctypes.data, kept, None, None, labels.ctypes.data))
    assert records.tobytes() == fr["records"].tobytes() and labels.tobytes() == fr["labels"].tobytes()


def test_the_shared_clearance_scratch_is_never_reused_stale(session):
    """frontiers() and plan() put their clearance transform into one scratch volume: each call fills it for its own
    clearance, so a plan with another clearance in between leaves the frontiers what they were."""
    fus, _ = session
    a = fus.frontiers(labels=True, min_voxels=1, clearance=0.03)
    got = fus.plan(goals=world_of(fus, (0, 0, 0), np.array([[31, 32, 5]])), clearance=0.07, through_unknown=True)
    b = fus.frontiers(labels=True, min_voxels=1, clearance=0.03)
    c = fus.frontiers(labels=True, min_voxels=1, clearance=0.07)
    assert a["records"].tobytes() == b["records"].tobytes() and a["labels"].tobytes() == b["labels"].tobytes()
    assert c["n_voxels"] <= a["n_voxels"]
    check(fus, got, clearance=0.07, through_unknown=True)


def test_the_next_frame_is_that_of_a_session_that_never_asked(dev):
    from tests.test_gpu_frontier_pipeline import feed, open_session
    out = []
    for ask in (False, True):
        fus, oid, synth = open_session()
        if ask:
            fus.plan(clearance=0.07, field=True)
            fus.plan(box="camera", size=24, through_unknown=True)
        feed(fus, synth, oid, 3)
        synth.close()
        out.append([fus.volume("tsdf", 0), fus.volume("weights", 0), fus.volume("tsdf", oid), fus.volume("weights", oid),
                    *fus.pose(0), *fus.pose(oid), *fus.background_pose()])
        fus.close()
    assert len(out[0]) == len(out[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(*out))


def read_plan(path):
    """[(count, reachable, cost, length_m, rep f32 (3,), path f32 (n, 3))] of a plan.txt."""
    lines = Path(path).read_text().splitlines()
    assert lines[0].startswith("# count reachable cost length_m rep_x rep_y rep_z n_path")
    out, k = [], 1
    while k < len(lines):
        r = lines[k].split()
        assert len(r) == 8
        n = int(r[7])
        pts = np.array([[np.float32(v) for v in line.split()] for line in lines[k + 1:k + 1 + n]], np.float32).reshape(-1, 3)
        assert len(pts) == n
        out.append((int(r[0]), int(r[1]), int(r[2]), float(r[3]), np.array([np.float32(v) for v in r[4:7]], np.float32), pts))
        k += 1 + n
    return out


def check_plan_file(rows, voxel):
    """What holds for every plan.txt: a path starts at the representative, moves by 26-neighbour steps whose lengths
    sum to length_m, and is there exactly where the cluster is reachable."""
    for count, reachable, cost, length_m, rep, pts in rows:
        assert reachable in (0, 1) and (len(pts) > 0) == bool(reachable) and count >= 1
        if not reachable:
            assert cost in (pl.UNREACHED, pl.BLOCKED) and length_m == 0
            continue
        assert np.abs(pts[0] - rep).max() < 1e-6
        steps = np.linalg.norm(np.diff(pts.astype(np.float64), axis=0), axis=1)
        kind = (steps / voxel) ** 2  # 1, 2 or 3: a face, an edge or a corner step
        assert (np.abs(kind - np.rint(kind)) < 1e-3).all() and (np.rint(kind) >= 1).all() and (np.rint(kind) <= 3).all()
        assert cost == int((2 + np.rint(kind)).sum())
        assert abs(steps.sum() - length_m) < 1e-4 and 3 * (len(pts) - 1) <= cost <= 5 * (len(pts) - 1)


def assert_file_is_the_plan(rows, got, order):
    """The rows of a plan.txt are Fusion.plan()'s clusters, in the order of frontiers.txt."""
    by_label = {g["label"]: g for g in got["clusters"]}
    assert len(rows) == len(order) == len(by_label)  # the file keeps the order of frontiers.txt
    for (count, reachable, cost, length_m, rep, pts), c in zip(rows, order):
        g = by_label[c["label"]]
        assert (count, bool(reachable), cost) == (g["count"], g["reachable"], g["cost"])
        # the world points within one float32 ulp: the integers they come from are exact, only the last rounding may
        # differ where the order of the float64 operations does (as for frontiers.txt)
        assert np.float32(length_m) == np.float32(g["length_m"]) and one_ulp(rep, g["rep_world"])
        assert pts.shape == g["path_world"].shape and one_ulp(pts, g["path_world"])


def test_write_results_writes_the_file_only_with_the_switch(dev, tmp_path):
    out = {}
    for on in (False, True):
        fus, _ = new_session()
        if on:
            fus.setup_output(False, False, frontier_min_voxels=3, exp_plan=True, plan_clearance=0.07)
        else:
            fus.setup_output(False, False)
        fus.write_results(tmp_path / str(on), volumes=False)
        if on:
            got = fus.plan(min_voxels=3, clearance=0.07)
            order = fus.frontiers(min_voxels=3, clearance=0.07)["clusters"]
        fus.close()
        out[on] = listing(tmp_path / str(on))
    assert set(out[True]) - set(out[False]) == {"plan.txt"} and set(out[False]) <= set(out[True])
    assert all(out[True][k] == v for k, v in out[False].items())
    rows = read_plan(tmp_path / "True" / "plan.txt")
    check_plan_file(rows, float(np.float32(VOX)))
    assert len(rows) >= 2
    assert_file_is_the_plan(rows, got, order)


def test_the_apps_write_the_file_and_nothing_else_changes(dev, tmp_path):
    """Both apps: with --plan the results gain plan.txt and no other byte changes, without and with
    --plan-through-unknown.  On the staged sequence -- apps/run_tum.py and apps/emfusion_synth --sequence, which
    tests/test_gpu_cpp_app.py holds equal to the Python loop -- the file is, row by row, the Fusion.plan() of a session
    that was fed the same frames in this process: the start voxel under the tracked camera (clamped into the volume,
    whose near face lies half a voxel behind the first camera), the clearance, the switch, the ties of the paths.  The
    synthetic stream of apps/emfusion_synth has no twin in this process; its file is checked against the frontiers.txt
    of the same run and for what holds for every plan."""
    from tests import tum_staging as T
    from tests.test_gpu_frontier_pipeline import read_frontiers
    from tests.test_gpu_voxel_color_app import _python_run
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    seq, masks, _ = T.stage(tmp_path)
    front = ["--frontiers", "--frontier-min-voxels", "4", "--frontier-clearance", "0.05"]
    plan = front + ["--plan", "--plan-clearance", "0.05"]
    small = ["--frames", "4", "--objects", "1", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    apps = {"synth": ([str(APP), *small], 5.12 / 64),
            "sequence": ([str(APP), "--sequence", seq, "--masks", str(masks), *T.SMALL], 0.04),
            "tum": ([sys.executable, str(ROOT / "apps" / "run_tum.py"), seq, "--masks", str(masks), *T.SMALL], 0.04)}
    files = {}
    for app, (cmd, voxel) in apps.items():
        outs = {}
        for name, extra in (("plain", front), ("plan", plan), ("unknown", plan + ["--plan-through-unknown"])):
            p = subprocess.run([*cmd, "--out", str(tmp_path / app / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
            outs[name] = listing(tmp_path / app / name)
        for name in ("plan", "unknown"):
            assert set(outs[name]) - set(outs["plain"]) == {"plan.txt"}, (app, name)
            assert all(outs[name][k] == v for k, v in outs["plain"].items()) and len(outs["plain"]) > 3
            rows = read_plan(tmp_path / app / name / "plan.txt")
            check_plan_file(rows, float(np.float32(voxel)))
            counts, rep, _, _ = read_frontiers(tmp_path / app / name / "frontiers.txt")
            assert [r[0] for r in rows] == counts and len(rows) >= 1, (app, name)
            assert np.array([r[4] for r in rows], np.float32).reshape(-1, 3).tobytes() == rep.tobytes()
            files[app, name] = rows
    assert any(r[1] for r in files["synth", "plan"])  # the supplied camera stands in the first slice: a plan, not an empty one
    fus = _python_run(T, seq, masks, False)  # the apps' loop on the same frames, kept open
    try:
        order = fus.frontiers(min_voxels=4, clearance=0.05)["clusters"]
        finite = {}
        for name, through in (("plan", False), ("unknown", True)):
            got = fus.plan(min_voxels=4, clearance=0.05, through_unknown=through)
            assert got["n_starts"] == 1 and (got["start_voxels"][0] >= 0).all() and (got["start_voxels"][0] < 64).all()
            finite[name] = got["n_finite"]
            for app in ("sequence", "tum"):
                assert_file_is_the_plan(files[app, name], got, order)
        assert finite["unknown"] > finite["plan"] >= 1  # the switch does matter on this scene
    finally:
        fus.close()


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.plan(goals=np.zeros((1, 3), np.float32)), lambda: fus.plan(goals=np.zeros((1, 3)), box=((0, 0, 0), (8, 8, 8)))):
            with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4, -4], [-4, -4]]
