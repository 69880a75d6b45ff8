"""Fusion.planes(patches=True), Fusion.object_support and the patch lines of planes.txt on a live session (DESIGN.md
5.26): the 64^3 background with one object of the plane finder's pipeline test, built here the same way.  The patches
equal tests/patches_reference.py applied to the records and labels that planes(labels=True) reports, byte for byte --
ids, counters, records and every rectangle's float64 bits; the counts of a plane's patches sum to the plane's; planes()
without the argument is what it was; object_support names the patch under the object; planes.txt carries the patch
lines only with the switch, from Python and from apps/emfusion_synth, and no other result byte changes; the sharded
path refuses; a checkpoint written after the calls equals one written without them and nothing of the session changes."""
import subprocess

import numpy as np
import pytest

from tests import patches_reference as qr
from tests.test_gpu_frontier_pipeline import APP, BG, ROOT, VOX, new_session, params

pytestmark = pytest.mark.gpu
TO_CAMERA = (0.0, 0.0, -1.0)


@pytest.fixture(scope="module")
def session(dev):
    fus, oid = new_session()
    yield fus, oid
    fus.close()


def raw_planes(fus, got):
    """The planes of a result as the restatement takes them: n, d and axes in box voxels, read back from the records that
    the result carries (pipeline.PLANE_DTYPE under the patches' rect_voxel is the patch's; the plane's own comes from the
    C entry again)."""
    import ctypes as C
    from emfusion_amd import pipeline
    recs, count = np.zeros(64, pipeline.PLANE_DTYPE), C.c_int32(0)
    lo_out, size_out, R, t = pipeline._box_outs()
    lo_arg, size_arg, _, _ = pipeline._box_args(got["box"], ())
    counters, votes = np.zeros(4, np.uint32), C.c_uint32(0)
    prm = np.zeros((), pipeline.PLANE_PARAMS_DTYPE)
    prm["K"], prm["refine"], prm["max_planes"], prm["peak_gap"] = 15, 1, 64, 2
    prm["angle_deg"], prm["bin_vox"], prm["band_vox"] = 20.0, 1.0, 2.0
    assert pipeline.load().emf_fusion_planes(fus._h, lo_arg, size_arg, prm.ctypes.data, lo_out, size_out, R, t, counters.ctypes.data,
                                             C.byref(votes), recs.ctypes.data, 64, C.byref(count)) == 0
    return recs[:count.value]


def world(fus, lo, v):
    """QueryBox::worldPoint in Python floats."""
    bg_R, bg_t = fus.background_pose()
    R, t = [[float(c) for c in row] for row in bg_R], [float(c) for c in bg_t]
    vs = float(np.float32(VOX))
    p = [(float(v[j]) + (float(lo[j]) - (float(BG) - 1.0) / 2.0)) * vs for j in range(3)]
    return [((R[i][0] * p[0] + R[i][1] * p[1]) + R[i][2] * p[2]) + t[i] for i in range(3)]


def check(fus, reach, min_voxels):
    """planes(patches=True, labels=True) against the restatement on its own records and labels."""
    got = fus.planes(labels=True, patches=True, patch_reach=reach, patch_min_voxels=min_voxels)
    planes = raw_planes(fus, got)
    lo, size = got["box"]
    rec = got["records"]
    labels = got["labels"].reshape(-1)[rec["index"]]
    P = max(int(p["label"]) for p in planes) + 1
    axes = np.zeros((P, 6), np.float32)
    for p in planes:
        axes[p["label"]] = p["axes"].astype(np.float32)
    patch = qr.patch_ids(rec, labels, size, reach)
    every = qr.patch_records(rec, labels, patch, size, axes)
    floor = max(25, got["min_votes"] // 4) if min_voxels is None else min_voxels
    want, kept = qr.emitted(every, floor, len(every), len(every))
    assert got["patch_counters"] == tuple(int(v) for v in qr.counters(labels, patch, kept))
    volume = np.full(size[0] * size[1] * size[2], -1, np.int32)
    volume[rec["index"]] = patch
    assert got["patch_ids"].dtype == np.int32 and got["patch_ids"].tobytes() == volume.tobytes()
    vs = float(np.float32(VOX))
    seen = 0
    for p, raw in zip(got["planes"], planes):
        mine = want[want["plane"] == raw["label"]]
        mine = mine[np.argsort(-mine["count"].astype(np.int64), kind="stable")]
        assert [q["id"] for q in p["patches"]] == mine["id"].tolist()
        plane = dict(n=[float(v) for v in raw["n"]], d=float(raw["d"]),
                     axes=[[float(v) for v in raw["axes"][:3]], [float(v) for v in raw["axes"][3:]]])
        for q, w in zip(p["patches"], mine):
            assert q["record"].tobytes() == w.tobytes()
            r = qr.rect(plane, w)
            rv = q["rect_voxel"]
            assert rv["center"].tobytes() == np.array(r["center"]).tobytes() and rv["half"].tobytes() == np.array(r["half"]).tobytes()
            assert rv["corners"].tobytes() == np.array(r["corners"]).tobytes() and float(rv["fill"]) == r["fill"] == q["fill"]
            assert rv["fit"]["n"].tobytes() == np.array(r["fit"]["n"]).tobytes() and float(rv["fit"]["d"]) == r["fit"]["d"]
            assert q["rect"]["center"].tobytes() == np.array(world(fus, lo, r["center"])).tobytes()
            assert q["rect"]["corners"].tobytes() == np.array([world(fus, lo, c) for c in r["corners"]]).tobytes()
            assert q["rect"]["half_m"].tobytes() == np.array([r["half"][0] * vs, r["half"][1] * vs]).tobytes()
            if r["fit"]["fitted"]:
                assert q["point"].tobytes() == np.array(world(fus, lo, r["fit"]["centroid"])).tobytes()
            assert q["count"] == int(w["count"]) and q["kind"] == p["kind"] and 0.0 < q["fill"] < 1.5
            assert q["bounds"] == (tuple(w["lo"].tolist()), tuple(w["hi"].tolist()))
            # the corners lie in the plane, the members between them
            for c in r["corners"]:
                assert abs(float(np.dot(plane["n"], c)) - plane["d"]) < 1e-9
            seen += 1
        if floor == 1:
            assert sum(q["count"] for q in p["patches"]) == p["count"]
    assert seen == kept == len(want)
    return got


def test_patches_equal_the_restatement(session):
    fus, _ = session
    got = check(fus, 1, None)
    assert got["patch_counters"][0] >= 1 and sum(len(p["patches"]) for p in got["planes"]) == got["patch_counters"][0]
    print("patches:", [(p["kind"], p["count"], [(q["id"], q["count"], round(q["fill"], 3)) for q in p["patches"]]) for p in got["planes"]])
    check(fus, 1, 1)
    check(fus, 2, 1)
    check(fus, 2, 40)


def test_without_the_argument_nothing_is_new(session):
    fus, _ = session
    plain, asked = fus.planes(labels=True), fus.planes(labels=True, patches=True)
    assert set(asked) - set(plain) == {"patch_counters", "patch_ids"} and set(plain) <= set(asked)
    assert set(plain) == {"planes", "box", "counters", "min_votes", "floor", "labels", "records"}
    for a, b in zip(plain["planes"], asked["planes"]):
        assert set(b) - set(a) == {"patches"}
        for key, value in a.items():
            assert np.asarray(value).tobytes() == np.asarray(b[key]).tobytes(), key
    for key in ("box", "counters", "min_votes", "floor"):
        assert plain[key] == asked[key]
    assert plain["labels"].tobytes() == asked["labels"].tobytes() and plain["records"].tobytes() == asked["records"].tobytes()


def test_bad_arguments_are_refused(dev):
    from emfusion_amd import pipeline
    fus, _ = new_session()
    with pytest.raises(pipeline.FusionError, match="no planes have been computed"):
        fus._plane_patches(dict(), [], None, None, 1.0, 1, 1, False)
    for kw, code in ((dict(patch_reach=0), -4), (dict(patch_reach=3), -5), (dict(patch_min_voxels=0), -4)):
        with pytest.raises(pipeline.FusionError) as err:
            fus.planes(patches=True, **kw)
        assert err.value.code == code, kw
    fus.close()


def test_object_support_names_the_patch_under_the_object(session):
    """The session's object hovers in front of the wall.  With up towards the camera the wall is the floor; under the
    default gap the object rests on nothing, and under a gap above its height it rests on the patch of the wall whose
    rectangle its centre lies over.  Both equal the restatement in Python floats."""
    fus, oid = session
    res = fus.object_support(up_hint=TO_CAMERA)
    planes = res["planes"]
    assert planes["floor"] is not None and set(res["objects"]) == {oid}
    shape = fus.object_shapes([oid])[0]
    assert shape["valid"]
    box = dict(center=[float(v) for v in shape["box_center_world"]], axes=[[float(v) for v in row] for row in shape["box_axes_world"]],
               half=[float(v) for v in shape["box_half"]])
    flat = [(k, q) for k, p in enumerate(planes["planes"]) for q in p["patches"]]

    def as_floats(q):
        return dict(kind=q["kind"], normal=[float(v) for v in q["normal"]], d=q["d"],
                    rect=dict(center=[float(v) for v in q["rect"]["center"]], axes=[[float(v) for v in row] for row in q["rect"]["axes"]],
                              half_m=[float(v) for v in q["rect"]["half_m"]]))

    want = qr.rests_on([as_floats(q) for _, q in flat], box)
    assert (res["objects"][oid] is None) == (want is None)
    floor_patches = [(k, q) for k, q in flat if q["kind"] == "floor"]
    assert floor_patches
    heights = [qr.support(*[as_floats(q)[key] for key in ("normal", "d")], as_floats(q)["rect"]["center"], as_floats(q)["rect"]["axes"],
                          as_floats(q)["rect"]["half_m"], box["center"], box["axes"], box["half"], 0.0) for _, q in floor_patches]
    print("support:", res["objects"], heights)
    over = [(abs(s), k, q["id"], s) for (k, q), (s, is_over) in zip(floor_patches, heights) if is_over]
    assert over, "the object is over no patch of the wall"
    gap = max(h[0] for h in over) + 0.01
    far = fus.object_support(gap=gap, up_hint=TO_CAMERA)["objects"][oid]
    want = qr.rests_on([as_floats(q) for _, q in flat], box, gap=gap)
    assert far is not None and (far["plane"], far["patch"], far["s"]) == (flat[want[0]][0], flat[want[0]][1]["id"], want[1])
    assert planes["planes"][far["plane"]]["kind"] in ("floor", "level")


def test_nothing_of_the_session_changes(session):
    fus, oid = session
    before = [fus.volume(k, i).tobytes() for i in (0, oid) for k in ("tsdf", "weights")]
    plain = fus.planes(labels=True)
    fus.planes(labels=True, patches=True, patch_reach=2)
    fus.object_support(up_hint=TO_CAMERA)
    again = fus.planes(labels=True)
    assert [fus.volume(k, i).tobytes() for i in (0, oid) for k in ("tsdf", "weights")] == before
    assert again["labels"].tobytes() == plain["labels"].tobytes() and again["records"].tobytes() == plain["records"].tobytes()
    assert repr([sorted(p.items(), key=lambda kv: kv[0]) for p in again["planes"]]) == \
        repr([sorted(p.items(), key=lambda kv: kv[0]) for p in plain["planes"]])


def test_a_checkpoint_after_the_calls_equals_one_without_them(dev, tmp_path):
    files = []
    for ask in (False, True):
        fus, oid = new_session()
        if ask:
            fus.planes(labels=True, patches=True)
            fus.object_support(up_hint=TO_CAMERA)
        fus.save_checkpoint(tmp_path / f"{ask}.ckpt")
        fus.close()
        files.append((tmp_path / f"{ask}.ckpt").read_bytes())
    assert files[0] == files[1] and len(files[0]) > 1000


def split_planes_file(path):
    """(the lines of planes.txt as they are without the switch, [(plane index, patch fields)], [support fields])."""
    lines = path.read_text().splitlines()
    plain, patches, support, planes = [lines[0]], [], [], -1
    for line in lines[1:]:
        f = line.split()
        if f[0] == "patch":
            assert len(f) == 19
            patches.append((planes, f[1:]))
        elif f[0] == "support":
            assert len(f) == 5
            support.append(f[1:])
        else:
            assert not support, "a plane after the support lines"
            planes += 1
            plain.append(line)
    return plain, patches, support


def check_patch_lines(patches, got):
    want = [(k, q) for k, p in enumerate(got["planes"]) for q in p["patches"]]
    assert len(patches) == len(want) >= 1
    for (k, f), (wk, q) in zip(patches, want):
        assert k == wk and int(f[0]) == q["id"] and int(f[1]) == q["count"]
        assert f[2:] == ["%.9g" % v for v in list(q["point"]) + list(q["rect"]["corners"].reshape(-1)) + [q["fill"]]], (f, q)


def test_write_results_writes_the_patch_lines_only_with_the_switch(dev, tmp_path):
    from tests.test_gpu_ground_pipeline import digest
    out, text = {}, {}
    cases = (("off", {}), ("planes", dict(exp_planes=True)), ("patches", dict(exp_planes=True, exp_plane_patches=True)),
             ("reach", dict(exp_planes=True, exp_plane_patches=True, plane_patch_reach=2, plane_patch_min=10, exp_object_shapes=True)),
             ("shapes", dict(exp_planes=True, exp_object_shapes=True)))
    for name, kw in cases:
        fus, oid = new_session()
        fus.setup_output(False, False, **kw)
        fus.write_results(tmp_path / name, volumes=False)
        if kw.get("exp_plane_patches"):
            plain, patches, support = split_planes_file(tmp_path / name / "planes.txt")
            got = fus.planes(patches=True, patch_reach=kw.get("plane_patch_reach", 1), patch_min_voxels=kw.get("plane_patch_min"))
            check_patch_lines(patches, got)
            text[name] = "\n".join(plain) + "\n"
            if kw.get("exp_object_shapes"):  # the lines are those of object_support with the file's own policy
                hit = fus.object_support(patch_reach=kw["plane_patch_reach"], patch_min_voxels=kw["plane_patch_min"])["objects"][oid]
                assert support == ([] if hit is None else [[str(oid), str(hit["plane"]), str(hit["patch"]), "%.9g" % hit["s"]]])
            else:
                assert support == []
        with pytest.raises(ValueError, match="needs exp_planes"):
            fus.setup_output(False, False, exp_plane_patches=True)
        fus.close()
        out[name] = digest(tmp_path / name)
    assert out["planes"] != out["off"] and set(out["planes"]) - set(out["off"]) == {"planes.txt"}
    # without the switch no byte changes; with it planes.txt alone does, and what it held before is still there, line by line
    for name, base in (("patches", "planes"), ("reach", "shapes")):
        assert set(out[name]) == set(out[base])
        assert all(out[name][k] == v for k, v in out[base].items() if k != "planes.txt") and out[name]["planes.txt"] != out[base]["planes.txt"]
        assert text[name] == (tmp_path / base / "planes.txt").read_text()


def test_the_app_writes_the_patch_lines_and_nothing_else_changes(dev, tmp_path):
    from tests.test_gpu_ground_pipeline import digest
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    small = [str(APP), "--frames", "4", "--objects", "1", "--bg-res", "64", "--obj-res", "32", "--width", "160", "--height", "120"]
    base = ["--planes", "--planes-min-votes", "30", "--object-shapes"]
    outs = {}
    for name, extra in (("planes", base), ("patches", base + ["--plane-patches", "--plane-patch-reach", "2", "--plane-patch-min", "12"])):
        p = subprocess.run([*small, "--out", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name] = digest(tmp_path / name)
    assert set(outs["patches"]) == set(outs["planes"])
    assert all(outs["patches"][k] == v for k, v in outs["planes"].items() if k != "planes.txt")
    plain, patches, support = split_planes_file(tmp_path / "patches" / "planes.txt")
    assert "\n".join(plain) + "\n" == (tmp_path / "planes" / "planes.txt").read_text()
    assert len(patches) >= 1 and all(int(f[1]) >= 12 for _, f in patches)
    counts = {}
    for k, f in patches:  # inside a plane by count descending
        assert counts.get(k, 1 << 62) >= int(f[1])
        counts[k] = int(f[1])
    for bad in (["--plane-patches"], ["--planes", "--plane-patch-reach", "2"], ["--planes", "--plane-patches", "--plane-patch-reach", "3"],
                ["--planes", "--plane-patch-min", "5"]):
        p = subprocess.run([*small, "--out", str(tmp_path / "bad"), *bad], cwd=ROOT, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--plane-patches" in p.stderr, (bad, p.stderr[-400:])


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.planes(patches=True), lambda: fus._plane_patches(dict(), [], None, None, 1.0, 1, 1, False),
                     lambda: fus.object_support()):
            with pytest.raises(pipeline.FusionError, match="the plane search is not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4, -4, -4], [-4, -4, -4]]
