"""Fusion.object_contacts on a live session: the two-sphere 64^3 session of
test_gpu_object_shape_pipeline.py.  Every record equals tests/contacts_reference.py applied to Fusion.volume(...) and
Fusion.pose(...) as bytes, every summary as float64 bits; background=False drops slot 0; an unknown id raises; the
session, its next frame and its checkpoint are those of a twin that never asked; contacts.txt appears with the switch
and only with it, from Python (equal to the Python result as strings) and from both apps; the usage errors; a sharded
session refuses.  The analytic spheres of the CPU test run through ops.contact_probe on the device."""
import subprocess
import sys

import numpy as np
import pytest

from tests import contacts_reference as cr
from tests.test_gpu_frontier_pipeline import APP, ROOT, listing, params
from tests.test_gpu_object_shape_pipeline import feed, open_session, snapshot

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def session(dev):
    fus, oids, synth = open_session()
    synth.close()
    yield fus, oids
    fus.close()


def model(fus, oid, side):
    """The volumes and the side record of one model, from what the session hands out."""
    fg = fus.volume("fgmask", oid) if oid else None
    R, t = fus.pose(oid) if oid else fus.background_pose()
    if oid:
        info = fus.object_info(oid)
        assert (float(side["voxel_size"]), float(side["truncdist"])) == (info["voxel_size"], info["truncdist"])
    tsdf = fus.volume("tsdf", oid)
    assert tuple(side["res"]) == tsdf.shape[::-1] and side["R"].tobytes() == R.tobytes() and side["t"].tobytes() == t.tobytes()
    assert side["voxel_size"] > 0 and side["truncdist"] > 0
    return cr.vol(tsdf, fus.volume("weights", oid), fg, side["voxel_size"])


def check_result(fus, got, oids, background, touch):
    ids = ([0] if background else []) + list(oids)
    assert got["ids"] == ids and got["sides"].dtype == cr.SIDE
    sides = dict(zip(ids, got["sides"]))
    vols = {i: model(fus, i, sides[i]) for i in ids}
    order = [(a, b) for a in oids for b in ids if a != b]
    assert [(p["a"], p["b"]) for p in got["pairs"]] == order  # grouped by probe; the background is no probe
    for k, p in enumerate(got["pairs"]):
        sa, sb = sides[p["a"]], sides[p["b"]]
        R, t = cr.contact_pose_np(sa["R"], sa["t"], sb["R"], sb["t"])
        assert p["R"].tobytes() == R.tobytes() and p["t"].tobytes() == t.tobytes()
        want_touch = cr.contact_touch_np(float(sa["voxel_size"]) if touch is None else touch, sb["truncdist"])
        assert f32(p["touch"]).tobytes() == want_touch.tobytes()
        want = cr.probe(vols[p["a"]], vols[p["b"]], cr.pair(0, 1, R, t, want_touch))
        assert p["record"].dtype == cr.CONTACT and p["record"].tobytes() == want.tobytes(), (p["a"], p["b"], p["record"], want)
        cr.check_identities(want)
        assert all(p[c] == int(want[c]) for c in cr.COUNTS) and p["surface"] > 0
        assert f32(p["min_s"]).tobytes() == want["min_s"].tobytes()
    at = {pair: k for k, pair in enumerate(order)}
    unordered = []
    for a, b in order:
        if (b, a) not in unordered:
            unordered.append((a, b))
    assert [(s["a"], s["b"]) for s in got["summaries"]] == unordered
    for s in got["summaries"]:
        ab = got["pairs"][at[(s["a"], s["b"])]]["record"]
        back = at.get((s["b"], s["a"]))
        assert s["record_ab"] == at[(s["a"], s["b"])] and s["record_ba"] == back
        ba = None if back is None else got["pairs"][back]["record"]
        want = cr.contact_summary_np(ab, ba, sides[s["a"]], sides[s["b"]])
        assert s["summary"].dtype == cr.SUMMARY and s["summary"].tobytes() == want.tobytes(), (s["summary"], want)
        assert cr.contact_summary_py(ab, ba, sides[s["a"]], sides[s["b"]]).tobytes() == want.tobytes()
        assert s["state"] == ("unseen", "apart", "touching", "penetrating")[int(want["state"])]
        assert np.float64(s["distance_m"]).tobytes() == want["distance_m"].tobytes() and s["saturated"] == bool(want["saturated"])
        assert (s["point"] is None) == (want["direction"] < 0) and (s["normal"] is None) == (not want["has_normal"])
    return got


def test_object_contacts_equal_the_reference(session):
    fus, oids = session
    before = snapshot(fus, oids)
    got = check_result(fus, fus.object_contacts(), oids, True, None)
    assert len(got["pairs"]) == 4 and len(got["summaries"]) == 3
    for p in got["pairs"]:
        print(p["a"], p["b"], {c: p[c] for c in cr.COUNTS}, p["min_s"])
    for touch in (0.0, 0.02, float("inf")):
        check_result(fus, fus.object_contacts(touch=touch), oids, True, touch)
    wide = fus.object_contacts(touch=float("inf"))
    assert all(p["touching"] == p["sampled"] for p in wide["pairs"])
    swapped = check_result(fus, fus.object_contacts(ids=oids[::-1]), oids[::-1], True, None)
    by = {(p["a"], p["b"]): p["record"].tobytes() for p in got["pairs"]}
    assert all(by[(p["a"], p["b"])] == p["record"].tobytes() for p in swapped["pairs"])
    none = fus.object_contacts(ids=[])
    assert none["pairs"] == [] and none["summaries"] == [] and none["ids"] == [0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, snapshot(fus, oids)))  # nothing of the session changed


def test_background_false_drops_slot_zero(session):
    fus, oids = session
    full = fus.object_contacts()
    got = check_result(fus, fus.object_contacts(background=False), oids, False, None)
    assert len(got["pairs"]) == 2 and len(got["summaries"]) == 1 and 0 not in got["ids"]
    by = {(p["a"], p["b"]): p["record"].tobytes() for p in full["pairs"]}
    assert all(by[(p["a"], p["b"])] == p["record"].tobytes() for p in got["pairs"])
    one = fus.object_contacts(ids=oids[:1], background=False)
    assert one["pairs"] == [] and one["summaries"] == [] and one["ids"] == oids[:1]
    alone = check_result(fus, fus.object_contacts(ids=oids[1:]), oids[1:], True, None)
    assert len(alone["pairs"]) == 1 and alone["summaries"][0]["record_ba"] is None


def test_an_unknown_id_raises(session):
    from emfusion_amd import pipeline
    fus, oids = session
    for bad in ([max(oids) + 7], [oids[0], 0], [-1], [oids[0], oids[0]]):
        with pytest.raises(pipeline.FusionError) as err:
            fus.object_contacts(ids=bad)
        assert err.value.code == -4, bad
    with pytest.raises(pipeline.FusionError):
        fus.object_contacts(touch=float("nan"))


def test_the_next_frame_and_the_checkpoint_are_those_of_a_session_that_never_asked(dev, tmp_path):
    out, files = [], []
    for ask in (False, True):
        fus, oids, synth = open_session()
        if ask:
            fus.object_contacts()
            fus.object_contacts(ids=oids[:1], background=False, touch=0.05)
        feed(fus, synth, oids, 3)
        synth.close()
        if ask:
            fus.object_contacts(touch=0.0)
        fus.save_checkpoint(tmp_path / f"{ask}.ckpt")
        files.append((tmp_path / f"{ask}.ckpt").read_bytes())
        out.append(snapshot(fus, oids) + [fus.image("segmentation"), fus.image("bg_raylengths")])
        fus.close()
    assert len(out[0]) == len(out[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(*out))
    assert files[0] == files[1] and len(files[0]) > 1000


def read_contacts(path):
    lines = path.read_text().splitlines()
    assert lines[0].startswith("# a b surface outside unknown masked sampled inside touching normals min_s") and "not a distance" in lines[0]
    rows = [line.split() for line in lines[1:]]
    assert all(len(r) == 10 + 7 for r in rows)
    for r in rows:
        n = [int(v) for v in r[:10]]
        assert n[0] > 0 and n[0] != n[1] and n[2] == sum(n[3:7]) and n[6] > 0 and n[7] <= n[6] and n[9] <= n[8] <= n[6]
        assert float(r[10]) <= 1.0
    return lines[1:]


def test_write_results_writes_the_file_only_with_the_switch(dev, tmp_path):
    from emfusion_amd import pipeline
    out, want = {}, {}
    for name, args in (("off", {}), ("on", dict(exp_object_contacts=True)), ("wide", dict(exp_object_contacts=True, contact_touch=0.3))):
        fus, oids, synth = open_session()
        synth.close()
        fus.setup_output(False, False, **args)
        fus.write_results(tmp_path / name, volumes=False)
        if args:
            got = fus.object_contacts(ids=sorted(oids), touch=args.get("contact_touch"))
            sides = dict(zip(got["ids"], got["sides"]))
            want[name] = [pipeline.contact_line(p["a"], p["b"], p["record"], sides[p["a"]], sides[p["b"]])
                          for p in got["pairs"] if p["sampled"] > 0]
        fus.close()
        out[name] = listing(tmp_path / name)
    for name in ("on", "wide"):
        assert set(out[name]) - set(out["off"]) == {"contacts.txt"} and set(out["off"]) <= set(out[name])
        assert all(out[name][k] == v for k, v in out["off"].items())  # every other file byte for byte
        assert read_contacts(tmp_path / name / "contacts.txt") == want[name]  # as strings
    assert len(want["wide"]) > 0 and want["wide"] != want["on"]
    fus = pipeline.Fusion(params())
    try:
        with pytest.raises(ValueError, match="needs exp_object_contacts"):
            fus.setup_output(False, False, contact_touch=0.01)
    finally:
        fus.close()


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
        for name, extra in (("plain", []), ("contacts", ["--object-contacts", "--contact-touch", "0.5"])):
            p = subprocess.run([*cmd, "--out", str(tmp_path / app / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
            outs[name] = listing(tmp_path / app / name)
        assert set(outs["contacts"]) - set(outs["plain"]) == {"contacts.txt"} and len(outs["plain"]) > 2, app
        assert all(outs["contacts"][k] == v for k, v in outs["plain"].items()), app
        rows = read_contacts(tmp_path / app / "contacts" / "contacts.txt")
        assert app != "synth" or len(rows) > 0


def test_the_usage_errors(tmp_path):
    """Refused before any device is touched."""
    if not APP.exists():
        pytest.fail("apps/emfusion_synth is not built (python -c 'import __graft_entry__ as g; g.build()')")
    tum = [sys.executable, str(ROOT / "apps" / "run_tum.py"), str(tmp_path)]
    for cmd, word in (([str(APP), "--contact-touch", "0.01", "--out", str(tmp_path)], "--object-contacts"),
                      ([str(APP), "--object-contacts"], "--out"),
                      ([str(APP), "--object-contacts", "--contact-touch", "-1", "--out", str(tmp_path)], "--contact-touch"),
                      ([*tum, "--contact-touch", "0.01"], "--object-contacts"),
                      ([*tum, "--object-contacts", "--contact-touch", "-1"], "--contact-touch")):
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and word in p.stderr, (cmd, p.returncode, p.stderr[-500:])
    assert not any(tmp_path.iterdir())


def test_refused_on_a_sharded_session(dev):
    from emfusion_amd import pipeline
    from tests.test_gpu_sharded_lifecycle import JOIN_S, run_ranks

    def body(r, comm, ready):
        fus = pipeline.Fusion(params(), comm)
        codes = []
        for call in (lambda: fus.object_contacts(), lambda: fus.object_contacts(ids=[], background=False)):
            with pytest.raises(pipeline.FusionError, match="not supported on the sharded path") as err:
                call()
            codes.append(err.value.code)
        ready.wait(timeout=JOIN_S)
        fus.close()
        return codes

    assert list(run_ranks(2, body)) == [[-4] * 2, [-4] * 2]


def test_the_analytic_spheres_on_the_device(dev):
    """The fixture of the CPU test through ops.contact_probe, in both libraries: the restatement's bytes, all six poses
    in one call, and the states physics asks for."""
    from emfusion_amd import _lib, ops
    from tests.parity_util import to_dev
    va, vb = cr.sphere_band(*cr.SPHERE_PROBE), cr.sphere_band(*cr.SPHERE_FIELD)
    pairs = np.array([cr.sphere_pair(dx) for dx in cr.SPHERE_DX], cr.PAIR)
    want = cr.expected([va, vb], pairs)
    volumes = [dict(tsdf=to_dev(v["tsdf"]), weights=to_dev(v["weights"]), voxel_size=v["voxel_size"]) for v in (va, vb)]
    for lib in (None, _lib.load_variant("_fma")):
        got = ops.contact_probe(volumes, pairs, lib=lib)
        assert got.tobytes() == want.tobytes(), (got, want)
    sa = cr.side(cr.SPHERE_PROBE[0], cr.SPHERE_PROBE[1], cr.SPHERE_TRUNC)
    sb = cr.side(cr.SPHERE_FIELD[0], cr.SPHERE_FIELD[1], cr.SPHERE_TRUNC)
    from emfusion_amd import pipeline
    assert [int(pipeline.contact_summary(r, None, sa, sb)["state"]) for r in got] == list(cr.SPHERE_STATES)
