"""The run-time switch table of the host classes (emfusion_amd/csrc/core/Switches.hpp) parses the environment exactly
as the scattered call sites did before the table existed -- oddities included: a switch that goes off on a leading '0'
stays on for "no", one that goes on on a leading '1' stays off for "yes".

Every case is a fresh child process (the product build's line about a demoted variable is printed once per process,
EMF_POOL_MIB is read once per process) that calls pipeline.describe_switches(); no GPU is needed.  The expected values
are literals, written from the parsing expressions the table replaced:

    x && x[0] == '0' -> off      EMF_BG_BANDS, EMF_INT_CULL, EMF_BG_OVERLAP, EMF_FAR_BOUNDS, EMF_ASYNC_UPLOAD,
                                 EMF_LAMBDA_TABLE, EMF_VOXEL_RCP, EMF_UNSEEN_TILES; demoted: EMF_RAY_FOOTPRINTS, EMF_PEER_FUSED,
                                 EMF_FUSE_POINTS, EMF_FUSE_VISIBILITY, EMF_EARLY_FAR_BOUNDS (x[0] != '0'), EMF_PEER_WAIT_IN_FRONT
    x && x[0] == '1' -> on       EMF_PER_VOLUME, EMF_FORCE_SHARDED; demoted: EMF_OBJ_CULL, EMF_FAR_SCAN
    atoi(x), 1 / 2 / 4 or throw  EMF_MARCH_ROWS
    atoi(x)                      demoted: EMF_TRACK_CHUNK, EMF_TRACK_WINDOW
    max(1, atoi(x))              EMF_PEER_TIMEOUT_MS
    strtoull(x, 0, 10)           EMF_POOL_MIB
    x[0] '2' -> 2, '1' -> 1, 0   demoted: EMF_BRICK_FLAGS
    streamPriority()             demoted: EMF_PRIO_MAIN / COPY / AUX / LISTS: unset or "" -> default; h + 1 -> 1; l - -> -1; else 0
    x != NULL                    demoted: EMF_TRACK_LOG"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
EMF_E_ARG = -4

DEFAULTS = {
    "EMF_PER_VOLUME": 0, "EMF_BG_BANDS": 1, "EMF_INT_CULL": 1, "EMF_BG_OVERLAP": 1, "EMF_FAR_BOUNDS": 1, "EMF_MARCH_ROWS": 1,
    "EMF_ASYNC_UPLOAD": 1, "EMF_LAMBDA_TABLE": 1, "EMF_FORCE_SHARDED": 0, "EMF_VOXEL_RCP": 1, "EMF_UNSEEN_TILES": 1,
    "EMF_POOL_MIB": 16384, "EMF_PEER_TIMEOUT_MS": 5000,
    "EMF_OBJ_CULL": 0, "EMF_TRACK_CHUNK": 8, "EMF_TRACK_WINDOW": 4, "EMF_FUSE_POINTS": 1, "EMF_FUSE_VISIBILITY": 1,
    "EMF_EARLY_FAR_BOUNDS": 1, "EMF_RAY_FOOTPRINTS": 1, "EMF_PEER_FUSED": 1, "EMF_FAR_SCAN": 0, "EMF_BRICK_FLAGS": 0,
    "EMF_PEER_WAIT_IN_FRONT": 1, "EMF_TRACK_LOG": 0, "EMF_PRIO_MAIN": 1, "EMF_PRIO_COPY": 1, "EMF_PRIO_AUX": -1,
    "EMF_PRIO_LISTS": -1,
}
PRODUCT = ["EMF_PER_VOLUME", "EMF_BG_BANDS", "EMF_INT_CULL", "EMF_BG_OVERLAP", "EMF_FAR_BOUNDS", "EMF_MARCH_ROWS",
           "EMF_ASYNC_UPLOAD", "EMF_LAMBDA_TABLE", "EMF_FORCE_SHARDED", "EMF_VOXEL_RCP", "EMF_UNSEEN_TILES", "EMF_POOL_MIB",
           "EMF_PEER_TIMEOUT_MS"]
DEMOTED = [n for n in DEFAULTS if n not in PRODUCT]
OFF_ON_ZERO = ["EMF_BG_BANDS", "EMF_INT_CULL", "EMF_BG_OVERLAP", "EMF_FAR_BOUNDS", "EMF_ASYNC_UPLOAD", "EMF_LAMBDA_TABLE",
               "EMF_VOXEL_RCP", "EMF_UNSEEN_TILES"]
ON_ON_ONE = ["EMF_PER_VOLUME", "EMF_FORCE_SHARDED"]
DBG_OFF_ON_ZERO = ["EMF_FUSE_POINTS", "EMF_FUSE_VISIBILITY", "EMF_EARLY_FAR_BOUNDS", "EMF_RAY_FOOTPRINTS", "EMF_PEER_FUSED",
                   "EMF_PEER_WAIT_IN_FRONT"]
DBG_ON_ON_ONE = ["EMF_OBJ_CULL", "EMF_FAR_SCAN"]
MARCH_MESSAGE = "EMFusion: EMF_MARCH_ROWS=%s (1, 2 or 4 lanes per background ray)"
WARNING = ("emfusion_amd: %s is set, but this build ignores it (a switch whose A/B is on record as lost; "
           "`make -C emfusion_amd/csrc dbg` builds libemf_fusion_dbg.so, which reads it)\n")


def _all(names, text, value):
    return {n: text for n in names}, {n: value for n in names}


# (id, library variant, environment, expected values that differ from DEFAULTS | (error code, message))
CASES = [("defaults", "", {}, {})]
# off only on a leading '0': the documented "0", and the spellings that look like "off" but are not
for text, value in (("0", 0), ("1", 1), ("", 1), ("00", 0), ("no", 1), ("off", 1), ("false", 1), ("0n", 0), (" 0", 1)):
    CASES.append(("lead0 %r" % text, "") + _all(OFF_ON_ZERO, text, value))
    CASES.append(("dbg lead0 %r" % text, "_dbg") + _all(DBG_OFF_ON_ZERO, text, value))
# one variable must not answer for another: alternate the two values over the list, then the other way round
for flip in (0, 1):
    CASES.append(("lead0 alternating %d" % flip, "", {n: str((k + flip) % 2) for k, n in enumerate(OFF_ON_ZERO)},
                  {n: (k + flip) % 2 for k, n in enumerate(OFF_ON_ZERO)}))
# on only on a leading '1'
for text, value in (("1", 1), ("0", 0), ("", 0), ("yes", 0), ("2", 0), ("on", 0), ("true", 0), ("10", 1), ("01", 0)):
    CASES.append(("lead1 %r" % text, "") + _all(ON_ON_ONE, text, value))
    CASES.append(("dbg lead1 %r" % text, "_dbg") + _all(DBG_ON_ON_ONE, text, value))
CASES.append(("lead1 one each", "", {"EMF_PER_VOLUME": "1"}, {"EMF_PER_VOLUME": 1}))
CASES.append(("lead1 the other", "", {"EMF_FORCE_SHARDED": "1"}, {"EMF_FORCE_SHARDED": 1}))
for text in ("1", "2", "4"):
    CASES.append(("march rows %s" % text, "", {"EMF_MARCH_ROWS": text}, {"EMF_MARCH_ROWS": int(text)}))
for text in ("0", "3", "x", "", "8", "-1"):
    CASES.append(("march rows %r refused" % text, "", {"EMF_MARCH_ROWS": text}, (EMF_E_ARG, MARCH_MESSAGE % text)))
for text, value in (("1024", 1024), ("0", 0), ("", 0), ("abc", 0), ("12MiB", 12)):
    CASES.append(("pool %r" % text, "", {"EMF_POOL_MIB": text}, {"EMF_POOL_MIB": value}))
for text, value in (("250", 250), ("60000", 60000), ("0", 1), ("-5", 1), ("abc", 1), ("", 1)):
    CASES.append(("peer timeout %r" % text, "", {"EMF_PEER_TIMEOUT_MS": text}, {"EMF_PEER_TIMEOUT_MS": value}))
for text, value in (("abc", 0), ("", 0), ("0", 0), ("12", 12), ("-3", -3), ("6x", 6)):
    CASES.append(("dbg track %r" % text, "_dbg", {"EMF_TRACK_CHUNK": text, "EMF_TRACK_WINDOW": text},
                  {"EMF_TRACK_CHUNK": value, "EMF_TRACK_WINDOW": value}))
for text, value in (("high", 1), ("+1", 1), ("1", 1), ("normal", 0), ("0", 0), ("low", -1), ("-1", -1), ("", None), ("x", 0)):
    CASES.append(("dbg priorities %r" % text, "_dbg", {n: text for n in DEFAULTS if n.startswith("EMF_PRIO_")},
                  {n: (DEFAULTS[n] if value is None else value) for n in DEFAULTS if n.startswith("EMF_PRIO_")}))
for text, value in (("0", 0), ("1", 1), ("2", 2), ("3", 0), ("", 0), ("21", 2), ("x", 0)):
    CASES.append(("dbg brick flags %r" % text, "_dbg", {"EMF_BRICK_FLAGS": text}, {"EMF_BRICK_FLAGS": value}))
for text in ("1", "0", ""):
    CASES.append(("dbg track log %r" % text, "_dbg", {"EMF_TRACK_LOG": text}, {"EMF_TRACK_LOG": 1}))
# the product build ignores every demoted variable, whatever it says
CASES.append(("demoted ignored", "", {"EMF_OBJ_CULL": "1", "EMF_TRACK_CHUNK": "3", "EMF_TRACK_WINDOW": "0", "EMF_FUSE_POINTS": "0",
                                      "EMF_FUSE_VISIBILITY": "0", "EMF_EARLY_FAR_BOUNDS": "0", "EMF_RAY_FOOTPRINTS": "0",
                                      "EMF_PEER_FUSED": "0", "EMF_FAR_SCAN": "1", "EMF_BRICK_FLAGS": "2",
                                      "EMF_PEER_WAIT_IN_FRONT": "0", "EMF_TRACK_LOG": "1", "EMF_PRIO_MAIN": "low",
                                      "EMF_PRIO_COPY": "low", "EMF_PRIO_AUX": "high", "EMF_PRIO_LISTS": "high"}, {}))
CASES.append(("dbg demoted read", "_dbg", {"EMF_OBJ_CULL": "1", "EMF_FUSE_POINTS": "0", "EMF_PRIO_AUX": "high"},
              {"EMF_OBJ_CULL": 1, "EMF_FUSE_POINTS": 0, "EMF_PRIO_AUX": 1}))

# describe_switches() twice: the second call must neither change a value nor repeat a line on stderr
CHILD = ("import json, sys\nfrom emfusion_amd import pipeline\n"
         "try:\n    first = pipeline.describe_switches()\n    d = pipeline.describe_switches()\n"
         "    assert d == first\n    print(json.dumps(d))\n"
         "except pipeline.FusionError as e:\n    print(json.dumps({'error': e.code, 'message': str(e)}))\n")


def _child(case):
    _, variant, env, _ = case
    clean = {k: v for k, v in os.environ.items() if not k.startswith("EMF_")}
    p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=dict(clean, EMF_FUSION_VARIANT=variant, **env),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.splitlines()[-1]), p.stderr


@pytest.fixture(scope="module")
def answers():
    assert (ROOT / "emfusion_amd" / "libemf_fusion_dbg.so").exists(), "built by __graft_entry__.build() (make dbg)"
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(zip((c[0] for c in CASES), pool.map(_child, CASES)))


def test_the_case_ids_are_unique():
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_table_parses_as_the_call_sites_did(answers, case):
    name, variant, env, want = case
    got, stderr = answers[name]
    if isinstance(want, tuple):
        assert got.get("error") == want[0] and want[1] in got["message"], got
        return
    assert sorted(got) == sorted(DEFAULTS), sorted(set(got) ^ set(DEFAULTS))  # every row, no other
    assert {n: row["value"] for n, row in got.items()} == dict(DEFAULTS, **want)
    assert {n: row["default"] for n, row in got.items()} == DEFAULTS
    assert {n for n, row in got.items() if row["kind"] == "product"} == set(PRODUCT)
    assert {n for n, row in got.items() if row["kind"] == "demoted"} == set(DEMOTED)
    for n, row in got.items():  # the product build reads the product rows only, the debug build all of them
        assert row["read"] is (variant == "_dbg" or n in PRODUCT), (n, row)
        assert row["doc"]
    # one line per demoted variable that is set, once, from the product build only
    for n in DEFAULTS:
        assert stderr.count(WARNING % n) == (1 if n in env and n in DEMOTED and variant == "" else 0), (n, stderr)


def test_every_path_selecting_product_switch_has_a_pair_test(answers):
    """a switch added to the table as selecting an execution path must be added to the pair test's list too"""
    from tests import test_gpu_switch_pairs
    got, _ = answers["defaults"]
    selecting = {n for n, row in got.items() if row["kind"] == "product" and row["path"] and row["type"] in ("on/off", "enumerated")}
    assert selecting == {"EMF_PER_VOLUME", "EMF_INT_CULL", "EMF_LAMBDA_TABLE", "EMF_VOXEL_RCP", "EMF_BG_OVERLAP", "EMF_FAR_BOUNDS",
                         "EMF_UNSEEN_TILES", "EMF_MARCH_ROWS"}
    assert selecting <= {name for name, _ in test_gpu_switch_pairs.SWITCHES}
