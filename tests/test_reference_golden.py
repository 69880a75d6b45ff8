"""Committed outputs of the REFERENCE'S OWN kernels (tests/golden/reference_v1.npz, made by
tests/golden/make_reference_golden.py from the reference's device code built for the host) --
CPU only, never skipped, needs neither the reference checkout nor oracle/_ref/.

  inputs : tests/reference_cases.py regenerates every input to the recorded SHA-256; this pins
           tests/scenes.py and numpy's generators against drift
  oracle : oracle/emf_oracle.c reproduces every recorded reference output, digest for digest, and
           array for array where the whole array is recorded (so a failure shows where)

The HIP kernels meet the same file in tests/test_gpu_reference_pinned.py.
"""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import reference_cases as rc
from tests.parity_util import assert_parity

GOLD = Path(__file__).resolve().parent / "golden" / "reference_v1.npz"


@pytest.fixture(scope="module")
def gold():
    data = dict(np.load(GOLD))
    return json.loads(str(data.pop("digests"))), data


def test_file_is_what_the_generator_documents(gold):
    digests, arrays = gold
    assert set(digests) == set(rc.CASES), "cases recorded != cases defined: regenerate the file"
    assert GOLD.stat().st_size <= 512 * 1024
    for name, case in rc.CASES.items():
        assert digests[name]["kind"] == case.kind
        recorded = {k.split("/", 1)[1] for k in arrays if k.startswith(name + "/")}
        assert recorded == (set(digests[name]["outputs"]) if case.small else set()), name
        for key in recorded:
            assert rc.digest(arrays[f"{name}/{key}"]) == digests[name]["outputs"][key], (name, key)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_inputs_regenerate_and_oracle_reproduces_the_reference(oracle, gold, name):
    digests, arrays = gold
    case, rec = rc.CASES[name], digests[name]
    inp = case.inputs()
    assert {k: rc.digest(v) for k, v in inp.items()} == rec["inputs"], "the inputs drifted"
    out = rc.RUN[case.kind](oracle, inp)
    assert set(out) == set(rec["outputs"])
    for key, got in out.items():
        if case.small:
            assert_parity(got, arrays[f"{name}/{key}"], f"{name}: {key}", exact=True)
        assert rc.digest(got) == rec["outputs"][key], f"{name}: {key} is not what the reference gives"
    case.check(inp, out)
