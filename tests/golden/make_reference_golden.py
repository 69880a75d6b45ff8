"""Writes tests/golden/reference_v1.npz: what the REFERENCE'S OWN kernels, built for the host
(oracle/build_ref.py -> oracle/_ref/libemf_ref.so), give on the cases of tests/reference_cases.py.

Unlike the other vectors in this directory these are not outputs of this repository's oracle: the
code that produced them is the reference's, compiled unchanged apart from the launch syntax
(IEEE single precision, no a*b+c contraction).  Data only: for every case a SHA-256 of each input
array and of each output array (tests.reference_cases.digest: NaNs and signed zeros canonical, as
assert_parity(exact=True) compares), and the whole output arrays of the small cases so that a
failure can show where.  Inputs are not stored: every test regenerates them and checks the digest.

Needs a checkout of the reference (EMF_REFERENCE_DIR).  Run from the repository root:
    python -m tests.golden.make_reference_golden
"""
import json
from pathlib import Path

import numpy as np

from oracle import build_ref, ref_binding
from tests import reference_cases as rc

OUT = Path(__file__).resolve().parent / "reference_v1.npz"
LIMIT = 512 * 1024


def main():
    if not ref_binding.available():
        assert build_ref.build(), "no reference checkout: set EMF_REFERENCE_DIR"
    arrays, digests = {}, {}
    for name, case in rc.CASES.items():
        inp = case.inputs()
        out = rc.RUN[case.kind](ref_binding, inp)
        case.check(inp, out)
        digests[name] = dict(kind=case.kind,
                             inputs={k: rc.digest(v) for k, v in inp.items()},
                             outputs={k: rc.digest(v) for k, v in out.items()})
        if case.small:
            for k, v in out.items():
                arrays[f"{name}/{k}"] = rc.canonical(v)
    arrays["digests"] = np.array(json.dumps(digests, sort_keys=True))
    np.savez_compressed(OUT, **arrays)
    size = OUT.stat().st_size
    biggest = max(p.stat().st_size for p in OUT.parent.glob("*.npz") if p != OUT)
    assert size <= LIMIT and size < biggest, (size, LIMIT, biggest)
    print(f"{OUT.name}: {len(digests)} cases, {len(arrays) - 1} arrays, {size} bytes")


if __name__ == "__main__":
    main()
