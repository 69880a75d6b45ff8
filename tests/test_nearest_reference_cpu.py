"""The nearest-site restatement (tests/nearest_reference.py) against itself -- all pairs equals the separable passes,
the index reproduces scipy's squared distance, the fixtures can see the early-stop bug -- and the argument checks of
emf_hip_distanceTransformNearest / emf_hip_distanceQuery, which reject before any launch and so need no device
(include/emf_hip.h "Distance field")."""
import ctypes as C

import numpy as np
import pytest

from emfusion_amd import _lib
from tests import distance_reference as dr
from tests import nearest_reference as nr

E_ARG, E_LIMIT = -4, -5
P, Q, R = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(12288)  # non-NULL, aligned, never dereferenced


def i3(*v):
    return (C.c_int32 * 3)(*v)


SMALL = [s for s in dr.SHAPES if int(np.prod(s)) <= dr.BRUTE_LIMIT]
TIE_CASES = [(c, s) for c in nr.TIE_CONTENTS for s in nr.TIE_SHAPES[c]]


def ident(s):
    return "x".join(str(v) for v in s)


@pytest.mark.parametrize("content", dr.CONTENTS)
@pytest.mark.parametrize("shape", SMALL, ids=ident)
def test_all_pairs_equals_the_separable_passes(shape, content):
    sites = dr.site_field(shape, content, seed=11)
    for cap in (0, 1, 5):
        b2, bn = nr.nearest_brute(sites, cap)
        s2, sn = nr.nearest_separable(sites, cap)
        assert b2.tobytes() == s2.tobytes() and bn.tobytes() == sn.tobytes(), (shape, content, cap)
        assert bn.dtype == np.int32


def test_all_pairs_equals_the_separable_passes_on_random_boxes():
    rng = np.random.default_rng(2121)
    for k in range(40):
        shape = tuple(int(v) for v in rng.integers(1, 9, 3))
        sites = rng.random(shape) < rng.choice([0.05, 0.2, 0.5])
        for cap in (0, 2):
            b2, bn = nr.nearest_brute(sites, cap)
            s2, sn = nr.nearest_separable(sites, cap)
            assert b2.tobytes() == s2.tobytes() and bn.tobytes() == sn.tobytes(), (k, shape, cap)


@pytest.mark.parametrize("case", TIE_CASES, ids=lambda c: c[0] + "-" + ident(c[1]))
def test_tie_contents(case):
    content, shape = case
    sites = nr.tie_field(shape, content)
    for cap in (0, 5):
        d2, near = nr.nearest_separable(sites, cap)
        nr.check_against_d2(sites, d2, near, cap)
        if sites.size <= dr.BRUTE_LIMIT:
            b2, bn = nr.nearest_brute(sites, cap)
            assert b2.tobytes() == d2.tobytes() and bn.tobytes() == near.tobytes(), (content, shape, cap)


@pytest.mark.parametrize("content", ["none", "far_corner", "p01", "p50", "all"])
@pytest.mark.parametrize("shape", dr.SHAPES, ids=ident)
def test_the_index_reproduces_the_squared_distance(shape, content):
    sites = dr.site_field(shape, content, seed=11)
    for cap in (0, 5):
        d2, near = nr.nearest_separable(sites, cap)
        nr.check_against_d2(sites, d2, near, cap)


def test_values_by_hand():
    sites = nr.tie_field((9, 9, 9), "octa")
    d2, near = nr.nearest_separable(sites)
    lin = nr.linear_index(sites.shape)
    assert d2[4, 4, 4] == 16 and near[4, 4, 4] == lin[0, 4, 4]  # six equally near: the smallest z' wins
    assert near[4, 4, 5] == lin[4, 4, 8] and near[4, 5, 4] == lin[4, 8, 4]
    assert near[4, 3, 3] == lin[4, 0, 4]  # (y 0) and (x 0) tie at 9 + 1: the smaller linear index is the smaller y'
    c2, cn = nr.nearest_separable(nr.tie_field((11, 11, 11), "octa"), cap=5)  # all six at exactly the cap
    assert c2[5, 5, 5] == 25 and cn[5, 5, 5] == 5 * 11 + 5 and cn[5, 5, 4] == (5 * 11 + 5) * 11
    assert c2[0, 0, 0] == dr.FAR and cn[0, 0, 0] == nr.NONE  # 50 > 25
    rows = nr.tie_field((1, 1, 65), "row_ends")
    assert nr.nearest_separable(rows)[1][0, 0, 31:34].tolist() == [0, 0, 64]  # the middle of the row goes left


def test_the_fixtures_see_the_early_stop():
    """A scan that stops at d * d >= best gives the right d2 and the wrong index: the octahedron's centre shows it."""
    sites = nr.tie_field((9, 9, 9), "octa")
    want2, want = nr.nearest_brute(sites)
    good2, good = nr.nearest_by_scan(sites, early_stop=False)
    assert good2.tobytes() == want2.tobytes() and good.tobytes() == want.tobytes()
    bad2, bad = nr.nearest_by_scan(sites, early_stop=True)
    assert bad2.tobytes() == want2.tobytes()
    assert bad[4, 4, 4] != want[4, 4, 4] and (bad != want).sum() > 1
    assert sites.reshape(-1)[bad.reshape(-1)].all()  # still a site at the right distance: only the tie rule is broken
    rng = np.random.default_rng(77)
    wrong = 0
    for _ in range(12):
        s = rng.random(tuple(int(v) for v in rng.integers(3, 9, 3))) < 0.2
        wrong += int((nr.nearest_by_scan(s, True)[1] != nr.nearest_brute(s)[1]).any())
        assert nr.nearest_by_scan(s, False)[1].tobytes() == nr.nearest_brute(s)[1].tobytes()
    assert wrong > 0


def test_header_declares_and_library_exports_the_new_entries():
    lib = _lib.load()
    for name in ("emf_hip_distanceTransformNearest", "emf_hip_nearestSiteScratchBytes", "emf_hip_distanceQuery"):
        assert name in _lib.declared_symbols() and name in _lib.SIGNATURES
        getattr(lib, name)
    assert _lib.DF_NONE == -1
    assert lib.emf_hip_nearestSiteScratchBytes(i3(5, 6, 7)) == 4 * 5 * 6 * 7
    assert lib.emf_hip_nearestSiteScratchBytes(i3(2049, 1, 1)) == 0
    assert lib.emf_hip_nearestSiteScratchBytes(i3(2048, 2048, 512)) == 0
    assert lib.emf_hip_nearestSiteScratchBytes(i3(4, 0, 4)) == 0


def test_nearest_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    size = i3(16, 16, 16)
    f = lib.emf_hip_distanceTransformNearest
    assert f(P, size, 2, 0, Q, None, None, R, 0.0, None) == E_ARG
    assert b"nearest or scratch is NULL" in lib.emf_hip_last_error_string()
    assert f(P, size, 2, 0, Q, None, R, None, 0.0, None) == E_ARG
    assert b"nearest or scratch is NULL" in lib.emf_hip_last_error_string()
    assert f(P, size, 2, 0, Q, None, C.c_void_p(4098), R, 0.0, None) == E_ARG
    assert f(P, size, 2, 0, Q, None, R, C.c_void_p(4097), 0.0, None) == E_ARG
    assert b"misaligned" in lib.emf_hip_last_error_string()
    assert f(P, size, 2, 0, Q, None, R, R, 0.0, None) == E_ARG  # no pass may read the index array it writes
    assert f(P, size, 2, 0, Q, None, Q, R, 0.0, None) == E_ARG
    # and everything the plain entry refuses
    assert f(None, size, 2, 0, Q, None, R, P, 0.0, None) == E_ARG
    assert f(P, size, 2, 0, None, None, R, Q, 0.0, None) == E_ARG
    assert f(P, None, 2, 0, Q, None, R, P, 0.0, None) == E_ARG
    assert f(P, i3(16, 0, 16), 2, 0, Q, None, R, P, 0.0, None) == E_ARG
    assert f(P, i3(2049, 1, 1), 2, 0, Q, None, R, P, 0.0, None) == E_LIMIT
    assert f(P, i3(2048, 2048, 512), 2, 0, Q, None, R, P, 0.0, None) == E_LIMIT
    assert f(P, size, 0, 0, Q, None, R, P, 0.0, None) == E_ARG
    assert f(P, size, 8, 0, Q, None, R, P, 0.0, None) == E_ARG
    assert f(P, size, 2, -1, Q, None, R, P, 0.0, None) == E_ARG
    assert f(P, size, 2, 0, Q, P, R, C.c_void_p(16384), 0.0, None) == E_ARG  # metres need a voxel size


def test_query_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    size = i3(16, 16, 16)
    f = lib.emf_hip_distanceQuery
    assert f(P, None, None, None, Q, 4, R, None, None, None) == E_ARG
    assert f(P, None, None, size, None, 4, R, None, None, None) == E_ARG
    assert f(P, None, None, size, Q, -1, R, None, None, None) == E_ARG
    assert f(P, None, None, size, Q, 4, None, None, None, None) == E_ARG  # an input without its output
    assert f(None, None, None, size, Q, 4, R, None, None, None) == E_ARG  # an output without its input
    assert f(None, P, None, size, Q, 4, None, None, None, None) == E_ARG
    assert f(None, None, P, size, Q, 4, None, R, None, None) == E_ARG
    assert b"go together" in lib.emf_hip_last_error_string()
    assert f(None, C.c_void_p(4098), None, size, Q, 4, None, R, None, None) == E_ARG
    assert f(P, None, None, i3(2049, 1, 1), Q, 4, R, None, None, None) == E_LIMIT
    assert f(P, None, None, size, Q, 0, R, None, None, None) == 0  # no points: nothing is launched
    assert f(None, None, None, size, Q, 4, None, None, None, None) == 0  # nothing to read: nothing is launched


def test_the_plain_entry_refuses_exactly_as_before():
    lib = _lib.load()
    size = i3(16, 16, 16)
    f = lib.emf_hip_distanceTransform
    assert f(P, size, 2, 0, None, None, 0.0, None) == E_ARG
    assert lib.emf_hip_last_error_string() == b"distanceTransform: classes, d2 or size is NULL"
    assert f(P, size, 9, 0, Q, None, 0.0, None) == E_ARG
    assert lib.emf_hip_last_error_string() == b"distanceTransform: site_mask 9 outside 1 .. 7"
    assert f(P, size, 2, -2, Q, None, 0.0, None) == E_ARG
    assert lib.emf_hip_last_error_string() == b"distanceTransform: cap -2"
    assert f(P, size, 2, 0, C.c_void_p(4098), None, 0.0, None) == E_ARG
    assert lib.emf_hip_last_error_string() == b"distanceTransform: misaligned arrays"
    assert f(P, i3(2049, 1, 1), 2, 0, Q, None, 0.0, None) == E_LIMIT
    assert lib.emf_hip_last_error_string() == b"distanceTransform: box axis 0 has 2049 voxels, above 2048"
