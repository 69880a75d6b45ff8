"""The restatement of the object shapes (tests/shape_reference.py) checked without a device: the two
statements of the moments agree; every solid voxel projects into the extents; the host-only entries
emf_fusion_shape_frame and emf_fusion_shape_box equal the restatement bit for bit on every fixture; the frame is
orthonormal, right-handed, sorted and signed by the rule; it agrees with numpy.linalg.eigh within 16 x the differences
measured here; the sweep count is the measured one plus two; and the structs of the header have the sizes of the numpy
dtypes."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import shape_reference as sr

ROOT = Path(__file__).resolve().parent.parent
LOOP_SHAPES = [s for s in sr.SHAPES if s[0] * s[1] * s[2] <= 5000]  # the plain loop on the small shapes
# measured over the fixtures of this file (numpy 2 / OpenBLAS LAPACK, x86-64): the worst |eigenvalue difference| / trace
# and, for axes whose eigenvalue is more than 1e-6 of the trace from its neighbours, the worst 1 - |dot|.  The test
# allows 16 x these, as a margin for another libm or LAPACK.
EIGH_VALUE_MEASURED = 2.5909347262213904e-16
EIGH_AXIS_MEASURED = 6.661338147750939e-16


@pytest.fixture(scope="module")
def records():
    """[(name, tsdf, weights, fg, moments, frame)] of every fixture, computed once."""
    out = []
    for name, tsdf, weights, fg in sr.cases():
        mom = sr.moments(tsdf, weights, fg)
        out.append((name, tsdf, weights, fg, mom, sr.frame(mom)))
    return out


def big_moments():
    """The record of a 128^3 all-solid volume in closed form: the sums pass 2^32."""
    n = 128
    s1, s2 = sum(range(n)), sum(i * i for i in range(n))
    m = np.zeros((), sr.MOMENTS)
    m["solid"] = m["observed"] = n ** 3
    m["sum"] = [s1 * n * n] * 3
    m["sum2"] = [s2 * n * n] * 3 + [s1 * s1 * n] * 3
    m["faces_free"], m["faces_unknown"], m["lo"], m["hi"] = 0, 0, 0, n - 1
    return m


@pytest.mark.parametrize("shape", LOOP_SHAPES)
def test_the_two_statements_of_the_moments_agree(shape):
    for content in sr.CONTENTS:
        tsdf, weights, fg = sr.volume(shape, content)
        for mask in (fg, None):
            a, b = sr.moments(tsdf, weights, mask), sr.moments_loop(tsdf, weights, mask)
            assert a.tobytes() == b.tobytes(), (shape, content, mask is not None, a, b)


def test_the_fixtures_cover_what_they_are_for(records):
    by = {name: mom for name, _, _, _, mom, _ in records}
    assert all(int(by[f"{s}-unobserved-nofg"]["observed"]) == 0 and tuple(by[f"{s}-unobserved-nofg"]["lo"]) == s
               for s in sr.SHAPES)
    assert all(int(by[f"{s}-all_solid-nofg"]["solid"]) == s[0] * s[1] * s[2] for s in sr.SHAPES)
    assert all(int(by[f"{s}-corner-fg"]["solid"]) == 1 and tuple(by[f"{s}-corner-fg"]["lo"]) == tuple(v - 1 for v in s)
               for s in sr.SHAPES)
    big = by["(40, 24, 20)-gated_block-fg"], by["(40, 24, 20)-gated_block-nofg"]
    assert 0 < int(big[0]["solid"]) < int(big[1]["solid"]) <= 2 * int(big[0]["solid"]) + 1  # the mask gates half
    shell = by["(40, 24, 20)-half_shell-nofg"]
    assert int(shell["faces_free"]) > 0 and int(shell["faces_unknown"]) > 0 and int(shell["solid"]) < int(shell["observed"])
    rnd = by["(33, 17, 9)-random-nofg"]
    assert int(rnd["solid"]) > 0 and int(rnd["faces_free"]) > 0 and int(rnd["faces_unknown"]) > 0
    assert int(big_moments()["sum2"][0]) == 11319377920 > 2 ** 32


def test_every_solid_voxel_projects_into_the_extents(records):
    seen = 0
    for name, tsdf, weights, fg, mom, fr in records:
        shape = tsdf.shape[::-1]
        for axes in (sr.axes_for(mom, shape), sr.skew_axes(shape)):
            e, ext = sr.projections(tsdf, weights, fg, axes), sr.extents(tsdf, weights, fg, axes)
            if len(e) == 0:
                assert np.isposinf(ext["lo"]).all() and np.isneginf(ext["hi"]).all(), name
                continue
            assert (e >= ext["lo"]).all() and (e <= ext["hi"]).all(), name
            assert (e.min(axis=0) == ext["lo"]).all() and (e.max(axis=0) == ext["hi"]).all(), name  # finite: float order
            seen += 1
    assert seen > 100


def test_the_key_map_preserves_the_float_order():
    v = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    k = sr.float_keys(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert sr.key_floats(k).tobytes() == v.tobytes()
    assert int(k[-1]) == 0xff800000 and int(k[0]) == 0x007fffff


def test_shape_frame_equals_the_restatement_bit_for_bit(records):
    from emfusion_amd import pipeline
    valid = 0
    for name, _, _, _, mom, fr in records + [("128^3", None, None, None, big_moments(), sr.frame(big_moments()))]:
        got = pipeline.shape_frame(mom)
        assert got.dtype == sr.FRAME and got.tobytes() == fr.tobytes(), (name, got, fr)
        valid += int(fr["valid"])
    assert valid >= 60
    empty = pipeline.shape_frame(np.zeros((), sr.MOMENTS))
    assert int(empty["valid"]) == 0 and empty.tobytes() == np.zeros((), sr.FRAME).tobytes()


def test_shape_box_equals_the_restatement_bit_for_bit(records):
    from emfusion_amd import pipeline
    R = sr.skew_axes((3, 3, 3))["A"]  # a rotation, f32
    t = np.array([0.25, -1.5, 0.75], np.float32)
    checked = 0
    for name, tsdf, weights, fg, mom, fr in records:
        if not int(fr["valid"]):
            continue
        res = tsdf.shape[::-1]
        ext = sr.extents(tsdf, weights, fg, fr["f32"])
        want = sr.box(mom, fr, ext, res, 0.0123, R, t)
        got = pipeline.shape_box(mom, fr, ext, res, 0.0123, R, t)
        assert got.tobytes() == want.tobytes(), (name, got, want)
        # what the box is for: every solid voxel's centre lies inside it (half a voxel cube is added per axis)
        z, y, x = np.nonzero(sr.solid_mask(tsdf, weights, fg))
        d = np.stack([x, y, z], axis=1) - want["center_vox"]
        along = d @ fr["axes"].reshape(3, 3).T
        assert (np.abs(along) <= want["half_vox"] + 1e-4).all(), name
        faces = int(mom["faces_free"]) + int(mom["faces_unknown"])
        assert np.isnan(want["completeness"]) if faces == 0 else want["completeness"] == int(mom["faces_free"]) / faces
        checked += 1
    assert checked >= 60


def test_the_frame_is_orthonormal_right_handed_sorted_and_signed(records):
    for name, _, _, _, mom, fr in records:
        if not int(fr["valid"]):
            continue
        A, ev = fr["axes"].reshape(3, 3), fr["eigenvalues"]
        assert np.abs(A @ A.T - np.eye(3)).max() < 1e-14, name
        assert np.linalg.det(A) > 0.999999 and np.abs(np.cross(A[0], A[1]) - A[2]).max() == 0.0, name
        assert ev[0] >= ev[1] >= ev[2] and ev[2] > -1e-9 * max(ev[0], 1.0), name
        for k in (0, 1):  # the component of largest magnitude, ties to the lowest index, is positive
            assert A[k][int(np.argmax(np.abs(A[k])))] > 0, name
        assert (fr["f32"]["A"] == fr["axes"].astype(np.float32)).all() and (fr["f32"]["c"] == fr["centroid"].astype(np.float32)).all()
        assert np.abs(fr["centroid"] - mom["sum"].astype(np.float64) / float(mom["solid"])).max() == 0.0


def test_the_frame_agrees_with_eigh(records):
    worst_value = worst_axis = 0.0
    for name, _, _, _, mom, fr in records:
        if not int(fr["valid"]):
            continue
        C = fr["covariance"]
        S = np.array([[C[0], C[3], C[4]], [C[3], C[1], C[5]], [C[4], C[5], C[2]]])
        trace = np.trace(S)
        if trace == 0:
            continue
        ev, vec = np.linalg.eigh(S)
        ev, vec = ev[::-1], vec[:, ::-1]
        worst_value = max(worst_value, np.abs(ev - fr["eigenvalues"]).max() / trace)
        A = fr["axes"].reshape(3, 3)
        for k in range(3):
            if min(abs(ev[k] - ev[j]) for j in range(3) if j != k) > 1e-6 * trace:
                worst_axis = max(worst_axis, 1.0 - abs(A[k] @ vec[:, k]))
    print(f"eigh: worst |eigenvalue difference| / trace {worst_value!r}, worst 1 - |dot| {worst_axis!r}")
    assert worst_value <= 16 * EIGH_VALUE_MEASURED and worst_axis <= 16 * EIGH_AXIS_MEASURED


def test_the_sweep_count_is_the_measured_one_plus_two(records):
    worst = max(sr.sweeps_to_settle(mom) for _, _, _, _, mom, fr in records if int(fr["valid"]))
    worst = max(worst, sr.sweeps_to_settle(big_moments()))
    print(f"jacobi: the slowest fixture settles after {worst} sweeps")
    assert sr.SWEEPS == worst + 2
    for _, _, _, _, mom, fr in records:  # ... so two more sweeps change no bit
        if int(fr["valid"]):
            assert sr.frame(mom, sr.SWEEPS + 2).tobytes() == fr.tobytes()


def header_struct_size(text, name):
    """sizeof of a struct of the header whose fields are naturally aligned scalars, arrays of them or such structs."""
    sizes = {"uint64_t": 8, "int32_t": 4, "uint32_t": 4, "float": 4, "double": 8,
             "emf_shape_axes_t": 48}
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    total = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind, names = decl.split(None, 1)
        for field in names.split(","):
            dims = re.findall(r"\[(\d+)\]", field)
            total += sizes[kind] * int(np.prod([int(d) for d in dims])) if dims else sizes[kind]
    return total


def test_struct_sizes_dtypes_and_entries():
    import ctypes as C

    from emfusion_amd import _lib, pipeline
    hip_h = (ROOT / "include" / "emf_hip.h").read_text()
    fusion_h = (ROOT / "include" / "emf_fusion.h").read_text()
    assert int(re.search(r"#define\s+EMF_HIP_ABI_VERSION\s+(\d+)", hip_h).group(1)) == 8
    assert int(re.search(r"#define\s+EMF_SHAPE_JACOBI_SWEEPS\s+(\d+)", hip_h).group(1)) == sr.SWEEPS == _lib.SHAPE_JACOBI_SWEEPS
    for name, dtype, mine, size in (("emf_shape_moments", _lib.SHAPE_MOMENTS_DTYPE, sr.MOMENTS, 128),
                                    ("emf_shape_axes", _lib.SHAPE_AXES_DTYPE, sr.AXES, 48),
                                    ("emf_shape_extents", _lib.SHAPE_EXTENTS_DTYPE, sr.EXTENTS, 24),
                                    ("emf_shape_frame", _lib.SHAPE_FRAME_DTYPE, sr.FRAME, 224),
                                    ("emf_shape_box", _lib.SHAPE_BOX_DTYPE, sr.BOX, 584)):
        assert header_struct_size(hip_h, name) == np.dtype(dtype).itemsize == mine.itemsize == size, name
        assert np.dtype(dtype) == mine, name
    assert C.sizeof(_lib.EmfShapeMoments) == 128 and C.sizeof(_lib.EmfShapeAxes) == 48 and C.sizeof(_lib.EmfShapeExtents) == 24
    declared = _lib.declared_symbols()
    lib, fus = _lib.load(), pipeline.load()
    assert lib.emf_hip_abi_version() == 8
    for name, nargs in (("emf_hip_shapeMoments", 6), ("emf_hip_shapeExtents", 7)):
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs
        getattr(lib, name)
    for name in ("emf_fusion_object_shapes", "emf_fusion_shape_frame", "emf_fusion_shape_box", "emf_fusion_set_shape_output"):
        assert name in pipeline.declared_symbols() and name in fusion_h and name in fus._emf_sigs
        getattr(fus, name)
    # said honestly from the start: the band is measured, not the body
    assert "OBSERVED SOLID BAND, NOT THE BODY" in hip_h and "NOT THE BODY" in fusion_h
    assert "NOT THE BODY" in pipeline.Fusion.object_shapes.__doc__
