"""The restatement of the ground map (tests/ground_reference.py) checked without a device: the two
statements of the bit planes agree; the host-only entry emf_fusion_ground_frame equals pipeline.ground_frame and the
restatement bit for bit on every fixture; the frame is orthonormal and right-handed; slots of two and three voxels leave
no hole in a rotated lattice and slots of one voxel do; with up along a signed box axis the planes are a transpose, a
flip and an any-reduction of the class volume; standable levels, headroom and the step rule hold on hand-made columns
and maps; and the structs of the header have the sizes of the numpy dtypes."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import ground_reference as rf

ROOT = Path(__file__).resolve().parent.parent
LOOP_SHAPES = [s for s in rf.SHAPES if s[0] * s[1] * s[2] <= 5000]
LOOP_SPECS = [("axis", 2, 1, 1), ("axis", 0, -1, 2), ("axis", 1, 1, 3), ("tilt20", 2), ("generic", 3), ("outside",), ("nan",)]


@pytest.mark.parametrize("shape", LOOP_SHAPES)
def test_the_two_statements_of_the_planes_agree(shape):
    for k, spec in enumerate(LOOP_SPECS):
        G, W, H, B = rf.spec_frame(shape, spec, rf.BINS[k % len(rf.BINS)])
        for content in ("random", "scene", "bytes_above_2"):
            v = rf.volume(shape, content)
            a, b = rf.planes(v, G, W, H, B), rf.planes_loop(v, G, W, H, B)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (shape, spec, content)
            if spec[0] in ("outside", "nan"):
                assert not a[0].any() and not a[1].any(), (shape, spec)


# ---- the frame ------------------------------------------------------------------------------------------------------

def frame_fixtures():
    """[(lo, size, res, voxel, R, t, up, cell, bin, ref, band)]"""
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    rng = np.random.default_rng(5)
    out = []
    for k, s in rf.AXES:  # the six signed axes; up along x takes the z axis for u
        up = [0.0, 0.0, 0.0]
        up[k] = float(s)
        out.append(((0, 0, 0), (40, 24, 16), (40, 24, 16), 1.0, eye, zero, up, 1.0, 1.0, (0, 0, 0), (-8.0, 8.0)))
        out.append(((3, 1, 2), (33, 9, 8), (64, 32, 16), 0.02, eye, zero, up, 0.04, 0.06, (0.1, 0.0, -0.1), (-0.3, 0.31)))
    for n in range(12):  # generic poses, ups, boxes
        R = rf.rotation(rng.normal(size=3), rng.uniform(0, 180)).astype(np.float32)
        t = rng.normal(size=3).astype(np.float32)
        res = tuple(int(v) for v in rng.integers(8, 200, 3))
        size = tuple(int(rng.integers(1, r + 1)) for r in res)
        lo = tuple(int(rng.integers(0, r - s + 1)) for r, s in zip(res, size))
        voxel = float(rng.uniform(0.005, 0.1))
        out.append((lo, size, res, voxel, R, t, rng.normal(size=3), voxel * rng.uniform(1, 4), voxel * rng.uniform(1, 4),
                    rng.normal(size=3), (-rng.uniform(0.1, 2), rng.uniform(0.1, 1))))
    # the camera convention of the sessions: up = minus the background's y axis
    R = rf.rotation((1, 0.2, 0), 25.0).astype(np.float32)
    out.append(((0, 0, 0), (512, 512, 512), (512, 512, 512), 0.01, R, zero, -R[:, 1].astype(np.float64), 0.02, 0.02,
                (0.0, 0.3, 0.0), (-1.5, 0.5)))
    return out


def c_frame(fx):
    from emfusion_amd import pipeline
    lo, size, res, voxel, R, t, up, cell, bin, ref, band = fx
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    f = lambda v, n: (C.c_float * n)(*[float(x) for x in np.asarray(v, np.float32).reshape(-1)])
    up, ref = np.ascontiguousarray(up, np.float64), np.ascontiguousarray(ref, np.float64)
    frame, pose = np.zeros(15, np.int32), np.zeros(12, np.float64)
    rc = pipeline.load().emf_fusion_ground_frame(i3(lo), i3(size), i3(res), float(voxel), f(R, 9), f(t, 3), up.ctypes.data,
                                                 float(cell), float(bin), ref.ctypes.data, float(band[0]), float(band[1]),
                                                 frame.ctypes.data, pose.ctypes.data)
    return rc, frame[:12].view(np.float32).reshape(3, 4).copy(), int(frame[12]), int(frame[13]), int(frame[14]), pose


@pytest.mark.parametrize("k", range(len(frame_fixtures())))
def test_the_frame_entry_the_numpy_frame_and_the_restatement_agree_bit_for_bit(k):
    from emfusion_amd import pipeline
    fx = frame_fixtures()[k]
    rc, G, W, H, B, pose = c_frame(fx)
    assert rc == 0
    mine = rf.frame(*fx)
    theirs = pipeline.ground_frame(*fx)
    for other in (mine, theirs):
        assert other[0].dtype == np.float32 and other[0].tobytes() == G.tobytes(), (other[0], G)
        assert tuple(other[1:4]) == (W, H, B)
        assert np.asarray(other[4], np.float64).tobytes() == pose.tobytes(), (other[4], pose)
    # orthonormal and right-handed; h is up
    R = pose[:9].reshape(3, 3)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
    up = np.asarray(fx[6], np.float64)
    assert np.abs(R[:, 2] - up / np.linalg.norm(up)).max() < 1e-15
    assert np.abs(np.cross(R[:, 2], R[:, 0]) - R[:, 1]).max() < 1e-15  # v = h x u
    # every voxel of the box lands inside the map, and the corners of the box reach its first and last cell
    lo, size = fx[0], fx[1]
    corners = np.array([[(size[a] - 0.5) if (c >> a) & 1 else -0.5 for a in range(3)] for c in range(8)])
    q = corners @ G[:2, :3].astype(np.float64).T + G[:2, 3]
    assert q.min() > -1e-3 and (np.floor(q.max(axis=0) - 1e-3) < (W, H)).all()
    assert (q.min(axis=0) < 1e-3).all() and (q.max(axis=0) > np.array([W, H]) - 1 - 1e-3).all()


def test_the_frame_refuses_what_it_cannot_answer():
    from emfusion_amd import pipeline
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    good = [(0, 0, 0), (40, 24, 16), (40, 24, 16), 1.0, eye, zero, (0.0, 0.0, 1.0), 1.0, 1.0, (0, 0, 0), (-8.0, 8.0)]

    def with_(**kw):
        names = ["lo", "size", "res", "voxel", "R", "t", "up", "cell", "bin", "ref", "band"]
        fx = list(good)
        for key, value in kw.items():
            fx[names.index(key)] = value
        return tuple(fx)

    for fx, code in ((with_(up=(0.0, 0.0, 0.0)), rf.E_ARG), (with_(up=(0.0, np.nan, 1.0)), rf.E_ARG),
                     (with_(up=(0.0, np.inf, 1.0)), rf.E_ARG), (with_(cell=0.0), rf.E_ARG), (with_(bin=-1.0), rf.E_ARG),
                     (with_(band=(0.5, 0.5)), rf.E_ARG), (with_(ref=(0.0, np.nan, 0.0)), rf.E_ARG),
                     (with_(band=(-8.0, 248.5)), rf.E_LIMIT), (with_(size=(2048, 24, 16), res=(2048, 24, 16)), rf.E_LIMIT),
                     (with_(cell=0.01), rf.E_LIMIT)):
        rc = c_frame(fx)[0]
        assert rc == code, (fx, rc)
        with pytest.raises(rf.FrameError) as e:
            rf.frame(*fx)
        assert e.value.code == code
        with pytest.raises(ValueError):
            pipeline.ground_frame(*fx)
    # 256 bins and 2048 cells are taken: 2047 voxels at a cell of one open 2048 cells
    assert c_frame(with_(band=(-8.0, 248.0)))[4] == 256
    assert c_frame(with_(size=(2047, 24, 16), res=(2047, 24, 16)))[2] == 2048
    # x along up: u comes from the background's z axis
    rc, G, W, H, B, pose = c_frame(with_(up=(1.0, 0.0, 0.0)))
    assert rc == 0 and np.abs(pose[:9].reshape(3, 3)[:, 0] - (0, 0, 1)).max() == 0


def test_metres_round_to_bins_on_the_careful_side():
    from emfusion_amd import pipeline
    assert pipeline.ground_bins(0.75, 0.5, 0.25) == (3, 2)
    assert pipeline.ground_bins(0.76, 0.49, 0.25) == (4, 1)
    assert pipeline.ground_bins(0.3, 0.05, 0.02) == (16, 2)     # in float32 0.3 / 0.02 lies just above 15: up
    assert pipeline.ground_bins(0.0, 0.0, 0.02) == (1, 0)       # R < 1 becomes 1
    assert pipeline.ground_bins(0.01, 0.019, 0.02) == (1, 0)
    assert pipeline.ground_bins(1e9, 1e9, 0.02) == (4096, 4096)


# ---- holes ----------------------------------------------------------------------------------------------------------

def empty_interior_slots(n, slot, R, offset):
    """How many slots of `slot` voxels that lie wholly inside an n^3 lattice box (rotated by R, shifted by offset)
    receive no voxel centre."""
    c = (n - 1) / 2.0
    g = np.arange(n, dtype=np.float64) - c
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    q = p @ R.T / slot + offset
    idx = np.floor(q).astype(np.int64)
    lo, hi = idx.min(axis=0), idx.max(axis=0)
    dims = hi - lo + 1
    filled = np.zeros(dims, bool)
    filled[tuple((idx - lo).T)] = True
    grid = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    inside = np.ones(len(grid), bool)
    for corner in range(8):
        s = (grid + [(corner >> a) & 1 for a in range(3)] - offset) * slot  # a corner of the slot, rotated frame
        back = s @ R                                                       # R^T applied: back in the lattice frame
        inside &= (np.abs(back) <= n / 2.0).all(axis=1)
    return int((inside & ~filled.reshape(-1)).sum()), int(inside.sum())


def test_slots_of_two_voxels_leave_no_holes_and_slots_of_one_do():
    rng = np.random.default_rng(11)
    empty = {1: 0, 2: 0, 3: 0}
    interior = {1: 0, 2: 0, 3: 0}
    for _ in range(20):
        R = rf.rotation(rng.normal(size=3), rng.uniform(5, 85))
        offset = rng.uniform(0, 1, 3)
        for slot in (1, 2, 3):
            e, n = empty_interior_slots(40, slot, R, offset)
            empty[slot] += e
            interior[slot] += n
    assert min(interior.values()) > 1000
    # a closed ball of radius sqrt(3) / 2 always holds a lattice point, and a cube of side 2 holds one of radius 1
    assert empty[2] == 0 and empty[3] == 0, empty
    assert empty[1] > 0, "slots of one voxel are refused on a tilted frame because they leave holes"
    # ... and none where the frame is along the axes: there a slot of one voxel is fine
    assert empty_interior_slots(40, 1, np.eye(3), np.array([0.5, 0.5, 0.5]))[0] == 0


# ---- axis-aligned ups: a transpose, a flip and an any-reduction --------------------------------------------------------

@pytest.mark.parametrize("axis,sign", rf.AXES)
@pytest.mark.parametrize("c", [1, 2])
def test_axis_aligned_planes_are_a_transpose_a_flip_and_an_any_reduction(axis, sign, c):
    shape = (13, 10, 7)
    v = rf.volume(shape, "random", seed=3)
    bins = -(-shape[axis] // c)
    G, W, H, B = rf.spec_frame(shape, ("axis", axis, sign, c), bins)
    assert rf.aligned(G)
    rows = G[:, :3]
    assert (np.sort(np.abs(rows), axis=1)[:, :2] == 0).all() and np.abs(np.abs(rows).max(axis=1) - 1.0 / c).max() < 1e-6
    ax = [int(np.argmax(np.abs(r))) for r in rows]       # the box axis of u, v, h
    sg = [float(np.sign(r[a])) for r, a in zip(rows, ax)]
    assert ax[2] == axis and sg[2] == sign and sorted(ax) == [0, 1, 2]
    occ, fre = rf.planes(v, G, W, H, B)
    for plane, cls in ((occ, rf.OCCUPIED), (fre, rf.FREE)):
        m = (v == cls).transpose(2, 1, 0)                  # [x, y, z]
        m = m.transpose(ax[1], ax[0], ax[2])               # [v axis, u axis, h axis]
        for d, sign_d in enumerate((sg[1], sg[0], sg[2])):
            if sign_d < 0:
                m = np.flip(m, axis=d)                      # cells start at the face the ground axis leaves from
        m = np.pad(m, [(0, -n % c) for n in m.shape])
        nv, nu, nh = (n // c for n in m.shape)
        m = m.reshape(nv, c, nu, c, nh, c).any(axis=(1, 3, 5))
        assert nh == B and nv <= H <= nv + 1 and nu <= W <= nu + 1
        bits = np.zeros((H, W, B), bool)
        bits[:m.shape[0], :m.shape[1], :] = m
        got = np.zeros((H, W, B), bool)
        for h in range(B):
            got[:, :, h] = (plane[:, :, h >> 6] >> np.uint64(h & 63)) & np.uint64(1) != 0
        assert (got == bits).all(), (axis, sign, c, cls)


# ---- cells: standable levels on hand-made columns ----------------------------------------------------------------------

def column(B, occ=(), fre=()):
    s = ["U"] * B
    for k in fre:
        s[k] = "F"
    for k in occ:
        s[k] = "O"
    return "".join(s)


@pytest.mark.parametrize("states,R,expected", [
    # headroom exactly R and R - 1
    (column(16, occ=[2, 8], fre=range(3, 8)), 5, (2, 8, 5, 1)),
    (column(16, occ=[2, 7], fre=range(3, 7)), 5, (-1, 7, 0, 0)),
    # a level at B - 1 - R stands, one at B - R does not (its headroom would leave the band)
    (column(16, occ=[10], fre=range(11, 16)), 5, (10, 10, 5, 1)),
    (column(16, occ=[11], fre=range(12, 16)), 5, (-1, 11, 0, 0)),
    (column(16, occ=[15]), 1, (-1, 15, 0, 0)),
    # an OCC bit inside the headroom; the fre bit under it does not count
    (column(16, occ=[2, 5], fre=range(3, 12)), 5, (5, 5, 6, 1)),
    (column(16, occ=[2, 5], fre=range(3, 12)), 2, (2, 5, 2, 2)),
    # an UNK slot inside the headroom
    (column(16, occ=[2], fre=[3, 4, 6, 7, 8]), 3, (-1, 2, 0, 0)),
    (column(16, occ=[2], fre=[3, 4, 6, 7, 8]), 2, (2, 2, 2, 1)),
    # levels on both sides of the word boundary at bins 63 / 64
    (column(130, occ=[63], fre=range(64, 70)), 5, (63, 63, 6, 1)),
    (column(130, occ=[64], fre=range(65, 70)), 5, (64, 64, 5, 1)),
    (column(130, occ=[60], fre=range(61, 66)), 5, (60, 60, 5, 1)),
    (column(130, occ=[60], fre=range(61, 64)), 5, (-1, 60, 0, 0)),
    (column(130, occ=[10, 63, 64, 127, 128], fre=list(range(11, 63)) + list(range(65, 127)) + [129]), 1, (10, 128, 52, 3)),
    (column(256, occ=[0], fre=range(1, 256)), 255, (0, 0, 255, 1)),
    (column(256, occ=[0], fre=range(1, 256)), 256, (-1, 0, 0, 0)),
    # the lowest standable level is the floor; two storeys
    (column(64, occ=[5, 30], fre=list(range(6, 30)) + list(range(31, 64))), 10, (5, 30, 24, 2)),
    (column(1, occ=[0]), 1, (-1, 0, 0, 0)),
    (column(8), 1, (-1, -1, 0, 0)),
    (column(8, fre=range(8)), 1, (-1, -1, 0, 0)),
])
def test_standable_levels_on_hand_made_columns(states, R, expected):
    assert rf.cell_of_states(states, R) == expected
    # ... and through the bit planes
    B, words = len(states), rf.words_of(len(states))
    occ, fre = np.zeros((1, 1, words), np.uint64), np.zeros((1, 1, words), np.uint64)
    for k, s in enumerate(states):
        if s == "O":
            occ[0, 0, k >> 6] |= np.uint64(1) << np.uint64(k & 63)
            fre[0, 0, k >> 6] |= np.uint64(1) << np.uint64(k & 63) if k % 2 else np.uint64(0)  # occ wins over fre
        elif s == "F":
            fre[0, 0, k >> 6] |= np.uint64(1) << np.uint64(k & 63)
    assert rf.column_states(occ[0, 0], fre[0, 0], B) == states
    assert tuple(int(v) for v in rf.cells(occ, fre, B, R)[0, 0]) == expected


# ---- classes: the step rule ----------------------------------------------------------------------------------------------

def records_of(floors, tops=None):
    floors = np.asarray(floors, np.int16)
    rec = np.zeros(floors.shape, rf.CELL_DTYPE)
    rec["floor"] = floors
    rec["top"] = floors if tops is None else np.asarray(tops, np.int16)
    return rec


def test_the_step_rule():
    F, O, U = rf.FREE, rf.OCCUPIED, rf.UNKNOWN
    # a step of exactly S passes, S + 1 does not -- and marks both sides
    rec = records_of([[4, 4, 6, 6, 9, 9]])
    assert rf.classes2d(rec, 2)[0].tolist() == [[F, F, F, O, O, F]]
    assert rf.classes2d(rec, 3)[0].tolist() == [[F, F, F, F, F, F]]
    assert rf.classes2d(rec, 0)[0].tolist() == [[F, O, O, O, O, F]]
    # diagonal neighbours count: the middle cell touches the high corner by a corner only
    rec = records_of([[4, 4, 4], [4, 4, 4], [4, 4, 9]])
    assert rf.classes2d(rec, 2)[0].tolist() == [[F, F, F], [F, O, O], [F, O, O]]
    # a neighbour without a floor constrains nothing: matter without a floor is occupied, nothing at all is unknown
    rec = records_of([[4, -1, 9], [4, -1, 9]], tops=[[4, 7, 9], [4, -1, 9]])
    assert rf.classes2d(rec, 0)[0].tolist() == [[F, O, F], [F, U, F]]
    # the map's edge is no neighbour
    assert rf.classes2d(records_of([[7]]), 0)[0].tolist() == [[F]]
    assert rf.classes2d(records_of([[-1]], tops=[[-1]]), 0)[0].tolist() == [[U]]
    assert rf.classes2d(records_of([[0, 200]]), 199)[0].tolist() == [[O, O]]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------

def test_the_header_the_ctypes_mirrors_and_the_exports():
    from emfusion_amd import _lib, pipeline
    hip_h = (ROOT / "include" / "emf_hip.h").read_text()
    fusion_h = (ROOT / "include" / "emf_fusion.h").read_text()
    assert int(re.search(r"#define\s+EMF_HIP_ABI_VERSION\s+(\d+)", hip_h).group(1)) == 8
    assert int(re.search(r"#define\s+EMF_GROUND_MAX_BINS\s+(\d+)", hip_h).group(1)) == rf.MAX_BINS == _lib.GROUND_MAX_BINS
    assert int(re.search(r"#define\s+EMF_DF_MAX_AXIS\s+(\d+)", hip_h).group(1)) == rf.MAX_AXIS
    assert np.dtype(_lib.GROUND_CELL_DTYPE) == rf.CELL_DTYPE and rf.CELL_DTYPE.itemsize == 8
    assert C.sizeof(_lib.EmfGroundFrame) == 60
    assert "Ground map" in hip_h and "typedef struct emf_ground_frame" in hip_h and "typedef struct emf_ground_cell" in hip_h
    declared = _lib.declared_symbols()
    lib, fus = _lib.load(), pipeline.load()
    for name, nargs in (("emf_hip_groundColumns", 6), ("emf_hip_groundCells", 7), ("emf_hip_groundClasses", 5)):
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs
        getattr(lib, name)
    for name in ("emf_fusion_ground_map", "emf_fusion_copy_ground_map", "emf_fusion_ground_frame", "emf_fusion_set_ground_output",
                 "emf_fusion_ground_classes_ptr"):
        assert name in pipeline.declared_symbols() and name in fusion_h and name in fus._emf_sigs
        getattr(fus, name)
    assert "POLICY, NOT" in pipeline.Fusion.ground_map.__doc__
