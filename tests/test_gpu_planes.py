"""emf_hip_planeSurface, emf_hip_planeDirections, emf_hip_planeOffsets and emf_hip_planeAssign (include/emf_hip.h
"Planes") against tests/planes_reference.py, byte for byte: boxes that fill, miss and exceed the 32 x 8 x 8
tile, a box at an unaligned origin whose neighbours come from outside it, boxes that touch the volume's faces and a
2048 x 2 x 2 one; analytic planes, random volumes with every special value, zero gradients, infinities and unseen
volumes with the unseen-tile map and without it; K, capacity, D, S and P at their ends; outputs poisoned beforehand, a
second call into the dirty buffers, the library built with contraction on, and every refusal."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import planes_reference as pr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

POISON = 0xA5
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
EXTRA = 5                # records of room behind the capacity

# (volume shape, box or None, content), shapes (nx, ny, nz)
CASES = [
    ((1, 1, 1), None, "random"),
    ((3, 3, 3), None, "random"),
    ((32, 8, 8), None, "random"),
    ((33, 9, 9), None, "random"),
    ((31, 7, 7), None, "random"),
    ((33, 9, 9), None, "tilted"),
    ((33, 9, 9), None, "axis"),
    ((96, 40, 40), ((5, 3, 7), (64, 16, 16)), "random"),
    ((96, 40, 40), ((5, 3, 7), (64, 16, 16)), "tilted"),
    ((96, 40, 40), ((17, 9, 13), (64, 16, 16)), "axis"),
    ((40, 24, 20), None, "tilted"),                           # the box touches all six faces
    ((40, 24, 20), ((7, 8, 4), (33, 16, 16)), "random"),      # ... the three upper ones
    ((40, 24, 20), ((0, 0, 0), (33, 9, 9)), "random"),        # ... the three lower ones
    ((2048, 2, 2), None, "random"),                           # no voxel has six neighbours
    ((2048, 4, 4), ((0, 1, 1), (2048, 2, 2)), "random"),
    ((12, 10, 9), None, "infinite"),
    ((13, 5, 5), None, "zero_gradient"),
    ((40, 24, 20), None, "unseen"),
    ((4, 328, 200), None, "random"),                          # 1 x 41 x 25 = 1025 tiles: the tile scan crosses its carry
]
_expected = {}


def case_id(c):
    box = "" if c[1] is None else "-" + "x".join(map(str, c[1][1])) + "at" + "x".join(map(str, c[1][0]))
    return "x".join(map(str, c[0])) + box + "-" + c[2]


def expected(case):
    """(tsdf, weights, lo, size, records, counts) of the restatement, computed once, shared and read-only."""
    if case not in _expected:
        shape, box, content = case
        tsdf, weights = pr.volume(shape, content)
        rec, counts = pr.records(tsdf, weights, box)
        lo, size = ((0, 0, 0), shape) if box is None else box
        for a in (tsdf, weights, rec):
            a.setflags(write=False)
        _expected[case] = (tsdf, weights, lo, size, rec, counts)
    return _expected[case]


def i3(v):
    return (C.c_int32 * 3)(*[int(c) for c in v])


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def poisoned(n, dtype):
    from emfusion_amd.devmem import DeviceArray
    return DeviceArray((n,), dtype).fill_bytes_(POISON)


def ptr(a):
    return None if a is None else C.c_void_p(a.ptr)


def unseen_map(d_tsdf, d_weights, shape):
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    m = DeviceArray((ops.unseen_tile_bytes(shape),), np.uint8)
    ops.rebuild_unseen_tiles(d_tsdf, d_weights, m)
    return m


def run_surface(lib, case, capacity, d_unseen=None, volumes=None):
    """The entry into poisoned outputs, twice: (records device array, counters device array); checked against the
    restatement here."""
    tsdf, weights, lo, size, rec, counts = expected(case)
    d_tsdf, d_weights = volumes or (to_dev(tsdf), to_dev(weights))
    d_rec = poisoned(capacity + EXTRA, pr.VOXEL)
    d_cnt = poisoned(4 + EXTRA, np.uint32)
    scratch_bytes = lib.emf_hip_planeSurfaceScratchBytes(i3(size))
    tiles = math.ceil(size[0] / 32) * math.ceil(size[1] / 8) * math.ceil(size[2] / 8)
    assert scratch_bytes == 4 * tiles
    d_scratch = poisoned(scratch_bytes + EXTRA, np.uint8)
    want = pr.counters(counts, capacity)
    for again in (False, True):
        rc = lib.emf_hip_planeSurface(ptr(d_tsdf), ptr(d_weights), i3(case[0]), i3(lo), i3(size), ptr(d_unseen), ptr(d_rec),
                                      capacity, ptr(d_cnt), ptr(d_scratch), None)
        assert rc == 0, lib.emf_hip_last_error_string()
        got_cnt, got = d_cnt.numpy(), d_rec.numpy()
        assert got_cnt[:4].tobytes() == want.tobytes(), (case, capacity, again, got_cnt[:4], want)
        assert (got_cnt[4:].view(np.uint8) == POISON).all()
        n = int(want[2])
        assert got[:n].tobytes() == rec[:n].tobytes(), (case, capacity, again)
        assert (got[n:].view(np.uint8) == POISON).all(), "written beyond the records"
        assert (d_scratch.numpy()[scratch_bytes:] == POISON).all()
    assert d_tsdf.numpy().tobytes() == tsdf.tobytes() and d_weights.numpy().tobytes() == weights.tobytes()
    return d_rec, d_cnt


def vote_params(rec, size):
    """Directions, shifts and planes for the vote entries: the restatement's own host steps where the records yield
    some, completed by fixed ones up to the limits."""
    rng = np.random.default_rng(len(rec) + size[0])
    extra = rng.normal(size=(pr.MAX_PLANES, 3))
    extra /= np.linalg.norm(extra, axis=1, keepdims=True)
    found = [d[2] for d in pr.directions(pr.direction_bins(rec, 15), 15, 1, 20.0)]
    if found:  # a second direction 10 degrees from the strongest: with a gate of 60 degrees a record aligns with both
        a = np.asarray(found[0])
        t = np.cross(a, [0.3, 0.5, 0.8])
        found.insert(1, list(math.cos(math.radians(10)) * a + math.sin(math.radians(10)) * t / np.linalg.norm(t)))
    dirs = np.array((found + list(extra))[:pr.MAX_DIRS], np.float32)
    frames = [pr.offset_frame([float(v) for v in n], size, 1.0) for n in dirs]
    shift = np.array([f[3] for f in frames], np.float32)
    d = [f[0] + (k % 7 + 0.5) * (f[1] / 7.0) for k, f in enumerate(frames)]
    if len(rec):  # plane 0 passes through the records along the strongest direction
        x, y, z = pr.voxel_of(rec["index"], size)
        d[0] = float(np.median(dirs[0, 0] * x + dirs[0, 1] * y + dirs[0, 2] * z))
    normals = np.concatenate([dirs, extra[:pr.MAX_PLANES - len(dirs)].astype(np.float32)])
    planes = np.concatenate([normals, np.resize(np.array(d, np.float32), (pr.MAX_PLANES, 1))], 1).astype(np.float32)
    planes[5] = planes[0]                    # equal |e| to two planes: the lower index takes every member
    planes[6, :3], planes[7, :3] = (0, 0, -1), (0, 0, -1)
    planes[6, 3], planes[7, 3] = -(size[2] // 2 - 0.5), -(size[2] // 2 + 0.5)  # |e| = 0.5 to both for z = size / 2
    return dirs, shift, planes


def run_votes(lib, case, d_rec, d_cnt, capacity, Ks=(1, 2, 15, 16, 31)):
    tsdf, weights, lo, size, rec, counts = expected(case)
    rec = rec[:min(len(rec), capacity)]
    before = d_rec.numpy().tobytes()
    for K in Ks:
        want = pr.direction_bins(rec, K)
        d_bins = poisoned(6 * K * K + EXTRA, np.uint32)
        for again in (False, True):
            assert lib.emf_hip_planeDirections(ptr(d_rec), ptr(d_cnt), capacity, K, ptr(d_bins), None) == 0
            got = d_bins.numpy()
            assert got[:6 * K * K].tobytes() == want.tobytes(), (case, K, again)
            assert (got[6 * K * K:].view(np.uint8) == POISON).all()
    dirs, shift, planes = vote_params(rec, size)
    cos2 = float(np.float32(math.cos(math.radians(60.0)) ** 2))
    for D, S, inv_bin in ((1, 1, 1e-3), (16, 4096, 1.0), (16, 37, 0.5), (3, 4096, 16.0)):
        want = pr.offset_hist(rec, size, dirs[:D], shift[:D], cos2, inv_bin, S)
        d_hist = poisoned(D * S + EXTRA, np.uint32)
        for again in (False, True):
            assert lib.emf_hip_planeOffsets(ptr(d_rec), ptr(d_cnt), capacity, i3(size), fp(dirs), fp(shift), D, cos2, inv_bin, S,
                                            ptr(d_hist), None) == 0
            got = d_hist.numpy()
            assert got[:D * S].tobytes() == want.tobytes(), (case, D, S, again)
            assert (got[D * S:].view(np.uint8) == POISON).all()
    for P, gate, band in ((1, cos2, 2.0), (64, cos2, 1.5), (64, 0.0, 1e9), (8, 1.0, 0.0)):
        want_labels, want_mom = pr.assign(rec, size, planes[:P], gate, band)
        d_labels, d_mom = poisoned(capacity + EXTRA, np.int16), poisoned(P + EXTRA, pr.MOMENTS)
        for again in (False, True):
            assert lib.emf_hip_planeAssign(ptr(d_rec), ptr(d_cnt), capacity, i3(size), fp(planes), P, gate, band, ptr(d_labels),
                                           ptr(d_mom), None) == 0
            got_labels, got_mom = d_labels.numpy(), d_mom.numpy()
            assert got_labels[:len(rec)].tobytes() == want_labels.tobytes(), (case, P, again)
            assert (got_labels[len(rec):].view(np.uint8) == POISON).all()
            assert got_mom[:P].tobytes() == want_mom.tobytes(), (case, P, again, got_mom[:P], want_mom)
            assert (got_mom[P:].view(np.uint8) == POISON).all()
    assert d_rec.numpy().tobytes() == before  # the records are only read
    return rec, dirs, planes, cos2


def lib_():
    from emfusion_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_stage_is_exact(dev, case):
    lib = lib_()
    need = expected(case)[5][1]
    capacity = max(need, 1)
    d_rec, d_cnt = run_surface(lib, case, capacity)
    run_votes(lib, case, d_rec, d_cnt, capacity)


@pytest.mark.parametrize("case", [CASES[3], CASES[8], CASES[10]], ids=case_id)
def test_capacities(dev, case):
    """0 (no records array at all), one below the need, exact, and far above it."""
    lib = lib_()
    tsdf, weights, lo, size, rec, counts = expected(case)
    need = counts[1]
    assert need > 40
    volumes = (to_dev(tsdf), to_dev(weights))
    d_cnt, d_scratch = poisoned(4, np.uint32), poisoned(lib.emf_hip_planeSurfaceScratchBytes(i3(size)), np.uint8)
    assert lib.emf_hip_planeSurface(ptr(volumes[0]), ptr(volumes[1]), i3(case[0]), i3(lo), i3(size), None, None, 0, ptr(d_cnt),
                                    ptr(d_scratch), None) == 0
    assert d_cnt.numpy().tobytes() == pr.counters(counts, 0).tobytes()
    for capacity in (need - 1, need, size[0] * size[1] * size[2]):
        d_rec, d_cnt = run_surface(lib, case, capacity, volumes=volumes)
        if capacity == need - 1:
            run_votes(lib, case, d_rec, d_cnt, capacity, Ks=(15,))


def test_what_the_vote_cases_hold(dev):
    """So that their exactness means something: records aligned with two directions at once, members of the lower of two
    planes at equal distance, none of the higher one's."""
    case = CASES[8]
    tsdf, weights, lo, size, rec, counts = expected(case)
    dirs, shift, planes = vote_params(rec, size)
    cos2 = np.float32(0.25)
    both = pr._aligned(dirs[0], rec["g"], cos2) & pr._aligned(dirs[1], rec["g"], cos2)
    assert both.sum() > 100
    labels, mom = pr.assign(rec, size, planes, np.float32(0.0), 1e9)
    assert mom[0]["count"] > 0 and mom[5]["count"] == 0
    z = pr.voxel_of(rec["index"], size)[2]
    labels, mom = pr.assign(rec, size, planes[6:8], np.float32(0.0), 0.5)
    mid = size[2] // 2
    assert (z == mid).sum() > 20 and (labels[z == mid] == 0).all() and mom[1]["count"] == (z == mid + 1).sum() > 20
    assert mom[0]["count"] == (z == mid).sum() + (z == mid - 1).sum()


def test_a_label_that_comes_back_is_a_run_of_its_own(dev):
    """Labels A, B, A, A, B, B, A, none within one wave (tests/test_planes_reference_cpu.py checks that they are): the sums
    and bounds of a run must not reach across another label to an earlier run of the same one."""
    lib = lib_()
    rec, size, planes, cos2, band = pr.recurring_labels()
    want_labels, want_mom = pr.assign(rec, size, planes, cos2, band)
    d_rec, d_cnt = to_dev(rec), to_dev(np.array([0, len(rec), len(rec), 0], np.uint32))
    d_labels, d_mom = poisoned(len(rec) + EXTRA, np.int16), poisoned(len(planes) + EXTRA, pr.MOMENTS)
    for again in (False, True):
        assert lib.emf_hip_planeAssign(ptr(d_rec), ptr(d_cnt), len(rec), i3(size), fp(planes), len(planes), float(cos2), band,
                                       ptr(d_labels), ptr(d_mom), None) == 0
        got_labels, got_mom = d_labels.numpy(), d_mom.numpy()
        assert got_labels[:len(rec)].tobytes() == want_labels.tobytes(), again
        assert got_mom[:len(planes)].tobytes() == want_mom.tobytes(), (again, got_mom[:len(planes)], want_mom)
        assert (got_labels[len(rec):].view(np.uint8) == POISON).all() and (got_mom[len(planes):].view(np.uint8) == POISON).all()


@pytest.mark.parametrize("case", [CASES[8], CASES[9], CASES[17], CASES[7]], ids=case_id)
def test_the_unseen_tile_map_changes_no_byte(dev, case):
    lib = lib_()
    tsdf, weights = expected(case)[:2]
    volumes = (to_dev(tsdf), to_dev(weights))
    d_map = unseen_map(volumes[0], volumes[1], case[0])
    skipped = int((d_map.numpy() != 0).sum())
    if case[2] == "unseen":
        assert skipped == d_map.shape[0]
    elif case[2] != "random":
        assert 0 < skipped < d_map.shape[0]  # deep behind the surface nothing is observed
    run_surface(lib, case, max(expected(case)[5][1], 1), d_unseen=d_map, volumes=volumes)


def test_the_contraction_build_gives_the_same_bytes(dev):
    from emfusion_amd import _lib
    fma = _lib.load_variant("_fma")
    for case in (CASES[3], CASES[8], CASES[9], CASES[11]):
        capacity = max(expected(case)[5][1], 1)
        d_rec, d_cnt = run_surface(fma, case, capacity)
        run_votes(fma, case, d_rec, d_cnt, capacity, Ks=(15, 16))


def test_the_wrappers(dev):
    from emfusion_amd import ops
    case = CASES[8]
    tsdf, weights, lo, size, rec, counts = expected(case)
    d_tsdf, d_weights = to_dev(tsdf), to_dev(weights)
    d_rec, d_cnt = ops.plane_surface(d_tsdf, d_weights, box=(lo, size), unseen_tiles=unseen_map(d_tsdf, d_weights, case[0]))
    assert d_cnt.numpy().tobytes() == pr.counters(counts, size[0] * size[1] * size[2]).tobytes()
    assert d_rec.numpy()[:len(rec)].tobytes() == rec.tobytes()
    assert ops.plane_directions(d_rec, d_cnt, 15).numpy().tobytes() == pr.direction_bins(rec, 15).tobytes()
    # the whole finder with the device's stages in place of the restatement's

    class Device:
        records = staticmethod(lambda t, w, box: ops.plane_surface(d_tsdf, d_weights, box=box)[0].numpy()[:len(rec)])
        direction_bins = staticmethod(lambda r, K: ops.plane_directions(d_rec, d_cnt, K).numpy())
        offset_hist = staticmethod(lambda r, s, dirs, shift, cos2, inv_bin, S: ops.plane_offsets(d_rec, d_cnt, s, dirs, shift, cos2, inv_bin, S).numpy())

        @staticmethod
        def assign(r, s, planes, cos2, band):
            labels, mom = ops.plane_assign(d_rec, d_cnt, s, planes, cos2, band)
            return labels.numpy()[:len(rec)], mom.numpy()

    want = pr.find_planes(tsdf, weights, (lo, size), min_votes=30)
    got = pr.find_planes(tsdf, weights, (lo, size), min_votes=30, stages=Device)
    assert len(want[0]) == 1 and want[0][0]["count"] > 300
    assert repr(got[0]) == repr(want[0]) and got[2].tobytes() == want[2].tobytes()
    n = np.asarray((0.3, 1.0, -0.45)) / np.linalg.norm((0.3, 1.0, -0.45))
    assert math.degrees(math.acos(min(1.0, float(np.dot(n, got[0][0]["n"]))))) < math.degrees(math.atan(math.sqrt(2) / 15))


def test_the_refusals(dev):
    """EMF_E_ARG / EMF_E_LIMIT with nothing enqueued: the poisoned outputs keep every byte."""
    lib = lib_()
    case = CASES[3]
    tsdf, weights, lo, size, rec, counts = expected(case)
    d_tsdf, d_weights = to_dev(tsdf), to_dev(weights)
    cap = 64
    d_rec, d_cnt, d_scr = poisoned(cap, pr.VOXEL), poisoned(4, np.uint32), poisoned(64, np.uint8)
    outs = [d_rec, d_cnt, d_scr]

    def surface(code, tsdf=d_tsdf, weights=d_weights, res=case[0], lo=lo, size=size, records=d_rec, capacity=cap, counters=d_cnt,
                scratch=d_scr, offset=0):
        rec_ptr = None if records is None else C.c_void_p(records.ptr + offset)
        rc = lib.emf_hip_planeSurface(ptr(tsdf), ptr(weights), i3(res), i3(lo), i3(size), None, rec_ptr, capacity, ptr(counters),
                                      ptr(scratch), None)
        assert rc == code, (rc, lib.emf_hip_last_error_string())

    surface(E_ARG, tsdf=None)
    surface(E_ARG, weights=None)
    surface(E_ARG, counters=None)
    surface(E_ARG, scratch=None)
    surface(E_ARG, records=None)                 # with a capacity above 0
    surface(E_ARG, offset=4)                     # misaligned records
    surface(E_ARG, size=(0, 9, 9))
    surface(E_ARG, size=(33, -1, 9))
    surface(E_ARG, lo=(1, 0, 0))                 # the box leaves the volume
    surface(E_ARG, lo=(-1, 0, 0), size=(8, 8, 8))
    surface(E_LIMIT, res=(4096, 9, 9), size=(2049, 9, 9))
    surface(E_LIMIT, res=(2048, 2048, 2048), size=(2048, 2048, 512))   # 2^31 voxels
    surface(E_LIMIT, capacity=0x80000000)
    assert lib.emf_hip_planeSurfaceScratchBytes(i3((2049, 1, 1))) == 0 and lib.emf_hip_planeSurfaceScratchBytes(i3((0, 1, 1))) == 0
    assert lib.emf_hip_planeSurfaceScratchBytes(None) == 0

    K = 15
    d_bins = poisoned(6 * 31 * 31, np.uint32)
    outs.append(d_bins)
    for args, code in (((None, ptr(d_cnt), cap, K, ptr(d_bins)), E_ARG), ((ptr(d_rec), None, cap, K, ptr(d_bins)), E_ARG),
                       ((ptr(d_rec), ptr(d_cnt), cap, K, None), E_ARG), ((ptr(d_rec), ptr(d_cnt), 0, K, ptr(d_bins)), E_ARG),
                       ((ptr(d_rec), ptr(d_cnt), cap, 0, ptr(d_bins)), E_ARG), ((ptr(d_rec), ptr(d_cnt), cap, 32, ptr(d_bins)), E_LIMIT),
                       ((C.c_void_p(d_rec.ptr + 8), ptr(d_cnt), cap, K, ptr(d_bins)), E_ARG),
                       ((ptr(d_rec), ptr(d_cnt), 0x80000000, K, ptr(d_bins)), E_LIMIT)):
        assert lib.emf_hip_planeDirections(*args, None) == code, (args, lib.emf_hip_last_error_string())

    dirs = np.zeros((17, 3), np.float32)
    dirs[:, 0] = 1
    shift = np.zeros(17, np.float32)
    d_hist = poisoned(16 * 64, np.uint32)
    outs.append(d_hist)

    def offsets(code, records=d_rec, counters=d_cnt, capacity=cap, size=size, dirs=fp(dirs), shift=fp(shift), D=2, cos2=0.5,
                inv_bin=1.0, S=64, hist=d_hist):
        rc = lib.emf_hip_planeOffsets(ptr(records), ptr(counters), capacity, i3(size), dirs, shift, D, cos2, inv_bin, S, ptr(hist), None)
        assert rc == code, (rc, lib.emf_hip_last_error_string())

    offsets(E_ARG, records=None)
    offsets(E_ARG, counters=None)
    offsets(E_ARG, capacity=0)
    offsets(E_ARG, size=(33, 0, 9))
    offsets(E_LIMIT, size=(2049, 1, 1))
    offsets(E_ARG, dirs=None)
    offsets(E_ARG, shift=None)
    offsets(E_ARG, D=0)
    offsets(E_LIMIT, D=17)
    offsets(E_ARG, S=0)
    offsets(E_LIMIT, S=4097)
    offsets(E_ARG, cos2=-0.1)
    offsets(E_ARG, cos2=1.5)
    offsets(E_ARG, cos2=float("nan"))
    offsets(E_ARG, hist=None)

    planes = np.zeros((65, 4), np.float32)
    planes[:, 2] = 1
    d_labels, d_mom = poisoned(cap, np.int16), poisoned(64, pr.MOMENTS)
    outs += [d_labels, d_mom]

    def assign(code, records=d_rec, counters=d_cnt, capacity=cap, size=size, planes=fp(planes), P=2, cos2=0.5, band=1.0,
               labels=d_labels, moments=d_mom, offset=0):
        mom_ptr = None if moments is None else C.c_void_p(moments.ptr + offset)
        rc = lib.emf_hip_planeAssign(ptr(records), ptr(counters), capacity, i3(size), planes, P, cos2, band, ptr(labels), mom_ptr, None)
        assert rc == code, (rc, lib.emf_hip_last_error_string())

    assign(E_ARG, records=None)
    assign(E_ARG, counters=None)
    assign(E_ARG, capacity=0)
    assign(E_ARG, size=(0, 1, 1))
    assign(E_ARG, planes=None)
    assign(E_ARG, P=0)
    assign(E_LIMIT, P=65)
    assign(E_ARG, cos2=2.0)
    assign(E_ARG, band=-1.0)
    assign(E_ARG, band=float("nan"))
    assign(E_ARG, labels=None)
    assign(E_ARG, moments=None)
    assign(E_ARG, offset=4)
    from emfusion_amd import devmem
    devmem.synchronize()
    for o in outs:
        assert (o.numpy().view(np.uint8) == POISON).all(), "a refused call wrote something"
