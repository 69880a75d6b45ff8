"""emf_hip_absorbVolume (include/emf_hip.h "Absorbing a volume") against tests/absorb_reference.py, byte for
byte, in the default library and in the one built with a*b+c contraction on: destinations and sources of the
restatement's shapes and contents with and without the source's mask and unseen-tile map; the six poses of the contacts
test, sample points exactly on the source's first and last cells; voxel-size ratios 1, 0.8 and 2; truncation ratios 1,
0.5 and 2; destination weights 0, negative, NaN and at maxWeight; NaN and -0.0 tsdf at a source corner; the whole box, one
voxel, a box that cuts tiles, an empty box, the library's covering box.  The destination lies between poisoned guards, the
record is poisoned beforehand and nothing is written beyond it; inputs are only read; a second call; every refusal."""
import ctypes as C

import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import shape_reference as sr
from tests.parity_util import to_dev
from tests.resample_util import GUARD, POISON, Guarded, lib_for, upload_src

pytestmark = pytest.mark.gpu

f32 = np.float32
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
EXTRA = 3    # records of room behind the one a call writes


def run(dst, src, pose, box, variants=("", "_fma"), maps=(False, True), twice=True):
    """One absorption in every asked library, with and without the source's unseen-tile map, into a guarded destination
    and a poisoned record, and once more on top of the result; returns the expected (tsdf, weights, record)."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    want = ar.absorb(dst, src, pose, box)
    ar.check_identities(want[2])
    after = dict(dst, tsdf=want[0], weights=want[1])
    want2 = ar.absorb(after, src, pose, box) if twice else None
    for with_map in maps:
        d_src = upload_src(src, with_map)
        for variant in variants:
            gt, gw = Guarded(dst["tsdf"]), Guarded(dst["weights"])
            d_dst = dict(tsdf=gt.view, weights=gw.view, voxel_size=dst["voxel_size"], truncdist=dst["truncdist"],
                         max_weight=dst["max_weight"])
            rec = DeviceArray((1 + EXTRA,), ar.ABSORB).fill_bytes_(POISON)
            for expect in (want, want2):
                if expect is None:
                    continue
                assert ops.absorb_volume(d_dst, d_src, pose, box=box, out=rec, lib=lib_for(variant)) is rec
                got = rec.numpy()
                assert got[0].tobytes() == expect[2].tobytes(), (variant, with_map, got[0], expect[2])
                assert (got[1:].view(np.uint8) == POISON).all(), "written beyond the record"
                t, w = gt.read(), gw.read()
                bad = np.argwhere((t.view(np.uint32) != expect[0].view(np.uint32)) | (w.view(np.uint32) != expect[1].view(np.uint32)))
                assert len(bad) == 0, (variant, with_map, len(bad), bad[:3], [(t[tuple(b)], expect[0][tuple(b)], w[tuple(b)],
                                                                               expect[1][tuple(b)]) for b in bad[:3]])
        # inputs are only read
        assert d_src["tsdf"].numpy().tobytes() == src["tsdf"].tobytes() and d_src["weights"].numpy().tobytes() == src["weights"].tobytes()
        assert src["fg"] is None or d_src["fg_mask"].numpy().tobytes() == src["fg"].tobytes()
    return want


def test_the_poses_are_those_of_the_contacts_test():
    from tests.test_gpu_contacts import poses
    for a, b in zip(ar.poses(0.0125), poses(0.0125)):
        assert (a[0] is None) == (b[0] is None) and (a[0] is None or np.array_equal(a[0], b[0]))
        assert np.array_equal(np.asarray(a[1], f32), np.asarray(b[1], f32), equal_nan=True)


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_one_destination_against_three_sources(dev, shape, content):
    """The sweep of absorb_reference.cases: with and without masks, a source of the destination's lattice, a finer and a
    coarser one, six poses; truncation ratios, destination contents and boxes in turn."""
    total = np.zeros((), ar.ABSORB)
    for name, dst, src, pose, box in ar.cases(shape, content):
        want = run(dst, src, pose, box, twice=name.endswith("whole"))
        for k in ar.COUNTS:
            total[k] += want[2][k]
    assert total["fused"] > 0 and total["outside"] > 0 and total["visited"] > total["fused"]
    if shape != (1, 1, 1) and content in ("half_shell", "gated_block", "random"):
        assert total["unknown"] > 0 and total["masked"] > 0


def test_whole_boxes_of_the_large_destinations(dev):
    """Every case of the two destinations with more than one tile per axis over the WHOLE box (the sweep gives each case
    one kind of box): several workgroups, tiles the volume cuts on every axis."""
    fresh = mixed = 0
    for shape in ((40, 24, 20), (33, 17, 9), (64, 8, 8)):
        for content in ("half_shell", "gated_block", "all_solid"):
            for name, dst, src, pose, box in ar.cases(shape, content, boxes=("whole",)):
                if "pose4" in name or "pose5" in name:
                    continue
                want = run(dst, src, pose, box, variants=("",), maps=(True,), twice=False)
                fresh, mixed = fresh + int(want[2]["fresh"]), mixed + int(want[2]["fused"] - want[2]["fresh"])
    assert fresh > 1000 and mixed > 1000, (fresh, mixed)


def test_equal_lattices_read_the_sources_own_bits_and_the_edge_cells(dev):
    """Voxel size 0.25 and whole-voxel shifts make q exact: q = v + shift.  u is then the source's tsdf at a voxel, bit
    for bit (equal truncation distances), and q is exactly 0, exactly N - 2 (the last inside cell) and exactly N - 1
    (outside) for some voxels of the box."""
    shape = (33, 17, 9)
    rng = np.random.default_rng(5)
    other = rng.uniform(-0.999, 0.999, shape[::-1]).astype(f32)
    src = ar.src_vol(other, np.full(other.shape, 3.0, f32), None, 0.25, 0.5)
    dt, dw, _ = sr.volume(shape, "random")
    dst = ar.dst_vol(dt, dw, 0.25, 0.5, ar.MAX_WEIGHT)
    for shift in ((0, 0, 0), (-3, 0, 0), (2, 0, 0), (1, -2, 1), (0, 3, -4)):
        pose = ar.pose_of(None, [0.25 * s for s in shift])
        want = run(dst, src, pose, ar.whole(dst), twice=False)
        inside = [max(0, min(shape[j] - 1, shape[j] - 2 - shift[j]) - max(0, -shift[j]) + 1) for j in range(3)]  # q in [0, N - 2]
        assert want[2]["fused"] == inside[0] * inside[1] * inside[2] and want[2]["unknown"] == 0
        assert want[2]["outside"] == want[2]["visited"] - want[2]["fused"]
        with np.errstate(invalid="ignore"):
            fresh = ~(dw > 0)
        z, y, x = np.nonzero(fresh)
        ok = (x + shift[0] >= 0) & (x + shift[0] <= shape[0] - 2) & (y + shift[1] >= 0) & (y + shift[1] <= shape[1] - 2) & \
             (z + shift[2] >= 0) & (z + shift[2] <= shape[2] - 2)
        z, y, x = z[ok], y[ok], x[ok]
        assert len(x) > 100 and want[0][z, y, x].tobytes() == other[z + shift[2], y + shift[1], x + shift[0]].tobytes()
        assert (want[1][z, y, x] == 3.0).all()


def test_source_values_at_a_cells_corner(dev):
    """NaN and -0.0 tsdf and a zero, a negative and a NaN weight at single corners of the source's cells, into a
    destination with weights 0, negative, NaN and at maxWeight."""
    dst, src, poses = ar.planted_case()
    for pose in poses:
        want = run(dst, src, pose, ar.whole(dst))
        assert want[2]["unknown"] > 0 and want[2]["fresh"] > 0 and want[2]["fused"] > want[2]["fresh"] and want[2]["saturated"] > 0
    with np.errstate(invalid="ignore"):
        capped = (dst["weights"] == ar.MAX_WEIGHT) & (want[1] == ar.MAX_WEIGHT) & (want[0].view(np.uint32) != dst["tsdf"].view(np.uint32))
    assert capped.sum() > 0  # fused at the cap: the tsdf moves, the weight word is not stored


def test_the_covering_box_of_the_library(dev):
    """box=None: emf_hip_occupancyObjectBox.  The volumes equal those of the whole box; the records differ in what lies
    outside alone."""
    from emfusion_amd import ops
    dt, dw, _ = sr.volume((40, 24, 20), "half_shell")
    st, sw, sf = sr.volume((33, 17, 9), "all_solid")
    dst, src = ar.dst_vol(dt, dw, 0.01, 0.04, ar.MAX_WEIGHT), ar.src_vol(st, sw, sf, 0.004, 0.03)
    for R, t in ar.poses(0.004)[:5]:
        pose = ar.pose_of(R, t)
        box = ops.absorb_box((40, 24, 20), 0.01, (33, 17, 9), 0.004, pose)
        full = ar.absorb(dst, src, pose)
        want = run(dst, src, pose, box, variants=("",), twice=False)
        assert want[0].tobytes() == full[0].tobytes() and want[1].tobytes() == full[1].tobytes()
        for k in ("unknown", "masked", "saturated", "fused", "fresh", "solid"):
            assert want[2][k] == full[2][k]
        assert want[2]["visited"] < full[2]["visited"] or t[0] == 100.0
        d_dst = dict(tsdf=to_dev(dt), weights=to_dev(dw), voxel_size=0.01, truncdist=0.04, max_weight=ar.MAX_WEIGHT)
        got = ops.absorb_volume(d_dst, upload_src(src, False), pose)  # the plain return value
        assert got.dtype == ar.ABSORB == ops.ABSORB_DTYPE and got.tobytes() == want[2].tobytes()
        assert d_dst["tsdf"].numpy().tobytes() == want[0].tobytes()
    assert full[2]["fused"] == 0 and min(box[1]) == 0  # the last pose: everything outside, an empty box


def test_the_refusals(dev):
    from emfusion_amd import _lib, ops
    lib = lib_for("")
    dt, dw, _ = sr.volume((5, 3, 2), "random")
    st, sw, sf = sr.volume((5, 3, 2), "all_solid")
    dst, src = ar.dst_vol(dt, dw, 0.01, 0.04, ar.MAX_WEIGHT), ar.src_vol(st, sw, sf, 0.01, 0.04)
    d_t, d_w, s = to_dev(dt), to_dev(dw), upload_src(src, False)
    rec = ops.DeviceArray((1 + EXTRA,), ar.ABSORB).fill_bytes_(POISON)
    eye, zero = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(0, 0, 0)

    def i3(*v):
        return (C.c_int32 * 3)(*v)

    def call(tsdf=d_t.ptr, weights=d_w.ptr, res=(5, 3, 2), voxel=0.01, trunc=0.04, max_weight=64.0, stsdf=s["tsdf"].ptr,
             sweights=s["weights"].ptr, mask=s["fg_mask"].ptr, tiles=None, sres=(5, 3, 2), svoxel=0.01, strunc=0.04, source=True,
             R=eye, t=zero, lo=(0, 0, 0), size=(5, 3, 2), record=rec.ptr):
        so = _lib.EmfAbsorbSource()
        so.tsdf, so.weights, so.fgVolMask, so.unseenTiles = stsdf, sweights, mask, tiles
        so.res, so.voxelSize, so.truncdist = i3(*sres), svoxel, strunc
        return lib.emf_hip_absorbVolume(tsdf, weights, None if res is None else i3(*res), voxel, trunc, max_weight,
                                        C.byref(so) if source else None, R, t, None if lo is None else i3(*lo),
                                        None if size is None else i3(*size), record, None)

    nan, inf = float("nan"), float("inf")
    for bad in (dict(tsdf=None), dict(weights=None), dict(res=None), dict(source=False), dict(stsdf=None), dict(sweights=None),
                dict(R=None), dict(t=None), dict(lo=None), dict(size=None), dict(record=None),
                dict(tsdf=d_t.ptr + 2), dict(weights=d_w.ptr + 1), dict(stsdf=s["tsdf"].ptr + 2), dict(sweights=s["weights"].ptr + 3),
                dict(record=rec.ptr + 4),
                dict(stsdf=d_t.ptr), dict(sweights=d_w.ptr), dict(stsdf=d_t.ptr, sweights=d_w.ptr), dict(weights=d_t.ptr),
                dict(stsdf=d_t.ptr + 8), dict(mask=d_w.ptr + 4), dict(tiles=d_t.ptr + 100), dict(record=d_t.ptr + 8),
                dict(record=s["weights"].ptr),
                dict(res=(0, 3, 2)), dict(res=(5, -1, 2)), dict(sres=(5, 3, 0)),
                dict(voxel=0.0), dict(voxel=-0.01), dict(voxel=nan), dict(voxel=inf), dict(svoxel=0.0), dict(svoxel=nan),
                dict(trunc=0.0), dict(trunc=inf), dict(strunc=-1.0), dict(strunc=nan), dict(max_weight=0.0), dict(max_weight=nan),
                dict(max_weight=inf), dict(trunc=1e-30, strunc=1e30), dict(trunc=1e30, strunc=1e-30),
                dict(lo=(-1, 0, 0)), dict(lo=(0, 0, 2), size=(5, 3, 1)), dict(size=(6, 3, 2)), dict(lo=(1, 0, 0)), dict(size=(5, -1, 2)),
                dict(lo=(6, 0, 0), size=(0, 3, 2))):
        assert call(**bad) == E_ARG, bad
    for bad in (dict(res=(2049, 1, 1)), dict(sres=(1, 1, 2049)), dict(res=(2048, 2048, 512)), dict(sres=(2048, 2048, 512))):
        assert call(**bad) == E_LIMIT, bad
    dev.synchronize()
    assert (rec.numpy().view(np.uint8) == POISON).all()  # nothing enqueued
    assert d_t.numpy().tobytes() == dt.tobytes() and d_w.numpy().tobytes() == dw.tobytes()
    # an empty box succeeds and writes the neutral record
    for lo, size in (((0, 0, 0), (5, 0, 2)), ((5, 3, 2), (0, 0, 0)), ((2, 1, 1), (0, 2, 1))):
        rec.fill_bytes_(POISON)
        assert call(lo=lo, size=size) == 0
        got = rec.numpy()
        assert got[0].tobytes() == ar.neutral((5, 3, 2)).tobytes() and (got[1:].view(np.uint8) == POISON).all()
    assert d_t.numpy().tobytes() == dt.tobytes() and d_w.numpy().tobytes() == dw.tobytes()
    assert call() == 0
    want = ar.absorb(dst, src, ar.pose_of())
    assert rec.numpy()[0].tobytes() == want[2].tobytes() and d_t.numpy().tobytes() == want[0].tobytes()
    assert d_w.numpy().tobytes() == want[1].tobytes() and want[2]["fused"] > 0
