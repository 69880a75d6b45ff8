"""emf_hip_seedVolume and emf_hip_releaseVolume (include/emf_hip.h "Lifting a volume") against
tests/lift_reference.py, byte for byte, in the default library and in the one built with a*b+c contraction on: the sweep
of the restatement -- destinations of its shapes, unobserved, fully observed, half observed and with weights 0, negative,
NaN and at maxWeight, against a source or claimant on the same lattice, a finer and a coarser one, with and without the
mask (the release: a claim mask, a NULL claim, an all-zero claim) and the unseen-tile map, under the six poses and the
truncation ratios 1, 0.5 and 2; the whole box, one voxel, a box that cuts tiles, an empty box, the library's covering box;
equal lattices at a voxel size of 0.25 where q is exact; a second call.  The destination lies between poisoned guards, the
record is poisoned beforehand and nothing is written beyond it; inputs are only read; every refusal."""
import ctypes as C

import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import lift_reference as lr
from tests import shape_reference as sr
from tests.parity_util import to_dev
from tests.resample_util import GUARD, POISON, Guarded, lib_for, upload_src

pytestmark = pytest.mark.gpu

f32 = np.float32
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
EXTRA = 3    # records of room behind the one a call writes


def upload_claim(claim):
    return dict(fg_mask=None if claim["fg"] is None else to_dev(claim["fg"]), res=claim["res"], voxel_size=claim["voxel_size"])


def compare(kind, variant, rec, gt, gw, expect, dtype):
    got = rec.numpy()
    assert got[0].tobytes() == expect[2].tobytes(), (kind, variant, got[0], expect[2])
    assert (got[1:].view(np.uint8) == POISON).all(), "written beyond the record"
    t, w = gt.read(), gw.read()
    bad = np.argwhere((t.view(np.uint32) != expect[0].view(np.uint32)) | (w.view(np.uint32) != expect[1].view(np.uint32)))
    assert len(bad) == 0, (kind, variant, len(bad), bad[:3], [(t[tuple(b)], expect[0][tuple(b)], w[tuple(b)], expect[1][tuple(b)])
                                                                 for b in bad[:3]])


def run_seed(dst, src, pose, box, variants=("", "_fma"), maps=(False, True), twice=True):
    """One seed in every asked library, with and without the source's unseen-tile map, into a guarded destination and a
    poisoned record, and once more on top of the result; returns the expected (tsdf, weights, record)."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    want = lr.seed(dst, src, pose, box)
    lr.check_identities(want[2])
    want2 = None
    if twice:  # what was seeded is KEPT now, everything else falls where it fell
        want2 = lr.seed(dict(dst, tsdf=want[0], weights=want[1]), src, pose, box)
        assert want2[0].tobytes() == want[0].tobytes() and want2[1].tobytes() == want[1].tobytes() and want2[2]["seeded"] == 0
        assert want2[2]["kept"] == want[2]["kept"] + want[2]["seeded"]
    for with_map in maps:
        d_src = upload_src(src, with_map)
        for variant in variants:
            gt, gw = Guarded(dst["tsdf"]), Guarded(dst["weights"])
            d_dst = dict(tsdf=gt.view, weights=gw.view, voxel_size=dst["voxel_size"], truncdist=dst["truncdist"],
                         max_weight=dst["max_weight"])
            rec = DeviceArray((1 + EXTRA,), lr.SEED).fill_bytes_(POISON)
            for expect in (want, want2):
                if expect is None:
                    continue
                assert ops.seed_volume(d_dst, d_src, pose, box=box, out=rec, lib=lib_for(variant)) is rec
                compare("seed", (variant, with_map), rec, gt, gw, expect, lr.SEED)
        # inputs are only read
        assert d_src["tsdf"].numpy().tobytes() == src["tsdf"].tobytes() and d_src["weights"].numpy().tobytes() == src["weights"].tobytes()
        assert src["fg"] is None or d_src["fg_mask"].numpy().tobytes() == src["fg"].tobytes()
    return want


def run_release(dst, claim, pose, box, variants=("", "_fma"), twice=True):
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    want = lr.release(dst, claim, pose, box)
    lr.check_identities(want[2])
    want2 = None
    if twice:  # what was released is EMPTY now
        want2 = lr.release(dict(dst, tsdf=want[0], weights=want[1]), claim, pose, box)
        assert want2[0].tobytes() == want[0].tobytes() and want2[1].tobytes() == want[1].tobytes() and want2[2]["released"] == 0
        assert want2[2]["empty"] == want[2]["empty"] + want[2]["released"]
    d_claim = upload_claim(claim)
    for variant in variants:
        gt, gw = Guarded(dst["tsdf"]), Guarded(dst["weights"])
        d_dst = dict(tsdf=gt.view, weights=gw.view, voxel_size=dst["voxel_size"])
        rec = DeviceArray((1 + EXTRA,), lr.RELEASE).fill_bytes_(POISON)
        for expect in (want, want2):
            if expect is None:
                continue
            assert ops.release_volume(d_dst, d_claim, pose, box=box, out=rec, lib=lib_for(variant)) is rec
            compare("release", variant, rec, gt, gw, expect, lr.RELEASE)
    assert claim["fg"] is None or d_claim["fg_mask"].numpy().tobytes() == claim["fg"].tobytes()
    return want


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_seed_one_destination_from_three_sources(dev, shape, content):
    total = np.zeros((), lr.SEED)
    for name, dst, src, pose, box in lr.seed_cases(shape, content):
        want = run_seed(dst, src, pose, box, twice=name.endswith("whole"))
        for k in lr.SEED_COUNTS:
            total[k] += want[2][k]
    assert total["kept"] > 0 and total["outside"] > 0 and total["visited"] > total["seeded"]
    if min(shape) >= 8 and content in ("half_shell", "gated_block", "random", "all_solid"):
        assert total["seeded"] > 0 and total["saturated"] > 0
    if min(shape) >= 8 and content in ("half_shell", "gated_block", "random"):
        assert total["unknown"] > 0 and total["masked"] > 0


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_release_one_destination_to_three_claimants(dev, shape, content):
    total = np.zeros((), lr.RELEASE)
    for name, dst, claim, pose, box in lr.release_cases(shape, content):
        want = run_release(dst, claim, pose, box, twice="whole" in name)
        assert not name.endswith("-zero") or want[2]["released"] == 0
        for k in lr.RELEASE_COUNTS:
            total[k] += want[2][k]
    assert total["empty"] > 0
    if shape != (1, 1, 1):
        assert total["released"] > 0 and total["free_space"] > 0 and total["outside"] > 0 and total["unclaimed"] > 0


def test_whole_boxes_of_the_large_destinations(dev):
    """Every case of the destinations with more than one tile over the WHOLE box (the sweep gives each case one kind of
    box): several workgroups, tiles the volume cuts on every axis."""
    seeded = released = 0
    for shape in ((40, 24, 20), (33, 17, 9), (64, 8, 8)):
        for content in ("half_shell", "gated_block", "all_solid"):
            for name, dst, src, pose, box in lr.seed_cases(shape, content, boxes=("whole",)):
                if "pose4" in name or "pose5" in name:
                    continue
                seeded += int(run_seed(dst, src, pose, box, variants=("",), maps=(True,), twice=False)[2]["seeded"])
            for name, dst, claim, pose, box in lr.release_cases(shape, content, boxes=("whole",)):
                if "pose4" in name or "pose5" in name:
                    continue
                released += int(run_release(dst, claim, pose, box, variants=("",), twice=False)[2]["released"])
    assert seeded > 1000 and released > 1000, (seeded, released)


def test_the_planted_corners_and_both_band_rules(dev):
    """NaN and -0.0 tsdf and a zero, a negative and a NaN weight at single corners of the source's cells, a wall saturated
    on both sides; truncation ratio 0.5 (s saturated, u not) and 2 (the opposite)."""
    sat = {}
    for name, ratio, dst, src, pose in lr.planted_cases():
        want = run_seed(dst, src, pose, ar.whole(dst))
        assert want[2]["unknown"] > 0 and want[2]["kept"] > 0 and want[2]["seeded"] > 0
        sat[name[-5:], ratio] = int(want[2]["saturated"])
    assert 0 < sat["pose0", 0.5] == sat["pose0", 1.0] < sat["pose0", 2.0]


def test_equal_lattices_where_q_is_exact(dev):
    """Voxel size 0.25 and shifts of whole and half voxels make q exact: q = v + shift lands exactly on 0, on N - 2 (the
    last inside cell), on N - 1 (outside) and on the .5 ties of rint, which go to the even voxel."""
    shape = (33, 17, 9)
    rng = np.random.default_rng(5)
    other = rng.uniform(-0.999, 0.999, shape[::-1]).astype(f32)
    fg = rng.choice(np.array([0, 1, 255], np.uint8), shape[::-1])
    src = ar.src_vol(other, np.full(other.shape, 3.0, f32), fg, 0.25, 0.5)
    dt, dw, _ = sr.volume(shape, "random")
    dst = ar.dst_vol(dt, dw, 0.25, 0.5, lr.MAX_WEIGHT)
    claim = lr.claim_of(fg, shape, 0.25)
    with np.errstate(invalid="ignore"):
        fresh, band = ~(dw > 0), (dw > 0) & (np.abs(dt) < 1)
    for shift in ((0, 0, 0), (-3, 0, 0), (2, 0, 0), (1, -2, 1), (0, 3, -4), (0.5, 0, 0), (1.5, -0.5, 2.5)):
        pose = ar.pose_of(None, [0.25 * s for s in shift])
        want = run_seed(dst, src, pose, ar.whole(dst), twice=False)
        rel = run_release(dst, claim, pose, ar.whole(dst), twice=False)
        z, y, x = np.meshgrid(*[np.arange(n) for n in shape[::-1]], indexing="ij")
        q = [c + s for c, s in zip((x, y, z), shift)]
        inside = np.ones(x.shape, bool)
        for j in range(3):
            inside &= (q[j] >= 0) & (q[j] + 1 < shape[j])  # the pad-1 rule: q in [0, N - 1)
        r = [np.rint(np.where(inside, c, 0)).astype(np.int64) for c in q]  # numpy's rint: ties to even
        gate = inside & (fg[r[2], r[1], r[0]] != 0)
        assert want[2]["outside"] == (fresh & ~inside).sum() > 0 and want[2]["unknown"] == 0
        assert want[2]["masked"] == (fresh & inside & ~gate).sum() > 0
        assert rel[2]["released"] == (band & gate).sum() > 100 and rel[2]["unclaimed"] == (band & inside & ~gate).sum() > 0
        if all(float(s).is_integer() for s in shift):  # a seeded voxel holds the source's own bits
            ok = fresh & gate
            zz, yy, xx = np.nonzero(ok)
            moved = other[zz + int(shift[2]), yy + int(shift[1]), xx + int(shift[0])]
            assert want[2]["seeded"] == ok.sum() > 100 and want[0][ok].tobytes() == moved.tobytes() and (want[1][ok] == 3.0).all()


def test_the_covering_box_of_the_library(dev):
    """box=None: emf_hip_occupancyObjectBox.  The volumes equal those of the whole box; the records differ in what lies
    outside (and, for the seed, in what is kept) alone."""
    from emfusion_amd import ops
    dt, dw, _ = sr.volume((40, 24, 20), "half_shell")
    st, sw, sf = sr.volume((33, 17, 9), "all_solid")
    dst, src = ar.dst_vol(dt, dw, 0.01, 0.04, lr.MAX_WEIGHT), ar.src_vol(st, sw, sf, 0.004, 0.03)
    claim = lr.claim_of(sf, (33, 17, 9), 0.004)
    for R, t in ar.poses(0.004)[:5]:
        pose = ar.pose_of(R, t)
        box = ops.absorb_box((40, 24, 20), 0.01, (33, 17, 9), 0.004, pose)
        full = lr.seed(dst, src, pose)
        want = run_seed(dst, src, pose, box, variants=("",), twice=False)
        assert want[0].tobytes() == full[0].tobytes() and want[1].tobytes() == full[1].tobytes()
        for k in ("unknown", "masked", "saturated", "seeded", "solid"):
            assert want[2][k] == full[2][k]
        assert want[2]["visited"] < full[2]["visited"] or t[0] == 100.0
        d_dst = dict(tsdf=to_dev(dt), weights=to_dev(dw), voxel_size=0.01, truncdist=0.04, max_weight=lr.MAX_WEIGHT)
        got = ops.seed_volume(d_dst, upload_src(src, False), pose)  # the plain return value
        assert got.dtype == lr.SEED == ops.SEED_DTYPE and got.tobytes() == want[2].tobytes()
        assert d_dst["tsdf"].numpy().tobytes() == want[0].tobytes()
        rfull = lr.release(dst, claim, pose)
        rwant = run_release(dst, claim, pose, box, variants=("",), twice=False)
        assert rwant[0].tobytes() == rfull[0].tobytes() and rwant[1].tobytes() == rfull[1].tobytes()
        for k in ("unclaimed", "released", "solid"):
            assert rwant[2][k] == rfull[2][k]
        d_dst = dict(tsdf=to_dev(dt), weights=to_dev(dw), voxel_size=0.01)
        got = ops.release_volume(d_dst, upload_claim(claim), pose)
        assert got.dtype == lr.RELEASE == ops.RELEASE_DTYPE and got.tobytes() == rwant[2].tobytes()
        assert d_dst["weights"].numpy().tobytes() == rwant[1].tobytes()
    assert full[2]["seeded"] == 0 and min(box[1]) == 0  # the last pose: everything outside, an empty box


def test_the_refusals_of_the_seed(dev):
    from emfusion_amd import _lib, ops
    lib = lib_for("")
    dt, dw, _ = sr.volume((5, 3, 2), "random")
    st, sw, sf = sr.volume((5, 3, 2), "all_solid")
    dst, src = ar.dst_vol(dt, dw, 0.01, 0.04, lr.MAX_WEIGHT), ar.src_vol(st, sw, sf, 0.01, 0.04)
    d_t, d_w, s = to_dev(dt), to_dev(dw), upload_src(src, False)
    rec = ops.DeviceArray((1 + EXTRA,), lr.SEED).fill_bytes_(POISON)
    eye, zero = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(0, 0, 0)

    def i3(*v):
        return (C.c_int32 * 3)(*v)

    def call(tsdf=d_t.ptr, weights=d_w.ptr, res=(5, 3, 2), voxel=0.01, trunc=0.04, max_weight=64.0, stsdf=s["tsdf"].ptr,
             sweights=s["weights"].ptr, mask=s["fg_mask"].ptr, tiles=None, sres=(5, 3, 2), svoxel=0.01, strunc=0.04, source=True,
             R=eye, t=zero, lo=(0, 0, 0), size=(5, 3, 2), record=rec.ptr):
        so = _lib.EmfAbsorbSource()
        so.tsdf, so.weights, so.fgVolMask, so.unseenTiles = stsdf, sweights, mask, tiles
        so.res, so.voxelSize, so.truncdist = i3(*sres), svoxel, strunc
        return lib.emf_hip_seedVolume(tsdf, weights, None if res is None else i3(*res), voxel, trunc, max_weight,
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
        assert got[0].tobytes() == lr.neutral(lr.SEED, (5, 3, 2)).tobytes() and (got[1:].view(np.uint8) == POISON).all()
    assert d_t.numpy().tobytes() == dt.tobytes() and d_w.numpy().tobytes() == dw.tobytes()
    assert call() == 0
    want = lr.seed(dst, src, ar.pose_of())
    assert rec.numpy()[0].tobytes() == want[2].tobytes() and d_t.numpy().tobytes() == want[0].tobytes()
    assert d_w.numpy().tobytes() == want[1].tobytes() and want[2]["seeded"] > 0


def test_the_refusals_of_the_release(dev):
    from emfusion_amd import ops
    lib = lib_for("")
    dt, dw, _ = sr.volume((5, 3, 2), "all_solid")
    _, _, sf = sr.volume((5, 3, 2), "all_solid")
    dst, claim = ar.dst_vol(dt, dw, 0.01, 0.04, lr.MAX_WEIGHT), lr.claim_of(sf, (5, 3, 2), 0.01)
    d_t, d_w, d_c = to_dev(dt), to_dev(dw), to_dev(sf)
    rec = ops.DeviceArray((1 + EXTRA,), lr.RELEASE).fill_bytes_(POISON)
    eye, zero = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(0, 0, 0)

    def i3(*v):
        return (C.c_int32 * 3)(*v)

    def call(tsdf=d_t.ptr, weights=d_w.ptr, res=(5, 3, 2), voxel=0.01, mask=d_c.ptr, cres=(5, 3, 2), cvoxel=0.01, R=eye, t=zero,
             lo=(0, 0, 0), size=(5, 3, 2), record=rec.ptr):
        return lib.emf_hip_releaseVolume(tsdf, weights, None if res is None else i3(*res), voxel, mask,
                                         None if cres is None else i3(*cres), cvoxel, R, t, None if lo is None else i3(*lo),
                                         None if size is None else i3(*size), record, None)

    nan, inf = float("nan"), float("inf")
    for bad in (dict(tsdf=None), dict(weights=None), dict(res=None), dict(cres=None), dict(R=None), dict(t=None), dict(lo=None),
                dict(size=None), dict(record=None),
                dict(tsdf=d_t.ptr + 2), dict(weights=d_w.ptr + 1), dict(record=rec.ptr + 4),
                dict(weights=d_t.ptr), dict(mask=d_t.ptr), dict(mask=d_w.ptr + 4), dict(record=d_t.ptr + 8), dict(record=d_w.ptr),
                dict(record=d_c.ptr),
                dict(res=(0, 3, 2)), dict(res=(5, -1, 2)), dict(cres=(5, 3, 0)),
                dict(voxel=0.0), dict(voxel=-0.01), dict(voxel=nan), dict(voxel=inf), dict(cvoxel=0.0), dict(cvoxel=nan),
                dict(lo=(-1, 0, 0)), dict(lo=(0, 0, 2), size=(5, 3, 1)), dict(size=(6, 3, 2)), dict(lo=(1, 0, 0)), dict(size=(5, -1, 2)),
                dict(lo=(6, 0, 0), size=(0, 3, 2))):
        assert call(**bad) == E_ARG, bad
    for bad in (dict(res=(2049, 1, 1)), dict(cres=(1, 1, 2049)), dict(res=(2048, 2048, 512)), dict(cres=(2048, 2048, 512), mask=None)):
        assert call(**bad) == E_LIMIT, bad
    dev.synchronize()
    assert (rec.numpy().view(np.uint8) == POISON).all()  # nothing enqueued
    assert d_t.numpy().tobytes() == dt.tobytes() and d_w.numpy().tobytes() == dw.tobytes()
    for lo, size in (((0, 0, 0), (5, 0, 2)), ((5, 3, 2), (0, 0, 0)), ((2, 1, 1), (0, 2, 1))):
        rec.fill_bytes_(POISON)
        assert call(lo=lo, size=size) == 0
        got = rec.numpy()
        assert got[0].tobytes() == lr.neutral(lr.RELEASE, (5, 3, 2)).tobytes() and (got[1:].view(np.uint8) == POISON).all()
    assert d_t.numpy().tobytes() == dt.tobytes() and d_w.numpy().tobytes() == dw.tobytes()
    assert call() == 0
    want = lr.release(dst, claim, ar.pose_of())
    assert rec.numpy()[0].tobytes() == want[2].tobytes() and d_t.numpy().tobytes() == want[0].tobytes()
    assert d_w.numpy().tobytes() == want[1].tobytes() and want[2]["released"] > 0
    assert d_c.numpy().tobytes() == sf.tobytes()
