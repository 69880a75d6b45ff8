"""emf_hip_absorbVolumeColor, emf_hip_seedVolumeColor and emf_hip_releaseVolumeColor (include/emf_hip.h "Absorbing a
volume" and "Lifting a volume") against tests/transfer_color_reference.py, byte for byte, in the default
library and in the one built with a*b+c contraction on: the sweeps of the absorption's and the lift's restatements with
colour volumes attached -- entries with about a third Wc == 0, weights up to the cap, the full u16 range in all four values
-- over the shapes (1,1,1), (5,3,2), (33,17,9), (64,8,8), (40,24,20), with and without the mask and the unseen-tile map, the
boxes whole / one / cut / empty, the truncation ratios 1, 0.5 and 2 and the planted wall.  Per case the colour volume, the
colour record, tsdf, weights and the geometry record equal the restatement, and tsdf, weights and the geometry record equal
the PLAIN entry's output on a copy of the same inputs.  The destination's three arrays lie between poisoned guards, both
records are poisoned beforehand and nothing is written beyond them; src_color = NULL; a second call; inputs are only read;
every refusal with nothing enqueued."""
import ctypes as C

import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import lift_reference as lr
from tests import shape_reference as sr
from tests import transfer_color_reference as tc
from tests.parity_util import to_dev
from tests.resample_util import GUARD, POISON, Guarded, lib_for, upload_src

pytestmark = pytest.mark.gpu

f32 = np.float32
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
EXTRA = 3    # records of room behind the one a call writes


class GuardedColor:
    """A colour volume between two poisoned guards; the view is 8-byte aligned (GUARD u16 quadruples in front)."""

    def __init__(self, host):
        from emfusion_amd.devmem import DeviceArray, DeviceView
        self.n = host.size // 4
        self.buf = DeviceArray((self.n + 2 * GUARD, 4), np.uint16).fill_bytes_(POISON)
        self.view = DeviceView(self.buf.ptr + 8 * GUARD, host.shape, np.uint16)
        self.view.copy_from(host)

    def read(self):
        raw = self.buf.numpy()
        assert (raw[:GUARD].view(np.uint8) == POISON).all() and (raw[GUARD + self.n:].view(np.uint8) == POISON).all(), \
            "written outside the colour volume"
        return raw[GUARD:GUARD + self.n].reshape(self.view.shape)


def upload_color(src, d_src):
    return dict(d_src, color=None if src.get("color") is None else to_dev(src["color"]))


def upload_claim(claim):
    return dict(fg_mask=None if claim["fg"] is None else to_dev(claim["fg"]), res=claim["res"], voxel_size=claim["voxel_size"])


def compare(what, rec, crec, gt, gw, gc, expect):
    got, cgot = rec.numpy(), crec.numpy()
    assert got[0].tobytes() == expect[2].tobytes(), (what, got[0], expect[2])
    assert cgot[0].tobytes() == expect[4].tobytes(), (what, cgot[0], expect[4])
    assert (got[1:].view(np.uint8) == POISON).all() and (cgot[1:].view(np.uint8) == POISON).all(), "written beyond a record"
    t, w, c = gt.read(), gw.read(), gc.read()
    assert t.tobytes() == expect[0].tobytes() and w.tobytes() == expect[1].tobytes(), what
    bad = np.argwhere((c != expect[3]).any(axis=3))
    assert len(bad) == 0, (what, len(bad), bad[:3], [(c[tuple(b)], expect[3][tuple(b)]) for b in bad[:3]])


def run(kind, dst, other, pose, box, variants=("", "_fma"), maps=(False, True), twice=True):
    """One colour pass of `kind` (absorb | seed | release) in every asked library -- absorb and seed with and without the
    source's unseen-tile map -- into a guarded destination with poisoned records, once more on top of the result, and the
    plain entry on a copy of the same inputs; returns the expected (tsdf, weights, record, color, colour record)."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    statement = dict(absorb=tc.absorb_color, seed=tc.seed_color, release=tc.release_color)[kind]
    call = dict(absorb=ops.absorb_volume, seed=ops.seed_volume, release=ops.release_volume)[kind]
    dtype, which = dict(absorb=(ar.ABSORB, "fused"), seed=(lr.SEED, "seeded"), release=(lr.RELEASE, "released"))[kind]
    want = statement(dst, other, pose, box)
    tc.check_identities(want[2], want[4], which)
    want2 = statement(dict(dst, tsdf=want[0], weights=want[1], color=want[3]), other, pose, box) if twice else None
    if want2 is not None and kind != "absorb":  # KEPT / EMPTY now: no colour byte moves
        assert want2[3].tobytes() == want[3].tobytes() and want2[4].tobytes() == tc.moved().tobytes()
    for with_map in (maps if kind != "release" else (False,)):
        d_other = upload_claim(other) if kind == "release" else upload_color(other, upload_src(other, with_map))
        for variant in variants:
            gt, gw, gc = Guarded(dst["tsdf"]), Guarded(dst["weights"]), GuardedColor(dst["color"])
            d_dst = dict(tsdf=gt.view, weights=gw.view, color=gc.view, voxel_size=dst["voxel_size"], truncdist=dst["truncdist"],
                         max_weight=dst["max_weight"])
            rec = DeviceArray((1 + EXTRA,), dtype).fill_bytes_(POISON)
            crec = DeviceArray((1 + EXTRA,), tc.COLOR_MOVED).fill_bytes_(POISON)
            for expect in (want, want2):
                if expect is None:
                    continue
                got = call(d_dst, d_other, pose, box=box, out=rec, color_out=crec, lib=lib_for(variant))
                assert got[0] is rec and got[1] is crec
                compare((kind, variant, with_map), rec, crec, gt, gw, gc, expect)
            # the plain entry on a copy of the same inputs, once per case and library: the same tsdf, weights and geometry record
            if with_map and len(maps) > 1:
                continue
            pt, pw = Guarded(dst["tsdf"]), Guarded(dst["weights"])
            plain = DeviceArray((1,), dtype).fill_bytes_(POISON)
            call(dict(d_dst, tsdf=pt.view, weights=pw.view, color=None), d_other, pose, box=box, out=plain, lib=lib_for(variant))
            assert plain.numpy()[0].tobytes() == want[2].tobytes()
            assert pt.read().tobytes() == want[0].tobytes() and pw.read().tobytes() == want[1].tobytes()
        # inputs are only read
        if kind == "release":
            assert other["fg"] is None or d_other["fg_mask"].numpy().tobytes() == other["fg"].tobytes()
        else:
            assert d_other["tsdf"].numpy().tobytes() == other["tsdf"].tobytes()
            assert d_other["weights"].numpy().tobytes() == other["weights"].tobytes()
            assert other["fg"] is None or d_other["fg_mask"].numpy().tobytes() == other["fg"].tobytes()
            assert other["color"] is None or d_other["color"].numpy().tobytes() == other["color"].tobytes()
    return want


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_absorb_with_colour(dev, shape, content):
    colored = uncolored = nulls = 0
    for name, dst, src, pose, box in tc.absorb_cases(shape, content):
        want = run("absorb", dst, src, pose, box, twice=name.rsplit("-", 2)[1] == "whole")
        colored, uncolored = colored + int(want[4]["colored"]), uncolored + int(want[4]["uncolored"])
        nulls += src["color"] is None
    assert nulls > 0
    if min(shape) >= 8 and content in ("half_shell", "gated_block", "random", "all_solid"):
        assert colored > 0 and uncolored > 0


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_seed_with_colour(dev, shape, content):
    colored = uncolored = nulls = 0
    for name, dst, src, pose, box in tc.seed_cases(shape, content):
        want = run("seed", dst, src, pose, box, twice=name.rsplit("-", 2)[1] == "whole")
        colored, uncolored = colored + int(want[4]["colored"]), uncolored + int(want[4]["uncolored"])
        nulls += src["color"] is None
    assert nulls > 0
    if min(shape) >= 8 and content in ("half_shell", "gated_block", "random", "all_solid"):
        assert colored > 0 and uncolored > 0


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_release_with_colour(dev, shape, content):
    cleared = zero = 0
    for name, dst, claim, pose, box in tc.release_cases(shape, content):
        want = run("release", dst, claim, pose, box, twice="whole" in name)
        cleared, zero = cleared + int(want[4]["colored"]), zero + int(want[4]["uncolored"])
    if min(shape) >= 8:
        assert cleared > 0 and zero > 0


def test_whole_boxes_of_the_large_destinations(dev):
    """Every case of the destinations with more than one tile over the WHOLE box: several workgroups, tiles the volume cuts
    on every axis."""
    moved = dict(absorb=0, seed=0, release=0)
    for shape in ((40, 24, 20), (33, 17, 9), (64, 8, 8)):
        for content in ("half_shell", "gated_block", "all_solid"):
            for kind, cases in (("absorb", tc.absorb_cases), ("seed", tc.seed_cases), ("release", tc.release_cases)):
                for name, dst, other, pose, box in cases(shape, content, boxes=("whole",)):
                    if "pose4" in name or "pose5" in name:
                        continue
                    want = run(kind, dst, other, pose, box, variants=("",), maps=(True,), twice=False)
                    moved[kind] += int(want[4]["colored"]) + int(want[4]["uncolored"])
    assert min(moved.values()) > 1000, moved


def test_the_planted_wall_and_the_three_ratios(dev):
    for name, ratio, dst, src, pose in tc.planted_cases():
        for kind, which in (("absorb", "fused"), ("seed", "seeded")):
            want = run(kind, dst, src, pose, ar.whole(dst))
            assert want[2][which] > 0 and want[2]["unknown"] > 0, (name, kind)


def test_the_cap_at_the_top_of_the_range_and_the_plain_return(dev):
    """maxWeight 300: capq is 65535; maxWeight 0.001: capq is 1.  Without out= the calls return numpy records."""
    from emfusion_amd import ops
    shape = (33, 17, 9)
    st, sw, sf = sr.volume(shape, "all_solid")
    dt, dw, _ = sr.volume(shape, "random")
    for max_weight in (300.0, 0.001):
        dst = dict(ar.dst_vol(dt, dw, 0.01, 0.04, max_weight), color=tc.color_volume(shape, "hostile", 7))
        src = dict(ar.src_vol(st, sw, sf, 0.01, 0.04), color=tc.color_volume(shape, "hostile", 8))
        for kind in ("absorb", "seed"):
            want = run(kind, dst, src, ar.pose_of(None, (0.0031, 0.0047, 0.0013)), ar.whole(dst), maps=(False,), twice=False)
            assert want[4]["colored"] > 50
    d_dst = dict(tsdf=to_dev(dt), weights=to_dev(dw), color=to_dev(dst["color"]), voxel_size=0.01, truncdist=0.04, max_weight=0.001)
    got = ops.absorb_volume(d_dst, upload_color(src, upload_src(src, False)), ar.pose_of(None, (0.0031, 0.0047, 0.0013)))
    want = tc.absorb_color(dst, src, ar.pose_of(None, (0.0031, 0.0047, 0.0013)))
    assert got[0].dtype == ar.ABSORB and got[1].dtype == tc.COLOR_MOVED == ops.COLOR_MOVED_DTYPE
    assert got[0].tobytes() == want[2].tobytes() and got[1].tobytes() == want[4].tobytes()
    assert d_dst["color"].numpy().tobytes() == want[3].tobytes()
    claim = lr.claim_of(sf, shape, 0.01)
    got = ops.release_volume(d_dst, upload_claim(claim), ar.pose_of())
    rel = tc.release_color(dict(dst, tsdf=want[0], weights=want[1], color=want[3]), claim, ar.pose_of())
    assert got[0].tobytes() == rel[2].tobytes() and got[1].tobytes() == rel[4].tobytes() and rel[4]["colored"] > 50
    assert d_dst["color"].numpy().tobytes() == rel[3].tobytes()


def i3(*v):
    return (C.c_int32 * 3)(*v)


def test_the_refusals(dev):
    from emfusion_amd import _lib, ops
    lib = lib_for("")
    shape = (5, 3, 2)
    dt, dw, _ = sr.volume(shape, "random")
    st, sw, sf = sr.volume(shape, "all_solid")
    dc, sc = tc.color_volume(shape, "weighted", 1), tc.color_volume(shape, "hostile", 2)
    dst = dict(ar.dst_vol(dt, dw, 0.01, 0.04, lr.MAX_WEIGHT), color=dc)
    src = dict(ar.src_vol(st, sw, sf, 0.01, 0.04), color=sc)
    d_t, d_w, d_c, s = to_dev(dt), to_dev(dw), to_dev(dc), upload_color(src, upload_src(src, False))
    recs = {k: ops.DeviceArray((1 + EXTRA,), d).fill_bytes_(POISON) for k, d in (("absorb", ar.ABSORB), ("seed", lr.SEED), ("release", lr.RELEASE))}
    crec = ops.DeviceArray((1 + EXTRA,), tc.COLOR_MOVED).fill_bytes_(POISON)
    eye, zero = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(0, 0, 0)
    nan, inf = float("nan"), float("inf")

    def transfer(kind):
        entry = getattr(lib, "emf_hip_%sVolumeColor" % kind)

        def call(tsdf=d_t.ptr, weights=d_w.ptr, color=d_c.ptr, res=shape, voxel=0.01, trunc=0.04, max_weight=64.0, stsdf=s["tsdf"].ptr,
                 sweights=s["weights"].ptr, mask=s["fg_mask"].ptr, tiles=None, scolor=s["color"].ptr, sres=shape, svoxel=0.01,
                 strunc=0.04, source=True, R=eye, t=zero, lo=(0, 0, 0), size=shape, record=recs[kind].ptr, crecord=crec.ptr):
            so = _lib.EmfAbsorbSource()
            so.tsdf, so.weights, so.fgVolMask, so.unseenTiles = stsdf, sweights, mask, tiles
            so.res, so.voxelSize, so.truncdist = i3(*sres), svoxel, strunc
            return entry(tsdf, weights, color, None if res is None else i3(*res), voxel, trunc, max_weight,
                         C.byref(so) if source else None, scolor, R, t, None if lo is None else i3(*lo),
                         None if size is None else i3(*size), record, crecord, None)
        return call

    def release(tsdf=d_t.ptr, weights=d_w.ptr, color=d_c.ptr, res=shape, voxel=0.01, mask=s["fg_mask"].ptr, cres=shape, cvoxel=0.01,
                R=eye, t=zero, lo=(0, 0, 0), size=shape, record=recs["release"].ptr, crecord=crec.ptr):
        return lib.emf_hip_releaseVolumeColor(tsdf, weights, color, None if res is None else i3(*res), voxel, mask,
                                              None if cres is None else i3(*cres), cvoxel, R, t, None if lo is None else i3(*lo),
                                              None if size is None else i3(*size), record, crecord, None)

    # what the colour entries add, then what their siblings refuse
    color_bad = [dict(color=None), dict(crecord=None), dict(color=d_c.ptr + 4), dict(color=d_c.ptr + 2), dict(crecord=crec.ptr + 4),
                 dict(color=d_t.ptr), dict(color=d_w.ptr + 8), dict(color=s["fg_mask"].ptr), dict(crecord=d_t.ptr + 8), dict(crecord=d_w.ptr),
                 dict(crecord=d_c.ptr + 16), dict(crecord=s["fg_mask"].ptr + 8), dict(color=crec.ptr), dict(tsdf=d_c.ptr),
                 dict(weights=d_c.ptr + 8)]
    transfer_bad = color_bad + [dict(scolor=s["color"].ptr + 4), dict(scolor=d_c.ptr), dict(scolor=crec.ptr), dict(color=s["color"].ptr),
                                dict(color=s["tsdf"].ptr), dict(color=s["weights"].ptr + 8), dict(crecord=s["tsdf"].ptr),
                                dict(crecord=s["color"].ptr + 8), dict(tiles=d_c.ptr + 16),
                                dict(tsdf=None), dict(weights=None), dict(res=None), dict(source=False), dict(stsdf=None),
                                dict(sweights=None), dict(R=None), dict(t=None), dict(lo=None), dict(size=None), dict(record=None),
                                dict(tsdf=d_t.ptr + 2), dict(stsdf=s["tsdf"].ptr + 2), dict(stsdf=d_t.ptr), dict(weights=d_t.ptr),
                                dict(res=(0, 3, 2)), dict(sres=(5, 3, 0)), dict(voxel=0.0), dict(svoxel=nan), dict(trunc=inf),
                                dict(strunc=-1.0), dict(max_weight=0.0), dict(max_weight=nan), dict(trunc=1e-30, strunc=1e30),
                                dict(lo=(-1, 0, 0)), dict(size=(6, 3, 2)), dict(size=(5, -1, 2))]
    for kind in ("absorb", "seed"):
        call = transfer(kind)
        for bad in transfer_bad + [dict(record=crec.ptr), dict(crecord=recs[kind].ptr), dict(record=recs[kind].ptr + 4)]:
            assert call(**bad) == E_ARG, (kind, bad)
        for bad in (dict(res=(2049, 1, 1)), dict(sres=(1, 1, 2049)), dict(res=(2048, 2048, 512))):
            assert call(**bad) == E_LIMIT, (kind, bad)
    for bad in color_bad + [dict(record=crec.ptr), dict(crecord=recs["release"].ptr), dict(tsdf=None), dict(cres=None), dict(record=None),
                            dict(weights=d_t.ptr), dict(mask=d_t.ptr), dict(res=(0, 3, 2)), dict(cvoxel=nan), dict(size=(6, 3, 2))]:
        assert release(**bad) == E_ARG, bad
    assert release(res=(2049, 1, 1)) == E_LIMIT
    dev.synchronize()
    for r in list(recs.values()) + [crec]:
        assert (r.numpy().view(np.uint8) == POISON).all()  # nothing enqueued
    assert d_t.numpy().tobytes() == dt.tobytes() and d_w.numpy().tobytes() == dw.tobytes() and d_c.numpy().tobytes() == dc.tobytes()
    # an empty box succeeds and writes both neutral records
    for kind, call, neutral in (("absorb", transfer("absorb"), ar.neutral(shape)), ("seed", transfer("seed"), lr.neutral(lr.SEED, shape)),
                                ("release", release, lr.neutral(lr.RELEASE, shape))):
        for lo, size in (((0, 0, 0), (5, 0, 2)), ((5, 3, 2), (0, 0, 0)), ((2, 1, 1), (0, 2, 1))):
            recs[kind].fill_bytes_(POISON), crec.fill_bytes_(POISON)
            assert call(lo=lo, size=size) == 0
            got, cgot = recs[kind].numpy(), crec.numpy()
            assert got[0].tobytes() == neutral.tobytes() and (got[1:].view(np.uint8) == POISON).all()
            assert cgot[0].tobytes() == tc.moved().tobytes() and (cgot[1:].view(np.uint8) == POISON).all()
    assert d_t.numpy().tobytes() == dt.tobytes() and d_w.numpy().tobytes() == dw.tobytes() and d_c.numpy().tobytes() == dc.tobytes()
    # and the calls as they stand run: src_color NULL, then the source's colour
    assert transfer("absorb")(scolor=None) == 0
    want = tc.absorb_color(dst, dict(src, color=None), ar.pose_of())
    assert recs["absorb"].numpy()[0].tobytes() == want[2].tobytes() and crec.numpy()[0].tobytes() == want[4].tobytes()
    assert d_c.numpy().tobytes() == want[3].tobytes() and want[2]["fused"] == want[4]["uncolored"] > 0
    assert transfer("absorb")() == 0
    want = tc.absorb_color(dict(dst, tsdf=want[0], weights=want[1], color=want[3]), src, ar.pose_of())
    assert d_c.numpy().tobytes() == want[3].tobytes() and d_t.numpy().tobytes() == want[0].tobytes() and want[4]["colored"] > 0
    assert crec.numpy()[0].tobytes() == want[4].tobytes()
