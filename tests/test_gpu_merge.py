"""emf_hip_mergeVolume and emf_hip_mergeVolumeColor (include/emf_hip.h "Merging a volume") against
tests/merge_reference.py, byte for byte, in the default library and in the one built with a*b+c contraction on: the sweep of
the absorption's restatement with count volumes attached -- pairs (0, 0), fg == bg, fg one above and one below bg, and a
pair whose sum rounds -- over the shapes (1,1,1), (5,3,2), (33,17,9), (64,8,8), (40,24,20), with and without the source's
unseen-tile map, plain and with colour; whole boxes of the destinations with more than one tile; equal lattices where q
lands on 0, N - 2, N - 1 and the .5 ties of rint; per case tsdf, weights and the record equal ops.absorb_volume's on a copy
of the same inputs.  The destination's arrays lie between poisoned guards, the records are poisoned beforehand and nothing
is written beyond them; a second call; inputs are only read; every refusal with nothing enqueued."""
import ctypes as C

import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import merge_reference as mr
from tests import shape_reference as sr
from tests import transfer_color_reference as tc
from tests.parity_util import to_dev
from tests.resample_util import GUARD, POISON, Guarded, lib_for, upload_src
from tests.test_gpu_transfer_color import GuardedColor

pytestmark = pytest.mark.gpu

f32 = np.float32
E_ARG, E_LIMIT = -4, -5  # include/emf_hip.h EMF_E_ARG, EMF_E_LIMIT
EXTRA = 3    # records of room behind the one a call writes


class GuardedPairs:
    """A count volume between two poisoned guards; the view is 8-byte aligned (GUARD pairs in front)."""

    def __init__(self, host):
        from emfusion_amd.devmem import DeviceArray, DeviceView
        self.n = host.size // 2
        self.buf = DeviceArray((self.n + 2 * GUARD, 2), np.float32).fill_bytes_(POISON)
        self.view = DeviceView(self.buf.ptr + 8 * GUARD, host.shape, np.float32)
        self.view.copy_from(host)

    def read(self):
        raw = self.buf.numpy()
        assert (raw[:GUARD].view(np.uint8) == POISON).all() and (raw[GUARD + self.n:].view(np.uint8) == POISON).all(), \
            "written outside the count volume"
        return raw[GUARD:GUARD + self.n].reshape(self.view.shape)


def upload(src, with_map):
    d = dict(upload_src(src, with_map), fgbg=to_dev(src["fgbg"]))
    if "color" in src:
        d["color"] = None if src["color"] is None else to_dev(src["color"])
    return d


def bits(a):
    return a.view(np.uint32)


def run(dst, src, pose, box, variants=("", "_fma"), maps=(False, True), twice=True):
    """One merge -- with colour where dst has a colour volume -- in every asked library, with and without the source's
    unseen-tile map, into a guarded destination with poisoned records, once more on top of the result, and the plain
    absorption on a copy of the same inputs; returns the expected tuple of merge_reference.merge(_color)."""
    from emfusion_amd import ops
    from emfusion_amd.devmem import DeviceArray
    colored = "color" in dst
    statement = mr.merge_color if colored else mr.merge
    want = statement(dst, src, pose, box)
    mr.check_identities(want[2], want[4])
    after = dict(dst, tsdf=want[0], weights=want[1], fgbg=want[3])
    if colored:
        after["color"] = want[5]
    want2 = statement(after, src, pose, box) if twice else None
    for with_map in maps:
        d_src = upload(src, with_map)
        for variant in variants:
            gt, gw, gp = Guarded(dst["tsdf"]), Guarded(dst["weights"]), GuardedPairs(dst["fgbg"])
            gc = GuardedColor(dst["color"]) if colored else None
            d_dst = dict(tsdf=gt.view, weights=gw.view, fgbg=gp.view, voxel_size=dst["voxel_size"], truncdist=dst["truncdist"],
                         max_weight=dst["max_weight"])
            if colored:
                d_dst["color"] = gc.view
            rec = DeviceArray((1 + EXTRA,), ar.ABSORB).fill_bytes_(POISON)
            cnt = DeviceArray((1 + EXTRA,), mr.MERGE_COUNTS).fill_bytes_(POISON)
            crec = DeviceArray((1 + EXTRA,), tc.COLOR_MOVED).fill_bytes_(POISON) if colored else None
            for expect in (want, want2):
                if expect is None:
                    continue
                got = ops.merge_volume(d_dst, d_src, pose, box=box, out=rec, counts_out=cnt, color_out=crec, lib=lib_for(variant))
                assert got[0] is rec and got[1] is cnt and (not colored or got[2] is crec)
                what = (variant, with_map)
                r, c = rec.numpy(), cnt.numpy()
                assert r[0].tobytes() == expect[2].tobytes(), (what, r[0], expect[2])
                assert c[0].tobytes() == expect[4].tobytes(), (what, c[0], expect[4])
                assert (r[1:].view(np.uint8) == POISON).all() and (c[1:].view(np.uint8) == POISON).all(), "written beyond a record"
                t, w, p = gt.read(), gw.read(), gp.read()
                assert t.tobytes() == expect[0].tobytes() and w.tobytes() == expect[1].tobytes(), what
                bad = np.argwhere((bits(p) != bits(expect[3])).any(axis=3))
                assert len(bad) == 0, (what, len(bad), bad[:3], [(p[tuple(b)], expect[3][tuple(b)]) for b in bad[:3]])
                if colored:
                    k = crec.numpy()
                    assert k[0].tobytes() == expect[6].tobytes() and (k[1:].view(np.uint8) == POISON).all(), (what, k[0], expect[6])
                    assert gc.read().tobytes() == expect[5].tobytes(), what
            # the plain absorption on a copy of the same inputs, once per case and library: the same tsdf, weights and record
            if with_map and len(maps) > 1:
                continue
            pt, pw = Guarded(dst["tsdf"]), Guarded(dst["weights"])
            plain = DeviceArray((1,), ar.ABSORB).fill_bytes_(POISON)
            assert ops.ABSORB_DTYPE == ar.ABSORB
            ops.absorb_volume(dict(tsdf=pt.view, weights=pw.view, voxel_size=dst["voxel_size"], truncdist=dst["truncdist"],
                                   max_weight=dst["max_weight"]), d_src, pose, box=box, out=plain, lib=lib_for(variant))
            assert plain.numpy()[0].tobytes() == want[2].tobytes()
            assert pt.read().tobytes() == want[0].tobytes() and pw.read().tobytes() == want[1].tobytes()
        # inputs are only read
        assert d_src["tsdf"].numpy().tobytes() == src["tsdf"].tobytes() and d_src["weights"].numpy().tobytes() == src["weights"].tobytes()
        assert d_src["fg_mask"].numpy().tobytes() == src["fg"].tobytes() and d_src["fgbg"].numpy().tobytes() == src["fgbg"].tobytes()
        assert src.get("color") is None or d_src["color"].numpy().tobytes() == src["color"].tobytes()
    return want


@pytest.mark.parametrize("colored", (False, True), ids=("plain", "colour"))
@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_one_destination_against_three_sources(dev, shape, content, colored):
    """The sweep of merge_reference.cases: a source of the destination's lattice, a finer and a coarser one, six poses;
    truncation ratios, destination contents, boxes and count volumes in turn."""
    fused = foreground = gained = 0
    for name, dst, src, pose, box in (mr.color_cases if colored else mr.cases)(shape, content):
        kind = name.rsplit("-", 2)[1] if colored else name.rsplit("-", 1)[1]
        want = run(dst, src, pose, box, twice=kind == "whole")
        fused, foreground, gained = fused + int(want[2]["fused"]), foreground + int(want[4]["foreground"]), gained + int(want[4]["gained"])
    assert fused > 0
    if min(shape) >= 8:
        assert fused > foreground > gained > 0, (fused, foreground, gained)


def test_whole_boxes_of_the_large_destinations(dev):
    """Every case of the destinations with more than one tile over the WHOLE box: several workgroups, tiles the volume
    cuts on every axis."""
    fresh = mixed = 0
    for shape in ((40, 24, 20), (33, 17, 9), (64, 8, 8)):
        for content in ("half_shell", "gated_block", "all_solid"):
            for cases in (mr.cases, mr.color_cases):
                for name, dst, src, pose, box in cases(shape, content, boxes=("whole",)):
                    if "pose4" in name or "pose5" in name:
                        continue
                    want = run(dst, src, pose, box, variants=("",), maps=(True,), twice=False)
                    fresh, mixed = fresh + int(want[2]["fresh"]), mixed + int(want[2]["fused"] - want[2]["fresh"])
    assert fresh > 1000 and mixed > 1000, (fresh, mixed)


def test_equal_lattices_the_edge_cells_and_the_ties_of_rint(dev):
    """Voxel size 0.25 and shifts of whole and half voxels make q exact: q = v + shift.  With whole shifts q is exactly 0,
    exactly N - 2 (the last inside cell) and exactly N - 1 (outside) for some voxels of the box and a FRESH voxel's pair
    is the pair of source voxel v + shift; with half shifts every rint is a tie and goes to the even voxel."""
    shape = (33, 17, 9)
    rng = np.random.default_rng(5)
    other = rng.uniform(-0.999, 0.999, shape[::-1]).astype(f32)
    pairs = mr.count_volume(shape, 2)
    src = dict(ar.src_vol(other, np.full(other.shape, 3.0, f32), np.ones(other.shape, np.uint8), 0.25, 0.5), fgbg=pairs)
    dt, dw, _ = sr.volume(shape, "random")
    dst = dict(ar.dst_vol(dt, dw, 0.25, 0.5, ar.MAX_WEIGHT), fgbg=mr.count_volume(shape, 1))
    with np.errstate(invalid="ignore"):
        fresh = ~(dw > 0)
    for shift in ((0, 0, 0), (-3, 0, 0), (2, 0, 0), (1, -2, 1), (0, 3, -4)):
        want = run(dst, src, ar.pose_of(None, [0.25 * s for s in shift]), ar.whole(dst), twice=False)
        inside = [max(0, min(shape[j] - 1, shape[j] - 2 - shift[j]) - max(0, -shift[j]) + 1) for j in range(3)]  # q in [0, N - 2]
        assert want[2]["fused"] == inside[0] * inside[1] * inside[2] and want[2]["unknown"] == 0
        z, y, x = np.nonzero(fresh)
        ok = (x + shift[0] >= 0) & (x + shift[0] <= shape[0] - 2) & (y + shift[1] >= 0) & (y + shift[1] <= shape[1] - 2) & \
             (z + shift[2] >= 0) & (z + shift[2] <= shape[2] - 2)
        z, y, x = z[ok], y[ok], x[ok]
        assert len(x) > 100 and want[3][z, y, x].tobytes() == pairs[z + shift[2], y + shift[1], x + shift[0]].tobytes()
    for shift in ((0.5, 0, 0), (0.5, 0.5, 0.5), (-1.5, 2.5, 0.5)):
        want = run(dst, src, ar.pose_of(None, [0.25 * s for s in shift]), ar.whole(dst), twice=False)
        z, y, x = np.nonzero(fresh)
        q = [x + shift[0], y + shift[1], z + shift[2]]
        ok = np.ones(len(x), bool)
        for j in range(3):
            ok &= (q[j] >= 0) & (q[j] + 1 < shape[j])
        r = [np.rint(c[ok]).astype(np.int64) for c in q]  # numpy rounds ties to even as well
        assert ok.sum() > 100 and want[3][z[ok], y[ok], x[ok]].tobytes() == pairs[r[2], r[1], r[0]].tobytes()
        assert any((c[ok] % 1 == 0.5).any() for c in q)


def test_source_values_at_a_cells_corner(dev):
    """The planted wall: NaN and -0.0 tsdf and a zero, a negative and a NaN weight at single corners of the source's cells,
    into a destination with weights 0, negative, NaN and at maxWeight."""
    dst, src, poses = mr.planted_case()
    for pose in poses:
        want = run(dst, src, pose, ar.whole(dst))
        assert want[2]["unknown"] > 0 and want[2]["fresh"] > 0 and want[2]["fused"] > want[2]["fresh"] and want[2]["masked"] > 0


def test_the_covering_box_and_the_plain_return(dev):
    """box=None: emf_hip_occupancyObjectBox; without out= the call returns numpy records."""
    from emfusion_amd import ops
    for colored in (False, True):
        name, dst, src, pose, _ = next(iter((mr.color_cases if colored else mr.cases)((40, 24, 20), "half_shell", boxes=("whole",))))
        src = dict(src, voxel_size=f32(0.004))
        full = (mr.merge_color if colored else mr.merge)(dst, src, pose)
        d_dst = dict(tsdf=to_dev(dst["tsdf"]), weights=to_dev(dst["weights"]), fgbg=to_dev(dst["fgbg"]), voxel_size=dst["voxel_size"],
                     truncdist=dst["truncdist"], max_weight=dst["max_weight"])
        if colored:
            d_dst["color"] = to_dev(dst["color"])
        got = ops.merge_volume(d_dst, upload(src, False), pose)
        assert len(got) == (3 if colored else 2) and got[0].dtype == ar.ABSORB and got[1].dtype == mr.MERGE_COUNTS == ops.MERGE_COUNTS_DTYPE
        assert got[0]["visited"] < full[2]["visited"] and got[0]["fused"] == full[2]["fused"] > 0
        assert got[1].tobytes() == full[4].tobytes() and (not colored or got[2].tobytes() == full[6].tobytes())
        assert d_dst["tsdf"].numpy().tobytes() == full[0].tobytes() and d_dst["weights"].numpy().tobytes() == full[1].tobytes()
        assert d_dst["fgbg"].numpy().tobytes() == full[3].tobytes()
        assert not colored or d_dst["color"].numpy().tobytes() == full[5].tobytes()


def i3(*v):
    return (C.c_int32 * 3)(*v)


def test_the_refusals(dev):
    from emfusion_amd import _lib, ops
    lib = lib_for("")
    shape = (5, 3, 2)
    dt, dw, _ = sr.volume(shape, "random")
    st, sw, sf = sr.volume(shape, "all_solid")
    dp, sp = mr.count_volume(shape, 1), mr.count_volume(shape, 2)
    dc, sc = tc.color_volume(shape, "weighted", 1), tc.color_volume(shape, "hostile", 2)
    dst = dict(ar.dst_vol(dt, dw, 0.01, 0.04, ar.MAX_WEIGHT), fgbg=dp, color=dc)
    src = dict(ar.src_vol(st, sw, sf, 0.01, 0.04), fgbg=sp, color=sc)
    d_t, d_w, d_p, d_c, s = to_dev(dt), to_dev(dw), to_dev(dp), to_dev(dc), upload(src, False)
    rec = ops.DeviceArray((1 + EXTRA,), ar.ABSORB).fill_bytes_(POISON)
    cnt = ops.DeviceArray((1 + EXTRA,), mr.MERGE_COUNTS).fill_bytes_(POISON)
    crec = ops.DeviceArray((1 + EXTRA,), tc.COLOR_MOVED).fill_bytes_(POISON)
    eye, zero = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(0, 0, 0)
    nan, inf = float("nan"), float("inf")

    def call(colored, tsdf=d_t.ptr, weights=d_w.ptr, fgbg=d_p.ptr, color=d_c.ptr, res=shape, voxel=0.01, trunc=0.04, max_weight=64.0,
             stsdf=s["tsdf"].ptr, sweights=s["weights"].ptr, mask=s["fg_mask"].ptr, tiles=None, sfgbg=s["fgbg"].ptr,
             scolor=s["color"].ptr, sres=shape, svoxel=0.01, strunc=0.04, source=True, R=eye, t=zero, lo=(0, 0, 0), size=shape,
             record=rec.ptr, counts=cnt.ptr, crecord=crec.ptr):
        so = _lib.EmfAbsorbSource()
        so.tsdf, so.weights, so.fgVolMask, so.unseenTiles = stsdf, sweights, mask, tiles
        so.res, so.voxelSize, so.truncdist = i3(*sres), svoxel, strunc
        head = (None if res is None else i3(*res), voxel, trunc, max_weight, C.byref(so) if source else None)
        tail = (R, t, None if lo is None else i3(*lo), None if size is None else i3(*size), record, counts)
        if colored:
            return lib.emf_hip_mergeVolumeColor(tsdf, weights, fgbg, color, *head, sfgbg, scolor, *tail, crecord, None)
        return lib.emf_hip_mergeVolume(tsdf, weights, fgbg, *head, sfgbg, *tail, None)

    # what the merge adds, then what the absorption refuses
    merge_bad = [dict(mask=None), dict(fgbg=None), dict(sfgbg=None), dict(counts=None),
                 dict(fgbg=d_p.ptr + 4), dict(sfgbg=s["fgbg"].ptr + 4), dict(counts=cnt.ptr + 4),
                 dict(fgbg=d_t.ptr), dict(fgbg=d_w.ptr + 8), dict(fgbg=s["fgbg"].ptr), dict(fgbg=s["tsdf"].ptr), dict(fgbg=s["fg_mask"].ptr),
                 dict(fgbg=rec.ptr), dict(fgbg=cnt.ptr), dict(sfgbg=d_p.ptr + 8), dict(sfgbg=d_t.ptr), dict(sfgbg=d_w.ptr + 8),
                 dict(sfgbg=rec.ptr + 8), dict(sfgbg=cnt.ptr), dict(counts=d_t.ptr + 8), dict(counts=d_w.ptr), dict(counts=d_p.ptr + 16),
                 dict(counts=rec.ptr + 8), dict(counts=s["tsdf"].ptr), dict(counts=s["fgbg"].ptr + 8), dict(counts=s["fg_mask"].ptr + 8),
                 dict(tsdf=d_p.ptr), dict(weights=d_p.ptr + 8), dict(record=d_p.ptr), dict(record=cnt.ptr), dict(tiles=d_p.ptr + 16),
                 dict(stsdf=d_p.ptr), dict(mask=d_p.ptr + 4)]
    absorb_bad = [dict(tsdf=None), dict(weights=None), dict(res=None), dict(source=False), dict(stsdf=None), dict(sweights=None),
                  dict(R=None), dict(t=None), dict(lo=None), dict(size=None), dict(record=None),
                  dict(tsdf=d_t.ptr + 2), dict(weights=d_w.ptr + 1), dict(stsdf=s["tsdf"].ptr + 2), dict(record=rec.ptr + 4),
                  dict(stsdf=d_t.ptr), dict(sweights=d_w.ptr), dict(weights=d_t.ptr), dict(mask=d_w.ptr + 4), dict(tiles=d_t.ptr + 100),
                  dict(record=d_t.ptr + 8), dict(record=s["weights"].ptr),
                  dict(res=(0, 3, 2)), dict(res=(5, -1, 2)), dict(sres=(5, 3, 0)), dict(voxel=0.0), dict(voxel=nan), dict(svoxel=inf),
                  dict(trunc=0.0), dict(strunc=nan), dict(max_weight=0.0), dict(max_weight=inf), dict(trunc=1e-30, strunc=1e30),
                  dict(lo=(-1, 0, 0)), dict(lo=(0, 0, 2), size=(5, 3, 1)), dict(size=(6, 3, 2)), dict(size=(5, -1, 2))]
    color_bad = [dict(color=None), dict(crecord=None), dict(color=d_c.ptr + 4), dict(crecord=crec.ptr + 4), dict(scolor=s["color"].ptr + 4),
                 dict(color=d_t.ptr), dict(color=d_p.ptr), dict(color=s["fgbg"].ptr), dict(color=cnt.ptr), dict(color=s["color"].ptr),
                 dict(crecord=d_p.ptr + 8), dict(crecord=cnt.ptr), dict(crecord=s["fgbg"].ptr), dict(crecord=rec.ptr),
                 dict(fgbg=d_c.ptr), dict(fgbg=s["color"].ptr), dict(fgbg=crec.ptr), dict(counts=d_c.ptr + 8), dict(counts=crec.ptr),
                 dict(counts=s["color"].ptr + 8), dict(sfgbg=d_c.ptr + 8), dict(sfgbg=crec.ptr)]
    for colored in (False, True):
        for bad in merge_bad + absorb_bad + (color_bad if colored else []):
            assert call(colored, **bad) == E_ARG, (colored, bad)
        for bad in (dict(res=(2049, 1, 1)), dict(sres=(1, 1, 2049)), dict(res=(2048, 2048, 512))):
            assert call(colored, **bad) == E_LIMIT, (colored, bad)
    dev.synchronize()
    for r in (rec, cnt, crec):
        assert (r.numpy().view(np.uint8) == POISON).all()  # nothing enqueued
    untouched = lambda: d_t.numpy().tobytes() == dt.tobytes() and d_w.numpy().tobytes() == dw.tobytes() and \
        d_p.numpy().tobytes() == dp.tobytes() and d_c.numpy().tobytes() == dc.tobytes()
    assert untouched()
    # an empty box succeeds and writes the neutral records
    for colored in (False, True):
        for lo, size in (((0, 0, 0), (5, 0, 2)), ((5, 3, 2), (0, 0, 0)), ((2, 1, 1), (0, 2, 1))):
            for r in (rec, cnt, crec):
                r.fill_bytes_(POISON)
            assert call(colored, lo=lo, size=size) == 0
            got, cgot, kgot = rec.numpy(), cnt.numpy(), crec.numpy()
            assert got[0].tobytes() == ar.neutral(shape).tobytes() and (got[1:].view(np.uint8) == POISON).all()
            assert cgot[0].tobytes() == mr.counts().tobytes() and (cgot[1:].view(np.uint8) == POISON).all()
            if colored:
                assert kgot[0].tobytes() == tc.moved().tobytes() and (kgot[1:].view(np.uint8) == POISON).all()
            else:
                assert (kgot.view(np.uint8) == POISON).all()
    assert untouched()
    # and the calls as they stand run: plain, then with colour on top of it
    assert call(False) == 0
    want = mr.merge(dst, src, ar.pose_of())
    assert rec.numpy()[0].tobytes() == want[2].tobytes() and cnt.numpy()[0].tobytes() == want[4].tobytes() and want[2]["fused"] > 0
    assert d_t.numpy().tobytes() == want[0].tobytes() and d_w.numpy().tobytes() == want[1].tobytes()
    assert d_p.numpy().tobytes() == want[3].tobytes() and d_c.numpy().tobytes() == dc.tobytes()
    assert call(True) == 0
    want = mr.merge_color(dict(dst, tsdf=want[0], weights=want[1], fgbg=want[3]), src, ar.pose_of())
    assert rec.numpy()[0].tobytes() == want[2].tobytes() and cnt.numpy()[0].tobytes() == want[4].tobytes()
    assert crec.numpy()[0].tobytes() == want[6].tobytes() and d_c.numpy().tobytes() == want[5].tobytes()
    assert d_p.numpy().tobytes() == want[3].tobytes() and d_t.numpy().tobytes() == want[0].tobytes()
