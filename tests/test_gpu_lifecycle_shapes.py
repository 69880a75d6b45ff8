"""The life-cycle kernels (lifecycle.hip, k_hide_label of pixel_ops.hip) at the sizes and values that steer them, against
the numpy references of tests/lifecycle_cases.py; tests/test_lifecycle_cases_cpu.py shows that each case reaches what it
is named for.  Order statistics, counts, masks and the masses of weights k / 4096 are compared byte for byte; the one
tolerance of the file is the derived bound of the arbitrary-weights mass."""
import math

import numpy as np
import pytest

from tests import lifecycle_cases as LC
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu
f32 = np.float32
I3 = np.eye(3, dtype=f32)
Z3 = np.zeros(3, f32)
EMF_E_SHAPE, EMF_E_ARG = -2, -4


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops as _ops
    return _ops


def same_stats(got, want):
    (gn, g10, g90), (n, p10, p90) = got, want
    assert gn == n
    assert g10.tobytes() == p10.astype(f32).tobytes(), (g10, p10)
    assert g90.tobytes() == p90.astype(f32).tobytes(), (g90, p90)


# ---- order statistics ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", LC.ORDER_CASES, ids=[LC.order_id(c) for c in LC.ORDER_CASES])
def test_select_by_bit_pattern_equals_sorting(ops, dev, case):
    points, mask = LC.order_case(case)
    pad_points, pad_mask = case[3]
    got = ops.masked_point_stats(to_dev(points, dev, pad_points), to_dev(mask, dev, pad_mask), I3, Z3)
    same_stats(got, LC.sorted_stats(points, mask, I3, Z3))


@pytest.mark.parametrize("n", LC.COUNTS)
def test_select_at_small_counts(ops, dev, n):
    points, mask = LC.counts_case(n)
    same_stats(ops.masked_point_stats(to_dev(points, dev), to_dev(mask, dev, 3), I3, Z3),
               LC.sorted_stats(points, mask, I3, Z3))


def test_select_of_rotated_points_pitched(ops, dev):
    w, h, R, t = LC.ROTATED
    points, mask = LC.cloud_image(w, h, seed=1)
    same_stats(ops.masked_point_stats(to_dev(points, dev, 2), to_dev(mask, dev, 5), R, t),
               LC.sorted_stats(points, mask, R, t))


def test_second_call_on_the_same_buffers_equals_a_fresh_call(ops, dev):
    """A full case, then fewer points in other buckets, with the scratch and the output of the first call: nothing of
    the first call (histograms, prefixes, residual ranks, count) may survive into the second."""
    from emfusion_amd.devmem import DeviceArray
    from emfusion_amd._lib import load
    full_points, full_mask = LC.order_case(LC.ORDER_CASES[1])
    points, mask = LC.counts_case(11)
    buffers = (DeviceArray.zeros((int(load().emf_hip_pointStatsScratchBytes()) // 4,), np.uint32).fill_bytes_(0x5A),
               DeviceArray.zeros((7,), f32).fill_bytes_(0x5A))
    first = ops.masked_point_stats(to_dev(full_points, dev), to_dev(full_mask, dev), I3, Z3, buffers=buffers)
    same_stats(first, LC.sorted_stats(full_points, full_mask, I3, Z3))
    second = ops.masked_point_stats(to_dev(points, dev), to_dev(mask, dev), I3, Z3, buffers=buffers)
    fresh = ops.masked_point_stats(to_dev(points, dev), to_dev(mask, dev), I3, Z3)
    same_stats(second, fresh)
    same_stats(second, LC.sorted_stats(points, mask, I3, Z3))
    assert second[0] == 11 < first[0]


@pytest.mark.parametrize("case", LC.EXTENT_CASES, ids=[c[0] for c in LC.EXTENT_CASES])
def test_extent_stats_equal_mesh_cloud_plus_points(ops, dev, case):
    c = LC.extent_case(case)
    got = ops.object_extent_stats(to_dev(c["points"], dev, 1), to_dev(c["mask"], dev, 2), c["R"], c["t"],
                                  to_dev(c["tsdf"]), to_dev(c["weights"]),
                                  None if c["fg"] is None else to_dev(c["fg"]), c["voxel"])
    same_stats(got, LC.extent_reference(c))


def test_extent_stats_refuse_a_flat_volume(ops, dev):
    """Resolution (1, 8, 8) has no cube (and n.x - 1 = 0 would divide): the shape error, and nothing enqueued."""
    from emfusion_amd.devmem import DeviceArray
    from emfusion_amd._lib import EmfHipError, load
    points, mask = LC.cloud_image(5, 3, seed=2)
    vol = np.ones((8, 8, 1), f32)
    buffers = (DeviceArray.zeros((int(load().emf_hip_pointStatsScratchBytes()) // 4,), np.uint32).fill_bytes_(0x5A),
               DeviceArray.zeros((7,), f32).fill_bytes_(0x5A))
    with pytest.raises(EmfHipError) as err:
        ops.object_extent_stats(to_dev(points), to_dev(mask), I3, Z3, to_dev(vol), to_dev(vol), None, 0.02,
                                buffers=buffers)
    assert err.value.code == EMF_E_SHAPE
    assert (buffers[0].numpy().view(np.uint8) == 0x5A).all() and (buffers[1].numpy().view(np.uint8) == 0x5A).all()


# ---- association mass --------------------------------------------------------------------------------------------------

def seeded_mass_out(ops):
    from emfusion_amd.devmem import DeviceArray
    from emfusion_amd._lib import load
    return DeviceArray.zeros((int(load().emf_hip_maskAssociationMassBytes()) // 8,), np.float64).fill_bytes_(0x3F)


@pytest.mark.parametrize("with_match", [False, True], ids=["alone", "match"])
@pytest.mark.parametrize("w, h", LC.MASS_SIZES, ids=[f"{w}x{h}" for w, h in LC.MASS_SIZES])
def test_mass_of_dyadic_weights_is_exact(ops, dev, w, h, with_match):
    seg, match, k = LC.mass_case(w, h)
    m = match if with_match else None
    pad_seg, pad_match, pad_assoc = LC.MASS_PADS
    # the output starts as non-zero bytes (0x3F3F...: doubles near 4.8e-4): a partial that is added to, or left
    # unwritten, shows
    n, total = ops.mask_association_mass(to_dev(seg, dev, pad_seg), None if m is None else to_dev(m, dev, pad_match),
                                         to_dev(LC.weights_of(k), dev, pad_assoc), out=seeded_mass_out(ops))
    want_n, want = LC.mass_reference(seg, m, k)
    assert n == want_n
    assert np.float64(total).tobytes() == want.tobytes(), (total, want)


def test_mass_of_arbitrary_weights(ops, dev):
    """float32 weights in [0, 1] against math.fsum.  The kernels add n values in n - 1 additions, in some fixed order;
    each addition rounds a partial sum that is at most n (every weight is <= 1), so it errs by at most half an ulp of
    it, <= n * 2^-53; n - 1 of them: |sum - exact| < n * n * 2^-53."""
    w, h = 257, 241
    rng = np.random.default_rng(8)
    seg, match, _ = LC.mass_case(w, h)
    assoc = rng.uniform(0, 1, (h, w)).astype(f32)
    inside = (seg != 0) | (match != 0)
    n, total = ops.mask_association_mass(to_dev(seg, dev, 2), to_dev(match, dev), to_dev(assoc, dev, 1),
                                         out=seeded_mass_out(ops))
    exact = math.fsum(assoc[inside].astype(np.float64).tolist())
    assert n == int(inside.sum())
    print("arbitrary weights: n", n, "sum", total, "exact", exact, "error", total - exact, "bound", n * n * 2.0 ** -53)
    assert abs(total - exact) <= n * n * 2.0 ** -53


def test_batched_masses_and_verdicts_against_numpy(ops, dev):
    b, c = LC.BATCH, LC.batched_case()
    want_counts, want_sums, want_verdict = LC.batched_reference(c)
    segs = [to_dev(s, dev) for s in c["segs"]]
    assocs = [to_dev(LC.weights_of(k), dev) for k in c["ks"]]
    matches = [None if m is None else to_dev(m, dev, 1 + i % 3) for i, m in enumerate(c["matches"])]
    verdict = dict(nall=b["nall"], list_pos=c["list_pos"], visible=c["visible"], ex_low=c["ex_low"],
                   assoc_thresh=b["thresh"])
    counts, sums, got_verdict = ops.mask_association_masses(segs, assocs, matches, verdict, seed_byte=0x3F)
    assert np.array_equal(counts, want_counts), np.flatnonzero(counts != want_counts)
    assert sums.tobytes() == want_sums.tobytes(), np.flatnonzero(sums != want_sums)
    # the tie (thr * count == sum) is kept, the invisible and the low-existence object go, the positions of no object
    # of the call and the padding are zero (the array started as 7.0)
    assert got_verdict.tobytes() == want_verdict.tobytes(), (got_verdict, want_verdict)


# ---- overlap, carving, hiding ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", LC.OVERLAP_KINDS)
@pytest.mark.parametrize("w, h", LC.IMAGE_SIZES, ids=[f"{w}x{h}" for w, h in LC.IMAGE_SIZES])
def test_overlap_counts_equal_counting(ops, dev, w, h, kind):
    seg, model = LC.overlap_case(w, h, kind)
    n, inter, area = ops.mask_overlap(to_dev(seg, dev, 3), to_dev(model, dev, 6))
    want_n, want_inter, want_area = LC.overlap_reference(seg, model)
    assert n == want_n
    assert np.array_equal(inter, want_inter), np.flatnonzero(inter != want_inter)   # absent ids included: zero
    assert np.array_equal(area, want_area), np.flatnonzero(area != want_area)


@pytest.mark.parametrize("with_match", [False, True], ids=["model", "match"])
@pytest.mark.parametrize("obj_id", [1, 255])
@pytest.mark.parametrize("kind", LC.CARVE_KINDS)
@pytest.mark.parametrize("w, h", LC.IMAGE_SIZES, ids=[f"{w}x{h}" for w, h in LC.IMAGE_SIZES])
def test_carve_equals_where(ops, dev, w, h, kind, obj_id, with_match):
    seg, model, match = LC.carve_case(w, h, kind, obj_id)
    m = match if with_match else None
    d_seg = to_dev(seg, dev, 1)
    pre, post = ops.carve_mask(d_seg, to_dev(model, dev, 4), obj_id, None if m is None else to_dev(m, dev, 2))
    want, want_pre, want_post = LC.carve_reference(seg, model, m, obj_id)
    assert (pre, post) == (want_pre, want_post)
    assert d_seg.numpy().tobytes() == want.tobytes()


def test_carve_refusals_leave_the_mask_alone(ops, dev):
    from emfusion_amd._lib import EmfHipError
    seg, model, match = LC.carve_case(161, 77, "mixed", 1)
    d_seg, d_model = to_dev(seg, dev, 1), to_dev(model, dev)
    for obj_id, other, code in ((0, d_model, EMF_E_ARG), (256, d_model, EMF_E_ARG),
                                (1, to_dev(model[:, :-1], dev), EMF_E_SHAPE), (1, to_dev(model[:-1], dev), EMF_E_SHAPE)):
        with pytest.raises(EmfHipError) as err:
            ops.carve_mask(d_seg, other, obj_id)
        assert err.value.code == code, (obj_id, err.value)
    with pytest.raises(EmfHipError) as err:
        ops.carve_mask(d_seg, d_model, 1, to_dev(match[:-1], dev))
    assert err.value.code == EMF_E_SHAPE
    assert d_seg.numpy().tobytes() == seg.tobytes()


def test_hide_label_equals_masked_copies(ops, dev):
    host = LC.hide_case()
    for label in (LC.HIDE["label"], LC.HIDE["absent"]):
        seg, vert, nrm, bgv, bgn = (to_dev(a, dev, p) for a, p in zip(host, LC.HIDE["pads"]))
        ops.hide_label(seg, label, vert, nrm, bgv, bgn)
        want_seg, want_vert, want_nrm = LC.hide_reference(*host, label)
        assert seg.numpy().tobytes() == want_seg.tobytes()
        # the label's pixels: the background's vertex and normal; all others untouched -- NaN payloads included
        assert vert.numpy().tobytes() == want_vert.tobytes() and nrm.numpy().tobytes() == want_nrm.tobytes()
        assert bgv.numpy().tobytes() == host[3].tobytes() and bgn.numpy().tobytes() == host[4].tobytes()
