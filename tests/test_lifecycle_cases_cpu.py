"""The inputs of tests/test_gpu_lifecycle_shapes.py, checked without a GPU: every case reaches the property it is named
for, shown from the references of tests/lifecycle_cases.py alone -- which key byte of the selected element decides, where
the rank lies against a run or the sign change, how many points are left, which bands of k_mask_mass hold rows.  A
generator that is changed so that a case misses its property fails here, not silently on the GPU."""
import math

import numpy as np
import pytest

from tests import lifecycle_cases as LC

f32 = np.float32
I3 = np.eye(3, dtype=f32)
Z3 = np.zeros(3, f32)


def channel_cases():
    seen = []
    for case in LC.ORDER_CASES:
        w, h, chans, _ = case
        for axis, name in enumerate(chans):
            seen.append(pytest.param(case, axis, name, id=f"{w}x{h}-{'xyz'[axis]}-{name}"))
    return seen


def test_every_case_runs_where_the_list_says():
    at = {}
    for w, h, chans, pad in LC.ORDER_CASES:
        assert len(set(chans)) == 3                                           # the selections of a call diverge
        for name in chans:
            at.setdefault(name, set()).add((w, h))
    assert set(at) == set(LC.CHANNELS)
    assert all((64, 48) in sizes for sizes in at.values())                    # each case at 64 x 48
    sign = at["sign_last_negative"] & at["sign_first_positive"]
    assert sign >= {(1, 1), (5, 3), (257, 3), (161, 77)}
    assert at["tie_run"] >= {(161, 77), (640, 480)}
    assert 257 * 3 < LC.TIE_MIN <= 64 * 48                                    # why tie_run is absent at 5 x 3 and 257 x 3
    pitched = {c[:2]: c[3] for c in LC.ORDER_CASES if c[3] != (0, 0)}           # points and mask, padded differently
    assert set(pitched) == {(1, 1), (5, 3), (257, 3), (161, 77)} and all(a and b and a != b for a, b in pitched.values())
    assert sum(1 for c in LC.ORDER_CASES if c[:2] == (640, 480)) == 1


@pytest.mark.parametrize("case, axis, name", channel_cases())
def test_channel_reaches_its_property(case, axis, name):
    points, mask = LC.order_case(case)
    v = points[..., axis].reshape(-1)
    n = v.size
    assert mask.all() and np.isfinite(v).all() and not (v == 0).any()          # no +0, no -0, nothing non-finite
    count, p10, p90 = LC.sorted_stats(points, mask, I3, Z3)
    s = np.sort(v)
    r10, r90 = LC.ranks(n)
    assert count == n and 0 <= r10 <= r90 < n
    # the identity transform hands the bit patterns through
    assert p10[axis].tobytes() == s[r10].tobytes() and p90[axis].tobytes() == s[r90].tobytes()
    key = LC.order_key(s)
    assert (np.diff(key.astype(np.int64)) >= 0).all()                          # the key order is the float order here
    assert np.array_equal(LC.key_value(key).view(np.uint32), s.view(np.uint32))
    spread = n >= 10 and name != "all_equal"
    if name == "all_equal":
        assert s[0] == s[-1]
    elif name == "low_byte_only":
        assert len(np.unique(key >> 8)) == 1 and (n < 10 or len(np.unique(key & 255)) > 1)
    elif name == "sign_last_negative":
        assert (v < 0).sum() == r10 + 1 and s[r10] < 0 and (r10 + 1 == n or s[r10 + 1] > 0)
        assert key[r10] >> 31 == 0 and (r10 + 1 == n or key[r10 + 1] >> 31 == 1)
    elif name == "sign_first_positive":
        assert (v < 0).sum() == r10 and s[r10] > 0 and (r10 == 0 or s[r10 - 1] < 0)
        assert key[r10] >> 31 == 1 and (r10 == 0 or key[r10 - 1] >> 31 == 0)
    elif name == "tie_run":
        for r in (r10, r90):
            lo, hi = np.searchsorted(s, s[r], "left"), np.searchsorted(s, s[r], "right")
            assert hi - lo >= 1000 and lo < r < hi - 1                         # strictly inside the run
            assert lo >= 1 and hi <= n - 1                                     # other values on both sides,
            assert key[lo] - key[lo - 1] == 1 and key[hi] - key[hi - 1] == 1   # one key step away
    elif name in ("byte_ff", "byte_00"):
        want = 0xFFFFFF if name == "byte_ff" else 0
        for r in (r10, r90):
            assert key[r] & 0xFFFFFF == want, hex(key[r])
            for bits in (8, 16, 24):                                           # company in every later pass
                assert ((key >> bits) == (key[r] >> bits)).sum() > 1, bits
        assert (s[r10] < 0) == (name == "byte_00")                             # one case on either side of the key map
    elif name == "denormal_and_huge":
        tiny = np.abs(v) < np.finfo(f32).tiny
        for part in (tiny, np.abs(v) > 1e29, (np.abs(v) > 0.01) & (np.abs(v) < 10)):
            assert (part & (v < 0)).sum() > n // 10 and (part & (v > 0)).sum() > n // 10
    if spread:
        assert p90[axis] > p10[axis]


@pytest.mark.parametrize("n", LC.COUNTS)
def test_counts_leave_n_distinct_points(n):
    points, mask = LC.counts_case(n)
    valid = (mask != 0) & np.any(points != 0, axis=2)
    assert valid.sum() == n and (mask != 0).sum() == n + 3                     # three masked pixels hold (0, 0, 0)
    assert all(len(np.unique(points[valid][:, i])) == n for i in range(3))
    count, p10, p90 = LC.sorted_stats(points, mask, I3, Z3)
    r10, r90 = LC.ranks(n)
    assert count == n and (r10, r90) == {2: (0, 1), 9: (0, 8), 10: (1, 9), 11: (1, 9), 19: (1, 17), 20: (2, 18)}[n]
    assert np.all(p90 > p10)
    s = np.sort(points[valid], axis=0)
    assert np.array_equal(p10, s[r10]) and np.array_equal(p90, s[r90])
    # the values outside the mask would move the answer
    assert not np.array_equal(np.sort(points.reshape(-1, 3), axis=0)[LC.ranks(points.size // 3)[0]], p10)


def test_rotated_case_has_points_and_spread():
    w, h, R, t = LC.ROTATED
    points, mask = LC.cloud_image(w, h, seed=1)
    n, p10, p90 = LC.sorted_stats(points, mask, R, t)
    assert 1000 < n < (mask != 0).sum() and np.all(p90 > p10)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and not np.allclose(R, np.eye(3), atol=0.1)


@pytest.mark.parametrize("case", LC.EXTENT_CASES, ids=[c[0] for c in LC.EXTENT_CASES])
def test_extent_case_reaches_its_property(case):
    name, res, with_fg, size = case
    c = LC.extent_case(case)
    nx, ny, nz = res
    assert c["tsdf"].shape == c["weights"].shape == (nz, ny, nx) and (c["fg"] is not None) == with_fg
    cloud = LC.mesh_cloud(c["tsdf"], c["weights"], c["fg"], c["voxel"])
    valid = (c["mask"] != 0) & np.any(c["points"] != 0, axis=2)
    n, p10, p90 = LC.extent_reference(c)
    assert n == len(cloud) + valid.sum()
    if name == "no_crossing":
        assert len(cloud) == 0 and valid.sum() > 500
        return
    first, second, between = LC.interp_branches(c["tsdf"], c["weights"], c["fg"])
    assert first + second + between == len(cloud) > 0
    assert first > 0 and second > 0 and between > 0                            # vertex_interp: p1, p2, interpolated
    bits = c["tsdf"].view(np.uint32)
    assert (bits == 0).any() and (c["tsdf"] == f32(5e-6)).any() and (c["tsdf"] == f32(-5e-6)).any()
    if name == "empty_image_mask":
        assert valid.sum() == 0 and n == len(cloud) > 300
        return
    assert valid.sum() > 0
    if c["tsdf"].size > 100:
        assert len(cloud) > 300 and valid.sum() > 500
        assert (c["weights"] == 0).sum() == c["tsdf"].size // 10
        # the foreground mask takes cubes away; the cloud weighs in: the points alone give other percentiles
        assert with_fg == (len(cloud) < len(LC.mesh_cloud(c["tsdf"], c["weights"], None, c["voxel"])))
        alone = LC.sorted_stats(c["points"], c["mask"], c["R"], c["t"])
        assert not np.array_equal(alone[1], p10) and not np.array_equal(alone[2], p90)


def test_extent_resolutions():
    assert [c[1] for c in LC.EXTENT_CASES[:8:2]] == [(33, 31, 35), (30, 22, 18), (2, 2, 2), (2, 9, 3)]
    assert len(LC.mesh_cloud(*LC.extent_volume((2, 2, 2))[:2], None, 0.02)) > 3   # the one cube carries surface


# ---- association mass --------------------------------------------------------------------------------------------------

def test_mass_sizes_reach_what_they_are_listed_for():
    assert LC.MASS_SIZES == [(300, 7), (257, 241), (64, 480), (33, 481), (1, 1), (640, 480)]
    assert 300 > LC.MASS_LANES and LC.mass_bands(7) == (1, 7, 1)               # a second stride step
    assert 257 - LC.MASS_LANES == 1 and LC.mass_bands(241) == (2, 121, 1)      # one lane in it; 119 empty workgroups
    assert LC.mass_bands(480) == (2, LC.MASS_BLOCKS, 2)                        # every band full
    assert LC.mass_bands(481) == (3, 161, 1)                                   # bands of three, a last band of one row
    assert LC.mass_bands(1) == (1, 1, 1) and LC.mass_bands(120) == (1, 120, 1)  # (the old test: one row a band)


@pytest.mark.parametrize("w, h", LC.MASS_SIZES)
def test_mass_case_is_exact_and_reaches_the_edges(w, h):
    seg, match, k = LC.mass_case(w, h)
    assert seg[-1].any() and seg[:, -1].any()                                  # the last row and the last column
    assert w * h <= 1 << 20 and k.min() >= 0 and k.max() <= 4096
    wts = LC.weights_of(k)
    assert wts.dtype == f32 and np.array_equal(wts.astype(np.float64) * 4096, k)  # multiples of 2^-12, exactly
    for m in (None, match):
        n, total = LC.mass_reference(seg, m, k)
        inside = (seg != 0) if m is None else ((seg != 0) | (m != 0))
        assert n == inside.sum() > 0
        assert total == math.fsum(wts[inside].astype(np.float64).tolist())     # the integer sum is the exact sum
        # ... and any order gives it: forwards, backwards, pairwise
        assert total == np.cumsum(wts[inside].astype(np.float64))[-1] == np.sum(wts[inside][::-1].astype(np.float64))
    if w * h > 1:
        assert ((match != 0) & (seg == 0)).any()                               # the match mask adds pixels
        assert len(np.unique(k)) > 1


def test_batched_case_reaches_its_verdicts():
    b, c = LC.BATCH, LC.batched_case()
    counts, sums, verdict = LC.batched_reference(c)
    assert b["n"] == 33 > 32 and len(counts) == 33                             # a second chunk of the table
    with_match = [i for i, m in enumerate(c["matches"]) if m is not None]
    assert min(with_match) < 32 <= max(with_match) and len(with_match) < 33
    thr = f32(b["thresh"])
    tie, light = b["tie"], b["light"]
    assert np.float64(thr * f32(counts[tie])) == sums[tie]                     # a tie in float arithmetic: kept
    assert np.float64(thr * f32(counts[light])) > sums[light]
    assert np.float64(thr * f32(counts[light])) - sums[light] == 2.0 ** -12
    pos = c["list_pos"]
    assert len(set(pos.tolist())) == 33 and pos.max() < b["nall"] == 35 and len(verdict) == 36
    assert verdict[pos[tie]] == 0 and verdict[pos[light]] == 1
    for i in (b["invisible"], b["ex_low"]):                                    # heavy enough: deleted for the other reason
        assert np.float64(thr * f32(counts[i])) < sums[i] and verdict[pos[i]] == 1
    free = np.setdiff1d(np.arange(36), pos)
    assert len(free) == 3 and not verdict[free].any()                          # other ranks' positions and the padding
    assert 5 < verdict.sum() < 30                                              # both verdicts occur among the rest


# ---- overlap, carving, hiding ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w, h", LC.IMAGE_SIZES)
def test_overlap_cases(w, h):
    seg, model = LC.overlap_case(w, h, "mixed")
    n, inter, area = LC.overlap_reference(seg, model)
    assert inter[255] > 0 and inter[0] == area[0] == 0
    if w * h >= 700:
        assert set(np.unique(model)) == {0, 1, 2, 254, 255} and set(np.unique(seg)) == {0, 1, 200, 255}
        assert all(0 < inter[i] < area[i] for i in (1, 2, 254, 255))
        assert not inter[3:254].any() and not area[3:254].any()
        assert inter[1] == ((seg != 0) & (model == 1)).sum()
    seg, model = LC.overlap_case(w, h, "one_region")
    n, inter, area = LC.overlap_reference(seg, model)
    assert n == inter[255] == area[255] == w * h and inter.sum() == w * h
    seg, model = LC.overlap_case(w, h, "empty_mask")
    n, inter, area = LC.overlap_reference(seg, model)
    assert n == 0 and not inter.any() and area[255] > 0


@pytest.mark.parametrize("w, h", LC.IMAGE_SIZES)
@pytest.mark.parametrize("obj_id", [1, 255])
def test_carve_cases(w, h, obj_id):
    for with_match in (False, True):
        seg, model, match = LC.carve_case(w, h, "mixed", obj_id)
        want, pre, post = LC.carve_reference(seg, model, match if with_match else None, obj_id)
        assert pre > post and (w * h < 15 or post > 0)
        if w * h >= 15 and with_match:
            assert post < LC.carve_reference(seg, model, None, obj_id)[2]      # the match mask takes pixels of its own
        seg, model, match = LC.carve_case(w, h, "everything", obj_id)
        want, pre, post = LC.carve_reference(seg, model, match if with_match else None, obj_id)
        assert pre == w * h and post == 0 and not want.any()
        seg, model, match = LC.carve_case(w, h, "nothing", obj_id)
        want, pre, post = LC.carve_reference(seg, model, match if with_match else None, obj_id)
        assert pre == post == w * h and np.array_equal(want, seg)
        seg, model, match = LC.carve_case(w, h, "empty_mask", obj_id)
        assert LC.carve_reference(seg, model, match if with_match else None, obj_id)[1:] == (0, 0)


def test_hide_case():
    seg, vert, nrm, bgv, bgn = LC.hide_case()
    assert seg.shape == (LC.HIDE["h"], LC.HIDE["w"]) and len(set(LC.HIDE["pads"])) == 5
    hit = seg == LC.HIDE["label"]
    nan = np.isnan(nrm).any(axis=2)
    assert (hit & nan).any() and (~hit & nan).any() and np.isnan(bgn[hit]).any() and np.isnan(bgv[hit]).any()
    s, v, n = LC.hide_reference(seg, vert, nrm, bgv, bgn, LC.HIDE["label"])
    assert not (s == LC.HIDE["label"]).any() and (s == 0).sum() == (seg == 0).sum() + hit.sum()
    assert v[hit].tobytes() == bgv[hit].tobytes() and n[~hit].tobytes() == nrm[~hit].tobytes()
    assert not (seg == LC.HIDE["absent"]).any()
    s, v, n = LC.hide_reference(seg, vert, nrm, bgv, bgn, LC.HIDE["absent"])
    assert s.tobytes() == seg.tobytes() and v.tobytes() == vert.tobytes() and n.tobytes() == nrm.tobytes()
