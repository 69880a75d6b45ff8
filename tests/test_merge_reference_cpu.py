"""tests/merge_reference.py against itself (include/emf_hip.h "Merging a volume"): the vectorised statement
of the device stage and the loop agree byte for byte on the cases the GPU test runs (the loops over at most 12 x 6 x 5
voxels of each case's box), with the count identities; tsdf, weights and the record are the absorption's; the sweep
reaches every kind of count pair the rule tells apart; identity pose, equal lattices and an unobserved destination carry
the source's in-band foreground voxels over with their own pairs and nothing else; a source whose mask is all zero changes
nothing; the dtype of the count record is the library mirror's.  The host steps of a session's merge: the union of the two
bands in numpy, in Python floats and through emf_fusion_merge_union, byte for byte; the resize arithmetic and the shift;
pipeline.merged_line round-trips a hand-made event.  The host steps of the automatic merge, in numpy and in plain Python:
the overlap quotient, the pair ordering (an object once per frame, ties by id) and the bookkeeping sums."""
import numpy as np
import pytest

from tests import absorb_reference as ar
from tests import merge_reference as mr
from tests import shape_reference as sr

f32 = np.float32


def loop_box(box, limit=(12, 6, 5)):
    lo, size = box
    return lo, tuple(min(s, m) for s, m in zip(size, limit))


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("content", sr.CONTENTS)
@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_two_statements_agree_and_the_band_is_the_absorptions(shape, content):
    for name, dst, src, pose, box in mr.cases(shape, content):
        box = loop_box(box)
        a, b = mr.merge(dst, src, pose, box), mr.merge_loop(dst, src, pose, box)
        assert same(a, b), (name, a[2], b[2], a[4], b[4])
        mr.check_identities(a[2], a[4])
        assert same(a[:3], ar.absorb(dst, src, pose, box)), name
        lo, size = box
        keep = np.ones(dst["tsdf"].shape, bool)
        keep[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = False
        assert a[3][keep].tobytes() == dst["fgbg"][keep].tobytes(), name
        assert int((a[3].view(np.uint32) != dst["fgbg"].view(np.uint32)).any(axis=3).sum()) <= a[2]["fused"], name


def test_the_planted_wall():
    dst, src, poses = mr.planted_case()
    box = ((6, 2, 1), (18, 9, 6))
    for pose in poses:
        assert same(mr.merge(dst, src, pose, box), mr.merge_loop(dst, src, pose, box))
        full = mr.merge(dst, src, pose)
        mr.check_identities(full[2], full[4])
        assert full[2]["fused"] > full[4]["foreground"] > 0 and full[2]["masked"] > 0


def test_the_sweep_reaches_every_kind_of_pair():
    """Over all cases the GPU test runs (tests/test_gpu_merge.py: the same generator, whole boxes as they come) the
    restatement meets each kind of pair the rule tells apart; otherwise that test proves less than it claims."""
    kinds = {}
    for shape in ar.SHAPES:
        for content in sr.CONTENTS:
            for _, dst, src, pose, box in mr.cases(shape, content):
                mr.merge(dst, src, pose, box, kinds=kinds)
    for name in mr.KINDS:
        assert kinds.get(name, 0) > 0, (name, kinds)


def test_the_count_volumes_hold_the_pairs_they_promise():
    c = mr.count_volume((33, 17, 9), 1)
    fg, bg = c[..., 0], c[..., 1]
    assert (c == np.rint(c)).all() and (c >= 0).all()
    for found in ((fg == 0) & (bg == 0), (fg == bg) & (fg > 0), fg == bg + 1, bg == fg + 1, fg == mr.BIG):
        assert found.sum() > 50
    assert f32(mr.BIG) + f32(1) == f32(mr.BIG) and f32(mr.BIG) + f32(3) == f32(mr.BIG + 4)  # such a sum rounds


def test_identity_carries_the_foreground_band_over_with_its_own_pairs():
    """Identity pose, equal lattices, equal truncation, an unobserved destination: the source's in-band voxels that its
    mask calls foreground arrive with their own tsdf and their own pairs, and nothing else changes."""
    shape = (33, 17, 9)
    st, sw, sf = sr.volume(shape, "half_shell")
    dt, dw, _ = sr.volume(shape, "unobserved")
    dst = dict(ar.dst_vol(dt, dw, 0.01, 0.04, 64.0), fgbg=mr.count_volume(shape, 1))
    src = dict(ar.src_vol(st, sw, sf, 0.01, 0.04), fgbg=mr.count_volume(shape, 2))
    tsdf, weights, rec, fgbg, cnt = mr.merge(dst, src, ar.pose_of())
    changed = weights.view(np.uint32) != dw.view(np.uint32)
    assert rec["fused"] == rec["fresh"] == changed.sum() > 50
    assert (sf[changed] != 0).all() and (np.abs(st[changed]) < 1).all()
    assert tsdf[changed].tobytes() == st[changed].tobytes()
    assert fgbg[changed].tobytes() == src["fgbg"][changed].tobytes()
    assert fgbg[~changed].tobytes() == dst["fgbg"][~changed].tobytes() and tsdf[~changed].tobytes() == dt[~changed].tobytes()
    want = int((src["fgbg"][changed][:, 0] > src["fgbg"][changed][:, 1]).sum())
    assert cnt["foreground"] == cnt["gained"] == want > 0


def test_a_source_whose_mask_is_all_zero_changes_nothing():
    shape = (33, 17, 9)
    st, sw, sf = sr.volume(shape, "all_solid")
    dt, dw, _ = sr.volume(shape, "random")
    dst = dict(ar.dst_vol(dt, dw, 0.01, 0.04, 64.0), fgbg=mr.count_volume(shape, 1))
    src = dict(ar.src_vol(st, sw, np.zeros_like(sf), 0.01, 0.04), fgbg=mr.count_volume(shape, 2))
    for pose in (ar.pose_of(), ar.pose_of(None, (0.0031, 0.0047, 0.0013))):
        tsdf, weights, rec, fgbg, cnt = mr.merge(dst, src, pose)
        assert rec["fused"] == 0 and rec["masked"] > 1000 and cnt.tobytes() == mr.counts().tobytes()
        assert tsdf.tobytes() == dst["tsdf"].tobytes() and weights.tobytes() == dst["weights"].tobytes()
        assert fgbg.tobytes() == dst["fgbg"].tobytes()
        assert same(mr.merge(dst, src, pose, ((6, 2, 1), (12, 6, 5))), mr.merge_loop(dst, src, pose, ((6, 2, 1), (12, 6, 5))))


def test_the_colour_of_a_merge_is_the_absorptions():
    from tests import transfer_color_reference as tc
    for name, dst, src, pose, box in mr.color_cases((33, 17, 9), "half_shell"):
        got = mr.merge_color(dst, src, pose, box)
        assert same(got[:5], mr.merge(dst, src, pose, box)), name
        tc.check_identities(got[2], got[6], "fused")


def test_the_record_is_the_library_mirrors():
    from emfusion_amd import _lib
    assert np.dtype(_lib.MERGE_COUNTS_DTYPE) == mr.MERGE_COUNTS


def test_the_union_of_the_bands_three_ways():
    """union_np, union_py and emf_fusion_merge_union agree byte for byte: rotated and shifted poses, unequal lattices, an
    object without a solid voxel on either side, neither."""
    from emfusion_amd import pipeline
    from tests.contacts_reference import rot_z
    rng = np.random.default_rng(11)
    none = ((33, 17, 9), (-1, -1, -1))
    for k in range(40):
        d_res, s_res = rng.integers(2, 200, 3), rng.integers(2, 200, 3)
        d = none if k % 7 == 3 else tuple(np.sort(np.stack([rng.integers(0, d_res), rng.integers(0, d_res)]), axis=0))
        s = none if k % 5 == 2 else tuple(np.sort(np.stack([rng.integers(0, s_res), rng.integers(0, s_res)]), axis=0))
        R = np.eye(3, dtype=f32) if k % 3 == 0 else np.asarray(rot_z(float(rng.uniform(-180, 180))), f32).reshape(3, 3)
        t = rng.uniform(-1, 1, 3).astype(f32)
        args = (d, d_res, 0.01 * (1 + k % 3), s, s_res, 0.0125, R, t)
        a, b, c = mr.union_np(*args), mr.union_py(*args), pipeline.merge_union(*args[:6], (R, t))
        if k % 7 == 3 and k % 5 == 2:
            assert a is None and b is None and c is None
            continue
        for got in (b, c):
            assert a[0].tobytes() == got[0].tobytes() and a[1].tobytes() == got[1].tobytes(), (k, a, got)
        assert (a[0] <= a[1]).all()
    assert mr.union_np(none, (8, 8, 8), 0.01, none, (8, 8, 8), 0.01, np.eye(3), np.zeros(3)) is None
    assert pipeline.merge_union(none, (8, 8, 8), 0.01, none, (8, 8, 8), 0.01, (np.eye(3), np.zeros(3))) is None
    # identity, equal lattices: the union of the bounds themselves
    lo, hi = mr.union_np(((2, 3, 4), (5, 6, 7)), (9, 9, 9), 0.25, ((0, 1, 2), (8, 3, 5)), (9, 9, 9), 0.25, np.eye(3), np.zeros(3))
    assert lo.tolist() == [-1.0, -0.75, -0.5] and hi.tolist() == [1.0, 0.5, 0.75]


def test_the_growth_and_the_shift():
    assert mr.grow((32, 32, 32), 0.01, (-0.1, -0.1, -0.1), (0.1, 0.1, 0.1)) is None      # contained: 15.5 voxels either way
    n, offset, centre = mr.grow((32, 32, 32), 0.01, (-0.1, -0.1, -0.1), (0.3, 0.1, 0.1))
    assert n == 80 and offset == (10 - 24, -24, -24) and centre.tolist() == [f32(10) * f32(0.01), 0.0, 0.0]
    assert mr.grow((32, 32, 32), 0.01, (-0.1, -0.1, -0.1), (0.3, 0.1, 0.1), max_res=64) is None  # beyond the cap: not grown
    v = np.arange(2 * 3 * 4, dtype=f32).reshape(2, 3, 4)
    s = mr.shifted(v, 6, (-1, -2, -3))
    assert s[3:5, 2:5, 1:5].tobytes() == v.tobytes() and s.sum() == v.sum()
    assert mr.shifted(v, 2, (2, 1, 0)).tolist() == [[[6, 7], [10, 11]], [[18, 19], [22, 23]]]
    pairs = np.array([[[[0, 0], [1, 1], [2, 1], [1, 2], [3, 0]]]], f32)
    assert mr.fg_mask_of(pairs).tolist() == [[[0, 0, 255, 0, 255]]]


def test_the_line_round_trips_an_event():
    from emfusion_amd import pipeline
    e = np.zeros((), pipeline._merge_event_dtype())
    e["dst"], e["src"], e["frame"], e["clipped"], e["automatic"], e["res_before"], e["res_after"] = 3, 7, 12, 1, 0, 32, 80
    e["lo"], e["size"] = (1, 2, 3), (40, 41, 42)
    for k, name in enumerate(ar.COUNTS):
        e["record"][name] = 2 ** 33 + k
    e["record"]["lo"], e["record"]["hi"] = (4, 5, 6), (7, 8, 9)
    e["counts"]["foreground"], e["counts"]["gained"] = 500, 17
    e["color"]["colored"], e["color"]["uncolored"] = 2 ** 40 + 1, 5
    e["overlap"] = (0.625, 1 / 3)
    for k, name in enumerate(("dst_R", "src_R", "R")):
        e[name] = np.arange(9, dtype=f32) / (7 + k)
    e["dst_t"], e["src_t"], e["t"] = (0.1, -1e-9, 3.0000002), (1, 2, 3), (-0.5, 0.25, 1e20)
    event = pipeline.Fusion._merge_event(e)
    row = pipeline.merged_line(event).split()
    assert len(row) == 13 + 8 + 6 + 4 + 2 + 36
    assert [int(v) for v in row[:13]] == [3, 7, 12, 1, 0, 32, 80, 1, 2, 3, 40, 41, 42]
    assert [int(v) for v in row[13:21]] == [2 ** 33 + k for k in range(8)] and [int(v) for v in row[21:27]] == [4, 5, 6, 7, 8, 9]
    assert [int(v) for v in row[27:31]] == [500, 17, 2 ** 40 + 1, 5]
    assert [float(v) for v in row[31:33]] == [0.625, float("%.9g" % (1 / 3))]
    poses = np.array([np.float32(v) for v in row[33:]], f32)  # %.9g carries a float32 exactly
    assert poses.tobytes() == b"".join(np.asarray(event[k], f32).tobytes() for k in ("dst_R", "dst_t", "src_R", "src_t", "R", "t"))


def test_the_pair_ordering_takes_an_object_once_and_breaks_ties_by_id():
    """Five objects.  2-3 is the best pair (0.9) and goes first, which takes 2 and 3 out of 1-2 and 3-4; 4-5 follows.
    Without 2-3, 1-2 and 3-4 tie at 0.75 and the smaller pair of ids goes first.  A pair below the threshold, a pair
    with a small surface and a pair probed one way only never qualify."""
    rec = {(1, 2): (100, 75), (2, 1): (100, 10), (3, 4): (200, 20), (4, 3): (100, 75), (2, 3): (100, 90), (3, 2): (100, 0),
           (4, 5): (100, 60), (5, 4): (100, 55), (1, 5): (100, 49), (5, 1): (100, 49), (1, 3): (63, 63), (3, 1): (100, 100),
           (1, 4): (100, 100)}
    for statement in (mr.merge_pairs_np, mr.merge_pairs_py):
        assert statement(rec) == [(2, 3, 0.9, 0.0), (4, 5, 0.6, 0.55)]
        assert statement(rec, min_surface=63) == [(1, 3, 1.0, 1.0), (4, 5, 0.6, 0.55)]
        without = {k: v for k, v in rec.items() if k not in ((2, 3), (3, 2))}
        assert statement(without) == [(1, 2, 0.75, 0.1), (3, 4, 0.1, 0.75)]  # the tie: the smaller pair of ids first
        assert statement(without, min_overlap=0.8) == [] and statement({}) == []
        assert statement({(1, 2): (0, 0), (2, 1): (0, 0)}, min_overlap=0.0, min_surface=0) == [(1, 2, 0.0, 0.0)]
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(2, 7))
        rec = {(a, b): (int(rng.integers(0, 200)), 0) for a in range(1, n + 1) for b in range(1, n + 1) if a != b}
        rec = {k: (s, int(rng.integers(0, s + 1))) for k, (s, _) in rec.items()}
        a, b = mr.merge_pairs_np(rec, 0.3, 20), mr.merge_pairs_py(rec, 0.3, 20)
        assert a == b
        ids = [i for p in a for i in p[:2]]
        assert len(ids) == len(set(ids)) and all(p[0] < p[1] for p in a)
        assert [max(p[2:]) for p in a] == sorted([max(p[2:]) for p in a], reverse=True)
    assert mr.overlap_np([3, 0], [1, 0]).tolist() == [mr.overlap_py(3, 1), 0.0] == [1 / 3, 0.0]


def test_the_bookkeeping_sums():
    a, b = (3, 1, [0.5, 0.25, 0.0]), (2, 4, [0.125, 0.5])
    for statement in (mr.bookkeeping_np, mr.bookkeeping_py):
        ex, non, scores = statement(a, b)
        assert (ex, non, list(scores)) == (5, 5, [0.625, 0.75, 0.0])
        assert list(statement((1, 0, []), b)[2]) == [0.125, 0.5] and list(statement(a, (0, 0, []))[2]) == [0.5, 0.25, 0.0]
