"""The restatement of the motion masks (tests/motion_reference.py) on hand-made images: what the GPU tests compare the
kernels with has to be right by itself."""
import numpy as np

from tests import motion_reference as mr


def run(cand, m=None, **params):
    p, b = mr.scene(cand, m)
    return mr.motion_masks(p, b, **params)


def test_one_pixel_bridge_is_cut_by_one_erosion():
    c = mr.two_blobs_with_bridge(48, 64)
    joined = run(c, erode=0, min_pixels=1)
    assert joined["count"] == 1
    cut = run(c, erode=1, min_pixels=1)
    assert cut["count"] == 2
    a, b = mr.proposals(cut)
    assert a["x1"] < 32 <= b["x0"] or b["x1"] < 32 <= a["x0"]  # one on each side of the gap


def test_overlapping_blobs_at_different_ray_lengths_get_two_labels():
    c, m = mr.overlapping_blobs(48, 64)
    r = run(c, m, erode=0, min_pixels=1, continuity=0.05)
    assert r["count"] == 2
    left, right = sorted(mr.proposals(r), key=lambda q: q["x0"])
    assert left["x1"] == 31 and right["x0"] == 32
    assert run(c, m, erode=0, min_pixels=1, continuity=0.25)["count"] == 1  # 0.25 apart joins at 0.25: <=


def test_blob_below_min_pixels_is_dropped():
    c = mr.big_and_small(48, 64)  # the small blob has 2 x 3 = 6 pixels
    assert run(c, erode=0, min_pixels=6)["count"] == 2
    r = run(c, erode=0, min_pixels=7)
    assert r["count"] == 1 and r["info"][0][1] == 48 * 42
    assert not r["masks"][0][45:47, 60:63].any() and (r["labels"][45:47, 60:63] == -1).all()


def test_area_ties_go_to_the_smaller_label_and_truncate_in_order():
    c = mr.blob_grid(48, 64)  # 6 x 8 blobs of 25 pixels
    n_blobs = 6 * 8
    full = run(c, erode=0, min_pixels=1, max_masks=16)
    assert full["count"] == 16 < n_blobs
    labels = [q["label"] for q in mr.proposals(full)]
    assert labels == sorted(labels) and labels[0] == 1 * 64 + 1
    assert all(q["area"] == 25 for q in mr.proposals(full))
    # the first k of the same order, whatever k is
    for k in (1, 3, 8):
        r = run(c, erode=0, min_pixels=1, max_masks=k)
        assert r["count"] == k and [q["label"] for q in mr.proposals(r)] == labels[:k]
        assert r["masks"].shape == (k, 48, 64) and (r["labels"] < k).all()
    # a larger blob comes first although its label is the largest
    c[40:47, 50:60] = True
    r = run(c, erode=0, min_pixels=1, max_masks=4)
    first = mr.proposals(r)[0]
    assert first["area"] > 25 and first["label"] > mr.proposals(r)[1]["label"]


def test_all_miss_background_gives_no_proposals():
    p, _ = mr.scene(np.ones((48, 64), bool))
    r = mr.motion_masks(p, np.zeros((48, 64), np.float32), erode=0, min_pixels=1)
    assert r["count"] == 0 and (r["labels"] == -1).all() and not r["masks"].any() and not r["info"].any()


def test_labels_are_minimum_linear_indices():
    for name, p, b, params in mr.cases(45, 67):
        r = mr.motion_masks(p, b, erode=0, **params)
        comp = r["components"]
        for root in np.unique(comp[comp >= 0]):
            assert np.nonzero(comp.reshape(-1) == root)[0][0] == root, name
        for q in mr.proposals(r):
            inside = r["labels"] == r["labels"].reshape(-1)[q["label"]]
            ys, xs = np.nonzero(inside)
            assert q["label"] == (ys * 67 + xs).min() and q["area"] == inside.sum(), name
            assert (q["x0"], q["y0"], q["x1"], q["y1"]) == (xs.min(), ys.min(), xs.max(), ys.max()), name


def test_labels_agree_with_scipy_label_where_continuity_does_not_cut():
    from scipy import ndimage
    for name in ("bridge", "serpentine", "checkerboard"):
        (_, p, b, params), = [c for c in mr.cases(45, 67) if c[0] == name]
        comp = mr.motion_masks(p, b, erode=0, **params)["components"]
        ref, n = ndimage.label(comp >= 0)  # 4-connectivity
        assert len(np.unique(comp[comp >= 0])) == n, name
        for k in range(1, n + 1):
            assert len(np.unique(comp[ref == k])) == 1, name


def test_serpentine_is_one_component_and_checkerboard_all_singletons():
    r = run(mr.serpentine(45, 67), erode=0, min_pixels=1)
    assert r["count"] == 1 and r["info"][0][0] == 0 and r["info"][0][1] == mr.serpentine(45, 67).sum()
    r = run(mr.checkerboard(45, 67), erode=0, min_pixels=1, max_masks=16)
    assert r["count"] == 16 and [q["label"] for q in mr.proposals(r)] == list(range(0, 32, 2))
    assert all(q["area"] == 1 for q in mr.proposals(r))


def test_non_finite_inputs_are_never_candidates():
    p, b = mr.scene(np.ones((8, 8), bool))
    p[1, 1, 0] = np.nan
    p[2, 2, 2] = np.inf
    b[3, 3] = np.nan
    p[4, 4, 2] = -1.0
    r = mr.motion_masks(p, b, erode=0, min_pixels=1)
    assert r["count"] == 1
    for y, x in ((1, 1), (2, 2), (3, 3), (4, 4)):
        assert r["labels"][y, x] == -1
    assert (r["labels"] == 0).sum() == 60
