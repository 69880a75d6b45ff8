"""The frontier restatement (tests/frontier_reference.py) on hand-made volumes with known answers, and the argument
checks of emf_hip_frontierLabel / emf_hip_frontierClusters, which reject before any launch and so need no device
(include/emf_hip.h "Frontiers")."""
import ctypes as C

import numpy as np

from emfusion_amd import _lib
from tests import frontier_reference as fr

E_ARG, E_LIMIT = -4, -5
P = C.c_void_p(4096)  # a non-NULL, aligned pointer that is never dereferenced
FREE, OCC, UNK = fr.FREE, fr.OCCUPIED, fr.UNKNOWN


def i3(*v):
    return (C.c_int32 * 3)(*v)


def members(labels, record):
    return {tuple(int(v) for v in p[::-1]) for p in np.argwhere(labels == record["label"])}  # (x, y, z)


def test_a_free_cube_in_unknown_has_its_shell_as_one_cluster():
    for k in (1, 2, 3, 5):
        c = np.full((k + 4, k + 3, k + 2), UNK, np.uint8)
        c[2:2 + k, 1:1 + k, 1:1 + k] = FREE
        labels, kept, counts = fr.frontiers(c)
        shell = k ** 3 - max(k - 2, 0) ** 3
        assert counts == (1, 1, shell) and len(kept) == 1
        r = kept[0]
        assert r["count"] == shell and r["label"] == (2 * (k + 3) + 1) * (k + 2) + 1
        assert r["lo"].tolist() == [1, 1, 2] and r["hi"].tolist() == [k, k, k + 1]
        assert tuple(int(v) for v in r["rep"]) in members(labels, r)
        assert (labels >= 0).sum() == shell and set(np.unique(labels)) == {-1, int(r["label"])}
        if k >= 3:
            assert labels[3, 2, 2] == -1  # the inside is free but no frontier


def test_two_rooms_behind_a_wall_are_two_clusters():
    c = np.full((5, 5, 11), UNK, np.uint8)
    c[1:4, 1:4, 1:4] = FREE
    c[1:4, 1:4, 7:10] = FREE
    c[:, :, 4:7] = OCC
    labels, kept, counts = fr.frontiers(c)
    assert counts[:2] == (2, 2) and kept["count"].tolist() == [25, 25]  # the 26 shell voxels less the one whose only
    # neighbour that is not free is the wall
    assert kept["label"].tolist() == [(1 * 5 + 1) * 11 + 1, (1 * 5 + 1) * 11 + 7]
    assert fr.session_order(kept)["label"].tolist() == kept["label"].tolist()  # ties: the smaller label first


def test_corner_contact_joins_and_a_gap_of_one_does_not():
    c = np.full((5, 5, 7), UNK, np.uint8)
    c[1, 1, 1] = c[2, 2, 2] = FREE  # touch by a corner only
    labels, kept, counts = fr.frontiers(c)
    assert counts == (1, 1, 2) and kept[0]["count"] == 2 and labels[2, 2, 2] == labels[1, 1, 1] == (1 * 5 + 1) * 7 + 1
    c[2, 2, 2] = UNK
    c[1, 1, 3] = FREE  # two apart
    labels, kept, counts = fr.frontiers(c)
    assert counts == (2, 2, 2) and labels[1, 1, 3] != labels[1, 1, 1]


def test_what_is_no_frontier():
    c = np.full((3, 3, 3), OCC, np.uint8)
    c[1, 1, 1] = FREE  # free next to occupied only
    assert fr.frontiers(c)[2] == (0, 0, 0)
    c = np.full((3, 3, 3), FREE, np.uint8)  # unknown beyond the box face does not count
    assert fr.frontiers(c)[2] == (0, 0, 0)
    c[1, 1, 2] = 3  # class byte 3 is neither free nor unknown
    assert fr.frontiers(c)[2] == (0, 0, 0)
    c = np.full((1, 1, 3), 3, np.uint8)
    c[0, 0, 1] = UNK
    assert fr.frontiers(c)[2] == (0, 0, 0)  # 3 next to unknown is not free
    c[0, 0, 0] = FREE
    assert fr.frontiers(c)[2] == (1, 1, 1)


def test_the_clearance_gate_keeps_d2_equal_to_min_d2():
    c = np.full((1, 1, 5), UNK, np.uint8)
    c[0, 0, [1, 3]] = FREE
    d2 = np.array([[[0, 4, 0, 3, 0]]], np.int32)
    labels = fr.frontiers(c, d2, 4)[0]
    assert labels.reshape(-1).tolist() == [-1, 1, -1, -1, -1]  # 4 stays, 3 = min_d2 - 1 goes
    d2[0, 0, 3] = fr.FAR
    assert fr.frontiers(c, d2, 4)[0].reshape(-1).tolist() == [-1, 1, -1, 3, -1]  # "far" passes
    assert fr.frontiers(c, d2, 0)[2] == fr.frontiers(c)[2] == (2, 2, 2)  # min_d2 <= 0: no gate


def test_min_voxels_keeps_count_equal_to_min_voxels():
    c = np.full((1, 3, 12), UNK, np.uint8)
    c[0, 1, 0:3] = FREE
    c[0, 1, 5:7] = FREE
    c[0, 1, 9] = FREE
    for min_voxels, want in ((1, [3, 2, 1]), (2, [3, 2]), (3, [3]), (4, [])):
        labels, kept, counts = fr.frontiers(c, min_voxels=min_voxels)
        assert kept["count"].tolist() == want and counts == (len(want), 3, 6)


def test_a_tie_of_the_representative_goes_to_the_smaller_index():
    c = np.full((1, 3, 4), UNK, np.uint8)
    c[0, 1, 1:3] = FREE  # x = 1, 2: sum 3, centre (2 * 3 + 2) // 4 = 2: no tie, x = 2
    assert fr.frontiers(c)[1][0]["rep"].tolist() == [2, 1, 0]
    c = np.full((3, 3, 3), UNK, np.uint8)
    c[1, 0, 1] = c[1, 2, 1] = c[0, 1, 1] = c[2, 1, 1] = FREE  # a ring around (1, 1, 1): all four at distance 1
    labels, kept, counts = fr.frontiers(c)
    assert counts == (1, 1, 4) and kept[0]["sum"].tolist() == [4, 4, 4]
    assert kept[0]["rep"].tolist() == [1, 1, 0] and kept[0]["label"] == 4  # the smallest linear index of the four


def test_world_points_by_hand():
    r = np.zeros(1, fr.RECORD)
    r["count"], r["sum"], r["rep"] = 2, [[3, 4, 5]], [[1, 2, 3]]
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    centroid, rep = fr.world_points(r, (10, 0, 0), (64, 64, 64), 0.5, R, (1, 2, 3))
    # rep: (1 + 10 - 31.5, 2 - 31.5, 3 - 31.5) * 0.5 = (-10.25, -14.75, -14.25), rotated (x, y) -> (-y, x), shifted
    assert rep.dtype == np.float32 and rep.tolist() == [[14.75 + 1, -10.25 + 2, -14.25 + 3]]
    assert centroid.tolist() == [[14.75 + 1, -10.0 + 2, -14.5 + 3]]


def test_null_and_shape_arguments_are_rejected_before_any_launch():
    lib = _lib.load()
    size = i3(16, 16, 16)
    f = lib.emf_hip_frontierLabel
    assert f(None, size, None, 0, P, P, None) == E_ARG
    assert f(P, None, None, 0, P, P, None) == E_ARG
    assert f(P, size, None, 0, None, P, None) == E_ARG
    assert f(P, size, None, 0, P, None, None) == E_ARG
    assert f(P, i3(16, 0, 16), None, 0, P, P, None) == E_ARG
    assert f(P, i3(16, 16, -3), None, 0, P, P, None) == E_ARG
    assert f(P, i3(2049, 1, 1), None, 0, P, P, None) == E_LIMIT
    assert f(P, i3(1, 1, 2049), None, 0, P, P, None) == E_LIMIT
    assert f(P, i3(2048, 2048, 512), None, 0, P, P, None) == E_LIMIT
    assert b"2^31 - 1" in lib.emf_hip_last_error_string()
    g = lib.emf_hip_frontierClusters
    assert g(None, size, 1, 4, P, P, 4, P, None) == E_ARG
    assert g(P, None, 1, 4, P, P, 4, P, None) == E_ARG
    assert g(P, size, 1, 4, None, P, 4, P, None) == E_ARG  # clusters without scratch
    assert g(P, size, 1, 4, P, None, 4, P, None) == E_ARG  # capacity without records
    assert g(P, size, 1, 4, P, P, 4, None, None) == E_ARG
    assert g(P, i3(0, 16, 16), 1, 4, P, P, 4, P, None) == E_ARG
    assert g(P, i3(16, -1, 16), 1, 4, P, P, 4, P, None) == E_ARG
    assert g(P, i3(16, 2049, 16), 1, 4, P, P, 4, P, None) == E_LIMIT
    assert g(P, i3(2048, 2048, 512), 1, 4, P, P, 4, P, None) == E_LIMIT
    assert g(P, size, 0, 4, P, P, 4, P, None) == E_ARG
    assert b"min_voxels" in lib.emf_hip_last_error_string()
    assert g(P, size, -2, 4, P, P, 4, P, None) == E_ARG
    assert g(P, size, 1, 4, P, P, -1, P, None) == E_ARG
    assert b"capacity" in lib.emf_hip_last_error_string()
    assert g(P, size, 1, 16 ** 3 + 1, P, P, 4, P, None) == E_ARG  # more clusters than voxels


def test_scratch_size_and_declared_symbols():
    lib = _lib.load()
    names = _lib.declared_symbols()
    for name in ("emf_hip_frontierLabel", "emf_hip_frontierScratchBytes", "emf_hip_frontierClusters"):
        assert name in names and name in _lib.SIGNATURES
    assert C.sizeof(_lib.EmfFrontierCluster) == 72 == np.dtype(_lib.FRONTIER_CLUSTER_DTYPE).itemsize == fr.RECORD.itemsize
    for field, (offset, _) in ((n, (getattr(_lib.EmfFrontierCluster, n).offset, 0)) for n, *_ in _lib.FRONTIER_CLUSTER_DTYPE):
        assert np.dtype(_lib.FRONTIER_CLUSTER_DTYPE).fields[field][1] == offset == fr.RECORD.fields[field][1]
    s = lib.emf_hip_frontierScratchBytes
    assert s(i3(0, 4, 4), 1) == 0 and s(i3(4, 4, 2049), 1) == 0 and s(None, 1) == 0 and s(i3(2048, 2048, 512), 1) == 0
    n, nc = 512 ** 3, 100000
    assert 0 < s(i3(512, 512, 512), nc) <= 4 * (n // 256) + 65 * nc + 1024  # the bound the header states
    assert s(i3(512, 512, 512), 0) <= 4 * (n // 256) + 1024
    assert s(i3(4, 4, 4), 3) < s(i3(4, 4, 4), 300)
