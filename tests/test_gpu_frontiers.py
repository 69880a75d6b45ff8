"""The frontier kernels (include/emf_hip.h "Frontiers"; ops.frontier_labels, ops.frontier_clusters)
against tests/frontier_reference.py.  Every comparison is tobytes() equality: the frontier set, the labels, the
statistics and the representative are integer functions of the class bytes.  The shapes are the smallest at which the
kernels can go wrong -- rows of 1, 63, 64, 65 voxels, more than two chunks, the longest row, an axis of 1, more rows
than a workgroup holds -- not the workload's."""
import ctypes as C

import numpy as np
import pytest

from tests import frontier_reference as fr
from tests.parity_util import to_dev

pytestmark = pytest.mark.gpu

MIN_D2 = (0, 1, 4)
MIN_VOXELS = (1, 2, 9)
_expected = {}


def expected(shape, content):
    """(classes, d2, {min_d2: (labels, every record in label order, frontier voxels)}), computed once and shared."""
    key = (shape, content)
    if key not in _expected:
        classes, d2 = fr.class_field(shape, content), fr.d2_field(shape)
        by_gate = {}
        for min_d2 in MIN_D2:
            labels = fr.labels_of(fr.flags_of(classes, d2, min_d2))
            every = fr.records_of(labels)
            for a in (labels, every):
                a.setflags(write=False)
            by_gate[min_d2] = (labels, every, int((labels >= 0).sum()))
        classes.setflags(write=False)
        d2.setflags(write=False)
        _expected[key] = (classes, d2, by_gate)
    return _expected[key]


def poisoned(n):
    from emfusion_amd.devmem import DeviceArray
    return DeviceArray.from_numpy(np.frombuffer(b"\xee" * (72 * n), fr.RECORD))


@pytest.mark.parametrize("content", fr.CONTENTS)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_labels_and_records_are_exact(dev, shape, content):
    from emfusion_amd import ops
    classes, d2, by_gate = expected(shape, content)
    d_classes, d_d2 = to_dev(classes), to_dev(d2)
    for min_d2 in MIN_D2:
        want_labels, every, voxels = by_gate[min_d2]
        labels = ops.frontier_labels(d_classes, d2=d_d2, min_d2=min_d2)
        got_labels = labels.numpy()
        assert got_labels.dtype == np.int32 and got_labels.shape == shape
        assert got_labels.tobytes() == want_labels.tobytes(), \
            (shape, content, min_d2, int((got_labels != want_labels).sum()), np.argwhere(got_labels != want_labels)[:4].tolist())
        assert labels.counters.numpy().tolist() == [0, len(every), voxels]
        for min_voxels in MIN_VOXELS:
            want = fr.keep(every, min_voxels)
            sink = poisoned(len(every))  # as many as there are clusters: what is not kept stays as it was
            _, counts = ops.frontier_clusters(labels, min_voxels=min_voxels, capacity=len(every), records=sink)
            got = sink.numpy()
            assert counts == (len(want), len(every), voxels), (shape, content, min_d2, min_voxels)
            assert got[:len(want)].tobytes() == want.tobytes(), (shape, content, min_d2, min_voxels)
            assert got[len(want):].tobytes() == b"\xee" * (72 * (len(every) - len(want)))
            for r in got[:len(want)]:  # the representative is a member of its cluster
                assert got_labels[r["rep"][2], r["rep"][1], r["rep"][0]] == r["label"]
        for capacity in sorted({0, 1, max(len(every) - 1, 0)}):
            sink = poisoned(capacity + 1)
            _, counts = ops.frontier_clusters(labels, min_voxels=1, capacity=capacity, records=_prefix(sink, capacity))
            got = sink.numpy()
            written = min(capacity, len(every))
            assert counts == (len(every), len(every), voxels)  # the counters are full whatever the capacity
            assert got[:written].tobytes() == every[:written].tobytes() and got[written:].tobytes() == b"\xee" * (72 * (capacity + 1 - written))
        # a second run into the same buffers gives the same bytes
        again = ops.frontier_labels(d_classes, d2=d_d2, min_d2=min_d2, out=labels)
        assert again is labels and labels.numpy().tobytes() == want_labels.tobytes()
        records, counts = ops.frontier_clusters(labels, min_voxels=1)
        assert records.tobytes() == every.tobytes() and counts == (len(every), len(every), voxels)
    # no gate: d2 NULL is min_d2 == 0
    assert ops.frontier_labels(d_classes).numpy().tobytes() == by_gate[0][0].tobytes()
    assert d_classes.numpy().tobytes() == classes.tobytes() and d_d2.numpy().tobytes() == d2.tobytes()  # only read


def _prefix(sink, n):
    """The first n records of a device array, as a device array of its own shape."""
    from emfusion_amd.devmem import DeviceView
    return DeviceView(sink.ptr, (n,), fr.RECORD)


def test_the_contents_are_what_they_claim(dev):
    shape = (9, 17, 65)
    for content, clusters in (("checker", 1), ("serpentine", 1), ("halves", 1), ("all_free", 0), ("all_unknown", 0)):
        assert len(expected(shape, content)[2][0][1]) == clusters, content
    lattice = expected(shape, "lattice")[2][0][1]
    assert len(lattice) == 3 * 6 * 22 and (lattice["count"] == 1).all()  # as many clusters as the box can hold
    assert expected(shape, "serpentine")[2][0][2] > 9 * 17 * 65 // 5  # a walk through the whole box
    ends = expected((4, 5, 65), "row_ends")[2][0]
    assert ends[2] == 20 and len(ends[1]) == 2  # neighbours in linear index are no neighbours in space


def test_a_wrong_cluster_count_stays_inside_the_tables(dev):
    """n_clusters is the host's copy of a device counter.  A smaller value drops the clusters of the largest labels, a
    larger one changes nothing (include/emf_hip.h emf_hip_frontierClusters)."""
    from emfusion_amd import _lib, ops
    from emfusion_amd.devmem import DeviceArray
    shape = (4, 5, 65)
    every = expected(shape, "lattice")[2][0][1]
    labels = ops.frontier_labels(to_dev(expected(shape, "lattice")[0]))
    lib, size = _lib.load(), (C.c_int32 * 3)(*shape[::-1])
    for n_clusters, want in ((len(every) - 3, every[:-3]), (len(every) + 5, every)):
        scratch = DeviceArray((lib.emf_hip_frontierScratchBytes(size, n_clusters),), np.uint8)
        sink = poisoned(len(every) + 5)
        _lib.check("emf_hip_frontierClusters",
                   lib.emf_hip_frontierClusters(C.c_void_p(labels.ptr), size, 1, n_clusters, C.c_void_p(scratch.ptr),
                                                C.c_void_p(sink.ptr), len(every) + 5, C.c_void_p(labels.counters.ptr), None))
        got = sink.numpy()
        assert labels.counters.numpy().tolist() == [len(want), len(every), len(every)]
        assert got[:len(want)].tobytes() == want.tobytes() and got[len(want):].tobytes() == b"\xee" * (72 * (len(got) - len(want)))


def test_chained_with_the_distance_transform(dev):
    """ops.frontiers on the transform's own d2: the clearance gate as the session uses it."""
    from emfusion_amd import ops
    classes = np.random.default_rng(0xF7).choice(np.array([0, 0, 0, 0, 0, 0, 1, 2, 2], np.uint8), (12, 20, 70))
    d_classes = to_dev(classes)
    d2 = ops.distance_transform(d_classes, site_mask=2, cap=2)
    from tests import distance_reference as dr
    want_d2 = dr.distance_transform(classes, 2, 2)
    assert d2.numpy().tobytes() == want_d2.tobytes()
    for min_voxels in (1, 5):
        labels, records, counts = ops.frontiers(d_classes, d2=d2, min_d2=4, min_voxels=min_voxels)
        want_labels, want, want_counts = fr.frontiers(classes, want_d2, 4, min_voxels)
        assert labels.numpy().tobytes() == want_labels.tobytes() and records.tobytes() == want.tobytes() and counts == want_counts
        assert 0 < want_counts[0] <= want_counts[1] < want_counts[2] < fr.frontiers(classes)[2][2]  # the gate does bite
