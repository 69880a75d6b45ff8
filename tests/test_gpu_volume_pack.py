"""The lossless buffer packer on the device (include/emf_hip.h "Packed buffers": emf_hip_packClassify / packRank /
packGather / unpackFill / unpackLiterals through ops.pack_buffer / ops.unpack_buffer) against the numpy restatement
of the record (tests/pack_reference.py), byte for byte."""
import numpy as np
import pytest

from tests import pack_reference as PR

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SIZES = [4, 1020, 1024, 1028, 65536, 65540, 3 * MIB + 516]  # the last: 3073 chunks (> 1024, the scan's stride), ragged
CONTENTS = ["zero", "negzero", "nan", "random", "mixture", "diff0", "diff1", "diff255", "tail255"]
NEGZERO, NAN, W64 = 0x80000000, 0x7FC00123, 0x42800000  # -0.0f, a quiet NaN with a payload, 64.0f
GUARD = 1024
_cache = {}


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops
    return ops


def make(content: str, nbytes: int) -> np.ndarray:
    n = nbytes // 4
    nchunks = (n + PR.WORDS - 1) // PR.WORDS
    rng = np.random.default_rng(nbytes * 31 + CONTENTS.index(content))
    if content == "zero":
        return np.zeros(n, np.uint32)
    if content == "negzero":
        return np.full(n, NEGZERO, np.uint32)
    if content == "nan":
        return np.full(n, NAN, np.uint32)
    if content == "random":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if content == "mixture":
        a = np.zeros(nchunks * PR.WORDS, np.uint32).reshape(nchunks, PR.WORDS)
        kind = rng.integers(0, 3, nchunks)
        fills = np.array([NEGZERO, NAN, W64, 1, 0xFFFFFFFF], np.uint32)
        a[kind == 1] = fills[rng.integers(0, len(fills), int((kind == 1).sum()))][:, None]
        a[kind == 2] = rng.integers(0, 1 << 32, (int((kind == 2).sum()), PR.WORDS), dtype=np.uint64).astype(np.uint32)
        return a.reshape(-1)[:n].copy()
    if content.startswith("diff"):  # uniform chunks; one differing word in the first, a middle and the last chunk
        pos = int(content[4:])
        a = np.full(n, W64, np.uint32)
        for c in sorted({0, nchunks // 2, nchunks - 1}):
            valid = min(PR.WORDS, n - c * PR.WORDS)
            a[c * PR.WORDS + min(pos, valid - 1)] = W64 + 1
        return a
    assert content == "tail255"  # zero chunks whose only non-zero word is the last one: word 255, and the tail's last
    a = np.zeros(n, np.uint32)
    for c in sorted({0, nchunks // 2, nchunks - 1}):
        valid = min(PR.WORDS, n - c * PR.WORDS)
        a[c * PR.WORDS + valid - 1] = 7
    return a


def case(content, nbytes):
    """(source words, the restatement's record) -- computed once and left unchanged."""
    key = (content, nbytes)
    if key not in _cache:
        src = make(content, nbytes)
        src.setflags(write=False)
        _cache[key] = (src, PR.pack(src))
    return _cache[key]


CASES = [(c, s) for s in SIZES for c in CONTENTS]


@pytest.mark.parametrize("content,nbytes", CASES)
def test_record_equals_the_restatement_and_repeats(ops, dev, content, nbytes):
    src, want = case(content, nbytes)
    d = dev.DeviceArray.from_numpy(src)
    got = ops.pack_buffer(d, arena_chunks=1000)
    assert len(got) == len(want) and got == want
    assert ops.pack_buffer(d, arena_chunks=1000) == got
    counts = PR.class_counts(want)
    if content == "zero":
        assert counts[1] == counts[2] == 0 and len(want) == 24 + (counts[0] + 7) // 8 * 8
    if content in ("negzero", "nan"):
        assert counts[0] == counts[2] == 0
    if content.startswith("diff") or content == "tail255":  # (a chunk of one word is uniform whatever it holds)
        assert counts[2] >= 1 or nbytes == 4


@pytest.mark.parametrize("content,nbytes", CASES)
def test_unpack_restores_the_source_and_spares_the_guard(ops, dev, content, nbytes):
    src, record = case(content, nbytes)
    assert PR.unpack(record) == src.tobytes()  # (the restatement's own round trip)
    raw = dev.DeviceArray((nbytes + GUARD,), np.uint8).fill_bytes_(0xFF)
    ops.unpack_buffer(record, dev.DeviceView(raw.ptr, (nbytes // 4,), np.uint32), arena_chunks=700)
    back = raw.numpy()
    assert back[:nbytes].tobytes() == src.tobytes()
    assert (back[nbytes:] == 0xFF).all()


@pytest.mark.parametrize("content,nbytes", [("random", 65540), ("mixture", 65540), ("mixture", 3 * MIB + 516),
                                            ("random", 3 * MIB + 516), ("diff255", 3 * MIB + 516)])
def test_gather_in_unequal_rank_ranges_equals_one_range(ops, dev, content, nbytes):
    src, want = case(content, nbytes)
    d = dev.DeviceArray.from_numpy(src)
    p = ops.pack_arrays(d)
    nl = p["nliteral"]
    assert nl == PR.class_counts(want)[2] and nl >= 3
    whole = ops.pack_gather(d, p, 0, nl)
    assert whole.tobytes() == want[len(want) - nl * PR.CHUNK:]
    cuts = [0, 1, 1 + (nl - 1) // 3, nl - 1, nl, nl]  # unequal parts, one of a single chunk, one empty
    parts = [ops.pack_gather(d, p, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [len(x) for x in parts] == [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    assert ops.pack_buffer(d, splits=[b - a for a, b in zip(cuts[:-1], cuts[1:])]) == want


def test_bad_arguments_are_refused_before_any_launch(ops, dev):
    from emfusion_amd import _lib
    d = dev.DeviceArray.zeros((512,), np.uint32)
    L = _lib.load()
    assert L.emf_hip_packClassify(d.ptr, 6, d.ptr, d.ptr, None) == -4          # not a multiple of 4
    assert L.emf_hip_packClassify(d.ptr + 4, 1024, d.ptr, d.ptr, None) == -4   # not 16-byte aligned
    assert L.emf_hip_packClassify(None, 1024, d.ptr, d.ptr, None) == -1
    assert L.emf_hip_packClassify(d.ptr, (1 << 40) + 4, d.ptr, d.ptr, None) == -5
    assert L.emf_hip_packGather(d.ptr, 2048, d.ptr, 1, 2, d.ptr, None) == -4   # ranks [1, 3) of 2 chunks
    assert L.emf_hip_unpackLiterals(d.ptr, 2048, d.ptr, 3, 0, d.ptr, None) == -4
    assert L.emf_hip_unpackFill(d.ptr, 2048, d.ptr, d.ptr, d.ptr, 3, None) == -4
    assert L.emf_hip_packScratchBytes(0) == 0 and L.emf_hip_packScratchBytes(1024 * 257) == 8 * 3
    with pytest.raises(ValueError):
        ops.unpack_buffer(PR.pack(np.zeros(256, np.uint32)), d)                  # a record of another size
    assert (d.numpy() == 0).all()


def test_offsets_past_four_gib(ops, dev):
    """4 GiB + 2052 bytes of zeros with a literal or a uniform chunk at chunk 0, on both sides of the 4 GiB line and
    in the ragged last chunk (one word).  Only the small arrays and 4 KiB slices travel to the host."""
    nbytes = (1 << 32) + 2052
    n = nbytes // 4
    nchunks = (nbytes + 1023) // 1024
    assert nchunks == 4194307
    rng = np.random.default_rng(5)
    special = {0: rng.integers(1, 1 << 32, 256, dtype=np.uint64).astype(np.uint32),         # literal
               4194303: np.full(256, W64, np.uint32),                                        # uniform
               4194304: rng.integers(1, 1 << 32, 256, dtype=np.uint64).astype(np.uint32),   # literal, past 2^32
               nchunks - 1: np.array([NAN], np.uint32)}                                      # the ragged chunk: uniform
    host = np.zeros(n, np.uint32)  # (untouched pages of it are never committed)
    d = dev.DeviceArray.zeros((n,), np.uint32)
    for c, w in special.items():
        host[c * 256:c * 256 + len(w)] = w
        dev.DeviceView(d.ptr + c * 1024, (len(w),), np.uint32).copy_from(w)
    want = PR.pack(host)
    cls = PR.parse(want)[1]
    assert sorted(np.flatnonzero(cls).tolist()) == sorted(special) and PR.class_counts(want) == [nchunks - 4, 2, 2]

    got = ops.pack_buffer(d)
    assert len(got) == len(want) and got == want

    raw = dev.DeviceArray((nbytes + GUARD,), np.uint8).fill_bytes_(0xFF)
    ops.unpack_buffer(got, dev.DeviceView(raw.ptr, (n,), np.uint32))
    for c in list(special) + [1000, 3000000]:
        lo = max(0, c * 1024 - 1536)
        hi = min(nbytes, lo + 4096)
        back = dev.DeviceView(raw.ptr + lo, (hi - lo,), np.uint8).numpy()
        assert back.tobytes() == host[lo // 4:hi // 4].tobytes(), c
    assert (dev.DeviceView(raw.ptr + nbytes, (GUARD,), np.uint8).numpy() == 0xFF).all()
