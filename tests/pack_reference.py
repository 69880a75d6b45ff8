"""numpy restatement of the packed record of include/emf_hip.h "Packed buffers" (test infrastructure): what the
device packer and the checkpoint files are compared with, byte for byte.

    u64 nbytes; u32 nchunks; u32 nuniform; u32 nliteral; u32 0
    u8  class[nchunks]            zero-padded to a multiple of 8 bytes
    u32 uniform[nuniform]         chunk order, zero-padded to a multiple of 8 bytes
    u8  literal[nliteral][1024]   chunk order; a ragged last chunk is zero-padded

class 0: every word of the chunk is 0; class 1: every word is the same non-zero word; class 2: anything else.
Words are compared as bits."""
from __future__ import annotations

import numpy as np

CHUNK = 1024
WORDS = CHUNK // 4


def as_words(data) -> np.ndarray:
    """bytes / any contiguous array -> its little-endian u32 words (a view where it can be)."""
    if isinstance(data, np.ndarray):
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    else:
        raw = np.frombuffer(data, np.uint8)
    assert raw.size % 4 == 0, "a packed buffer is a whole number of 32-bit words"
    return raw.view("<u4")


def classify(words: np.ndarray):
    """(class u8 [nchunks], first word u32 [nchunks]) of a word array; the ragged tail compares its valid words only."""
    n = words.size
    nchunks = (n + WORDS - 1) // WORDS
    full = n // WORDS
    cls = np.empty(nchunks, np.uint8)
    first = np.empty(nchunks, np.uint32)
    step = 1 << 16  # chunks per slice: bounds the temporaries for multi-GiB inputs
    for lo in range(0, full, step):
        hi = min(full, lo + step)
        blk = words[lo * WORDS:hi * WORDS].reshape(-1, WORDS)
        if not blk.any():  # (the same answer as below, without the temporaries)
            first[lo:hi] = 0
            cls[lo:hi] = 0
            continue
        f = blk[:, 0]
        uni = (blk == f[:, None]).all(axis=1)
        first[lo:hi] = f
        cls[lo:hi] = np.where(uni, np.where(f == 0, 0, 1), 2)
    if full < nchunks:
        tail = words[full * WORDS:]
        first[full] = tail[0]
        cls[full] = (0 if tail[0] == 0 else 1) if (tail == tail[0]).all() else 2
    return cls, first


def _pad8(b: bytes) -> bytes:
    return b + bytes(-len(b) % 8)


def header(nbytes: int, nchunks: int, nuniform: int, nliteral: int) -> bytes:
    return np.array([nbytes], "<u8").tobytes() + np.array([nchunks, nuniform, nliteral, 0], "<u4").tobytes()


def pack(data) -> bytes:
    words = as_words(data)
    assert words.size > 0
    cls, first = classify(words)
    lit = np.flatnonzero(cls == 2)
    uniform = first[cls == 1].astype("<u4")
    parts = [header(words.size * 4, cls.size, uniform.size, lit.size), _pad8(cls.tobytes()), _pad8(uniform.tobytes())]
    for c in lit:
        chunk = words[c * WORDS:(c + 1) * WORDS].tobytes()
        parts.append(chunk + bytes(CHUNK - len(chunk)))
    return b"".join(parts)


def parse(record):
    """(nbytes, class array, uniform words, literal bytes (nliteral, 1024)) of a record; ValueError if its lengths
    or counts disagree."""
    mv = memoryview(record)
    if len(mv) < 24:
        raise ValueError("record shorter than its header")
    nbytes = int(np.frombuffer(mv[:8], "<u8")[0])
    nchunks, nu, nl, zero = (int(v) for v in np.frombuffer(mv[8:24], "<u4"))
    if nbytes == 0 or nbytes % 4 or nchunks != (nbytes + CHUNK - 1) // CHUNK or zero:
        raise ValueError("inconsistent header")
    o_uni = 24 + (nchunks + 7) // 8 * 8
    o_lit = o_uni + (4 * nu + 7) // 8 * 8
    if len(mv) != o_lit + nl * CHUNK:
        raise ValueError(f"record of {len(mv)} bytes, header says {o_lit + nl * CHUNK}")
    cls = np.frombuffer(mv[24:24 + nchunks], np.uint8)
    if int((cls == 1).sum()) != nu or int((cls == 2).sum()) != nl or (cls > 2).any():
        raise ValueError("class array and counts disagree")
    return (nbytes, cls, np.frombuffer(mv[o_uni:o_uni + 4 * nu], "<u4"),
            np.frombuffer(mv[o_lit:], np.uint8).reshape(nl, CHUNK))


def record_size(record) -> int:
    """Length in bytes of the record that starts at record[0] (from its header alone)."""
    mv = memoryview(record)
    nchunks, nu, nl = (int(v) for v in np.frombuffer(mv[8:20], "<u4"))
    return 24 + (nchunks + 7) // 8 * 8 + (4 * nu + 7) // 8 * 8 + nl * CHUNK


def unpack(record) -> bytes:
    nbytes, cls, uniform, literals = parse(record)
    out = np.zeros(cls.size * WORDS, "<u4")
    rows = out.reshape(-1, WORDS)
    rows[cls == 1] = uniform[:, None]
    rows[cls == 2] = literals.view("<u4").reshape(-1, WORDS)
    return out.tobytes()[:nbytes]


def class_counts(record):
    cls = parse(record)[1]
    return [int((cls == k).sum()) for k in range(3)]
