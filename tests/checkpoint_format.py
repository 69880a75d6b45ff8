"""The checkpoint file format of emfusion_amd/csrc/core/Checkpoint.cpp restated in Python (test infrastructure):
assemble a file from packed records (tests/pack_reference.py) and take one apart again.

    header   magic "EMFCKPT\\0"; u32 version; u32 headerBytes; 56 parameter words; u64 FNV-1a of the bytes before it
    sections {u32 tag; i32 id; u32 which; u32 0; u64 bytes} + payload, zero-padded to 8 bytes:
             SESS, OBJ (one per object), LOGS, MESH (one per kept mesh), PACK (one per volume buffer), END!
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"EMFCKPT\0"
VERSION = 1
HEADER_BYTES = 16 + 4 * 56 + 8
VOL_TSDF, VOL_WEIGHTS, VOL_COLOR, VOL_FGBG = 0, 1, 5, 6
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def fnv1a(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _pad8(b: bytes) -> bytes:
    return b + bytes(-len(b) % 8)


def params_block(width=160, height=120, K=None, bg_res=(64, 64, 64), bg_voxel=0.04, obj_res=(32, 32, 32),
                 volume_pose_t=(0.0, 0.0, 1.28), materialize=0) -> bytes:
    """The 56 parameter words, reference defaults for what has no argument here."""
    if K is None:
        f = 525.0 * width / 640.0
        K = [f, 0, width // 2 - 0.5, 0, f, height // 2 - 0.5, 0, 0, 1]
    b = struct.pack("<2i9f2fi3i2f3if", width, height, *K, 0.04, 4.5, 7, *bg_res, bg_voxel, 10.0, *obj_res, 10.0)
    b += struct.pack("<12f", *IDENTITY, *volume_pose_t)
    b += struct.pack("<f2i4fifi", 2.0, 100, 30, 0.1, 0.5, 0.2, 5.0, 40 * 40, 0.1, 20)
    b += struct.pack("<9f2i", 1e3, 1e-8, 1e-8, 2.0, 0.2, 64.0, 0.02, 0.8, 1.0, 0, materialize)
    assert len(b) == 4 * 56
    return b


def header(params: bytes, magic=MAGIC, version=VERSION) -> bytes:
    h = magic + struct.pack("<2I", version, HEADER_BYTES) + params
    return h + struct.pack("<Q", fnv1a(h))


def section(tag: bytes, ident: int, which: int, payload: bytes) -> bytes:
    assert len(tag) == 4
    return tag + struct.pack("<iIIQ", ident, which, 0, len(payload)) + _pad8(payload)


def pose_bytes(R=IDENTITY, t=(0.0, 0.0, 0.0)) -> bytes:
    return struct.pack("<12f", *R, *t)


def session(frame_count, next_id, color, ids, visible=(), color_map=None) -> bytes:
    cm = bytes(768) if color_map is None else bytes(color_map)
    b = struct.pack("<4i", frame_count, next_id, int(color), len(ids)) + pose_bytes()
    b += struct.pack(f"<{len(ids)}i", *ids) + struct.pack(f"<i{len(visible)}i", len(visible), *visible) + cm
    return section(b"SESS", 0, 0, b)


def obj(ident, res, voxel=0.01, trunc=0.1, t=(0.0, 0.0, 1.0), ex=1, non_ex=0, scores=()) -> bytes:
    b = struct.pack("<4i2f", ident, *res, voxel, trunc) + pose_bytes(t=t)
    b += struct.pack(f"<4i{len(scores)}d", ex, non_ex, len(scores), 0, *scores)
    return section(b"OBJ ", ident, 0, b)


def logs() -> bytes:
    return section(b"LOGS", 0, 0, struct.pack("<3i", 0, 0, 0) + bytes(4))


def pack_section(ident, which, record: bytes) -> bytes:
    return section(b"PACK", ident, which, record)


END = section(b"END!", 0, 0, b"")


def split(data: bytes):
    """(header bytes, [(tag, id, which, payload offset, payload bytes)]) of a complete file."""
    assert data[:8] == MAGIC
    out = []
    at = HEADER_BYTES
    while True:
        tag = data[at:at + 4]
        ident, which, zero, n = struct.unpack_from("<iIIQ", data, at + 4)
        assert zero == 0 and at + 24 + n <= len(data), "section runs past the file"
        out.append((tag, ident, which, at + 24, n))
        at += 24 + (n + 7) // 8 * 8
        if tag == b"END!":
            break
    assert at == len(data)
    return data[:HEADER_BYTES], out


def records(data: bytes):
    """{(id, which): record bytes} of a file."""
    return {(i, w): data[off:off + n] for tag, i, w, off, n in split(data)[1] if tag == b"PACK"}
