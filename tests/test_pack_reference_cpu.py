"""CPU checks of the checkpoint's host side: the numpy restatement of the packed record round-trips its own cases,
and emf_fusion_checkpoint_info (no device, no handle) parses a file the test assembles from the restatement's records
and refuses damaged ones."""
import struct

import numpy as np
import pytest

from tests import checkpoint_format as CF
from tests import pack_reference as PR


def _cases():
    rng = np.random.default_rng(11)
    rnd = lambda n: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    mixed = np.zeros(5 * 256 + 7, np.uint32)
    mixed[256:512] = 0x80000000          # -0.0f: uniform, not zero
    mixed[512:768] = rnd(256)            # literal
    mixed[768:1024] = 0x42800000         # 64.0f
    mixed[1024 + 255] = 1                # zero but for its last word: literal
    mixed[1280:] = 0x7FC00001            # ragged tail, one NaN pattern: uniform
    return {"one_word": np.array([5], np.uint32), "zeros": np.zeros(300, np.uint32), "random": rnd(1000),
            "mixed": mixed, "ragged_literal": np.concatenate([np.zeros(256, np.uint32), rnd(3)])}


@pytest.mark.parametrize("name", list(_cases()))
def test_restatement_round_trips(name):
    a = _cases()[name]
    rec = PR.pack(a)
    assert PR.unpack(rec) == a.tobytes()
    assert PR.record_size(rec) == len(rec) and len(rec) % 8 == 0
    nbytes, cls, uniform, literals = PR.parse(rec)
    assert nbytes == a.nbytes and len(cls) == (a.nbytes + 1023) // 1024
    assert PR.pack(np.frombuffer(PR.unpack(rec), np.uint32)) == rec


def test_restatement_layout_of_a_known_buffer():
    rec = PR.pack(_cases()["mixed"])
    assert PR.class_counts(rec) == [1, 3, 2]
    assert struct.unpack_from("<QIIII", rec) == ((5 * 256 + 7) * 4, 6, 3, 2, 0)
    assert rec[24:32] == bytes([0, 1, 2, 1, 2, 1, 0, 0])                                   # classes, padded to 8
    assert struct.unpack_from("<4I", rec, 32) == (0x80000000, 0x42800000, 0x7FC00001, 0)    # uniform words, padded
    assert len(rec) == 24 + 8 + 16 + 2 * 1024 and rec[-4:] == struct.pack("<I", 1)
    with pytest.raises(ValueError):
        PR.parse(rec[:-8])
    with pytest.raises(ValueError):
        PR.parse(rec[:24] + bytes([2]) + rec[25:])


# ---- checkpoint_info on an assembled file --------------------------------------------------------------------------

BG, OBJ_RES = (16, 16, 16), (8, 8, 10)


def assembled(color=False):
    """A complete file: background 16^3, one object (id 3) of 8 x 8 x 10, every record from the restatement."""
    rng = np.random.default_rng(3)
    nb, no = int(np.prod(BG)), int(np.prod(OBJ_RES))
    tsdf = np.zeros(nb, np.float32)
    tsdf[1000:1300] = rng.standard_normal(300).astype(np.float32)
    vols = [(0, CF.VOL_TSDF, tsdf), (0, CF.VOL_WEIGHTS, np.full(nb, 64.0, np.float32))]
    if color:
        vols.append((0, CF.VOL_COLOR, np.zeros((nb, 4), np.uint16)))
    vols += [(3, CF.VOL_TSDF, rng.standard_normal(no).astype(np.float32)), (3, CF.VOL_WEIGHTS, np.zeros(no, np.float32)),
             (3, CF.VOL_FGBG, np.ones((no, 2), np.float32))]
    if color:
        vols.append((3, CF.VOL_COLOR, rng.integers(0, 65535, (no, 4)).astype(np.uint16)))
    parts = [CF.header(CF.params_block(bg_res=BG, bg_voxel=0.08, obj_res=(8, 8, 8))),
             CF.session(7, 4, color, [3], visible=[3]), CF.obj(3, OBJ_RES, scores=[0.0, 0.25, 0.75]), CF.logs()]
    recs = [(i, w, PR.pack(v)) for i, w, v in vols]
    parts += [CF.pack_section(i, w, r) for i, w, r in recs]
    return parts + [CF.END], recs


@pytest.fixture()
def info():
    from emfusion_amd import pipeline
    return pipeline


@pytest.mark.parametrize("color", [False, True])
def test_checkpoint_info_parses_an_assembled_file(info, tmp_path, color):
    parts, recs = assembled(color)
    path = tmp_path / "a.ckpt"
    path.write_bytes(b"".join(parts))
    d = info.checkpoint_info(path)
    assert d["version"] == 1 and d["frame_index"] == 7 and d["next_id"] == 4 and d["color"] is color
    assert d["file_bytes"] == path.stat().st_size
    assert d["params"]["width"] == 160 and d["params"]["height"] == 120 and d["params"]["bg_res"] == list(BG)
    assert d["params"]["bg_voxel_size"] == pytest.approx(0.08, rel=1e-6) and d["params"]["max_tsdf_weight"] == 64
    assert [(o["id"], o["res"]) for o in d["objects"]] == [(3, list(OBJ_RES))]
    assert [(r["id"], r["which"]) for r in d["records"]] == [(i, w) for i, w, _ in recs]
    for r, (_, _, rec) in zip(d["records"], recs):
        assert r["chunks"] == PR.class_counts(rec) and r["packed_bytes"] == len(rec)
        assert path.read_bytes()[r["offset"]:r["offset"] + len(rec)] == rec
    # the file taken apart again by the restatement of the format
    assert [v for k, v in sorted(CF.records(path.read_bytes()).items())] == [r for _, _, r in sorted(recs)]


def _refused(info, path, data):
    path.write_bytes(data)
    with pytest.raises(info.FusionError) as e:
        info.checkpoint_info(path)
    assert e.value.code == -4  # EMF_E_ARG
    return str(e.value)


def test_checkpoint_info_refuses_damaged_files(info, tmp_path):
    parts, _ = assembled()
    good = b"".join(parts)
    p = tmp_path / "bad.ckpt"
    prm = CF.params_block(bg_res=BG, bg_voxel=0.08, obj_res=(8, 8, 8))
    assert "magic" in _refused(info, p, CF.header(prm, magic=b"EMFCKPX\0") + good[CF.HEADER_BYTES:])
    assert "version" in _refused(info, p, CF.header(prm, version=2) + good[CF.HEADER_BYTES:])
    flipped = bytearray(good)
    flipped[40] ^= 1  # one bit of the intrinsics
    assert "checksum" in _refused(info, p, bytes(flipped))
    # cut inside the session section, inside the first packed record's literals, in front of the end marker
    off = np.cumsum([len(x) for x in parts])
    for cut in (int(off[0]) + 40, int(off[4]) - 512, int(off[-2]), CF.HEADER_BYTES - 3):
        assert "truncated" in _refused(info, p, good[:cut]), cut
    # whole sections missing although the end marker is there
    assert "truncated" in _refused(info, p, b"".join(parts[:-2]) + CF.END)
    # a record whose class array disagrees with its counts
    bad = bytearray(good)
    bad[int(off[3]) + 24 + 24] = 2
    assert "class array" in _refused(info, p, bytes(bad))
    with pytest.raises(info.FusionError):
        info.checkpoint_info(tmp_path / "does_not_exist.ckpt")
