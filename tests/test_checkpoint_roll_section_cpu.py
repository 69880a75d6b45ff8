"""Checkpoint version 2 (csrc/core/Checkpoint.cpp): a session whose background has been rolled writes
the version 1 layout plus one trailing "ROLL" section behind the last packed record.  emf_fusion_checkpoint_info (no
device) parses a file assembled here from the format's restatement and refuses misplaced or damaged sections."""
import struct

import numpy as np
import pytest

from emfusion_amd import pipeline
from tests import checkpoint_format as CF
from tests.test_pack_reference_cpu import BG, assembled


def mesh_bytes(nv, nt, colors=False):
    rng = np.random.default_rng(nv + nt)
    out = struct.pack("<QQII", nv, nt, int(colors), int(colors and nv > 0))
    out += rng.standard_normal(3 * nv).astype(np.float32).tobytes() * 2  # cloud, normals
    out += rng.integers(0, max(nv, 1), 4 * nt).astype(np.int32).tobytes()
    if colors and nv > 0:
        out += rng.integers(0, 255, 3 * nv).astype(np.uint8).tobytes()
    return out


def roll_payload(origin=(32, 8, -8), follow=1, step=(32, 8, 8), look=0.5, keep=1, slabs=((6, (0, 0, 0), (33, 16, 16), 9, 3),)):
    out = struct.pack("<3i", *origin) + struct.pack("<i3ifi", follow, *step, look, keep) + CF.pose_bytes(t=(0.64, 0.16, 0.5))
    out += struct.pack("<i", len(slabs))
    for frame, org, res, nv, nt in slabs:
        out += struct.pack("<7i", frame, *org, *res) + mesh_bytes(nv, nt)
    return out


def v2_file(payload=None, version=2, roll_at=-1):
    parts, _ = assembled()
    prm = CF.params_block(bg_res=BG, bg_voxel=0.08, obj_res=(8, 8, 8))
    parts[0] = CF.header(prm, version=version)
    roll = CF.section(b"ROLL", 0, 0, roll_payload() if payload is None else payload)
    parts.insert(len(parts) + roll_at, roll)  # -1: in front of the end marker
    return b"".join(parts)


def test_checkpoint_info_reads_a_rolled_session(tmp_path):
    path = tmp_path / "rolled.ckpt"
    path.write_bytes(v2_file())
    d = pipeline.checkpoint_info(path)
    assert d["version"] == 2 and d["background_origin"] == [32, 8, -8] and d["retired_slabs"] == 1
    assert d["frame_index"] == 7 and d["file_bytes"] == path.stat().st_size and len(d["records"]) == 5


def test_a_never_rolled_file_reports_version_1_and_a_zero_origin(tmp_path):
    path = tmp_path / "plain.ckpt"
    path.write_bytes(b"".join(assembled()[0]))
    d = pipeline.checkpoint_info(path)
    assert d["version"] == 1 and d["background_origin"] == [0, 0, 0] and d["retired_slabs"] == 0


def refused(tmp_path, data):
    path = tmp_path / "bad.ckpt"
    path.write_bytes(data)
    with pytest.raises(pipeline.FusionError) as e:
        pipeline.checkpoint_info(path)
    assert e.value.code == -4  # EMF_E_ARG
    return str(e.value)


def test_misplaced_and_damaged_roll_sections_are_refused(tmp_path):
    assert "roll section out of place" in refused(tmp_path, v2_file(version=1))             # version 1 has none
    assert "roll section out of place" in refused(tmp_path, v2_file(roll_at=-2))            # in front of the last record
    parts, _ = assembled()
    parts[0] = CF.header(CF.params_block(bg_res=BG, bg_voxel=0.08, obj_res=(8, 8, 8)), version=2)
    assert "version 2 without its roll section" in refused(tmp_path, b"".join(parts))
    two = v2_file()
    roll = CF.section(b"ROLL", 0, 0, roll_payload())
    assert "roll section out of place" in refused(tmp_path, two[:-len(CF.END)] + roll + CF.END)  # twice
    assert "shorter than its contents" in refused(tmp_path, v2_file(roll_payload()[:-16]))     # a mesh cut short
    assert "follow parameters" in refused(tmp_path, v2_file(roll_payload(step=(0, 8, 8))))
    assert "follow parameters" in refused(tmp_path, v2_file(roll_payload(step=(33, 8, 8))))  # what the setter refuses
    assert "follow parameters" in refused(tmp_path, v2_file(roll_payload(look=float("nan"))))
    good = roll_payload(slabs=((5, (4, 4, 4), (2, 2, 2), 1, 0),))
    at = good.index(struct.pack("<QQ", 1, 0))  # the slab's vertex count: claim more vertices than the section could hold
    huge = good[:at] + struct.pack("<Q", 1 << 40) + good[at + 8:]
    assert "exceeds" in refused(tmp_path, v2_file(huge))
    assert "format version 3" in refused(tmp_path, v2_file(version=3))
