"""Colour in and out on the host: 8-bit RGB / RGBA PNG decoding in C++ (core/Readers.cpp through emf_io_read_color_png)
and in Python (emfusion_amd/readers.py) against arrays -- the PNGs are encoded here with zlib, one per filter type plus
a mixed one -- and the PLY writer with and without vertex colours."""
import hashlib
import struct
import zlib

import numpy as np
import pytest

from emfusion_amd import pipeline, readers

SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def _filter_rows(img, filters):
    """PNG 9.2 scan-line filters applied to (H, W, C) u8; filters: one type 0..4 per row."""
    h, w, bpp = img.shape
    raw = img.reshape(h, w * bpp).astype(np.int32)
    out = bytearray()
    zero = np.zeros(w * bpp, np.int32)
    for y in range(h):
        f = int(filters[y])
        a = np.concatenate([zero[:bpp], raw[y, :-bpp]])
        b = raw[y - 1] if y else zero
        c = np.concatenate([zero[:bpp], b[:-bpp]])
        if f == 0:
            pred = zero
        elif f == 1:
            pred = a
        elif f == 2:
            pred = b
        elif f == 3:
            pred = (a + b) >> 1
        else:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out.append(f)
        out += ((raw[y] - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def encode_png(img, filters=None, color_type=None, depth=8, interlace=0, split_idat=False):
    h, w, bpp = img.shape
    color_type = {3: 2, 4: 6}[bpp] if color_type is None else color_type
    filters = [0] * h if filters is None else filters
    data = zlib.compress(_filter_rows(img, filters), 6)
    idat = _chunk(b"IDAT", data) if not split_idat else _chunk(b"IDAT", data[:7]) + _chunk(b"IDAT", data[7:])
    return (SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace)) +
            _chunk(b"tEXt", b"Comment\0colour test") + idat + _chunk(b"IEND", b""))


def _image(channels, w=37, h=23, seed=4):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    img[: h // 2] = (np.arange(w)[None, :, None] * 5 + np.arange(h // 2)[:, None, None] * 3) % 256  # smooth part
    return img


DECODERS = [("python", readers.read_png_color), ("c++", pipeline.read_color_png)]


@pytest.mark.parametrize("name,decode", DECODERS)
@pytest.mark.parametrize("channels", [3, 4])
def test_rgb_and_rgba_png_decode_with_every_filter(tmp_path, name, decode, channels):
    img = _image(channels)
    h = img.shape[0]
    cases = {f"f{f}": [f] * h for f in range(5)}
    cases["mixed"] = [(3 * y + 1) % 5 for y in range(h)]
    for label, filters in cases.items():
        path = tmp_path / f"{label}.png"
        path.write_bytes(encode_png(img, filters, split_idat=label == "mixed"))
        got = decode(path)
        assert got.dtype == np.uint8 and got.shape == img.shape[:2] + (3,), (name, label)
        assert np.array_equal(got, img[..., :3]), (name, label, channels)  # alpha dropped


@pytest.mark.parametrize("name,decode", DECODERS)
def test_unsupported_truncated_and_oversized_pngs_are_rejected(tmp_path, name, decode):
    img = _image(3)
    good = encode_png(img)
    bad = {
        "palette": encode_png(img[..., :1], color_type=3),
        "gray": encode_png(img[..., :1], color_type=0),
        "rgb16": encode_png(np.concatenate([img, img], -1), color_type=2, depth=16),
        "interlaced": encode_png(img, interlace=1),
        "truncated_chunk": good[: len(good) - 40],
        "truncated_header": good[:20],
        "short_data": SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", 37, 23, 8, 2, 0, 0, 0)) +
                      _chunk(b"IDAT", zlib.compress(b"\0" * 100)) + _chunk(b"IEND", b""),
        "long_data": SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 4, 8, 2, 0, 0, 0)) +
                     _chunk(b"IDAT", zlib.compress(b"\0" * 100000)) + _chunk(b"IEND", b""),
        "bad_filter": SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 2, 0, 0, 0)) +
                      _chunk(b"IDAT", zlib.compress(b"\x07" + b"\0" * 6 + b"\0" + b"\0" * 6)) + _chunk(b"IEND", b""),
        # a header that promises 100000 x 100000 pixels: refused before anything is allocated or inflated
        "oversized": SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", 100000, 100000, 8, 2, 0, 0, 0)) +
                     _chunk(b"IDAT", zlib.compress(b"\0" * 64)) + _chunk(b"IEND", b""),
        "not_png": b"P6\n2 2\n255\n" + b"\0" * 12,
    }
    for label, blob in bad.items():
        path = tmp_path / f"{label}.png"
        path.write_bytes(blob)
        with pytest.raises((ValueError, pipeline.FusionError)):
            decode(path)
    path = tmp_path / "good.png"
    path.write_bytes(good)
    assert np.array_equal(decode(path), img)


def test_depth_reader_still_refuses_colour_and_colour_reader_depth(tmp_path):
    img = _image(3)
    p = tmp_path / "rgb.png"
    p.write_bytes(encode_png(img))
    with pytest.raises(ValueError):
        readers.read_png_gray(p)
    with pytest.raises(pipeline.FusionError):
        pipeline.read_depth_png(p)
    d = tmp_path / "depth.png"
    readers.write_png_gray16(d, np.arange(12, dtype=np.uint16).reshape(3, 4))
    with pytest.raises(ValueError):
        readers.read_png_color(d)
    with pytest.raises(pipeline.FusionError):
        pipeline.read_color_png(d)


def test_tum_reader_hands_out_the_colour_image(tmp_path):
    (tmp_path / "rgb").mkdir()
    (tmp_path / "depth").mkdir()
    img = _image(4, 8, 6)
    (tmp_path / "rgb" / "1.0.png").write_bytes(encode_png(img, [4] * 6))
    readers.write_png_gray16(tmp_path / "depth" / "1.0.png", np.full((6, 8), 5000, np.uint16))
    (tmp_path / "associations.txt").write_text("1.0 rgb/1.0.png 1.0 depth/1.0.png\n")
    r = readers.TUMReader(tmp_path)
    assert np.array_equal(r.color(0), img[..., :3])
    assert r.depth(0).shape == (6, 8)


# ---- PLY ------------------------------------------------------------------------------------------------

def _mesh():
    rng = np.random.default_rng(12)
    v = rng.normal(size=(7, 3)).astype(np.float32)
    v[0] = (0, -0.0, 1e-7)
    n = rng.normal(size=(7, 3)).astype(np.float32) * 100
    t = np.array([[3, 0, 1, 2], [3, 2, 3, 4], [3, 4, 5, 6]], np.int32)
    c = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    c[1] = (0, 255, 7)
    return v, n, t, c


# sha256 of the file the PARENT commit's writer produced for _mesh() (recorded by this test before the change)
PLY_DIGEST_WITHOUT_COLOUR = "9cddac888cf6f7cd0822aa464c2b16792e4f19fca879218ca2cdc702d0eab8c2"


def test_ply_without_colour_is_the_parents_file(tmp_path):
    v, n, t, _ = _mesh()
    path = tmp_path / "plain.ply"
    pipeline.write_mesh(path, v, n, t)
    data = path.read_bytes()
    want = ("ply\nformat ascii 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nelement face 3\n"
            "property list uchar int vertex_index\nend_header\n")
    want += "".join("%f %f %f %f %f %f\n" % (*map(float, a), *map(float, b)) for a, b in zip(v, n))
    want += "".join("%d %d %d %d\n" % tuple(r) for r in t)
    assert data == want.encode()
    assert hashlib.sha256(data).hexdigest() == PLY_DIGEST_WITHOUT_COLOUR


def test_ply_with_colour_round_trips(tmp_path):
    v, n, t, c = _mesh()
    path = tmp_path / "colour.ply"
    pipeline.write_mesh(path, v, n, t, colors=c)
    lines = path.read_text().split("\n")
    end = lines.index("end_header")
    header = lines[:end]
    props = [ln.split()[1:] for ln in header if ln.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["float", "nx"], ["float", "ny"], ["float", "nz"],
                     ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"], ["list", "uchar", "int", "vertex_index"]]
    assert "element vertex 7" in header and "element face 3" in header
    assert header.index("property uchar red") < header.index("element face 3")
    body = lines[end + 1:]
    rows = [ln.split() for ln in body[:7]]
    assert all(len(r) == 9 for r in rows)
    assert np.array_equal(np.array([r[6:] for r in rows], np.int64), c)
    assert np.allclose(np.array([r[:3] for r in rows], np.float64), v, atol=5e-7)
    assert np.array_equal(np.array([ln.split() for ln in body[7:10]], np.int64), t)
    assert body[10:] == [""]
    # the plain writer's lines are the coloured writer's lines without the colour columns
    plain = tmp_path / "plain.ply"
    pipeline.write_mesh(plain, v, n, t)
    pl = plain.read_text().split("\n")
    assert [" ".join(r[:6]) for r in rows] == pl[pl.index("end_header") + 1:][:7]
