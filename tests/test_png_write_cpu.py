"""CPU: fealess::WritePng16 (cadreco_write_png16), the mirror of ReadPng16 that CadRecoTrainViews writes the depth renders
with: it round-trips through cadreco_read_png16, and an independent zlib + struct decode of the file finds the PNG
signature, an IHDR of 16-bit greyscale, valid chunk CRCs, filter byte 0 on every row and big-endian samples."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from cadreco_py import lib as _cad


def _decode(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    o, chunks = 8, []
    while o < len(data):
        (n,) = struct.unpack(">I", data[o:o + 4])
        t, d = data[o + 4:o + 8], data[o + 8:o + 8 + n]
        (crc,) = struct.unpack(">I", data[o + 8 + n:o + 12 + n])
        assert crc == zlib.crc32(t + d) & 0xFFFFFFFF, t
        chunks.append((t, d))
        o += 12 + n
    assert o == len(data)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, interlace) == (16, 0, 0, 0, 0)
    raw = zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT"))
    row = 1 + 2 * w
    assert len(raw) == h * row
    assert all(raw[y * row] == 0 for y in range(h))                       # filter type 0 (None) on every row
    px = b"".join(raw[y * row + 1:(y + 1) * row] for y in range(h))
    return np.frombuffer(px, ">u2").reshape(h, w).astype(np.uint16)


def _images():
    rng = np.random.default_rng(3)
    yield np.zeros((1, 1), np.uint16)
    yield np.full((1, 1), 65535, np.uint16)
    yield np.array([[0, 65535, 1, 256, 255]], np.uint16)
    for h, w in ((5, 3), (9, 17), (3, 641), (31, 7)):
        yield rng.integers(0, 65536, (h, w)).astype(np.uint16)
    img = rng.integers(0, 65536, (48, 33)).astype(np.uint16)
    img[::3] = 0
    img[1::5] = 65535
    yield img


@pytest.mark.parametrize("k", range(8))
def test_write_png16_round_trip_and_format(tmp_path, k):
    img = list(_images())[k]
    lib = _cad()
    path = str(tmp_path / f"{k}.png").encode()
    assert lib.cadreco_write_png16(path, img.ctypes.data, img.shape[1], img.shape[0]) == 0
    assert np.array_equal(_decode(path.decode()), img)
    out = np.zeros(img.size, np.uint16)
    w, h = C.c_int(), C.c_int()
    assert lib.cadreco_read_png16(path, out.ctypes.data, out.size, C.byref(w), C.byref(h)) == 0
    assert (w.value, h.value) == (img.shape[1], img.shape[0])
    assert np.array_equal(out.reshape(img.shape), img)


def test_write_png16_refuses(tmp_path):
    lib = _cad()
    img = np.ones((4, 4), np.uint16)
    assert lib.cadreco_write_png16(str(tmp_path / "no" / "dir.png").encode(), img.ctypes.data, 4, 4) == -1
    assert lib.cadreco_write_png16(str(tmp_path / "a.png").encode(), img.ctypes.data, 0, 4) == -1
    assert lib.cadreco_write_png16(str(tmp_path / "b.png").encode(), None, 4, 4) == -1
