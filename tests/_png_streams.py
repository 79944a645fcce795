"""Checks of a PNG stream that use nothing of this project: the chunk structure and CRCs, Pillow's pixels, zlib's inflate of the
IDAT payloads against the filter rule of include/uwip.h restated in numpy, and zlib's own Z_RLE deflate as the size reference.
Shared by the emulated, the GPU and the CLI tests of the device PNG encoder."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

SIG = b"\x89PNG\r\n\x1a\n"


def chunks(stream):
    """[(type, payload)] of a stream; every CRC is checked, and nothing may follow IEND."""
    assert stream[:8] == SIG
    pos, out = 8, []
    while pos < len(stream):
        n, = struct.unpack(">I", stream[pos:pos + 4])
        typ, body = stream[pos + 4:pos + 8], stream[pos + 8:pos + 8 + n]
        assert len(body) == n
        assert zlib.crc32(typ + body) == struct.unpack(">I", stream[pos + 8 + n:pos + 12 + n])[0], typ
        out.append((typ, body))
        pos += 12 + n
    assert pos == len(stream) and out[-1] == (b"IEND", b"")
    return out


def zlib_stream(stream):
    ch = chunks(stream)
    assert ch[0][0] == b"IHDR" and all(t == b"IDAT" for t, _ in ch[1:-1]), [t for t, _ in ch]      # no ancillary chunks
    return b"".join(b for t, b in ch if t == b"IDAT")


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered(img, filt):
    """The filtered bytes of img ([H, W, 3] BGR or [H, W] grey), type bytes included.  filt -1: per row the type 0..4 with the
    smallest sum of min(v, 256 - v), ties to the lowest type, the row above row 0 taken as zeros; 0..4: that type."""
    rgb = img[..., ::-1] if img.ndim == 3 else img
    H, W = img.shape[:2]
    bpp = 3 if img.ndim == 3 else 1
    x = rgb.reshape(H, W * bpp).astype(np.int32)
    a = np.zeros_like(x); a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, bpp:] = x[:-1, :-bpp]
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]).astype(np.uint8)      # [5, H, W * bpp]
    v = cand.astype(np.int64)
    cost = np.minimum(v, 256 - v).sum(axis=2)                                                          # [5, H]
    types = np.argmin(cost, axis=0) if filt < 0 else np.full(H, filt)                                  # argmin: first minimum
    rows = cand[types, np.arange(H)]
    return np.concatenate([types.astype(np.uint8)[:, None], rows], axis=1).tobytes()


def check_stream(stream, img, filt, bound, chunk):
    """Pillow's pixels are img's; the inflated IDATs are exactly the filtered bytes; the stream keeps to the bound.  Returns
    (the zlib stream, the filtered bytes)."""
    got = np.asarray(Image.open(io.BytesIO(stream)))
    want = img[..., ::-1] if img.ndim == 3 else img
    assert got.shape == want.shape and np.array_equal(got, want)
    z = zlib_stream(stream)
    raw = zlib.decompress(z)                               # checks the Adler-32 as well
    assert raw == filtered(img, filt)
    assert 0 < len(stream) <= bound
    assert len(chunks(stream)) == 2 + (len(raw) + chunk - 1) // chunk + 1      # IHDR, one IDAT per chunk, the Adler-32's, IEND
    return z, raw


def rle_reference_bytes(raw, chunk):
    """zlib's own Z_RLE deflate of raw, one fresh raw-deflate object per chunk, flushed with Z_FULL_FLUSH: the summed lengths."""
    total = 0
    for i in range(0, len(raw), chunk):
        o = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        total += len(o.compress(raw[i:i + chunk]) + o.flush(zlib.Z_FULL_FLUSH))
    return total
