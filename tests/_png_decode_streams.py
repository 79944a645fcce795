"""PNG streams for the tests of the device PNG decoder, built without this project's code: any samples per pixel 1..4, any
row filter (forced, or a cycle in which every type follows every other), and the zlib stream by a recipe -- stored, fixed,
Huffman only, RLE, level 1, level 9 with memLevel 9, in one IDAT or cut every 1000 bytes, or flushed (full / sync) with an
IDAT per flush.  Also Pillow's own output, and a restatement of the host reader (imgio::read_png, cli/imgio.hpp) for streams
Pillow does not read.  Shared by the emulated, the ABI and the GPU tests."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

from _png_streams import SIG, _paeth

Z_FIXED = getattr(zlib, "Z_FIXED", 4)
CTYPE = {1: 0, 2: 4, 3: 2, 4: 6}
MODE = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
SHAPES = ((1, 1), (1, 300), (300, 1), (5, 7), (97, 113), (200, 333))
CHUNK = 32768


def de_bruijn_5():
    """0..4 in a cycle of 25 in which every type is followed by every type (itself included)."""
    k, n, a, seq = 5, 2, [0] * 10, []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


MIX = de_bruijn_5()


def content(H, W, spp, kind="uw", seed=0):
    """[H, W, spp] uint8 samples in file order: smooth gradients with texture, or noise."""
    rng = np.random.default_rng(seed * 7919 + H * 131 + W * 17 + spp)
    if kind == "noise":
        return rng.integers(0, 256, size=(H, W, spp), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * (3 + c) + y * (5 - c) + 40 * c) % 256 for c in range(spp)], axis=-1)
    tex = rng.integers(0, 12, size=(H, W, spp))
    flat = (x // 9 + y // 5) % 3 == 0
    out = np.where(flat[..., None], base // 16 * 16, (base + tex) % 256)
    return out.astype(np.uint8)


def period97():
    """200 x 333 grey noise with a period of 97 rows: zlib at level 9 finds the matches at distance 97 * 334 = 32398."""
    rng = np.random.default_rng(97)
    block = rng.integers(0, 256, size=(97, 333, 1), dtype=np.uint8)
    return np.concatenate([block, block, block[:6]], axis=0)


def filtered(arr, filt):
    """The filtered bytes of arr [H, W, spp], type bytes included; filt 0..4, or "mix": MIX from row 0 on."""
    H, W, spp = arr.shape
    x = arr.reshape(H, W * spp).astype(np.int32)
    a = np.zeros_like(x); a[:, spp:] = x[:, :-spp]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, spp:] = x[:-1, :-spp]
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]).astype(np.uint8)
    types = np.array([MIX[r % 25] for r in range(H)]) if filt == "mix" else np.full(H, filt)
    rows = cand[types, np.arange(H)]
    return np.concatenate([types.astype(np.uint8)[:, None], rows], axis=1).tobytes()


def _obj(level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8):
    return zlib.compressobj(level, zlib.DEFLATED, 15, mem, strategy)


def _flushed(raw, every, mode, level=6, mem=8):
    o, parts = _obj(level, mem=mem), []
    for i in range(0, len(raw), every):
        last = i + every >= len(raw)
        parts.append(o.compress(raw[i:i + every]) + (o.flush() if last else o.flush(mode)))
    return parts


# name -> raw bytes -> the IDAT payloads
RECIPES = {
    "stored": lambda raw: [zlib.compress(raw, 0)],
    "fixed": lambda raw: [(lambda o: o.compress(raw) + o.flush())(_obj(6, Z_FIXED))],
    "huffman": lambda raw: [(lambda o: o.compress(raw) + o.flush())(_obj(6, zlib.Z_HUFFMAN_ONLY))],
    "rle": lambda raw: [(lambda o: o.compress(raw) + o.flush())(_obj(6, zlib.Z_RLE))],
    "l1": lambda raw: [zlib.compress(raw, 1)],
    "l9m9": lambda raw: [(lambda o: o.compress(raw) + o.flush())(_obj(9, mem=9))],
    "l6cut1000": lambda raw: (lambda z: [z[i:i + 1000] for i in range(0, len(z), 1000)])(zlib.compress(raw, 6)),
    "full32k": lambda raw: _flushed(raw, CHUNK, zlib.Z_FULL_FLUSH),
    "sync32k": lambda raw: _flushed(raw, CHUNK, zlib.Z_SYNC_FLUSH, 9, 9),
    "full10k": lambda raw: _flushed(raw, 10000, zlib.Z_FULL_FLUSH),
}


def chunk(typ, body):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def ihdr(H, W, spp, depth=8, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, CTYPE[spp], 0, 0, interlace))


def assemble(H, W, spp, idats):
    return SIG + ihdr(H, W, spp) + b"".join(chunk(b"IDAT", p) for p in idats) + chunk(b"IEND", b"")


def stream(arr, filt, recipe):
    """A PNG of arr [H, W, spp] with the row filter `filt` and the zlib stream of RECIPES[recipe]."""
    H, W, spp = arr.shape
    return assemble(H, W, spp, RECIPES[recipe](filtered(arr, filt)))


def pil_stream(arr, **kw):
    H, W, spp = arr.shape
    buf = io.BytesIO()
    Image.fromarray(arr[..., 0] if spp == 1 else arr, MODE[spp]).save(buf, format="PNG", **kw)
    return buf.getvalue()


def expected(arr, channels=3):
    """What the host reader returns for a stream of arr: alpha dropped, RGB -> BGR, grey replicated (or kept: channels 1)."""
    spp = arr.shape[2]
    if spp <= 2:
        return arr[..., 0].copy() if channels == 1 else np.repeat(arr[..., :1], 3, axis=2)
    return np.ascontiguousarray(arr[..., 2::-1])


def pil_pixels(s, channels=3):
    """Pillow's decode of a valid stream in the host reader's layout."""
    im = Image.open(io.BytesIO(s))
    a = np.asarray(im)
    return expected(a.reshape(a.shape[0], a.shape[1], -1), channels)


def idat_span(s):
    """(offset of the first IDAT's payload, offset behind the last IDAT's payload) in the file."""
    pos, first, last = 8, None, None
    while pos + 12 <= len(s):
        n, = struct.unpack(">I", s[pos:pos + 4])
        if s[pos + 4:pos + 8] == b"IDAT":
            first = pos + 8 if first is None else first
            last = pos + 8 + n
        pos += 12 + n
    return first, last


def read_png_restated(s, force_color=True):
    """imgio::read_png in numpy / Python: the pixels, or None where it returns false."""
    if len(s) < 33 or s[:8] != SIG:
        return None
    pos, z, W, H, depth, ctype, inter = 8, b"", 0, 0, 0, 0, 0
    while pos + 12 <= len(s):
        n, = struct.unpack(">I", s[pos:pos + 4])
        typ, d = s[pos + 4:pos + 8], s[pos + 8:pos + 8 + n]
        if pos + 12 + n > len(s):
            return None
        if typ == b"IHDR":
            W, H, depth, ctype, _, _, inter = struct.unpack(">IIBBBBB", s[pos + 8:pos + 21])
        elif typ == b"IDAT":
            z += d
        elif typ == b"IEND":
            break
        pos += 12 + n
    spp = {0: 1, 2: 3, 4: 2, 6: 4}.get(ctype, 0)
    if depth != 8 or inter != 0 or W == 0 or H == 0 or not spp:
        return None
    try:
        o = zlib.decompressobj()
        raw = o.decompress(z)
        if not o.eof:
            return None
    except zlib.error:
        return None
    stride = W * spp
    if len(raw) != (stride + 1) * H:
        return None
    px = np.zeros((H, stride), dtype=np.uint8)
    for y in range(H):
        ft, line = raw[y * (stride + 1)], raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)]
        out = px[y]
        for i in range(stride):
            a = int(out[i - spp]) if i >= spp else 0
            b = int(px[y - 1, i]) if y else 0
            c = int(px[y - 1, i - spp]) if y and i >= spp else 0
            pred = (0, a, b, (a + b) >> 1, int(_paeth(np.int32(a), np.int32(b), np.int32(c))))[ft] if ft <= 4 else 0
            out[i] = (line[i] + pred) & 255
    return expected(px.reshape(H, W, spp), 3 if force_color or spp > 2 else 1)
