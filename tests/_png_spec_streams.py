"""The streams for the tests of the PNG decoder's found block starts (segmented = 2): foreign zlib streams of several deflate
blocks whose matches reach across the block boundaries, streams with nothing to find, and one that carries a whole deflate
stream inside stored blocks.  Built from tests/_png_decode_streams.py and zlib alone; `blocks()` is an independent walk of a
deflate stream (RFC 1951, lengths only) that lists where its blocks start."""
import struct
import zlib

import numpy as np

import _png_decode_streams as pd

CHUNKS = (1024, 4096, 16384)


def _l6(arr):
    H, W, spp = arr.shape
    return pd.assemble(H, W, spp, [zlib.compress(pd.filtered(arr, "mix"), 6)])


def zstream(s):
    """The zlib stream of a PNG: its IDAT payloads."""
    pos, z = 8, b""
    while pos + 12 <= len(s):
        n, = struct.unpack(">I", s[pos:pos + 4])
        if s[pos + 4:pos + 8] == b"IDAT":
            z += s[pos + 8:pos + 8 + n]
        pos += 12 + n
    return z


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DEXT = [0, 0, 0, 0] + [i // 2 - 1 for i in range(4, 30)]
_CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _code(lens):
    """{(length, code): symbol} of the canonical code of `lens`."""
    out, code = {}, 0
    for l in range(1, 16):
        for s, x in enumerate(lens):
            if x == l:
                out[(l, code)] = s
                code += 1
        code <<= 1
    return out


def blocks(z):
    """[(start bit behind the zlib header, type, inflated offset)] of every deflate block of the zlib stream z."""
    d = z[2:]
    pos = 0

    def bits(n):
        nonlocal pos
        v = (int.from_bytes(d[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def sym(code):
        nonlocal pos
        v, c = int.from_bytes(d[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7), 0
        for l in range(1, 16):
            c = (c << 1) | ((v >> (l - 1)) & 1)
            if (l, c) in code:
                pos += l
                return code[(l, c)]
        raise ValueError("no code")

    fixed_ll = _code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    fixed_d = _code([5] * 32)
    out, produced = [], 0
    while True:
        start = pos
        final, typ = bits(1), bits(2)
        out.append((start, typ, produced))
        if typ == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            bits(16)
            pos += 8 * n
            produced += n
        else:
            if typ == 1:
                ll, dd = fixed_ll, fixed_d
            else:
                nl, nd, nc = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(nc):
                    cl[_CLORD[i]] = bits(3)
                clc, lens = _code(cl), []
                while len(lens) < nl + nd:
                    s = sym(clc)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    elif s == 17:
                        lens += [0] * (3 + bits(3))
                    else:
                        lens += [0] * (11 + bits(7))
                ll, dd = _code(lens[:nl]), _code(lens[nl:nl + nd])
            while True:
                s = sym(ll)
                if s < 256:
                    produced += 1
                elif s == 256:
                    break
                else:
                    produced += _LBASE[s - 257] + bits(_LEXT[s - 257])
                    bits(_DEXT[sym(dd)])
        if final:
            return out


def stream_e():
    """2 x 60000 grey, filter 0, whose pixels are B's raw deflate bytes (cut or zero-padded to the frame), in stored blocks of
    65535 bytes written by hand: B's dynamic blocks lie in the compressed input verbatim and byte-aligned."""
    raw = zstream(_l6(pd.content(200, 333, 3)))[2:-4][:120000]
    px = np.frombuffer(raw + bytes(120000 - len(raw)), dtype=np.uint8).reshape(2, 60000, 1)
    data = pd.filtered(px, 0)
    z = b"\x78\x01"
    for i in range(0, len(data), 65535):
        part = data[i:i + 65535]
        z += bytes([1 if i + 65535 >= len(data) else 0]) + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
    z += struct.pack(">I", zlib.adler32(data))
    return pd.assemble(2, 60000, 1, [z]), px


def streams():
    """name -> (stream, array in file order)"""
    a, b, c, d = pd.content(97, 113, 3), pd.content(200, 333, 3), pd.period97(), pd.content(97, 113, 3, "noise")
    e, e_px = stream_e()
    return {"A": (_l6(a), a), "B": (_l6(b), b), "Bp": (pd.pil_stream(b), b), "C": (_l6(c), c), "D": (_l6(d), d),
            "Dfixed": (pd.stream(a, "mix", "fixed"), a), "E": (e, e_px)}


def damaged_a():
    """A with every single-bit flip in the 40 bytes from compressed byte 18611 on (its second block's header and first symbols),
    cut at half its IDAT, and with another Adler-32."""
    s = _l6(pd.content(97, 113, 3))
    a, b = pd.idat_span(s)
    out = []
    for i in range(40):
        for bit in range(8):
            t = bytearray(s)
            t[a + 2 + 18611 + i] ^= 1 << bit
            out.append((f"flip_{i}_{bit}", bytes(t)))
    z = zstream(s)
    out.append(("cut", pd.assemble(97, 113, 3, [z[:len(z) // 2]])))           # a whole IDAT that holds half the stream
    out.append(("filecut", s[:a + (b - a) // 2]))                            # the file ends inside its IDAT
    t = bytearray(s)
    t[b - 1] ^= 0x40
    out.append(("adler", bytes(t)))
    return out
