"""JPEG streams for the decoder tests, written by Pillow (libjpeg-turbo) at test time: the domain on which the host decoder
(jpeg::decode, cli/jpeg.hpp) was checked against Pillow's decode without a difference."""
import io

import numpy as np
from PIL import Image, ImageFile

from uwimageproc_amd import synth

# Pillow's encoder fails with "Suspension not allowed here" on tiny images with its default buffer
ImageFile.MAXBLOCK = 1 << 22

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (61, 83), (135, 243)]
FORMS = {"plain": {}, "optimize": {"optimize": True}, "rstblocks": {"restart_marker_blocks": 3}, "rstrows": {"restart_marker_rows": 1}}


def content(H, W, kind="uw", seed=0):
    """[H, W, 3] BGR frame: underwater-like, or noise."""
    if kind == "noise":
        return np.random.default_rng(seed + 31 * H + W).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return np.ascontiguousarray(synth.uw_stream(seed, 1, H, W)[0])


def pil_stream(img, quality=95, subsampling=0, **kw):
    """img: [H, W, 3] BGR with subsampling 0 / 1 / 2, or [H, W] grey (subsampling ignored)."""
    buf = io.BytesIO()
    if img.ndim == 2:
        Image.fromarray(img, "L").save(buf, format="JPEG", quality=quality, **kw)
    else:
        Image.fromarray(np.ascontiguousarray(img[..., ::-1]), "RGB").save(buf, format="JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def pil_decode(stream, channels=3):
    """Pillow's pixels in the layout of the library: [H, W, 3] BGR (a grey stream replicated) or [H, W] grey."""
    im = Image.open(io.BytesIO(stream))
    if channels == 1:
        return np.asarray(im.convert("L") if im.mode != "L" else im)
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def segment_start(stream):
    """Offset of the first entropy-coded byte (behind the SOS header)."""
    sos = stream.index(b"\xff\xda")
    return sos + 2 + ((stream[sos + 2] << 8) | stream[sos + 3])


def strip_dht(stream):
    """The stream without its DHT segments (a Motion-JPEG frame that relies on the Annex K tables)."""
    out, pos = bytearray(stream[:2]), 2
    while True:
        assert stream[pos] == 0xFF
        m = stream[pos + 1]
        L = (stream[pos + 2] << 8) | stream[pos + 3]
        if m != 0xC4:
            out += stream[pos:pos + 2 + L]
        pos += 2 + L
        if m == 0xDA:
            break
    return bytes(out) + stream[pos:]


def kinds():
    """(name, stream, channels of the batch) for every size x subsampling 0 / 1 / 2 / grey x form."""
    for H, W in SIZES:
        img = content(H, W)
        for sub in (0, 1, 2, "grey"):
            for form, kw in FORMS.items():
                src = np.ascontiguousarray(img[..., 1]) if sub == "grey" else img
                yield f"{H}x{W}_s{sub}_{form}", pil_stream(src, 95, 0 if sub == "grey" else sub, **kw), 3


def write_mjpeg_avi(path, jpegs, fps, width, height):
    """A minimal RIFF AVI with one Motion-JPEG video stream (what `ffmpeg -c:v mjpeg` writes, without the index)."""
    import struct

    def chunk(tag, body):
        return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")

    def lst(kind, body):
        return chunk(b"LIST", kind + body)
    avih = struct.pack("<14I", int(1e6 / fps), 0, 0, 0x10, len(jpegs), 0, 1, 0, width, height, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII", 0, 0, 0, 0, 1, int(fps), 0, len(jpegs), 0, 0xFFFFFFFF, 0) + struct.pack("<4h", 0, 0, width, height)
    strf = struct.pack("<IiiHHIIiiII", 40, width, height, 1, 24, 0x47504A4D, width * height * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi = lst(b"movi", b"".join(chunk(b"00dc", j) for j in jpegs))
    body = b"AVI " + hdrl + movi
    open(path, "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)


def misplaced_rst(stream):
    """A restart-marker stream whose first RST0 is renumbered RST1: the host decoder resynchronises at any RSTn and returns
    the same pixels; for the device decoder the markers are out of cyclic order (UWIP_JPEG_HOST_ONLY)."""
    a = segment_start(stream)
    at = stream.index(b"\xff\xd0", a)
    return stream[:at] + b"\xff\xd1" + stream[at + 2:]


def sampled_1x2(stream):
    """A 4:2:2 stream (luma 2x1) with the luma sampling factors rewritten to 1x2: as many blocks per MCU, another geometry.
    The host decoder reads it (rows replicated); the device decoder reports UWIP_JPEG_HOST_ONLY."""
    sof = stream.index(b"\xff\xc0")
    assert stream[sof + 9] == 3 and stream[sof + 11] == 0x21 and stream[sof + 14] == 0x11
    return stream[:sof + 11] + b"\x12" + stream[sof + 12:]
