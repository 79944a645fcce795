"""CPU: the device JPEG decoder's entry points are declared, exported and bound; uwip_jpeg_info is the host decoder's header
parse with its rejections; without a device (or with null arguments) the decoder fails loudly and touches nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _jpeg_forge_cases as fc
import _jpeg_streams as js

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uwip_jpeg_info", "uwip_jpeg_decode", "uwip_jpeg_decode_host")


def test_symbols_declared_exported_and_bound():
    import uwimageproc_amd._native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uwip.h")).read(), flags=re.S)
    l = C.CDLL(nat.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(l, n), n
        assert n in nat.SIGNATURES, n
    nat.lib()
    for name, val in (("UWIP_JPEG_BAD_STREAM", -1), ("UWIP_JPEG_SIZE_MISMATCH", -2), ("UWIP_JPEG_HOST_ONLY", -3)):
        assert re.search(r"#define\s+%s\s+\(%d\)" % (name, val), text), name


def test_info_on_streams_of_each_kind():
    import uwimageproc_amd as uw
    for name, stream, _ in js.kinds():
        H, W = (int(v) for v in name.split("_")[0].split("x"))
        assert uw.jpeg.info(stream) == (H, W, 1 if "_sgrey_" in name else 3), name
    s = js.pil_stream(js.content(17, 33), 90, 2)
    assert uw.jpeg.info(js.strip_dht(s)) == (17, 33, 3)


def test_info_rejections():
    import uwimageproc_amd as uw
    import io
    from PIL import Image
    img = js.content(17, 33)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(buf, format="JPEG", progressive=True)
    good = js.pil_stream(img, 90, 2)
    sof = good.index(b"\xff\xc0")
    for bad in (buf.getvalue(), good[:sof + 6], good[:js.segment_start(good) - 3], good[:3], b"", b"\x89PNG\r\n\x1a\n" + bytes(64),
                good[:sof + 4] + b"\x0c" + good[sof + 5:]):                     # 12-bit precision
        with pytest.raises(uw.UwipError):
            uw.jpeg.info(bad)


def test_info_of_forged_geometries():
    """An MCU of more than 10 blocks is no baseline stream (T.81 B.2.3): UWIP_ERR_UNSUPPORTED.  The SOF factors of a single
    component do not matter; every other triple of factors 1..2 parses."""
    import uwimageproc_amd as uw
    import uwimageproc_amd._native as nat
    s = fc.twelve_blocks().stream
    buf = (C.c_uint8 * len(s)).from_buffer_copy(s)
    r, c, ch = C.c_int32(5), C.c_int32(5), C.c_int32(5)
    assert nat.lib().uwip_jpeg_info(C.cast(buf, C.c_void_p), len(s), C.byref(r), C.byref(c), C.byref(ch)) == nat.UWIP_ERR_UNSUPPORTED
    with pytest.raises(uw.UwipError):
        uw.jpeg.info(s)
    for W, H in fc.SIZES:
        for n, f in fc.equality_grey(W, H):
            assert uw.jpeg.info(f.stream) == (H, W, 1), n
        for n, f in fc.equality_colour(W, H):
            assert uw.jpeg.info(f.stream) == (H, W, 3), n
    for n, f in fc.header_streams() + fc.restart_streams():
        assert uw.jpeg.info(f.stream) == (53, 37, 3), n
    # one component: any factors that SOF can hold, 1..4, and no others (libjpeg refuses those too)
    g = fc.equality_grey_to_4()[0][1].stream
    at = g.index(b"\xff\xc0") + 11
    assert g[at] == 0x43 and uw.jpeg.info(g) == (53, 37, 1)
    for n, f in fc.equality_grey_to_4():
        assert uw.jpeg.info(f.stream) == (53, 37, 1), n
    for byte in (0x44, 0x14, 0x41):
        assert uw.jpeg.info(g[:at] + bytes([byte]) + g[at + 1:]) == (53, 37, 1), hex(byte)
    for byte in (0x51, 0x15, 0x01, 0x10, 0x00, 0xF1):
        with pytest.raises(uw.UwipError):
            uw.jpeg.info(g[:at] + bytes([byte]) + g[at + 1:])
        with pytest.raises(Exception):
            js.pil_decode(g[:at] + bytes([byte]) + g[at + 1:], 1)


def test_null_arguments_and_no_device():
    import torch
    import uwimageproc_amd as uw
    import uwimageproc_amd._native as nat
    l = nat.lib()
    b = nat.BatchU8()
    b.rows, b.cols, b.channels, b.frames, b.step, b.frame_stride = 8, 8, 3, 1, 24, 192
    st = (C.c_int32 * 1)(77)
    s = js.pil_stream(js.content(8, 8), 90, 0)
    buf = (C.c_uint8 * len(s)).from_buffer_copy(s)
    ptrs = (C.c_void_p * 1)(C.cast(buf, C.c_void_p))
    sizes = (C.c_size_t * 1)(len(s))
    for fn in (l.uwip_jpeg_decode, l.uwip_jpeg_decode_host):
        assert fn(None, ptrs, sizes, 1, C.byref(b), None, st) != nat.UWIP_OK
        assert fn(None, None, None, 1, None, None, None) != nat.UWIP_OK
    assert st[0] == 77
    r = C.c_int32(5)
    assert l.uwip_jpeg_info(None, 0, C.byref(r), C.byref(r), C.byref(r)) == nat.UWIP_ERR_INVALID and r.value == 5
    assert l.uwip_jpeg_info(C.cast(buf, C.c_void_p), len(s), None, None, None) == nat.UWIP_ERR_INVALID
    with pytest.raises(uw.UwipError):
        uw.jpeg.decode(None, [s])
    if not torch.cuda.is_available():
        with pytest.raises(uw.UwipError):
            uw.Context(0)
