"""CPU: the device PNG decoder's entry points are declared, exported and bound; uwip_png_info is the host reader's chunk walk
and IHDR rules with their rejections; without a device (or with null arguments) the decoder fails loudly and touches nothing."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import _png_decode_streams as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uwip_png_info", "uwip_png_decode", "uwip_png_decode_host")


def test_symbols_declared_exported_and_bound():
    import uwimageproc_amd._native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uwip.h")).read(), flags=re.S)
    l = C.CDLL(nat.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(l, n), n
        assert n in nat.SIGNATURES, n
    nat.lib()
    for name, val in (("UWIP_PNG_BAD_STREAM", -1), ("UWIP_PNG_SIZE_MISMATCH", -2)):
        assert re.search(r"#define\s+%s\s+\(%d\)" % (name, val), text), name
    assert C.sizeof(nat.PngDecodeOpts) == 16


def test_info_on_streams_of_each_kind():
    import uwimageproc_amd as uw
    assert (uw.png.BAD_STREAM, uw.png.SIZE_MISMATCH) == (-1, -2)
    for H, W in pd.SHAPES:
        for spp in (1, 2, 3, 4):
            arr = pd.content(H, W, spp)
            want = (H, W, 1 if spp <= 2 else 3)
            assert uw.png.info(pd.stream(arr, "mix", "l6cut1000")) == want
            assert uw.png.info(pd.pil_stream(arr)) == want
            assert uw.png.info(pd.stream(arr, 0, "stored") + b"trailing bytes") == want


def test_info_rejections():
    from PIL import Image
    import uwimageproc_amd as uw
    arr = pd.content(17, 33, 3)
    good = pd.stream(arr, "mix", "l9m9")
    a, b = pd.idat_span(good)
    pal, deep = io.BytesIO(), io.BytesIO()
    Image.fromarray(arr).convert("P").save(pal, format="PNG")
    Image.fromarray(np.arange(17 * 33, dtype=np.uint16).reshape(17, 33) * 100).save(deep, format="PNG")
    adam7 = bytearray(good)
    adam7[good.index(b"IHDR") + 16] = 1
    no_idat = pd.assemble(17, 33, 3, [])
    fdict = bytearray(good)
    fdict[a + 1] |= 0x20
    method = bytearray(good)
    method[a] ^= 0x01
    for bad in (pal.getvalue(), deep.getvalue(), bytes(adam7), no_idat, bytes(fdict), bytes(method), good[:b - 1], good[:32], good[:3], b"",
                b"\xff\xd8\xff\xe0" + bytes(64), pd.SIG + pd.ihdr(0, 33, 3) + good[33:], pd.SIG + pd.ihdr(17, 33, 3, depth=4) + good[33:]):
        with pytest.raises(uw.UwipError):
            uw.png.info(bad)
    # a stream cut behind its last IDAT has lost only IEND: the host reader reads it
    assert uw.png.info(good[:b + 4]) == (17, 33, 3)


def test_null_arguments_and_no_device():
    import torch
    import uwimageproc_amd as uw
    import uwimageproc_amd._native as nat
    l = nat.lib()
    b = nat.BatchU8()
    b.rows, b.cols, b.channels, b.frames, b.step, b.frame_stride = 8, 8, 3, 1, 24, 192
    st = (C.c_int32 * 1)(77)
    s = pd.stream(pd.content(8, 8, 3), 0, "l1")
    buf = (C.c_uint8 * len(s)).from_buffer_copy(s)
    ptrs = (C.c_void_p * 1)(C.cast(buf, C.c_void_p))
    sizes = (C.c_size_t * 1)(len(s))
    for fn in (l.uwip_png_decode, l.uwip_png_decode_host):
        rc = fn(None, ptrs, sizes, 1, C.byref(b), None, st)
        assert rc != nat.UWIP_OK
        if not torch.cuda.is_available():
            assert rc == nat.UWIP_ERR_HIP                      # no device: that, not a quiet host decode
        assert fn(None, None, None, 1, None, None, None) != nat.UWIP_OK
    assert st[0] == 77
    r = C.c_int32(5)
    assert l.uwip_png_info(None, 0, C.byref(r), C.byref(r), C.byref(r)) == nat.UWIP_ERR_INVALID and r.value == 5
    assert l.uwip_png_info(C.cast(buf, C.c_void_p), len(s), None, None, None) == nat.UWIP_ERR_INVALID
    junk = (C.c_uint8 * 64)()
    assert l.uwip_png_info(C.cast(junk, C.c_void_p), 64, C.byref(r), C.byref(r), C.byref(r)) == nat.UWIP_ERR_UNSUPPORTED and r.value == 5
    with pytest.raises(uw.UwipError):
        uw.png.decode(None, [s])
    with pytest.raises(uw.UwipError):
        uw.png.decode_into(None, [s], None)
    if not torch.cuda.is_available():
        with pytest.raises(uw.UwipError):
            uw.Context(0)
