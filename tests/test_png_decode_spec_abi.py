"""CPU: uwip_png_decode_opts with the found block starts: still 16 bytes with chunk_bytes where the reserved word was, segmented
3 and a chunk_bytes outside its mode or its range are refused, and without a device the decoder still fails with UWIP_ERR_HIP."""
import ctypes as C
import os
import re

import pytest

import _png_decode_streams as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_struct_keeps_its_size_and_offsets():
    import uwimageproc_amd._native as nat
    o = nat.PngDecodeOpts
    assert C.sizeof(o) == 16
    assert (o.segmented.offset, o.chunk_bytes.offset, o.d_counts.offset) == (0, 4, 8)
    assert o.chunk_bytes.size == 4
    text = open(os.path.join(ROOT, "include", "uwip.h")).read()
    body = re.search(r"typedef struct uwip_png_decode_opts \{(.*?)\} uwip_png_decode_opts;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+\*?(\w+);", body) == [("int32_t", "segmented"), ("int32_t", "chunk_bytes"), ("uint64_t", "d_counts")]


def _call(opts):
    import uwimageproc_amd._native as nat
    l = nat.lib()
    b = nat.BatchU8()
    b.rows, b.cols, b.channels, b.frames, b.step, b.frame_stride = 8, 8, 3, 1, 24, 192
    st = (C.c_int32 * 1)(77)
    s = pd.stream(pd.content(8, 8, 3), 0, "l1")
    buf = (C.c_uint8 * len(s)).from_buffer_copy(s)
    ptrs = (C.c_void_p * 1)(C.cast(buf, C.c_void_p))
    sizes = (C.c_size_t * 1)(len(s))
    rcs = [fn(None, ptrs, sizes, 1, C.byref(b), C.byref(opts) if opts is not None else None, st) for fn in (l.uwip_png_decode, l.uwip_png_decode_host)]
    assert st[0] == 77
    assert rcs[0] == rcs[1]
    return rcs[0]


def test_options_out_of_range_are_refused_and_no_device_is_still_an_error():
    import torch
    import uwimageproc_amd._native as nat
    O = nat.PngDecodeOpts
    refused = [O(3, 0, None), O(-2, 0, None), O(1, 4096, None), O(0, 4096, None), O(-1, 4096, None), O(2, 255, None), O(2, (1 << 20) + 1, None),
               O(2, -1, None)]
    for o in refused:
        assert _call(o) == nat.UWIP_ERR_INVALID, (o.segmented, o.chunk_bytes)
    # in range: without a context the call fails because there is no device (or, where there is one, for the missing context)
    for o in (None, O(2, 0, None), O(2, 256, None), O(2, 1 << 20, None), O(1, 0, None), O(0, 0, None), O(-1, 0, None)):
        rc = _call(o)
        assert rc != nat.UWIP_OK
        if not torch.cuda.is_available():
            assert rc == nat.UWIP_ERR_HIP
    assert nat.UWIP_ERR_HIP != nat.UWIP_ERR_INVALID


def test_python_passes_chunk_bytes_and_needs_a_context():
    import inspect
    import uwimageproc_amd as uw
    assert inspect.signature(uw.png.decode).parameters["chunk_bytes"].default == 0
    assert inspect.signature(uw.png.decode_into).parameters["chunk_bytes"].default == 0
    s = pd.stream(pd.content(8, 8, 3), 0, "l1")
    with pytest.raises(uw.UwipError):
        uw.png.decode(None, [s], segmented=2, chunk_bytes=4096)
