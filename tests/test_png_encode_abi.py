"""CPU: the device PNG encoder's entry points are declared, exported and bound; uwip_png_bound is a host-pure bound that covers
a stored-only encoding; without a device the encoder fails with UWIP_ERR_HIP instead of falling back."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uwip_png_bound", "uwip_png_chunk_bytes", "uwip_png_encode", "uwip_png_encode_host")


def test_symbols_declared_exported_and_bound():
    import uwimageproc_amd._native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uwip.h")).read(), flags=re.S)
    l = C.CDLL(nat.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(l, n), n
        assert n in nat.SIGNATURES, n
    nat.lib()


def test_bound_is_zero_for_bad_geometries_and_monotone():
    import uwimageproc_amd as uw
    assert uw.png.chunk_bytes() == 32768
    for bad in ((0, 8, 3), (8, 0, 1), (8, 8, 2), (8, 8, 4), (65536, 8, 1), (8, 65536, 3), (-1, 8, 1)):
        assert uw.png.bound(*bad) == 0, bad
    assert uw.png.bound(65535, 65535, 3) > 65535 * 65535 * 3
    for ch in (1, 3):
        prev_r = 0
        for rows in (1, 2, 7, 97, 270, 1080, 2160, 65535):
            prev_c = 0
            for cols in (1, 5, 113, 333, 1920, 3840, 65535):
                b = uw.png.bound(rows, cols, ch)
                assert b > prev_c, (rows, cols, ch)
                prev_c = b
            assert prev_c > prev_r
            prev_r = prev_c


def _stored_only_size(rows, cols, ch, chunk):
    """Length of a PNG whose zlib stream holds stored blocks only, laid out as the header comment of uwip_png_bound has it."""
    filtered = rows * (1 + cols * ch)
    nch = -(-filtered // chunk)
    idats = sum(12 + (2 if c == 0 else 0) + 5 + min(chunk, filtered - c * chunk) + (5 if c + 1 < nch else 0) for c in range(nch))
    return 8 + 25 + idats + (12 + 4) + 12


def test_bound_covers_a_stored_only_encoding():
    import uwimageproc_amd as uw
    chunk = uw.png.chunk_bytes()
    for shape in ((1, 1, 1), (1, 1, 3), (1, 300, 1), (300, 1, 1), (5, 7, 3), (97, 113, 3), (200, 333, 1), (1080, 1920, 3)):
        s = _stored_only_size(*shape, chunk)
        assert s <= uw.png.bound(*shape) <= s + 8, shape          # and it is tight: the last chunk has no empty block


def test_no_cpu_fallback_without_device():
    import torch
    import uwimageproc_amd as uw
    import uwimageproc_amd._native as nat
    l = nat.lib()
    b = nat.BatchU8()
    b.rows, b.cols, b.channels, b.frames, b.step, b.frame_stride = 8, 8, 1, 1, 8, 64
    want = nat.UWIP_ERR_INVALID if torch.cuda.is_available() else nat.UWIP_ERR_HIP     # with a device a null context is a bad argument
    assert l.uwip_png_encode(None, C.byref(b), -1, None, 0, None) == want
    assert l.uwip_png_encode_host(None, C.byref(b), -1, None, 0, None) == want
    with pytest.raises(uw.UwipError):
        uw.png.encode(None, torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(uw.UwipError):
            uw.Context(0)
