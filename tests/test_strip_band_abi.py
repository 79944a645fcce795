"""CPU: uwip_strip_stack_host -- the stack of csrc/strip_core.hpp, the source k_strip_stack runs -- equals the numpy mirror
(tests/_strip_band_mirror.py) byte for byte, and refuses what the header says it refuses.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

import _strip_band_cases as cases
import _strip_band_mirror as bm
import uwimageproc_amd._native as nat


def stack_host(frame, levels):
    h, w = frame.shape[:2]
    out = np.full((levels, h, w, 3), 0xA5, np.uint8)
    rc = nat.lib().uwip_strip_stack_host(np.ascontiguousarray(frame).ctypes.data, w, h, levels, out.ctypes.data)
    assert rc == nat.UWIP_OK
    return out


@pytest.mark.parametrize("w,h", cases.STACK_SIZES)
def test_stack_host_equals_the_mirror(w, h):
    f = cases.stack_frame(w, h)
    assert np.array_equal(stack_host(f, 4), bm.stack(f, 4))
    for levels in (1, 2, 3):                                 # fewer levels are the first ones, and nothing is written behind them
        buf = np.full((4, h, w, 3), 0xA5, np.uint8)
        assert nat.lib().uwip_strip_stack_host(f.ctypes.data, w, h, levels, buf.ctypes.data) == nat.UWIP_OK
        assert np.array_equal(buf[:levels], bm.stack(f, levels)) and (buf[levels:] == 0xA5).all()


def test_one_pixel_and_one_row():
    for w, h in ((1, 1), (1, 9), (9, 1)):
        f = cases.stack_frame(w, h)
        assert np.array_equal(stack_host(f, 4), bm.stack(f, 4))


def test_defaults():
    c = nat.StripBandsConfig()
    c.levels = -1
    assert nat.lib().uwip_strip_bands_config_default(C.byref(c)) == nat.UWIP_OK
    assert c.levels == 4 and list(c.ramp) == [1, 2, 4, 8] and list(c.reserved) == [0, 0, 0]
    assert C.sizeof(nat.StripBandsConfig) == 32
    assert nat.lib().uwip_strip_bands_config_default(None) == nat.UWIP_ERR_INVALID


def test_error_rules():
    l = nat.lib()
    f = cases.stack_frame(5, 7)
    out = np.full((4, 7, 5, 3), 0xA5, np.uint8)
    p, o = f.ctypes.data, out.ctypes.data
    for args in ((None, 5, 7, 4, o), (p, 5, 7, 4, None), (p, 0, 7, 4, o), (p, 5, 0, 4, o), (p, -1, 7, 4, o), (p, 32769, 7, 4, o),
                 (p, 5, 32769, 4, o), (p, 5, 7, 0, o), (p, 5, 7, 5, o), (p, 5, 7, -1, o)):
        assert l.uwip_strip_stack_host(*args) == nat.UWIP_ERR_INVALID, args
    assert (out == 0xA5).all()                               # a refused call writes nothing
    assert l.uwip_strip_stack_host(p, 5, 7, 4, o) == nat.UWIP_OK
    assert l.uwip_strip_bands(None, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_band_level(None, 0, 1, o) == nat.UWIP_ERR_INVALID
