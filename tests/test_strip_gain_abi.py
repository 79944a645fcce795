"""CPU: the gain compensation's entry points that need no device -- the config defaults, the argument checks, and
uwip_strip_gain_solve_host (csrc/strip_core.hpp, the source k_strip_gain_solve runs) against the numpy mirror on the
mirror's own statistics: gq equal, g bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _strip_gain_cases as cases
import _strip_gain_mirror as gm


def _lib():
    import uwimageproc_amd._native as nat
    return nat, nat.lib()


def solve_host(st, seg, cfg=None):
    nat, l = _lib()
    n = len(seg)
    st, seg = np.ascontiguousarray(st, np.uint64), np.ascontiguousarray(seg, np.int32)
    gq, g = np.full((n, 3), -1, np.int32), np.full((n, 3), np.nan)
    rc = l.uwip_strip_gain_solve_host(st.ctypes.data, seg.ctypes.data, n, C.byref(cfg) if cfg is not None else None, gq.ctypes.data, g.ctypes.data)
    return rc, gq, g


def test_config_defaults():
    nat, l = _lib()
    cfg = nat.StripGainConfig()
    assert C.sizeof(cfg) == 32
    assert l.uwip_strip_gain_config_default(C.byref(cfg)) == nat.UWIP_OK
    assert cfg.sigma_n == 10.0 and cfg.sigma_g == np.float32(0.1) and (cfg.lo, cfg.hi, cfg.min_pixels) == (5, 250, 64)
    assert list(cfg.reserved) == [0, 0, 0]
    assert l.uwip_strip_gain_config_default(None) == nat.UWIP_ERR_INVALID
    import uwimageproc_amd.strip as strip
    assert strip.GAIN == 0x100 and not strip.GAIN & 3


def test_null_handles_are_refused():
    nat, l = _lib()
    gq = np.full((2, 3), 4096, np.int32)
    assert l.uwip_strip_gains(None, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_gain_values(None, gq.ctypes.data, None, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_set_gains(None, gq.ctypes.data) == nat.UWIP_ERR_INVALID
    seg = np.zeros(2, np.int32)
    assert l.uwip_strip_gain_solve_host(None, seg.ctypes.data, 2, None, gq.ctypes.data, None) == nat.UWIP_ERR_INVALID
    st = np.zeros((2, 7), np.uint64)
    assert l.uwip_strip_gain_solve_host(st.ctypes.data, None, 2, None, gq.ctypes.data, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_gain_solve_host(st.ctypes.data, seg.ctypes.data, -1, None, gq.ctypes.data, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_gain_solve_host(None, None, 0, None, None, None) == nat.UWIP_OK


@pytest.mark.parametrize("field,value", [("sigma_n", 0.0), ("sigma_n", -1.0), ("sigma_g", 0.0), ("sigma_g", -0.1), ("sigma_g", float("nan")),
                                         ("lo", 251), ("lo", -1), ("hi", 256), ("hi", 4), ("min_pixels", 0), ("min_pixels", -5)])
def test_invalid_configurations_are_refused(field, value):
    nat, l = _lib()
    cfg = nat.StripGainConfig()
    l.uwip_strip_gain_config_default(C.byref(cfg))
    assert solve_host(np.zeros((2, 7), np.uint64), np.zeros(2, np.int32), cfg)[0] == nat.UWIP_OK
    setattr(cfg, field, value)
    assert solve_host(np.zeros((2, 7), np.uint64), np.zeros(2, np.int32), cfg)[0] == nat.UWIP_ERR_INVALID


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_solve_host_equals_the_mirror(name):
    nat, l = _lib()
    _, ch, st, gq, g = cases.expected(name)
    rc, hq, hg = solve_host(st, ch["seg"])
    assert rc == nat.UWIP_OK and np.array_equal(hq, gq)
    assert np.array_equal(hg.view(np.uint64), g.view(np.uint64))
    # and with another configuration, so that the configuration is seen to arrive
    cfg = nat.StripGainConfig()
    l.uwip_strip_gain_config_default(C.byref(cfg))
    cfg.sigma_n, cfg.sigma_g, cfg.min_pixels = 7.5, 1.0, 1000
    eq, eg = gm.solve(st, ch["seg"], sigma_n=7.5, sigma_g=1.0, min_pixels=1000)
    rc, hq, hg = solve_host(st, ch["seg"], cfg)
    assert rc == nat.UWIP_OK and np.array_equal(hq, eq) and np.array_equal(hg.view(np.uint64), eg.view(np.uint64))
    assert not np.array_equal(eq, gq)
