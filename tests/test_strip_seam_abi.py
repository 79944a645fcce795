"""CPU: the seam entries of the C ABI that need no device -- uwip_strip_seam_path_host (the source k_strip_seam_path steps
through) against the numpy mirror, the defaults, the structure's size, and the error rules: a refused call writes nothing."""
import ctypes as C

import numpy as np
import pytest

import _strip_seam_mirror as mm
import uwimageproc_amd._native as nat


def path_host(cost, steps=None, states=None):
    cost = np.ascontiguousarray(cost, np.uint32)
    T, S = cost.shape if steps is None else (steps, states)
    seam = np.full(max(T, 1) + 1, -7, np.int32)              # one canary behind the steps
    total = C.c_uint64(0xDEADBEEF)
    rc = nat.lib().uwip_strip_seam_path_host(cost.ctypes.data, T, S, seam.ctypes.data, C.byref(total))
    return rc, seam, total.value


def assert_equals_mirror(cost):
    rc, seam, total = path_host(cost)
    T = cost.shape[0]
    want, wtotal = mm.path(cost)
    assert rc == nat.UWIP_OK and seam[T] == -7
    assert np.array_equal(seam[:T], want) and total == wtotal


def test_defaults_and_size():
    assert C.sizeof(nat.StripSeamConfig) == 16
    c = nat.StripSeamConfig(-1, (C.c_int32 * 3)(5, 5, 5))
    assert nat.lib().uwip_strip_seam_config_default(C.byref(c)) == nat.UWIP_OK
    assert c.prior == 1024 and list(c.reserved) == [0, 0, 0]
    assert nat.lib().uwip_strip_seam_config_default(None) == nat.UWIP_ERR_INVALID


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (37, 53), (300, 20), (20, 300), (640, 360)])
@pytest.mark.parametrize("hi", [2, 3, 1 << 22])
def test_path_host_equals_the_mirror(shape, hi):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + hi)
    assert_equals_mirror(rng.integers(0, hi, shape).astype(np.uint32))         # hi 2, 3: ties nearly everywhere


def test_path_host_on_the_largest_total():
    cost = np.full((1023, 3), mm.OUTSIDE, np.uint32)
    rc, seam, total = path_host(cost)
    assert rc == nat.UWIP_OK and total == 1023 * mm.OUTSIDE and 2 ** 32 - 2 ** 23 < total < 2 ** 32
    assert np.all(seam[:1023] == 0)                          # pinned by the ties
    assert_equals_mirror(np.full((3, 1023), mm.OUTSIDE, np.uint32))


def test_path_host_refuses_and_writes_nothing():
    l = nat.lib()
    good = np.ones((4, 5), np.uint32)
    for steps, states in ((0, 5), (4, 0), (-1, 5), (1024, 5), (4, 1024)):
        cost = good if steps * states <= 20 else np.ones((max(steps, 1), max(states, 1)), np.uint32)
        rc, seam, total = path_host(cost, steps, states)
        assert rc == nat.UWIP_ERR_INVALID and np.all(seam == -7) and total == 0xDEADBEEF, (steps, states)
    bad = good.copy()
    bad[3, 4] = mm.OUTSIDE + 1                                # beyond the largest cost: totals could pass 2^32
    rc, seam, total = path_host(bad)
    assert rc == nat.UWIP_ERR_INVALID and np.all(seam == -7) and total == 0xDEADBEEF
    seam, total = np.zeros(4, np.int32), C.c_uint64(0)
    assert l.uwip_strip_seam_path_host(None, 4, 5, seam.ctypes.data, C.byref(total)) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_seam_path_host(good.ctypes.data, 4, 5, None, C.byref(total)) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_seam_path_host(good.ctypes.data, 4, 5, seam.ctypes.data, None) == nat.UWIP_ERR_INVALID


def test_null_strip_is_refused():
    l = nat.lib()
    assert l.uwip_strip_seams(None, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_seam_values(None, None, None, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_set_seams(None, None, None) == nat.UWIP_ERR_INVALID


def test_mode_value():
    import re, os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwip.h")).read()
    assert re.search(r"#define UWIP_STRIP_SEAM\s+4\b", text)
    from uwimageproc_amd.strip import MODES
    assert MODES["seam"] == 4
