"""CPU: the strip mosaic's entry points that need no device -- the config defaults, the argument checks, and
uwip_strip_chain_host (csrc/strip_core.hpp, the source k_strip_chain runs) against the numpy mirror, bit for bit."""
import ctypes as C

import numpy as np

import _strip_cases as cases
import _strip_mirror as sm


def _lib():
    import uwimageproc_amd._native as nat
    return nat, nat.lib()


def test_config_defaults():
    nat, l = _lib()
    cfg = nat.StripConfig()
    assert l.uwip_strip_config_default(C.byref(cfg), 360, 640) == nat.UWIP_OK
    assert (cfg.rows, cfg.cols, cfg.max_canvas_rows, cfg.max_canvas_cols) == (360, 640, 16384, 16384)
    assert cfg.max_scale == 4.0 and cfg.seed == 1 and cfg.detect_flags == 0 and cfg.match_flags == 0
    assert cfg.batch >= 1 and cfg.max_frames >= cfg.batch and cfg.videoWidth == 0 and cfg.videoHeight == 0
    assert C.sizeof(nat.StripSegment) == 32 and C.sizeof(nat.StripConfig) == 48
    assert l.uwip_strip_config_default(None, 360, 640) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_config_default(C.byref(cfg), 0, 640) == nat.UWIP_ERR_INVALID


def test_argument_checks_without_device():
    nat, l = _lib()
    cfg = nat.StripConfig()
    l.uwip_strip_config_default(C.byref(cfg), 37, 53)
    h, n = C.c_void_p(), C.c_int(7)
    segs = (nat.StripSegment * 2)()
    canvas = nat.BatchU8(None, 159, 159 * 38, 38, 53, 3, 1)       # not a segment's geometry, and no strip to hold one
    assert l.uwip_strip_create(None, C.byref(cfg), C.byref(h)) == nat.UWIP_ERR_INVALID and not h.value
    assert l.uwip_strip_add(None, C.byref(canvas), None, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_layout(None, segs, 2, C.byref(n)) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_transforms(None, None, None, None, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_render(None, 0, 0, None, C.byref(canvas), None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_reset(None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_count(None, C.byref(n)) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_destroy(None) == nat.UWIP_OK
    assert l.uwip_strip_last_error(None) == b"null strip"
    # the host chain: cap < 0, a cap without room, no output count, a canvas limit smaller than a frame
    H, r = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (2, 1)), np.full(2, 0.5, np.float32)
    args = lambda **k: [k.get("w", 53), 37, 16384, k.get("max_cols", 16384), 4.0, H.ctypes.data, r.ctypes.data, 2, None, None, None, None]
    assert l.uwip_strip_chain_host(*args(), segs, -1, C.byref(n)) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_chain_host(*args(), None, 1, C.byref(n)) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_chain_host(*args(), segs, 2, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_chain_host(*args(max_cols=52), segs, 2, C.byref(n)) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_chain_host(*args(w=1), segs, 2, C.byref(n)) == nat.UWIP_ERR_INVALID
    assert l.uwip_strip_chain_host(*args(), segs, 2, C.byref(n)) == nat.UWIP_OK and n.value == 1


def test_chain_host_equals_the_mirror_on_case_c():
    nat, l = _lib()
    _, H, ratio, kw = cases.case_c()
    exp = sm.chain(H, ratio, 53, 37, **kw)
    assert tuple(s[0] for s in exp["segs"]) == cases.C_STARTS
    got = cases.chain_host(H, ratio, 53, 37, **kw)
    cases.assert_chain_equal(got, exp)
    few = cases.chain_host(H, ratio, 53, 37, cap=2, **kw)       # a short list: the first two, and the full count
    assert few["segs"] == exp["segs"][:2] and few["n_segs"] == len(exp["segs"])


def test_chain_host_equals_the_mirror_on_cases_a_and_b():
    nat, l = _lib()
    for (_, H, ratio, kw), (w, h) in ((cases.case_a(), (53, 37)), (cases.case_b(), (9, 7)), (cases.case_b(identical=True), (9, 7))):
        cases.assert_chain_equal(cases.chain_host(H, ratio, w, h, **kw), sm.chain(H, ratio, w, h, **kw))
