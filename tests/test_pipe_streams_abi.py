"""CPU: the streams entries of the pipe (uwip_pipe_streams*, uwip_pipe_step_streams, uwip_pipe_collect; include/uwip.h) are
declared, exported and bound, their configuration defaults are what the header says, null handles and null arguments are
refused without touching a device, and without a device there is no pipe to give them: no fallback.  The refusals that need a
pipe (n != frames, UWIP_EMIT_KEYFRAMES without key-frame mode, depth < 2, a bad format) are in test_pipe_streams_gpu.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uwip_pipe_streams_config_default", "uwip_pipe_streams", "uwip_pipe_step_streams", "uwip_pipe_collect", "uwip_pipe_result_params")


def test_symbols_declared_exported_and_bound():
    import uwimageproc_amd._native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uwip.h")).read(), flags=re.S)
    l = C.CDLL(nat.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(l, n), n
        assert n in nat.SIGNATURES, n
    nat.lib()
    for macro, v in (("UWIP_STREAM_JPEG", 0), ("UWIP_STREAM_PNG", 1), ("UWIP_EMIT_ALL", 0), ("UWIP_EMIT_KEYFRAMES", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, v), text), macro


def test_config_defaults_and_layout():
    import uwimageproc_amd._native as nat
    from uwimageproc_amd import pipeline as pl
    l = nat.lib()
    sc = nat.PipeStreamsConfig()
    C.memset(C.byref(sc), 0xAB, C.sizeof(sc))
    assert l.uwip_pipe_streams_config_default(C.byref(sc)) == nat.UWIP_OK
    assert (sc.format, sc.quality, sc.png_filter, sc.emit, sc.slot_bytes, sc.depth, sc.reserved) == (pl.STREAM_JPEG, 95, -1, pl.EMIT_ALL, 0, 2, 0)
    assert l.uwip_pipe_streams_config_default(None) == nat.UWIP_ERR_INVALID
    assert C.sizeof(nat.PipeStreamsConfig) == 32 and C.sizeof(nat.StreamOut) == 24           # the header's structs
    assert (nat.StreamOut.index.offset, nat.StreamOut.row_id.offset, nat.StreamOut.size.offset, nat.StreamOut.offset.offset) == (0, 4, 8, 16)


def test_null_handles_and_arguments_are_refused():
    import uwimageproc_amd._native as nat
    l = nat.lib()
    sc = nat.PipeStreamsConfig()
    l.uwip_pipe_streams_config_default(C.byref(sc))
    t = C.c_uint64(7)
    n = C.c_int(5)
    need = C.c_size_t(9)
    status = (C.c_int32 * 4)()
    outs = (nat.StreamOut * 5)()
    ptrs = (C.c_void_p * 4)()
    sizes = (C.c_size_t * 4)()
    assert l.uwip_pipe_streams(None, C.byref(sc)) == nat.UWIP_ERR_INVALID
    assert l.uwip_pipe_streams(None, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_pipe_step_streams(None, ptrs, sizes, 4, C.byref(t)) == nat.UWIP_ERR_INVALID and t.value == 7
    assert l.uwip_pipe_step_streams(None, None, None, 4, None) == nat.UWIP_ERR_INVALID
    assert l.uwip_pipe_collect(None, 1, status, None, outs, 5, C.byref(n), None, 0, C.byref(need)) == nat.UWIP_ERR_INVALID
    assert (n.value, need.value) == (5, 9)                   # a null pipe: nothing is touched
    assert l.uwip_pipe_result_params(None, 1, status, status) == nat.UWIP_ERR_INVALID


def test_no_pipe_without_a_device():
    import torch
    import uwimageproc_amd as uw
    import uwimageproc_amd._native as nat
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    l = nat.lib()
    h = C.c_void_p()
    assert l.uwip_ctx_create(0, None, C.byref(h)) == nat.UWIP_ERR_HIP and not h.value        # no context, hence no pipe
    with pytest.raises(uw.UwipError) as e:
        uw.Context(0)
    assert e.value.code == nat.UWIP_ERR_HIP
