"""GPU: the strip mosaic (uwip_strip_*, csrc/strip.hip) against the numpy mirror (tests/_strip_mirror.py), exactly.

Cases A-C (tests/_strip_cases.py) inject the homographies, so chain and render are compared without the matcher; the
end-to-end test runs the matcher on a synthetic stream and feeds the mirror the device's own transforms."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _strip_cases as cases
import _strip_mirror as sm
from _layouts import LAYOUTS, assert_only_frames_written, place, place_like
from uwimageproc_amd import Strip, UwipError, batch_of, synth
from uwimageproc_amd import videostrip as vs

pytestmark = pytest.mark.gpu
MODES = (("feather", sm.FEATHER), ("first", sm.FIRST), ("last", sm.LAST))
FILL = (7, 99, 200)

# End to end: the largest distance, in pixels, between the translation of a chained G_k and the stream's true offset
# k * uw_stream_shift, measured on the MI355X for the frozen stream below.  The test asserts twice
# this; the factor covers later matcher changes only.
E2E_MEASURED_MAX_DEV = 0.3534          # at k = 1; [0, 0.3534, 0.0153, 0.0864, 0.0951, 0.0512] for k = 0..5


@functools.lru_cache(maxsize=None)
def expected(name):
    """The mirror's answer for a case, computed once: (case, chain, {(segment, mode): (canvas, cover)})."""
    case = {"a": cases.case_a, "b": cases.case_b, "b_same": functools.partial(cases.case_b, identical=True), "c": cases.case_c}[name]()
    frames, H, ratio, kw = case
    h, w = frames.shape[1:3]
    ch = sm.chain(H, ratio, w, h, **kw)
    out = {(si, m): sm.render(frames, ch["Ginv"], s, m, FILL) for si, s in enumerate(ch["segs"]) for _, m in MODES}
    return case, ch, out


def injected_strip(ctx, frames_view, H, ratio, kw, per_add):
    n, h, w = frames_view.shape[:3]
    fields = {"max_canvas_rows": kw["max_rows"], "max_canvas_cols": kw["max_cols"], "max_scale": kw["max_scale"]} if kw else {}
    s = Strip(ctx, h, w, batch=per_add, max_frames=n, **fields)
    dH, dr = torch.from_numpy(np.ascontiguousarray(H)).cuda(), torch.from_numpy(np.ascontiguousarray(ratio)).cuda()
    for k in range(0, n, per_add):
        s.add(frames_view[k:k + per_add], dH[k:k + per_add].contiguous(), dr[k:k + per_add].contiguous())
    return s


def assert_chain(s, ch):
    segs = s.layout()
    assert [tuple(g) for g in segs] == ch["segs"]
    cases.assert_chain_equal({**s.transforms(), "segs": [tuple(g) for g in segs]}, ch)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_case_a_every_mode_in_every_layout(ctx, layout):
    """Frames and canvas in each layout: the three write-out bodies, the cover plane, and nothing written outside."""
    (frames, H, ratio, kw), ch, exp = expected("a")
    _, _, _, _, rows, cols = ch["segs"][0]
    assert cols > 2 * cases.TILE_W and rows > 2 * cases.TILE_H and len(ch["segs"]) == 1
    fbuf, fview = place(frames, layout, "cuda")
    before = fbuf.clone()
    s = injected_strip(ctx, fview, H, ratio, kw, per_add=3)
    assert_chain(s, ch)
    for name, m in MODES:
        cbuf, cview = place_like((1, rows, cols, 3), layout, "cuda")
        vbuf, vview = place_like((1, rows, cols), "packed", "cuda")
        canvas, cover = s.render(0, name, FILL, cover=vview[0], out=cview[0])
        ec, ev = exp[(0, m)]
        assert int((canvas.cpu().numpy() != ec).sum()) == 0, name
        assert int((cover.cpu().numpy() != ev).sum()) == 0, name
        assert_only_frames_written(cbuf, cview)
        assert_only_frames_written(vbuf, vview)
    assert_only_frames_written(fbuf, fview, before=before)
    s.close()


@pytest.mark.parametrize("name", ["b", "b_same"])
def test_case_b_more_frames_than_one_cull_chunk(ctx, name):
    (frames, H, ratio, kw), ch, exp = expected(name)
    assert len(frames) > cases.CULL_CHUNK and len(ch["segs"]) == 1
    s = injected_strip(ctx, torch.from_numpy(frames).cuda(), H, ratio, kw, per_add=100)
    assert_chain(s, ch)
    for mname, m in MODES:
        canvas, cover = s.render(0, mname, FILL, cover=True)
        ec, ev = exp[(0, m)]
        assert np.array_equal(canvas.cpu().numpy(), ec) and np.array_equal(cover.cpu().numpy(), ev), mname
    if name == "b_same":
        assert (exp[(0, sm.FEATHER)][1] == 255).all()            # 300 covering frames: the count saturates
    s.close()


def test_case_c_device_chain_equals_host_chain_equals_mirror(ctx):
    (frames, H, ratio, kw), ch, exp = expected("c")
    assert tuple(g[0] for g in ch["segs"]) == cases.C_STARTS
    cases.assert_chain_equal(cases.chain_host(H, ratio, 53, 37, **kw), ch)
    s = injected_strip(ctx, torch.from_numpy(frames).cuda(), H, ratio, kw, per_add=5)
    assert_chain(s, ch)
    for si in range(len(ch["segs"])):
        canvas, cover = s.render(si, "feather", FILL, cover=True)
        ec, ev = exp[(si, sm.FEATHER)]
        assert np.array_equal(canvas.cpu().numpy(), ec) and np.array_equal(cover.cpu().numpy(), ev), si
    s.close()


def test_argument_checks(ctx):
    (frames, H, ratio, kw), ch, _ = expected("c")
    d = torch.from_numpy(frames).cuda()
    s = injected_strip(ctx, d, H, ratio, kw, per_add=12)
    one = torch.from_numpy(np.ascontiguousarray(H[:1])).cuda(), torch.from_numpy(ratio[:1].copy()).cuda()
    with pytest.raises(UwipError):
        s.add(d[:1], *one)                                       # more than max_frames: refused, nothing queued
    assert len(s) == 12
    with pytest.raises(UwipError):
        s.render(0, out=torch.empty((5, 5, 3), dtype=torch.uint8, device="cuda"))      # before any layout
    segs = s.layout()
    with pytest.raises(UwipError):
        s.render(0, out=torch.empty((segs[0].rows + 1, segs[0].cols, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(UwipError):
        s.render(0, out=torch.empty((segs[0].rows, segs[0].cols), dtype=torch.uint8, device="cuda"))       # one channel
    n = C.c_int(0)
    assert s._l.uwip_strip_layout(s._h, None, 0, C.byref(n)) != 0
    s.reset()
    assert len(s) == 0
    b = batch_of(d[:1])
    assert s._l.uwip_strip_add(s._h, C.byref(b), C.c_void_p(one[0].data_ptr()), None) != 0      # H without ratio
    s.add(d[:2], torch.from_numpy(np.ascontiguousarray(H[:2])).cuda(), torch.from_numpy(ratio[:2].copy()).cuda())
    with pytest.raises(UwipError):
        s.add(d[2:3])                                            # a matched frame into an injected strip
    s.close()


def test_end_to_end_stream(ctx):
    """Six frames of a translating camera through detect and match: one segment, the render equals the mirror fed with the
    device's own transforms, and the chained translations follow the stream's true offsets."""
    n, rows, cols = 6, 360, 640
    frames = synth.uw_stream(0, n, rows, cols, step_frac=0.2)
    d = torch.from_numpy(frames).cuda()
    s = Strip(ctx, rows, cols, batch=4, max_frames=n)
    s.add(d[:4])
    s.add(d[4:])
    segs = s.layout()
    assert [(g.first, g.count) for g in segs] == [(0, n)]
    t = s.transforms()
    stored = vs.resize_bgr(ctx, d).cpu().numpy()                 # what the strip keeps: the working-size frames
    assert stored.shape[1:3] == (rows, cols)
    for name, m in (("feather", sm.FEATHER), ("last", sm.LAST)):
        canvas, cover = s.render(0, name, FILL, cover=True)
        ec, ev = sm.render(stored, t["Ginv"], tuple(segs[0]), m, FILL)
        assert np.array_equal(canvas.cpu().numpy(), ec) and np.array_equal(cover.cpu().numpy(), ev), name
    sx, sy = synth.uw_stream_shift(cols, 0.2)
    dev = [float(np.hypot(t["G"][k][2] - k * sx, t["G"][k][5] - k * sy)) for k in range(n)]
    print("strip end to end: deviation of G_k's translation from k * shift, px:", [round(v, 4) for v in dev])
    assert max(d_ / k for k, d_ in enumerate(dev) if k) <= 1.0, "more than a pixel per accumulated pair: a finding, not a tolerance"
    assert max(dev) <= 2.0 * E2E_MEASURED_MAX_DEV
    s.close()


def test_a_strip_that_outlives_its_context_is_dropped_not_destroyed():
    """uwip.h: a strip is bound to its context and is destroyed before it.  The Python objects keep that contract when they
    are closed in the wrong order: closing a Strip whose Context is already closed does not call uwip_strip_destroy with the
    freed context (the context's close has released the device memory; the strip's handle is dropped)."""
    import uwimageproc_amd as uw
    c = uw.Context(0)
    s = Strip(c, 37, 53, batch=2, max_frames=2)
    c.close()
    s.close()
    assert s._h is None
