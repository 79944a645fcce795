"""GPU: the strip's gain compensation (uwip_strip_gains, uwip_strip_render with UWIP_STRIP_GAIN; csrc/strip.hip) against the
numpy mirror (tests/_strip_gain_mirror.py), exactly.

Cases A, C, D and E (tests/_strip_gain_cases.py) inject the homographies, so the statistics, the solve and the gained render
are compared without the matcher; the end-to-end test runs the matcher on a synthetic stream whose frames were given known
gains and asserts only what does not depend on the matched homographies' last bits."""
import numpy as np
import pytest
import torch

import _strip_gain_cases as cases
import _strip_gain_mirror as gm
import _strip_mirror as sm
from _layouts import LAYOUTS, assert_only_frames_written, place, place_like
from uwimageproc_amd import Strip, UwipError, synth

pytestmark = pytest.mark.gpu
MODES = (("feather", sm.FEATHER), ("first", sm.FIRST), ("last", sm.LAST))
FILL = cases.FILL


def injected_strip(ctx, frames_view, H, ratio, kw, per_add):
    n, h, w = frames_view.shape[:3]
    fields = {"max_canvas_rows": kw["max_rows"], "max_canvas_cols": kw["max_cols"], "max_scale": kw["max_scale"]} if kw else {}
    s = Strip(ctx, h, w, batch=per_add, max_frames=n, **fields)
    dH, dr = torch.from_numpy(np.ascontiguousarray(H)).cuda(), torch.from_numpy(np.ascontiguousarray(ratio)).cuda()
    for k in range(0, n, per_add):
        s.add(frames_view[k:k + per_add], dH[k:k + per_add].contiguous(), dr[k:k + per_add].contiguous())
    return s


def renders(s, nseg, gain):
    return {(si, m): tuple(t.cpu().numpy() for t in s.render(si, name, FILL, cover=True, gain=gain)) for si in range(nseg) for name, m in MODES}


@pytest.mark.parametrize("name", ["a", "c", "d", "e"])
def test_stats_gains_and_gained_renders_equal_the_mirror(ctx, name):
    (frames, H, ratio, kw), ch, st, gq, g = cases.expected(name)
    s = injected_strip(ctx, torch.from_numpy(np.array(frames)).cuda(), H, ratio, kw, per_add=5)
    assert [tuple(x) for x in s.layout()] == ch["segs"]
    plain = renders(s, len(ch["segs"]), gain=False)
    s.gains()
    v = s.gain_values()
    assert np.array_equal(v["stats"], st)
    assert np.array_equal(v["gq"], gq)
    assert np.array_equal(v["g"].view(np.uint64), g.view(np.uint64))             # bit for bit
    for k in range(len(frames)):                                                 # a pair across a break: all-zero statistics
        if k == 0 or ch["seg"][k] != ch["seg"][k - 1]:
            assert not v["stats"][k].any()
    if name == "e":
        assert int(v["stats"][1][4:].max()) > 2 ** 32
    exp = cases.expected_render(name)
    for key, (canvas, cover) in renders(s, len(ch["segs"]), gain=True).items():
        assert int((canvas != exp[key][0]).sum()) == 0 and int((cover != exp[key][1]).sum()) == 0, key
    # the ungained renders are what they were before the gains were computed
    for key, (canvas, cover) in renders(s, len(ch["segs"]), gain=False).items():
        assert np.array_equal(canvas, plain[key][0]) and np.array_equal(cover, plain[key][1]), key
    assert any(not np.array_equal(plain[key][0], exp[key][0]) for key in plain) or name == "e"
    s.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_gained_render_in_every_layout(ctx, layout):
    """Case A with frames and canvas in each layout: the three write-out bodies of the gained kernel, nothing written outside."""
    (frames, H, ratio, kw), ch, st, gq, g = cases.expected("a")
    exp = cases.expected_render("a")
    _, _, _, _, rows, cols = ch["segs"][0]
    fbuf, fview = place(frames, layout, "cuda")
    before = fbuf.clone()
    s = injected_strip(ctx, fview, H, ratio, kw, per_add=3)
    s.layout()
    s.gains()
    assert np.array_equal(s.gain_values()["gq"], gq)
    for name, m in MODES:
        cbuf, cview = place_like((1, rows, cols, 3), layout, "cuda")
        vbuf, vview = place_like((1, rows, cols), "packed", "cuda")
        canvas, cover = s.render(0, name, FILL, cover=vview[0], out=cview[0], gain=True)
        assert int((canvas.cpu().numpy() != exp[(0, m)][0]).sum()) == 0, name
        assert int((cover.cpu().numpy() != exp[(0, m)][1]).sum()) == 0, name
        assert_only_frames_written(cbuf, cview)
        assert_only_frames_written(vbuf, vview)
    assert_only_frames_written(fbuf, fview, before=before)
    s.close()


@pytest.mark.parametrize("value", [1024, 4096, 16384])
def test_injected_gains(ctx, value):
    """Every gain at the smallest, the unit and the largest value: 16384 saturates case D's pixels at 255, 4096 is the
    ungained render."""
    (frames, H, ratio, kw), ch, _, _, _ = cases.expected("d")
    exp = cases.expected_render("d", value)
    s = injected_strip(ctx, torch.from_numpy(np.array(frames)).cuda(), H, ratio, kw, per_add=10)
    s.layout()
    s.set_gains(np.full((len(frames), 3), value, np.int32))
    v = s.gain_values()
    assert (v["gq"] == value).all() and (v["g"] == value / 4096.0).all() and not v["stats"].any()
    got = renders(s, len(ch["segs"]), gain=True)
    for key in got:
        assert np.array_equal(got[key][0], exp[key][0]) and np.array_equal(got[key][1], exp[key][1]), key
    if value == 16384:
        assert (exp[(0, sm.LAST)][0] == 255).sum() > 1000
    if value == 4096:
        plain = renders(s, len(ch["segs"]), gain=False)
        assert all(np.array_equal(plain[key][0], got[key][0]) for key in got)
    with pytest.raises(UwipError):
        s.set_gains(np.full((len(frames), 3), 1023, np.int32))
    with pytest.raises(UwipError):
        s.set_gains(np.full((len(frames), 3), 16385, np.int32))
    s.close()


def test_error_rules(ctx):
    (frames, H, ratio, kw), ch, _, gq, _ = cases.expected("a")
    d = torch.from_numpy(np.array(frames)).cuda()
    dH, dr = torch.from_numpy(np.ascontiguousarray(H)).cuda(), torch.from_numpy(np.ascontiguousarray(ratio)).cuda()
    s = Strip(ctx, 37, 53, batch=8, max_frames=9)
    with pytest.raises(UwipError):
        s.gains()                                                # an empty strip
    s.add(d, dH, dr)
    with pytest.raises(UwipError) as e:
        s.gains()                                                # before a layout
    assert "uwip_strip_layout" in str(e.value)
    with pytest.raises(UwipError):
        s.set_gains(np.full((8, 3), 4096, np.int32))
    s.layout()
    with pytest.raises(UwipError) as e:
        s.render(0, gain=True)                                   # a layout, but no gains yet
    assert "UWIP_STRIP_GAIN" in str(e.value)
    with pytest.raises(UwipError):
        s.gain_values()
    for bad in ({"sigma_n": 0.0}, {"sigma_g": -1.0}, {"lo": 200, "hi": 100}, {"hi": 256}, {"lo": -1}, {"min_pixels": 0}):
        with pytest.raises(UwipError):
            s.gains(**bad)
    with pytest.raises(UwipError):
        s.render(0, gain=True)                                   # the refused calls left no gains behind
    s.gains()
    assert np.array_equal(s.gain_values()["gq"], gq)
    s.render(0, gain=True)
    s.layout()                                                   # the same layout again: the gains stay
    s.render(0, gain=True)
    import ctypes as C
    from uwimageproc_amd import batch_of
    out = torch.empty((s.segments[0].rows, s.segments[0].cols, 3), dtype=torch.uint8, device="cuda")
    b = batch_of(out)
    for mode in (3, 0x100 | 3, 0x200, 0x300, 4):                 # every other bit above the three modes stays invalid
        assert s._l.uwip_strip_render(s._h, 0, mode, None, C.byref(b), None) != 0, mode
    s.add(d[:1], dH[:1].contiguous(), dr[:1].contiguous())       # an add drops the gains
    s.layout()
    with pytest.raises(UwipError):
        s.render(0, gain=True)
    s.gains()
    s.render(0, gain=True)
    s.reset()                                                    # so does a reset
    s.add(d, dH, dr)
    s.layout()
    with pytest.raises(UwipError):
        s.render(0, gain=True)
    s.render(0)
    s.close()


def test_end_to_end_stream(ctx):
    """Six frames of a translating camera, each times a gain of its own, through detect and match: gains succeeds, every gq
    is in range, and the ungained render is what it was."""
    n, rows, cols = 6, 360, 640
    frames = synth.uw_stream(0, n, rows, cols, step_frac=0.2).astype(np.float64)
    gains = np.random.default_rng(4).uniform(0.8, 1.25, (n, 1, 1, 3))
    d = torch.from_numpy(np.clip(np.floor(frames * gains + 0.5), 0, 255).astype(np.uint8)).cuda()
    s = Strip(ctx, rows, cols, batch=4, max_frames=n)
    s.add(d[:4])
    s.add(d[4:])
    segs = s.layout()
    before = [s.render(i, "feather").cpu().numpy() for i in range(len(segs))]
    s.gains()
    v = s.gain_values()
    assert v["gq"].shape == (n, 3) and (v["gq"] >= 1024).all() and (v["gq"] <= 16384).all() and np.isfinite(v["g"]).all()
    for i in range(len(segs)):
        assert np.array_equal(s.render(i, "feather").cpu().numpy(), before[i])
        assert s.render(i, "feather", gain=True).shape == before[i].shape
    s.close()
