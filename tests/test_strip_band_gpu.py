"""GPU: the strip's multi-band blending (uwip_strip_bands, uwip_strip_render with UWIP_STRIP_MULTIBAND; csrc/strip.hip) against
the numpy mirror (tests/_strip_band_mirror.py), exactly.

The cases of tests/_strip_band_cases.py inject the homographies, so the stacks and the render are compared without the
matcher; the end-to-end test runs the matcher on a synthetic stream and feeds the mirror the device's own transforms."""
import ctypes as C

import numpy as np
import pytest
import torch

import _strip_band_cases as cases
import _strip_band_mirror as bm
import _strip_mirror as sm
from _layouts import LAYOUTS, assert_only_frames_written, place, place_like
from uwimageproc_amd import Strip, UwipError, batch_of, synth
from uwimageproc_amd import videostrip as vs

pytestmark = pytest.mark.gpu
FILL = cases.FILL
OLD_MODES = ("feather", "first", "last")


def injected_strip(ctx, frames_view, H, ratio, kw, per_add):
    n, h, w = frames_view.shape[:3]
    fields = {"max_canvas_rows": kw["max_rows"], "max_canvas_cols": kw["max_cols"], "max_scale": kw["max_scale"]} if kw else {}
    s = Strip(ctx, h, w, batch=per_add, max_frames=n, **fields)
    dH, dr = torch.from_numpy(np.ascontiguousarray(H)).cuda(), torch.from_numpy(np.ascontiguousarray(ratio)).cuda()
    for k in range(0, n, per_add):
        s.add(frames_view[k:k + per_add], dH[k:k + per_add].contiguous(), dr[k:k + per_add].contiguous())
    return s


def strip_of(ctx, name, per_add=16):
    (frames, H, ratio, kw), ch, gq, _ = cases.expected(name)
    s = injected_strip(ctx, torch.from_numpy(np.array(frames)).cuda(), H, ratio, kw, per_add)
    assert [tuple(x) for x in s.layout()] == ch["segs"]
    return s


@pytest.mark.parametrize("w,h", cases.STACK_SIZES)
def test_band_levels_equal_the_mirror_in_every_layout(ctx, w, h):
    frames = np.stack([cases.stack_frame(w, h), cases.stack_frame(w, h)[::-1, ::-1].copy(), cases.stack_frame(h + w, h)[:, :w].copy()])
    exp = np.stack([bm.stack(f, 4) for f in frames], axis=1)
    I = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (3, 1))
    for layout in LAYOUTS:
        fbuf, fview = place(frames, layout, "cuda")
        before = fbuf.clone()
        s = injected_strip(ctx, fview, I, np.full(3, 0.5, np.float32), {}, per_add=2)
        s.bands()
        for k in range(3):
            for l in range(1, 5):
                assert np.array_equal(s.band_level(k, l), exp[l - 1][k]), (layout, k, l)
        s.bands(levels=2, ramp=(3, 5))                       # fewer levels: the first ones again, level 3 is gone
        assert np.array_equal(s.band_level(2, 2), exp[1][2])
        with pytest.raises(UwipError):
            s.band_level(2, 3)
        assert_only_frames_written(fbuf, fview, before=before)
        s.close()


@pytest.mark.parametrize("name", ["a", "c", "d", "f", "g", "h"])
def test_multiband_renders_equal_the_mirror_in_every_layout(ctx, name):
    (frames, _, _, _), ch, gq, _ = cases.expected(name)
    levels, ramp, gained = cases.RENDER[name]
    exp, big = cases.expected_render(name)
    s = strip_of(ctx, name, per_add=7)
    if gained:
        s.gains()
        assert np.array_equal(s.gain_values()["gq"], gq)
    s.bands(levels=levels, ramp=ramp)
    for si, seg in enumerate(ch["segs"]):
        rows, cols = seg[4], seg[5]
        for layout in LAYOUTS:
            cbuf, cview = place_like((1, rows, cols, 3), layout, "cuda")
            vbuf, vview = place_like((1, rows, cols), "packed", "cuda")
            canvas, cover = s.render(si, "multiband", FILL, cover=vview[0], out=cview[0], gain=gained)
            assert int((canvas.cpu().numpy() != exp[si][0]).sum()) == 0, (si, layout)
            assert int((cover.cpu().numpy() != exp[si][1]).sum()) == 0, (si, layout)
            assert_only_frames_written(cbuf, cview)
            assert_only_frames_written(vbuf, vview)
    if name == "h":
        assert big > 2 ** 32
    if name == "g":
        assert int(exp[0][1].max()) == 9 and len(frames) > 256
    s.close()


@pytest.mark.parametrize("levels,ramp", [(1, (3,)), (2, (1, 40)), (3, (2, 2, 4096)), (4, (16, 8, 4, 2))])
def test_levels_and_ramps_on_case_f(ctx, levels, ramp):
    s = strip_of(ctx, "f")
    s.bands(levels=levels, ramp=ramp)
    exp, _ = cases.expected_render("f", levels, ramp)
    canvas, cover = s.render(0, "multiband", FILL, cover=True)
    assert np.array_equal(canvas.cpu().numpy(), exp[0][0]) and np.array_equal(cover.cpu().numpy(), exp[0][1])
    assert not np.array_equal(exp[0][0], cases.expected_render("f")[0][0][0])      # another configuration, another canvas
    s.close()


@pytest.mark.parametrize("value", [1024, 4096, 16384])
def test_injected_gains(ctx, value):
    (frames, _, _, _), ch, _, _ = cases.expected("d")
    exp, _ = cases.expected_render("d", gains=value)
    s = strip_of(ctx, "d")
    s.set_gains(np.full((len(frames), 3), value, np.int32))
    s.bands()
    got = {si: tuple(t.cpu().numpy() for t in s.render(si, "multiband", FILL, cover=True, gain=True)) for si in range(len(ch["segs"]))}
    for si in got:
        assert np.array_equal(got[si][0], exp[si][0]) and np.array_equal(got[si][1], exp[si][1]), si
    if value == 16384:
        assert (exp[0][0] == 255).sum() > 1000                # the saturating multiply is reached
    if value == 4096:
        for si in got:
            assert np.array_equal(s.render(si, "multiband", FILL).cpu().numpy(), got[si][0])
    s.close()


def test_other_modes_are_what_they_were(ctx):
    """FEATHER / FIRST / LAST, ungained and gained, byte for byte before and after a bands call."""
    (frames, _, _, _), ch, _, _ = cases.expected("d")
    s = strip_of(ctx, "d")
    s.gains()

    def renders():
        return {(si, m, g): tuple(t.cpu().numpy() for t in s.render(si, m, FILL, cover=True, gain=g))
                for si in range(len(ch["segs"])) for m in OLD_MODES for g in (False, True)}

    before = renders()
    s.bands()
    s.render(0, "multiband", FILL, gain=True)
    after = renders()
    for key in before:
        assert np.array_equal(before[key][0], after[key][0]) and np.array_equal(before[key][1], after[key][1]), key
    s.close()


def test_error_rules(ctx):
    (frames, H, ratio, kw), ch, _, _ = cases.expected("a")
    exp, _ = cases.expected_render("a")
    d = torch.from_numpy(np.array(frames)).cuda()
    dH, dr = torch.from_numpy(np.ascontiguousarray(H)).cuda(), torch.from_numpy(np.ascontiguousarray(ratio)).cuda()
    s = Strip(ctx, 37, 53, batch=8, max_frames=9)
    with pytest.raises(UwipError) as e:
        s.bands()                                                # no frame
    assert "no frame" in str(e.value)
    s.add(d, dH, dr)
    s.layout()
    with pytest.raises(UwipError) as e:
        s.render(0, "multiband")                                 # no stacks yet
    assert "UWIP_STRIP_MULTIBAND" in str(e.value)
    with pytest.raises(UwipError):
        s.band_level(0, 1)
    for bad in ({"levels": 0}, {"levels": 5}, {"levels": -1}, {"ramp": (0, 2, 4, 8)}, {"ramp": (1, 2, 4, 4097)}, {"ramp": (1, -2, 4, 8)},
                {"levels": 2, "ramp": (1, 0)}):
        with pytest.raises(UwipError):
            s.bands(**bad)
        with pytest.raises(UwipError):
            s.render(0, "multiband")                             # a refused call leaves no stacks behind
    s.bands(levels=2, ramp=(1, 2, 0, -7))                        # ramps beyond the levels are not read
    s.bands()                                                    # after the refused calls a valid one succeeds
    assert np.array_equal(s.render(0, "multiband", FILL).cpu().numpy(), exp[0][0])
    assert s._l.uwip_strip_bands(s._h, None) == 0                # NULL: the defaults
    assert np.array_equal(s.render(0, "multiband", FILL).cpu().numpy(), exp[0][0])
    s.layout()                                                   # a layout keeps the stacks
    s.render(0, "multiband")
    with pytest.raises(UwipError):
        s.render(0, "multiband", gain=True)                      # no gains: the gain's own rule holds
    out = torch.empty((s.segments[0].rows, s.segments[0].cols, 3), dtype=torch.uint8, device="cuda")
    b = batch_of(out)
    for mode in (4, 0x100 | 4, 0x200 | 3, 7):
        assert s._l.uwip_strip_render(s._h, 0, mode, None, C.byref(b), None) != 0, mode
    for bad in ((-1, 1), (8, 1), (0, 0), (0, 5)):
        with pytest.raises(UwipError):
            s.band_level(*bad)
    s.add(d[:1], dH[:1].contiguous(), dr[:1].contiguous())       # an add drops the stacks
    s.layout()
    with pytest.raises(UwipError):
        s.render(0, "multiband")
    with pytest.raises(UwipError):
        s.band_level(0, 1)
    s.bands()
    s.render(0, "multiband")
    s.reset()                                                    # so does a reset
    s.add(d, dH, dr)
    s.layout()
    with pytest.raises(UwipError):
        s.render(0, "multiband")
    s.render(0)
    s.bands()
    assert np.array_equal(s.render(0, "multiband", FILL).cpu().numpy(), exp[0][0])
    s.close()


def test_end_to_end_stream(ctx):
    """Six frames of a translating camera through detect and match: the multiband render, ungained and gained, equals the
    mirror fed with the device's own transforms, stored frames and gains."""
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
    assert stored.shape[1:3] == s.stored_size() == (rows, cols)
    s.gains()
    gq = s.gain_values()["gq"]
    s.bands()
    lv = bm.stacks(stored, 4)
    for k in (0, n - 1):
        assert np.array_equal(s.band_level(k, 4), lv[4][k])
    for gain in (False, True):
        canvas, cover = s.render(0, "multiband", FILL, cover=True, gain=gain)
        ec, ev = bm.render(stored, t["Ginv"], tuple(segs[0]), 4, bm.DEFAULT_RAMP, gq if gain else None, FILL, lv=lv)
        assert np.array_equal(canvas.cpu().numpy(), ec) and np.array_equal(cover.cpu().numpy(), ev), gain
    s.close()
