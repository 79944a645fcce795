"""GPU: the strip's seam finding (uwip_strip_seams, uwip_strip_set_seams, uwip_strip_render with UWIP_STRIP_SEAM; csrc/strip.hip)
against the numpy mirror (tests/_strip_seam_mirror.py), exactly.

The cases of tests/_strip_seam_cases.py inject the homographies, so the seams and the render are compared without the matcher;
the end-to-end test runs the matcher on a synthetic stream and feeds the mirror the device's own transforms and gains."""
import ctypes as C

import numpy as np
import pytest
import torch

import _strip_gain_mirror as gm
import _strip_mirror as sm
import _strip_seam_cases as cases
import _strip_seam_mirror as mm
from _layouts import LAYOUTS, assert_only_frames_written, place, place_like
from uwimageproc_amd import Strip, UwipError, batch_of, synth
from uwimageproc_amd import videostrip as vs

pytestmark = pytest.mark.gpu
FILL = cases.FILL


def injected_strip(ctx, frames_view, H, ratio, kw, per_add):
    n, h, w = frames_view.shape[:3]
    fields = {"max_canvas_rows": kw["max_rows"], "max_canvas_cols": kw["max_cols"], "max_scale": kw["max_scale"]} if kw else {}
    s = Strip(ctx, h, w, batch=per_add, max_frames=n, **fields)
    dH, dr = torch.from_numpy(np.ascontiguousarray(H)).cuda(), torch.from_numpy(np.ascontiguousarray(ratio)).cuda()
    for k in range(0, n, per_add):
        s.add(frames_view[k:k + per_add], dH[k:k + per_add].contiguous(), dr[k:k + per_add].contiguous())
    return s


def strip_of(ctx, name, per_add=16, frames_view=None):
    (frames, H, ratio, kw), ch = cases.expected(name)[:2]
    s = injected_strip(ctx, torch.from_numpy(np.array(frames)).cuda() if frames_view is None else frames_view, H, ratio, kw, per_add)
    assert [tuple(x) for x in s.layout()] == ch["segs"]
    return s


def assert_seams(s, seam, ori, total):
    v = s.seam_values()
    assert np.array_equal(v["orient"], ori)
    assert np.array_equal(v["seam"], seam), np.nonzero((v["seam"] != seam).any(axis=1))[0][:10]
    assert np.array_equal(v["total"], total)


@pytest.mark.parametrize("name", ["a", "c", "d", "f", "g", "s", "ow", "oh", "l"])
def test_seams_and_renders_equal_the_mirror_in_every_layout(ctx, name):
    (frames, _, _, _), ch, gq, seam, ori, total, costs = cases.expected(name)
    exp = cases.expected_render(name)
    gained = gq is not None
    for layout in LAYOUTS:
        fbuf, fview = place(frames, layout, "cuda")
        before = fbuf.clone()
        s = strip_of(ctx, name, per_add=7, frames_view=fview)
        if gained:
            s.gains()
            assert np.array_equal(s.gain_values()["gq"], gq)
        s.seams()
        assert_seams(s, seam, ori, total)
        for si, seg in enumerate(ch["segs"]):
            rows, cols = seg[4], seg[5]
            cbuf, cview = place_like((1, rows, cols, 3), layout, "cuda")
            vbuf, vview = place_like((1, rows, cols), "packed", "cuda")
            canvas, cover = s.render(si, "seam", FILL, cover=vview[0], out=cview[0], gain=gained)
            assert int((canvas.cpu().numpy() != exp[si][0]).sum()) == 0, (si, layout)
            assert int((cover.cpu().numpy() != exp[si][1]).sum()) == 0, (si, layout)
            assert_only_frames_written(cbuf, cview)
            assert_only_frames_written(vbuf, vview)
        assert_only_frames_written(fbuf, fview, before=before)
        s.close()
    if name == "g":
        assert len(costs) > 4 * cases.ROUND and int(exp[0][1].max()) == 9 and len(frames) > 256
    if name == "l":
        assert -(-frames.shape[2] // 16) * frames.shape[1] > cases.BACK_LDS_WORDS
    if name in ("ow", "oh"):
        C = costs[cases.O_NO_OVERLAP]
        assert np.all(C == mm.OUTSIDE) and max(frames.shape[1:3]) > 256 and max(frames.shape[1:3]) % 64
    if name == "f":
        for k, C in costs.items():
            assert int(total[k]) < cases.straight_best(C)[1]


def test_gains_change_the_seams_of_case_d(ctx):
    """The costs are those of the gained frames: the device's totals with and without gains are the mirror's, and differ."""
    _, _, _, seam, ori, total, _ = cases.expected("d")
    _, _, _, seam0, ori0, total0, _ = cases.expected("d", gained=False)
    s = strip_of(ctx, "d")
    s.seams()
    assert_seams(s, seam0, ori0, total0)
    s.gains()
    s.seams()
    assert_seams(s, seam, ori, total)
    assert not np.array_equal(total, total0)
    s.close()


def test_object_that_moved(ctx):
    (frames, _, _, _), ch, _, seam, ori, total, costs = cases.expected("s")
    y0, y1, x0, x1 = cases.S_BLOCK
    s = strip_of(ctx, "s")
    s.seams()
    v = s.seam_values()
    sm1 = v["seam"][1][:96]
    assert np.all(sm1[:y0 - 6] == 11) and np.all(sm1[y1 + 6:] == 11) and np.all(sm1[y0:y1] == 5)
    assert int(v["total"][1]) == 405504 and cases.straight_best(costs[1]) == (5, 1277952)
    canvas = s.render(0, "seam", FILL).cpu().numpy()
    assert np.array_equal(canvas, cases.expected_render("s")[0][0])
    where = (slice(y0, y1), slice(cases.S_PITCH + x0, cases.S_PITCH + x1))
    assert np.all(canvas[where] == np.array(cases.S_VALUE, np.uint8))            # the block is whole
    first = s.render(0, "first", FILL).cpu().numpy()
    assert not np.any(np.all(first[where] == np.array(cases.S_VALUE, np.uint8), axis=2))     # FIRST loses it
    assert not np.array_equal(s.render(0, "feather", FILL).cpu().numpy()[where], canvas[where])
    s.close()


def test_injected_seams_give_last_and_first(ctx):
    for name in ("a", "ow"):
        (frames, _, _, _), ch = cases.expected(name)[:2]
        n, h, w = frames.shape[:3]
        s = strip_of(ctx, name)
        nseg = len(ch["segs"])
        last = [s.render(si, "last", FILL).cpu().numpy() for si in range(nseg)]
        first = [s.render(si, "first", FILL).cpu().numpy() for si in range(nseg)]
        zero = np.zeros((n, max(w, h)), np.int32)
        for o in (0, 1):
            S = w if o else h
            for seam, ori, want in ((zero, o, last), (zero + (S - 1), o | 2, last), (zero + S, o, first)):
                full = np.full_like(zero, -5)                # entries beyond a seam's steps are not read
                full[:, :(h if o else w)] = seam[:, :(h if o else w)]
                s.set_seams(full, np.full(n, ori, np.int32))
                v = s.seam_values()
                assert not v["total"].any()
                for si in range(nseg):
                    assert np.array_equal(s.render(si, "seam", FILL).cpu().numpy(), want[si]), (name, o, ori, si)
        s.close()


def test_identical_frames_give_first(ctx):
    frames = np.repeat(np.random.default_rng(9).integers(0, 256, (1, 20, 30, 3), dtype=np.uint8), 3, axis=0)
    H = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (3, 1))
    s = injected_strip(ctx, torch.from_numpy(frames).cuda(), H, np.full(3, 0.5, np.float32), {}, 3)
    s.layout()
    s.seams()
    assert not s.seam_values()["total"].any()
    assert np.array_equal(s.render(0, "seam", FILL).cpu().numpy(), s.render(0, "first", FILL).cpu().numpy())
    s.close()


def test_other_modes_are_what_they_were(ctx):
    """FEATHER / FIRST / LAST / MULTIBAND, ungained and gained, byte for byte before and after a seams call."""
    ch = cases.expected("d")[1]
    s = strip_of(ctx, "d")
    s.gains()
    s.bands()

    def renders():
        return {(si, m, g): tuple(t.cpu().numpy() for t in s.render(si, m, FILL, cover=True, gain=g))
                for si in range(len(ch["segs"])) for m in ("feather", "first", "last", "multiband") for g in (False, True)}

    before = renders()
    s.seams()
    s.render(0, "seam", FILL, gain=True)
    after = renders()
    for key in before:
        assert np.array_equal(before[key][0], after[key][0]) and np.array_equal(before[key][1], after[key][1]), key
    s.close()


@pytest.mark.parametrize("value", [1024, 4096, 16384])
def test_injected_gains(ctx, value):
    (frames, _, _, _), ch = cases.expected("d")[:2]
    gq = np.full((len(frames), 3), value, np.int32)
    seam, ori, total = mm.seams(frames, ch["G"], ch["Ginv"], ch["seg"], gq)
    s = strip_of(ctx, "d")
    s.set_gains(gq)
    s.seams()
    assert_seams(s, seam, ori, total)
    for si, seg in enumerate(ch["segs"]):
        ec, ev = mm.render(frames, ch["Ginv"], seg, seam, ori, gq, FILL)
        canvas, cover = s.render(si, "seam", FILL, cover=True, gain=True)
        assert np.array_equal(canvas.cpu().numpy(), ec) and np.array_equal(cover.cpu().numpy(), ev), si
        if value == 16384 and si == 0:
            assert (ec == 255).sum() > 1000                   # the saturating multiply is reached
        if value == 4096:
            assert np.array_equal(s.render(si, "seam", FILL).cpu().numpy(), ec)
    s.close()


def test_error_and_dropping_rules(ctx):
    (frames, H, ratio, kw), ch, _, seam, ori, total, _ = cases.expected("a")
    exp = cases.expected_render("a")
    n, h, w = frames.shape[:3]
    d = torch.from_numpy(np.array(frames)).cuda()
    dH, dr = torch.from_numpy(np.ascontiguousarray(H)).cuda(), torch.from_numpy(np.ascontiguousarray(ratio)).cuda()
    s = Strip(ctx, h, w, batch=8, max_frames=9)
    s.add(d, dH, dr)
    with pytest.raises(UwipError) as e:
        s.seams()                                                # no layout
    assert "uwip_strip_layout" in str(e.value)
    with pytest.raises(UwipError):
        s.set_seams(seam, ori)
    s.layout()
    with pytest.raises(UwipError) as e:
        s.render(0, "seam")                                      # no seams yet
    assert "UWIP_STRIP_SEAM" in str(e.value)
    with pytest.raises(UwipError):
        s.seam_values()
    for bad in (-1, 4097):
        with pytest.raises(UwipError):
            s.seams(prior=bad)
        with pytest.raises(UwipError):
            s.render(0, "seam")                                  # a refused call leaves no seams behind
    s.seams()
    assert_seams(s, seam, ori, total)
    assert np.array_equal(s.render(0, "seam", FILL).cpu().numpy(), exp[0][0])
    # a refused injection leaves the seams as they were
    S1, T1 = (w, h) if ori[1] & 1 else (h, w)
    for k, t, val in ((1, 0, S1 + 1), (1, T1 - 1, -1), (n - 1, 3, 1 << 20)):
        bad = seam.copy()
        bad[k, t] = val
        with pytest.raises(UwipError):
            s.set_seams(bad, ori)
    bad_o = ori.copy()
    bad_o[2] = 4
    with pytest.raises(UwipError):
        s.set_seams(seam, bad_o)
    assert s._l.uwip_strip_set_seams(s._h, None, ori.ctypes.data) != 0 and s._l.uwip_strip_set_seams(s._h, seam.ctypes.data, None) != 0
    assert_seams(s, seam, ori, total)
    first_bad = seam.copy()
    first_bad[0] = 12345                                         # a segment's first frame: not read
    s.set_seams(first_bad, ori)
    assert np.array_equal(s.render(0, "seam", FILL).cpu().numpy(), exp[0][0])
    assert s._l.uwip_strip_seams(s._h, None) == 0                # NULL: the defaults
    assert_seams(s, seam, ori, total)
    assert s._l.uwip_strip_seam_values(s._h, None, None, None) == 0              # every pointer may be NULL
    with pytest.raises(UwipError):
        s.render(0, "seam", gain=True)                           # no gains: the gain's own rule holds
    out = torch.empty((s.segments[0].rows, s.segments[0].cols, 3), dtype=torch.uint8, device="cuda")
    b = batch_of(out)
    for mode in (0x200 | 4, 0x104 | 0x200, 5, 4 | 8):
        assert s._l.uwip_strip_render(s._h, 0, mode, None, C.byref(b), None) != 0, mode
    s.layout()                                                   # listing the same layout again keeps the seams
    s.render(0, "seam")
    # gains and injected gains drop them
    s.gains()
    with pytest.raises(UwipError):
        s.render(0, "seam")
    s.seams()
    s.render(0, "seam", gain=True)
    s.set_gains(np.full((n, 3), 4096, np.int32))
    with pytest.raises(UwipError):
        s.render(0, "seam", gain=True)
    s.seams()
    assert np.array_equal(s.render(0, "seam", FILL, gain=True).cpu().numpy(), exp[0][0])
    s.add(d[:1], dH[:1].contiguous(), dr[:1].contiguous())       # an add drops the seams, and so does the layout after it
    with pytest.raises(UwipError):
        s.seam_values()
    s.layout()
    with pytest.raises(UwipError):
        s.render(0, "seam")
    s.seams()
    s.render(0, "seam")
    s.reset()                                                    # so does a reset
    s.add(d, dH, dr)
    s.layout()
    with pytest.raises(UwipError):
        s.render(0, "seam")
    s.render(0)
    s.seams()
    assert np.array_equal(s.render(0, "seam", FILL).cpu().numpy(), exp[0][0])
    s.close()


def test_frames_beyond_1023_are_refused(ctx):
    frames = torch.zeros((2, 8, 1024, 3), dtype=torch.uint8, device="cuda")
    H = np.tile(np.array([1.0, 0, 100.0, 0, 1.0, 0, 0, 0, 1.0]), (2, 1))
    s = injected_strip(ctx, frames, H, np.full(2, 0.5, np.float32), {}, 2)
    s.layout()
    with pytest.raises(UwipError) as e:
        s.seams()
    assert "1023" in str(e.value)
    with pytest.raises(UwipError):
        s.render(0, "seam")
    s.render(0, "last")
    s.close()


def test_end_to_end_stream(ctx):
    """Six frames of a translating camera through detect and match: seams and the SEAM render, ungained and gained, equal the
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
    for gain in (False, True):
        gq = None
        if gain:
            s.gains()
            gq = s.gain_values()["gq"]
        s.seams()
        seam, ori, total = mm.seams(stored, t["G"], t["Ginv"], t["seg"], gq)
        assert_seams(s, seam, ori, total)
        canvas, cover = s.render(0, "seam", FILL, cover=True, gain=gain)
        ec, ev = mm.render(stored, t["Ginv"], tuple(segs[0]), seam, ori, gq, FILL)
        assert np.array_equal(canvas.cpu().numpy(), ec) and np.array_equal(cover.cpu().numpy(), ev), gain
    s.close()
