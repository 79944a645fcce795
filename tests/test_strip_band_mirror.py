"""CPU: known answers of the multi-band mirror (tests/_strip_band_mirror.py) by itself -- the stack on frames whose levels can
be written down, the three exact properties of the render (one covering frame = FIRST, constant frames = FEATHER, identical
frames under the identity = FIRST), the cover plane, the visiting order -- and the seam measure on case F."""
import numpy as np
import pytest

import _strip_band_cases as cases
import _strip_band_mirror as bm
import _strip_gain_mirror as gm
import _strip_mirror as sm

FILL = cases.FILL
# the mirror's values on case F with the defaults; the mode may be retuned down to a quarter of the way
# towards FEATHER, not further
R_MULTIBAND, R_FEATHER = 0.8887, 0.5039


def test_constant_frame_gives_constant_levels():
    f = np.empty((11, 13, 3), np.uint8)
    f[:] = (3, 128, 255)
    lv = bm.stack(f, 4)
    assert lv.shape == (4, 11, 13, 3) and (lv == f[None]).all()


def test_single_peak_gives_the_kernel_at_the_holes():
    f = np.zeros((33, 33, 3), np.uint8)
    f[16, 16] = 255
    k = np.array(bm.K)
    for l in range(4):
        s = 1 << l
        exp = np.zeros((33, 33), np.int64)
        at = 16 + (np.arange(5) - 2) * s                    # s = 8: rows and columns 0 and 32, the frame's border
        exp[np.ix_(at, at)] = (255 * np.outer(k, k) + 128) >> 8
        assert (bm.level(f, s) == exp[..., None]).all(), l
    assert (bm.stack(f, 1)[0] == bm.level(f, 1)).all()


def _one_level(cur, s):
    """the definition, written with explicit loops over the taps (no vector clamp)"""
    h, w = cur.shape[:2]
    out = np.zeros_like(cur)
    for y in range(h):
        for x in range(w):
            acc = np.zeros(3, np.int64)
            for i in range(5):
                yy = min(max(y + (i - 2) * s, 0), h - 1)
                for j in range(5):
                    xx = min(max(x + (j - 2) * s, 0), w - 1)
                    acc += bm.K[i] * bm.K[j] * cur[yy, xx]
            out[y, x] = (acc + 128) >> 8
    return out


def test_stack_equals_the_definition_with_loops():
    f = cases.stack_frame(5, 7)
    lv = bm.stack(f, 4)
    cur = f.astype(np.int64)
    for l in range(4):
        cur = _one_level(cur, 1 << l)
        assert (lv[l] == cur).all(), l


@pytest.mark.parametrize("name", ["a", "c"])
def test_one_covering_frame_equals_first(name):
    (frames, _, _, _), ch, _, _ = cases.expected(name)
    exp, _ = cases.expected_render(name)
    for si, s in enumerate(ch["segs"]):
        first, cover = sm.render(frames, ch["Ginv"], s, sm.FIRST, FILL)
        canvas, cov = exp[si]
        assert np.array_equal(cov, cover)                        # the cover plane is that of the other modes
        assert (cover == 1).any() and (canvas[cover == 1] == first[cover == 1]).all()
        assert (canvas[cover == 0] == np.array(FILL, np.uint8)).all()
        assert (cover >= 2).sum() == 0 or (canvas[cover >= 2] != first[cover >= 2]).any()


@pytest.mark.parametrize("name", ["a", "c"])
@pytest.mark.parametrize("gained", [False, True])
def test_constant_frames_give_the_feather_canvas(name, gained):
    (frames, _, _, _), ch, _, _ = cases.expected(name)
    rng = np.random.default_rng(7)
    const = np.empty_like(frames)
    const[:] = rng.integers(0, 256, (len(frames), 1, 1, 3), dtype=np.uint8)
    gq = rng.integers(1024, 16385, (len(frames), 3)).astype(np.int32) if gained else None
    for s in ch["segs"]:
        got, cov = bm.render(const, ch["Ginv"], s, 4, bm.DEFAULT_RAMP, gq, FILL)
        if gained:
            exp, ecov = gm.render_gain(const, ch["Ginv"], s, gq, sm.FEATHER, FILL)
        else:
            exp, ecov = sm.render(const, ch["Ginv"], s, sm.FEATHER, FILL)
        assert np.array_equal(got, exp) and np.array_equal(cov, ecov)


def test_identical_frames_under_the_identity_give_first():
    f = cases.stack_frame(53, 37)
    frames = np.repeat(f[None], 5, axis=0)
    H = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (5, 1))
    ch = sm.chain(H, np.full(5, 0.5, np.float32), 53, 37)
    for ramp in (bm.DEFAULT_RAMP, (1, 1, 1, 1), (4096, 7, 300, 2)):
        got, cov = bm.render(frames, ch["Ginv"], ch["segs"][0], 4, ramp, None, FILL)
        assert np.array_equal(got, f) and (cov == 5).all()
    assert np.array_equal(sm.render(frames, ch["Ginv"], ch["segs"][0], sm.FIRST, FILL)[0], f)


@pytest.mark.parametrize("name", ["a", "g"])
def test_visiting_order_changes_nothing(name):
    (frames, _, _, _), ch, _, lv = cases.expected(name)
    exp, _ = cases.expected_render(name)
    for si, s in enumerate(ch["segs"]):
        got, cov = bm.render(frames, ch["Ginv"], s, fill=FILL, reverse=True, lv=lv)
        assert np.array_equal(got, exp[si][0]) and np.array_equal(cov, exp[si][1])


def test_case_g_crosses_the_chunk_and_case_h_the_32_bits():
    (frames, _, _, _), ch, _, _ = cases.expected("g")
    assert len(ch["segs"]) == 1 and ch["segs"][0][1] == 300
    assert int(cases.expected_render("g")[0][0][1].max()) == 9
    _, big = cases.expected_render("h")
    assert big > 2 ** 32, "case H is there for numerators beyond 32 bits"
    (frames, _, _, _), ch, _, _ = cases.expected("h")
    assert (cases.expected_render("h")[0][0][1] == 16).all()


def test_negative_numerators_floor():
    """Bands are signed.  One frame and one level: b = floor((2 w D + w) / (2 w)) = D exactly, also where D < 0, so the pixel is
    the frame's own; a truncating division would give D + 1 there and a pixel one level too bright."""
    f = cases.stack_frame(53, 37)
    lv = bm.stack(f, 1)
    assert (f.astype(np.int64) - lv[0]).min() < 0 < (f.astype(np.int64) - lv[0]).max()
    ch = sm.chain(np.array([[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]]), np.full(1, 0.5, np.float32), 53, 37)
    for ramp in ((1,), (3,), (4096,)):
        got, _ = bm.render(f[None], ch["Ginv"], ch["segs"][0], 1, ramp, None, FILL)
        assert np.array_equal(got, f)


def test_seam_measure_on_case_f():
    r = cases.seam_ratios()
    print("case F: r(feather) = %.4f, r(last) = %.4f, r(multiband) = %.4f" % (r["feather"], r["last"], r["multiband"]))
    assert r["multiband"] >= R_MULTIBAND - (R_MULTIBAND - R_FEATHER) / 4
    assert r["feather"] < r["multiband"]
