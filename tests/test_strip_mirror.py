"""CPU: known answers of tests/_strip_mirror.py itself, the reference the strip tests compare the library with."""
import numpy as np

import _strip_cases as cases
import _strip_mirror as sm

I9 = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]


def _rand(n, h, w, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def test_identity_gives_the_frame():
    f = _rand(1, 37, 53)
    c = sm.chain([I9], [0.5], 53, 37)
    assert c["segs"] == [(0, 1, 0, 0, 37, 53)]
    for mode in (sm.FEATHER, sm.FIRST, sm.LAST):
        out, cover = sm.render(f, c["Ginv"], c["segs"][0], mode)
        assert np.array_equal(out, f[0]) and (cover == 1).all()


def test_integer_translation_in_last_mode_gives_the_moved_pixels():
    f = _rand(2, 37, 53)
    c = sm.chain([I9, [1.0, 0, 20.0, 0, 1.0, 7.0, 0, 0, 1.0]], [0.5, 0.5], 53, 37)
    assert c["segs"] == [(0, 2, 0, 0, 44, 73)]
    out, cover = sm.render(f, c["Ginv"], c["segs"][0], sm.LAST, fill=(9, 8, 7))
    exp = np.empty((44, 73, 3), np.uint8)
    exp[:] = (9, 8, 7)
    exp[:37, :53] = f[0]
    exp[7:, 20:] = f[1]
    assert np.array_equal(out, exp)
    assert cover.max() == 2 and cover[0, 60] == 0 and cover[10, 30] == 2
    first, _ = sm.render(f, c["Ginv"], c["segs"][0], sm.FIRST, fill=(9, 8, 7))
    exp[:37, :53] = f[0]
    assert np.array_equal(first, exp)


def test_two_identical_frames_in_feather_give_the_frame():
    f = _rand(1, 37, 53)
    f = np.concatenate([f, f])
    c = sm.chain([I9, I9], [0.5, 0.5], 53, 37)
    out, cover = sm.render(f, c["Ginv"], c["segs"][0], sm.FEATHER)
    assert np.array_equal(out, f[0]) and (cover == 2).all()


def _second_starts(H1, ratio=0.5, **kw):
    c = sm.chain([I9, H1], [0.5, ratio], 53, 37, **kw)
    return c["why"][1], c


def test_rule_1_no_homography():
    why, c = _second_starts([1.0, 0, 5.0, 0, 1.0, 0, 0, 0, 1.0], ratio=-2.0)
    assert why == 1 and len(c["segs"]) == 2 and np.array_equal(c["G"][1], I9)
    assert _second_starts([1.0, 0, 5.0, 0, 1.0, 0, 0, 0, 1.0])[0] == 0


def test_rule_2_not_finite_or_denominator_not_positive():
    assert _second_starts([1.0, 0, float("nan"), 0, 1.0, 0, 0, 0, 1.0])[0] == 2
    assert _second_starts([1.0, 0, 0, 0, 1.0, 0, 0, 0, 0.0])[0] == 2            # division by [8] = 0
    assert _second_starts([1.0, 0, 0, 0, 1.0, 0, -0.02, 0, 1.0])[0] == 2        # 1 - 0.02 * 52 < 0 at the right corners


def test_rule_3_reflection_is_not_the_inputs_orientation():
    assert _second_starts([-1.0, 0, 52.0, 0, 1.0, 0, 0, 0, 1.0])[0] == 3


def test_rule_4_area_out_of_bounds():
    assert _second_starts([5.0, 0, 0, 0, 5.0, 0, 0, 0, 1.0])[0] == 4
    assert _second_starts([0.2, 0, 0, 0, 0.2, 0, 0, 0, 1.0])[0] == 4
    assert _second_starts([4.0, 0, 0, 0, 4.0, 0, 0, 0, 1.0])[0] == 0            # the bound itself is inside


def test_rule_5_canvas_limit():
    assert _second_starts([1.0, 0, 147.0, 0, 1.0, 0, 0, 0, 1.0], max_cols=200)[0] == 0      # cols = 200
    assert _second_starts([1.0, 0, 147.5, 0, 1.0, 0, 0, 0, 1.0], max_cols=200)[0] == 5      # ceil -> 201
    assert _second_starts([1.0, 0, 0, 0, 1.0, -64.0, 0, 0, 1.0], max_rows=100)[0] == 5


def test_case_a_shows_what_it_is_for():
    """The frozen seed: no break, at least three tiles each way, some pixel covered three times, at least 10 % fill."""
    frames, H, ratio, kw = cases.case_a()
    c = sm.chain(H, ratio, 53, 37, **kw)
    assert len(c["segs"]) == 1
    _, _, _, _, rows, cols = c["segs"][0]
    assert cols > 2 * cases.TILE_W and rows > 2 * cases.TILE_H
    _, cover = sm.render(frames, c["Ginv"], c["segs"][0])
    assert cover.max() >= 3 and (cover == 0).mean() >= 0.10


def test_case_c_breaks_where_it_says():
    frames, H, ratio, kw = cases.case_c()
    c = sm.chain(H, ratio, 53, 37, **kw)
    assert tuple(s[0] for s in c["segs"]) == cases.C_STARTS
    assert {k: w for k, w in enumerate(c["why"]) if w} == cases.C_RULES
