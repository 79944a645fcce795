"""CPU: the numpy mirror of the seam finding (tests/_strip_seam_mirror.py) against its own known answers -- the byte-for-byte
consequences of the definitions, the enumeration of all paths on small costs with planted ties, and
the bound total <= the cheapest straight line on every case."""
import itertools

import numpy as np
import pytest

import _strip_mirror as sm
import _strip_seam_cases as cases
import _strip_seam_mirror as mm

FILL = cases.FILL
# the mirror's values on case F with the default prior: mean |Pa - Pb| in 8-bit levels across the
# winner's changes for LAST and for SEAM, and their ratio; a retuned prior may give up a quarter of the way to 1, not more
M_LAST, M_SEAM = 71.27, 65.34
R_SEAM = M_SEAM / M_LAST


def brute(C):
    """every path of a cost [T, S]: the cheapest total, and the path the tie rules choose among the cheapest"""
    T, S = C.shape
    best = None
    for end in range(S):
        for moves in itertools.product((0, -1, 1), repeat=T - 1):        # backwards from the end: the predecessor's offset
            p, ok = [end], True
            for m in moves:
                p.append(p[-1] + m)
                ok = ok and 0 <= p[-1] < S
            if not ok:
                continue
            tot = sum(int(C[T - 1 - i][s]) for i, s in enumerate(p))
            if best is None or tot < best:
                best = tot
    return best


def tie_path(C):
    """the definition read literally, in Python integers"""
    T, S = C.shape
    E = [[int(v) for v in C[0]]]
    for t in range(1, T):
        row = []
        for s in range(S):
            m = E[-1][s]
            if s > 0 and E[-1][s - 1] < m:
                m = E[-1][s - 1]
            if s + 1 < S and E[-1][s + 1] < m:
                m = E[-1][s + 1]
            row.append(int(C[t][s]) + m)
        E.append(row)
    s = E[-1].index(min(E[-1]))
    seam = [0] * T
    for t in range(T - 1, -1, -1):
        seam[t] = s
        if t:
            m = min(E[t - 1][max(s - 1, 0):s + 2])
            s = s if E[t - 1][s] == m else (s - 1 if s > 0 and E[t - 1][s - 1] == m else s + 1)
    return seam, min(E[-1])


TIES = {
    "prefer s over s - 1": (np.array([[5, 5, 9, 9, 9], [9, 1, 9, 9, 9], [9, 1, 9, 9, 9], [9, 1, 9, 9, 9]]), [1, 1, 1, 1]),
    "prefer s over s + 1": (np.array([[9, 5, 5, 9, 9], [9, 1, 9, 9, 9], [9, 1, 9, 9, 9], [9, 1, 9, 9, 9]]), [1, 1, 1, 1]),
    "prefer s - 1 over s + 1": (np.array([[5, 9, 5, 9, 9], [9, 1, 9, 9, 9], [9, 1, 9, 9, 9], [9, 1, 9, 9, 9]]), [0, 1, 1, 1]),
    "the smallest end": (np.array([[1, 9, 1], [1, 9, 1], [1, 9, 1], [1, 9, 1], [1, 9, 1]]), [0, 0, 0, 0, 0]),
    "all equal": (np.full((5, 3), 7), [0, 0, 0, 0, 0]),
}


@pytest.mark.parametrize("name", sorted(TIES))
def test_path_against_the_enumeration_with_planted_ties(name):
    C, want = TIES[name]
    assert C.shape in ((4, 5), (5, 3))
    seam, total = mm.path(C)
    assert total == brute(C) == mm.path_cost(C, seam)
    assert list(seam) == want == tie_path(C)[0]


def test_path_against_the_enumeration_on_random_costs():
    rng = np.random.default_rng(3)
    for shape in ((4, 5), (5, 3), (1, 4), (6, 1)):
        for hi in (3, 1000):                                # tie-heavy and not
            for _ in range(20):
                C = rng.integers(0, hi, shape)
                seam, total = mm.path(C)
                assert total == brute(C) == mm.path_cost(C, seam)
                assert (list(seam), total) == tie_path(C)
                assert np.all(np.abs(np.diff(seam)) <= 1)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_total_is_at_most_the_cheapest_straight_line(name):
    _, ch, _, seam, ori, total, costs = cases.expected(name)
    assert len(costs) == sum(c - 1 for _, c, *_ in ch["segs"])
    for k, C in costs.items():
        T = C.shape[0]
        assert int(total[k]) <= cases.straight_best(C)[1]
        assert int(total[k]) == mm.path_cost(C, seam[k][:T]) and np.all(seam[k][T:] == -1)
        assert C.max() <= mm.OUTSIDE and T * mm.OUTSIDE < 2 ** 32
    firsts = [f for f, *_ in ch["segs"]]
    assert np.all(seam[firsts] == -1) and np.all(total[firsts] == 0)


def test_translated_pair_has_the_straight_seam_of_the_prior():
    """w = 64, h = 96, d = 40, prior 1024: seam 11 at every step and total 98304 (the issue's own figures)"""
    rng = np.random.default_rng(5)
    scene = rng.integers(0, 256, (96, 110, 3), dtype=np.uint8)
    frames = np.stack([scene[:, :64], scene[:, 40:104]])
    H = np.tile(np.array([1.0, 0, 40.0, 0, 1.0, 0, 0, 0, 1.0]), (2, 1))
    ch = sm.chain(H, np.full(2, 0.5, np.float32), 64, 96)
    seam, ori, total = mm.seams(frames, ch["G"], ch["Ginv"], ch["seg"])
    assert ori[1] == 1 and np.all(seam[1] == 11) and int(total[1]) == 98304
    for prior, d in ((512, 40), (1024, 41), (0, 40)):
        Hd = np.tile(np.array([1.0, 0, float(d), 0, 1.0, 0, 0, 0, 1.0]), (2, 1))
        fr = np.stack([scene[:, :64], scene[:, d:d + 64]])
        chd = sm.chain(Hd, np.full(2, 0.5, np.float32), 64, 96)
        seam, ori, total = mm.seams(fr, chd["G"], chd["Ginv"], chd["seg"], prior=prior)
        S = 64
        im = [abs(min(s, S - 1 - s) - min(s + d, S - 1 - s - d)) for s in range(S - d)]
        want = 0 if prior == 0 else im.index(min(im))
        assert np.all(seam[1] == want) and int(total[1]) == 96 * prior * min(im)


def test_object_that_moved():
    (frames, _, _, _), ch, _, seam, ori, total, costs = cases.expected("s")
    y0, y1, x0, x1 = cases.S_BLOCK
    assert ori[1] == 1
    sm1 = seam[1][:96]
    assert np.all(sm1[:y0 - 6] == 11) and np.all(sm1[y1 + 6:] == 11) and np.all(sm1[y0:y1] == 5)
    assert not any(x0 <= s < x1 for s in sm1[y0:y1])        # no seam pixel lies inside the block
    assert int(total[1]) == 405504
    assert cases.straight_best(costs[1]) == (5, 1277952)
    canvas = cases.expected_render("s")[0][0]
    block = canvas[y0:y1, cases.S_PITCH + x0:cases.S_PITCH + x1]
    assert np.all(block == np.array(cases.S_VALUE, np.uint8))            # the block is whole
    first = sm.render(frames, ch["Ginv"], ch["segs"][0], sm.FIRST, FILL)[0]
    assert not np.any(np.all(first[y0:y1, cases.S_PITCH + x0:cases.S_PITCH + x1] == np.array(cases.S_VALUE, np.uint8), axis=2))   # FIRST loses it
    # a feathered strip shows it twice as dark: neither the block nor the floor
    feather = sm.render(frames, ch["Ginv"], ch["segs"][0], sm.FEATHER, FILL)[0]
    assert not np.array_equal(feather[y0:y1, cases.S_PITCH + x0:cases.S_PITCH + x1], block)


def test_orientations():
    for name in ("ow", "oh"):
        (frames, _, _, _), ch, _, seam, ori, total, costs = cases.expected(name)
        assert len(ch["segs"]) == 1
        # +x, -x, +y, -y, the tie (axis 0 wins it), two pairs without overlap
        want = [0, 1, 3, 0, 2, 0, 1, 3] if name == "ow" else [0, 0, 2, 1, 3, 0, 0, 2]
        assert list(ori) == want
        for k in (cases.O_NO_OVERLAP, cases.O_NO_OVERLAP + 1):
            C = costs[k]
            assert np.all(C == mm.OUTSIDE) and np.all(seam[k][:C.shape[0]] == 0) and int(total[k]) == C.shape[0] * mm.OUTSIDE
        assert max(C.shape[1] for C in costs.values()) == 300
        cover = cases.expected_render(name)[0][1]
        assert cover.max() >= 2


def test_single_cover_equals_first_and_every_pixel_is_its_winner():
    for name in ("a", "c", "d", "f", "ow"):
        (frames, _, _, _), ch, gq, seam, ori, _, _ = cases.expected(name)
        for si, seg in enumerate(ch["segs"]):
            canvas, cover, winner = cases.expected_render(name)[si]
            import _strip_gain_mirror as gm
            g = gq if gq is not None else np.full((len(frames), 3), 4096, np.int32)
            first, fcover = gm.render_gain(frames, ch["Ginv"], seg, g, sm.FIRST, FILL)
            assert np.array_equal(cover, fcover)
            one = cover == 1
            assert np.array_equal(canvas[one], first[one]) and np.all(canvas[cover == 0] == np.array(FILL, np.uint8))
            for k in range(seg[0], seg[0] + seg[1]):
                single = gm.render_gain(frames, ch["Ginv"], (k, 1) + tuple(seg[2:]), g, sm.FIRST, FILL)[0]
                assert np.array_equal(canvas[winner == k], single[winner == k])
            assert np.all((winner >= 0) == (cover > 0))


def test_injected_seams_give_last_and_first():
    (frames, _, _, _), ch, _, seam, ori, _, _ = cases.expected("a")
    n, h, w = frames.shape[:3]
    seg = ch["segs"][0]
    last, first = (sm.render(frames, ch["Ginv"], seg, m, FILL)[0] for m in (sm.LAST, sm.FIRST))
    zero = np.zeros((n, max(w, h)), np.int32)
    for o in (0, 1):
        assert np.array_equal(mm.render(frames, ch["Ginv"], seg, zero, np.full(n, o, np.int32), None, FILL)[0], last)
        S = w if o else h
        assert np.array_equal(mm.render(frames, ch["Ginv"], seg, zero + (S - 1), np.full(n, o | 2, np.int32), None, FILL)[0], last)
        assert np.array_equal(mm.render(frames, ch["Ginv"], seg, zero + S, np.full(n, o, np.int32), None, FILL)[0], first)


def test_identical_frames_under_the_identity_give_first():
    rng = np.random.default_rng(9)
    frames = np.repeat(rng.integers(0, 256, (1, 20, 30, 3), dtype=np.uint8), 3, axis=0)
    H = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (3, 1))
    ch = sm.chain(H, np.full(3, 0.5, np.float32), 30, 20)
    seam, ori, total = mm.seams(frames, ch["G"], ch["Ginv"], ch["seg"])
    assert np.all(total == 0)
    canvas = mm.render(frames, ch["Ginv"], ch["segs"][0], seam, ori, None, FILL)[0]
    assert np.array_equal(canvas, sm.render(frames, ch["Ginv"], ch["segs"][0], sm.FIRST, FILL)[0])


def test_gains_change_the_costs_of_case_d():
    _, _, gq, _, _, total, costs = cases.expected("d")
    _, _, none, _, _, total0, costs0 = cases.expected("d", gained=False)
    assert gq is not None and none is None
    assert any(not np.array_equal(costs[k], costs0[k]) for k in costs) and not np.array_equal(total, total0)


def test_found_seams_of_case_f_are_not_straight():
    _, _, _, seam, _, total, costs = cases.expected("f")
    for k, C in costs.items():
        print("case F pair %d: found %d, best straight %d" % (k, int(total[k]), cases.straight_best(C)[1]))
        assert int(total[k]) < cases.straight_best(C)[1] and len(set(seam[k][:C.shape[0]])) > 1


def test_seam_measure_on_case_f():
    m = cases.seam_measures()
    r = m["seam"] / m["last"]
    print("case F: last %.2f over %d samples, seam %.2f over %d samples, ratio %.4f" % (m["last"], m["n_last"], m["seam"], m["n_seam"], r))
    assert abs(m["last"] - M_LAST) < 0.01                   # LAST does not depend on the prior: the recorded value itself
    assert r <= R_SEAM + (1.0 - R_SEAM) / 4
