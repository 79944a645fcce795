"""CPU: known answers of the gain compensation's numpy mirror (tests/_strip_gain_mirror.py) alone, so that the device and
the host, which are compared with it bit for bit, are not compared with a mirror of the same mistake."""
import numpy as np

import _strip_gain_cases as cases
import _strip_gain_mirror as gm
import _strip_mirror as sm

# The seam measure (gm.seam_measure) of case D after compensation over the one before it, measured with the mirror
# (DESIGN.md section 7d).  Each is asserted at the measured value plus a quarter of its distance to 1: a wrong sign or a
# transposed pair lands above that, and nothing depends on the last digit.
D_SEAM_RATIO_DEFAULTS = 0.4054
D_SEAM_RATIO_SIGMA_G_1 = 0.1365


def _bound(measured):
    return measured + 0.25 * (1.0 - measured)


def test_identical_frames_get_unit_gains():
    rng = np.random.default_rng(2)
    one = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    frames = np.stack([one] * 4)
    H = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (4, 1))
    ch = sm.chain(H, np.full(4, 0.5, np.float32), 53, 37)
    st = gm.stats(frames, ch["G"], ch["Ginv"], ch["seg"])
    assert not st[0].any() and (st[1:, 0] > 1000).all()
    assert np.array_equal(st[1:, 1:4], st[1:, 4:7])         # the sample at an integer position is the pixel
    gq, g = gm.solve(st, ch["seg"])
    assert (gq == 4096).all() and np.allclose(g, 1.0, rtol=0, atol=1e-12)


def test_two_frames_against_the_closed_form():
    """n = 2: [[N (A^2 wN + wg), -N A B wN], [-N A B wN, N (B^2 wN + wg)]] g = [N wg, N wg], solved by Cramer's rule."""
    N, Sa, Sb = 1000, (100 * 1024 * 1000, 80 * 1024 * 1000, 150 * 1024 * 1000), (120 * 1024 * 1000, 80 * 1024 * 1000, 90 * 1024 * 1000)
    st = np.array([[0] * 7, [N, *Sa, *Sb]], np.uint64)
    gq, g = gm.solve(st, np.zeros(2, np.int32), sigma_n=10.0, sigma_g=0.5)
    wN, wg = 1.0 / 100.0, 1.0 / 0.25
    for c in range(3):
        A, B = Sa[c] / (N * 1024.0), Sb[c] / (N * 1024.0)
        a11, a12, a22, r = A * A * wN + wg, -A * B * wN, B * B * wN + wg, wg
        det = a11 * a22 - a12 * a12
        g0, g1 = (r * a22 - a12 * r) / det, (a11 * r - a12 * r) / det
        assert abs(g[0][c] - g0) <= 1e-12 and abs(g[1][c] - g1) <= 1e-12
        assert gq[0][c] == int(np.floor(g0 * 4096 + 0.5)) and gq[1][c] == int(np.floor(g1 * 4096 + 0.5))
        if A < B:                                           # the darker frame is raised, the brighter one lowered
            assert g[0][c] > 1.0 > g[1][c]
        elif A == B:
            assert abs(g[0][c] - 1.0) <= 1e-12 and abs(g[1][c] - 1.0) <= 1e-12 and gq[0][c] == gq[1][c] == 4096
        else:
            assert g[0][c] < 1.0 < g[1][c]


def test_quantisation_clamps_and_survives_non_finite_gains():
    assert [gm.quantise(v) for v in (0.0, 0.25, 1.0, 4.0, 100.0, float("nan"), float("inf"))] == [1024, 1024, 4096, 16384, 16384, 4096, 4096]
    assert gm.apply_gain(np.array([[255 * 1024, 1024, 100 * 1024]], np.int64), [16384, 1024, 4096]).tolist() == [[255 * 1024, 256, 100 * 1024]]


def test_case_d_invalid_pairs_leave_unit_gains():
    (frames, H, ratio, kw), ch, st, gq, g = cases.expected("d")
    assert [(s[0], s[1]) for s in ch["segs"]] == [(0, cases.D_ALONE), (cases.D_ALONE, 1)]
    assert not st[cases.D_NO_OVERLAP].any()                              # no overlap at all
    assert int(st[cases.D_FEW][0]) == cases.D_FEW_PIXELS < gm.DEFAULTS["min_pixels"]
    assert not st[cases.D_ALONE].any()                                   # a one-frame segment
    # frame 5 has no valid pair on either side, frame 9 has no pair: g = 1 exactly
    for k in (cases.D_NO_OVERLAP, cases.D_ALONE):
        assert (g[k] == 1.0).all() and (gq[k] == 4096).all()
    # the blocks of 0 and 255 are dropped: the pairs of frames 2, 3, 7 and 8 count fewer pixels than their overlap holds
    h, w = frames.shape[1:3]
    for k in (2, 3, 7, 8):
        dx, dy = cases.D_OFFSETS[k]
        overlap = (w - int(np.ceil(abs(dx)))) * (h - int(np.ceil(abs(dy))))
        assert 100 <= overlap - int(st[k][0]) <= 120, k     # the block is 10 x 12; a half-pixel sample across its middle is valid
    for k in (1, 4):                                                     # no block nearby: the whole overlap counts
        dx, dy = cases.D_OFFSETS[k]
        assert int(st[k][0]) == (w - int(np.ceil(abs(dx)))) * (h - int(np.ceil(abs(dy))))


def test_case_d_seams_shrink():
    (frames, H, ratio, kw), ch, st, gq, g = cases.expected("d")
    args = (frames, ch["G"], ch["Ginv"], ch["seg"])
    before = gm.seam_measure(*args, np.full_like(gq, 4096))
    after = gm.seam_measure(*args, gq)
    gq1, _ = gm.solve(st, ch["seg"], sigma_g=1.0)
    after1 = gm.seam_measure(*args, gq1)
    print(f"case D seam measure: {before:.4f} before, {after:.4f} with the defaults (ratio {after / before:.4f}), "
          f"{after1:.4f} with sigma_g = 1 (ratio {after1 / before:.4f})")
    assert after / before <= _bound(D_SEAM_RATIO_DEFAULTS)
    assert after1 / before <= _bound(D_SEAM_RATIO_SIGMA_G_1)
    # and the gains times the true ones are closer to one constant per connected run of frames than the true ones are
    true = cases.d_true_gains()
    for lo, hi in ((0, 5), (6, 9)):
        spread = lambda v: float((v[lo:hi].max(axis=0) / v[lo:hi].min(axis=0)).max())
        assert spread(g * true) < spread(true)
