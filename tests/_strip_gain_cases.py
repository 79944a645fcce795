"""The gain compensation's test cases (a plain helper module: no fixtures), shared by the CPU and the GPU tests.  Each
returns (frames [n, h, w, 3] uint8, H [n, 9] float64, ratio [n] float32, chain keyword arguments) as _strip_cases does;
`expected(name)` is the mirror's whole answer for a case, computed once and not to be changed by its users.

  A, C   of _strip_cases: perspective pairs, partial tiles, every segment break (a pair across a break has all-zero stats).
  D      ten 53 x 37 frames cut from one smooth scene at integer and half-pixel translations, each times a known gain per
         channel in 0.8..1.25 and rounded.  Frame 5 lies a whole frame width beyond frame 4 (no overlap at all, same segment);
         frame 6 shares 3 x 7 = 21 pixels with frame 5 (fewer than min_pixels); frames 2 and 7 carry a block of 0 and 255 inside
         their overlaps, which lo / hi drop; frame 9 is a segment of its own.
  E      two 160 x 120 frames of values 200..250 under the identity: N x 255 x 1024 passes 2^32."""
import functools

import numpy as np

import _strip_cases as base
import _strip_gain_mirror as gm
import _strip_mirror as sm

case_a, case_c = base.case_a, base.case_c

D_OFFSETS = ((0, 0), (12, 3), (10.5, 2.5), (13, -2), (11.5, 4), (60, 0), (50, 30), (12, 2), (9.5, -3), (11, 1))   # frame k against k - 1
D_NO_OVERLAP, D_FEW, D_BLOCKS, D_ALONE = 5, 6, (2, 7), 9
D_FEW_PIXELS = 21


def d_true_gains():
    return np.random.default_rng(23).uniform(0.8, 1.25, (len(D_OFFSETS), 3))


def case_d():
    n, h, w = len(D_OFFSETS), 37, 53
    rng = np.random.default_rng(17)
    # the scene on a half-pixel grid: a few sinusoids per channel, 60..190
    pos = np.cumsum(np.array(D_OFFSETS, np.float64), axis=0)
    pos -= pos.min(axis=0)
    SW, SH = int(2 * (pos[:, 0].max() + w)) + 2, int(2 * (pos[:, 1].max() + h)) + 2
    yy, xx = np.meshgrid(np.arange(SH) / 2.0, np.arange(SW) / 2.0, indexing="ij")
    scene = np.zeros((SH, SW, 3))
    for c in range(3):
        for _ in range(4):
            fx, fy, ph = rng.uniform(0.02, 0.12), rng.uniform(0.02, 0.12), rng.uniform(0, 2 * np.pi)
            scene[..., c] += np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
    scene = 125.0 + scene * (65.0 / 4.0)
    gains = d_true_gains()
    frames = np.zeros((n, h, w, 3), np.uint8)
    H = np.zeros((n, 9))
    for k in range(n):
        ox, oy = int(round(2 * pos[k, 0])), int(round(2 * pos[k, 1]))
        cut = scene[oy:oy + 2 * h:2, ox:ox + 2 * w:2]
        frames[k] = np.clip(np.floor(cut * gains[k] + 0.5), 0, 255).astype(np.uint8)
        H[k] = [1.0, 0, D_OFFSETS[k][0], 0, 1.0, D_OFFSETS[k][1], 0, 0, 1.0]
    for k in D_BLOCKS:                                   # columns 14..25 overlap both neighbours: six of 0, six of 255
        frames[k, 10:20, 14:20] = 0
        frames[k, 10:20, 20:26] = 255
    ratio = np.full(n, 0.5, np.float32)
    ratio[D_ALONE] = -2.0
    return frames, H, ratio, {"max_cols": 4096, "max_rows": 4096, "max_scale": 4.0}


def case_e():
    rng = np.random.default_rng(29)
    frames = rng.integers(200, 251, (2, 120, 160, 3), dtype=np.uint8)
    H = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (2, 1))
    return frames, H, np.full(2, 0.5, np.float32), {}


CASES = {"a": case_a, "c": case_c, "d": case_d, "e": case_e}
FILL = (7, 99, 200)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, chain, stats [n, 7], gq [n, 3], g [n, 3]) by the mirror, with the default configuration."""
    case = CASES[name]()
    frames, H, ratio, kw = case
    h, w = frames.shape[1:3]
    ch = sm.chain(H, ratio, w, h, **kw)
    st = gm.stats(frames, ch["G"], ch["Ginv"], ch["seg"])
    gq, g = gm.solve(st, ch["seg"])
    for a in (frames, st, gq, g):
        a.setflags(write=False)
    return case, ch, st, gq, g


@functools.lru_cache(maxsize=None)
def expected_render(name, gains="solved"):
    """{(segment, mode): (canvas, cover)} by the mirror for a case: with its solved gains, or every gain = the given value."""
    (frames, _, _, _), ch, _, gq, _ = expected(name)
    if gains != "solved":
        gq = np.full((len(frames), 3), int(gains), np.int32)
    return {(si, m): gm.render_gain(frames, ch["Ginv"], s, gq, m, FILL) for si, s in enumerate(ch["segs"]) for m in (sm.FEATHER, sm.FIRST, sm.LAST)}
