"""The seam finding's test cases (a plain helper module: no fixtures), shared by the CPU and the GPU tests.  Each case returns
(frames [n, h, w, 3] uint8, H [n, 9] float64, ratio [n] float32, chain keyword arguments) as _strip_cases does; `expected(name)`
and `expected_render(name)` are the mirror's answers, computed once and not to be changed by their users.

  A, C   of _strip_cases: perspective pairs, partial tiles, every segment break.
  D      of _strip_gain_cases with its solved gains: the costs are those of the gained frames.
  F      of _strip_band_cases: four 64 x 96 frames misregistered by (1.5, 1) px.  The seam measure is taken here.
  G      of _strip_band_cases: 300 frames of 9 x 7, 299 pairs: more than one round of 64 pairs, up to nine frames on a pixel.
  S      "an object that moved": two 64 x 96 frames cut 40 px apart from a texture of 2 x 2 blocks, exactly registered; frame 1
         carries a solid block at rows 38..57, columns 6..17, across the medial line of the overlap (columns 0..23, medial 11/12).
  OW, OH orientations, on 300 x 20 and 20 x 300 frames (more than 256 states on one axis, not a multiple of 64): pairs moving
         +x, -x, +y, -y, the tie |dx| == |dy|, and a pair inside one segment whose frames do not overlap at all.
  L      two 520 x 480 frames: 33 x 480 words of back pointers are more than the path kernel keeps in LDS."""
import functools

import numpy as np

import _strip_band_cases as bcases
import _strip_cases as base
import _strip_gain_cases as gcases
import _strip_mirror as sm
import _strip_seam_mirror as mm

FILL = gcases.FILL
ROUND = 64                       # pairs per round (csrc/strip.hip: kSeamRound)
BACK_LDS_WORDS = 15360           # back pointers k_strip_seam_path keeps in LDS (kSeamBackLdsWords)
S_PITCH, S_BLOCK = 40, (38, 58, 6, 18)          # case S: rows 38..57, columns 6..17 of frame 1
S_VALUE = (250, 20, 130)
O_MOVES = ((0, 0), (30, 0), (-30, 0), (0, 5), (0, -5), (6, 6), (400, 0), (-370, 3))    # H[k]'s translation: k onto k - 1
O_NO_OVERLAP = 6


def case_s():
    n, h, w = 2, 96, 64
    rng = np.random.default_rng(61)
    sw = w + S_PITCH
    scene = np.repeat(np.repeat(rng.integers(0, 256, (h // 2, sw // 2, 3), dtype=np.uint8), 2, axis=0), 2, axis=1)
    frames = np.stack([scene[:, k * S_PITCH:k * S_PITCH + w] for k in range(n)]).copy()
    y0, y1, x0, x1 = S_BLOCK
    frames[1, y0:y1, x0:x1] = S_VALUE
    H = np.tile(np.array([1.0, 0, S_PITCH, 0, 1.0, 0, 0, 0, 1.0]), (n, 1))
    return frames, H, np.full(n, 0.5, np.float32), {}


def _case_o(w, h, swap):
    n = len(O_MOVES)
    frames = np.random.default_rng(67 + swap).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    H = np.zeros((n, 9))
    for k, (a, b) in enumerate(O_MOVES):
        tx, ty = (b, a) if swap else (a, b)
        H[k] = [1.0, 0, tx, 0, 1.0, ty, 0, 0, 1.0]
    return frames, H, np.full(n, 0.5, np.float32), {}


def case_ow():
    return _case_o(300, 20, False)


def case_oh():
    return _case_o(20, 300, True)


def case_l():
    n, h, w = 2, 480, 520
    assert -(-w // 16) * h > BACK_LDS_WORDS
    frames = np.random.default_rng(71).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    H = np.tile(np.array([1.0, 0, 200.0, 0, 1.0, 13.0, 0, 0, 1.0]), (n, 1))
    return frames, H, np.full(n, 0.5, np.float32), {}


CASES = {"a": base.case_a, "c": base.case_c, "d": gcases.case_d, "f": bcases.case_f, "g": bcases.case_g, "s": case_s, "ow": case_ow,
         "oh": case_oh, "l": case_l}
GAINED = ("d",)


@functools.lru_cache(maxsize=None)
def expected(name, gained=None, prior=mm.DEFAULT_PRIOR):
    """(case, chain, gq [n, 3] or None, seam [n, L], orient [n], total [n], costs {k: C}) by the mirror; gained None: the case's
    own (D: its solved gains, the others: none)"""
    if name == "d":
        case, ch, _, gq, _ = gcases.expected("d")
    else:
        case = CASES[name]()
        frames, H, ratio, kw = case
        ch = sm.chain(H, ratio, frames.shape[2], frames.shape[1], **kw)
        gq = None
    if gained is False or (gained is None and name not in GAINED):
        gq = None
    elif gq is None:
        gq = np.random.default_rng(73).integers(2048, 8193, (len(case[0]), 3)).astype(np.int32)
    costs = {}
    seam, ori, total = mm.seams(case[0], ch["G"], ch["Ginv"], ch["seg"], gq, prior, costs)
    for a in (case[0], seam, ori, total, *costs.values()):
        a.setflags(write=False)
    return case, ch, gq, seam, ori, total, costs


@functools.lru_cache(maxsize=None)
def expected_render(name, gained=None):
    """{segment: (canvas, cover, winner)} by the mirror with the case's found seams"""
    (frames, _, _, _), ch, gq, seam, ori, _, _ = expected(name, gained)
    out = {}
    for si, s in enumerate(ch["segs"]):
        inter = {}
        canvas, cover = mm.render(frames, ch["Ginv"], s, seam, ori, gq, FILL, inter)
        out[si] = (canvas, cover, inter["winner"])
    return out


def straight_best(C):
    """the cheapest straight line through a cost [T, S]: (state, total)"""
    col = np.asarray(C, np.int64).sum(axis=0)
    return int(np.argmin(col)), int(col.min())


@functools.lru_cache(maxsize=None)
def seam_measures():
    """Case F by the mirror alone: the mean |Pa - Pb| in 8-bit levels where the winner changes between 4-neighbours -> last, seam"""
    (frames, _, _, _), ch, _, seam, ori, _, _ = expected("f")
    inter = {}
    mm.render(frames, ch["Ginv"], ch["segs"][0], seam, ori, None, FILL, inter)
    first = ch["segs"][0][0]
    last = mm.seam_measure(inter["P"], inter["ok"], mm.winners_last(inter["ok"]))
    found = mm.seam_measure(inter["P"], inter["ok"], np.where(inter["winner"] >= 0, inter["winner"] - first, -1))
    return {"last": last[0], "seam": found[0], "n_last": last[1], "n_seam": found[1]}
