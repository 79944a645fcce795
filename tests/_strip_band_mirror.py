"""The strip mosaic's multi-band blending restated in numpy, for the tests (a plain helper module: no fixtures).  It takes
nothing from csrc/strip_core.hpp; the sampling, the bilinear taps and the gain are _strip_gain_mirror's.  The definitions are

  stack    a trous, undecimated, in the frame's own coordinates: level 0 is the frame; with s = 2^l and k = (1, 4, 6, 4, 1)
           L[l+1](y, x, c) = (sum_i sum_j k_i k_j L[l](clamp(y + (i-2) s, 0, h-1), clamp(x + (j-2) s, 0, w-1), c) + 128) >> 8,
           one rounding per level, u8.
  render   every covering frame k of a canvas pixel has its taps and its feather weight q_k; S[k][l] = the bilinear sample of
           level l of frame k (each times the frame's gain, when there are gains), D[k][l] = S[k][l] - S[k][l+1];
           qmax = max_k q_k; w[k][l] = max(0, q_k - qmax + ramp[l]); N[l] = sum_k w[k][l] D[k][l], W[l] = sum_k w[k][l];
           NL = sum_k q_k S[k][levels], WL = sum_k q_k; b = sum_l floor((2 N[l] + W[l]) / (2 W[l])) (towards minus infinity);
           out = clamp(floor((NL + (b + 512) WL) / (1024 WL)), 0, 255); uncovered pixels take the fill.

Python's and numpy's // on integers is the floor division."""
import numpy as np

from _strip_gain_mirror import apply_gain, bilinear, sample

DEFAULT_LEVELS, DEFAULT_RAMP = 4, (1, 2, 4, 8)
K = (1, 4, 6, 4, 1)


def level(cur, s):
    """One level from the one before it: cur [h, w, 3] integers, s = the distance of the taps -> [h, w, 3] int64"""
    cur = np.asarray(cur).astype(np.int64)
    h, w = cur.shape[:2]
    # separable without a rounding in between: the same integers as the double sum (test_strip_band_mirror.py has the loops)
    rows = sum(K[i] * cur[np.clip(np.arange(h) + (i - 2) * s, 0, h - 1)] for i in range(5))
    acc = sum(K[j] * rows[:, np.clip(np.arange(w) + (j - 2) * s, 0, w - 1)] for j in range(5))
    return (acc + 128) >> 8


def stack(frame, levels=DEFAULT_LEVELS):
    """frame [h, w, 3] uint8 -> [levels, h, w, 3] uint8: levels 1 .. levels"""
    cur, out = np.asarray(frame), []
    for l in range(levels):
        cur = level(cur, 1 << l)
        out.append(cur.astype(np.uint8))
    return np.stack(out)


def stacks(frames, levels=DEFAULT_LEVELS):
    """frames [n, h, w, 3] -> [levels + 1, n, h, w, 3]: level 0 is the frames themselves"""
    frames = np.asarray(frames)
    st = np.stack([stack(f, levels) for f in frames], axis=1)
    return np.concatenate([frames[None], st])


def render(frames, Ginv, segment, levels=DEFAULT_LEVELS, ramp=DEFAULT_RAMP, gq=None, fill=(0, 0, 0), reverse=False, inter=None, lv=None):
    """frames [n, h, w, 3] uint8, Ginv [n, 9], segment = (first, count, x0, y0, rows, cols) -> (canvas [rows, cols, 3] uint8,
    cover [rows, cols] uint8).  gq [n, 3]: gains in 1/4096 or None; reverse: visit the frames backwards; inter: a dict that
    receives max_abs_numerator = max |2 N[l] + W[l]|; lv: stacks(frames, levels) when the caller has them already."""
    frames = np.asarray(frames)
    first, count, x0, y0, rows, cols = segment
    h, w = frames.shape[1:3]
    if lv is None:
        lv = np.concatenate([frames[None], np.zeros((levels,) + frames.shape, np.uint8)])
        for k in range(first, first + count):
            lv[1:, k] = stack(frames[k], levels)
    py, px = np.meshgrid(np.arange(rows, dtype=np.float64) + float(y0), np.arange(cols, dtype=np.float64) + float(x0), indexing="ij")
    order = list(range(first, first + count))
    if reverse:
        order.reverse()
    qmax = np.zeros((rows, cols), np.int64)
    cnt = np.zeros((rows, cols), np.int64)
    for k in order:
        ok, _, q = sample(Ginv[k], px, py, w, h)
        qmax = np.maximum(qmax, q)
        cnt += ok
    N = np.zeros((levels, rows, cols, 3), np.int64)
    W = np.zeros((levels, rows, cols), np.int64)
    NL = np.zeros((rows, cols, 3), np.int64)
    WL = np.zeros((rows, cols), np.int64)
    for k in order:
        ok, taps, q = sample(Ginv[k], px, py, w, h)
        S = [bilinear(lv[l][k], taps) for l in range(levels + 1)]
        if gq is not None:
            S = [apply_gain(P, gq[k]) for P in S]
        for l in range(levels):
            wk = np.where(ok, np.maximum(q - qmax + int(ramp[l]), 0), 0)
            N[l] += wk[..., None] * (S[l] - S[l + 1])
            W[l] += wk
        NL += q[..., None] * S[levels]
        WL += q
    m = cnt > 0
    out = np.empty((rows, cols, 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    b = np.zeros((int(m.sum()), 3), np.int64)
    big = 0
    for l in range(levels):
        Wm = W[l][m][:, None]
        assert (Wm >= int(ramp[l])).all()
        num = 2 * N[l][m] + Wm
        big = max(big, int(np.abs(num).max())) if num.size else big
        b += num // (2 * Wm)
    WLm = WL[m][:, None]
    out[m] = np.clip((NL[m] + (b + 512) * WLm) // (1024 * WLm), 0, 255).astype(np.uint8)
    if inter is not None:
        inter["max_abs_numerator"] = big
    return out, np.minimum(cnt, 255).astype(np.uint8)


def laplacian_energy(canvas, cover):
    """The sum of squares of the 4-neighbour Laplacian over the interior pixels that two or more frames cover."""
    c = canvas.astype(np.int64)
    lap = 4 * c[1:-1, 1:-1] - c[:-2, 1:-1] - c[2:, 1:-1] - c[1:-1, :-2] - c[1:-1, 2:]
    m = cover[1:-1, 1:-1] >= 2
    return float((lap[m] ** 2).sum())
