"""The strip mosaic's gain compensation restated in numpy, for the tests (a plain helper module: no fixtures).  It takes
nothing from csrc/strip_core.hpp; the sampling is _strip_mirror's (restated here as a function of plane points: there it is
written into the render).  The definitions are

  pair     frame k (not its segment's first) against frame k - 1: every integer pixel (x, y) of frame k goes to the plane by
           d = ((G6 x) + (G7 y)) + G8 > 0, px, py by IEEE division, both finite; frame k - 1 is sampled there under its Ginv
           (covered, taps and 5-bit fractions as in the render); Pb = 1024 * pixel, Pa = taps times 10-bit weights; the pixel
           is valid iff all six values lie in [1024 lo, 1024 hi].  stats[k] = N, Sa[3], Sb[3] over the valid pixels.
  solve    per segment and channel; a pair with N < min_pixels is left out; A = Sa / (N 1024), B = Sb / (N 1024),
           wN = 1 / sigma_n^2, wg = 1 / sigma_g^2 (the sigmas are float32 values);  for the pair (a, b) = (k - 1, k):
           diag[a] += N ((A A) wN + wg), diag[b] += N ((B B) wN + wg), off[a] = -(N ((A B) wN)), rhs[a] += N wg, rhs[b] += N wg;
           a frame whose diag is 0 gets diag = rhs = 1; Thomas elimination forwards and backwards;
           gq = clamp(floor(g 4096 + 0.5), 1024, 16384), 4096 when g is not finite.
  apply    Pg = min((P gq + 2048) >> 12, 255 * 1024), in front of the blend of every mode; the cover plane does not change."""
import math

import numpy as np

from _strip_mirror import FEATHER, FIRST, _div

DEFAULTS = {"sigma_n": 10.0, "sigma_g": 0.1, "lo": 5, "hi": 250, "min_pixels": 64}


def sample(A, px, py, w, h):
    """Plane points (arrays) under A = Ginv of a w x h frame -> covered, (x, x1, y, y1, fx, fy), feather weight q."""
    A = [np.float64(v) for v in A]
    with np.errstate(all="ignore"):
        d = ((A[6] * px) + (A[7] * py)) + A[8]
        u = (((A[0] * px) + (A[1] * py)) + A[2]) / d
        v = (((A[3] * px) + (A[4] * py)) + A[5]) / d
        ok = (d > 0.0) & (np.abs(u) < 1048576.0) & (np.abs(v) < 1048576.0)
        U = np.floor((np.where(ok, u, 0.0) * 32.0) + 0.5).astype(np.int64)
        V = np.floor((np.where(ok, v, 0.0) * 32.0) + 0.5).astype(np.int64)
    ok &= (U >= 0) & (U <= 32 * (w - 1)) & (V >= 0) & (V <= 32 * (h - 1))
    U, V = np.where(ok, U, 0), np.where(ok, V, 0)
    x, fx, y, fy = U >> 5, U & 31, V >> 5, V & 31
    xn, yn = (U + 16) >> 5, (V + 16) >> 5
    q = 1 + np.minimum(np.minimum(xn, w - 1 - xn), np.minimum(yn, h - 1 - yn))
    return ok, (x, np.minimum(x + 1, w - 1), y, np.minimum(y + 1, h - 1), fx, fy), np.where(ok, q, 0)


def bilinear(frame, taps):
    x, x1, y, y1, fx, fy = taps
    f = frame.astype(np.int64)
    return (((32 - fx) * (32 - fy))[..., None] * f[y, x] + (fx * (32 - fy))[..., None] * f[y, x1]
            + ((32 - fx) * fy)[..., None] * f[y1, x] + (fx * fy)[..., None] * f[y1, x1])


def pair_samples(frames, G, Ginv, k, lo=5, hi=250):
    """Frame k against frame k - 1: (Pa [h, w, 3], Pb [h, w, 3], valid [h, w])."""
    h, w = frames.shape[1:3]
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    g = [np.float64(v) for v in G[k]]
    with np.errstate(all="ignore"):
        d = ((g[6] * x) + (g[7] * y)) + g[8]
        px = (((g[0] * x) + (g[1] * y)) + g[2]) / d
        py = (((g[3] * x) + (g[4] * y)) + g[5]) / d
    ok = (d > 0.0) & np.isfinite(px) & np.isfinite(py)
    cov, taps, _ = sample(Ginv[k - 1], np.where(ok, px, 0.0), np.where(ok, py, 0.0), w, h)
    Pa = bilinear(frames[k - 1], taps)
    Pb = 1024 * frames[k].astype(np.int64)
    valid = ok & cov & ((Pa >= 1024 * lo) & (Pa <= 1024 * hi) & (Pb >= 1024 * lo) & (Pb <= 1024 * hi)).all(axis=2)
    return Pa, Pb, valid


def stats(frames, G, Ginv, seg, lo=5, hi=250):
    """-> [n, 7] uint64: N, Sa[3], Sb[3] of every frame's pair with the frame before it; zeros for a segment's first frame."""
    n = len(frames)
    out = np.zeros((n, 7), np.uint64)
    for k in range(1, n):
        if seg[k] != seg[k - 1]:
            continue
        Pa, Pb, valid = pair_samples(frames, G, Ginv, k, lo, hi)
        out[k] = [int(valid.sum())] + [int(Pa[valid][:, c].sum()) for c in range(3)] + [int(Pb[valid][:, c].sum()) for c in range(3)]
    return out


def quantise(g):
    if not math.isfinite(g):
        return 4096
    return int(min(max(math.floor((g * 4096.0) + 0.5), 1024), 16384))


def solve(st, seg, sigma_n=10.0, sigma_g=0.1, min_pixels=64, **_):
    """st [n, 7], seg [n] -> (gq [n, 3] int32, g [n, 3] float64)."""
    n = len(seg)
    sn, sg = float(np.float32(sigma_n)), float(np.float32(sigma_g))
    wN, wg = _div(1.0, sn * sn), _div(1.0, sg * sg)
    g, gq = np.zeros((n, 3)), np.zeros((n, 3), np.int32)
    first = 0
    while first < n:
        end = first + 1
        while end < n and seg[end] == seg[first]:
            end += 1
        m = end - first
        for c in range(3):
            diag, off, rhs = [0.0] * m, [0.0] * m, [0.0] * m
            for i in range(1, m):
                N = int(st[first + i][0])
                if N < min_pixels:
                    continue
                Nd = float(N)
                A, B = _div(float(int(st[first + i][1 + c])), Nd * 1024.0), _div(float(int(st[first + i][4 + c])), Nd * 1024.0)
                diag[i - 1] = diag[i - 1] + (Nd * (((A * A) * wN) + wg))
                diag[i] = diag[i] + (Nd * (((B * B) * wN) + wg))
                off[i - 1] = -(Nd * ((A * B) * wN))
                rhs[i - 1] = rhs[i - 1] + (Nd * wg)
                rhs[i] = rhs[i] + (Nd * wg)
            for i in range(m):
                if diag[i] == 0.0:
                    diag[i] = rhs[i] = 1.0
            cc, e = list(diag), list(rhs)
            for i in range(1, m):
                mul = _div(off[i - 1], cc[i - 1])
                cc[i] = diag[i] - (mul * off[i - 1])
                e[i] = rhs[i] - (mul * e[i - 1])
            x = [0.0] * m
            x[m - 1] = _div(e[m - 1], cc[m - 1])
            for i in range(m - 2, -1, -1):
                x[i] = _div(e[i] - (off[i] * x[i + 1]), cc[i])
            for i in range(m):
                g[first + i][c] = x[i]
                gq[first + i][c] = quantise(x[i])
        first = end
    return gq, g


def apply_gain(P, gq):
    """P int64 [..., 3] (0 .. 255 * 1024), gq [3]"""
    return np.minimum((P * np.asarray(gq, np.int64) + 2048) >> 12, 255 * 1024)


def render_gain(frames, Ginv, segment, gq, mode=FEATHER, fill=(0, 0, 0)):
    """_strip_mirror.render with every sample times its frame's gain -> (canvas [rows, cols, 3], cover [rows, cols])."""
    frames = np.asarray(frames)
    first, count, x0, y0, rows, cols = segment
    h, w = frames.shape[1:3]
    py, px = np.meshgrid(np.arange(rows, dtype=np.float64) + float(y0), np.arange(cols, dtype=np.float64) + float(x0), indexing="ij")
    num = np.zeros((rows, cols, 3), np.int64)
    den = np.zeros((rows, cols), np.int64)
    cnt = np.zeros((rows, cols), np.int64)
    order = range(first, first + count) if mode != FIRST else range(first + count - 1, first - 1, -1)
    for k in order:
        ok, taps, q = sample(Ginv[k], px, py, w, h)
        P = apply_gain(bilinear(frames[k], taps), gq[k])
        cnt += ok
        if mode == FEATHER:
            num += q[..., None] * P
            den += q
        else:                           # visited so that the winner comes last: it overwrites
            num = np.where(ok[..., None], P, num)
            den = np.where(ok, 1, den)
    out = np.empty((rows, cols, 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    m = den > 0
    if mode == FEATHER:
        out[m] = ((num[m] + 512 * den[m][:, None]) // (1024 * den[m][:, None])).astype(np.uint8)
    else:
        out[m] = ((num[m] + 512) >> 10).astype(np.uint8)
    return out, np.minimum(cnt, 255).astype(np.uint8)


def seam_measure(frames, G, Ginv, seg, gq, lo=5, hi=250):
    """The sum over the pairs of the mean absolute difference, in 8-bit levels, of the two frames' gained samples over the
    pair's valid pixels."""
    total = 0.0
    for k in range(1, len(frames)):
        if seg[k] != seg[k - 1]:
            continue
        Pa, Pb, valid = pair_samples(frames, G, Ginv, k, lo, hi)
        if valid.any():
            total += float(np.abs(apply_gain(Pa[valid], gq[k - 1]) - apply_gain(Pb[valid], gq[k])).mean()) / 1024.0
    return total
