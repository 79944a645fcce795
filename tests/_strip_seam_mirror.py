"""The strip mosaic's seam finding restated in numpy, for the tests (a plain helper module: no fixtures).  It takes nothing from
csrc/strip_core.hpp; the sampling, the bilinear taps and the gain multiply are _strip_gain_mirror's.  The definitions are

  orient   c = ((w - 1) 0.5, (h - 1) 0.5) goes to the plane under G_{k-1} (d > 0, IEEE divisions, both finite) and from there
           under Ginv_k (d > 0, u, v by division, both finite); dx = cx - u, dy = cy - v, or 0, 0 when a step fails.
           |dy| >= |dx|: axis 0 (steps t = x, states s = y), sign +1 iff dy >= 0; else axis 1 (t = y, s = x), sign from dx.
           orient = axis | (2 if sign < 0).
  cost     pixel (x, y) of frame k goes to the plane under G_k; frame k - 1 is sampled there.  Either fails: C = 1 << 22.
           Pb = gain(1024 pixel, gq_k), Pa = gain(bilinear, gq_{k-1}), D = sum_c |Pa - Pb|; a_k = min(s, S - 1 - s),
           a_p = min(s_p, S - 1 - s_p) with s_p the state coordinate of k - 1's nearest pixel (x + (fx >= 16), y + (fy >= 16));
           C = D + prior |a_k - a_p|, laid out [t][s].
  path     E[0] = C[0]; E[t][s] = C[t][s] + min(E[t-1][s], E[t-1][s-1], E[t-1][s+1]), ties in that order; the end is the
           smallest s among the minima of E[T-1]; seam[t] by walking back.
  render   frames painted in ascending order: a frame paints a pixel it covers where no frame has painted yet, and (not its
           segment's first) where sign (s - seam[t]) >= 0 at its nearest source pixel (t, s).  (P + 512) >> 10."""
import numpy as np

import _strip_gain_mirror as gm
from _strip_mirror import _div

OUTSIDE = 1 << 22
DEFAULT_PRIOR = 1024


def axis_of(o):
    return int(o) & 1


def sign_of(o):
    return -1 if int(o) & 2 else 1


def orient(G, Ginv, k, w, h):
    cx, cy = float(w - 1) * 0.5, float(h - 1) * 0.5
    g, A = [float(v) for v in G[k - 1]], [float(v) for v in Ginv[k]]
    dx = dy = 0.0
    d = ((g[6] * cx) + (g[7] * cy)) + g[8]
    if d > 0.0:
        px, py = _div(((g[0] * cx) + (g[1] * cy)) + g[2], d), _div(((g[3] * cx) + (g[4] * cy)) + g[5], d)
        if np.isfinite(px) and np.isfinite(py):
            d2 = ((A[6] * px) + (A[7] * py)) + A[8]
            if d2 > 0.0:
                u, v = _div(((A[0] * px) + (A[1] * py)) + A[2], d2), _div(((A[3] * px) + (A[4] * py)) + A[5], d2)
                if np.isfinite(u) and np.isfinite(v):
                    dx, dy = cx - u, cy - v
    if abs(dy) >= abs(dx):
        return 0 if dy >= 0.0 else 2
    return 1 if dx >= 0.0 else 3


def pair(frames, G, Ginv, k, gq=None):
    """Frame k against frame k - 1 on k's grid: (valid [h, w], Pa, Pb [h, w, 3] gained, xn, yn [h, w] of k - 1's nearest pixel)."""
    h, w = frames.shape[1:3]
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    g = [np.float64(v) for v in G[k]]
    with np.errstate(all="ignore"):
        d = ((g[6] * x) + (g[7] * y)) + g[8]
        px = (((g[0] * x) + (g[1] * y)) + g[2]) / d
        py = (((g[3] * x) + (g[4] * y)) + g[5]) / d
    ok = (d > 0.0) & np.isfinite(px) & np.isfinite(py)
    cov, taps, _ = gm.sample(Ginv[k - 1], np.where(ok, px, 0.0), np.where(ok, py, 0.0), w, h)
    ga, gb = ((4096,) * 3, (4096,) * 3) if gq is None else (gq[k - 1], gq[k])
    Pa = gm.apply_gain(gm.bilinear(frames[k - 1], taps), ga)
    Pb = gm.apply_gain(1024 * frames[k].astype(np.int64), gb)
    tx, _, ty, _, fx, fy = taps
    return ok & cov, Pa, Pb, tx + (fx >= 16), ty + (fy >= 16)


def cost(frames, G, Ginv, k, axis, gq=None, prior=DEFAULT_PRIOR):
    """-> C [T, S] int64"""
    h, w = frames.shape[1:3]
    valid, Pa, Pb, xn, yn = pair(frames, G, Ginv, k, gq)
    D = np.abs(Pa - Pb).sum(axis=2)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    S, s, sp = (w, xs, xn) if axis else (h, ys, yn)
    ak, ap = np.minimum(s, S - 1 - s), np.minimum(sp, S - 1 - sp)
    C = np.where(valid, D + int(prior) * np.abs(ak - ap), OUTSIDE).astype(np.int64)
    return C if axis else np.ascontiguousarray(C.T)


def path(C):
    """C [T, S] -> (seam [T] int32, total)"""
    C = np.asarray(C, np.int64)
    T, S = C.shape
    big = np.int64(1) << 62
    E = C[0].copy()
    back = np.zeros((T, S), np.int8)
    for t in range(1, T):
        left, right = np.concatenate(([big], E[:-1])), np.concatenate((E[1:], [big]))
        m, bp = E.copy(), np.zeros(S, np.int8)
        take = left < m
        m, bp = np.where(take, left, m), np.where(take, 1, bp)
        take = right < m
        m, bp = np.where(take, right, m), np.where(take, 2, bp)
        back[t] = bp
        E = C[t] + m
    s = int(np.argmin(E))                                   # the first of the minima
    total = int(E[s])
    seam = np.zeros(T, np.int32)
    for t in range(T - 1, -1, -1):
        seam[t] = s
        if t:
            s += (0, -1, 1)[back[t][s]]
    return seam, total


def path_cost(C, seam):
    return int(sum(int(C[t][s]) for t, s in enumerate(seam)))


def seams(frames, G, Ginv, seg, gq=None, prior=DEFAULT_PRIOR, costs=None):
    """-> seam [n, max(w, h)] int32 (-1 beyond T and for a segment's first frame), orient [n] int32, total [n] uint64;
    costs: a dict that receives every pair's C"""
    n, h, w = frames.shape[:3]
    seam, ori, total = np.full((n, max(w, h)), -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)
    for k in range(1, n):
        if seg[k] != seg[k - 1]:
            continue
        ori[k] = orient(G, Ginv, k, w, h)
        C = cost(frames, G, Ginv, k, axis_of(ori[k]), gq, prior)
        sm_, tot = path(C)
        seam[k, :len(sm_)], total[k] = sm_, tot
        if costs is not None:
            costs[k] = C
    return seam, ori, total


def render(frames, Ginv, segment, seam, ori, gq=None, fill=(0, 0, 0), inter=None):
    """-> (canvas [rows, cols, 3], cover [rows, cols]); inter: a dict that receives `winner` [rows, cols] (-1: uncovered), and
    P [count, rows, cols, 3], ok [count, rows, cols] of every frame of the segment"""
    frames = np.asarray(frames)
    first, count, x0, y0, rows, cols = segment
    h, w = frames.shape[1:3]
    py, px = np.meshgrid(np.arange(rows, dtype=np.float64) + float(y0), np.arange(cols, dtype=np.float64) + float(x0), indexing="ij")
    win = np.full((rows, cols), -1, np.int64)
    val = np.zeros((rows, cols, 3), np.int64)
    cnt = np.zeros((rows, cols), np.int64)
    Ps, oks = [], []
    for k in range(first, first + count):
        ok, taps, _ = gm.sample(Ginv[k], px, py, w, h)
        P = gm.bilinear(frames[k], taps)
        if gq is not None:
            P = gm.apply_gain(P, gq[k])
        cnt += ok
        paint = ok & (win < 0)
        if k > first:
            tx, _, ty, _, fx, fy = taps
            xn, yn = tx + (fx >= 16), ty + (fy >= 16)
            t, s = (yn, xn) if axis_of(ori[k]) else (xn, yn)
            paint |= ok & (sign_of(ori[k]) * (s - seam[k][t].astype(np.int64)) >= 0)
        win = np.where(paint, k, win)
        val = np.where(paint[..., None], P, val)
        if inter is not None:
            Ps.append(P)
            oks.append(ok)
    out = np.empty((rows, cols, 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    m = win >= 0
    out[m] = ((val[m] + 512) >> 10).astype(np.uint8)
    if inter is not None:
        inter.update(winner=win, P=np.stack(Ps), ok=np.stack(oks))
    return out, np.minimum(cnt, 255).astype(np.uint8)


def winners_last(ok):
    """ok [count, rows, cols] -> the largest covering index relative to the segment's first frame, -1 where none"""
    idx = np.arange(len(ok))[:, None, None]
    return np.where(ok, idx, -1).max(axis=0)


def seam_measure(P, ok, winner):
    """The mean, in 8-bit levels, of |P_a - P_b| over the pixels where the winner changes between 4-neighbours: for a pixel p
    and its right or lower neighbour q with winners a != b, both frames are sampled at p and at q, wherever both cover the pixel
    (a change where neither pixel has both is a frame's border, not a seam).  Both sides count, so the measure does not favour
    the side a seam's cost was taken on.  winner: indices into P (relative to the segment), -1 = none.  -> (mean, samples)"""
    tot, n = 0.0, 0
    for dy, dx in ((0, 1), (1, 0)):
        a = winner[:winner.shape[0] - dy, :winner.shape[1] - dx]
        b = winner[dy:, dx:]
        ys, xs = np.nonzero((a != b) & (a >= 0) & (b >= 0))
        for y, x in zip(ys, xs):
            ia, ib = int(a[y, x]), int(b[y, x])
            for at in ((y, x), (y + dy, x + dx)):
                if ok[(ia,) + at] and ok[(ib,) + at]:
                    tot += float(np.abs(P[(ia,) + at] - P[(ib,) + at]).mean()) / 1024.0
                    n += 1
    return tot / max(n, 1), n
