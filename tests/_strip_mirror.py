"""The strip mosaic's arithmetic restated in numpy, for the tests (a plain helper module: no fixtures).  The chain runs in
Python floats, the render is vectorised over the canvas.  It takes nothing from csrc/strip_core.hpp: the definitions are

  chain    G_first = I; G_k = (G_{k-1} H_k) / (G_{k-1} H_k)[8]; frame k starts a new segment when (1) its pair's ratio is -2.0,
           (2) an entry of G_k is not finite, or a denominator (g x + h y) + G8 is <= 0 at a pixel-centre corner, or a mapped
           corner is not finite, (3) a cross product of consecutive edges of the mapped quad is <= 0, (4) the shoelace area
           leaves [(w-1)(h-1) / s^2, (w-1)(h-1) s^2], (5) the segment's integer box with this frame exceeds the canvas limit.
  sample   plane point (X + x0, Y + y0) under Ginv = adj(G) sign(det G); d > 0; u, v by IEEE division, |u|, |v| < 2^20;
           U = floor(32 u + 0.5); covered iff 0 <= U <= 32 (w - 1) and likewise V; taps (U >> 5, min(. + 1, w - 1)), 5-bit
           fractions; P = sum of taps times 10-bit weights.
  blend    LAST / FIRST: the largest / smallest covering index, (P + 512) >> 10; FEATHER: q = 1 + min(xn, w-1-xn, yn, h-1-yn),
           xn = (U + 16) >> 5, out = (sum q P + 512 sum q) // (1024 sum q).

Every sum of three terms is ((a x) + (b y)) + c; numpy's multiply and add are separate IEEE operations, as are Python's.
There is no culling here: every frame of the segment is sampled at every canvas pixel."""
import math

import numpy as np

FEATHER, FIRST, LAST = 0, 1, 2
MODES = {"feather": FEATHER, "first": FIRST, "last": LAST}


def _adjugate_signed(G):
    A = [G[4] * G[8] - G[5] * G[7], G[2] * G[7] - G[1] * G[8], G[1] * G[5] - G[2] * G[4],
         G[5] * G[6] - G[3] * G[8], G[0] * G[8] - G[2] * G[6], G[2] * G[3] - G[0] * G[5],
         G[3] * G[7] - G[4] * G[6], G[1] * G[6] - G[0] * G[7], G[0] * G[4] - G[1] * G[3]]
    det = ((G[0] * A[0]) + (G[1] * A[3])) + (G[2] * A[6])
    s = -1.0 if det < 0.0 else 1.0
    return [a * s for a in A]


def _div(a, b):
    """IEEE division of Python floats (no ZeroDivisionError)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def map_corners(G, w, h):
    """The mapped pixel-centre corners [(x, y)] * 4, or None when rule 2 breaks."""
    if not all(math.isfinite(g) for g in G):
        return None
    q = []
    for cx, cy in ((0.0, 0.0), (w - 1.0, 0.0), (w - 1.0, h - 1.0), (0.0, h - 1.0)):
        d = ((G[6] * cx) + (G[7] * cy)) + G[8]
        if not d > 0.0:
            return None
        x = _div(((G[0] * cx) + (G[1] * cy)) + G[2], d)
        y = _div(((G[3] * cx) + (G[4] * cy)) + G[5], d)
        if not (math.isfinite(x) and math.isfinite(y)):
            return None
        q.append((x, y))
    return q


def break_rule(G, w, h, max_scale):
    """Which of rules 2-4 a candidate G breaks (0: none) and its mapped corners."""
    q = map_corners(G, w, h)
    if q is None:
        return 2, None
    for i in range(4):
        (x0, y0), (x1, y1), (x2, y2) = q[i], q[(i + 1) % 4], q[(i + 2) % 4]
        if not ((x1 - x0) * (y2 - y1)) - ((y1 - y0) * (x2 - x1)) > 0.0:
            return 3, q
    s = 0.0
    for i in range(4):
        (x0, y0), (x1, y1) = q[i], q[(i + 1) % 4]
        s = s + ((x0 * y1) - (x1 * y0))
    area, a0, s2 = 0.5 * s, float(w - 1) * float(h - 1), float(max_scale) * float(max_scale)
    if not (area >= a0 / s2 and area <= a0 * s2):
        return 4, q
    return 0, q


def chain(H, ratio, w, h, max_rows=16384, max_cols=16384, max_scale=4.0):
    """H [n][9] float64, ratio [n] float32.  Returns a dict: G, Ginv [n, 9] float64; seg [n] int32; box [n, 4] int32;
    segs: list of (first, count, x0, y0, rows, cols); why [n]: the rule that started a segment at that frame (0: joined)."""
    H = np.asarray(H, np.float64).reshape(-1, 9)
    ratio = np.asarray(ratio, np.float32)
    n = len(H)
    G_all, Gi_all, seg, fb, segs, why = [], [], [], [], [], []
    first, sb, Gp = 0, None, None
    max_scale = float(np.float32(max_scale))

    def close(end):
        x0, y0 = int(sb[0]), int(sb[1])
        segs.append((first, end - first, x0, y0, int(sb[3] - sb[1]) + 1, int(sb[2] - sb[0]) + 1))

    for k in range(n):
        rule, G, b, nb = 0, None, None, None
        if k == first and k == 0:
            rule = -1
        elif float(ratio[k]) == -2.0:
            rule = 1
        else:
            Hk = [float(v) for v in H[k]]
            M = [((Gp[3 * i] * Hk[j]) + (Gp[3 * i + 1] * Hk[3 + j])) + (Gp[3 * i + 2] * Hk[6 + j]) for i in range(3) for j in range(3)]
            G = [_div(m, M[8]) for m in M]
            rule, q = break_rule(G, w, h, max_scale)
            if rule == 0:
                xs, ys = [p[0] for p in q], [p[1] for p in q]
                b = [math.floor(min(xs)), math.floor(min(ys)), math.ceil(max(xs)), math.ceil(max(ys))]
                nb = [min(b[0], sb[0]), min(b[1], sb[1]), max(b[2], sb[2]), max(b[3], sb[3])]
                if nb[2] - nb[0] + 1 > max_cols or nb[3] - nb[1] + 1 > max_rows:
                    rule = 5
        if rule != 0:
            if k > first:
                close(k)
            first = k
            G = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
            b = [0, 0, w - 1, h - 1]
            nb = list(b)
        sb, Gp = nb, G
        why.append(max(rule, 0) if k else 0)
        fb.append(b)
        seg.append(len(segs))
        G_all.append(G)
        Gi_all.append(_adjugate_signed(G))
    if n:
        close(n)
    box = np.zeros((n, 4), np.int32)
    for k in range(n):
        _, _, x0, y0, rows, cols = segs[seg[k]]
        b = fb[k]
        box[k] = (min(max(b[0] - 1 - x0, 0), cols - 1), min(max(b[1] - 1 - y0, 0), rows - 1),
                  min(max(b[2] + 1 - x0, 0), cols - 1), min(max(b[3] + 1 - y0, 0), rows - 1))
    return {"G": np.array(G_all, np.float64).reshape(n, 9), "Ginv": np.array(Gi_all, np.float64).reshape(n, 9),
            "seg": np.array(seg, np.int32), "box": box, "segs": segs, "why": why}


def render(frames, Ginv, segment, mode=FEATHER, fill=(0, 0, 0)):
    """frames [n, h, w, 3] uint8 (all frames of the strip), Ginv [n, 9], segment = (first, count, x0, y0, rows, cols).
    Returns (canvas [rows, cols, 3] uint8, cover [rows, cols] uint8)."""
    frames = np.asarray(frames)
    first, count, x0, y0, rows, cols = segment
    h, w = frames.shape[1:3]
    py, px = np.meshgrid(np.arange(rows, dtype=np.float64) + float(y0), np.arange(cols, dtype=np.float64) + float(x0), indexing="ij")
    num = np.zeros((rows, cols, 3), np.int64)
    den = np.zeros((rows, cols), np.int64)
    cnt = np.zeros((rows, cols), np.int64)
    order = range(first, first + count) if mode != FIRST else range(first + count - 1, first - 1, -1)
    with np.errstate(all="ignore"):
        for k in order:
            A = [np.float64(v) for v in Ginv[k]]
            d = ((A[6] * px) + (A[7] * py)) + A[8]
            u = (((A[0] * px) + (A[1] * py)) + A[2]) / d
            v = (((A[3] * px) + (A[4] * py)) + A[5]) / d
            ok = (d > 0.0) & (np.abs(u) < 1048576.0) & (np.abs(v) < 1048576.0)
            U = np.floor((np.where(ok, u, 0.0) * 32.0) + 0.5).astype(np.int64)
            V = np.floor((np.where(ok, v, 0.0) * 32.0) + 0.5).astype(np.int64)
            ok &= (U >= 0) & (U <= 32 * (w - 1)) & (V >= 0) & (V <= 32 * (h - 1))
            U, V = np.where(ok, U, 0), np.where(ok, V, 0)
            x, fx, y, fy = U >> 5, U & 31, V >> 5, V & 31
            x1, y1 = np.minimum(x + 1, w - 1), np.minimum(y + 1, h - 1)
            f = frames[k].astype(np.int64)
            P = (((32 - fx) * (32 - fy))[..., None] * f[y, x] + (fx * (32 - fy))[..., None] * f[y, x1]
                 + ((32 - fx) * fy)[..., None] * f[y1, x] + (fx * fy)[..., None] * f[y1, x1])
            cnt += ok
            if mode == FEATHER:
                xn, yn = (U + 16) >> 5, (V + 16) >> 5
                q = 1 + np.minimum(np.minimum(xn, w - 1 - xn), np.minimum(yn, h - 1 - yn))
                q = np.where(ok, q, 0)
                num += q[..., None] * P
                den += q
            else:                       # visited so that the winner comes last: it overwrites
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
