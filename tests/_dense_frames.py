"""Frames that take the overlap detector past its keypoint cap, and a sort-based restatement of the cap rule.

The frames are lattices of small Gaussian dots on a flat background, rendered in integer arithmetic so that every machine
produces the same bytes (each frame is pinned by a CRC32 in the tests).  The detector's contrast factor is one number per
frame, so a lattice of EQUAL dots gives responses that are tied bit for bit; a lattice of jittered dots gives distinct ones.

The restatement (`candidates`, `select`) states the rule and nothing of how the oracle or the device get there: no radix,
no histogram, one sort.
  1. a candidate is a pixel of a level's determinant-of-Hessian map, at least 8 pixels from the border, whose response is
     above the detector threshold, strictly above its 8 neighbours and the 9 + 9 pixels of the adjacent levels, and whose
     2-D quadratic refinement moves it by at most one pixel (float32, the operation order of detect() in
     oracle/uwip_oracle_overlap.c);
  2. thr = the bit pattern of the 2048-th largest response;
  3. the first 2048 candidates in (level, y, x) order with bits >= thr are kept."""
import functools
import zlib

import numpy as np

MAXKP = 2048
BORDER = 8
NLEV = 4
DTHRESH = np.float32(0.001)
KC_REF = np.float32(0.5)

BACKGROUND = 60
SIGMA = 1.6
AMPLITUDE = 120.0
# the dot profile on a half-pixel grid, 12 fractional bits: G[j] = exp(-(j / 2)^2 / (2 sigma^2)), j = 0 .. 16 (+-8 px)
_G = np.rint(4096.0 * np.exp(-(np.arange(17) / 2.0) ** 2 / (2.0 * SIGMA * SIGMA))).astype(np.int64)


def _axis(n, period):
    """dot centres period / 2 + k * period < n along one axis, in half pixels; per centre the pixel range it is stamped
    on (|pixel - centre| <= 8, clipped to the image) and the profile there"""
    out = []
    c2 = period
    while c2 < 2 * n:
        lo, hi = max(0, -((16 - c2) // 2)), min(n - 1, (c2 + 16) // 2)
        out.append((lo, hi + 1, _G[np.abs(2 * np.arange(lo, hi + 1) - c2)]))
        c2 += 2 * period
    return out


def lattice(h, w, period, jitter, seed, keep=None, nudge=None):
    """8UC1 plane: background 60 plus Gaussian dots (sigma 1.6 px) of amplitude 120 + jitter * U(-1, 1), one draw per dot
    in raster order from default_rng(seed), in 1/256 grey levels.  keep: only the first `keep` dots of the raster order are
    drawn.  nudge: (dot index, amplitude change in 1/256 grey levels)."""
    ys, xs = _axis(h, period), _axis(w, period)
    ndots = len(ys) * len(xs)
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, ndots) if jitter else np.zeros(ndots)
    amp = np.rint((AMPLITUDE + float(jitter) * u) * 256.0).astype(np.int64)
    if nudge is not None:
        amp[nudge[0]] += nudge[1]
    acc = np.zeros((h, w), np.int64)                    # 8 + 12 + 12 fractional bits
    for d in range(ndots if keep is None else keep):
        y0, y1, gy = ys[d // len(xs)]
        x0, x1, gx = xs[d % len(xs)]
        acc[y0:y1, x0:x1] += amp[d] * (gy[:, None] * gx[None, :])
    return np.clip(BACKGROUND + ((acc + (1 << 31)) >> 32), 0, 255).astype(np.uint8)


def flat(h, w, level=90):
    return np.full((h, w), level, np.uint8)


def crc(frame):
    return zlib.crc32(np.ascontiguousarray(frame).tobytes())


# The boundary frames: a 240 x 320 lattice of period 8 with a jitter of 5 grey levels has 2080 candidates; dropping dots from
# the end of the raster order takes two candidates away per dot around the boundary (1144 dots: 2049, 1143 dots: 2047), and
# lowering the amplitude of dot 1143 by 5000 / 256 grey levels gives the 2048 in between.  Found by search on the CPU with
# the restatement below; the tests assert the totals.
_boundary = lambda **kw: lattice(240, 320, 8, 5, 2, **kw)

# name -> (builder, CRC32 of the frame).  Shapes: 360 x 640 and 240 x 320 only.
CASES = {
    "under": (lambda: lattice(360, 640, 7, 60, 1), 0xf19daf60),
    "just_over": (lambda: lattice(360, 640, 10, 60, 1), 0x3c423a95),
    "over": (lambda: lattice(360, 640, 8, 60, 1), 0xe21e3683),
    "all_tied": (lambda: lattice(360, 640, 10, 0, 1), 0x35b251c4),
    "tied": (lambda: lattice(360, 640, 8, 0, 1), 0x670fd0cf),
    "flat": (lambda: flat(360, 640), 0x96ec94d9),
    "small_tied": (lambda: lattice(240, 320, 8, 0, 1), 0x8d1b8ba9),
    "b2047": (lambda: _boundary(keep=1143), 0x59553385),
    "b2048": (lambda: _boundary(keep=1144, nudge=(1143, -5000)), 0xc473556d),
    "b2049": (lambda: _boundary(keep=1144), 0x89b736ff),
}
LARGE = ("under", "just_over", "over", "all_tied", "tied", "flat")           # 360 x 640
SMALL = ("small_tied", "b2047", "b2048", "b2049")                            # 240 x 320

# the matcher's input: 360 x 640 crops of one jittered period-8 canvas
CANVAS_CRC = 0x3525881d


@functools.lru_cache(maxsize=None)
def canvas():
    c = lattice(400, 700, 8, 60, 3)
    c.setflags(write=False)
    return c


def crop(dx, dy):
    return np.ascontiguousarray(canvas()[dy:dy + 360, dx:dx + 640])


def gray_to_bgr(g):
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))


@functools.lru_cache(maxsize=None)
def frame(name):
    f = CASES[name][0]()
    f.setflags(write=False)
    return f


# ---- the rule, restated ----------------------------------------------------------------------------------------------
CAND = np.dtype([("level", "i4"), ("yi", "i4"), ("xi", "i4"), ("response", "f4")])


def ldet_levels(orc, gray):
    return [orc.scale_space_level(gray, lv)[3] for lv in range(NLEV)]


def threshold(kcontrast, relative):
    """the detector threshold: 1e-3, or with the relative flag 1e-3 * min(1, (k / 0.5)^2) in float32"""
    if not relative:
        return DTHRESH
    kr = np.float32(kcontrast) / KC_REF
    ks = kr * kr
    if not ks < np.float32(1.0):
        ks = np.float32(1.0)
    return DTHRESH * ks


def candidates(ldet, dthr=DTHRESH):
    """every candidate of the four maps, in (level, y, x) order"""
    h, w = ldet[0].shape
    B = BORDER
    win = lambda D, dy, dx: D[B + dy:h - B + dy, B + dx:w - B + dx]
    f32 = np.float32
    out = []
    for lv in range(NLEV):
        D = ldet[lv]
        v = win(D, 0, 0)
        ok = v > dthr
        for l2 in (lv - 1, lv, lv + 1):
            if l2 < 0 or l2 >= NLEV:
                continue
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if l2 != lv or dy or dx:
                        ok &= v > win(ldet[l2], dy, dx)
        vxp, vxm, vyp, vym = win(D, 0, 1), win(D, 0, -1), win(D, 1, 0), win(D, -1, 0)
        with np.errstate(all="ignore"):
            Dx, Dy = f32(0.5) * (vxp - vxm), f32(0.5) * (vyp - vym)
            Dxx, Dyy = (vxp + vxm) - f32(2.0) * v, (vyp + vym) - f32(2.0) * v
            Dxy = f32(0.25) * (win(D, 1, 1) + win(D, -1, -1)) - f32(0.25) * (win(D, 1, -1) + win(D, -1, 1))
            det = Dxx * Dyy - Dxy * Dxy
            ox, oy = -(Dyy * Dx - Dxy * Dy) / det, -(Dxx * Dy - Dxy * Dx) / det
            ok &= (det != 0) & (np.abs(ox) <= 1) & (np.abs(oy) <= 1)
        assert det.dtype == np.float32 and ox.dtype == np.float32
        yy, xx = np.nonzero(ok)                          # row-major: (y, x) order
        c = np.zeros(len(yy), CAND)
        c["level"], c["yi"], c["xi"], c["response"] = lv, yy + B, xx + B, v[yy, xx]
        out.append(c)
    return np.concatenate(out)


def bits(c):
    return np.ascontiguousarray(c["response"]).view(np.uint32)


def select(c):
    """the candidates the cap keeps"""
    if len(c) <= MAXKP:
        return c
    b = bits(c)
    thr = np.sort(b)[len(b) - MAXKP]
    return c[np.nonzero(b >= thr)[0][:MAXKP]]


def facts(c):
    """what a case exercises: total candidates; for a capped frame the threshold bits, how many are >= / == it, how many
    share its high 16 bits, and how many strictly stronger ones the raster cutoff drops"""
    f = {"total": len(c), "kept": min(len(c), MAXKP)}
    if len(c) > MAXKP:
        b = bits(c)
        thr = np.sort(b)[len(b) - MAXKP]
        ge = np.nonzero(b >= thr)[0]
        f.update(thr=int(thr), ge=len(ge), eq=int((b == thr).sum()), bin16=int(((b >> 16) == (thr >> 16)).sum()),
                 stronger_dropped=int((b[ge[MAXKP:]] > thr).sum()))
    return f


@functools.lru_cache(maxsize=None)
def _case_candidates(name):
    import _oracle
    c = candidates(ldet_levels(_oracle.load(), frame(name)))
    c.setflags(write=False)
    return c


def assert_reaches_its_path(name, f):
    """the property a case is there for, on facts(candidates) of its frame: a frame that no longer reaches its path
    fails here instead of passing vacuously"""
    t = f["total"]
    if name == "under":              # the accept-everything branch, with a real load
        assert MAXKP // 2 < t <= MAXKP, f
    elif name == "flat":
        assert t == 0, f
    elif name in ("b2047", "b2048", "b2049"):
        assert t == int(name[1:]), f
    elif name == "just_over":        # a few hundred dropped, a unique threshold
        assert MAXKP < t < MAXKP + 512 and f["ge"] == MAXKP and f["eq"] == 1, f
    elif name == "over":             # the second pass picks among several candidates of one high-16 bin
        assert t > MAXKP + 1024 and f["ge"] == MAXKP and f["eq"] == 1 and f["bin16"] >= 8, f
    elif name == "all_tied":         # one response value: the raster cutoff alone decides
        assert t > MAXKP and f["eq"] == f["ge"] == t, f
    elif name == "tied":             # a tie at the threshold larger than the cap itself
        assert t > 2 * MAXKP and f["eq"] > MAXKP and f["ge"] == f["eq"], f
    elif name == "small_tied":       # ties at the threshold push strictly stronger candidates past the cutoff
        assert t > MAXKP and f["eq"] >= 2 and f["stronger_dropped"] >= 1, f
    else:
        raise KeyError(name)


def case_candidates(name):
    """candidates of a named case under the default (fixed) threshold, computed once per process"""
    return _case_candidates(name)


@functools.lru_cache(maxsize=None)
def crop_candidates(dx, dy):
    import _oracle
    c = candidates(ldet_levels(_oracle.load(), crop(dx, dy)))
    c.setflags(write=False)
    return c


GUARD = 14336         # entries behind the 2048 the oracle may write: more than any frame here has candidates


def oracle_detect(orc, gray, upright=False, relative_threshold=False):
    """orc.detect_describe() into buffers with a guard zone behind entry 2047: the oracle may not write there"""
    import ctypes as C
    gray = np.ascontiguousarray(gray)
    kps = np.zeros(MAXKP + GUARD, orc.KP)
    desc = np.zeros((MAXKP + GUARD, 64), np.uint8)
    kps.view(np.uint8)[MAXKP * orc.KP.itemsize:] = 0xA5
    desc[MAXKP:] = 0xA5
    kc = C.c_float(0)
    n = orc.lib.orc_detect_describe_ex(gray, gray.shape[0], gray.shape[1], kps.ctypes.data, desc.reshape(-1), C.byref(kc),
                                       (1 if upright else 0) | (16 if relative_threshold else 0))
    assert 0 <= n <= MAXKP
    assert np.all(kps.view(np.uint8)[MAXKP * orc.KP.itemsize:] == 0xA5) and np.all(desc[MAXKP:] == 0xA5), "written past the cap"
    return kps[:n].copy(), desc[:n].copy(), kc.value


def assert_equals_restatement(kps, c):
    """oracle or device keypoints == select(c), exactly, on the fields the restatement states"""
    exp = select(c)
    assert len(kps) == len(exp) == min(len(c), MAXKP)
    for fld in ("level", "yi", "xi"):
        assert np.array_equal(kps[fld], exp[fld]), fld
    assert np.array_equal(np.ascontiguousarray(kps["response"]).view(np.uint32), bits(exp)), "response"
