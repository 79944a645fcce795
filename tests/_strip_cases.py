"""The strip mosaic's test cases (a plain helper module: no fixtures), shared by the CPU and the GPU tests.  Each returns
(frames [n, h, w, 3] uint8, H [n, 9] float64, ratio [n] float32, chain keyword arguments); H[k] takes frame k onto frame
k - 1, entry 0 is never read."""
import ctypes as C

import numpy as np

TILE_W, TILE_H = 64, 16          # k_strip_render's tile (csrc/strip.hip: kTileW, kTileH)
CULL_CHUNK = 256                 # frames per pass of its cull list (kCullChunk)
SEED_A = 3


def _frames(rng, n, h, w):
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def case_a(seed=SEED_A):
    """Eight 53 x 37 frames, identity plus perturbations: linear part +-0.03, translation (20, 7) +- 3, perspective +-2e-5."""
    rng = np.random.default_rng(seed)
    n, h, w = 8, 37, 53
    frames = _frames(rng, n, h, w)
    H = np.zeros((n, 9))
    for k in range(n):
        lin = rng.uniform(-0.03, 0.03, 4)
        t = np.array([20.0, 7.0]) + rng.uniform(-3.0, 3.0, 2)
        p = rng.uniform(-2e-5, 2e-5, 2)
        H[k] = [1.0 + lin[0], lin[1], t[0], lin[2], 1.0 + lin[3], t[1], p[0], p[1], 1.0]
    return frames, H, np.full(n, 0.5, np.float32), {}


def case_b(identical=False, n=300):
    """300 frames of 9 x 7 (more than one chunk of the cull list), integer translations of 1-2 px along x -- or none at all, so that
    every pixel is covered 300 times and the cover plane saturates."""
    assert n > CULL_CHUNK
    rng = np.random.default_rng(11)
    h, w = 7, 9
    frames = _frames(rng, n, h, w)
    H = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (n, 1))
    if not identical:
        H[:, 2] = rng.integers(1, 3, n)
        H[:, 5] = (np.arange(n) % 8 == 0)          # one row down every eighth frame: a canvas of a few tile rows
    return frames, H, np.full(n, 0.5, np.float32), {}


def case_c():
    """Twelve pairs with a break of every kind: no homography at 3, a reflection at 5, a 5x zoom at 7, a translation beyond
    max_canvas_cols = 200 at 9."""
    rng = np.random.default_rng(5)
    n, h, w = 12, 37, 53
    frames = _frames(rng, n, h, w)
    H = np.zeros((n, 9))
    ratio = np.full(n, 0.6, np.float32)
    for k in range(n):
        H[k] = [1.0 + 0.01 * rng.uniform(-1, 1), 0.01 * rng.uniform(-1, 1), 15.0 + rng.uniform(-1, 1),
                0.01 * rng.uniform(-1, 1), 1.0 + 0.01 * rng.uniform(-1, 1), 3.0 + rng.uniform(-1, 1), 1e-5 * rng.uniform(-1, 1),
                1e-5 * rng.uniform(-1, 1), 1.0]
    ratio[3] = -2.0
    H[5] = [-1.0, 0, w - 1.0, 0, 1.0, 0, 0, 0, 1.0]
    H[7] = [5.0, 0, 0, 0, 5.0, 0, 0, 0, 1.0]
    H[9] = [1.0, 0, 400.0, 0, 1.0, 0, 0, 0, 1.0]
    return frames, H, ratio, {"max_cols": 200, "max_rows": 16384, "max_scale": 4.0}


C_STARTS = (0, 3, 5, 7, 9)       # where case C's segments begin
C_RULES = {3: 1, 5: 3, 7: 4, 9: 5}


def chain_host(H, ratio, w, h, max_rows=16384, max_cols=16384, max_scale=4.0, cap=None):
    import uwimageproc_amd._native as nat
    l = nat.lib()
    H = np.ascontiguousarray(H, np.float64).reshape(-1, 9)
    ratio = np.ascontiguousarray(ratio, np.float32)
    n = len(H)
    cap = n if cap is None else cap
    G, Gi = np.full((n, 9), np.nan), np.full((n, 9), np.nan)
    seg, box = np.full(n, -1, np.int32), np.full((n, 4), -1, np.int32)
    segs = (nat.StripSegment * max(cap, 1))()
    ns = C.c_int(-1)
    rc = l.uwip_strip_chain_host(w, h, max_rows, max_cols, max_scale, H.ctypes.data, ratio.ctypes.data, n, G.ctypes.data, Gi.ctypes.data,
                                 seg.ctypes.data, box.ctypes.data, segs, cap, C.byref(ns))
    assert rc == nat.UWIP_OK
    return {"G": G, "Ginv": Gi, "seg": seg, "box": box,
            "segs": [(s.first, s.count, s.x0, s.y0, s.rows, s.cols) for s in segs[:min(cap, ns.value)]], "n_segs": ns.value}


def assert_chain_equal(got, exp):
    assert got["segs"] == exp["segs"]
    assert np.array_equal(got["seg"], exp["seg"]) and np.array_equal(got["box"], exp["box"])
    for key in ("G", "Ginv"):                   # bit for bit
        assert np.array_equal(got[key].view(np.uint64), exp[key].view(np.uint64)), key
