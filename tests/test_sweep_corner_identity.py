"""A fact about cv::CLAHE's blend in the image's four corner cells, on the CPU in float32: where the four neighbouring tiles are
one tile, the blend of the LUT value T with itself rounds back to T wherever the pixel lies,

    RNE(clamp((T*xa1 + T*xa)*ya1 + (T*xa1 + T*xa)*ya)) == T     for every T in 0..255,

with the kernel's own float32 expressions for xa, xa1, ya, ya1 over all columns and rows of the geometries the sweep
meets at 1920x1080 and 3840x2160 (grids 2, 4, 8, 16, 32, padded where cv::CLAHE pads).  The check is separable: the
distinct values of top = fl(fl(T*xa1) + fl(T*xa)) per T first, then fl(fl(top*ya1) + fl(top*ya)) over all ya.  Every
operation is one numpy float32 statement, so nothing is contracted.

A form of k_clahe_sweep that counts corner cells by grey level instead of blending rests on this identity.  It was built and
measured in round 6 and is not in the tree (it did not pay, CHANGELOG); the identity is pinned here for whoever tries again."""
import numpy as np

GRIDS = (2, 4, 8, 16, 32)
SIZES = ((1080, 1920), (2160, 3840))
F32 = np.float32


def _tile(n, g, padded):
    """tile extent along one axis as make_geom (clahe_internal.hpp) has it: cv::CLAHE pads BOTH axes when either needs it"""
    return (n + (g - n % g) if padded else n) // g


def _weights(n, tile):
    """(a, a1) of the coordinates 0..n-1: t = fl(fl(p * inv) - 0.5), a = t - floor(t), a1 = fl(1 - a)"""
    inv = F32(1.0) / F32(tile)
    p = np.arange(n).astype(F32)
    t = p * inv
    t = t - F32(0.5)
    a = t - np.floor(t)
    a1 = F32(1.0) - a
    assert a.dtype == F32 and a1.dtype == F32
    return a, a1


def _all_weights():
    xs, ys = [], []
    for rows, cols in SIZES:
        for g in GRIDS:
            padded = not (cols % g == 0 and rows % g == 0)
            xs.append(_weights(cols, _tile(cols, g, padded)))
            ys.append(_weights(rows, _tile(rows, g, padded)))

    def uniq(pairs):
        a = np.concatenate([p[0] for p in pairs])
        a1 = np.concatenate([p[1] for p in pairs])
        both = np.unique(np.stack([a, a1], axis=1), axis=0)
        return both[:, 0].copy(), both[:, 1].copy()
    return uniq(xs), uniq(ys)


def _blend1(t, a1, a):
    """fl(fl(t * a1) + fl(t * a)), one float32 operation per statement; t: (n, 1), a / a1: (m,)"""
    lo = t * a1
    hi = t * a
    s = lo + hi
    assert s.dtype == F32
    return s


def test_geometries_include_padded_grids():
    assert _tile(1080, 16, True) == 68 and _tile(1920, 16, True) == 121        # 1080 % 16 != 0 pads both axes
    assert _tile(1080, 32, True) == 34 and _tile(1920, 32, True) == 61
    assert _tile(2160, 32, True) == 68 and _tile(3840, 32, True) == 121
    assert _tile(1080, 8, False) == 135 and _tile(3840, 16, False) == 240


def test_blend_of_one_tile_with_itself_rounds_to_its_value():
    (xa, xa1), (ya, ya1) = _all_weights()
    assert xa.size > 1000 and ya.size > 1000
    assert float(xa.min()) >= 0.0 and float(xa.max()) < 1.0 and float(ya.min()) >= 0.0 and float(ya.max()) < 1.0
    worst = 0.0
    for T in range(256):
        t = np.full((1, 1), T, F32)
        tops = np.unique(_blend1(t, xa1, xa))                 # the distinct tops of this T over every column
        res = _blend1(tops.reshape(-1, 1), ya1, ya)           # ... against every row
        worst = max(worst, float(np.abs(res.astype(np.float64) - T).max()))
        out = np.clip(np.rint(res), 0, 255)                   # rint: round half to even, as v_cvt_pk_u8_f32
        assert np.all(out == T), (T, tops, res[out != T][:4])
    # eight roundings of values below 256, each within 2^-24 relative: 8 * 256 * 2^-24 = 2^-13
    assert worst <= 2.0 ** -13, worst
