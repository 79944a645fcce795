"""k_clahe_sweep on inputs built for its corner cells and its by-grey-level LUT layout: all 5 x 51 output histograms,
count for count, against the histogram of the oracle's CLAHE output.

In a corner cell the four neighbouring tiles are one tile; what the H / tail / group counters receive there depends on how
many of a group's clip limits still clip, so each corner of the plane holds a different regime, and every regime visits
every corner.  The packed LUTs are read as quads of limits from a swizzled [grey][quad] layout: a wrong quad position shows
for one class of v mod 16 only, so the second test makes every class equally likely."""
import numpy as np
import pytest
import torch

from uwimageproc_amd import aclahe

pytestmark = pytest.mark.gpu


def _regime(rng, k, rows, cols):
    if k == 0:
        return (rng.integers(0, 6, (rows, cols)) * 40 + 10).astype(np.uint8)       # 6 grey levels: every limit clips
    if k == 1:
        return (rng.integers(0, 20, (rows, cols)) * 12 + 3).astype(np.uint8)       # ~20 levels: the last group repeats
    if k == 2:
        return rng.integers(0, 256, (rows, cols)).astype(np.uint8)                 # white noise: almost nothing clips
    return np.full((rows, cols), 255, np.uint8)                                    # blown out


def _corner_plane(seed, rows, cols, variant):
    """Four quadrants, split off-centre so that the borders follow no tile grid; corner i (TL, TR, BR, BL) holds regime
    (i + variant) mod 4, so the four variants put each regime into each corner once."""
    rng = np.random.default_rng(seed)
    ry, rx = rows * 5 // 11, cols * 6 // 11
    v = np.empty((rows, cols), np.uint8)
    boxes = [(slice(0, ry), slice(0, rx)), (slice(0, ry), slice(rx, cols)), (slice(ry, rows), slice(rx, cols)), (slice(ry, rows), slice(0, rx))]
    for i, (sy, sx) in enumerate(boxes):
        v[sy, sx] = _regime(rng, (i + variant) % 4, sy.stop - sy.start, sx.stop - sx.start)
    return v


def _band_plane(seed, rows, cols):
    """Blocks of 8 x 8 pixels, each drawing uniformly from one 16-level band [16 b, 16 b + 16) with b uniform per block:
    every class of v mod 16 is equally likely in every tile, and every band occurs."""
    rng = np.random.default_rng(seed)
    band = rng.integers(0, 16, ((rows + 7) // 8, (cols + 7) // 8))
    band = np.repeat(np.repeat(band, 8, axis=0), 8, axis=1)[:rows, :cols]
    return (band * 16 + rng.integers(0, 16, (rows, cols))).astype(np.uint8)


def _check_all_255(ctx, orc, frames):
    t = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    _, hist = aclahe.sweep_histograms(ctx, t)
    hist = hist.cpu().numpy()
    assert hist.shape == (len(frames), len(aclahe.BLOCK_SIZES), len(aclahe.CLIP_LIMITS), 256)
    for f in range(len(frames)):
        for gi, g in enumerate(aclahe.BLOCK_SIZES):
            for ci, cl in enumerate(aclahe.CLIP_LIMITS):
                exp = np.bincount(orc.clahe(frames[f], float(cl), g, g).ravel(), minlength=256)
                assert np.array_equal(hist[f, gi, ci], exp), (f, g, cl)


@pytest.mark.parametrize("variants", [(0, 1), (2, 3)])
@pytest.mark.parametrize("shape", [(64, 96), (97, 161), (135, 240)])
def test_sweep_corner_cells_exact(ctx, orc, shape, variants):
    """(64, 96): corner cells below 512 pixels on every grid; (97, 161): whole groups of 512 pixels plus a
    remainder; (135, 240): padded 16 x 16 and 32 x 32 grids whose last cells are small or empty.  Two frames per call
    (blockIdx.z > 0)."""
    frames = np.stack([_corner_plane(31 + k, shape[0], shape[1], k) for k in variants])
    _check_all_255(ctx, orc, frames)


@pytest.mark.parametrize("shape", [(33, 65), (96, 160), (5, 7)])
def test_sweep_every_grey_class_exact(ctx, orc, shape):
    """Every v mod 16 class equally likely (banded blocks, then plain uniform bytes): the quad swizzle of the packed LUTs, on
    cells from smaller than a wave to several groups of 512."""
    rng = np.random.default_rng(77)
    frames = np.stack([_band_plane(41, *shape), rng.integers(0, 256, shape).astype(np.uint8)])
    _check_all_255(ctx, orc, frames)
