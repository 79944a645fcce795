"""The multi-band blending's test cases (a plain helper module: no fixtures), shared by the CPU and the GPU tests.  Each case
returns (frames [n, h, w, 3] uint8, H [n, 9] float64, ratio [n] float32, chain keyword arguments) as _strip_cases does;
`expected(name)` and `expected_render(...)` are the mirror's answers, computed once and not to be changed by their users.

  A, C   of _strip_cases: perspective pairs, partial tiles, every segment break.
  D      of _strip_gain_cases, rendered with its solved gains.
  F      four 64 x 96 frames cut 40 px apart from a texture of 2 x 2 pixel blocks and chained with a homography that is wrong by
         (1.5, 1) px: the misregistration the mode is for.  The seam measure is taken here.
  G      300 frames of 9 x 7 one pixel apart in one segment: the listing crosses its chunk of 256 frames, up to nine frames
         cover a pixel.
  H      16 near-identical checker frames of 0 / 255 under the identity with every ramp at 4096: |2 N + W| passes 2^32."""
import functools

import numpy as np

import _strip_band_mirror as bm
import _strip_cases as base
import _strip_gain_cases as gcases
import _strip_mirror as sm

FILL = gcases.FILL
STACK_SIZES = ((5, 7), (53, 37), (70, 20), (72, 20))       # w x h: smaller than every hole distance; odd; across the 64 x 16 tile
                                                           # in both directions with rows of bytes, and with rows of whole words
H_RAMP = (4096, 4096, 4096, 4096)


def stack_frame(w, h):
    return np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)


def case_f():
    n, h, w, pitch = 4, 96, 64, 40
    rng = np.random.default_rng(41)
    sw = w + (n - 1) * pitch
    scene = np.repeat(np.repeat(rng.integers(0, 256, (h // 2, sw // 2 + 1, 3), dtype=np.uint8), 2, axis=0), 2, axis=1)
    frames = np.stack([scene[:, k * pitch:k * pitch + w] for k in range(n)])
    H = np.tile(np.array([1.0, 0, pitch + 1.5, 0, 1.0, 1.0, 0, 0, 1.0]), (n, 1))
    return np.ascontiguousarray(frames), H, np.full(n, 0.5, np.float32), {}


def case_g():
    n, h, w = 300, 7, 9
    assert n > base.CULL_CHUNK
    frames = np.random.default_rng(43).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    H = np.tile(np.array([1.0, 0, 1.0, 0, 1.0, 0, 0, 0, 1.0]), (n, 1))
    return frames, H, np.full(n, 0.5, np.float32), {}


def case_h():
    n, h, w = 16, 20, 24
    rng = np.random.default_rng(47)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    frames = np.repeat(checker[None, :, :, None], n, axis=0).repeat(3, axis=3)
    for k in range(n):                                     # near-identical: three pixels of every frame are flipped
        for _ in range(3):
            y, x = rng.integers(0, h), rng.integers(0, w)
            frames[k, y, x] = 255 - frames[k, y, x]
    H = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]), (n, 1))
    return np.ascontiguousarray(frames), H, np.full(n, 0.5, np.float32), {}


CASES = {"a": base.case_a, "c": base.case_c, "d": gcases.case_d, "f": case_f, "g": case_g, "h": case_h}
# what each case is rendered with: (levels, ramp, gained)
RENDER = {"a": (4, bm.DEFAULT_RAMP, False), "c": (4, bm.DEFAULT_RAMP, False), "d": (4, bm.DEFAULT_RAMP, True),
          "f": (4, bm.DEFAULT_RAMP, False), "g": (4, bm.DEFAULT_RAMP, False), "h": (4, H_RAMP, False)}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, chain, gq [n, 3] or None, stacks [5, n, h, w, 3]) by the mirrors; gq: case D's solved gains."""
    if name == "d":
        case, ch, _, gq, _ = gcases.expected("d")
    else:
        case = CASES[name]()
        frames, H, ratio, kw = case
        ch = sm.chain(H, ratio, frames.shape[2], frames.shape[1], **kw)
        gq = None
    lv = bm.stacks(case[0], 4)
    lv.setflags(write=False)
    case[0].setflags(write=False)
    return case, ch, gq, lv


@functools.lru_cache(maxsize=None)
def expected_render(name, levels=None, ramp=None, gains=None):
    """{segment: (canvas, cover)} and the largest |2 N + W| by the mirror; levels / ramp None: the case's own (RENDER);
    gains: None = the case's own (D: solved, the others: none), or one value for every gain."""
    (frames, _, _, _), ch, gq, lv = expected(name)
    L, R, gained = RENDER[name]
    levels, ramp = L if levels is None else levels, R if ramp is None else ramp
    if gains is not None:
        gq = np.full((len(frames), 3), int(gains), np.int32)
    elif not gained:
        gq = None
    out, big = {}, 0
    for si, s in enumerate(ch["segs"]):
        inter = {}
        out[si] = bm.render(frames, ch["Ginv"], s, levels, ramp, gq, FILL, inter=inter, lv=lv[:levels + 1])
        big = max(big, inter["max_abs_numerator"])
    return out, big


@functools.lru_cache(maxsize=None)
def seam_ratios():
    """Case F: the Laplacian energy over the pixels two or more frames cover, relative to FIRST's -> feather, last, multiband"""
    (frames, _, _, _), ch, _, lv = expected("f")
    seg = ch["segs"][0]
    first, cover = sm.render(frames, ch["Ginv"], seg, sm.FIRST, FILL)
    e0 = bm.laplacian_energy(first, cover)
    r = {}
    for name, mode in (("feather", sm.FEATHER), ("last", sm.LAST)):
        r[name] = bm.laplacian_energy(sm.render(frames, ch["Ginv"], seg, mode, FILL)[0], cover) / e0
    r["multiband"] = bm.laplacian_energy(expected_render("f")[0][0][0], cover) / e0
    return r
