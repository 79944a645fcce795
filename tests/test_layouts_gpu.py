"""Every u8 entry point outside the codecs on padded, gapped and misaligned batches (tests/_layouts.py): three distinct
frames, source and destination placed in a canary-filled buffer, in each of the five layouts and in one mixed pair.

Two combinations matter that packed tensors and odd widths never reach: a vector body under padding (step and
frame_stride multiples of 4 / 8 / 16 but larger than a row / a frame), and a fast-path SHAPE whose base, step or
frame_stride diverts the call to the general kernel.  The comparison is the one the entry's packed test makes, with its
tolerance; the 0xA5 padding doubles as the read check (a histogram, window minimum or resize tap that takes padding in
cannot match the oracle), and after every call the canaries are checked: destinations untouched outside their frames,
inputs untouched everywhere."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _knee_mirror as knee_mirror
import _oracle
from _layouts import assert_only_frames_written, place, place_like
from uwimageproc_amd import PipeConfig, batch_of, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import dehaze_oracle as dz  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9                       # the float64 dehaze stages (tests/test_dehaze_gpu.py)
F = 3

# (source layout, destination layout); an in-place entry uses the first
PAIRS = [("packed", "packed"), ("pad16", "pad16"), ("pad8", "pad8"), ("pad4", "pad4"), ("odd", "odd"), ("pad16", "odd")]
PAIR_IDS = [s if s == d else f"{s}-to-{d}" for s, d in PAIRS]
IN_PLACE = ["packed", "pad16", "pad8", "pad4", "odd"]
# (24, 64): every vector form is eligible; (9, 36): cols % 4 == 0 only, rows no multiple of GS3_ROWS; (11, 37): no vector
# form by width, here also under the aligned-padded layouts
PIXEL_SHAPES = [(24, 64), (9, 36), (11, 37)]

pairs = pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
layouts = pytest.mark.parametrize("layout", IN_PLACE)
pixel_shapes = pytest.mark.parametrize("shape", PIXEL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")


class Placed:
    """A batch in a layout, with the copy of its buffer that an input is compared with afterwards."""

    def __init__(self, frames, layout, like=False):
        self.buf, self.view = place_like(frames, layout, "cuda") if like else place(frames, layout, "cuda")
        self.before = self.buf.clone()
        self.b = batch_of(self.view)
        torch.cuda.synchronize()

    @property
    def ref(self):
        return C.byref(self.b)

    def untouched(self):
        assert_only_frames_written(self.buf, self.view, before=self.before)

    def only_frames_written(self):
        assert_only_frames_written(self.buf, self.view)

    def numpy(self):
        return self.view.cpu().numpy()


def _src(frames, layout):
    return Placed(frames, layout)


def _dst(shape, layout):
    return Placed(shape, layout, like=True)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _bgr(shape):
    a = synth.uw_batch(31, F, *shape)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _noise(shape):
    a = np.random.default_rng(shape[0] * 131 + shape[1]).integers(0, 256, (F,) + shape + (3,), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _planes(shape):
    orc = _oracle.load()
    a = np.stack([orc.bgr_to_v(f) for f in _bgr(shape)])
    a[1] = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


# ---- pixel entries ------------------------------------------------------------------------------------------------------------

@pixel_shapes
@pairs
def test_bgr_to_v(ctx, orc, shape, pair):
    src, dst = _src(_bgr(shape), pair[0]), _dst((F,) + shape, pair[1])
    ctx.call("uwip_bgr_to_v", src.ref, dst.ref)
    ctx.sync()
    got = dst.numpy()
    for f in range(F):
        assert np.array_equal(got[f], orc.bgr_to_v(_bgr(shape)[f])), f
    src.untouched(); dst.only_frames_written()


@pytest.mark.parametrize("rule", [0, 1])
@pixel_shapes
@pairs
def test_GaussianBlur3(ctx, orc, shape, pair, rule):
    a = _planes(shape).copy()
    a[2] = (a[2] // 64) * 2                                  # few levels: many exact /16 ties
    src, dst = _src(a, pair[0]), _dst(a.shape, pair[1])
    ctx.call("uwip_GaussianBlur3", src.ref, dst.ref, rule)
    ctx.sync()
    got = dst.numpy()
    for f in range(F):
        assert np.array_equal(got[f], orc.gaussian3(a[f], rule)), f
    src.untouched(); dst.only_frames_written()


@functools.lru_cache(maxsize=None)
def _cvt_cases(shape, space):
    """(input, to_bgr, opencv32, expected) for one space: forward, back from the oracle's forward, and the 3.2 Lab form"""
    orc = _oracle.load()
    img = _noise(shape)
    fwd = np.stack([orc.cvt_space(f, space) for f in img])
    cases = [(img, 0, 0, fwd), (fwd, 1, 0, np.stack([orc.cvt_space(f, space, True) for f in fwd]))]
    if space == 3:
        cases.append((img, 1, 1, np.stack([orc.cvt_space(f, 3, True, opencv32=True) for f in img])))
    return cases


@pytest.mark.parametrize("space", [1, 2, 3, 4])
@pixel_shapes
@pairs
def test_cvtColor_ex(ctx, orc, shape, pair, space):
    for img, to_bgr, rule, exp in _cvt_cases(shape, space):
        src, dst = _src(img, pair[0]), _dst(img.shape, pair[1])
        ctx.call("uwip_cvtColor_ex", src.ref, dst.ref, space, to_bgr, rule)
        ctx.sync()
        assert np.array_equal(dst.numpy(), exp), (to_bgr, rule)
        src.untouched(); dst.only_frames_written()


@pixel_shapes
@pairs
def test_hsv_replace_v(ctx, orc, shape, pair):
    img = _bgr(shape)
    vnew = np.stack([orc.clahe(p, 3.0, 2, 2) for p in _planes(shape)])
    src, v, dst = _src(img, pair[0]), _src(vnew, pair[0]), _dst(img.shape, pair[1])
    ctx.call("uwip_hsv_replace_v", src.ref, v.ref, dst.ref)
    ctx.sync()
    got = dst.numpy()
    for f in range(F):
        assert np.array_equal(got[f], orc.hsv_replace_v(img[f], vnew[f])), f
    src.untouched(); v.untouched(); dst.only_frames_written()
    # the mixed pair once more with the V planes in a third layout
    if pair[0] != pair[1]:
        v, dst = _src(vnew, "pad4"), _dst(img.shape, pair[1])
        ctx.call("uwip_hsv_replace_v", src.ref, v.ref, dst.ref)
        ctx.sync()
        assert np.array_equal(dst.numpy()[2], orc.hsv_replace_v(img[2], vnew[2]))
        src.untouched(); v.untouched(); dst.only_frames_written()


@pixel_shapes
@layouts
def test_hsv_replace_v_without_v_new(ctx, orc, shape, layout):
    """The kernel's other form, every pixel keeping its own V: uwip_hsv_replace_v refuses a null v_new, an HSV letter of
    uwip_histretch is what launches it (the 8-bit round trip, in place)."""
    img = _bgr(shape)
    t = _src(img, layout)
    ctx.call("uwip_histretch", t.ref, b"V", 2, 98)
    ctx.sync()
    got = t.numpy()
    for f in range(F):
        exp, rc = orc.histretch(img[f], "V")
        assert rc == 0 and np.array_equal(got[f], exp), f
        assert np.array_equal(got[f], orc.hsv_replace_v(img[f], orc.bgr_to_v(img[f]))), f
    t.only_frames_written()


@pixel_shapes
@layouts
def test_getHistogram(ctx, orc, shape, layout):
    for frames in (_bgr(shape), _planes(shape)):
        ch = 3 if frames.ndim == 4 else 1
        t = _src(frames, layout)
        hist = torch.full((F, ch, 256), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.call("uwip_getHistogram", t.ref, _ptr(hist))
        ctx.sync()
        h = hist.cpu().numpy()
        for f in range(F):
            for c in range(ch):
                plane = frames[f, ..., c] if ch == 3 else frames[f]
                assert np.array_equal(h[f, c].astype(np.float32), orc.getHistogram(plane)), (f, c)
        t.untouched()


@pixel_shapes
@layouts
def test_apply_lut(ctx, shape, layout):
    """No oracle call exists for the bare LUT pass: the reference is the table look-up itself."""
    rng = np.random.default_rng(7)
    for frames in (_bgr(shape), _planes(shape)):
        ch = 3 if frames.ndim == 4 else 1
        lut = rng.integers(0, 256, (F, ch, 256), dtype=np.uint8)
        t = _src(frames, layout)
        d_lut = torch.from_numpy(lut).cuda()
        torch.cuda.synchronize()
        ctx.call("uwip_apply_lut", t.ref, _ptr(d_lut))
        ctx.sync()
        got = t.numpy()
        for f in range(F):
            for c in range(ch):
                plane = frames[f, ..., c] if ch == 3 else frames[f]
                assert np.array_equal(got[f, ..., c] if ch == 3 else got[f], lut[f, c][plane]), (f, c)
        t.only_frames_written()


@pytest.mark.parametrize("letters,fixed", [("RGB", False), ("RHG", False), ("LaV", False), ("LaV", True)])
@pixel_shapes
@layouts
def test_histretch(ctx, orc, shape, layout, letters, fixed):
    img = _bgr(shape)
    t = _src(img, layout)
    if fixed:
        ctx.call("uwip_histretch_ex", t.ref, letters.encode(), 2, 98, 1)        # UWIP_HISTRETCH_FIXED_ORDER
    else:
        ctx.call("uwip_histretch", t.ref, letters.encode(), 2, 98)
    ctx.sync()
    got = t.numpy()
    for f in range(F):
        if "L" in letters:                                   # Lab letters: the oracle's extended entry (test_hls_lab_letters_and_fixed_order)
            exp = orc.histretch_ex(img[f], letters, fixed_order=fixed)
        else:
            exp, rc = orc.histretch(img[f], letters)
            assert rc == 0
        assert np.array_equal(got[f], exp), f
    t.only_frames_written()


@pixel_shapes
@layouts
def test_imgChannelStretch_plane_and_lane(ctx, orc, shape, layout):
    planes = _planes(shape)
    t = _src(planes, layout)
    ctx.call("uwip_imgChannelStretch", t.ref, 0, 2, 98)
    ctx.sync()
    got = t.numpy()
    for f in range(F):
        exp = planes[f].copy()
        orc.imgChannelStretch(exp, 2, 98)
        assert np.array_equal(got[f], exp), f
    t.only_frames_written()
    img = _bgr(shape)
    t = _src(img, layout)
    ctx.call("uwip_imgChannelStretch", t.ref, 1, 5, 90)
    ctx.sync()
    got = t.numpy()
    for f in range(F):
        exp = img[f].copy()
        orc.imgChannelStretch(exp[..., 1], 5, 90)
        assert np.array_equal(got[f], exp), f
    t.only_frames_written()


@pixel_shapes
@layouts
def test_entropy(ctx, orc, shape, layout):
    planes = _planes(shape)
    t = _src(planes, layout)
    e = torch.zeros(F, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.call("uwip_entropy", t.ref, _ptr(e))
    ctx.sync()
    e = e.cpu().numpy()
    for f in range(F):
        assert abs(float(e[f]) - orc.entropy(planes[f])) <= 1e-5, f
    t.untouched()


@pixel_shapes
@layouts
def test_calcBlur(ctx, orc, shape, layout):
    img = _bgr(shape)
    t = _src(img, layout)
    b = torch.zeros(F, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.call("uwip_calcBlur", t.ref, _ptr(b))
    ctx.sync()
    b = b.cpu().numpy()
    for f in range(F):
        assert abs(float(b[f]) - orc.calcBlur(img[f])) <= 1e-4, f          # test_calcBlur's bound
    t.untouched()


def _smallest_resize_source(ctx):
    """The smallest source shape (by pixel count, then by rows) whose working size is a multiple of 16 wide."""
    for n in range(1, 17):
        for rows in range(1, n + 1):
            if n % rows == 0:
                oh, ow = C.c_int(0), C.c_int(0)
                assert ctx._l.uwip_overlap_working_size(rows, n // rows, C.byref(oh), C.byref(ow)) == 0
                if ow.value % 16 == 0:
                    return (rows, n // rows), (oh.value, ow.value)
    raise AssertionError("no such shape")


@pytest.mark.parametrize("which", ["smallest", "odd_source_width"])
@pairs
def test_resize_bgr(ctx, orc, pair, which):
    """Source and destination sizes are coupled by uwip_overlap_working_size, and the working width is 640 for EVERY source
    width (test_layouts_helper.py asserts it), so no source shape gives an odd destination width: the second shape has an odd
    SOURCE width instead (1283 columns down to 640, 22 rows), the first is the smallest source there is."""
    if which == "smallest":
        sshape, dshape = _smallest_resize_source(ctx)
    else:
        sshape = (45, 1283)
        dshape = orc.resize_dims(*sshape)
    assert dshape[1] == 640
    img = _noise(sshape)
    src, dst = _src(img, pair[0]), _dst((F,) + dshape + (3,), pair[1])
    ctx.call("uwip_resize_bgr", src.ref, dst.ref)
    ctx.sync()
    got = dst.numpy()
    for f in range(F):
        assert np.array_equal(got[f], orc.resize_bgr(img[f])), f
    src.untouched(); dst.only_frames_written()


# ---- CLAHE --------------------------------------------------------------------------------------------------------------------

# (128, 256) under (2, 2): 8192-pixel tiles, the BP tile-histogram form when aligned, the slot-keyed one when not;
# (33, 32) under (32, 32): one-pixel-wide tiles, the band kernels
CLAHE_GEOMETRIES = [((128, 256), (2, 2)), ((128, 256), (8, 8)), ((45, 80), (4, 4)), ((33, 32), (32, 32))]
CLAHE_SHAPES = [(128, 256), (45, 80), (33, 32)]
PER_FRAME = [(2.0, 2), (3.5, 8), (0.5, 32)]                  # (clip limit, grid) of frames 0, 1, 2
clahe_shapes = pytest.mark.parametrize("shape", CLAHE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")


@functools.lru_cache(maxsize=None)
def _clahe_ref(shape, grid, clip):
    orc = _oracle.load()
    return [orc.clahe(p, clip, grid[0], grid[1], 0, want_luts=True) for p in _planes(shape)]


@pytest.mark.parametrize("shape,grid", CLAHE_GEOMETRIES, ids=lambda v: f"{v[0]}x{v[1]}")
@pairs
def test_clahe_luts_and_apply(ctx, shape, grid, pair):
    planes = _planes(shape)
    ref = _clahe_ref(shape, grid, 2.5)
    src, dst = _src(planes, pair[0]), _dst(planes.shape, pair[1])
    luts = torch.zeros((F, grid[0] * grid[1], 256), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.call("uwip_clahe_luts", src.ref, C.c_double(2.5), grid[0], grid[1], 0, _ptr(luts))
    ctx.call("uwip_clahe", src.ref, dst.ref, C.c_double(2.5), grid[0], grid[1], 0)
    ctx.sync()
    luts, got = luts.cpu().numpy(), dst.numpy()
    for f in range(F):
        assert np.array_equal(luts[f], ref[f][1]), f
        assert np.array_equal(got[f], ref[f][0]), f
    src.untouched(); dst.only_frames_written()


@clahe_shapes
@pairs
def test_clahe_per_frame(ctx, orc, shape, pair):
    planes = _planes(shape)
    src, dst = _src(planes, pair[0]), _dst(planes.shape, pair[1])
    cl = (C.c_double * F)(*[c for c, _ in PER_FRAME])
    gr = (C.c_int32 * F)(*[g for _, g in PER_FRAME])
    ctx.call("uwip_clahe_per_frame", src.ref, dst.ref, cl, gr, 0)
    ctx.sync()
    got = dst.numpy()
    for f, (c, g) in enumerate(PER_FRAME):
        assert np.array_equal(got[f], orc.clahe(planes[f], c, g, g)), f
    src.untouched(); dst.only_frames_written()


@functools.lru_cache(maxsize=None)
def _sweep_ref(shape):
    """per frame: the oracle's entropy table and all 5 x 51 output histograms"""
    orc = _oracle.load()
    tabs, hists = [], []
    for p in _planes(shape):
        tabs.append(orc.sweep(p))
        hists.append(np.stack([np.stack([np.bincount(orc.clahe(p, 0.5 * ci, g, g).ravel(), minlength=256) for ci in range(51)])
                               for g in (2, 4, 8, 16, 32)]))
    return tabs, hists


@clahe_shapes
@layouts
def test_aclahe_sweep_and_sweep_hist(ctx, shape, layout):
    tabs, hists = _sweep_ref(shape)
    t = _src(_planes(shape), layout)
    ent = torch.zeros((F, 5, 51), dtype=torch.float32, device="cuda")
    ent2 = torch.zeros((F, 5, 51), dtype=torch.float32, device="cuda")
    hist = torch.zeros((F, 5, 51, 256), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.call("uwip_aclahe_sweep", t.ref, 0, _ptr(ent))
    ctx.call("uwip_aclahe_sweep_hist", t.ref, 0, _ptr(ent2), _ptr(hist))
    ctx.sync()
    assert torch.equal(ent, ent2)
    ent, hist = ent.cpu().numpy(), hist.cpu().numpy()
    for f in range(F):
        assert np.abs(ent[f] - tabs[f]).max() <= 1e-5, f
        assert np.array_equal(hist[f], hists[f]), f
    t.untouched()


@functools.lru_cache(maxsize=None)
def _auto_ref(shape):
    orc = _oracle.load()
    out = []
    for p in _planes(shape):
        filt = orc.gaussian3(p)
        # a clip limit outside the swept grid: the exact entropies, as uwip_aclahe_auto_ex evaluates them
        exact = lambda g, c: orc.entropy(orc.clahe(filt, c, (2, 4, 8, 16, 32)[g], (2, 4, 8, 16, 32)[g]))
        bs, cl = knee_mirror.select_parameters(orc.sweep(filt), entropy_at=exact)
        out.append(((bs, cl), orc.clahe(p, float(cl), bs, bs)))
    return out


@clahe_shapes
@pairs
def test_aclahe_auto_ex(ctx, shape, pair):
    """UWIP_ACLAHE_PREFILTER, the form the pipe runs: blur, sweep and choice on the source, the final CLAHE into dst"""
    planes = _planes(shape)
    ref = _auto_ref(shape)
    src, dst = _src(planes, pair[0]), _dst(planes.shape, pair[1])
    bs, cl = (C.c_int32 * F)(), (C.c_int32 * F)()
    ctx.call("uwip_aclahe_auto_ex", src.ref, dst.ref, 0, 1, bs, cl)
    ctx.sync()
    got = dst.numpy()
    for f in range(F):
        assert (bs[f], cl[f]) == ref[f][0], (f, bs[f], cl[f], ref[f][0])
        assert np.array_equal(got[f], ref[f][1]), f
    src.untouched(); dst.only_frames_written()


# ---- dehaze -------------------------------------------------------------------------------------------------------------------

# (96, 272): rows above the guided filter's 81-row minimum, cols % 16 == 0, one seam of every strip width in use;
# (83, 257): no vector form by width, under the aligned-padded layouts only
DEHAZE_CASES = [((96, 272), p) for p in PAIRS] + [((83, 257), p) for p in PAIRS if "odd" not in p and p[0] != "packed"]
DEHAZE_IDS = [f"{s[0]}x{s[1]}-{p[0] if p[0] == p[1] else p[0] + '-to-' + p[1]}" for s, p in DEHAZE_CASES]
dehaze_cases = pytest.mark.parametrize("shape,pair", DEHAZE_CASES, ids=DEHAZE_IDS)


@functools.lru_cache(maxsize=None)
def _dehaze_ref(shape):
    out = []
    for img in _bgr(shape):
        normI = dz.normalize_input(img)
        B, idx = dz.background_light(normI, 15)
        out.append({"normI": normI, "B": B, "idx": list(idx), "traw": dz.transmission_map(normI, B),
                    "refined": dz.refined_t(normI, B), "restored": dz.RC_correction(normI, 15)})
    return out


@functools.lru_cache(maxsize=None)
def _gf_ref(shape, r):
    p = np.random.default_rng(5).random((F,) + shape)
    return p, [dz.guided_filter(dz.normalize_input(img), p[f], r, 1e-3) for f, img in enumerate(_bgr(shape))]


def _profiled(ctx, fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    try:
        fn()
        ctx.sync()
        return ctx.prof_results()
    finally:
        ctx.prof_enable(False)


def _expect_winfilter15(shape, layout):
    return shape[1] % 4 == 0 and layout != "odd"


@dehaze_cases
def test_dehaze_background_light_and_transmission(ctx, shape, pair):
    """Both are input-only entries (the source layout of the pair is what counts).  The profile says which window filter ran:
    k_winfilter15 under packed / pad16 / pad8 / pad4 at 272 columns, the general k_winfilter under `odd` and at 257 columns --
    so neither case silently exercises the other's path."""
    ref = _dehaze_ref(shape)
    src = _src(_bgr(shape), pair[0])
    B = torch.zeros((F, 3), dtype=torch.float64, device="cuda")
    idx = torch.zeros((F, 2), dtype=torch.int32, device="cuda")
    t = torch.zeros((F, 2) + shape, dtype=torch.float64, device="cuda")
    Bo = torch.from_numpy(np.stack([r["B"] for r in ref])).cuda()
    torch.cuda.synchronize()
    prof = _profiled(ctx, lambda: ctx.call("uwip_dehaze_background_light", src.ref, 15, _ptr(B), _ptr(idx)))
    assert ("k_winfilter15" in prof) == _expect_winfilter15(shape, pair[0]), sorted(prof)
    assert ("k_winfilter<max>" in prof) != _expect_winfilter15(shape, pair[0]), sorted(prof)
    print(f"{shape} {pair[0]}: uwip_dehaze_background_light ran {sorted(k for k in prof if 'winfilter' in k)}")
    prof = _profiled(ctx, lambda: ctx.call("uwip_dehaze_transmission", src.ref, _ptr(Bo), _ptr(t)))
    assert ("k_winfilter15" in prof) == _expect_winfilter15(shape, pair[0]), sorted(prof)
    B, idx, t = B.cpu().numpy(), idx.cpu().numpy(), t.cpu().numpy()
    for f in range(F):
        assert idx[f].tolist() == ref[f]["idx"], f
        assert np.abs(B[f] - ref[f]["B"]).max() <= 1e-15, f
        assert np.abs(t[f, 0] - ref[f]["traw"][:, :, 0]).max() <= 1e-12 and np.abs(t[f, 1] - ref[f]["traw"][:, :, 1]).max() <= 1e-12, f
    src.untouched()


@pytest.mark.parametrize("r", [40, 12])
@dehaze_cases
def test_guided_filter(ctx, shape, pair, r):
    p, qo = _gf_ref(shape, r)
    src = _src(_bgr(shape), pair[0])
    dp = torch.from_numpy(p).cuda()
    q = torch.zeros_like(dp)
    torch.cuda.synchronize()
    ctx.call("uwip_guided_filter", src.ref, _ptr(dp), r, C.c_double(1e-3), _ptr(q))
    ctx.sync()
    q = q.cpu().numpy()
    for f in range(F):
        assert np.abs(q[f] - qo[f]).max() <= TOL, (f, float(np.abs(q[f] - qo[f]).max()))
    src.untouched()


@dehaze_cases
def test_dehaze_rc_correction_and_full(ctx, shape, pair):
    """uwip_dehaze without UWIP_DEHAZE_FULL, both taps wanted (the unfused recovery), then the full chain with the guard: the
    exposure tail is ill-conditioned against 1-ulp differences upstream (test_exposure_tail_in_isolation), so it is checked
    on the device's own RC_correction output, as there."""
    ref = _dehaze_ref(shape)
    src, dst = _src(_bgr(shape), pair[0]), _dst((F,) + shape + (3,), pair[1])
    rt = torch.zeros((F, 2) + shape, dtype=torch.float64, device="cuda")
    fo = torch.zeros((F,) + shape + (3,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    prof = _profiled(ctx, lambda: ctx.call("uwip_dehaze", src.ref, dst.ref, 15, 0, None, _ptr(rt), _ptr(fo)))
    assert ("k_winfilter15" in prof) == _expect_winfilter15(shape, pair[0]), sorted(prof)
    rt, restored, got = rt.cpu().numpy(), fo.cpu().numpy(), dst.numpy()
    for f in range(F):
        tb, tg = ref[f]["refined"]
        assert np.abs(rt[f, 0] - tb).max() <= TOL and np.abs(rt[f, 1] - tg).max() <= TOL, f
        assert np.abs(restored[f] - ref[f]["restored"]).max() <= TOL, f
        _oracle.assert_u8_differs_only_at_rounding_ties(got[f], ref[f]["restored"], what=f"RC u8, frame {f}")
    src.untouched(); dst.only_frames_written()
    # the fused recovery (no refined-t tap) must give the same float image
    dst = _dst((F,) + shape + (3,), pair[1])
    fo2 = torch.zeros_like(fo)
    torch.cuda.synchronize()
    ctx.call("uwip_dehaze", src.ref, dst.ref, 15, 0, None, None, _ptr(fo2))
    ctx.sync()
    fo2 = fo2.cpu().numpy()
    for f in range(F):
        assert np.abs(fo2[f] - ref[f]["restored"]).max() <= TOL, f
        _oracle.assert_u8_differs_only_at_rounding_ties(dst.numpy()[f], ref[f]["restored"], what=f"fused RC u8, frame {f}")
    src.untouched(); dst.only_frames_written()
    # UWIP_DEHAZE_FULL | UWIP_DEHAZE_GUARD_S
    dst = _dst((F,) + shape + (3,), pair[1])
    ff = torch.zeros_like(fo)
    torch.cuda.synchronize()
    ctx.call("uwip_dehaze", src.ref, dst.ref, 15, 3, None, None, _ptr(ff))
    ctx.sync()
    ff, got = ff.cpu().numpy(), dst.numpy()
    for f in range(F):
        exp = dz.adaptiveExp_tail(ref[f]["normI"], fo2[f], guard_s=True)
        assert not np.isnan(exp).any()
        assert np.abs(ff[f] - exp).max() <= TOL, (f, float(np.abs(ff[f] - exp).max()))
        _oracle.assert_u8_differs_only_at_rounding_ties(got[f], exp, what=f"FULL u8, frame {f}")
    src.untouched(); dst.only_frames_written()


@dehaze_cases
def test_dehaze_histretch(ctx, orc, shape, pair):
    """The chained call against the two calls (test_chained_dehaze_histretch_equals_two_calls), the two calls themselves on
    placed batches as well; and the stretch against the oracle on the device's own dehazed bytes."""
    src = _src(_bgr(shape), pair[0])
    one, two = _dst((F,) + shape + (3,), pair[1]), _dst((F,) + shape + (3,), pair[1])
    ctx.call("uwip_dehaze", src.ref, two.ref, 15, 3, None, None, None)
    ctx.sync()
    dehazed = two.numpy()
    ctx.call("uwip_histretch_ex", two.ref, b"RGB", 2, 98, 0)
    ctx.call("uwip_dehaze_histretch", src.ref, one.ref, 15, 3, b"RGB", 2, 98, 0)
    ctx.sync()
    got = one.numpy()
    assert np.array_equal(got, two.numpy())
    for f in range(F):
        exp, rc = orc.histretch(dehazed[f], "RGB")
        assert rc == 0 and np.array_equal(got[f], exp), f
    src.untouched(); one.only_frames_written(); two.only_frames_written()


# ---- overlap ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _overlap_ref():
    orc = _oracle.load()
    frames = synth.uw_stream(3, F, 480, 640)
    gray = np.stack([orc.resize_gray(f) for f in frames])
    return frames, gray, [orc.detect_describe(g)[:2] for g in gray]


@pytest.mark.parametrize("kind", ["bgr", "gray"])
@pytest.mark.parametrize("layout", ["packed", "pad16", "odd"])
def test_overlap_detect(ctx, layout, kind):
    from uwimageproc_amd import videostrip as vs
    frames, gray, ref = _overlap_ref()
    assert gray.shape[1:] == (480, 640)
    src = _src(frames if kind == "bgr" else gray, layout)
    feats = vs.Features(ctx, F)
    ctx.call("uwip_overlap_detect", src.ref, feats._h, 0)
    ctx.sync()
    for s in range(F):
        kps, desc = feats.download(s)
        ek, ed = ref[s]
        assert len(kps) == len(ek) and len(kps) > 30
        for fld in ("xi", "yi", "level", "x", "y", "response", "co", "si"):
            assert np.array_equal(kps[fld], ek[fld]), (s, fld)
        assert np.array_equal(desc, ed), s
    feats.close()
    src.untouched()


# ---- the chain ----------------------------------------------------------------------------------------------------------------

def test_pipe_step_on_placed_batches(ctx):
    """One uwip_pipe_step at 270 x 480, two frames: `in` pad16 and `out` odd give the bytes, ratios and (BS, CL) of the same step
    on packed buffers (whose parity test_pipe_c_abi_reference_defaults_step_and_host_form pins)."""
    Fp, H, W = 2, 270, 480
    frames = synth.uw_stream(0, Fp, H, W)
    l = ctx._l
    cfg = PipeConfig()
    assert l.uwip_pipe_config_default(C.byref(cfg), Fp, H, W) == 0
    cfg.videoWidth, cfg.videoHeight = 640, 480
    results = []
    for lin, lout in (("packed", "packed"), ("pad16", "odd")):
        h = C.c_void_p()
        ctx.call("uwip_pipe_create", C.byref(cfg), None, C.byref(h))
        src, dst = _src(frames, lin), _dst(frames.shape, lout)
        ratio = torch.zeros(Fp, dtype=torch.float32, device="cuda")
        info = torch.zeros((Fp, 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        try:
            rc = l.uwip_pipe_step(h, src.ref, dst.ref, _ptr(ratio), _ptr(info))
            assert rc == 0, l.uwip_pipe_last_error(h)
            bs, cl = (C.c_int32 * Fp)(), (C.c_int32 * Fp)()
            assert l.uwip_pipe_last_params(h, bs, cl) == 0
            assert l.uwip_pipe_sync(h) == 0
        finally:
            l.uwip_pipe_destroy(h)
        src.untouched(); dst.only_frames_written()
        results.append((dst.numpy(), ratio.cpu().numpy(), info.cpu().numpy(), list(zip(bs, cl))))
    a, b = results
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2])
    assert a[3] == b[3]
    assert a[0].std() > 10                                   # a real image came out


# ---- aliasing the ABI allows --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["pad16", "odd"])
def test_cvtColor_and_hsv_replace_v_in_place(ctx, orc, layout):
    """include/uwip.h: "dst may alias src" (uwip_cvtColor), "bgr_out may alias bgr" (uwip_hsv_replace_v), and the launchers
    hold no refusal (uwip_GaussianBlur3 has one): the in-place call gives the out-of-place result."""
    shape = (24, 64)
    img = _noise(shape)
    for space in (1, 2, 3, 4):
        for inp, to_bgr, rule, exp in _cvt_cases(shape, space):
            if rule:
                continue                                     # uwip_cvtColor is the 3.4.x form
            t = _src(inp, layout)
            ctx.call("uwip_cvtColor", t.ref, t.ref, space, to_bgr)
            ctx.sync()
            assert np.array_equal(t.numpy(), exp), (space, to_bgr)
            t.only_frames_written()
    vnew = np.stack([orc.clahe(p, 3.0, 2, 2) for p in _planes(shape)])
    t, v = _src(img, layout), _src(vnew, layout)
    ctx.call("uwip_hsv_replace_v", t.ref, v.ref, t.ref)
    ctx.sync()
    got = t.numpy()
    for f in range(F):
        assert np.array_equal(got[f], orc.hsv_replace_v(img[f], vnew[f])), f
    t.only_frames_written(); v.untouched()
