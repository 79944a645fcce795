"""GPU: uwip_png_encode (csrc/png_encode.hip) through the C ABI and uwimageproc_amd.png.  Every stream is checked without this
project's code (tests/_png_streams.py): Pillow decodes it to the input's pixels, zlib inflates its IDATs to exactly the
filtered bytes the rule of include/uwip.h gives in numpy, and it keeps to uwip_png_bound; a slot one byte short is a status.
Being lossless is not enough, so the size of the zlib stream is held against zlib's own Z_RLE deflate of the same bytes."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import _png_streams as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
REAL = os.path.join(ROOT, "tests", "golden", "real")

pytestmark = pytest.mark.gpu


def _noise(shape, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _constant(shape):
    return np.full(shape, 93, np.uint8)


def _ramp(shape):
    img = np.zeros(shape, np.uint8)
    img[...] = (np.arange(shape[1]) % 256).reshape((1, -1) + (1,) * (len(shape) - 2))
    return img


def _checker(shape):
    img = (((np.indices(shape[:2]).sum(0)) & 1) * 200 + 20).astype(np.uint8)
    return img if len(shape) == 2 else np.ascontiguousarray(np.repeat(img[..., None], 3, 2))


def _fibonacci(shape):
    """Grey: byte values whose counts follow 1, 1, 2, 3, 5, ... (shuffled, so they stay literals): 22 symbols in 66 600 bytes,
    an unlimited Huffman code of depth 21."""
    n = shape[0] * shape[1]
    vals, a, b, s = [], 1, 1, 0
    while len(vals) < n:
        vals += [s * 7 + 3] * min(a, n - len(vals))
        a, b, s = b, a + b, s + 1
    v = np.array(vals, np.uint8)
    np.random.default_rng(5).shuffle(v)
    return v.reshape(shape)


def _photo(shape):
    img = np.asarray(Image.open(os.path.join(REAL, "in_BUL_T1A_0028.jpg")).convert("RGB"))[400:400 + shape[0], 800:800 + shape[1], ::-1]
    return np.ascontiguousarray(img if len(shape) == 3 else img[..., 1])


SHAPES = [(1, 1), (1, 300), (300, 1), (5, 7, 3), (97, 113, 3), (200, 333)]
CONTENTS = {"noise": _noise, "constant": _constant, "ramp": _ramp, "checker": _checker}


def _encode(ctx, frames, filt=-1, slot=None):
    """frames [F, H, W(, 3)] -> (list of streams or None where the slot is too small, sizes)"""
    import torch
    import uwimageproc_amd as uw
    dev = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    H, W = int(dev.shape[1]), int(dev.shape[2])
    if slot is None:
        slot = uw.png.bound(H, W, 3 if dev.dim() == 4 else 1)
    streams, sizes = uw.png.encode_device(ctx, dev, filt, slot_bytes=slot)
    ctx.sync()
    sizes = sizes.cpu().tolist()
    flat = streams.cpu().numpy()
    return [flat[f, :sizes[f]].tobytes() if sizes[f] > 0 else None for f in range(len(sizes))], sizes, flat


def _bound(img):
    import uwimageproc_amd as uw
    return uw.png.bound(img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_shape_content_and_filter(ctx, shape):
    import uwimageproc_amd as uw
    chunk = uw.png.chunk_bytes()
    frames = np.stack([fn(shape) for fn in CONTENTS.values()])
    for filt in (-1, 0, 1, 2, 3, 4):
        streams, sizes, _ = _encode(ctx, frames, filt)
        for f, name in enumerate(CONTENTS):
            ps.check_stream(streams[f], frames[f], filt, _bound(frames[f]), chunk)
    # the wrapper's default: adaptive, its own slots (the noise frame outgrows the raw size: the second pass with the bound)
    import torch
    assert uw.png.encode(ctx, torch.from_numpy(frames).cuda()) == _encode(ctx, frames, -1)[0]
    # noise is stored: nothing gained, and no more lost than the per-chunk and per-frame constants
    z, raw = ps.check_stream(_encode(ctx, frames[:1], 0)[0][0], frames[0], 0, _bound(frames[0]), chunk)
    assert len(z) <= len(raw) + 10 * (-(-len(raw) // chunk)) + 6


def test_fibonacci_counts_need_the_length_limit(ctx):
    import uwimageproc_amd as uw
    img = _fibonacci((200, 333))
    streams, _, _ = _encode(ctx, img[None], 0)
    z, raw = ps.check_stream(streams[0], img, 0, _bound(img), uw.png.chunk_bytes())
    assert len(z) <= 1.02 * ps.rle_reference_bytes(raw, uw.png.chunk_bytes()) + 6


def test_photograph_crop_ramp_and_constant_are_as_small_as_zlib_rle(ctx):
    """zlib-stream length <= 1.02 x (zlib's Z_RLE raw deflate, level 6, one fresh object per chunk, Z_FULL_FLUSH) + 6 bytes of
    header and Adler-32: the coder differs from that reference only in block structure and in tie order among equal counts."""
    import uwimageproc_amd as uw
    chunk = uw.png.chunk_bytes()
    for img in (_photo((96, 128, 3)), _photo((96, 128)), _ramp((97, 113, 3)), _constant((97, 113, 3)), _ramp((200, 333)), _constant((200, 333))):
        z, raw = ps.check_stream(_encode(ctx, img[None])[0][0], img, -1, _bound(img), chunk)
        ref = ps.rle_reference_bytes(raw, chunk)
        print(img.shape, "zlib stream", len(z), "zlib Z_RLE per chunk", ref, "ratio %.4f" % (len(z) / ref))
        assert len(z) <= 1.02 * ref + 6, (img.shape, len(z), ref)


@pytest.mark.parametrize("ch", [3, 1])
def test_padded_batch_and_a_slot_one_byte_short(ctx, ch):
    """3 frames, a padded step, an odd frame_stride, a base pointer off by 1; then every frame in turn gets a slot one byte short:
    it reports minus the length it has with a sufficient slot and leaves its slot alone, and its neighbours do not change."""
    import torch
    import uwimageproc_amd as uw
    F, H, W = 3, 97, 113
    shape = (H, W, 3) if ch == 3 else (H, W)
    frames = np.stack([_photo(shape), _constant(shape), _checker(shape)])
    packed, lens, _ = _encode(ctx, frames)
    for f in range(F):
        ps.check_stream(packed[f], frames[f], -1, _bound(frames[f]), uw.png.chunk_bytes())
    step, fs, off = W * ch + 13, (W * ch + 13) * H + 1001, 1
    buf = torch.full((off + F * fs + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + off) % 2 == 1 and fs % 2 == 1
    view = torch.as_strided(buf, (F, H, W, ch), (fs, step, ch, 1), off)
    view.copy_(torch.from_numpy(frames.reshape(F, H, W, ch)).cuda())
    b = uw.batch_of(view)
    assert (b.step, b.frame_stride) == (step, fs)
    dev = view if ch == 3 else view[..., 0]
    assert _encode(ctx, dev)[0] == packed
    assert len(set(lens)) == 3
    for short in range(F):
        slot = lens[short] - 1
        streams = torch.full((F, slot), 0xEE, dtype=torch.uint8, device="cuda")
        sizes = torch.zeros((F,), dtype=torch.int64, device="cuda")
        ctx.call("uwip_png_encode", __import__("ctypes").byref(b), -1, uw._native._P(streams.data_ptr()), slot, uw._native._P(sizes.data_ptr()))
        ctx.sync()
        got, flat = sizes.cpu().tolist(), streams.cpu().numpy()
        for f in range(F):
            if lens[f] <= slot:
                assert got[f] == lens[f] and flat[f, :lens[f]].tobytes() == packed[f], (short, f)
                assert (flat[f, lens[f]:] == 0xEE).all()
            else:
                assert got[f] == -lens[f], (short, f)
                assert (flat[f] == 0xEE).all(), (short, f)
        assert got[short] == -lens[short]
    # the C entry itself: a filter outside -1 .. 4 is UWIP_ERR_INVALID
    import ctypes as C
    import uwimageproc_amd._native as nat
    n = torch.zeros((F,), dtype=torch.int64, device="cuda")
    assert nat.lib().uwip_png_encode(ctx._h, C.byref(b), 5, None, 0, C.c_void_p(n.data_ptr())) == nat.UWIP_ERR_INVALID


def test_pngenc_check_reads_the_stream_back_with_the_host_reader(tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)
    p = str(tmp_path / "a.ppm")
    img = _photo((96, 128, 3))
    open(p, "wb").write(b"P6\n128 96\n255\n" + np.ascontiguousarray(img[..., ::-1]).tobytes())
    for extra in ([], ["grey"], ["--filter", "4"]):
        r = subprocess.run([os.path.join(BIN, "pngenc_check"), p] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("lossless "), r.stdout + r.stderr


def test_uwpipe_device_png_writes_the_pixels_of_png(tmp_path):
    from uwimageproc_amd import synth
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)
    n, B, H, W = 4, 2, 135, 240
    names = []
    for i, f in enumerate(synth.uw_stream(0, n, H, W)):
        names.append(str(tmp_path / f"in{i}.ppm"))
        open(names[-1], "wb").write(b"P6\n%d %d\n255\n" % (W, H) + np.ascontiguousarray(f[..., ::-1]).tobytes())
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(names) + "\n")
    out = {}
    for flag in ("--png", "--device-png"):
        d = tmp_path / flag.strip("-")
        d.mkdir()
        r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B), "--guard-s", flag, lst, "out_"], capture_output=True, text=True,
                           timeout=600, cwd=str(d))
        assert r.returncode == 0, r.stdout + r.stderr
        out[flag] = {f: np.asarray(Image.open(str(d / f))) for f in sorted(os.listdir(str(d))) if f.endswith(".png")}
        if flag == "--device-png":
            assert "encoded on the host" not in r.stdout
            for f in out[flag]:
                ps.chunks(open(str(d / f), "rb").read())
    a, b = out["--png"], out["--device-png"]
    assert list(a) == list(b) and len(a) == n
    for f in a:
        assert np.array_equal(a[f], b[f]), f
