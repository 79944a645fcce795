"""GPU: uwip_jpeg_encode (csrc/jpeg_encode.hip) writes, byte for byte, the streams of the host codec the CLIs write their
files with (jpeg::encode, cli/jpeg.hpp).  cli/bin/jpegenc_check makes the comparison in-process and keeps both streams;
for quality 95 the files of cli/bin/imgconv are compared as well.  Every comparison is exact equality of bytes, and every
device stream is decoded with Pillow next to the host encoder's."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
REAL = os.path.join(ROOT, "tests", "golden", "real")

from uwimageproc_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)


def _decode(stream):
    return np.asarray(Image.open(io.BytesIO(stream)))


_count = [0]


def _check(tmp_path, img, quality):
    """img: [H, W, 3] BGR or [H, W] grey.  Runs jpegenc_check on it; returns the host encoder's stream."""
    _count[0] += 1
    grey = img.ndim == 2
    p = str(tmp_path / f"c{_count[0]}.{'pgm' if grey else 'ppm'}")
    H, W = img.shape[:2]
    body = img.tobytes() if grey else np.ascontiguousarray(img[..., ::-1]).tobytes()
    open(p, "wb").write(b"P%d\n%d %d\n255\n" % (5 if grey else 6, W, H) + body)
    return _check_file(tmp_path, p, quality, grey)


def _check_file(tmp_path, path, quality, grey=False):
    d, h = str(tmp_path / "dev.jpg"), str(tmp_path / "host.jpg")
    for f in (d, h):
        if os.path.exists(f):
            os.remove(f)
    cmd = [os.path.join(BIN, "jpegenc_check"), path, str(quality)] + (["grey"] if grey else []) + ["--out=" + d, "--host-out=" + h]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("identical "), (path, quality, r.stdout + r.stderr)
    dev, host = open(d, "rb").read(), open(h, "rb").read()
    assert dev == host and int(r.stdout.split()[1]) == len(host)
    assert np.array_equal(_decode(dev), _decode(host))
    return host


def _imgconv(tmp_path, img):
    """The file cli/bin/imgconv writes for img (quality 95)."""
    a, j = str(tmp_path / "ic.png"), str(tmp_path / "ic.jpg")
    if img.ndim == 2:
        Image.fromarray(img).save(a)
    else:
        Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(a)
    r = subprocess.run([os.path.join(BIN, "imgconv"), a, j] + (["grey"] if img.ndim == 2 else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    return open(j, "rb").read()


def _encode(ctx, frames, quality=95):
    import torch
    import uwimageproc_amd as uw
    return uw.jpeg.encode(ctx, torch.from_numpy(np.ascontiguousarray(frames)).cuda(), quality)


def _photo_crop():
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(REAL, "in_BUL_T1A_0028.jpg")).convert("RGB"))[:533, :801, ::-1])


def _noise(shape, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _last_ac_only(H, W):
    """Grey frame whose blocks are a DC level plus the (7, 7) basis function: at quality 50 (quantiser 99 there, >= 10
    elsewhere) the only non-zero AC coefficient is the last of the zig-zag: ZRL x 3, run 14, no EOB."""
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    blk = 128 + 100 * np.outer(k, k)
    img = np.tile(blk, ((H + 7) // 8, (W + 7) // 8))[:H, :W]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


SHAPES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (270, 483), (1080, 1920)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synth_frames_every_shape(tmp_path, ctx, shape):
    H, W = shape
    img = synth.uw_stream(0, 1, H, W)[0]
    host = _check(tmp_path, img, 95)
    assert host == _imgconv(tmp_path, img)
    assert _encode(ctx, img[None])[0] == host
    g = np.ascontiguousarray(img[..., 1])
    hg = _check(tmp_path, g, 95)
    assert hg == _imgconv(tmp_path, g)
    assert _encode(ctx, g[None])[0] == hg


def test_single_4k_frame(tmp_path, ctx):
    img = np.tile(synth.uw_stream(0, 1, 1080, 1920)[0], (2, 2, 1))
    img[1080:, :, :] = img[1080:, ::-1, :]
    assert img.shape == (2160, 3840, 3)
    host = _check(tmp_path, img, 95)
    assert host == _imgconv(tmp_path, img)
    assert _encode(ctx, img[None])[0] == host


def test_photograph_crop_and_real_fixtures(tmp_path, ctx):
    photo = _photo_crop()
    assert photo.shape == (533, 801, 3)
    host = _check(tmp_path, photo, 95)
    assert host == _imgconv(tmp_path, photo)
    assert _encode(ctx, photo[None])[0] == host
    for n in ("in_BUL_T1A_0028.jpg", "in_BUL_T1A_0209.jpg", "in_PIS_T1A_259.jpg"):
        host = _check_file(tmp_path, os.path.join(REAL, n), 95)
        j = str(tmp_path / "conv.jpg")
        assert subprocess.run([os.path.join(BIN, "imgconv"), os.path.join(REAL, n), j], capture_output=True, timeout=300).returncode == 0
        assert open(j, "rb").read() == host
    # the grey fixture, as a grey batch of two different frames as well
    g = np.asarray(Image.open(os.path.join(REAL, "in_aclahe_crowd.png")).convert("L"))
    hg = _check(tmp_path, g, 95)
    assert hg == _imgconv(tmp_path, g)
    g2 = np.ascontiguousarray(g[::-1])
    assert _encode(ctx, np.stack([g, g2])) == [hg, _check(tmp_path, g2, 95)]


@pytest.mark.parametrize("quality", [1, 50, 75, 95, 100])
def test_qualities_and_special_contents(tmp_path, ctx, quality):
    photo = _photo_crop()[:270, :483]
    cases = [synth.uw_stream(0, 1, 270, 483)[0], photo, np.full((50, 70, 3), 200, np.uint8), np.full((50, 70), 7, np.uint8),
             _noise((96, 130, 3)), _noise((40, 56)), _last_ac_only(64, 72)]
    for img in cases:
        host = _check(tmp_path, img, quality)
        assert _encode(ctx, img[None], quality)[0] == host
    if quality == 100:
        host = _check(tmp_path, _noise((96, 130, 3)), 100)
        sos = host.index(b"\xff\xda")
        assert b"\xff\x00" in host[sos:]                 # stuffed bytes in the entropy-coded segment
    # out of range: clamped to 1 .. 100 as the host encoder does
    if quality in (1, 100):
        assert _encode(ctx, photo[None], quality + (5 if quality == 100 else -7))[0] == _check(tmp_path, photo, quality)


def test_batch_layouts_equal_the_packed_one(ctx):
    import torch
    import uwimageproc_amd as uw
    F, H, W = 3, 61, 83
    frames = np.stack([synth.uw_stream(0, 1, H, W)[0], _noise((H, W, 3), 5), _photo_crop()[100:100 + H, 200:200 + W]])
    for ch in (3, 1):
        fr = frames if ch == 3 else np.ascontiguousarray(frames[..., 0])
        packed = _encode(ctx, fr)
        step, fs, off = W * ch + 13, (W * ch + 13) * H + 1001, 5           # wide rows, gaps between frames, base % 16 == 5
        buf = torch.full((off + F * fs + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        assert (buf.data_ptr() + off) % 16 == 5
        view = torch.as_strided(buf, (F, H, W, ch), (fs, step, ch, 1), off)
        view.copy_(torch.from_numpy(fr.reshape(F, H, W, ch)).cuda())
        b = uw.batch_of(view)
        assert (b.step, b.frame_stride) == (step, fs)
        assert uw.jpeg.encode(ctx, view if ch == 3 else view[..., 0]) == packed
        # misaligned output slots too
        streams, sizes = uw.jpeg.encode_device(ctx, view if ch == 3 else view[..., 0], 95, slot_bytes=H * W * ch + 1001)
        ctx.sync()
        assert [streams[f, : int(sizes[f])].cpu().numpy().tobytes() for f in range(F)] == packed


def test_batch_of_64_equals_single_frames(tmp_path, ctx):
    import torch
    import uwimageproc_amd as uw
    H, W = 135, 243
    frames = synth.uw_stream(0, 64, H, W).copy()
    frames[7] = _noise((H, W, 3), 11)
    frames[40] = 13
    slot = H * W * 3 + 1024
    streams, sizes = uw.jpeg.encode_device(ctx, torch.from_numpy(frames).cuda(), 95, slot_bytes=slot)
    ctx.sync()
    sizes = sizes.cpu().numpy()
    streams = streams.cpu().numpy()
    for f in range(64):
        one_s, one_n = uw.jpeg.encode_device(ctx, torch.from_numpy(frames[f:f + 1]).cuda(), 95, slot_bytes=slot)
        ctx.sync()
        n = int(one_n[0])
        assert n > 0 and sizes[f] == n, f
        assert streams[f, :n].tobytes() == one_s[0, :n].cpu().numpy().tobytes(), f
    for f in (0, 7, 40, 63):
        assert streams[f, : sizes[f]].tobytes() == _check(tmp_path, frames[f], 95), f


def test_slot_too_small_for_one_frame_is_a_status(tmp_path, ctx):
    import torch
    import uwimageproc_amd as uw
    H, W = 120, 168
    frames = synth.uw_stream(0, 5, H, W).copy()
    frames[2] = _noise((H, W, 3), 21)
    host = [_check(tmp_path, frames[f], 100) for f in range(5)]
    lens = [len(h) for h in host]
    slot = max(lens[f] for f in (0, 1, 3, 4)) + 3
    assert slot < lens[2]                                    # the noisy frame does not fit, not even unstuffed
    dev = torch.from_numpy(frames).cuda()
    for s in (slot, lens[2] - 1):                            # far too small; one byte short (the unstuffed stream fits)
        streams, sizes = uw.jpeg.encode_device(ctx, dev, 100, slot_bytes=s)
        ctx.sync()
        sizes = sizes.cpu().tolist()
        flat = streams.cpu().numpy().reshape(-1)
        assert sizes[2] == -lens[2]
        for f in (0, 1, 3, 4):
            assert sizes[f] == lens[f] and flat[f * s: f * s + lens[f]].tobytes() == host[f], f
        # right behind the short slot: the next frame's stream, intact
        assert flat[3 * s: 3 * s + lens[3]].tobytes() == host[3]
    # exactly enough
    streams, sizes = uw.jpeg.encode_device(ctx, dev, 100, slot_bytes=lens[2])
    ctx.sync()
    assert sizes.cpu().tolist() == lens
    assert streams[2].cpu().numpy().tobytes() == host[2]
    with pytest.raises(uw.UwipError):
        uw.jpeg.encode(ctx, torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device="cuda"))
    # and the C entry itself: channels other than 1 or 3 is UWIP_ERR_INVALID
    import ctypes as C
    import uwimageproc_amd._native as nat
    b = uw.batch_of(dev)
    b.channels = 2
    n = torch.zeros((5,), dtype=torch.int64, device="cuda")
    assert nat.lib().uwip_jpeg_encode(ctx._h, C.byref(b), 95, None, 0, C.c_void_p(n.data_ptr())) == nat.UWIP_ERR_INVALID


def _write_mjpeg_avi(path, jpegs, fps, width, height):
    """A minimal RIFF AVI with one Motion-JPEG video stream (what `ffmpeg -c:v mjpeg` writes, without the index)."""
    def chunk(tag, body):
        return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    def lst(kind, body):
        return chunk(b"LIST", kind + body)
    avih = struct.pack("<14I", int(1e6 / fps), 0, 0, 0x10, len(jpegs), 0, 1, 0, width, height, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII", 0, 0, 0, 0, 1, int(fps), 0, len(jpegs), 0, 0xFFFFFFFF, 0) + struct.pack("<4h", 0, 0, width, height)
    strf = struct.pack("<IiiHHIIiiII", 40, width, height, 1, 24, 0x47504A4D, width * height * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi = lst(b"movi", b"".join(chunk(b"00dc", j) for j in jpegs))
    body = b"AVI " + hdrl + movi
    open(path, "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_uwpipe_device_jpeg_writes_the_same_files(tmp_path):
    n, B, H, W = 5, 2, 270, 480
    jpegs = []
    for f in synth.uw_stream(0, n, H, W):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(buf, format="JPEG", quality=92, subsampling=2)
        jpegs.append(buf.getvalue())
    avi = str(tmp_path / "clip.avi")
    _write_mjpeg_avi(avi, jpegs, 25.0, W, H)
    out = {}
    for flag in ("", "--device-jpeg"):
        d = tmp_path / ("dev" if flag else "host")
        d.mkdir()
        cmd = [os.path.join(BIN, "uwpipe"), "-b", str(B), "--guard-s"] + ([flag] if flag else []) + [avi, "out_"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(d))
        assert r.returncode == 0, r.stdout + r.stderr
        out[flag] = {f: open(str(d / f), "rb").read() for f in sorted(os.listdir(str(d)))}
    a, b = out[""], out["--device-jpeg"]
    assert list(a) == list(b) and len([f for f in a if f.endswith(".jpg")]) == n
    for f in a:
        assert a[f] == b[f], f
