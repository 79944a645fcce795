"""GPU: uwip_jpeg_decode (csrc/jpeg_decode.hip) returns, byte for byte, the pixels of the host codec the CLIs read their files
with (jpeg::decode, cli/jpeg.hpp; cli/bin/jpegdec_check makes that comparison in-process), and of Pillow's decode where
Pillow wrote the stream.  Every comparison is exact equality."""
import os
import subprocess

import numpy as np
import pytest

import _jpeg_streams as js
from uwimageproc_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
REAL = os.path.join(ROOT, "tests", "golden", "real")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)


def _dec(ctx, streams, channels=3, rounds=-1):
    import uwimageproc_amd as uw
    frames, status = uw.jpeg.decode(ctx, streams, channels, rounds)
    return frames.cpu().numpy(), status


def _check_tool(tmp_path, stream, *extra):
    p = str(tmp_path / "t.jpg")
    open(p, "wb").write(stream)
    r = subprocess.run([os.path.join(BIN, "jpegdec_check"), p] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("identical 1"), r.stdout + r.stderr


def _check_tool_all(tmp_path, streams, W, H, *extra):
    """Every stream through jpegdec_check at once, as the frames of a Motion-JPEG .avi: device == jpeg::decode, frame by frame."""
    p = str(tmp_path / "all.avi")
    js.write_mjpeg_avi(p, streams, 25.0, W, H)
    r = subprocess.run([os.path.join(BIN, "jpegdec_check"), p] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("identical %d" % len(streams)), r.stdout + r.stderr


@pytest.mark.parametrize("size", js.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_kind_equals_pillow_and_the_host_decoder(tmp_path, ctx, size):
    H, W = size
    img = js.content(H, W)
    for sub in (0, 1, 2, "grey"):
        src = np.ascontiguousarray(img[..., 1]) if sub == "grey" else img
        streams = [js.pil_stream(src, q, 0 if sub == "grey" else sub, **kw) for kw in js.FORMS.values() for q in (50, 100)]
        want = np.stack([js.pil_decode(s) for s in streams])
        got, status = _dec(ctx, streams)
        assert status == [0] * len(streams), (sub, status)
        assert np.array_equal(got, want), sub
        if sub == "grey":
            g1, status = _dec(ctx, streams, channels=1)
            assert status == [0] * len(streams) and np.array_equal(g1, want[..., 0])
            _check_tool_all(tmp_path, streams, W, H, "grey")
        _check_tool_all(tmp_path, streams, W, H)


def test_noise_spans_many_subsequences_at_every_round_count(tmp_path, ctx):
    import torch
    import uwimageproc_amd as uw
    noise = js.content(135, 243, "noise")
    for sub in (0, 1, 2):
        s = js.pil_stream(noise, 100, sub)
        assert b"\xff\x00" in s[js.segment_start(s):]
        assert len(s) > 40 * 128
        want = js.pil_decode(s)
        for rounds in (-1, 0, 1):
            got, status = _dec(ctx, [s], rounds=rounds)
            assert status == [0] and np.array_equal(got[0], want), (sub, rounds)
        _check_tool(tmp_path, s, "--rounds", "0")
        _check_tool(tmp_path, s)
    # the rounds settle subsequences the speculative pass alone leaves open
    s = js.pil_stream(noise, 100, 2)
    out = torch.empty((1, 135, 243, 3), dtype=torch.uint8, device="cuda")
    left = {}
    for rounds in (0, 3):
        uns = torch.zeros((2,), dtype=torch.int64, device="cuda")
        uw.jpeg.decode_into(ctx, [s], out, rounds, uns)
        ctx.sync()
        left[rounds], lanes = (int(v) for v in uns.cpu())
        assert lanes > 40
    assert left[3] < left[0]


def test_photographs_of_a_foreign_encoder(tmp_path, ctx):
    from PIL import Image
    for n in ("in_BUL_T1A_0028.jpg", "in_BUL_T1A_0209.jpg", "in_PIS_T1A_259.jpg"):
        s = open(os.path.join(REAL, n), "rb").read()
        got, status = _dec(ctx, [s])
        assert status == [0], n
        assert np.array_equal(got[0], js.pil_decode(s)), n
        r = subprocess.run([os.path.join(BIN, "jpegdec_check"), os.path.join(REAL, n)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("identical 1"), r.stdout + r.stderr


def test_stream_without_dht_uses_the_annex_k_tables(tmp_path, ctx):
    s = js.pil_stream(js.content(61, 83), 90, 2)
    t = js.strip_dht(s)
    assert t != s and b"\xff\xc4" not in t[:js.segment_start(t)]
    got, status = _dec(ctx, [t, s])
    assert status == [0, 0] and np.array_equal(got[0], js.pil_decode(s)) and np.array_equal(got[1], got[0])
    _check_tool(tmp_path, t)


def test_batch_of_64_mixed_kinds_with_bad_frames_and_a_strided_batch(tmp_path, ctx):
    import io
    import torch
    from PIL import Image
    import uwimageproc_amd as uw
    H, W, F = 135, 243, 64
    forms = list(js.FORMS.values())
    streams = []
    for f in range(F):
        img = js.content(H, W, "noise" if f % 9 == 4 else "uw", seed=f)
        sub = (0, 1, 2, "grey")[f % 4]
        src = np.ascontiguousarray(img[..., 1]) if sub == "grey" else img
        streams.append(js.pil_stream(src, (50, 92, 100)[f % 3], 0 if sub == "grey" else sub, **forms[(f // 4) % 4]))
    a = js.segment_start(streams[17])                        # frame 17: 4:2:2, the plain form
    assert b"\xff\xdd" not in streams[17][:a]                 # no restart markers: the device decodes it wherever it is cut
    streams[17] = streams[17][:a + (len(streams[17]) - a) // 2]
    buf = io.BytesIO()
    Image.fromarray(js.content(H, W)[..., ::-1].copy()).save(buf, format="JPEG", progressive=True)
    streams[20] = buf.getvalue()
    streams[33] = js.pil_stream(js.content(H - 1, W), 90, 2)
    want_status = [0] * F
    want_status[20], want_status[33] = uw.jpeg.BAD_STREAM, uw.jpeg.SIZE_MISMATCH
    # wide rows, gaps between frames, a misaligned base
    step, fs, off = W * 3 + 13, (W * 3 + 13) * H + 1001, 5
    raw = torch.full((off + F * fs + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(raw, (F, H, W, 3), (fs, step, 3, 1), off)
    status = uw.jpeg.decode_into(ctx, streams, view)
    ctx.sync()
    assert status.cpu().tolist() == want_status
    got = view.cpu().numpy()
    for f in range(F):
        if want_status[f] == 0:
            one, st = _dec(ctx, [streams[f]])
            assert st == [0] and np.array_equal(one[0], got[f]), f
            if f != 17:
                assert np.array_equal(got[f], js.pil_decode(streams[f])), f
    # the host decoder on the same frames, the truncated and the progressive one included (the tool wants one size: the
    # wrong-size frame is left out)
    _check_tool_all(tmp_path, streams[:33] + streams[34:], W, H)
    # nothing outside the frames was written (the slots of the two bad frames may hold anything)
    mask = torch.ones_like(raw, dtype=torch.bool)
    torch.as_strided(mask, (F, H, W * 3), (fs, step, 1), off).fill_(False)
    assert bool((raw[mask] == 0xA5).all())


def test_round_trip_on_the_device(ctx):
    import torch
    import uwimageproc_amd as uw
    for shape in ((2, 61, 83, 3), (2, 61, 83)):
        x = torch.from_numpy(np.stack([js.content(61, 83, k)[..., : (3 if len(shape) == 4 else 1)].reshape(shape[1:]) for k in ("uw", "noise")])).cuda()
        streams = uw.jpeg.encode(ctx, x, 95)
        got, status = _dec(ctx, streams, channels=3 if len(shape) == 4 else 1)
        assert status == [0, 0]
        want = np.stack([js.pil_decode(s, 3 if len(shape) == 4 else 1) for s in streams])
        assert np.array_equal(got, want)


def test_host_only_frames_are_reported_and_their_neighbours_intact(ctx):
    import uwimageproc_amd as uw
    H, W = 135, 243
    img = js.content(H, W)
    rst = js.pil_stream(img, 92, 2, restart_marker_rows=1)
    s422 = js.pil_stream(img, 92, 1)
    plain = js.pil_stream(js.content(H, W, "noise"), 92, 0)
    streams = [plain, js.misplaced_rst(rst), rst, js.sampled_1x2(s422), s422, rst[:-2] + b"\xff\xd7" + rst[-2:], plain]
    for rounds in (-1, 0):
        got, status = _dec(ctx, streams, rounds=rounds)
        assert status == [0, uw.jpeg.HOST_ONLY, 0, uw.jpeg.HOST_ONLY, 0, uw.jpeg.HOST_ONLY, 0], (rounds, status)
        for f in (0, 2, 4, 6):
            assert np.array_equal(got[f], js.pil_decode(streams[f])), (rounds, f)


def test_decode_of_nothing_and_of_nothing_that_parses(ctx):
    import uwimageproc_amd as uw
    frames, status = uw.jpeg.decode(ctx, [])
    assert tuple(frames.shape) == (0, 0, 0, 3) and status == []
    with pytest.raises(uw.UwipError):
        uw.jpeg.decode(ctx, [b"not a jpeg", b""])
    good = js.pil_stream(js.content(8, 8), 90, 0)
    got, status = _dec(ctx, [b"junk", good])
    assert status == [uw.jpeg.BAD_STREAM, 0] and np.array_equal(got[1], js.pil_decode(good))


def _uwpipe_outputs(tmp_path, tag, avi, flags, B=2):
    d = tmp_path / tag
    d.mkdir()
    r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B), "--guard-s"] + flags + [avi, "out_"], capture_output=True, text=True,
                       timeout=600, cwd=str(d))
    assert r.returncode == 0, r.stdout + r.stderr
    return {f: open(str(d / f), "rb").read() for f in sorted(os.listdir(str(d)))}, r.stdout


def _clip(n=5, H=270, W=480):
    return [js.pil_stream(np.ascontiguousarray(f), 92, 2) for f in synth.uw_stream(0, n, H, W)]



def test_uwpipe_device_decode_writes_the_same_files(tmp_path):
    jpegs = _clip()
    avi = str(tmp_path / "clip.avi")
    js.write_mjpeg_avi(avi, jpegs, 25.0, 480, 270)
    base, _ = _uwpipe_outputs(tmp_path, "host", avi, [])
    assert len([f for f in base if f.endswith(".jpg")]) == 5 and "out_uwpipe_report.txt" in base
    for tag, flags in (("dd", ["--device-decode"]), ("ddj", ["--device-decode", "--device-jpeg"]), ("ddk", ["--device-decode", "--keyframes"])):
        ref = base if tag != "ddk" else _uwpipe_outputs(tmp_path, "hostk", avi, ["--keyframes"])[0]
        got, out = _uwpipe_outputs(tmp_path, tag, avi, flags)
        assert "decoded on the host" not in out
        assert list(got) == list(ref), tag
        for f in ref:
            assert got[f] == ref[f], (tag, f)
    # a list of .jpg files instead of the .avi
    names = []
    for i, j in enumerate(jpegs):
        names.append(str(tmp_path / f"in{i}.jpg"))
        open(names[-1], "wb").write(j)
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(names) + "\n")
    a, _ = _uwpipe_outputs(tmp_path, "lhost", lst, [])
    b, _ = _uwpipe_outputs(tmp_path, "ldd", lst, ["--device-decode", "--device-jpeg"])
    assert list(a) == list(b)
    for f in a:
        assert a[f] == b[f], f


def test_uwpipe_device_decode_falls_back_to_the_host_decoder(tmp_path):
    frames = synth.uw_stream(0, 5, 270, 480)
    jpegs = _clip()
    jpegs[2] = js.sampled_1x2(js.pil_stream(np.ascontiguousarray(frames[2]), 92, 1))           # 270 x 480: as many MCUs either way
    jpegs[3] = js.misplaced_rst(js.pil_stream(np.ascontiguousarray(frames[3]), 92, 2, restart_marker_rows=1))
    avi = str(tmp_path / "clip.avi")
    js.write_mjpeg_avi(avi, jpegs, 25.0, 480, 270)
    base, _ = _uwpipe_outputs(tmp_path, "host", avi, [])
    for tag, flags in (("dd", ["--device-decode"]), ("ddj", ["--device-decode", "--device-jpeg"])):
        got, out = _uwpipe_outputs(tmp_path, tag, avi, flags)
        assert "frame 2: device decoder status -3, decoded on the host" in out and "frame 3: device decoder status -3" in out
        assert list(got) == list(base)
        for f in base:
            assert got[f] == base[f], (tag, f)
