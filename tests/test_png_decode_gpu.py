"""GPU: uwip_png_decode (csrc/png_decode.hip) returns, byte for byte, the pixels of the host reader the CLIs read their files
with (imgio::read_png, cli/imgio.hpp; cli/bin/pngdec_check makes that comparison in-process), and of Pillow's decode.  Every
comparison is exact equality."""
import io
import os
import subprocess

import numpy as np
import pytest

import _png_decode_streams as pd
from uwimageproc_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
REAL = os.path.join(ROOT, "tests", "golden", "real")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)


def _dec(ctx, streams, channels=3, segmented=-1):
    import uwimageproc_amd as uw
    frames, status = uw.png.decode(ctx, streams, channels, segmented)
    return frames.cpu().numpy(), status


def _check_tool(tmp_path, streams, *extra):
    """Every stream through pngdec_check at once: device == imgio::read_png, frame by frame."""
    names = []
    for i, s in enumerate(streams):
        names.append(str(tmp_path / f"t{i}.png"))
        open(names[-1], "wb").write(s)
    lst = str(tmp_path / "t.txt")
    open(lst, "w").write("\n".join(names) + "\n")
    r = subprocess.run([os.path.join(BIN, "pngdec_check"), lst] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("identical %d" % len(streams)), r.stdout + r.stderr


@pytest.mark.parametrize("size", pd.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_recipe_equals_pillow_and_the_host_reader(tmp_path, ctx, size):
    H, W = size
    for spp in (1, 2, 3, 4):
        arr = pd.content(H, W, spp)
        streams = [pd.stream(arr, filt, recipe) for recipe in pd.RECIPES for filt in ((0, 1, 2, 3, 4, "mix") if H * W < 1000 else ("mix", 4))]
        streams += [pd.pil_stream(arr), pd.pil_stream(arr, optimize=True)]
        want = np.stack([pd.pil_pixels(s) for s in streams])
        assert np.array_equal(want[0], pd.expected(arr))
        for seg in (0, 1):
            got, status = _dec(ctx, streams, segmented=seg)
            assert status == [0] * len(streams), (spp, seg, status)
            assert np.array_equal(got, want), (spp, seg)
        if spp <= 2:
            g1, status = _dec(ctx, streams, channels=1)
            assert status == [0] * len(streams) and np.array_equal(g1, want[..., 0])
            _check_tool(tmp_path, streams[::5], "grey")
        _check_tool(tmp_path, streams)
        _check_tool(tmp_path, streams[::3], "--segmented", "0")


def test_both_inflate_paths_by_their_counters(ctx):
    import torch
    import uwimageproc_amd as uw
    p97, rgb = pd.period97(), pd.content(97, 113, 3)
    own = uw.png.encode(ctx, torch.from_numpy(np.ascontiguousarray(p97[None, ..., 0])).cuda())[0]
    cases = {                       # name: (stream, pixels, segments accepted, serial frames) with segmented = 1
        "own": (own, p97, 3, 0),
        "full32k": (pd.stream(p97, 0, "full32k"), p97, 3, 0),
        "sync32k": (pd.stream(p97, 0, "sync32k"), p97, None, 1),       # reaches back across the flush points
        "full10k": (pd.stream(rgb, "mix", "full10k"), rgb, None, 1),    # windows of 10000 bytes, not 32768
        "l9m9": (pd.stream(p97, 0, "l9m9"), p97, 1, 0),                 # one segment: the whole stream
    }
    for name, (s, arr, acc, serial) in cases.items():
        H, W = arr.shape[:2]
        for seg in (1, 0):
            out = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda")
            counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
            status = uw.png.decode_into(ctx, [s], out, seg, counts)
            ctx.sync()
            assert status.cpu().tolist() == [0], (name, seg)
            assert np.array_equal(out.cpu().numpy()[0], pd.expected(arr)), (name, seg)
            a, r, n = (int(v) for v in counts.cpu())
            assert n == 1
            if seg == 0:
                assert (a, r) == (0, 1), (name, a, r)
            else:
                assert r == serial and (acc is None or a == acc), (name, a, r)
                if acc is None:
                    assert a < len(pd.RECIPES[name](pd.filtered(arr, 0)))      # not every segment was accepted


def test_batch_of_64_mixed_kinds_with_bad_frames_and_a_strided_batch(tmp_path, ctx):
    import torch
    from PIL import Image
    import uwimageproc_amd as uw
    H, W, F = 135, 243, 64
    recipes = list(pd.RECIPES)
    streams, arrs = [], []
    for f in range(F - 3):
        arr = pd.content(H, W, 1 + f % 4, "noise" if f % 9 == 4 else "uw", seed=f)
        arrs.append(arr)
        if f % 11 == 10:
            streams.append(pd.pil_stream(arr))
        elif f % 13 == 7 and arr.shape[2] in (1, 3):
            x = torch.from_numpy(pd.expected(arr, 1 if arr.shape[2] == 1 else 3)[None]).cuda()
            streams.append(uw.png.encode(ctx, x)[0])
        else:
            streams.append(pd.stream(arr, (0, 1, 2, 3, 4, "mix")[f % 6], recipes[f % len(recipes)]))
    good = streams[5]
    a, b = pd.idat_span(good)
    streams.append(good[:a + (b - a) // 2])
    buf = io.BytesIO()
    Image.fromarray(pd.content(H, W, 3)).convert("P").save(buf, format="PNG")
    streams.append(buf.getvalue())
    streams.append(pd.stream(pd.content(H - 1, W, 3), "mix", "l1"))
    want_status = [0] * (F - 3) + [uw.png.BAD_STREAM, uw.png.BAD_STREAM, uw.png.SIZE_MISMATCH]
    # wide rows, gaps between frames, a misaligned base
    step, fs, off = W * 3 + 13, (W * 3 + 13) * H + 1001, 5
    raw = torch.full((off + F * fs + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(raw, (F, H, W, 3), (fs, step, 3, 1), off)
    status = uw.png.decode_into(ctx, streams, view)
    ctx.sync()
    assert status.cpu().tolist() == want_status
    got = view.cpu().numpy()
    for f in range(F - 3):
        assert np.array_equal(got[f], pd.expected(arrs[f])), f
    _check_tool(tmp_path, streams)
    # nothing outside the frames was written (the slots of the bad frames may hold anything)
    mask = torch.ones_like(raw, dtype=torch.bool)
    torch.as_strided(mask, (F, H, W * 3), (fs, step, 1), off).fill_(False)
    assert bool((raw[mask] == 0xA5).all())


def test_round_trip_on_the_device(ctx):
    import torch
    import uwimageproc_amd as uw
    for shape in ((2, 200, 333, 3), (2, 200, 333)):
        nc = 3 if len(shape) == 4 else 1
        x = np.stack([pd.content(200, 333, nc, k)[..., :nc].reshape(shape[1:]) for k in ("uw", "noise")])
        for filt in (-1, 3):
            streams = uw.png.encode(ctx, torch.from_numpy(x).cuda(), filt)
            for seg in (1, 0):
                got, status = _dec(ctx, streams, channels=nc, segmented=seg)
                assert status == [0, 0] and np.array_equal(got, x), (shape, filt, seg)


def test_the_reference_input_of_aclahe(tmp_path, ctx):
    p = os.path.join(REAL, "in_aclahe_crowd.png")
    s = open(p, "rb").read()
    got, status = _dec(ctx, [s])
    assert status == [0] and np.array_equal(got[0], pd.pil_pixels(s))
    r = subprocess.run([os.path.join(BIN, "pngdec_check"), p], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("identical 1"), r.stdout + r.stderr


def test_damaged_streams_follow_the_host_reader(tmp_path, ctx):
    arr = pd.content(40, 50, 3)
    s = pd.stream(arr, "mix", "l9m9")
    a, b = pd.idat_span(s)
    streams = [s]
    for i in range(24):
        for bit in (0, 3, 7):
            t = bytearray(s)
            t[a + i] ^= 1 << bit
            streams.append(bytes(t))
    at = s.index(b"IHDR") + 4
    for i, val in ((9, 0), (9, 6), (9, 4), (9, 3), (8, 16), (12, 1), (3, 49), (7, 41)):
        streams.append(s[:at + i] + bytes([val]) + s[at + i + 1:])
    import uwimageproc_amd as uw
    want = [pd.read_png_restated(t) for t in streams]
    got, status = _dec(ctx, streams)
    for f, w in enumerate(want):
        try:
            size = uw.png.info(streams[f])[:2]
        except uw.UwipError:
            size = None
        if size is not None and size != (40, 50):
            assert status[f] == -2, f                      # an IHDR of another size: not inflated, whatever its stream holds
        elif w is not None:
            assert status[f] == 0 and np.array_equal(got[f], w), f
        else:
            assert status[f] == -1, f
    assert status[0] == 0 and sum(1 for v in status if v == 0) < len(status) // 3
    _check_tool(tmp_path, streams)


def test_decode_of_nothing_and_of_nothing_that_parses(ctx):
    import uwimageproc_amd as uw
    frames, status = uw.png.decode(ctx, [])
    assert tuple(frames.shape) == (0, 0, 0, 3) and status == []
    with pytest.raises(uw.UwipError):
        uw.png.decode(ctx, [b"not a png", b""])
    arr = pd.content(8, 8, 3)
    good = pd.stream(arr, 4, "l1")
    got, status = _dec(ctx, [b"junk", good])
    assert status == [uw.png.BAD_STREAM, 0] and np.array_equal(got[1], pd.expected(arr))


def _uwpipe_outputs(tmp_path, tag, lst, flags, B=2):
    d = tmp_path / tag
    d.mkdir()
    r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B), "--guard-s"] + flags + [lst, "out_"], capture_output=True, text=True,
                       timeout=600, cwd=str(d))
    assert r.returncode == 0, r.stdout + r.stderr
    return {f: open(str(d / f), "rb").read() for f in sorted(os.listdir(str(d)))}, r.stdout


def _png_list(tmp_path, streams):
    names = []
    for i, s in enumerate(streams):
        names.append(str(tmp_path / f"in{i}.png"))
        open(names[-1], "wb").write(s)
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(names) + "\n")
    return lst


def _clip(n=5, H=270, W=480):
    return [np.ascontiguousarray(f[..., ::-1]) for f in synth.uw_stream(0, n, H, W)]          # RGB, the file's order


def test_uwpipe_device_decode_reads_png_lists(tmp_path):
    frames = _clip()
    streams = [pd.stream(f, "mix", ("l6cut1000", "full32k", "l9m9", "rle", "fixed")[i]) for i, f in enumerate(frames)]
    lst = _png_list(tmp_path, streams)
    base, _ = _uwpipe_outputs(tmp_path, "host", lst, [])
    assert len([f for f in base if f.endswith(".jpg")]) == 5 and "out_uwpipe_report.txt" in base
    for tag, flags in (("dd", ["--device-decode"]), ("ddp", ["--device-decode", "--device-png"])):
        ref = base if tag == "dd" else _uwpipe_outputs(tmp_path, "hostp", lst, ["--device-png"])[0]
        got, out = _uwpipe_outputs(tmp_path, tag, lst, flags)
        assert "decoded on the host" not in out
        assert list(got) == list(ref), tag
        for f in ref:
            assert got[f] == ref[f], (tag, f)


def test_uwpipe_mixed_list_is_split_and_falls_back_per_frame(tmp_path):
    """.png and .jpg frames in one list: every step is split between the two decoders, and a JPEG frame only the host decoder
    reads shows the fallback line; the files are those of the run without the flag."""
    import _jpeg_streams as js
    frames = _clip()
    streams = [pd.stream(f, "mix", "l9m9") for f in frames]
    bgr = np.ascontiguousarray(frames[2][..., ::-1])
    streams[2] = js.sampled_1x2(js.pil_stream(bgr, 92, 1))
    streams[3] = js.pil_stream(np.ascontiguousarray(frames[3][..., ::-1]), 92, 2)
    lst = _png_list(tmp_path, streams)
    base, _ = _uwpipe_outputs(tmp_path, "host", lst, [])
    got, out = _uwpipe_outputs(tmp_path, "dd", lst, ["--device-decode"])
    assert "frame 2: device decoder status -3, decoded on the host" in out and out.count("decoded on the host") == 1
    assert list(got) == list(base)
    for f in base:
        assert got[f] == base[f], f


def test_uwpipe_palette_png_in_the_list(tmp_path):
    """A palette PNG is UWIP_PNG_BAD_STREAM on the device and `false` from the host reader (imgio::read_png reads no
    palette files: that is the contract the decoder follows), so no run of uwpipe writes that frame: with --device-decode the
    device refuses it, the host fallback is tried and fails, and the tool stops at that frame with the message it stops with
    when the flag is absent."""
    from PIL import Image
    frames = _clip()
    streams = [pd.pil_stream(f) for f in frames]
    buf = io.BytesIO()
    Image.fromarray(frames[2]).convert("P").save(buf, format="PNG")
    streams[2] = buf.getvalue()
    lst = _png_list(tmp_path, streams)
    outs = {}
    for tag, flags in (("host", []), ("dd", ["--device-decode"])):
        d = tmp_path / tag
        d.mkdir()
        r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", "2", "--guard-s"] + flags + [lst, "out_"], capture_output=True, text=True,
                           timeout=600, cwd=str(d))
        assert r.returncode != 0 and "cannot read frame 2" in r.stdout, r.stdout + r.stderr
        outs[tag] = {f: open(str(d / f), "rb").read() for f in sorted(os.listdir(str(d))) if f.endswith(".jpg")}
    # neither run writes the palette frame or anything behind it (the run without the flag reads a step ahead of the one it
    # writes, so it stops before it has written the first step)
    for tag in outs:
        assert set(outs[tag]) <= {"out_0000.jpg", "out_0001.jpg"}, (tag, list(outs[tag]))
