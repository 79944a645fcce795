"""GPU: uwip_png_decode with segmented = 2 (found block starts, csrc/png_decode.hip).  Foreign streams of several deflate blocks
are inflated without the one-wavefront serial pass and give mode 1's pixels, the host reader's, at the library's chunk size and
at 4096 bytes; streams with nothing to find and a stream that carries a deflate stream inside stored blocks lose no pixel; a
mixed batch with bad frames in a strided, gapped, misaligned view has mode 1's statuses and pixels.  Every comparison is exact
equality."""
import io
import os
import subprocess

import numpy as np
import pytest

import _png_decode_streams as pd
import _png_spec_streams as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)


@pytest.fixture(scope="module")
def streams():
    S = sp.streams()
    return S, {name: len(sp.blocks(sp.zstream(s))) for name, (s, _) in S.items()}


def _decode(ctx, s, arr, segmented, chunk_bytes=0):
    import torch
    import uwimageproc_amd as uw
    H, W = arr.shape[:2]
    out = torch.full((1, H, W, 3), 0x5A, dtype=torch.uint8, device="cuda")
    counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    status = uw.png.decode_into(ctx, [s], out, segmented, counts, chunk_bytes=chunk_bytes)
    ctx.sync()
    return out.cpu().numpy()[0], status.cpu().tolist()[0], counts.cpu().tolist()


@pytest.mark.parametrize("name", ("A", "B", "Bp", "C", "D", "Dfixed", "E"))
def test_each_stream_equals_mode_1_and_the_host_reader(ctx, streams, name):
    S, nblocks = streams
    s, arr = S[name]
    want = pd.expected(arr)
    ref, st, c1 = _decode(ctx, s, arr, 1)
    assert st == 0 and np.array_equal(ref, want) and c1 == [1, 0, 1]
    for cb in (0, 4096):
        got, st, c = _decode(ctx, s, arr, 2, cb)
        print(name, cb, "status", st, "counts", c)
        assert st == 0 and np.array_equal(got, ref), (name, cb, st)
        assert c[2] == 1
        if name in ("A", "B", "Bp", "C"):
            assert c[1] == 0 and 2 <= c[0] <= nblocks[name], (name, cb, c, nblocks[name])
        else:
            assert c[0] + c[1] >= 1
        if name == "E":
            assert c[0] <= 2, c                                   # nothing that starts inside a stored block's payload


def test_batch_of_64_mixed_kinds_with_bad_frames_in_a_strided_view_equals_mode_1(ctx):
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
    step, fs, off = W * 3 + 13, (W * 3 + 13) * H + 1001, 5
    results = {}
    for seg, cb in ((1, 0), (2, 0), (2, 4096)):
        raw = torch.full((off + F * fs + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(raw, (F, H, W, 3), (fs, step, 3, 1), off)
        counts = torch.zeros((3,), dtype=torch.int64, device="cuda")
        status = uw.png.decode_into(ctx, streams, view, seg, counts, chunk_bytes=cb)
        ctx.sync()
        assert status.cpu().tolist() == want_status, (seg, cb)
        mask = torch.ones_like(raw, dtype=torch.bool)
        torch.as_strided(mask, (F, H, W * 3), (fs, step, 1), off).fill_(False)
        assert bool((raw[mask] == 0xA5).all()), (seg, cb)          # nothing outside the frames was written
        results[(seg, cb)] = (view.cpu().numpy()[:F - 3], counts.cpu().tolist())
        print(seg, cb, "counts", results[(seg, cb)][1])
    ref = results[(1, 0)][0]
    for f in range(F - 3):
        assert np.array_equal(ref[f], pd.expected(arrs[f])), f
    for key in ((2, 0), (2, 4096)):
        assert np.array_equal(results[key][0], ref), key
        assert results[key][1][2] == F
    # mode 2 sent frames through the found block starts: fewer of them took the serial pass than have no segments of their own
    assert results[(2, 4096)][1][0] > results[(1, 0)][1][0]


def test_pngdec_check_on_pillows_stream(tmp_path, streams):
    S, _ = streams
    p = str(tmp_path / "bp.png")
    open(p, "wb").write(S["Bp"][0])
    for extra in (["--segmented", "2"], ["--segmented", "2", "--chunk-bytes", "4096"]):
        r = subprocess.run([os.path.join(BIN, "pngdec_check"), p] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("identical 1"), r.stdout + r.stderr
