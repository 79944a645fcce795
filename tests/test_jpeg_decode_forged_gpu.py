"""GPU: uwip_jpeg_decode on streams no libjpeg encoder writes (tests/_jpeg_forge.py): every device-eligible triple of sampling
factors, one-component streams with any SOF factors, restart intervals around the MCU count, unusual header forms, and the four
faults of UWIP_JPEG_BAD_STREAM each beside its valid twin.  The pixels are Pillow's, byte for byte, wherever the stream is
inside the forge's amplitude bound, and the host decoder's (cli/bin/jpegdec_check) otherwise; the statuses are the ones
include/uwip.h states."""
import os
import subprocess

import numpy as np
import pytest

import _jpeg_forge_cases as fc
import _jpeg_streams as js

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True, timeout=600)


def _dec(ctx, streams, channels=3, rounds=-1):
    import uwimageproc_amd as uw
    frames, status = uw.jpeg.decode(ctx, streams, channels, rounds)
    return frames.cpu().numpy(), status


def _equal_pillow(ctx, named, channels=3, rounds=-1):
    """One batched call; every frame status 0 and Pillow's pixels."""
    streams = [f.stream for _, f in named]
    got, status = _dec(ctx, streams, channels, rounds)
    assert status == [0] * len(named), [(n, s) for (n, _), s in zip(named, status) if s]
    for (n, f), g in zip(named, got):
        assert np.array_equal(g, js.pil_decode(f.stream, channels)), (n, channels, rounds)


def _check_tool_all(tmp_path, streams, W, H, *extra):
    p = str(tmp_path / "all.avi")
    js.write_mjpeg_avi(p, streams, 25.0, W, H)
    r = subprocess.run([os.path.join(BIN, "jpegdec_check"), p] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("identical %d" % len(streams)), r.stdout + r.stderr


def test_factor_combinations_in_one_batch(ctx):
    named = fc.equality_colour(37, 53)
    assert len(named) == 54
    for rounds in (-1, 0):
        _equal_pillow(ctx, named, rounds=rounds)


def test_grey_with_any_sof_factors_in_one_batch(ctx):
    named = fc.equality_grey(37, 53) + fc.equality_grey_to_4()
    assert len(named) == 18
    _equal_pillow(ctx, named)
    _equal_pillow(ctx, named, channels=1)


@pytest.mark.parametrize("size", fc.SIZES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_block_and_one_pixel_frames(ctx, size):
    named = fc.equality_colour(*size) + fc.equality_grey(*size)
    _equal_pillow(ctx, named)
    _equal_pillow(ctx, fc.equality_grey(*size), channels=1)


def test_restart_intervals_and_header_forms_in_one_batch(ctx):
    named = fc.restart_streams() + fc.header_streams()
    assert len(named) == 26
    for rounds in (-1, 0):
        _equal_pillow(ctx, named, rounds=rounds)


def test_mcu_of_twelve_blocks_is_bad_stream(ctx):
    import uwimageproc_amd as uw
    good = fc.equality_colour(37, 53)[0][1].stream
    got, status = _dec(ctx, [good, fc.twelve_blocks().stream, good])
    assert status == [0, uw.jpeg.BAD_STREAM, 0]
    assert np.array_equal(got[0], js.pil_decode(good)) and np.array_equal(got[2], got[0])


def test_faults_and_their_twins_in_one_batch(tmp_path, ctx):
    import uwimageproc_amd as uw
    cases = fc.bad_streams()
    assert len(cases) == 16
    streams = [s.stream for _, bad, twin, _, _ in cases for s in (bad, twin)]
    for rounds in (-1, 0, 1):
        got, status = _dec(ctx, streams, rounds=rounds)
        assert status == [uw.jpeg.BAD_STREAM, 0] * len(cases), (rounds, [(c[0], s) for c, s in zip(cases, zip(status[::2], status[1::2]))])
        for i, (name, _, twin, inside, _) in enumerate(cases):
            if inside:
                assert np.array_equal(got[2 * i + 1], js.pil_decode(twin.stream)), (name, rounds)
        # the twins against the host decoder, which must refuse the faults
        _check_tool_all(tmp_path, streams, fc.BW, fc.BH, *(("--rounds", str(rounds)) if rounds >= 0 else ()))


def test_long_stream_at_three_round_counts(ctx):
    import torch
    import uwimageproc_amd as uw
    f = fc.long_stream()
    want = js.pil_decode(f.stream)
    out = torch.empty((1, 200, 120, 3), dtype=torch.uint8, device="cuda")
    left = {}
    for rounds in (0, 1, -1):
        out.fill_(0xA5)
        uns = torch.zeros((2,), dtype=torch.int64, device="cuda")
        status = uw.jpeg.decode_into(ctx, [f.stream], out, rounds, uns)
        ctx.sync()
        left[rounds], lanes = (int(v) for v in uns.cpu())
        assert lanes > 100
        # what a lane that started in the middle of the interval read never becomes the status
        assert status.cpu().tolist() == [0] and np.array_equal(out.cpu().numpy()[0], want), rounds
    assert left[0] > 0 and left[0] > left[1] >= left[-1]


def test_mixed_batch_strided_and_reversed(ctx):
    import torch
    import uwimageproc_amd as uw
    W, H = 37, 53
    mixed = fc.mixed_batch()
    F = len(mixed)
    assert [st for _, _, st in mixed].count(-1) == 2 and F > 12
    ref = {n: js.pil_decode(f.stream) for n, f, st in mixed if st == 0}
    # wide rows, gaps between frames, a misaligned base
    step, fs, off = W * 3 + 13, (W * 3 + 13) * H + 1001, 5
    for order in (mixed, mixed[::-1]):
        raw = torch.full((off + F * fs + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(raw, (F, H, W, 3), (fs, step, 3, 1), off)
        status = uw.jpeg.decode_into(ctx, [f.stream for _, f, _ in order], view)
        ctx.sync()
        assert status.cpu().tolist() == [st for _, _, st in order]
        got = view.cpu().numpy()
        for i, (n, _, st) in enumerate(order):
            if st == 0:
                assert np.array_equal(got[i], ref[n]), n
        # nothing outside the frames was written (the slots of the two bad frames may hold anything)
        mask = torch.ones_like(raw, dtype=torch.bool)
        torch.as_strided(mask, (F, H, W * 3), (fs, step, 1), off).fill_(False)
        assert bool((raw[mask] == 0xA5).all())


def test_host_decoder_in_process_on_the_equality_streams(tmp_path):
    named = fc.equality_colour(37, 53) + fc.equality_grey(37, 53) + fc.equality_grey_to_4() + fc.restart_streams() + fc.header_streams()
    _check_tool_all(tmp_path, [f.stream for _, f in named], 37, 53)
