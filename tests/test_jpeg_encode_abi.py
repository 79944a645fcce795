"""CPU: the device JPEG encoder's entry points are declared, exported and bound; uwip_jpeg_bound is a host-pure bound that
covers the host encoder's worst case; without a device the encoder fails loudly instead of falling back."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
NAMES = ("uwip_jpeg_bound", "uwip_jpeg_encode", "uwip_jpeg_encode_host")


def test_symbols_declared_exported_and_bound():
    import uwimageproc_amd._native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uwip.h")).read(), flags=re.S)
    l = C.CDLL(nat.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(l, n), n
        assert n in nat.SIGNATURES, n
    nat.lib()


def test_bound_is_positive_and_monotone():
    import uwimageproc_amd as uw
    for ch in (1, 3):
        prev_r = 0
        for rows in (1, 7, 8, 9, 16, 17, 270, 1080, 2160):
            prev_c = 0
            for cols in (1, 5, 8, 16, 33, 483, 1920, 3840):
                b = uw.jpeg.bound(rows, cols, ch)
                assert b > 0
                assert b >= prev_c, (rows, cols, ch)
                prev_c = b
            assert prev_c >= prev_r
            prev_r = prev_c
    assert uw.jpeg.bound(8, 8, 2) == 0 and uw.jpeg.bound(0, 8, 3) == 0          # bad geometry: no bound
    # the derivation in uwip.h: header + 2 * ceil(blocks * 1660 / 8) + 2
    assert uw.jpeg.bound(8, 8, 1) == 328 + 2 * ((1660 + 7) // 8) + 2
    assert uw.jpeg.bound(17, 33, 3) == 623 + 2 * ((2 * 3 * 6 * 1660 + 7) // 8) + 2


def test_bound_covers_the_host_encoder_on_noise_at_quality_100(tmp_path):
    """An 8 x 8 grey noise block at quality 100 (every quantiser 1: the longest codes the host encoder produces)."""
    import uwimageproc_amd as uw
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)
    worst = 0
    for seed in range(8):
        rng = np.random.default_rng(seed)
        img = rng.integers(0, 256, size=(8, 8), dtype=np.uint8)
        if seed == 7:
            img = ((np.indices((8, 8)).sum(0) & 1) * 255).astype(np.uint8)    # checkerboard: the largest coefficients
        p, h = str(tmp_path / f"n{seed}.pgm"), str(tmp_path / f"n{seed}.jpg")
        open(p, "wb").write(b"P5\n8 8\n255\n" + img.tobytes())
        # the host stream is written before the tool touches the device: without one it then fails (loudly), which is fine here
        r = subprocess.run([os.path.join(BIN, "jpegenc_check"), p, "100", "grey", "--host-out=" + h], capture_output=True, text=True,
                           timeout=120)
        assert os.path.exists(h), r.stdout + r.stderr
        worst = max(worst, os.path.getsize(h))
    assert worst > 328
    assert uw.jpeg.bound(8, 8, 1) >= worst


def test_no_cpu_fallback_without_device(tmp_path):
    import torch
    import uwimageproc_amd as uw
    import uwimageproc_amd._native as nat
    l = nat.lib()
    # no context: an error status, nothing is touched
    b = nat.BatchU8()
    b.rows, b.cols, b.channels, b.frames, b.step, b.frame_stride = 8, 8, 1, 1, 8, 64
    assert l.uwip_jpeg_encode(None, C.byref(b), 95, None, 0, None) != nat.UWIP_OK
    assert l.uwip_jpeg_encode_host(None, C.byref(b), 95, None, 0, None) != nat.UWIP_OK
    # a host tensor is refused, with or without a device: there is no CPU path
    with pytest.raises(uw.UwipError):
        uw.jpeg.encode(None, torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(uw.UwipError):
            uw.Context(0)
        p = str(tmp_path / "a.pgm")
        open(p, "wb").write(b"P5\n8 8\n255\n" + bytes(64))
        r = subprocess.run([os.path.join(BIN, "jpegenc_check"), p, "95", "grey"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "no HIP device" in r.stdout
