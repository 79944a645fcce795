"""GPU: the pipe's key-frame mode (uwip_pipe_keyframe_chain; csrc/kf_chain.hpp) gives the rows of videostrip's selector
loop (main.cpp:284-394, uwimageproc_amd.videostrip.select_keyframes) on the frames the overlap stage sees, for every batch
size and look-back, with every decision made on the device."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from uwimageproc_amd import synth
from uwimageproc_amd import videostrip as vs
from uwimageproc_amd.pipeline import FramePipe, keyframe_chain_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
H, W = 480, 640


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle(ctx, frames, p, k):
    return vs.select_keyframes(ctx, [_dev(f) for f in frames], minOverlap=p, kWindow=k)


def _overlap_only(frames, batch, p, k, D, eos=True, pipe=None):
    """The overlap stage alone on raw frames, `batch` per step, the last batch padded by repeating the final frame."""
    n = len(frames)
    own = pipe is None
    if own:
        pipe = FramePipe(0, batch, H, W, keyframes=dict(minOverlap=p, kWindow=k, lookback=D))
    ratios, infos = [], []
    nb = -(-n // batch)
    for s in range(nb):
        idx = [min(s * batch + j, n - 1) for j in range(batch)]
        if s == nb - 1 and eos:
            pipe.end_of_stream(n - s * batch)
        pipe.work.copy_(_dev(frames[idx]))
        pipe.stage_overlap()
        torch.cuda.synchronize()
        ratios.append(pipe.ratio.cpu().numpy().copy())
        infos.append(pipe.info.cpu().numpy().copy())
    rows = pipe.keyframe_rows()
    if own:
        pipe.close()
    return rows, np.concatenate(ratios), np.concatenate(infos)


def _same_rows(got, exp):
    assert [(g[0], g[1]) for g in got] == [(e[0], e[1]) for e in exp], (got, exp)
    for g, e in zip(got, exp):
        assert abs(g[3] - e[2]) <= 1e-6 and abs(g[4] - e[3]) <= 1e-6, (g, e)
        assert g[1] in (g[2], g[2] + 1)          # Frame: the key's index (trigger) or its read count (window frame)


def _check_ratio_info(rows, ratio, info, n, p, k):
    """d_ratio / d_info[..., 5] as uwip.h says: replay the walk with the pipe's own overlaps."""
    keys = [r[2] for r in rows]
    key, nrow, i = 0, 1, 1
    assert math.isnan(ratio[0]) and info[0, 5] == -1
    while i < n:
        assert info[i, 5] == key and not math.isnan(ratio[i]), (i, key, ratio[i], info[i])
        ov = 0.41 if ratio[i] == -2.0 else ratio[i]
        i += 1
        if np.float32(ov) <= np.float32(p):
            for _ in range(k):
                if i >= n:
                    break
                assert math.isnan(ratio[i]) and info[i, 5] == -1
                i += 1
            key = keys[nrow]
            nrow += 1
    assert nrow == len(rows)
    assert all(math.isnan(r) for r in ratio[n:]) and (info[n:, 5] == -1).all()      # padding frames stay out


@pytest.fixture(scope="module")
def stream():
    return synth.uw_stream(0, 22, H, W, step_frac=0.05)


@pytest.mark.parametrize("p,k", [(0.7, 2), (0.5, 11)])
def test_overlap_stage_matches_select_keyframes(ctx, stream, p, k):
    n = len(stream)
    exp = _oracle(ctx, stream, p, k)
    assert len(exp) >= 2                         # a window happens
    for batch in (1, 3, 5, 8, n):
        for D in (1, 2, 8):
            rows, ratio, info = _overlap_only(stream, batch, p, k, D)
            _same_rows(rows, exp)
            _check_ratio_info(rows, ratio, info, n, p, k)
    # the raw ratio of a compared frame is calcOverlap against its key
    rows, ratio, info = _overlap_only(stream, 5, p, k, 2)
    kf = vs.keyframe(ctx, _dev(stream[info[1, 5]]))
    vs.videoWidth, vs.videoHeight = W, H
    assert abs(vs.calcOverlap(ctx, kf, _dev(stream[1])) - ratio[1]) <= 1e-6


def test_every_frame_triggers_and_none(ctx, stream):
    n = 12
    fr = stream[:n]
    for p, k in ((1.0, 2), (1.0, 0)):
        exp = _oracle(ctx, fr, p, k)
        rows, ratio, info = _overlap_only(fr, 4, p, k, 1)
        _same_rows(rows, exp)
        _check_ratio_info(rows, ratio, info, n, p, k)
    rows, ratio, info = _overlap_only(fr, 4, -3.0, 11, 2)
    assert rows == [(0, 0, 0, 0.0, 0.0)]
    assert not np.isnan(ratio[1:n]).any() and (info[1:n, 5] == 0).all()


def test_slow_stream_fallback_rounds(ctx):
    # a slow pan: runs without a trigger longer than D, so keys set inside a batch need fallback rounds
    n = 24
    fr = synth.uw_stream_motion(0, n, H, W, step_frac=0.02)
    for p, k in ((0.75, 0), (0.8, 2)):
        exp = _oracle(ctx, fr, p, k)
        assert len(exp) >= 2, exp
        for batch, D in ((12, 2), (24, 1), (8, 1)):
            rows, ratio, info = _overlap_only(fr, batch, p, k, D)
            _same_rows(rows, exp)
            _check_ratio_info(rows, ratio, info, n, p, k)
        # the rounds the device walked at batch 8, D 1: the same walker on the host, fed with the overlaps that pipe computed
        # and the blurs of its frames, takes the device's path (uncompared pairs never decide anything) -- and gives its rows
        seen = {(int(info[i, 5]), i): float(ratio[i]) for i in range(n) if info[i, 5] >= 0}
        blur = vs.calcBlur(ctx, vs.resize_bgr(ctx, _dev(fr))).cpu().numpy()
        replay, rounds = keyframe_chain_host(lambda a, b: seen.get((a, b), 0.99), lambda f: float(blur[f]), n, 8, minOverlap=p,
                                             kWindow=k, lookback=1)
        assert [r[:3] for r in replay] == [r[:3] for r in rows]
        assert sum(rounds) > 0, rounds


def test_end_of_stream_inside_a_window_and_reset(ctx, stream):
    fr = stream[:11]
    exp = _oracle(ctx, fr, 0.7, 11)             # the stream ends inside a window: the best so far is reported
    rows, ratio, info = _overlap_only(fr, 4, 0.7, 11, 2)
    _same_rows(rows, exp)
    _check_ratio_info(rows, ratio, info, 11, 0.7, 11)
    # reset between two videos = two fresh pipes (no end-of-stream mark: a window still open is dropped by the reset)
    a, b = stream[:8], synth.uw_stream_motion(3, 12, H, W, step_frac=0.05)
    fresh = [_overlap_only(v, 4, 0.7, 2, 2, eos=False)[0] for v in (a, b)]
    pipe = FramePipe(0, 4, H, W, keyframes=dict(minOverlap=0.7, kWindow=2, lookback=2))
    got = []
    for v in (a, b):
        got.append(_overlap_only(v, 4, 0.7, 2, 2, eos=False, pipe=pipe)[0])
        pipe.have_prev = False                   # uwip_pipe_reset
    assert got == fresh
    pipe.close()


def test_whole_chain_resident_and_host_forms(ctx):
    F, n = 4, 10
    src = synth.uw_stream_motion(0, n, H, W, step_frac=0.05)
    kw = dict(video_size=(W, H), guard_s=True)
    ref = FramePipe(0, F, H, W, **kw)
    kfp = FramePipe(0, F, H, W, keyframes=dict(minOverlap=0.7, kWindow=2), **kw)
    hp = FramePipe(0, F, H, W, keyframes=dict(minOverlap=0.7, kWindow=2), **kw)
    h_in, h_out = hp.host_buffers()
    enhanced = []
    nb = -(-n // F)
    for s in range(nb):
        batch = src[[min(s * F + j, n - 1) for j in range(F)]]
        if s == nb - 1:
            kfp.end_of_stream(n - s * F)
            hp.end_of_stream(n - s * F)
        a, _ = ref.run(_dev(batch))
        b, _ = kfp.run(_dev(batch))
        torch.cuda.synchronize()
        assert torch.equal(a, b)                 # key-frame mode leaves the enhanced frames as they are
        enhanced += list(b.cpu().numpy()[:n - s * F])
        h_in[:] = batch
        hp.run_host(h_in, h_out)
        hp.sync()
        assert np.array_equal(h_out, b.cpu().numpy())
    exp = _oracle(ctx, enhanced, 0.7, 2)
    rows = kfp.keyframe_rows()
    _same_rows(rows, exp)
    assert hp.keyframe_rows() == rows
    for p_ in (ref, kfp, hp):
        p_.close()


def test_host_form_single_padded_batch(ctx):
    """A stream shorter than one batch through the host-buffer form: the end-of-stream mark given before the first
    run_host (which re-makes the C pipe for its staging area) keeps the padding out and closes the open window."""
    F = 4
    hp = FramePipe(0, F, H, W, video_size=(W, H), guard_s=True, keyframes=dict(minOverlap=1.0, kWindow=2))
    h_in, h_out = hp.host_buffers()
    for v, (p, n) in enumerate(((1.0, 2), (1.0, 3))):
        src = synth.uw_stream_motion(5 * v, n, H, W, step_frac=0.05)
        hp.end_of_stream(n)
        h_in[:] = src[[min(j, n - 1) for j in range(F)]]
        hp.run_host(h_in, h_out)
        hp.sync()
        rows = hp.keyframe_rows()
        # frame 1 triggers (minOverlap 1.0) and opens a window of 2 frames that the stream ends inside of (B-14)
        exp = _oracle(ctx, list(h_out[:n]), p, 2)
        _same_rows(rows, exp)
        assert len(rows) == 2 and all(r[2] < n for r in rows)
        ratio = hp.ratio.cpu().numpy()
        assert np.isnan(ratio[n:]).all() and np.isnan(ratio[0])
    hp.close()
    # the host form cannot follow resident steps of a chain: the pipe it re-makes would drop the chain
    kp = FramePipe(0, F, H, W, keyframes=dict(minOverlap=0.7, kWindow=2))
    kp.run(_dev(synth.uw_stream_motion(0, F, H, W)))
    a, b = kp.host_buffers()
    with pytest.raises(Exception):
        kp.run_host(a, b)
    kp.close()


def _save_png(path, bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path)


def _load(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))[..., ::-1].copy()


def _report_rows(path):
    rep = open(path).read().splitlines()
    return [l.split("\t") for l in rep[rep.index("ID\tFrame\tFilename\tOverlap\tBlur") + 1:]]


def test_uwpipe_keyframes_cli(ctx, tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)
    n, B = 9, 4                                  # the last batch holds one frame and three padding copies
    frames = synth.uw_stream_motion(0, n, H, W, step_frac=0.05)
    paths = []
    for i in range(n):
        paths.append(str(tmp_path / f"f{i:03d}.png"))
        _save_png(paths[-1], frames[i])
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    prefix = str(tmp_path / "out_")
    r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B), "--png", "--keyframes", "-k", "2", "-p", "0.7", lst, prefix],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = _report_rows(prefix + "videostrip_report.txt")
    # the same pipe through the Python binding (the enhanced frames the CLI wrote are the pipe's own)
    pipe = FramePipe(0, B, H, W, keyframes=dict(minOverlap=0.7, kWindow=2))
    nb = -(-n // B)
    for s in range(nb):
        if s == nb - 1:
            pipe.end_of_stream(n - s * B)
        pipe.run(_dev(frames[[min(s * B + j, n - 1) for j in range(B)]]))
    exp = pipe.keyframe_rows()
    pipe.close()
    assert len(exp) >= 2
    assert [(int(a[0]), int(a[1])) for a in rows] == [(e[0], e[1]) for e in exp]
    for a, e in zip(rows, exp):
        assert a[2] == f"{prefix}{e[2]:04d}.png" and os.path.exists(a[2])
        assert abs(float(a[3]) - e[3]) <= 1e-5 * max(1.0, abs(e[3])) and abs(float(a[4]) - e[4]) <= 1e-5 * max(1.0, abs(e[4]))
    enhanced = [_load(prefix + f"{i:04d}.png") for i in range(n)]
    got = _oracle(ctx, enhanced, 0.7, 2)
    assert [(g[0], g[1]) for g in got] == [(e[0], e[1]) for e in exp]
    # an MJPEG .avi of the same frames
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_cli import _write_mjpeg_avi
    import io
    from PIL import Image
    jpegs = []
    for f in frames:
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(bio, format="JPEG", quality=95)
        jpegs.append(bio.getvalue())
    avi = str(tmp_path / "clip.avi")
    _write_mjpeg_avi(avi, jpegs, 25.0, W, H)
    prefix2 = str(tmp_path / "avi_")
    r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", "3", "--png", "--keyframes", "-k", "2", "-p", "0.7", avi, prefix2],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows2 = _report_rows(prefix2 + "videostrip_report.txt")
    enhanced2 = [_load(prefix2 + f"{i:04d}.png") for i in range(n)]
    got2 = _oracle(ctx, enhanced2, 0.7, 2)
    assert [(int(a[0]), int(a[1])) for a in rows2] == [(g[0], g[1]) for g in got2]
    for a, g in zip(rows2, got2):
        assert abs(float(a[3]) - g[2]) <= 1e-5 and abs(float(a[4]) - g[3]) <= 1e-4 * max(1.0, abs(g[3]))
