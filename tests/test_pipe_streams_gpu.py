"""GPU: uwip_pipe_step_streams / uwip_pipe_collect (include/uwip.h; csrc/pipe_streams.hip) hand back, byte for byte, the streams
the existing entries give on a second, identical pipe: uwip_*_decode_host -> uwip_pipe_step -> uwip_*_encode of the enhanced
frames -- for every good frame (UWIP_EMIT_ALL) or for the key frames whose rows closed in the step (UWIP_EMIT_KEYFRAMES)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import _jpeg_streams as js
import uwimageproc_amd as uw
import uwimageproc_amd._native as nat
from uwimageproc_amd import synth
from uwimageproc_amd.pipeline import FramePipe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
H, W, F = 96, 128, 4                      # the guided filter needs >= 81 both ways
RAW = H * W * 3


def _scene(i, smooth=0):
    """Frame i: a scene of its own (no two frames overlap); smooth > 0: box-filtered that many times (a low calcBlur)."""
    f = synth.uw_stream(0, 1, H, W, seed0=1234 + 100 * i)[0].astype(np.float32)
    for _ in range(smooth):
        p = np.pad(f, ((1, 1), (1, 1), (0, 0)), mode="edge")
        f = sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) / 9.0
    return np.ascontiguousarray(np.clip(np.rint(f), 0, 255).astype(np.uint8))


def _jpg(img):
    return js.pil_stream(img, 95, 2)


def _png(ctx, img):
    return uw.png.encode(ctx, torch.from_numpy(img[None]).cuda())[0]


def _decode_ref(ctx, streams):
    """The existing entries on a mixed batch, run by run as uwpipe does: (frames [F, H, W, 3] device, statuses)."""
    out = torch.zeros((len(streams), H, W, 3), dtype=torch.uint8, device="cuda")
    status = []
    j0 = 0
    while j0 < len(streams):
        png = streams[j0][:8] == b"\x89PNG\r\n\x1a\n"
        j1 = j0 + 1
        while j1 < len(streams) and (streams[j1][:8] == b"\x89PNG\r\n\x1a\n") == png:
            j1 += 1
        mod = uw.png if png else uw.jpeg
        st = mod.decode_into(ctx, streams[j0:j1], out[j0:j1])
        ctx.sync()
        status += st.cpu().tolist()
        j0 = j1
    for f, s in enumerate(status):
        if s < 0:
            out[f].zero_()
    torch.cuda.synchronize()
    return out, status


def _encode_ref(ctx, frames, fmt, slot=RAW, quality=95, png_filter=-1):
    """uwip_jpeg_encode / uwip_png_encode of a device batch: [bytes | -needed] per frame."""
    if fmt == "jpeg":
        streams, sizes = uw.jpeg.encode_device(ctx, frames, quality, slot)
    else:
        streams, sizes = uw.png.encode_device(ctx, frames, png_filter, slot)
    ctx.sync()
    n = sizes.cpu().tolist()
    return [streams[f, :n[f]].cpu().numpy().tobytes() if n[f] >= 0 else int(n[f]) for f in range(len(n))]


def _same_ratio(a, b):
    return all((math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(a.tolist(), b.tolist()))


@pytest.mark.parametrize("fmt", ["jpeg", "png"])
def test_emit_all_equals_decode_step_encode(fmt):
    sp = FramePipe(0, F, H, W)
    ref = FramePipe(0, F, H, W)
    sp.streams(format=fmt)
    imgs = [_scene(i % 5) if i % 3 else _scene(i) for i in range(3 * F)]
    kind = "jjjj" "pppp" "jppj"               # a JPEG step, a PNG step, a mixed one
    streams = [_jpg(im) if k == "j" else _png(ref.ctx, im) for im, k in zip(imgs, kind)]
    want = []
    for s in range(3):
        frames, status = _decode_ref(ref.ctx, streams[s * F:(s + 1) * F])
        assert status == [0] * F
        work, ratio = ref.run(frames)
        ref.sync()
        want.append((_encode_ref(ref.ctx, work, fmt), ratio.cpu().numpy().copy(), list(ref.params)))
    # the loop of a caller: step k, then collect k - 1
    got, tickets, params, rparams = [], [], [], []
    for s in range(3):
        tickets.append(sp.run_streams(streams[s * F:(s + 1) * F]))
        if fmt == "png":
            params.append(list(sp.params))   # uwip_pipe_last_params keeps its meaning (it waits for the stream)
        if s:
            rparams.append(sp.result_params(tickets[s - 1]))
            got.append(sp.collect(tickets[s - 1]))
    rparams.append(sp.result_params(tickets[-1]))
    got.append(sp.collect(tickets[-1]))
    assert tickets == [1, 2, 3]
    for s in range(3):
        status, ratio, outs = got[s]
        enc, r, par = want[s]
        assert status.tolist() == [0] * F
        assert _same_ratio(ratio, r), (s, ratio, r)
        assert [(o[0], o[1]) for o in outs] == [(s * F + j, -1) for j in range(F)]
        for j in range(F):
            assert isinstance(enc[j], bytes) and outs[j][2] == enc[j], (s, j)
        assert rparams[s] == par
        if fmt == "png":
            assert params[s] == par
    sp.close()
    ref.close()


def _keyframe_stream():
    """13 frames for minOverlap 0.5, kWindow 5 and 4 frames per step, confirmed with the oracle chain on the CPU (dehaze,
    histretch, aclahe, calcOverlap and calcBlur of tests/_oracle.py fed to uwip_keyframe_chain_host): rows (0, 0, 0),
    (1, 7, 6), (2, 8, 8).  Frame 1 is frame 0 again (overlap 25: no trigger); frames 2..5 and 8..12 are smoothed scenes that
    come out of the enhancement without a keypoint (calcOverlap -2.0, counted as 0.41: a trigger; calcBlur 0); frames 6 and 7
    are sharp (blur 18.9 and 14.0).  So frame 2 triggers and its window closes at frame 7, in step 1, on frame 6; frame 8
    triggers in step 2, which emits nothing; frames 9..12 never beat it, and the stream ends inside that window in step 3 -- a
    batch of one frame and three padding copies -- whose row names frame 8 of step 2: its pixels were carried."""
    plan = [(0, 0), (0, 0)] + [(i, 3) for i in (8, 9, 10, 11)] + [(6, 0), (7, 0)] + [(i, 3) for i in range(8, 13)]
    return [_scene(i, smooth) for i, smooth in plan]


@pytest.mark.parametrize("fmt", ["jpeg", "png"])
def test_emit_keyframes_equals_the_rows_of_the_reference_run(fmt):
    kf = dict(minOverlap=0.5, kWindow=5, lookback=2)
    imgs = _keyframe_stream()
    n = len(imgs)
    streams = [_jpg(im) for im in imgs]
    nb = -(-n // F)
    sp = FramePipe(0, F, H, W, keyframes=kf)
    ref = FramePipe(0, F, H, W, keyframes=kf)
    sp.streams(format=fmt, emit="keyframes")
    enhanced, got = [], []
    for s in range(nb):
        batch = [streams[min(s * F + j, n - 1)] for j in range(F)]
        if s == nb - 1:
            sp.end_of_stream(n - s * F)
            ref.end_of_stream(n - s * F)
        frames, status = _decode_ref(ref.ctx, batch)
        work, _ = ref.run(frames)
        ref.sync()
        enhanced += _encode_ref(ref.ctx, work, fmt)[:n - s * F]
        t = sp.run_streams(batch)
        got.append(sp.collect(t))
    rows = ref.keyframe_rows()                # (id, frame, index, overlap, blur)
    ref.close()
    outs = [(s, o) for s in range(nb) for o in got[s][2]]
    print("rows", rows, "emitted per step", [len(g[2]) for g in got])
    assert [(o[1], o[0]) for _, o in outs] == [(r[0], r[2]) for r in rows]
    assert [r[:3] for r in rows] == [(0, 0, 0), (1, 7, 6), (2, 8, 8)]          # what the oracle chain gives on the CPU
    for _, o in outs:
        assert o[2] == enhanced[o[0]], o[:2]
    # the run holds what it was built for: a row on a frame of an earlier batch (the pixel carry), a step that emits nothing,
    # and a window closed by the end of the stream in a padded last batch
    assert any(o[0] < s * F for s, o in outs), outs
    assert any(len(g[2]) == 0 for g in got)
    ratios = np.concatenate([g[1] for g in got])[:n]
    compared = [i for i in range(n) if not math.isnan(ratios[i])]
    assert n % F != 0 and outs[-1][0] == nb - 1 and outs[-1][1][0] >= compared[-1] and compared[-1] + kf["kWindow"] > n - 1
    # the streams pipe's own rows are still there for uwip_pipe_keyframes
    assert [r[:3] for r in sp.keyframe_rows()] == [r[:3] for r in rows]
    sp.close()


def test_result_params_of_a_lagging_step_device_choice():
    """Five frames per step: the aclahe stage makes its choice on the device, and the parameters travel with the result."""
    F5 = 5
    sp = FramePipe(0, F5, H, W)
    ref = FramePipe(0, F5, H, W)
    sp.streams(format="jpeg")
    steps = [[_jpg(_scene(i + 5 * s)) for i in range(F5)] for s in range(2)]
    want = []
    for b in steps:
        frames = torch.zeros((F5, H, W, 3), dtype=torch.uint8, device="cuda")
        st = uw.jpeg.decode_into(ref.ctx, b, frames)
        ref.ctx.sync()
        assert st.cpu().tolist() == [0] * F5
        work, _ = ref.run(frames)
        ref.sync()
        want.append((list(ref.params), _encode_ref(ref.ctx, work, "jpeg")))
    t = [sp.run_streams(b) for b in steps]
    for s in range(2):
        assert sp.result_params(t[s]) == want[s][0]         # step 0's after step 1 was queued
        outs = sp.collect(t[s])[2]
        assert [o[2] for o in outs] == want[s][1]
        with pytest.raises(uw.UwipError):
            sp.result_params(t[s])                          # collected: gone
    sp.close()
    ref.close()


def test_bad_frames_are_blanked_reported_and_not_emitted():
    good = [_jpg(_scene(i)) for i in range(4)]
    prog = js.pil_stream(_scene(2), 95, 2, progressive=True)
    batch = [good[0], good[1][:20], prog, good[3]]
    ref = FramePipe(0, F, H, W)
    sp = FramePipe(0, F, H, W)
    sp.streams(format="jpeg")
    frames, status = _decode_ref(ref.ctx, batch)          # the two frames zero-filled
    assert status[0] == 0 and status[3] == 0 and status[1] < 0 and status[2] < 0
    work, ratio = ref.run(frames)
    ref.sync()
    enc = _encode_ref(ref.ctx, work, "jpeg")
    st, rt, outs = sp.collect(sp.run_streams(batch))
    assert st.tolist() == status
    assert [(o[0], o[1]) for o in outs] == [(0, -1), (3, -1)]
    assert outs[0][2] == enc[0] and outs[1][2] == enc[3]
    assert _same_ratio(rt, ratio.cpu().numpy())
    sp.close()
    ref.close()


def test_a_stream_that_outgrows_its_slot():
    # frame 1 is sharp and noisy, its neighbours come out of the enhancement nearly flat: its stream is by far the longest
    imgs = [_scene(8, 3), _scene(0), _scene(9, 3), _scene(10, 3)]
    batch = [_jpg(im) for im in imgs]
    ref = FramePipe(0, F, H, W)
    frames, status = _decode_ref(ref.ctx, batch)
    assert status == [0] * F
    work, _ = ref.run(frames)
    ref.sync()
    full = [len(e) for e in _encode_ref(ref.ctx, work, "jpeg", slot=uw.jpeg.bound(H, W, 3))]
    print("stream sizes", full)
    slot = (max(full[0], full[2], full[3]) + full[1]) // 2 | 1          # only frame 1 outgrows it; odd: misaligned slots
    assert max(full[0], full[2], full[3]) < slot < full[1]
    enc = _encode_ref(ref.ctx, work, "jpeg", slot=slot)
    assert enc[1] == -full[1]
    sp = FramePipe(0, F, H, W)
    sp.streams(format="jpeg", slot_bytes=slot)
    # through the C entry: the offsets are looked at as they come
    st = (C.c_int32 * F)()
    outs = (nat.StreamOut * (F + 1))()
    n, need = C.c_int(0), C.c_size_t(0)
    blob = (C.c_uint8 * ((F + 1) * slot))()
    t = sp.run_streams(batch)
    sp._call("uwip_pipe_collect", C.c_uint64(t), st, None, outs, F + 1, C.byref(n), blob, len(blob), C.byref(need))
    assert n.value == F and [outs[j].index for j in range(F)] == [0, 1, 2, 3]
    assert outs[1].size == -full[1]
    off = 0
    raw = bytes(blob)
    for j in range(F):
        assert outs[j].offset == off, j
        if j != 1:
            assert outs[j].size == full[j] and raw[off:off + full[j]] == enc[j], j
            off += full[j]
    assert need.value == off
    sp.close()
    ref.close()


def test_collect_rules_and_reset():
    kf = dict(minOverlap=0.5, kWindow=1, lookback=2)
    sp = FramePipe(0, F, H, W, keyframes=kf)
    sp.streams(format="jpeg", emit="keyframes", depth=2)
    batch = [_jpg(_scene(i)) for i in range(F)]
    t1 = sp.run_streams(batch)
    # a blob that is too small: the call fails with the needed size and the result stays collectable
    st = (C.c_int32 * F)()
    outs = (nat.StreamOut * (F + 1))()
    n, need = C.c_int(0), C.c_size_t(0)
    small = (C.c_uint8 * 16)()
    rc = sp._l.uwip_pipe_collect(sp._p, C.c_uint64(t1), st, None, outs, F + 1, C.byref(n), small, 16, C.byref(need))
    assert rc == nat.UWIP_ERR_INVALID and need.value > 16 and n.value >= 1
    rc = sp._l.uwip_pipe_collect(sp._p, C.c_uint64(t1), st, None, outs, 0, C.byref(n), small, 16, C.byref(need))
    assert rc == nat.UWIP_ERR_INVALID                    # too few entries as well
    first = sp.collect(t1)
    assert sum(len(o[2]) for o in first[2]) == need.value and len(first[2]) == n.value
    assert [o[1] for o in first[2]][0] == 0 and first[2][0][0] == 0      # row 0 is frame 0
    with pytest.raises(uw.UwipError):
        sp.collect(t1)                                   # once
    with pytest.raises(uw.UwipError):
        sp.collect(99)
    # depth results may wait; the step that would overwrite one is refused and queues nothing
    sp.have_prev = False                                 # uwip_pipe_reset: a new stream
    t2 = sp.run_streams(batch)
    t3 = sp.run_streams(batch)
    with pytest.raises(uw.UwipError) as e:
        sp.run_streams(batch)
    assert e.value.code == nat.UWIP_ERR_INVALID
    second = sp.collect(t2)
    # after the reset row IDs restart and nothing is carried: the same stream gives the same result
    assert [(o[0], o[1], o[2]) for o in second[2]] == [(o[0], o[1], o[2]) for o in first[2]]
    assert second[0].tolist() == first[0].tolist() and _same_ratio(second[1], first[1])
    t4 = sp.run_streams(batch)                           # the freed slot takes the next step
    third = sp.collect(t3)
    assert third[2] and all(o[0] >= F - 1 for o in third[2])     # the stream went on: frames F .. 2F - 1, or the carried F - 1
    sp.collect(t4)
    sp.close()


def test_configuration_errors():
    sp = FramePipe(0, F, H, W)
    for bad in (dict(emit="keyframes"), dict(depth=1), dict(png_filter=5)):
        with pytest.raises(uw.UwipError) as e:
            sp.streams(**bad)
        assert e.value.code == nat.UWIP_ERR_INVALID, bad
    sc = nat.PipeStreamsConfig()
    sp._l.uwip_pipe_streams_config_default(C.byref(sc))
    sc.format = 2
    assert sp._l.uwip_pipe_streams(sp._p, C.byref(sc)) == nat.UWIP_ERR_INVALID
    assert sp._l.uwip_pipe_streams(sp._p, None) == nat.UWIP_ERR_INVALID
    batch = [_jpg(_scene(i)) for i in range(F)]
    with pytest.raises(uw.UwipError):
        sp.run_streams(batch)                            # no streams configuration yet
    sp.streams()
    for wrong in (batch[:3], batch + batch[:1]):
        with pytest.raises(uw.UwipError) as e:
            sp.run_streams(wrong)                        # n != frames
        assert e.value.code == nat.UWIP_ERR_INVALID
    t = C.c_uint64(0)
    assert sp._l.uwip_pipe_step_streams(sp._p, None, None, F, C.byref(t)) == nat.UWIP_ERR_INVALID
    sp.collect(sp.run_streams(batch))
    with pytest.raises(uw.UwipError):
        sp.streams()                                     # not in the middle of a stream
    sp.close()


@pytest.mark.parametrize("flags", [[], ["--keyframes", "-k", "2", "-p", "0.5", "--device-png"]])
def test_uwpipe_streams_writes_the_same_files_and_reports(tmp_path, flags):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)
    n, B = 6, 4                                           # the last batch holds two frames and two padding copies
    paths = []
    for i in range(n):
        paths.append(str(tmp_path / f"f{i:03d}.jpg"))
        open(paths[-1], "wb").write(_jpg(_scene(i, smooth=2 if i in (3, 4) else 0)))
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    outs = {}
    for name, extra in (("plain", ["--device-decode", "--device-jpeg"]), ("streams", ["--streams"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B)] + extra + flags + [lst, "out_"], cwd=str(d), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = {f: open(str(d / f), "rb").read() for f in sorted(os.listdir(str(d)))}
    plain, st = outs["plain"], outs["streams"]
    reports = [f for f in plain if f.endswith("_report.txt")]
    assert "out_uwpipe_report.txt" in reports and ("out_videostrip_report.txt" in reports) == bool(flags)
    for f in reports:
        assert st[f] == plain[f], f
    ext = "png" if flags else "jpg"
    if flags:
        rep = plain["out_videostrip_report.txt"].decode().splitlines()
        named = [l.split("\t")[2] for l in rep[rep.index("ID\tFrame\tFilename\tOverlap\tBlur") + 1:]]
        want = sorted(set(named))
        assert 1 <= len(want) < n                         # only the key frames are written
    else:
        want = [f"out_{i:04d}.{ext}" for i in range(n)]
    assert sorted(f for f in st if f.endswith("." + ext)) == want
    for f in want:
        assert st[f] == plain[f], f
