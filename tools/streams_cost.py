"""What a step costs when frames arrive and leave compressed: ms per 64-frame 1080p step, host clock around whole steps, for
  (a) the synchronous sequence `uwpipe --device-decode --device-jpeg / --device-png` runs: uwip_*_decode_host, uwip_pipe_step,
      uwip_pipe_last_params, uwip_pipe_sync, the ratios' copy, uwip_*_encode_host of every frame -- three host waits per step;
  (b) uwip_pipe_step_streams with uwip_pipe_collect lagging one step (`uwpipe --streams`),
for JPEG and PNG, under UWIP_EMIT_ALL (predecessor mode) and under UWIP_EMIT_KEYFRAMES at the reference's defaults (minOverlap
0.4, kWindow 11), S guarded in the dehaze stage as in bench.py.  In key-frame mode (a) still encodes every frame, as uwpipe does; (b) only the key frames.  The two legs of a
configuration alternate, `--repeats` times each, and every repeat is reported (the spread is the answer to "is the difference
real").  Also the bytes that cross the link per step, each way.

    python tools/streams_cost.py [--steps N] [--repeats R] [--frames F] [--json out.json]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import uwimageproc_amd as uw  # noqa: E402
from uwimageproc_amd import synth  # noqa: E402
from uwimageproc_amd._native import _P, StreamOut, batch_of  # noqa: E402
from uwimageproc_amd.pipeline import FramePipe  # noqa: E402


def c_streams(streams):
    """The (pointers, sizes) arrays the C entries take, made once per batch outside the timed region: (bufs, ptrs, sizes)."""
    bufs = [(C.c_uint8 * len(s)).from_buffer_copy(s) for s in streams]
    return bufs, (_P * len(bufs))(*[C.addressof(b) for b in bufs]), (C.c_size_t * len(bufs))(*[len(s) for s in streams])


def jpeg_of(img):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1]), "RGB").save(buf, format="JPEG", quality=95, subsampling=2)
    return buf.getvalue()


class SyncLeg:
    """(a): the entries uwpipe calls today, in its order."""

    def __init__(self, F, H, W, fmt, kf):
        self.pipe = FramePipe(0, F, H, W, guard_s=True, keyframes=kf)
        self.F, self.fmt, self.raw = F, fmt, H * W * 3
        self.src = torch.empty((F, H, W, 3), dtype=torch.uint8, device="cuda")
        self.h_status = (C.c_int32 * F)()
        self.h_sizes = (C.c_int64 * F)()
        self.h_streams = np.empty((F, self.raw), np.uint8)
        self.bytes_out = 0

    def step(self, streams):
        p, F = self.pipe, self.F
        bufs, ptrs, sizes = streams
        b = batch_of(self.src)
        dec = "uwip_png_decode_host" if bytes(bufs[0][:4]) == b"\x89PNG" else "uwip_jpeg_decode_host"
        p.ctx.call(dec, ptrs, sizes, F, C.byref(b), None, self.h_status)
        work, ratio = p.run(self.src)
        _ = p.params                         # uwip_pipe_last_params
        p.sync()
        r = ratio.cpu()
        wb = batch_of(work)
        if self.fmt == "png":
            p.ctx.call("uwip_png_encode_host", C.byref(wb), -1, _P(self.h_streams.ctypes.data), self.raw, self.h_sizes)
        else:
            p.ctx.call("uwip_jpeg_encode_host", C.byref(wb), 95, _P(self.h_streams.ctypes.data), self.raw, self.h_sizes)
        self.bytes_out = sum(max(0, int(s)) for s in self.h_sizes) + r.numel() * 4
        return F

    def finish(self):
        self.pipe.sync()

    def close(self):
        self.pipe.close()


class StreamsLeg:
    """(b): step k is queued, then step k - 1 is collected."""

    def __init__(self, F, H, W, fmt, kf):
        self.pipe = FramePipe(0, F, H, W, guard_s=True, keyframes=kf)
        self.pipe.streams(format=fmt, emit="keyframes" if kf is not None else "all")
        self.F, self.prev, self.bytes_out, self.emitted, self.outgrown = F, None, 0, 0, 0
        # the C entries with buffers made once, as a C caller has them (uwpipe --streams): no Python copies in the timed region
        self.status, self.ratio, self.outs = (C.c_int32 * F)(), (C.c_float * F)(), (StreamOut * (F + 1))()
        self.blob = np.empty(((F + 1) * H * W * 3,), np.uint8)

    def _collect(self, t):
        n, need = C.c_int(0), C.c_size_t(0)
        self.pipe._call("uwip_pipe_collect", C.c_uint64(t), self.status, self.ratio, self.outs, self.F + 1, C.byref(n),
                        _P(self.blob.ctypes.data), self.blob.nbytes, C.byref(need))
        self.bytes_out = need.value + 24 * (self.F + 1) + 16 + 16 * self.F
        self.outgrown += sum(1 for e in range(n.value) if self.outs[e].size < 0)
        return n.value

    def step(self, streams):
        _, ptrs, sizes = streams
        tk = C.c_uint64(0)
        self.pipe._call("uwip_pipe_step_streams", ptrs, sizes, self.F, C.byref(tk))
        t = tk.value
        n = self._collect(self.prev) if self.prev is not None else 0
        self.prev = t
        return n

    def finish(self):
        n = self._collect(self.prev) if self.prev is not None else 0
        self.prev = None
        return n

    def close(self):
        self.pipe.close()


def timed(leg, batches, steps, warmup):
    for s in range(warmup):
        leg.step(batches[s % len(batches)])
    leg.finish()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    emitted = 0
    for s in range(steps):
        emitted += leg.step(batches[(warmup + s) % len(batches)]) or 0
    emitted += leg.finish() or 0
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps, emitted / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "streams_cost.py measures on a HIP device"
    F, H, W = a.frames, a.rows, a.cols
    raw = [synth.uw_stream_motion(k * F, F, H, W) for k in range(2)]
    ctx = uw.Context(0)
    inputs = {"jpeg": [[jpeg_of(f) for f in b] for b in raw],
              "png": [uw.png.encode(ctx, torch.from_numpy(b).cuda()) for b in raw]}
    ctx.close()
    res = []
    for fmt in ("jpeg", "png"):
        batches = [c_streams(b) for b in inputs[fmt]]
        bytes_in = float(np.mean([sum(len(s) for s in b) for b in inputs[fmt]]))
        for kf in (None, dict()):
            legs = {"sync": SyncLeg(F, H, W, fmt, kf), "streams": StreamsLeg(F, H, W, fmt, kf)}
            ms = {"sync": [], "streams": []}
            em = {"sync": [], "streams": []}
            for r in range(a.repeats):
                for name in ("sync", "streams"):                    # alternating
                    if kf is not None:
                        legs[name].pipe.have_prev = False           # every repeat is the same stream from its start
                    t, e = timed(legs[name], batches, a.steps, warmup=2 if r == 0 else 1)
                    ms[name].append(t)
                    em[name].append(e)
            for name in ("sync", "streams"):
                res.append(dict(format=fmt, emit="keyframes" if kf is not None else "all", form=name, frames=F, rows=H, cols=W,
                                steps=a.steps, ms_per_step=ms[name], ms_median=float(np.median(ms[name])), ms_min=min(ms[name]),
                                ms_max=max(ms[name]), frames_emitted_per_step=em[name][-1], bytes_in_per_step=bytes_in,
                                bytes_out_per_step=legs[name].bytes_out, raw_bytes_each_way_per_step=F * H * W * 3,
                                streams_outgrown=getattr(legs[name], "outgrown", None)))
                print(json.dumps(res[-1]), flush=True)
                legs[name].close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
