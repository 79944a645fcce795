"""What key-frame mode (uwip_pipe_keyframe_chain) costs per step: ms per 64-frame 1080p step of the whole pipe in
predecessor mode and in key-frame mode for D (lookback) in {1, 2, 4, 8} and kWindow in {0, 11}, with the reference's
as-written overlap area (videoWidth x videoHeight = 1920 x 1080, SURVEY B-8) and with a 640 x 480 area, plus the fallback
rounds the device walked (non-empty rounds per step; round 0 always runs).

    python tools/keyframe_cost.py [--steps N] [--frames F] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from uwimageproc_amd import synth  # noqa: E402
from uwimageproc_amd import videostrip as vs  # noqa: E402
from uwimageproc_amd.pipeline import FramePipe, keyframe_chain_host  # noqa: E402


def run(batches, F, H, W, area, kf, steps, warmup=2):
    pipe = FramePipe(0, F, H, W, video_size=area, guard_s=True, keyframes=kf)
    seen, blur = {}, []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    n, total = 0, 0.0
    # every step is timed on its own, between two events, and drained before the next (both modes alike): the key-frame
    # legs read the step's ratios back to count the rounds
    for s in range(warmup + steps):
        torch.cuda.synchronize()
        ev[0].record()
        pipe.run(batches[s % len(batches)])
        ev[1].record()
        torch.cuda.synchronize()
        if s >= warmup:
            total += ev[0].elapsed_time(ev[1])
        if kf is not None:
            ratio, info = pipe.ratio.cpu().numpy(), pipe.info.cpu().numpy()
            blur += [float(b) for b in vs.calcBlur(pipe.ctx, vs.resize_bgr(pipe.ctx, pipe.work)).cpu().numpy()]
            for i in range(F):
                if info[i, 5] >= 0:
                    seen[(int(info[i, 5]), n + i)] = float(ratio[i])
            n += F
    ms = total / steps
    out = {"ms_per_step": ms}
    if kf is not None:
        rows = pipe.keyframe_rows()
        # the rounds the device walked (warm-up steps included): the same chain on the host, fed with the overlaps the pipe
        # computed and the blurs of its frames (uncompared pairs never decide anything)
        _, rounds = keyframe_chain_host(lambda a, b: seen.get((a, b), 0.99), lambda f: blur[f], n, F, **kf)
        out.update(rows=len(rows), fallback_rounds_per_step=float(np.mean(rounds)), max_fallback_rounds=int(max(rounds)))
    pipe.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    F, H, W = a.frames, 1080, 1920
    batches = [torch.from_numpy(synth.uw_stream_motion(k * F, F, H, W)).cuda() for k in range(2)]
    res = []
    for area in ((W, H), (640, 480)):
        r = run(batches, F, H, W, area, None, a.steps)
        res.append(dict(mode="predecessor", area=list(area), **r))
        print(json.dumps(res[-1]), flush=True)
        for k in (0, 11):
            for D in (1, 2, 4, 8):
                r = run(batches, F, H, W, area, dict(kWindow=k, lookback=D), a.steps)
                res.append(dict(mode="keyframe", area=list(area), kWindow=k, lookback=D, **r))
                print(json.dumps(res[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
