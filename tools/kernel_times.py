"""Per-kernel time of one 64-frame sub-batch of the 1080p pipe on one stream (HIP events inside libuwip): the quick
before/after table for kernel work (GPU box).   python3 tools/kernel_times.py [frames] [reps] [seed0 ...]   (KT_4K=1: 3840x2160)
Without seed0: the translating scene of synth.uw_stream.  With one or more seed0: bench.py's scenes (synth.uw_stream_motion;
1234 is the headline scene, 1234 + 77777 j its further scenes), one table each, and k_clahe_sweep of every repeat."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from uwimageproc_amd import synth
from uwimageproc_amd.pipeline import FramePipe
F = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
seeds = [int(a) for a in sys.argv[3:]] or [None]
H, W = (2160, 3840) if os.environ.get("KT_4K") else (1080, 1920)
pipe = FramePipe(0, F, H, W, guard_s=True)
for seed0 in seeds:
    n = min(F, 16)
    base = synth.uw_stream(0, n, H, W) if seed0 is None else synth.uw_stream_motion(0, n, H, W, seed0=seed0)
    src = torch.from_numpy(np.concatenate([base] * ((F + len(base) - 1) // len(base)))[:F]).cuda()
    pipe.run(src); torch.cuda.synchronize()
    pipe.ctx.prof_enable(True)
    res, sweep = {}, []
    for _ in range(reps):
        pipe.ctx.prof_reset()
        pipe.run(src)
        torch.cuda.synchronize()
        one = pipe.ctx.prof_results()
        sweep.append(one.get("k_clahe_sweep", (0.0, 0))[0])
        for k, (ms, cnt) in one.items():
            res[k] = (res.get(k, (0.0, 0))[0] + ms, res.get(k, (0.0, 0))[1] + cnt)
    pipe.ctx.prof_enable(False)
    tot = sum(ms for ms, _ in res.values()) / reps
    print(f"{F} frames of {W}x{H}, {reps} reps, scene {'uw_stream' if seed0 is None else seed0}: {tot:.3f} ms of kernels per step")
    print("  k_clahe_sweep per repeat: " + " ".join(f"{ms:.3f}" for ms in sweep) + " ms")
    for k, (ms, cnt) in sorted(res.items(), key=lambda kv: -kv[1][0]):
        print(f"  {k:26s} {ms/reps:8.3f} ms  {cnt/reps:5.1f} launches  {100*ms/reps/tot:5.1f} %")
