#!/usr/bin/env python3
"""What the strip mosaic costs on the device: 64 frames of 360 x 640 chained 128 px apart (injected translations), rendered
after warm-up at least 20 times per mode; k_strip_render is timed by the library's per-kernel device events
(uwip_prof_enable).  Reported: ms per render, canvas megapixels/s, covered pixel-frames/s, and the ratio to a
device-to-device copy of the algorithmic bytes (canvas written plus frames read) timed in the same run; `gains` (the
statistics of the 63 pairs plus the solve, per-kernel device events and wall clock) and the gained render in each mode
(k_strip_render_gain) next to the ungained one; `bands` (k_strip_stack per level and in all) and the multiband render,
ungained and gained (k_strip_render_bands, k_strip_render_bands_gain), next to FEATHER of the same run, on both workloads;
`seams` (k_strip_seam_cost next to
k_strip_gain_stats of the same run, which visits the same pixels with the same sample; k_strip_seam_path per call and per pair)
and the SEAM render next to LAST of the same run, on both workloads; `add` per frame
through detect and match (uw_stream frames, wall clock around a drained stream) and `layout` (wall clock).
Culling: a render visits the frames of its own segment only, so frames of other segments cost nothing by construction (a
segment's canvas is the box of all its frames: none of them lies outside it).  What culling costs inside a segment is
measured on one of 1024 frames 15 px apart: every tile tests 1024 boxes in four chunks and lists about 47 of them.
usage: python tools/strip_cost.py [--repeats 20] [--out profiles/strip_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import uwimageproc_amd as uw  # noqa: E402
from uwimageproc_amd import synth  # noqa: E402


def timed(ctx, key, reps, call):
    """ms per launch of the kernel(s) `key` (one name or several: their sum) over `reps` calls after three warm-up calls"""
    for _ in range(3):
        call()
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(reps):
        call()
    prof = ctx.prof_results()
    ctx.prof_enable(False)
    keys = [key] if isinstance(key, str) else key
    return [prof[k][0] / reps for k in keys]


def multiband(ctx, s, canvas, reps, feather_ms, copy_ms, gained):
    """bands with the defaults and the multiband renders of segment 0, next to this run's FEATHER and device-to-device copy"""
    stack = timed(ctx, ["k_strip_stack_1", "k_strip_stack_2", "k_strip_stack_4", "k_strip_stack_8"], reps, s.bands)
    out = {"levels": 4, "ramp": [1, 2, 4, 8], "stack_ms_per_level": stack, "stack_ms": sum(stack)}
    ms = timed(ctx, "k_strip_render_bands", reps, lambda: s.render(0, "multiband", out=canvas))[0]
    out["render"] = {"ms": ms, "ratio_to_feather": ms / feather_ms}
    if gained:
        msg = timed(ctx, "k_strip_render_bands_gain", reps, lambda: s.render(0, "multiband", out=canvas, gain=True))[0]
        out["render_gain"] = {"ms": msg, "ratio_to_ungained": msg / ms, "ratio_to_feather": msg / feather_ms}
    if copy_ms:
        out["stack_ratio_to_d2d_copy"] = sum(stack) / copy_ms
        out["render"]["ratio_to_d2d_copy"] = ms / copy_ms
    return out


def seams(ctx, s, canvas, reps, pairs):
    """seams with the default prior and the SEAM render of segment 0, next to this run's k_strip_gain_stats and LAST render"""
    stats = timed(ctx, "k_strip_gain_stats", reps, s.gains)[0]
    cost, path = timed(ctx, ["k_strip_seam_cost", "k_strip_seam_path"], reps, s.seams)
    t0 = time.perf_counter()
    for _ in range(reps):
        s.seams()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    last = timed(ctx, "k_strip_render", reps, lambda: s.render(0, "last", out=canvas))[0]
    ms = timed(ctx, "k_strip_render_seam", reps, lambda: s.render(0, "seam", out=canvas))[0]
    msg = timed(ctx, "k_strip_render_seam_gain", reps, lambda: s.render(0, "seam", out=canvas, gain=True))[0]
    total = s.seam_values()["total"]
    return {"prior": 1024, "pairs": pairs, "rounds": -(-(pairs + 1) // 64), "gain_stats_ms": stats, "cost_ms": cost, "cost_ratio_to_gain_stats": cost / stats,
            "path_ms": path, "path_us_per_pair": path * 1e3 / pairs, "ms_wall": wall, "last_ms": last,
            "render": {"ms": ms, "ratio_to_last": ms / last}, "render_gain": {"ms": msg, "ratio_to_ungained": msg / ms},
            "mean_total": float(total[1:].astype(np.float64).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strip_cost.json"))
    a = ap.parse_args()
    reps = max(20, a.repeats)
    n, rows, cols, pitch = 64, 360, 640, 128
    ctx = uw.Context(0)
    rng = np.random.default_rng(1)
    frames = torch.from_numpy(rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)).cuda()
    H = np.tile(np.array([1.0, 0, float(pitch), 0, 1.0, 0, 0, 0, 1.0]), (n, 1))
    s = uw.Strip(ctx, rows, cols, batch=16, max_frames=n)
    dH, dr = torch.from_numpy(H).cuda(), torch.full((n,), 0.5, dtype=torch.float32, device="cuda")
    for k in range(0, n, 16):
        s.add(frames[k:k + 16], dH[k:k + 16].contiguous(), dr[k:k + 16].contiguous())
    t0 = time.perf_counter()
    seg = s.layout()[0]
    layout_ms = (time.perf_counter() - t0) * 1e3
    assert seg.count == n and seg.cols == cols + (n - 1) * pitch and seg.rows == rows
    out = {"frames": n, "frame": [rows, cols], "pitch_px": pitch, "canvas": [seg.rows, seg.cols], "repeats": reps, "layout_ms_wall": layout_ms,
           "render": {},
           "cull_1024_frames_960_outside": "frames outside a segment are never visited: 0 by construction"}
    canvas = torch.empty((seg.rows, seg.cols, 3), dtype=torch.uint8, device="cuda")
    for mode in ("feather", "first", "last"):
        _, cover = s.render(0, mode, cover=True, out=canvas)
        covered = int(cover.to(torch.int64).sum())
        for _ in range(3):
            s.render(0, mode, out=canvas)
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(reps):
            s.render(0, mode, out=canvas)
        ms, launches = ctx.prof_results()["k_strip_render"]
        ctx.prof_enable(False)
        ms /= launches
        out["render"][mode] = {"ms": ms, "canvas_mpix_per_s": seg.rows * seg.cols / ms / 1e3, "covered_pixel_frames_per_s": covered / ms * 1e3,
                               "covered_pixel_frames": covered}
    # gain compensation: `gains` = the memset, k_strip_gain_stats over 63 pairs and k_strip_gain_solve (device events per kernel,
    # and wall clock around a drained stream for the whole call), then the gained render in each mode
    for _ in range(3):
        s.gains()
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(reps):
        s.gains()
    prof = ctx.prof_results()
    ctx.prof_enable(False)
    t0 = time.perf_counter()
    for _ in range(reps):
        s.gains()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    stats_ms, solve_ms = (prof[k][0] / prof[k][1] for k in ("k_strip_gain_stats", "k_strip_gain_solve"))
    out["gains"] = {"stats_ms": stats_ms, "solve_ms": solve_ms, "ms": stats_ms + solve_ms, "ms_wall": wall, "pairs": n - 1,
                    "pair_mpix_per_s": (n - 1) * rows * cols / stats_ms / 1e3}
    out["render_gain"] = {}
    for mode in ("feather", "first", "last"):
        for _ in range(3):
            s.render(0, mode, out=canvas, gain=True)
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(reps):
            s.render(0, mode, out=canvas, gain=True)
        ms, launches = ctx.prof_results()["k_strip_render_gain"]
        ctx.prof_enable(False)
        ms /= launches
        out["render_gain"][mode] = {"ms": ms, "ratio_to_ungained": ms / out["render"][mode]["ms"]}
    # the device-to-device copy of the algorithmic bytes: the canvas written plus every frame read once
    nbytes = seg.rows * seg.cols * 3 + n * rows * cols * 3
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / reps
    out["d2d_copy"] = {"bytes": nbytes, "ms": copy_ms, "gb_per_s": 2 * nbytes / copy_ms / 1e6}
    for mode in out["render"]:
        out["render"][mode]["ratio_to_d2d_copy"] = out["render"][mode]["ms"] / copy_ms
    # multi-band blending on the same strip: the stacks of the 64 frames, then the render next to this run's FEATHER
    out["multiband"] = multiband(ctx, s, canvas, reps, out["render"]["feather"]["ms"], copy_ms, gained=True)
    out["seams"] = seams(ctx, s, canvas, reps, n - 1)          # after the gains of `multiband`'s caller: the costs use them
    s.close()
    del frames, canvas, src, dst
    # culling inside a segment: 1024 frames 15 px apart
    n2, pitch2 = 1024, 15
    f2 = torch.from_numpy(rng.integers(0, 256, (16, rows, cols, 3), dtype=np.uint8)).cuda()
    H2 = torch.from_numpy(np.tile(np.array([1.0, 0, float(pitch2), 0, 1.0, 0, 0, 0, 1.0]), (16, 1))).cuda()
    r2 = torch.full((16,), 0.5, dtype=torch.float32, device="cuda")
    s = uw.Strip(ctx, rows, cols, batch=16, max_frames=n2)
    for k in range(0, n2, 16):
        s.add(f2, H2, r2)
    seg2 = s.layout()[0]
    assert seg2.count == n2 and seg2.cols == cols + (n2 - 1) * pitch2
    canvas2 = torch.empty((seg2.rows, seg2.cols, 3), dtype=torch.uint8, device="cuda")
    _, cover2 = s.render(0, "feather", cover=True, out=canvas2)
    covered2 = n2 * rows * cols                              # every frame lies wholly inside (the cover plane saturates at 255)
    s.render(0, "feather", out=canvas2)
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(reps):
        s.render(0, "feather", out=canvas2)
    ms2, l2 = ctx.prof_results()["k_strip_render"]
    ctx.prof_enable(False)
    ms2 /= l2
    f64 = out["render"]["feather"]
    out["cull_in_segment_1024_frames"] = {"canvas": [seg2.rows, seg2.cols], "pitch_px": pitch2, "ms": ms2, "covered_pixel_frames": covered2,
                                          "ns_per_covered_pixel_frame": ms2 * 1e6 / covered2,
                                          "ns_per_covered_pixel_frame_64_frames": f64["ms"] * 1e6 / f64["covered_pixel_frames"]}
    s.gains()
    mb2 = multiband(ctx, s, canvas2, reps, ms2, 0.0, gained=True)
    mb2["feather_ms"] = ms2
    out["multiband_1024_frames"] = mb2
    out["seams_1024_frames"] = seams(ctx, s, canvas2, reps, n2 - 1)
    s.close()
    del f2, canvas2, cover2
    # add through resize, detect and match: 16 frames per call, the stream drained around the timed calls
    m = 48
    stream = torch.from_numpy(synth.uw_stream(0, m, rows, cols, step_frac=0.2)).cuda()
    s = uw.Strip(ctx, rows, cols, batch=16, max_frames=m)
    s.add(stream[:16])                                       # warm-up: workspaces, tables
    t0 = time.perf_counter()
    s.add(stream[16:32])
    s.add(stream[32:48])
    out["add_ms_per_frame_wall"] = (time.perf_counter() - t0) * 1e3 / 32
    t0 = time.perf_counter()
    segs = s.layout()
    out["layout_48_frames_ms_wall"] = (time.perf_counter() - t0) * 1e3
    out["matched_segments"] = [[g.first, g.count, g.rows, g.cols] for g in segs]
    s.close()
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
