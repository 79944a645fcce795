#!/usr/bin/env python3
"""bench.py -- frames/s of the per-frame pipe on synthetic 1080p frames.

  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A "step" is one pass of the hot path (bgdehaze -> histretch -> aclahe ->
videostrip-overlap) over one batch of synthetic 1920x1080 uchar3 frames that is
already resident in HBM.  Frames are independent units: with N > 1 every rank
runs the same per-GPU batch on its own GPU (weak scaling, no data-path
collective; torch.distributed is used only for the barrier and the max-over-
ranks time).  Rank 0 prints ONE JSON line with the whole-job frames/s.  A plain
run does only that; with --full the line also carries the self-checks, the HBM
roofline of the dominant kernel (timed live with HIP events on the launch
stream) and the CPU baseline (the oracle, timed on a bounded sample).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES hardware queues (default 4).  A rank has four
# sub-batch streams, the two copier lanes and the default stream: with 4 queues sub-batch streams share one and run
# strictly one after the other (measured, 4 sub-batches of 64 frames: 2650 frames/s with 4 queues, 2750 with 8 or 16;
# 8 sub-batches of 64 frames on 16 queues: 2880).  Must be set before the
# runtime initialises; a deployment sets it the same way.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# The library's defaults are the reference's rules (uwip.h).  The bench opts into ONE deviation and says so in `config.rules`:
# UWIP_DEHAZE_GUARD_S -- as written, one 0/0 in the exposure map S (BGDehaze.py:83) turns a whole frame into NaN -> black
# (SURVEY B-11), and a black frame is a trivial workload for every stage after it: a synthetic frame that happens to hit it
# would make the timed step cheaper, not dearer.  The overlap rule is the reference's (>= 4 good matches).
GUARD_S = True


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", choices=["1080p", "4k", "4k-paced"], default="1080p",
                    help="1080p: BASELINE.json's metric (default); 4k: the same pipe on 3840x2160 frames (configs 3/5), 128 frames per "
                         "step; 4k-paced: config 5's stream mode -- 600 frames arriving at 60 fps through host buffers, then unpaced")
    ap.add_argument("--frames", type=int, default=None, help="frames per GPU per step (default 512 at 1080p, 128 at 4K)")
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--cols", type=int, default=None)
    ap.add_argument("--paced-fps", type=float, default=60.0)
    ap.add_argument("--paced-frames", type=int, default=600)
    ap.add_argument("--paced-batch", type=int, default=1,
                    help="frames gathered before the pipe runs (latency vs launch size; measured at 4K@60: batch 1 -> 7 ms worst "
                         "arrival-to-delivery latency, 2 -> 29 ms, 4 -> 67 ms, all three keep up)")
    ap.add_argument("--streams", type=int, default=8, help="independent sub-batches in flight per GPU (HIP streams + host threads)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one handed its caller as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the self-checks, the host-buffer leg, the per-kernel / roofline pass, the "
                         "further scenes, the 4K leg and the CPU baseline; the --no-* / --scenes options below apply to these")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-matcher-bench", dest="matcher_bench", action="store_false",
                    help="skip the 2048 x 2048 matcher measurement (MFMA utilisation on BASELINE config 4's size)")
    ap.add_argument("--no-large-working-set", dest="large_ws", action="store_false",
                    help="skip the 1 GB single-launch measurement of k_clahe_apply (profiling runs: keeps the counter averages of "
                         "that kernel to the step's own launches)")
    ap.add_argument("--no-host-buffers", dest="host_buffers", action="store_false",
                    help="skip the upload/download-inclusive variant (timed on every rank after the main region)")
    ap.add_argument("--no-4k", dest="fourk", action="store_false",
                    help="skip the short 3840x2160 leg of the default line (configs 3 / 5: 6 steps + a 2 s paced 4K@60 stream)")
    ap.add_argument("--scenes", type=int, default=3,
                    help="synthetic scenes (different seed0) the timed region is repeated on after the headline scene: the cost of "
                         "the sweep depends on how many clip limits still clip, i.e. on the scene; the line reports each scene's "
                         "frames/s and sweep time and their min / median / max (1 = the headline scene only)")
    ap.add_argument("--no-pin", dest="pin", action="store_false",
                    help="do not restrict the rank to the CPUs of its GPU's NUMA node")
    a = ap.parse_args()
    big = a.config != "1080p"
    a.rows = a.rows or (2160 if big else 1080)
    a.cols = a.cols or (3840 if big else 1920)
    a.frames = a.frames or (128 if big else 512)
    return a


def synth_frames(n, H, W, seed0):
    """n consecutive frames of the synthetic underwater stream (one corner-rich scene, consecutive frames related
    by a known homography -- translation 3 % of the width + yaw <= 1 degree + zoom <= 1 % per frame, synth.uw_stream_motion),
    generated on the host cores in parallel"""
    from concurrent.futures import ThreadPoolExecutor
    from uwimageproc_amd import synth
    chunk = 4
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as ex:
        parts = list(ex.map(lambda k: synth.uw_stream_motion(k * chunk, min(chunk, n - k * chunk), H, W, seed0=seed0), range((n + chunk - 1) // chunk)))
    return np.concatenate(parts, axis=0)


def paced_stream(args, dev_index, dev, H, W):
    """BASELINE config 5's stream mode on this GPU: `paced_frames` frames of HxW arrive in page-locked host memory at
    `paced_fps`; every `paced_batch` frames the pipe runs (upload -> four stages -> download, one stream, frame order kept
    so the overlap chain is the stream's).  Reports the sustained rate and the worst arrival-to-result latency."""
    from uwimageproc_amd.pipeline import FramePipe
    B, n, fps = args.paced_batch, args.paced_frames, args.paced_fps
    frames = synth_frames(max(B, 8), H, W, 4321)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        pipe = FramePipe(dev_index, B, H, W, guard_s=GUARD_S)
    h_in, h_out = pipe.host_buffers()
    for w in range(2):                                   # warm-up: workspaces, tables
        h_in[...] = frames[:B]
        pipe.run_host(h_in, h_out)
        pipe.sync()                                      # compute stream AND both copy lanes
    sentinel_ok = True
    t0 = time.perf_counter() + 0.05
    lat, finish = [], t0
    for k in range(0, n - n % B, B):
        arrive_last = t0 + (k + B - 1) / fps
        now = time.perf_counter()
        if now < arrive_last:
            time.sleep(arrive_last - now)                # the batch is complete when its last frame has arrived
        for j in range(B):
            h_in[j] = frames[(k + j) % len(frames)]      # the "camera" writes into the pinned ring
        h_out[-1, -1, -1, :] = (1, 2, 3)                 # no dehazed + stretched frame ends in these bytes twice: proves the D2H landed
        _, t_out = pipe.run_host(h_in, h_out)
        pipe.wait_ticket(t_out)                          # the result is in h_out (the download lane has finished)
        pipe.ctx.sync()                                  # ... and the batch's overlap ratios are final (they follow the download request)
        finish = time.perf_counter()
        sentinel_ok = sentinel_ok and tuple(h_out[-1, -1, -1, :]) != (1, 2, 3)
        lat += [finish - (t0 + (k + j) / fps) for j in range(B)]
    done = len(lat)
    pipe.close()                                         # frees the host buffers too
    return {"frames": done, "arrival_fps": fps, "batch": B, "sustained_fps": done / (finish - t0),
            "keeps_up": bool(max(lat) < (B / fps) * 2 + 0.25), "worst_latency_ms": max(lat) * 1e3,
            "median_latency_ms": float(np.median(lat)) * 1e3, "result_seen_in_host_buffer": bool(sentinel_ok),
            "note": "latency = result downloaded - frame arrival; a frame waits for its batch to fill, then for upload + pipe + download"}


def cpu_baseline(H, W, spot=None):
    """The CPU restatement of the same per-frame pipe (kind = "port": the reference's OpenCV / numpy path itself cannot
    be built or imported here), plain C compiled `-O3 -march=native` on this host when gcc is present
    (else the prebuilt -O2 library), at the bench's full frame size:
      (i) one thread: one frame through dehaze -> histretch -> V -> sweep -> parameter choice -> CLAHE -> HSV merge,
          plus the overlap stage of one frame (detect + describe + match + homography);
     (ii) all host cores: one frame per thread (frames are independent), `cores` read at run time.
    Returns the cpu_baseline object."""
    import ctypes as C
    import subprocess
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _oracle
    from uwimageproc_amd import synth
    from uwimageproc_amd._native import lib as uwip_lib
    odir = os.path.join(ROOT, "oracle")
    srcs = sorted(os.path.join(odir, f) for f in os.listdir(odir) if f.endswith(".c"))
    build = "prebuilt oracle/liboracle.so (-O2)"
    orc = None
    try:
        so = os.path.join(tempfile.mkdtemp(prefix="uwip_cpu_"), "liboracle_native.so")
        subprocess.run(["gcc", "-O3", "-march=native", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-std=c11", "-o", so] + srcs + ["-lm"],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
        orc = _oracle.Oracle(C.CDLL(so))
        build = "gcc -O3 -march=native -ffp-contract=off (built on this host)"
    except Exception:
        orc = _oracle.load()
    # The parameter choice inside the CPU baseline and the spot check: the scipy mirror of the reference's own calls
    # (tests/_knee_mirror.py: curve_fit / splrep / splev as functions.py:49-93 makes them) when scipy imports -- a checker
    # independent of the product's MINPACK restatement; only without scipy the product's host function uwip_aclahe_select
    # (0.5 ms of ~2.9 s per frame) stands in, and `select_kind` says which it was.
    _sel_c = uwip_lib().uwip_aclahe_select
    try:
        import _knee_mirror
        import scipy.optimize  # noqa: F401
        select_kind = "scipy mirror of functions.py:49-93 (tests/_knee_mirror.py)"

        def select(tab):
            return _knee_mirror.select_parameters(np.asarray(tab, np.float32).reshape(5, 51))
    except Exception:
        select_kind = "uwip_aclahe_select (product host function: scipy not importable here)"

        def select(tab):
            bs, cl = C.c_int32(0), C.c_int32(0)
            t = np.ascontiguousarray(tab, np.float32)
            _sel_c(t.ctypes.data_as(C.POINTER(C.c_float)), 1, C.byref(bs), C.byref(cl), None)
            return bs.value, cl.value

    def one_frame(idx, timing=None):
        img = synth.uw_stream_motion(idx, 2, H, W)
        t = [time.perf_counter()]
        out, _ = orc.dehaze(img[1], 15, full=True, guard_s=GUARD_S); t.append(time.perf_counter())
        st, _ = orc.histretch(out, "RGB")
        v = orc.bgr_to_v(st)
        tab = np.ascontiguousarray(orc.sweep(orc.gaussian3(v)), np.float32); t.append(time.perf_counter())
        bs, cl = select(tab); t.append(time.perf_counter())
        fin = orc.hsv_replace_v(st, orc.clahe(v, float(cl), bs, bs)); t.append(time.perf_counter())
        # overlap against the predecessor: the key frame's features are cached (kframe->new_img), so one detect+describe,
        # one match + homography + overlapArea per frame
        g1 = orc.resize_gray(fin)
        k1, d1, _ = orc.detect_describe(g1)
        k0, d0, _ = orc.detect_describe(orc.resize_gray(img[0])) if timing is not None else (k1, d1, 0)
        t.append(time.perf_counter())
        idxm, dist = orc.match_knn2(d1, d0)
        gq, gt = orc.ratio_test(idxm, dist, len(d0))
        if len(gq) >= 4:
            _, Hm = orc.find_homography(k1["x"][gq], k1["y"][gq], k0["x"][gt], k0["y"][gt], g1.shape[1], g1.shape[0], seed=1)
            orc.overlapArea(Hm, W, H)
        t.append(time.perf_counter())
        if timing is not None:
            d = np.diff(t)
            timing.update({"dehaze_s": d[0], "histretch_sweep_s": d[1], "select_s": d[2], "clahe_hsv_s": d[3],
                           "overlap_s": d[4] / 2 + d[5]})          # d[4] held two detect+describe passes
        return 0

    check = None
    if spot is not None:
        try:
            check = spot_check_vs_oracle(orc, select, spot)
        except Exception as ex:
            check = {"ok": False, "error": f"{type(ex).__name__}: {str(ex)[:200]}"}
    parts = {}
    t0 = time.perf_counter()
    one_frame(0, parts)
    single = sum(parts.values())
    cores, quota = host_cpus()
    # a bounded sample: one frame per core the job may really use (the affinity mask, cut to the cgroup's CPU quota
    # when there is one), at most 256 and at most what half of the free memory holds at ~0.7 GB per frame in flight
    try:
        free_gb = os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE") / 2**30
    except (ValueError, OSError):
        free_gb = 64.0
    n = max(1, min(cores, int(np.ceil(quota)) if quota else cores, 256, int(free_gb / 2 / 0.7)))
    # two passes, the better one counts: the host is shared, and one pass in some dozens has come out 2-3x slow
    walls = []
    for _ in range(2):
        t1 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=n) as ex:
            list(ex.map(one_frame, range(1, n + 1)))
        walls.append(time.perf_counter() - t1)
    wall = min(walls)
    return {"value": n / wall, "unit": "frames/s", "cores": n, "cores_visible": cores, "cgroup_cpu_quota": quota, "kind": "port",
            "spot_check_vs_oracle": check, "parameter_choice": select_kind,
            "sample": f"{n} frames of {W}x{H}, one per host thread ({cores} CPUs in the affinity mask, cgroup quota "
                      f"{quota if quota else 'none'}), whole pipe in C ({build}), best of two passes; single thread: 1 frame; "
                      f"the ACLAHE parameter choice inside it: {select_kind}",
            "single_thread": {"value": 1.0 / single, "unit": "frames/s", "cores": 1, "seconds_per_frame": single, "parts": parts},
            "all_cores_wall_s": wall, "all_cores_walls_s": walls, "total_cpu_baseline_s": time.perf_counter() - t0}


def outputs_identical(rig):
    """The S sub-batches of a rank hold the same frames (Rig.__init__), so after any number of steps every sub-batch pipe
    must hold byte-identical enhanced frames, the same ACLAHE parameters and the same overlap ratios: a free check of
    the 8-stream arrangement the headline is timed on (call after rig.drain())."""
    p0 = rig.pipes[0]
    ok = True
    for p in rig.pipes[1:]:
        ok = ok and bool(torch.equal(p.work, p0.work)) and bool(torch.equal(p.ratio, p0.ratio)) and list(p.params) == list(p0.params)
    return ok


DUMP_FRAME_BYTES = 48 << 20      # the enhanced frames' share of --dump-outputs (everything together stays under 64 MB)


def dump_outputs(rig, path):
    """What the last timed step handed its caller (FramePipe.run -> uwip_pipe_step, then uwip_pipe_last_params), frames in
    sub-batch order, so that two builds can be compared output for output on the same seeded inputs (call after rig.drain()):
      enhanced.npy               float32 [F, H, W, 3] -- or, when that exceeds DUMP_FRAME_BYTES, [F, P, 3]: every frame at
                                 the same P pixel positions, a fixed seeded sample listed in enhanced_pixel_index.npy
      enhanced_pixel_index.npy   float64 [P] row-major pixel indices (y * W + x), only when sampled
      overlap_ratio.npy          float32 [F]
      aclahe_params.npy          float64 [F, 2] (BS, CL) of every frame"""
    os.makedirs(path, exist_ok=True)
    F, H, W = rig.F, rig.H, rig.W
    out = {"overlap_ratio": torch.cat([p.ratio for p in rig.pipes]).float().cpu().numpy(),
           "aclahe_params": np.array([bc for p in rig.pipes for bc in p.params], dtype=np.float64)}
    if F * H * W * 3 * 4 <= DUMP_FRAME_BYTES:
        out["enhanced"] = torch.cat([p.work for p in rig.pipes]).float().cpu().numpy()
    else:
        P = max(1, min(H * W, DUMP_FRAME_BYTES // (F * 3 * 4)))
        pix = np.sort(np.random.default_rng(20240611).choice(H * W, P, replace=False))
        idx = torch.from_numpy(pix).to(rig.dev)
        out["enhanced"] = torch.cat([p.work.view(rig.Fs, H * W, 3).index_select(1, idx) for p in rig.pipes]).float().cpu().numpy()
        out["enhanced_pixel_index"] = pix.astype(np.float64)
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)


def spot_capture(rig, dev_index):
    """What the oracle needs to check one frame of sub-batch 0 of the TIMED arrangement: the input frames, the outputs /
    parameters / ratios the timed steps left behind, and the device's dehaze output for the same frames (a separate
    un-chained uwip_dehaze call: the oracle chain is re-synchronised there, because the float64 dehaze agrees to 1e-9
    and its 8-bit cast only away from exact rounding ties)."""
    from uwimageproc_amd.pipeline import FramePipe
    p = rig.pipes[0]
    n = min(2, rig.Fs)
    cap = {"frames": rig.parts[0][:n].cpu().numpy().copy(), "out": p.work[:n].cpu().numpy().copy(), "params": list(p.params[:n]),
           "ratio": p.ratio[:n].cpu().numpy().copy(), "vw": p.vw, "vh": p.vh, "seed": p.seed}
    with torch.cuda.stream(torch.cuda.Stream(torch.device("cuda", dev_index))):
        probe = FramePipe(dev_index, n, rig.H, rig.W, guard_s=GUARD_S)
        probe.stage_dehaze(rig.parts[0][:n])
        probe.ctx.sync()
        cap["dehazed"] = probe.work.cpu().numpy().copy()
        probe.close()
    return cap


def spot_check_vs_oracle(orc, select, cap):
    """One frame of sub-batch 0 of the timed run against the oracle chain (the checker; never the thing measured)."""
    import ctypes as C
    f = len(cap["frames"]) - 1
    o, _ = orc.dehaze(cap["frames"][f], 15, full=True, guard_s=GUARD_S)
    d = np.abs(cap["dehazed"][f].astype(np.int16) - o.astype(np.int16))
    res = {"frame_of_sub_batch_0": f, "dehaze_max_abs_diff_levels": int(d.max()), "dehaze_frac_bytes_differing": float((d != 0).mean())}
    st, _ = orc.histretch(cap["dehazed"][f], "RGB")
    v = orc.bgr_to_v(st)
    tab = np.ascontiguousarray(orc.sweep(orc.gaussian3(v)), np.float32)
    bs, cl = select(tab)
    res["params_device"] = [int(x) for x in cap["params"][f]]
    res["params_from_oracle_table"] = [int(bs), int(cl)]
    res["params_equal"] = res["params_device"] == res["params_from_oracle_table"]
    b_, c_ = cap["params"][f]
    e = orc.hsv_replace_v(st, orc.clahe(v, float(c_), int(b_), int(b_)))
    res["output_equal"] = bool(np.array_equal(e, cap["out"][f]))
    if f >= 1:
        er, _, _ = orc.calcOverlap(cap["out"][f - 1], cap["out"][f], cap["vw"], cap["vh"], seed=cap["seed"])
        res["overlap_ratio_device"] = float(cap["ratio"][f])
        res["overlap_ratio_oracle"] = float(er)
        res["overlap_abs_err"] = abs(float(cap["ratio"][f]) - float(er))
    res["ok"] = bool(res["dehaze_max_abs_diff_levels"] <= 1 and res["dehaze_frac_bytes_differing"] <= 1e-2 and res["params_equal"]
                     and res["output_equal"] and res.get("overlap_abs_err", 0.0) <= 1e-6)
    res["note"] = ("dehaze: device bytes vs the C oracle (<= 1 level at rounding ties); from the device's dehazed bytes on: histretch, "
                   "V, blur, 255-evaluation sweep table -> parameter choice, CLAHE, HSV merge byte-exact; overlap ratio of the "
                   "device's frames f-1, f recomputed by the oracle (1e-6)")
    return res


I8_MFMA_PEAK_TOPS = 5000.0     # dense i8 = 2x the ~2.5 PFLOP/s dense BF16 rate (MI355X_MICROARCH.md, Matrix cores)
FP4_MFMA_PEAK_TOPS = 10000.0   # dense FP4 / FP6 through v_mfma_scale_f32_*_f8f6f4 = 4x BF16 per clock (same guide)


def matcher_form():
    """(form id, operand name) the library's matcher runs (UWIP_MATCH_FORM; default 4 = FP4 E2M1 operands, 3 = round 4's i8)"""
    f = int(os.environ.get("UWIP_MATCH_FORM", "4") or 4)
    return f, ("fp4 (E2M1 nibbles, v_mfma_scale_f32_16x16x128_f8f6f4)" if f in (4, 5, 6) else "i8 (0/1 bytes, v_mfma_i32_16x16x64_i8)")
# VALU issue: 1024 SIMDs.  The f32 rate in MI355X_MICROARCH.md (157 TFLOP/s vector f32 = 128 FMA lanes per CU and clock)
# is one wave64 instruction per SIMD every 2 clocks = 1229 G wave-instr/s at 2.4 GHz; on this chip a dependent-free
# stream of v_mul/v_add/v_fma_f32 issues one per 1.14 ns per SIMD (tools/ubench/valu_rate.hip) = 898 G/s, and the
# conversions / byte permutes / shift-adds the CLAHE kernels are made of take 1.83 ns.
VALU_SPEC_GINSTR = 1024 * 2.4 / 2.0
VALU_PEAK_GINSTR = 1024 / 1.14

# kernel name -> stage of the pipe
STAGE_OF = [("k_ov_", "overlap"), ("k_hist_u8", "histretch"), ("k_compose_luts", "histretch"), ("k_stretch_lut", "histretch"),
            ("k_apply_lut", "histretch"), ("k_bgr_to_v", "aclahe"), ("k_clahe_", "aclahe"), ("k_entropy", "aclahe"),
            ("k_hsv_replace_v", "aclahe"), ("k_gauss3", "aclahe")]
# SURVEY.md 8(d) algorithmic bytes per pixel (N = W*H):
#   histretch "RGB": read 3N + write 3N (apply).  SURVEY 8(d) also counts a 3N histogram read; in the chained call
#           the dehaze writer counts its own bytes (k_exp_out<1,HIST>), so that read does not happen          =   6 N
#   aclahe: sweep minimum 5 grids x 2N + final apply 3N = 13 N (8d), plus the colour conversions around it
#           (BGR -> V: 3N + N; HSV merge: 3N + N read, 3N write)                                         =  24 N
#   bgdehaze, from the implemented float64 pass list: k_winfilter15 3+6, k_bglight 3,
#           filter 1 solve 3+2+64, final 64+3+16, k_exp_prep 3+16+3+1, k_exp_S 3+1+8, filter 3 solve 3+8+32,
#           final 32+3+8, k_exp_out pass 0 3+16+8, pass 1 3+16+8+3                                       = 342 N
STAGE_BYTES_PER_PIXEL = {"histretch": 6.0, "aclahe": 24.0, "bgdehaze": 342.0}


def stage_of(kernel):
    for pre, st in STAGE_OF:
        if kernel.startswith(pre):
            return st
    return "bgdehaze"


def pmc_provenance(name, d):
    """which committed digest a replayed counter figure comes from: file, sha256, and -- written into it by
    tools/pmc_digest.py -- the tree it was taken from (git HEAD + dirty flag) and when"""
    import hashlib
    path = os.path.join(ROOT, "profiles", name)
    meta = d.get("_meta", {}) if isinstance(d, dict) else {}
    return {"file": f"profiles/{name}", "sha256_16": hashlib.sha256(open(path, "rb").read()).hexdigest()[:16],
            "mtime": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(os.path.getmtime(path))),
            "git_head_at_collection": meta.get("git_head"), "tree_dirty_at_collection": meta.get("dirty"), "collected": meta.get("collected")}


def pmc_entry(kernel, rows, cols):
    """Committed counter digest of the same command (tools/pmc_digest.py over separate rocprofv3 --pmc passes; the
    counters cannot be read inside this process).  The passes are taken at 1920x1080; for another frame size the
    per-frame counters of that digest are scaled by the pixel ratio (these kernels do a fixed amount of work per pixel)
    and the entry says so.  None when no matching profile is committed."""
    for name in ("r05_pmc.json", "r04_pmc.json", "r03_pmc.json", "r02_pmc.json"):
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", name)))
            e = d.get(f"{cols}x{rows}", {}).get(kernel)
            if e is not None:
                e = dict(e)
                e["digest"] = pmc_provenance(name, d)
                return e
            e = d.get("1920x1080", {}).get(kernel)
            if e is not None:
                k = (rows * cols) / (1080.0 * 1920.0)
                s = {key: (val * k if isinstance(val, (int, float)) and key.endswith("_per_frame") or key.endswith("per_frame_fetch_as_reported") else val)
                     for key, val in e.items()}
                s["scaled_from"] = f"1920x1080 counters x {k:.3f} (pixel ratio)"
                s["digest"] = pmc_provenance(name, d)
                return s
        except Exception:
            pass
    return None


def matcher_report(ctx, dev, pairs=64):
    """k_ov_match on a full 2048 x 2048 synthetic descriptor set per pair (BASELINE config 4 / SURVEY 8d):
    ops = 2 * Kq * Kt * 512 per pair, timed with HIP events, against the dense i8 MFMA peak."""
    import ctypes as C
    rng = np.random.default_rng(7)
    K = 2048
    fh = C.c_void_p()
    ctx.call("uwip_features_create", 2 * pairs, C.byref(fh))
    kps = np.zeros((K, 8), dtype=np.int32)
    kv = kps.view(np.float32)
    kv[:, 0] = rng.uniform(8, 632, K); kv[:, 1] = rng.uniform(8, 352, K)
    for slot in range(2 * pairs):
        desc = rng.integers(0, 256, (K, 64), dtype=np.uint8)
        desc[:, 60] &= 0x3f; desc[:, 61:] = 0                       # 486 payload bits, padded to 512
        ctx.call("uwip_features_upload", fh, slot, 360, 640, C.c_void_p(kps.ctypes.data), C.c_void_p(desc.ctypes.data), K)
    pq = (C.c_int32 * pairs)(*[2 * i for i in range(pairs)])
    pt = (C.c_int32 * pairs)(*[2 * i + 1 for i in range(pairs)])
    ratio = torch.empty((pairs,), dtype=torch.float32, device=dev)
    ctx.prof_reset(); ctx.prof_enable(True)
    reps = 3
    for _ in range(reps):
        ctx.call("uwip_overlap_match", fh, fh, pq, pt, pairs, 1920, 1080, 1, C.c_void_p(ratio.data_ptr()), None, None, None, None)
    ctx.sync()
    res = ctx.prof_results()
    ctx.prof_enable(False)
    ctx._l.uwip_features_destroy(fh)
    ms, cnt = res["k_ov_match"]
    avg = ms / cnt
    ops = 2.0 * K * K * 512 * pairs
    tops = ops / (avg * 1e-3) / 1e12
    form, operands = matcher_form()
    peak = FP4_MFMA_PEAK_TOPS if form in (4, 5, 6) else I8_MFMA_PEAK_TOPS
    out = {"kernel": "k_ov_match", "form": form, "operands": operands,
           "workload": f"{pairs} pairs x ({K} x {K}) 512-bit descriptors (config 4)", "ops_per_launch": ops,
           "avg_launch_ms": avg, "achieved": tops, "peak": peak, "unit": "TOP/s", "frac": tops / peak,
           "frac_of_i8_peak": tops / I8_MFMA_PEAK_TOPS, "frac_of_fp4_peak": tops / FP4_MFMA_PEAK_TOPS,
           "peaks": {"i8_dense_TOPs": I8_MFMA_PEAK_TOPS, "fp4_dense_TOPs": FP4_MFMA_PEAK_TOPS},
           "bound": "mfma"}
    try:                                                     # MFMA counters of the committed rocprofv3 --pmc pass of tools/matcher_only.py
        mp = "r05_matcher_pmc.json" if os.path.exists(os.path.join(ROOT, "profiles", "r05_matcher_pmc.json")) else "r04_matcher_pmc.json"
        out["mfma_counters"] = json.load(open(os.path.join(ROOT, "profiles", mp)))
        out["mfma_counters_digest"] = pmc_provenance(mp, out["mfma_counters"])
    except Exception:
        out["mfma_counters"] = None
    return out


def hbm_copy_rate(ctx, dev):
    """Measured copy bandwidth of this chip beside the nominal 8 TB/s: the library's own streaming
    kernel (k_apply_lut with identity tables: 16 B per lane, read + write in place) on a 1 GB buffer."""
    import ctypes as C
    from uwimageproc_amd import batch_of
    F, H, W = 162, 1080, 1920                                 # 162 x 6.22 MB = 1.008 GB
    buf = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev)
    lut = torch.arange(256, dtype=torch.uint8, device=dev).repeat(F, 3, 1).contiguous()
    b = batch_of(buf)
    ctx.call("uwip_apply_lut", C.byref(b), C.c_void_p(lut.data_ptr()))
    ctx.sync()
    ctx.prof_reset(); ctx.prof_enable(True)
    for _ in range(5):
        ctx.call("uwip_apply_lut", C.byref(b), C.c_void_p(lut.data_ptr()))
    ctx.sync()
    r = ctx.prof_results()
    ctx.prof_enable(False)
    ms, cnt = r["k_apply_lut"]
    nbytes = 2.0 * buf.numel()
    # the yardstick proper: a plain device-to-device copy of the same 1 GB by the runtime (torch Tensor.copy_: a streaming
    # kernel with nothing but loads and stores), timed with events on torch's stream -- the achievable rate every "fraction of
    # achievable" argument leans on (MI355X_MICROARCH.md measures 6.29 TB/s for a float4 copy).  k_apply_lut is NOT a copy:
    # every byte goes through a per-channel table in LDS (16 ds_read_u8 per 16-byte lane access), which is what its lower
    # figure shows.
    dst = torch.empty_like(buf)
    dst.copy_(buf)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        dst.copy_(buf)
    e1.record()
    torch.cuda.synchronize()
    copy_ms = e0.elapsed_time(e1) / 5
    del buf, lut, dst
    return {"GBps": nbytes / (copy_ms * 1e-3) / 1e9, "bytes_moved_per_launch": nbytes, "avg_launch_ms": copy_ms,
            "kernel": "runtime device-to-device copy of 1.008 GB (torch Tensor.copy_; read + write)",
            "lut_pass": {"GBps": nbytes / (ms / cnt * 1e-3) / 1e9, "avg_launch_ms": ms / cnt,
                         "kernel": "k_apply_lut (identity tables, in place: 1.008 GB read + 1.008 GB written per launch; every byte through an LDS table)"}}


def roofline_report(args, pipe, part0, dev, F, Fs, H, W):
    """roofline = the kernel with the largest share of the step (what the contract calls the dominant kernel), priced
    against the limit that binds it, with its HBM reading beside it; roofline.clahe_kernel = north_star's CLAHE kernel
    (the bilinear apply); roofline.clahe_whole = all kernels of one cv::CLAHE::apply against SURVEY 8(d)'s 3N bytes for
    the five grids of the sweep on the pipe's own V planes; roofline.matcher = k_ov_match against the dense i8 MFMA peak."""
    import ctypes as C
    from uwimageproc_amd import batch_of
    N = H * W
    ctx = pipe.ctx
    ctx.prof_reset()
    ctx.prof_enable(True)
    nprof = max(1, min(args.steps, 3))
    for _ in range(nprof):
        pipe.run(part0)
    torch.cuda.synchronize()
    res = ctx.prof_results()
    ctx.prof_enable(False)
    # one pass of sub-batch 0 = Fs frames on one stream; the step is S such passes on S streams
    kernels = {k: {"ms_per_subbatch": ms / nprof, "launches_per_subbatch": cnt / nprof, "stage": stage_of(k)} for k, (ms, cnt) in res.items()}
    if "k_clahe_apply" not in res:
        return None, kernels
    tot = sum(v["ms_per_subbatch"] for v in kernels.values())

    def hbm_entry(kernel, bytes_per_frame, frames_per_launch, ms, cnt):
        avg_ms = ms / cnt
        per_launch = bytes_per_frame * frames_per_launch
        ach = per_launch / (avg_ms * 1e-3) / 1e9
        e = pmc_entry(kernel, H, W)
        traffic = None if e is None else e["hbm_bytes_per_frame"] * frames_per_launch
        return {"bound": "hbm", "kernel": kernel, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                "traffic": traffic, "traffic_over_algorithmic": None if traffic is None else traffic / per_launch,
                "traffic_source": None if e is None else "committed rocprofv3 --pmc passes of the same command (profiles/*_pmc.json: "
                                  "2 x FETCH_SIZE + WRITE_SIZE per launch), not re-measured in this run",
                "traffic_digest": None if e is None else e.get("digest"),
                "avg_launch_ms": avg_ms, "algorithmic_bytes_per_launch": per_launch}

    # (1) the kernel with the largest share of the step
    dom_name = max(kernels.items(), key=lambda kv: kv[1]["ms_per_subbatch"])[0]
    dms, dcnt = res[dom_name]
    if dom_name.startswith("k_clahe_sweep"):
        # the sweep's algorithmic minimum is one read of the V plane per grid-size launch = N per frame
        hb = hbm_entry(dom_name, 1.0 * N, Fs, dms, dcnt)        # every grid-size launch covers the whole sub-batch
        hb["algorithmic_note"] = "8(d): one read of the V plane per grid size (N B per frame per launch)"
    elif dom_name.startswith("k_gf_ws_solve"):
        hb = hbm_entry(dom_name, (3 + 5 + 48) * N, Fs, dms, dcnt)
        hb["algorithmic_note"] = ("per frame, averaged over the two launches of a step (filter 1: guide 3N + two 8-bit p planes 2N read, "
                                  "64N written; filter 3: 3N + 8N read, 32N written)")
    elif dom_name.startswith("k_gf_ws_final"):
        hb = hbm_entry(dom_name, (48 + 3 + 12) * N, Fs, dms, dcnt)
        hb["algorithmic_note"] = "per frame, averaged over the two launches of a step (filter 1: 64N + 3N read, 16N written; filter 3: 32N + 3N, 8N)"
    else:
        hb = {"bound": "hbm", "kernel": dom_name, "avg_launch_ms": dms / dcnt, "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
              "frac": None, "traffic": None}
    e = pmc_entry(dom_name, H, W)
    valu = lds = None
    if e is not None and e.get("valu_insts_per_frame"):
        ginstr = e["valu_insts_per_frame"] * Fs / ((dms / dcnt) * 1e-3) / 1e9          # every launch covers the whole sub-batch
        valu = {"wave_instr_per_launch": e["valu_insts_per_frame"] * Fs, "achieved_Ginstr_per_s": ginstr,
                "peak_Ginstr_per_s": VALU_PEAK_GINSTR, "frac": ginstr / VALU_PEAK_GINSTR,
                "spec_peak_Ginstr_per_s": VALU_SPEC_GINSTR, "frac_of_spec": ginstr / VALU_SPEC_GINSTR,
                "mean_ns_per_instr_per_simd": 1024.0 / ginstr,
                "source": "SQ_INSTS_VALU of the committed rocprofv3 --pmc pass (profiles/), time from this run.  peak = the "
                          "measured issue rate of plain f32 operations (one per 1.14 ns per SIMD, tools/ubench/valu_rate.hip); "
                          "the kernel's mix also holds v_cvt_f32_ubyte / v_cvt_pk_u8_f32 / v_lshl_add at 1.83 ns, so "
                          "mean_ns_per_instr_per_simd against 1.14 .. 1.83 says how busy the issue port is; spec_peak = one "
                          "wave64 f32 instruction per 2 clocks at 2.4 GHz (128 FMA lanes per CU and clock)"}
    if e is not None and e.get("lds_idx_active_per_frame"):
        # the LDS pipe of a CU beside the issue ports: SQ_LDS_IDX_ACTIVE summed over the 256 CUs, 2.4 GHz
        cyc_cu = e["lds_idx_active_per_frame"] * Fs / 256.0
        lds = {"idx_active_cycles_per_cu_per_launch": cyc_cu, "busy_frac": cyc_cu / ((dms / dcnt) * 1e-3 * 2.4e9),
               "bank_conflict_frac_of_active": e.get("lds_bank_conflict_per_frame", 0.0) / e["lds_idx_active_per_frame"],
               "source": "SQ_LDS_IDX_ACTIVE / SQ_LDS_BANK_CONFLICT of the committed --pmc pass, time from this run"}
    # the contract's form: the dominant kernel against the HBM roofline with SURVEY 8(d)'s algorithmic bytes (achieved, peak,
    # frac, traffic).  For the sweep that reading is ~1 % -- it evaluates ~125 CLAHE outputs per pixel from one read of the
    # plane, VALU issue and the LDS pipe bind it -- so the limits that DO bind it ride along as `valu` / `lds` /
    # `binding_limit`, next to the HBM figures, not instead of them (rounds 2-4 had the VALU reading on top: VERDICT r4).
    roof = dict(hb)
    roof["hbm_frac"] = hb.get("frac")
    roof["valu"], roof["lds"] = valu, lds
    if dom_name.startswith("k_clahe_sweep") and valu is not None:
        roof["binding_limit"] = {"what": "VALU issue + LDS pipe", "valu_frac_of_measured_issue_rate": valu["frac"],
                                 "valu_frac_of_spec_rate": valu["frac_of_spec"], "lds_busy_frac": None if lds is None else lds["busy_frac"],
                                 "note": "DESIGN.md section 5: 16.5 VALU + 1.5 LDS instructions per evaluation, 24 ns per wave-evaluation per SIMD -> "
                                         "a 7.4 ms floor for this exact-f32 formulation on the bench's frames"}
    roof["ms_per_subbatch"] = kernels[dom_name]["ms_per_subbatch"]
    roof["share_of_step"] = kernels[dom_name]["ms_per_subbatch"] / tot
    roof["is"] = "the kernel with the largest share of the step's kernel time"

    # (2) the CLAHE kernel named by north_star: the final per-frame apply (read N + write N per frame), as launched
    # by the step (one launch per 64-frame sub-batch: 265 MB at 1080p, about the size of the 256 MB Infinity Cache)
    ms, cnt = res["k_clahe_apply"]
    ck = hbm_entry("k_clahe_apply", 2.0 * N, Fs * nprof / cnt, ms, cnt)
    ck["working_set"] = "one sub-batch launch of the step (input V written by the preceding pass; may hit in the Infinity Cache)"
    ck["share_of_step"] = kernels["k_clahe_apply"]["ms_per_subbatch"] / tot
    roof["clahe_kernel"] = ck
    # (2b) the same kernel on a working set the Infinity Cache cannot hold: ONE launch over >= 1 GB (V in + out of 256
    # 1080p frames = 1.06 GB), input last touched a whole buffer ago; the pipe's own V planes, repeated
    big_f = max(Fs, int(np.ceil(1.0e9 / (2.0 * N))))
    try:
        if not args.large_ws:
            raise RuntimeError("skipped (--no-large-working-set)")
        vown = pipe.v                                         # the V planes of sub-batch 0 (left by stage_aclahe)
        vin = vown.repeat((big_f + Fs - 1) // Fs, 1, 1)[:big_f].contiguous()
        vout = torch.empty_like(vin)
        ib, ob = batch_of(vin), batch_of(vout)
        ctx.call("uwip_clahe", C.byref(ib), C.byref(ob), C.c_double(3.0), 8, 8, 0)    # warm-up: tables, workspaces
        ctx.sync()
        ctx.prof_reset(); ctx.prof_enable(True)
        for _ in range(3):
            ctx.call("uwip_clahe", C.byref(ib), C.byref(ob), C.c_double(3.0), 8, 8, 0)
        ctx.sync()
        r2 = ctx.prof_results()
        ctx.prof_enable(False)
        ms2, cnt2 = r2["k_clahe_apply"]
        big = hbm_entry("k_clahe_apply", 2.0 * N, big_f, ms2, cnt2)
        big["working_set"] = f"one launch over {big_f} frames = {2.0 * N * big_f / 1e9:.2f} GB (> 256 MB Infinity Cache), CLAHE(3.0, 8x8)"
        ck["large_working_set"] = big

        # (2c) SURVEY 8(d)'s "CLAHE kernel" is the whole apply of cv::CLAHE: 3N = read N (tile histograms) + read N + write N
        # (interpolation).  All kernels of one uwip_clahe call: tile histograms + clip / LUT + interpolation.
        def whole(r, frames, label):
            parts = {k: r[k][0] / r[k][1] for k in r if k.startswith("k_clahe_")}
            t_ms = sum(parts.values())
            ach = 3.0 * N * frames / (t_ms * 1e-3) / 1e9
            return {"bound": "hbm", "kernels": {k: v * 1e3 for k, v in parts.items()}, "kernel_time_unit": "us per launch", "frames": frames,
                    "algorithmic_bytes": 3.0 * N * frames, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                    "workload": label}
        whole_big = whole(r2, big_f, f"uwip_clahe(3.0, 8x8) on {big_f} frames in one call")
        per_grid = {}
        vs = vin[:Fs]
        vo = vout[:Fs]
        ib, ob = batch_of(vs), batch_of(vo)
        for g_ in (2, 4, 8, 16, 32):
            ctx.call("uwip_clahe", C.byref(ib), C.byref(ob), C.c_double(3.0), g_, g_, 0)
            ctx.sync()
            ctx.prof_reset(); ctx.prof_enable(True)
            for _ in range(3):
                ctx.call("uwip_clahe", C.byref(ib), C.byref(ob), C.c_double(3.0), g_, g_, 0)
            ctx.sync()
            r3 = ctx.prof_results()
            ctx.prof_enable(False)
            per_grid[f"{g_}x{g_}"] = whole(r3, Fs, f"uwip_clahe(3.0, {g_}x{g_}) on the {Fs} V planes of sub-batch 0 (one call)")
        roof["clahe_whole"] = {"large_working_set": whole_big, "sub_batch": per_grid}
        del vin, vout, vs, vo
    except Exception as e:                                    # never lose the bench line over the side measurement
        ck["large_working_set"] = {"error": str(e)[:200]}
    try:
        roof["hbm_copy_measured"] = hbm_copy_rate(ctx, dev)
        roof["hbm_copy_measured_GBps"] = roof["hbm_copy_measured"]["GBps"]
    except Exception as e:
        roof["hbm_copy_measured"] = {"error": str(e)[:200]}
    # (3) per stage: kernel time against the stage's 8(d) algorithmic bytes
    stages = {}
    for k, v in kernels.items():
        st = stages.setdefault(v["stage"], {"ms_per_subbatch": 0.0})
        st["ms_per_subbatch"] += v["ms_per_subbatch"]
    for name, st in stages.items():
        st["share_of_step"] = st["ms_per_subbatch"] / tot
        if name in STAGE_BYTES_PER_PIXEL:
            by = STAGE_BYTES_PER_PIXEL[name] * N * Fs
            st["algorithmic_bytes_per_subbatch"] = by
            st["achieved_GBps"] = by / (st["ms_per_subbatch"] * 1e-3) / 1e9
            st["frac_of_hbm_peak"] = st["achieved_GBps"] / HBM_PEAK_GBS
    roof["stages"] = stages
    roof["subbatch_kernel_ms"] = tot
    top = sorted(kernels.items(), key=lambda kv: -kv[1]["ms_per_subbatch"])[:3]
    roof["largest_kernels"] = [{"kernel": k, "ms_per_subbatch": v["ms_per_subbatch"], "share": v["ms_per_subbatch"] / tot} for k, v in top]
    # (4) the matcher against the dense i8 MFMA peak: at the step's own keypoint counts and on a full 2048 x 2048 set
    if "k_ov_match" in res:
        info = pipe.info.cpu().numpy()
        mms, mcnt = res["k_ov_match"]
        ops = float(sum(2.0 * int(r[0]) * int(r[1]) * 512 for r in info)) * 1.0
        tops = ops / ((mms / mcnt) * 1e-3) / 1e12
        mform, mops = matcher_form()
        mpeak = FP4_MFMA_PEAK_TOPS if mform in (4, 5, 6) else I8_MFMA_PEAK_TOPS
        roof["matcher"] = {"in_step": {"kernel": "k_ov_match", "form": mform, "operands": mops, "pairs": int(len(info)),
                                       "mean_keypoints": float(np.mean(info[:, 0])),
                                       "ops_per_launch": ops, "avg_launch_ms": mms / mcnt, "achieved": tops, "peak": mpeak,
                                       "unit": "TOP/s", "frac": tops / mpeak, "frac_of_i8_peak": tops / I8_MFMA_PEAK_TOPS,
                                       "frac_of_fp4_peak": tops / FP4_MFMA_PEAK_TOPS, "bound": "mfma"}}
        if args.matcher_bench:
            try:
                roof["matcher"]["config4_2048x2048"] = matcher_report(ctx, dev)
            except Exception as ex:
                roof["matcher"]["config4_2048x2048"] = {"error": str(ex)[:200]}
    return roof, kernels


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes (one per GPU) from a parent that never
    makes a GPU runtime call, relay rank 0's JSON line, and exit with the worst return code.  A rank that finds fewer
    visible devices than ranks (a 1-GPU box) shares devices and rendezvous over gloo -- a plumbing rehearsal, flagged
    "ranks_share_gpu" in the line."""
    import subprocess
    n = args.gpus
    env = dict(os.environ)
    env.update({"WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(free_port()),
                "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    procs = []
    for r in range(n):
        e = dict(env)
        e.update({"RANK": str(r), "LOCAL_RANK": str(r)})
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=e,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out, _ = procs[0].communicate()
    rc = procs[0].returncode
    for pr in procs[1:]:
        rc = max(rc, abs(pr.wait()))
    sys.stdout.write(out.decode())
    sys.stdout.flush()
    sys.exit(rc)


class Rig:
    """S independent sub-batch pipes of one rank, each on its own HIP stream and driven by its own host thread (frames are
    independent units: the HBM-bound dehaze passes of one sub-batch overlap the VALU-bound sweep and the host-side ACLAHE
    parameter choice of another), plus the rank's one copier (upload lane + download lane) for the host-buffer mode."""

    def __init__(self, dev_index, dev, F, H, W, S, seed0):
        from uwimageproc_amd import Copier
        from uwimageproc_amd.pipeline import FramePipe
        assert F % S == 0, "--frames must be divisible by --streams"
        self.F, self.H, self.W, self.S, self.Fs = F, H, W, S, F // S
        Fs = self.Fs
        # one sub-batch worth of DISTINCT consecutive frames of the synthetic stream (seed = 1234 + index), the
        # same ones for every sub-batch: every launch works on Fs different images
        self.dev = dev
        self.src = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        self.load_scene(seed0)
        self.copier = Copier(dev_index)
        self.pipes = []
        for i in range(S):
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                self.pipes.append(FramePipe(dev_index, Fs, H, W, copier=self.copier, guard_s=GUARD_S))
        self.parts = [self.src[i * Fs:(i + 1) * Fs] for i in range(S)]
        self.bufs = None

    def load_scene(self, seed0):
        """(re)fill the resident input frames with `seed0`'s scene (in place: the sub-batch views stay valid)"""
        Fs, S = self.Fs, self.S
        distinct = min(Fs, 64)
        base = synth_frames(distinct, self.H, self.W, seed0)
        one = torch.from_numpy(np.concatenate([base] * ((Fs + distinct - 1) // distinct), axis=0)[:Fs]).to(self.dev)
        torch.cuda.synchronize()
        for i in range(S):
            self.src[i * Fs:(i + 1) * Fs].copy_(one)
        torch.cuda.synchronize()
        self.seed0 = seed0
        for p in getattr(self, "pipes", []):
            p.have_prev = False                  # a new video: no key frame carried over from the old scene

    def kernel_ms(self, name, reps=2):
        """event-bracketed time of one kernel per sub-batch pass of pipe 0 (uwip_prof_*), alone on the chip"""
        p = self.pipes[0]
        p.ctx.prof_reset(); p.ctx.prof_enable(True)
        for _ in range(reps):
            p.run(self.parts[0])
        p.sync()
        r = p.ctx.prof_results()
        p.ctx.prof_enable(False)
        return r[name][0] / reps if name in r else None

    def on_all(self, fn):
        """fn(i) for every sub-batch, each on its own host thread (a uwip context is single-threaded; one per thread)"""
        import threading
        if self.S == 1:
            fn(0)
            return
        th = [threading.Thread(target=fn, args=(i,)) for i in range(1, self.S)]
        for t in th:
            t.start()
        fn(0)
        for t in th:
            t.join()

    def run_steps(self, k):
        """k steps: every sub-batch thread runs its k passes back to back (no per-step rendezvous between the host threads).
        Default since round 4: ONE host thread submits the steps of all sub-batches round robin -- nothing in a step waits on
        the host any more, so threads would only exist to submit launches (measured: the same frames/s, 0.0035 instead of
        0.01-0.03 CPU-seconds per step); UWIP_BENCH_ONE_SUBMITTER=0 brings the thread per sub-batch back."""
        if os.environ.get("UWIP_BENCH_ONE_SUBMITTER", "1") == "1":
            for _ in range(k):
                for i in range(self.S):
                    self.pipes[i].run(self.parts[i])
            return
        def loop(i):
            for _ in range(k):
                self.pipes[i].run(self.parts[i])
        self.on_all(loop)

    def host_prepare(self):
        self.bufs = [p.host_buffers() for p in self.pipes]
        for i in range(self.S):
            self.bufs[i][0][...] = self.parts[i].cpu().numpy()
        torch.cuda.synchronize()

    def run_steps_host(self, k):
        """the same k steps with every frame uploaded from and downloaded to page-locked host memory"""
        # one thread here too (it waits for the copy tickets in the order it requested them; measured equal to a thread per
        # sub-batch: 2893-2914 against 2904-2919 frames/s end to end); UWIP_BENCH_ONE_SUBMITTER=0 brings the threads back
        if os.environ.get("UWIP_BENCH_ONE_SUBMITTER", "1") == "1":
            for _ in range(k):
                for i in range(self.S):
                    p, (hi, ho) = self.pipes[i], self.bufs[i]
                    p.run_host(hi, ho, prefetch=hi)
            return
        def loop(i):
            p, (hi, ho) = self.pipes[i], self.bufs[i]
            for _ in range(k):
                p.run_host(hi, ho, prefetch=hi)
        self.on_all(loop)

    def drain(self):
        for p in self.pipes:
            p.sync()
        torch.cuda.synchronize()

    def close(self):
        for p in self.pipes:
            p.close()
        self.copier.close()
        self.pipes, self.parts, self.src, self.bufs = [], [], None, None


def barrier(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def timed(rig, world, steps, warmup, host):
    """warm-up, then EXACTLY `steps` steps bracketed by barrier + synchronize on both sides; max over ranks"""
    from uwimageproc_amd import sharding
    run = rig.run_steps_host if host else rig.run_steps
    run(warmup)
    rig.drain()
    barrier(world)
    torch.cuda.synchronize()
    c0 = time.process_time()                      # CPU seconds of ALL threads of this rank (sub-batch threads, copier lanes, host pool)
    t0 = time.perf_counter()
    run(steps)
    rig.drain()                                   # compute streams and, in host mode, the last downloads
    barrier(world)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rig.last_host_cpu_s = time.process_time() - c0
    return sharding.max_over_ranks(dt)


def host_leg(rig, world, steps):
    """Host-buffer variant: the reference's own timed region brackets upload ... download (histretch.cpp:165,174-175,
    212-213,257-261).  Every step copies its frames from page-locked host memory to HBM and the processed frames back
    inside the timed region (the rank's copier: one upload and one download lane, batch k+1 arrives and batch k leaves
    under the kernels).  Runs on every rank; the time is the max over ranks."""
    from uwimageproc_amd import sharding
    rig.host_prepare()
    dt_h = timed(rig, world, steps, 1, host=True)
    same = all(np.array_equal(rig.bufs[i][1], rig.pipes[i].work.cpu().numpy()) for i in range(rig.S))
    same = sharding.max_over_ranks(0.0 if same else 1.0) == 0.0
    F = rig.F
    return {"value": world * F * steps / dt_h, "unit": "frames/s", "ms_per_step": dt_h / steps * 1e3,
            "gbytes_per_s_each_way_per_gpu": F * rig.H * rig.W * 3 * steps / dt_h / 1e9, "downloaded_equals_device": bool(same),
            "ranks": world,
            "note": "the same steps on every rank with page-locked host -> HBM and HBM -> page-locked host copies of every frame "
                    "inside the timed region (uwip_copier: one upload and one download lane per rank, requests served in order "
                    "at the full link rate, hand-overs waited for on the host: no device-side cross-stream barrier)"}


def fourk_leg(args, dev_index, dev, rank, world):
    """BASELINE configs 3 / 5 inside the default line: the same pipe on 3840x2160 frames (128 per GPU and step), 6 steps
    HBM-resident and 6 steps through host buffers, then config 5's paced 4K@60 stream (a short one: 2 s) on every rank."""
    from uwimageproc_amd import sharding
    H, W, F, S = 2160, 3840, 128, max(1, args.streams)
    rig = Rig(dev_index, dev, F, H, W, S, 1234 + 1000 * rank)        # the same scene as --config 4k
    steps = 6
    dt = timed(rig, world, steps, 1, host=False)
    out = {"workload": f"full pipe on {W}x{H} uchar3 frames, {F} per GPU and step", "steps": steps,
           "value": world * F * steps / dt, "unit": "frames/s", "ms_per_step": dt / steps * 1e3}
    if args.host_buffers:
        h = host_leg(rig, world, steps)
        out["value_end_to_end"] = h["value"]
        out["host_buffers"] = h
    rig.close()
    del rig
    torch.cuda.empty_cache()
    import copy
    a2 = copy.copy(args)
    a2.paced_frames = min(args.paced_frames, 120)
    paced = paced_stream(a2, dev_index, dev, H, W)
    paced["worst_latency_ms"] = sharding.max_over_ranks(paced["worst_latency_ms"])
    paced["sustained_fps_min_over_ranks"] = -sharding.max_over_ranks(-paced["sustained_fps"])
    paced["streams"] = f"one 60 fps camera per rank x {world}"
    out["paced_stream"] = paced
    return out


def host_cpus():
    """(CPUs in the affinity mask, cgroup CPU quota or None)"""
    vis = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = float(q) / float(per)
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    return vis, quota


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    ndev = torch.cuda.device_count()                         # a count only: no context is created by it
    # one process per GPU; with fewer devices than ranks (or UWIP_BENCH_BACKEND=gloo) several ranks share a GPU
    backend = os.environ.get("UWIP_BENCH_BACKEND", "nccl" if ndev >= local_world else "gloo")
    dev_index = local_rank if backend == "nccl" else local_rank % max(ndev, 1)
    # placement first: before the first GPU call and before any thread of this rank exists, restrict the process to the
    # CPUs next to its GPU (the sub-batch threads, the copier lanes, the host pool and the first-touched pinned
    # buffers all follow); the CPU baseline below widens the mask again for its own threads
    all_cpus = sorted(os.sched_getaffinity(0))
    placement = {"pinned": False, "error": "--no-pin"}
    if args.pin:
        from uwimageproc_amd import affinity
        placement = affinity.pin_rank_to_gpu(dev_index, ranks_on_node=min(local_world, max(ndev, 1)), local_rank=dev_index)
    assert torch.cuda.is_available(), "bench.py needs a HIP device (there is no CPU fallback)"
    dev = torch.device("cuda", dev_index)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from uwimageproc_amd import sharding
    F, H, W = args.frames, args.rows, args.cols
    S = max(1, args.streams)
    rig = Rig(dev_index, dev, F, H, W, S, 1234 + 1000 * rank)        # a different scene per rank, same size
    pipe = rig.pipes[0]

    dt = timed(rig, world, args.steps, args.warmup, host=False)
    host_cpu_s = sharding.max_over_ranks(rig.last_host_cpu_s)
    if args.dump_outputs and rank == 0:
        dump_outputs(rig, args.dump_outputs)
    # everything below the headline is --full's.  What was timed is also checked: the S sub-batches hold the same frames,
    # so every pipe must hold the same result
    same_out = (sharding.max_over_ranks(0.0 if outputs_identical(rig) else 1.0) == 0.0) if args.full else None
    spot = spot_capture(rig, dev_index) if (args.full and rank == 0 and not args.no_cpu_baseline) else None

    host = host_leg(rig, world, args.steps) if (args.full and args.host_buffers) else None
    if host is not None:
        host["host_cpu_s_per_step"] = sharding.max_over_ranks(rig.last_host_cpu_s) / args.steps

    # per-kernel timing pass (HIP events on the launch stream, inside libuwip)
    roof = None
    kernels = {}
    stages = pipe.stages()
    if args.full and rank == 0:
        roof, kernels = roofline_report(args, pipe, rig.parts[0], dev, F, rig.Fs, H, W)
    barrier(world)
    # the same timed region on further scenes (every rank; rank r's scenes differ from rank 0's as its headline scene does)
    scenes = None
    if args.full and args.scenes > 1:
        sc_steps = max(1, min(args.steps, 5))
        scenes = [{"seed0": rig.seed0, "frames_per_s": world * F * args.steps / dt, "ms_per_step": dt / args.steps * 1e3, "steps": args.steps,
                   "sweep_ms_per_subbatch": (kernels.get("k_clahe_sweep") or {}).get("ms_per_subbatch"), "is": "the headline scene (`value`)"}]
        for j in range(1, args.scenes):
            rig.load_scene(1234 + 1000 * rank + 77777 * j)
            dt_j = timed(rig, world, sc_steps, 1, host=False)
            same_out = same_out and sharding.max_over_ranks(0.0 if outputs_identical(rig) else 1.0) == 0.0
            scenes.append({"seed0": rig.seed0, "frames_per_s": world * F * sc_steps / dt_j, "ms_per_step": dt_j / sc_steps * 1e3,
                           "steps": sc_steps, "sweep_ms_per_subbatch": rig.kernel_ms("k_clahe_sweep")})
        barrier(world)

    rig.close()
    del rig, pipe
    torch.cuda.empty_cache()
    paced = None
    if args.config == "4k-paced":
        paced = paced_stream(args, dev_index, dev, H, W)
    fourk = None
    if args.full and args.config == "1080p" and args.fourk and (H, W) == (1080, 1920):
        try:
            fourk = fourk_leg(args, dev_index, dev, rank, world)
        except Exception as ex:                               # a side measurement never loses the line (all ranks take part)
            fourk = {"error": f"{type(ex).__name__}: {str(ex)[:200]}"}
    barrier(world)
    failed = False
    if rank == 0:
        cpu = None
        if args.full and not args.no_cpu_baseline:
            os.sched_setaffinity(0, all_cpus)                 # the CPU baseline may use every core the job was given
            cpu = cpu_baseline(H, W, spot)
        total_frames = world * F * args.steps
        line = {
            "metric": "frames/sec whole-node, 1080p full pipe (dehaze+stretch+CLAHE+overlap)" if (H, W) == (1080, 1920)
                      else f"frames/sec whole-node, {W}x{H} full pipe (dehaze+stretch+CLAHE+overlap)",
            "value": total_frames / dt,
            "value_end_to_end": None if host is None else host["value"],
            "unit": "frames/s",
            "n_gpus": world,
            "ranks_share_gpu": bool(world > max(ndev, 1)),
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "full": bool(args.full),
            "host_cpu_s_per_step": host_cpu_s / args.steps,
            "outputs_identical_across_streams": None if same_out is None else bool(same_out),
            "spot_check_vs_oracle": None if cpu is None else cpu.get("spot_check_vs_oracle"),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8 (histretch/CLAHE), f64 (dehaze), f32+i8 (overlap)",
            "data": "synthetic",
            "config": {"name": args.config,
                       "workload": f"full pipe bgdehaze->histretch->aclahe->videostrip-overlap on {W}x{H} uchar3 frames",
                       "frames_per_gpu_per_step": F, "streams_per_gpu": S, "stages": stages,
                       "rules": {"overlap": "reference default: any homography from >= 4 good matches (videostrip.cpp:252-272)",
                                 "detector_threshold": "reference-like default: fixed (SURF::create(400) is fixed, videostrip.cpp:206; the contrast-relative one is the opt-in)",
                                 "dehaze_S": ("OPT-IN DEVIATION UWIP_DEHAZE_GUARD_S: S = 1 where BGDehaze.py:83 divides 0 by 0 (as written the frame turns black, "
                                              "a trivial workload)") if GUARD_S else "reference default: unguarded (BGDehaze.py:83)",
                                 "entry": "uwip_pipe_step / uwip_pipe_step_host (C ABI: the chain, carry and throttle are the library's)"},
                       "host_threads_submitting": 1 if os.environ.get("UWIP_BENCH_ONE_SUBMITTER", "1") == "1" else S,
                       "parallelism": f"frame-batch x{world}", "rank0_placement": placement},
            "check_note": "outputs_identical_across_streams: the sub-batch pipes of a rank hold the same frames, so after the timed "
                          "steps all must hold byte-identical enhanced frames, ACLAHE parameters and overlap ratios (every rank); "
                          "spot_check_vs_oracle: one frame of sub-batch 0 of the timed run against the CPU oracle chain (rank 0, inside "
                          "the cpu_baseline leg); host_cpu_s_per_step: process CPU seconds of all threads of a rank over the timed region "
                          "/ steps, max over ranks; the exit code is non-zero when a check fails",
            "value_note": "value: frames resident in HBM when the timed region starts (the contract's definition); "
                          "value_end_to_end: every frame uploaded from and downloaded to page-locked host memory inside the "
                          "timed region (the reference's own timed region, histretch.cpp:165-216), same steps, max over ranks",
            "scenes": None if scenes is None else {
                "per_scene": scenes,
                "frames_per_s_min_median_max": [float(np.min([s["frames_per_s"] for s in scenes])), float(np.median([s["frames_per_s"] for s in scenes])),
                                                float(np.max([s["frames_per_s"] for s in scenes]))],
                "sweep_ms_min_max": [min(s["sweep_ms_per_subbatch"] or 0.0 for s in scenes), max(s["sweep_ms_per_subbatch"] or 0.0 for s in scenes)],
                "note": "the timed region repeated on other synthetic scenes of the same size (seed0 differs); the headline `value` is scene 0"},
            "roofline": roof,
            "cpu_baseline": cpu,
            "host_buffers": host,
            "paced_stream": paced,
            "config_4k": fourk,
            "kernels": kernels,
        }
        print(json.dumps(line))
        spot_res = line["spot_check_vs_oracle"]
        if spot_res is not None and not spot_res.get("ok", False):
            failed = True
    if same_out is False or (host is not None and not host["downloaded_equals_device"]):
        failed = True
    if world > 1:
        import torch.distributed as dist
        sys.stdout.flush()
        dist.barrier()                      # rank 0 may still have been busy with the CPU baseline
        dist.destroy_process_group()
    if failed:
        sys.stderr.write("bench.py: a self-check failed (outputs_identical_across_streams / spot_check_vs_oracle / downloaded_equals_device)\n")
        sys.exit(3)


if __name__ == "__main__":
    main()
