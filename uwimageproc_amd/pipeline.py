"""The per-frame pipe  bgdehaze -> histretch -> aclahe -> videostrip-overlap  on a
batch of frames resident in HBM.  The chain itself -- stage order, the feature-slot
carry between batches, the two-steps-in-flight throttle, the double-buffered host
front end -- lives behind the C ABI (``uwip_pipe_*``, csrc/pipe.cpp; include/uwip.h
"the whole per-frame chain"); this class is its ctypes caller and owns nothing but the
torch tensors it hands in.

Stage definitions (DESIGN.md "the pipe"):
  bgdehaze   main.py:14-20 / adaptiveExp_map (w = 15); as written by default (a 0/0 in S blackens the frame, B-11),
             guard_s=True substitutes S = 1 there (UWIP_DEHAZE_GUARD_S: what bench.py asks for, and says so)
  histretch  -c=RGB, percentiles 2/98 (histretch.cpp:154,217-254)
  aclahe     V of HSV (aclahe.cpp:152-154) -> ParametrosACLAHE (ACLAHE.py:9-129: 3x3 Gaussian prefilter :15,
             sweep = aclahe.cpp:160-193, parameter choice :66-129) -> CLAHE(CL,(BS,BS)) on the unfiltered V
             (python/main.py:19-20) -> back to BGR (aclahe.cpp:216)
  overlap    calcOverlap of every frame against its predecessor (videostrip.cpp:192-289),
             the last frame's features carried into the next batch; or, with ``keyframes=``, videostrip's key-frame
             selector (main.cpp:284-394) decided on the device over the stream of enhanced frames (``keyframe_rows``)
"""
from __future__ import annotations

import ctypes as C

import torch

from ._native import (KF_BLUR_FN, KF_OVERLAP_FN, Context, Copier, KeyframeConfig, KeyframeRow, PipeConfig, PipeStreamsConfig,
                      StreamOut, UwipError, batch_of, lib)

DEHAZE_FULL, DEHAZE_GUARD_S = 1, 2              # uwip.h
OVERLAP_MIN6 = 8
ACLAHE_PREFILTER, ACLAHE_ASYNC = 1, 4
PIPE_DEHAZE, PIPE_HISTRETCH, PIPE_ACLAHE, PIPE_OVERLAP, PIPE_ALL = 1, 2, 4, 8, 15
STREAM_JPEG, STREAM_PNG = 0, 1
EMIT_ALL, EMIT_KEYFRAMES = 0, 1


def keyframe_config(minOverlap=None, kWindow=None, lookback=None, max_rows=None) -> KeyframeConfig:
    """``uwip_keyframe_config``: the library's defaults (0.4, 11: videostrip.hpp:50-51) with the given fields replaced."""
    kc = KeyframeConfig()
    lib().uwip_keyframe_config_default(C.byref(kc))
    for name, v in (("minOverlap", minOverlap), ("kWindow", kWindow), ("lookback", lookback), ("max_rows", max_rows)):
        if v is not None:
            setattr(kc, name, v)
    return kc


def _row(r: KeyframeRow):
    return (r.id, r.frame, r.index, r.overlap, r.blur)


def keyframe_chain_host(overlap, blur, n_frames: int, batch: int, **kf):
    """The pipe's key-frame chain (csrc/kf_chain.hpp) with its batch / round scheme, on the host: overlap(key, frame) and
    blur(frame) give the values the device would compute.  Returns (rows [(id, frame, index, overlap, blur)], fallback
    rounds per batch).  uwip_keyframe_chain_host; needs no device."""
    kc = keyframe_config(**kf)
    ov_cb = KF_OVERLAP_FN(lambda _u, k, f: float(overlap(k, f)))
    bl_cb = KF_BLUR_FN(lambda _u, f: float(blur(f)))
    cap = n_frames + 1
    rows = (KeyframeRow * cap)()
    n = C.c_int(0)
    nb = max(1, -(-n_frames // batch))
    rounds = (C.c_int32 * nb)()
    rc = lib().uwip_keyframe_chain_host(C.byref(kc), int(n_frames), int(batch), ov_cb, bl_cb, None, rows, cap, C.byref(n), rounds)
    if rc:
        raise UwipError(rc, "uwip_keyframe_chain_host")
    return [_row(rows[i]) for i in range(n.value)], list(rounds)[:-(-n_frames // batch)]


class _DevView:
    """Raw device memory described through ``__cuda_array_interface__`` so that torch can wrap it without a copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


class FramePipe:
    """``uwip_pipe`` with the library's defaults = the reference's rules; the two deviations are opt-in: ``guard_s``
    (UWIP_DEHAZE_GUARD_S) and ``min6`` (UWIP_OVERLAP_MIN6).  ``keyframes`` = dict(minOverlap=, kWindow=, lookback=,
    max_rows=) (any subset; {} = the reference's 0.4 / 11) switches the overlap stage to videostrip's key-frame selector
    (uwip_pipe_keyframe_chain): ``keyframe_rows()`` returns the rows, ``end_of_stream(valid)`` marks the last batch.  In
    key-frame mode the host-buffer form (``run_host``) must be the pipe's first step: its staging area is made with a new
    C pipe, which keeps the key-frame configuration and a pending end-of-stream mark but not a chain already under way."""

    def __init__(self, device: int, frames: int, rows: int, cols: int, letters: str = "RGB", w: int = 15,
                 video_size=None, seed: int = 1, copier: "Copier | None" = None, guard_s: bool = False, min6: bool = False,
                 keyframes: "dict | None" = None):
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        # share torch's current stream so torch events / synchronize cover our kernels
        self.stream = torch.cuda.current_stream(self.dev)
        self.ctx = Context(device, stream=self.stream.cuda_stream)
        self._l = self.ctx._l
        self.copier = copier
        self._host_bufs = []
        self.F, self.H, self.W = frames, rows, cols
        self.seed = seed
        # the reference's globals videoWidth / videoHeight (main.cpp:238-239); as written they are the
        # full-resolution size
        self.vw, self.vh = video_size if video_size else (cols, rows)
        cfg = PipeConfig()
        self._l.uwip_pipe_config_default(C.byref(cfg), frames, rows, cols)
        cfg.letters = letters.encode()
        cfg.w = w
        cfg.dehaze_flags = DEHAZE_FULL | (DEHAZE_GUARD_S if guard_s else 0)
        cfg.match_flags = OVERLAP_MIN6 if min6 else 0
        cfg.videoWidth, cfg.videoHeight = self.vw, self.vh
        cfg.seed = seed
        # the staging area of the host-buffer form is torch's, so that the results can be looked at as tensors
        self._staging = None
        self._cfg = cfg
        self._p = None
        self.work = torch.empty((frames, rows, cols, 3), dtype=torch.uint8, device=self.dev)
        self.ratio = torch.empty((frames,), dtype=torch.float32, device=self.dev)
        self.info = torch.zeros((frames, 8), dtype=torch.int32, device=self.dev)
        self._own = (self.work, self.ratio, self.info)
        self.h_bs = (C.c_int32 * frames)()
        self.h_cl = (C.c_int32 * frames)()
        self._params = None
        self._k = 0
        self._kc = keyframe_config(**keyframes) if keyframes is not None else None
        self._eos = None             # a pending uwip_pipe_end_of_stream mark (the C pipe holds it too)
        self._chain_used = False     # an overlap stage has run in key-frame mode: the C pipe holds chain state and rows
        self._create()

    def _create(self):
        h = C.c_void_p()
        self.ctx.call("uwip_pipe_create", C.byref(self._cfg), self.copier._h if self.copier is not None else None, C.byref(h))
        self._p = h
        if self._kc is not None:
            self._call("uwip_pipe_keyframe_chain", C.byref(self._kc))
        if self._eos is not None:
            self._call("uwip_pipe_end_of_stream", self._eos)

    def _overlap_ran(self):
        # the step that ran the overlap stage consumed the end-of-stream mark
        self._eos = None
        self._chain_used = self._chain_used or self._kc is not None

    # ---- key-frame mode (uwip_pipe_keyframe_chain) ----------------------------------------------------------
    def end_of_stream(self, valid: int):
        """The next step is the stream's last and only its first `valid` frames are real (uwip_pipe_end_of_stream)."""
        self._call("uwip_pipe_end_of_stream", int(valid))
        self._eos = int(valid)

    def keyframe_rows(self):
        """Rows [(id, frame, index, overlap, blur)] closed since the last call (waits for the stream)."""
        out = []
        cap = 256
        buf = (KeyframeRow * cap)()
        while True:
            n = C.c_int(0)
            self._call("uwip_pipe_keyframes", buf, cap, C.byref(n))
            out += [_row(buf[i]) for i in range(n.value)]
            if n.value < cap:
                return out

    # ---- compressed frames in, compressed (key) frames out (uwip_pipe_streams) -------------------------------
    def streams(self, format: str = "jpeg", quality: int = 95, png_filter: int = -1, emit: str = "all", slot_bytes: int = 0,
                depth: int = 2):
        """Configure ``run_streams`` / ``collect``: the format of the emitted streams ("jpeg" / "png"), which frames are
        emitted ("all", or "keyframes" on a pipe made with ``keyframes=``), the slot per emitted frame (0 = the raw frame
        size) and how many steps' results stay collectable.  Before the first step or right after a reset."""
        sc = PipeStreamsConfig()
        self._l.uwip_pipe_streams_config_default(C.byref(sc))
        sc.format = {"jpeg": STREAM_JPEG, "png": STREAM_PNG}[format]
        sc.emit = {"all": EMIT_ALL, "keyframes": EMIT_KEYFRAMES}[emit]
        sc.quality, sc.png_filter, sc.slot_bytes, sc.depth = int(quality), int(png_filter), int(slot_bytes), int(depth)
        self._call("uwip_pipe_streams", C.byref(sc))
        self._slot_bytes = int(slot_bytes) if slot_bytes else self.H * self.W * 3

    def run_streams(self, streams) -> int:
        """One step on `frames` compressed frames (bytes objects, .jpg and .png mixed as they come): returns the ticket of
        the step's result without waiting for the device (uwip_pipe_step_streams)."""
        n = len(streams)
        bufs = [(C.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if len(b) else b"\0") for b in streams]
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        sizes = (C.c_size_t * n)(*[len(b) for b in streams])
        t = C.c_uint64(0)
        self._call("uwip_pipe_step_streams", ptrs, sizes, n, C.byref(t))
        self._overlap_ran()
        self._params = None
        return t.value

    def result_params(self, ticket: int):
        """[(BS, CL)] the aclahe stage chose in the step `ticket` names; waits for that step only, and must come before its
        ``collect`` (uwip_pipe_result_params)."""
        bs, cl = (C.c_int32 * self.F)(), (C.c_int32 * self.F)()
        self._call("uwip_pipe_result_params", C.c_uint64(ticket), bs, cl)
        return list(zip(bs, cl))

    def collect(self, ticket: int, blob_cap: "int | None" = None):
        """Wait for the step `ticket` names and return (status [frames], ratio [frames], [(index, row_id, bytes | -needed)]):
        the decoders' statuses, the step's ratios and the emitted streams (uwip_pipe_collect)."""
        import numpy as np

        F = self.F
        status = (C.c_int32 * F)()
        ratio = (C.c_float * F)()
        outs = (StreamOut * (F + 1))()
        n = C.c_int(0)
        need = C.c_size_t(0)
        args = (self._p, C.c_uint64(ticket), status, ratio, outs, F + 1, C.byref(n))
        blob, cap = None, 0
        if blob_cap is None:
            # ask for the size first: a call whose blob is too small fails, says how many bytes there are and keeps the result
            rc = self._l.uwip_pipe_collect(*args, None, 0, C.byref(need))
            if rc == 0:
                return np.array(status, dtype=np.int32), np.array(ratio, dtype=np.float32), \
                    [(outs[i].index, outs[i].row_id, b"" if outs[i].size >= 0 else int(outs[i].size)) for i in range(n.value)]
            cap = need.value
            if cap == 0:
                raise UwipError(rc, self._l.uwip_pipe_last_error(self._p).decode("utf-8", "replace"))
        else:
            cap = int(blob_cap)
        blob = (C.c_uint8 * max(1, cap))()
        self._call("uwip_pipe_collect", *args[1:], blob, cap, C.byref(need))
        raw = bytes(memoryview(blob)[:need.value])
        res = []
        for i in range(n.value):
            o = outs[i]
            res.append((o.index, o.row_id, raw[o.offset:o.offset + o.size] if o.size >= 0 else int(o.size)))
        return np.array(status, dtype=np.int32), np.array(ratio, dtype=np.float32), res

    def _call(self, name, *args):
        rc = getattr(self._l, name)(self._p, *args)
        if rc:
            raise UwipError(rc, self._l.uwip_pipe_last_error(self._p).decode("utf-8", "replace"))

    def close(self):
        if getattr(self, "_p", None):
            self._l.uwip_pipe_destroy(self._p)
            self._p = None
        for a in getattr(self, "_host_bufs", []):
            if a.ctypes.data in getattr(self.ctx, "_pinned", {}):
                self.ctx.host_free(a)
        self._host_bufs = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stages (uwip_pipe_stages: the chain tapped between its stages) ------------------------------
    def _stages(self, mask, src=None):
        sb = batch_of(src) if src is not None else None
        wb = batch_of(self.work)
        self._call("uwip_pipe_stages", mask, C.byref(sb) if sb is not None else None, C.byref(wb),
                   C.c_void_p(self.ratio.data_ptr()), C.c_void_p(self.info.data_ptr()))
        if mask & PIPE_OVERLAP:
            self._overlap_ran()
        if mask & PIPE_ACLAHE:
            self._params = None

    def stage_dehaze(self, src: torch.Tensor):
        self._stages(PIPE_DEHAZE, src)

    def stage_histretch(self):
        self._stages(PIPE_HISTRETCH)

    def stage_dehaze_histretch(self, src: torch.Tensor):
        """The two stages as one chained call: the dehaze writer hands the stretch its histogram."""
        self._stages(PIPE_DEHAZE | PIPE_HISTRETCH, src)

    def stage_aclahe(self):
        self._stages(PIPE_ACLAHE)

    def stage_overlap(self):
        self._stages(PIPE_OVERLAP)

    @property
    def params(self):
        """[(BS, CL)] of the most recent aclahe stage (waits for the stream the first time it is read after a stage)"""
        if self._params is None:
            self._call("uwip_pipe_last_params", self.h_bs, self.h_cl)
            self._params = list(zip(self.h_bs, self.h_cl))
        return self._params

    @property
    def have_prev(self):
        raise AttributeError("write-only: assign False to forget the carried key frame")

    @have_prev.setter
    def have_prev(self, value):
        assert not value
        self._call("uwip_pipe_reset")
        self._eos = None

    @property
    def v(self):
        """The V planes the aclahe stage left in the pipe ([F, H, W] uint8, device): a view, valid until the next step."""
        p = C.c_void_p()
        self._call("uwip_pipe_device_results", C.byref(p), None, None, None)
        try:
            return torch.as_tensor(_DevView(p.value, (self.F, self.H, self.W), "|u1"), device=self.dev)
        except Exception:
            import numpy as np                       # a torch without __cuda_array_interface__: through the host
            h = np.empty((self.F, self.H, self.W), np.uint8)
            self.ctx.call("uwip_memcpy_d2h", C.c_void_p(h.ctypes.data), p, h.nbytes)
            return torch.from_numpy(h).to(self.dev)

    def stages(self):
        return ["bgdehaze(adaptiveExp_map,w=15)", "histretch(RGB,2/98)", "aclahe(V:blur3+sweep+select+CLAHE,HSV->BGR)",
                "videostrip-overlap(frame vs predecessor: detect+describe+MFMA match+RANSAC+overlapArea)"]

    # ---- host-buffer front end (GpuMat::upload ... download, histretch.cpp:174-175,212-213) ------------
    def host_buffers(self):
        """Page-locked input / output frame buffers [F,H,W,3] owned by the library (freed by ``close``)."""
        shape = (self.F, self.H, self.W, 3)
        a, b = self.ctx.host_alloc(shape), self.ctx.host_alloc(shape)
        self._host_bufs += [a, b]
        return a, b

    def _host_state(self):
        if self._staging is None:
            # uwip_pipe_config.d_staging must be known at creation: the pipe is made anew (nothing has been carried yet;
            # _create applies the key-frame configuration and a pending end-of-stream mark again)
            assert self._k == 0
            if self._chain_used:
                raise UwipError(1, "key-frame mode: the host-buffer form must be the pipe's first step (the pipe is re-made "
                                   "for it, which would drop the chain and its unread rows)")
            n = self._l.uwip_pipe_staging_bytes(C.byref(self._cfg))
            self._staging = torch.empty((n,), dtype=torch.uint8, device=self.dev)
            self._cfg.d_staging = self._staging.data_ptr()
            self._l.uwip_pipe_destroy(self._p)
            self._create()
            fb = self.F * self.H * self.W * 3
            al = lambda x: (x + 255) & ~255
            st = self._staging
            self._h_work = [st[(2 + s) * fb:(3 + s) * fb].view(self.F, self.H, self.W, 3) for s in range(2)]
            r0 = al(4 * fb)
            self._h_ratio = [st[r0 + 4 * self.F * s:r0 + 4 * self.F * (s + 1)].view(torch.float32) for s in range(2)]
            i0 = r0 + al(8 * self.F)
            self._h_info = [st[i0 + 32 * self.F * s:i0 + 32 * self.F * (s + 1)].view(torch.int32).view(self.F, 8) for s in range(2)]

    def run_host(self, h_in, h_out, prefetch=None, h_ratio=None):
        """upload -> the four stages -> download; `h_in` / `h_out` come from ``host_buffers``.  With ``prefetch`` (the
        NEXT batch's input buffer) that batch's upload is requested now and runs under this batch's kernels, so a stream
        of batches never waits for the link.  Returns (upload ticket, download ticket) without waiting for the device:
        ``wait_ticket(t)`` blocks until that copy is complete -- `h_in` may be refilled after the first, `h_out` read
        after the second -- and ``sync()`` drains everything.  (uwip_pipe_step_host.)"""
        self._host_state()
        t = (C.c_uint64 * 3)()
        self._call("uwip_pipe_step_host", C.c_void_p(h_in.ctypes.data), C.c_void_p(h_out.ctypes.data),
                   C.c_void_p(h_ratio.ctypes.data) if h_ratio is not None else None,
                   C.c_void_p(prefetch.ctypes.data) if prefetch is not None else None, t)
        self._overlap_ran()
        slot = self._k % 2
        self.work, self.ratio, self.info = self._h_work[slot], self._h_ratio[slot], self._h_info[slot]
        self._k += 1
        self._params = None
        return t[0], t[1]

    def wait_ticket(self, ticket):
        self._call("uwip_pipe_wait", C.c_uint64(ticket))

    def sync(self):
        """Drain the pipe's stream and, when the host-buffer front end is in use, its outstanding copies."""
        self._call("uwip_pipe_sync")

    def run(self, src: torch.Tensor):
        """One step on frames resident in HBM (uwip_pipe_step: queued without a host wait, at most two steps in flight)."""
        self.work, self.ratio, self.info = self._own
        sb, wb = batch_of(src), batch_of(self.work)
        self._call("uwip_pipe_step", C.byref(sb), C.byref(wb), C.c_void_p(self.ratio.data_ptr()), C.c_void_p(self.info.data_ptr()))
        self._overlap_ran()
        self._params = None
        return self.work, self.ratio
