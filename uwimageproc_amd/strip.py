"""The strip mosaic over the C ABI (include/uwip.h, "strip mosaic"): the key frames main.cpp:368-381 writes, chained by the
homographies of videostrip.cpp:270 and rendered into one canvas per segment.  No compute here: ``Strip`` owns a
``uwip_strip`` and hands torch tensors to it."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional

import numpy as np

from ._native import UWIP_OK, Context, StripBandsConfig, StripConfig, StripGainConfig, StripSeamConfig, StripSegment, UwipError, batch_of

MODES = {"feather": 0, "first": 1, "last": 2, "multiband": 3, "seam": 4}      # UWIP_STRIP_FEATHER / FIRST / LAST / MULTIBAND / SEAM
GAIN = 0x100                                           # UWIP_STRIP_GAIN


class Segment(NamedTuple):
    """uwip_strip_segment: frames first..first + count - 1 on a rows x cols canvas whose pixel (0, 0) is the plane point
    (x0, y0) of the segment's first frame."""
    first: int
    count: int
    x0: int
    y0: int
    rows: int
    cols: int


class Strip:
    """``Strip(ctx, rows, cols, batch=..., max_frames=...)``: frames of rows x cols BGR, at most ``batch`` per ``add`` and
    ``max_frames`` in all.  Further keywords are fields of uwip_strip_config (max_canvas_rows, max_canvas_cols, max_scale,
    detect_flags, match_flags, seed, videoWidth, videoHeight)."""

    def __init__(self, ctx: Context, rows: int, cols: int, batch: int = 16, max_frames: int = 1024, **fields):
        self.ctx, self._l = ctx, ctx._l
        cfg = StripConfig()
        ctx.check(self._l.uwip_strip_config_default(C.byref(cfg), int(rows), int(cols)))
        cfg.batch, cfg.max_frames = int(batch), int(max_frames)
        for k, v in fields.items():
            if k not in dict(StripConfig._fields_):
                raise TypeError(f"unknown uwip_strip_config field {k!r}")
            setattr(cfg, k, v)
        self.cfg = cfg
        h = C.c_void_p()
        ctx.call("uwip_strip_create", C.byref(cfg), C.byref(h))
        self._h = h
        self.segments: List[Segment] = []
        self._injected = False             # the form of the strip: set by its first add

    def close(self):
        if getattr(self, "_h", None):
            # a strip is bound to its context (uwip.h: destroy it before the context).  When the context has been closed
            # first, its handle must not be touched any more: the strip is dropped, not destroyed into freed memory
            if getattr(self.ctx, "_h", None):
                self._l.uwip_strip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != UWIP_OK:
            raise UwipError(rc, self._l.uwip_strip_last_error(self._h).decode("utf-8", "replace"))

    def __len__(self) -> int:
        n = C.c_int(0)
        self._check(self._l.uwip_strip_count(self._h, C.byref(n)))
        return n.value

    def reset(self):
        self._check(self._l.uwip_strip_reset(self._h))
        self.segments = []

    def add(self, frames: "torch.Tensor", H: "Optional[torch.Tensor]" = None, ratio: "Optional[torch.Tensor]" = None):
        """frames: uint8 device tensor [n, rows, cols, 3] (any row / frame stride).  With H ([n, 9] or [n, 3, 3] float64) and
        ratio ([n] float32) on the device nothing is detected or matched: those are appended and the frames are stored as
        they are."""
        import torch

        b = batch_of(frames)
        if (H is None) != (ratio is None):
            raise ValueError("inject both H and ratio, or neither")
        if H is not None:
            assert H.is_cuda and H.dtype == torch.float64 and H.is_contiguous() and H.numel() == 9 * b.frames
            assert ratio.is_cuda and ratio.dtype == torch.float32 and ratio.is_contiguous() and ratio.numel() == b.frames
        torch.cuda.current_stream(frames.device).synchronize()
        self._check(self._l.uwip_strip_add(self._h, C.byref(b), C.c_void_p(H.data_ptr()) if H is not None else None,
                                           C.c_void_p(ratio.data_ptr()) if H is not None else None))
        self.ctx.sync()          # the caller's tensors may go once this returns
        self._injected = H is not None
        self.segments = []

    def layout(self) -> List[Segment]:
        segs, buf, n = [], (StripSegment * 64)(), C.c_int(0)
        while True:
            self._check(self._l.uwip_strip_layout(self._h, buf, 64, C.byref(n)))
            segs += [Segment(s.first, s.count, s.x0, s.y0, s.rows, s.cols) for s in buf[:n.value]]
            if n.value < 64:
                break
        self.segments = segs
        return segs

    def transforms(self):
        """After ``layout``: dict of G, Ginv [n, 9] float64, seg [n] int32, box [n, 4] int32 (numpy)."""
        n = len(self)
        G, Gi = np.zeros((n, 9)), np.zeros((n, 9))
        seg, box = np.zeros(n, np.int32), np.zeros((n, 4), np.int32)
        self._check(self._l.uwip_strip_transforms(self._h, G.ctypes.data, Gi.ctypes.data, seg.ctypes.data, box.ctypes.data))
        return {"G": G, "Ginv": Gi, "seg": seg, "box": box}

    def gains(self, **cfg):
        """After ``layout``: measure the overlaps of consecutive frames and solve one gain per frame and channel
        (uwip_strip_gains).  Keywords are fields of uwip_strip_gain_config (sigma_n, sigma_g, lo, hi, min_pixels) over its
        defaults.  An ``add``, a ``reset`` or a new layout drops the gains."""
        c = StripGainConfig()
        self._check(self._l.uwip_strip_gain_config_default(C.byref(c)))
        for k, v in cfg.items():
            if k not in ("sigma_n", "sigma_g", "lo", "hi", "min_pixels"):
                raise TypeError(f"unknown uwip_strip_gain_config field {k!r}")
            setattr(c, k, v)
        self._check(self._l.uwip_strip_gains(self._h, C.byref(c)))
        self.ctx.sync()

    def gain_values(self):
        """After ``gains`` or ``set_gains``: dict of gq [n, 3] int32 (gains in 1/4096), g [n, 3] float64, stats [n, 7] uint64
        (N, Sa[3], Sb[3] of each frame's pair with the frame before it) (numpy)."""
        n = len(self)
        gq, g, st = np.zeros((n, 3), np.int32), np.zeros((n, 3)), np.zeros((n, 7), np.uint64)
        self._check(self._l.uwip_strip_gain_values(self._h, gq.ctypes.data, g.ctypes.data, st.ctypes.data))
        return {"gq": gq, "g": g, "stats": st}

    def set_gains(self, gq):
        """After ``layout``: inject gains [n, 3] in 1/4096, each 1024..16384, instead of computing them."""
        gq = np.ascontiguousarray(gq, np.int32)
        if gq.shape != (len(self), 3):
            raise ValueError("gq: [frames, 3]")
        self._check(self._l.uwip_strip_set_gains(self._h, gq.ctypes.data))

    def bands(self, **cfg):
        """Build the stacks of every frame added so far and keep the ramps for ``render(mode="multiband")``
        (uwip_strip_bands).  Keywords are ``levels`` (1..4) and ``ramp`` (a sequence of ``levels`` values, each 1..4096) over
        the defaults 4 and (1, 2, 4, 8).  An ``add`` or a ``reset`` drops the stacks; a new layout keeps them."""
        c = StripBandsConfig()
        self._check(self._l.uwip_strip_bands_config_default(C.byref(c)))
        for k, v in cfg.items():
            if k == "levels":
                c.levels = int(v)
            elif k == "ramp":
                v = [int(r) for r in v]
                if len(v) > 4:
                    raise ValueError("ramp: at most four values")
                for i, r in enumerate(v):
                    c.ramp[i] = r
            else:
                raise TypeError(f"unknown uwip_strip_bands_config field {k!r}")
        self._check(self._l.uwip_strip_bands(self._h, C.byref(c)))
        self.ctx.sync()

    def band_level(self, frame: int, level: int):
        """After ``bands``: level 1..levels of a frame's stack, uint8 [rows, cols, 3] of the stored geometry (numpy)."""
        rows, cols = self.stored_size()
        out = np.zeros((rows, cols, 3), np.uint8)
        self._check(self._l.uwip_strip_band_level(self._h, int(frame), int(level), out.ctypes.data))
        return out

    def seams(self, **cfg):
        """After ``layout`` (and after ``gains``, whose gains the costs then use): find the seam of every frame against the
        frame before it, for ``render(mode="seam")`` (uwip_strip_seams).  Keyword: ``prior`` (0..4096) over the default 1024.
        An ``add``, a ``reset``, a new layout, ``gains`` and ``set_gains`` drop the seams."""
        c = StripSeamConfig()
        self._check(self._l.uwip_strip_seam_config_default(C.byref(c)))
        for k, v in cfg.items():
            if k != "prior":
                raise TypeError(f"unknown uwip_strip_seam_config field {k!r}")
            c.prior = int(v)
        self._check(self._l.uwip_strip_seams(self._h, C.byref(c)))
        self.ctx.sync()

    def seam_values(self):
        """After ``seams`` or ``set_seams``: dict of seam [n, max(cols, rows)] int32 of the stored geometry (-1 beyond a
        seam's steps and for a segment's first frame), orient [n] int32 (axis | 2 for sign -1), total [n] uint64 (numpy)."""
        n, (rows, cols) = len(self), self.stored_size()
        seam, ori, total = np.zeros((n, max(rows, cols)), np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)
        self._check(self._l.uwip_strip_seam_values(self._h, seam.ctypes.data, ori.ctypes.data, total.ctypes.data))
        return {"seam": seam, "orient": ori, "total": total}

    def set_seams(self, seam, orient):
        """After ``layout``: inject seams [n, max(cols, rows)] (entries 0..states) and orients [n] (0..3) instead of finding
        them."""
        rows, cols = self.stored_size()
        seam, orient = np.ascontiguousarray(seam, np.int32), np.ascontiguousarray(orient, np.int32)
        if seam.shape != (len(self), max(rows, cols)) or orient.shape != (len(self),):
            raise ValueError("seam: [frames, max(cols, rows)], orient: [frames]")
        self._check(self._l.uwip_strip_set_seams(self._h, seam.ctypes.data, orient.ctypes.data))

    def stored_size(self):
        """(rows, cols) of the frames as the strip keeps them: as given when H and ratio were injected, the working size
        (uwip_overlap_working_size) when they were matched."""
        if self._injected:
            return int(self.cfg.rows), int(self.cfg.cols)
        oh, ow = C.c_int(0), C.c_int(0)
        self.ctx.check(self._l.uwip_overlap_working_size(int(self.cfg.rows), int(self.cfg.cols), C.byref(oh), C.byref(ow)))
        return oh.value, ow.value

    def render(self, segment: int, mode: str = "feather", fill=(0, 0, 0), cover: bool = False, out: "Optional[torch.Tensor]" = None,
               gain: bool = False):
        """One segment of the last ``layout``: a uint8 tensor [rows, cols, 3] (``out``: a tensor of that shape to render
        into, any row stride), and with ``cover`` also the [rows, cols] count of covering frames.  ``gain``: every sample
        times its frame's gain (``gains`` or ``set_gains`` first).  ``mode="multiband"``: ``bands`` first; ``mode="seam"``:
        ``seams`` or ``set_seams`` first."""
        import torch

        if not self.segments:
            self.layout()
        s = self.segments[segment]
        dev = torch.device("cuda", self.ctx.device)
        if out is None:
            out = torch.empty((s.rows, s.cols, 3), dtype=torch.uint8, device=dev)
        if isinstance(cover, torch.Tensor):          # the caller's plane: packed [rows, cols]
            cov = cover
            assert cov.is_cuda and cov.dtype == torch.uint8 and cov.is_contiguous() and tuple(cov.shape) == (s.rows, s.cols)
            cover = True
        else:
            cov = torch.empty((s.rows, s.cols), dtype=torch.uint8, device=dev) if cover else None
        b = batch_of(out)
        f = (C.c_uint8 * 3)(*[int(v) for v in fill])
        torch.cuda.current_stream(dev).synchronize()
        self._check(self._l.uwip_strip_render(self._h, int(segment), MODES[mode] | (GAIN if gain else 0), f, C.byref(b), C.c_void_p(cov.data_ptr()) if cover else None))
        self.ctx.sync()
        return (out, cov) if cover else out
