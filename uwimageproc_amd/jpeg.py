"""cv2.imwrite(".jpg") / cv2.imencode(".jpg") for a batch, on the device (uwip_jpeg_encode, include/uwip.h).

The streams are baseline JFIF -- 4:2:0 for BGR frames, one component for grey ones, the Annex K tables scaled by
``quality`` -- and byte for byte what the CLIs' host codec (cli/jpeg.hpp) writes.  No compute happens here and there is no
CPU path: the frames are a device tensor and the kernels of csrc/jpeg_encode.hip do the work.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

from ._native import _P, Context, UwipError, UWIP_ERR_INVALID, batch_of, lib


def bound(rows: int, cols: int, channels: int) -> int:
    """Worst-case stream length of one frame (``uwip_jpeg_bound``; host only)."""
    return int(lib().uwip_jpeg_bound(int(rows), int(cols), int(channels)))


def encode_device(ctx: Context, frames, quality: int = 95, slot_bytes: Optional[int] = None) -> Tuple["object", "object"]:
    """Asynchronous form: returns ``(streams, sizes)`` device tensors, ``streams`` uint8 ``[F, slot_bytes]`` and ``sizes``
    int64 ``[F]`` (the length, or minus the needed length where a stream does not fit its slot).  The work is queued on the
    context's stream; ``ctx.sync()`` before another stream reads the tensors."""
    import torch

    if ctx is None or not isinstance(ctx, Context):
        raise UwipError(UWIP_ERR_INVALID, "a Context is needed (no HIP device? there is no CPU fallback)")
    if not frames.is_cuda:
        raise UwipError(UWIP_ERR_INVALID, "device tensor expected: there is no CPU fallback")
    if frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[-1] not in (1, 3)):
        raise UwipError(UWIP_ERR_INVALID, "frames must be [F, H, W, 3] (BGR) or [F, H, W] (grey): channels must be 1 or 3")
    b = batch_of(frames if frames.dim() != 3 else frames.unsqueeze(-1))
    if slot_bytes is None:
        slot_bytes = b.rows * b.cols * b.channels + 1024
    streams = torch.empty((b.frames, int(slot_bytes)), dtype=torch.uint8, device=frames.device)
    sizes = torch.empty((b.frames,), dtype=torch.int64, device=frames.device)
    # the context has a stream of its own: what torch queued for `frames` (and for the blocks the two new tensors reuse)
    # has to be done before the kernels read and write them
    torch.cuda.current_stream(frames.device).synchronize()
    ctx.call("uwip_jpeg_encode", C.byref(b), int(quality), _P(streams.data_ptr()), int(slot_bytes), _P(sizes.data_ptr()))
    return streams, sizes


def encode(ctx: Context, frames, quality: int = 95) -> List[bytes]:
    """``frames``: torch uint8 device tensor ``[F, H, W, 3]`` (BGR) or ``[F, H, W]`` (grey) -> one JPEG stream per frame.
    The slot is the raw frame size; a batch with a frame that outgrows it is encoded once more with ``bound()`` slots."""
    streams, sizes = encode_device(ctx, frames, quality)
    ctx.sync()
    n = sizes.cpu().tolist()
    if any(s < 0 for s in n):
        H, W = int(frames.shape[1]), int(frames.shape[2])
        streams, sizes = encode_device(ctx, frames, quality, bound(H, W, 3 if frames.dim() == 4 else 1))
        ctx.sync()
        n = sizes.cpu().tolist()
    return [streams[f, : n[f]].cpu().numpy().tobytes() for f in range(len(n))]
