"""cv2.imwrite(".png") / cv2.imencode(".png") for a batch, on the device (uwip_png_encode, include/uwip.h).

The streams are lossless PNG -- colour type 2 for BGR frames (RGB in the file), 0 for grey ones, adaptive row filters, a
deflate of runs and per-chunk Huffman codes -- whose pixels are the input's; the bytes are neither OpenCV's nor cli/imgio.hpp's.
No compute happens here and there is no CPU path: the frames are a device tensor and the kernels of csrc/png_encode.hip do the
work.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

from ._native import _P, Context, UwipError, UWIP_ERR_INVALID, batch_of, lib


def _need_context(ctx):
    if ctx is None or not isinstance(ctx, Context):
        raise UwipError(UWIP_ERR_INVALID, "a Context is needed (no HIP device? there is no CPU fallback)")


def bound(rows: int, cols: int, channels: int) -> int:
    """Worst-case stream length of one frame (``uwip_png_bound``; host only)."""
    return int(lib().uwip_png_bound(int(rows), int(cols), int(channels)))


def chunk_bytes() -> int:
    """Filtered bytes per independently coded chunk (``uwip_png_chunk_bytes``; host only)."""
    return int(lib().uwip_png_chunk_bytes())


def encode_device(ctx: Context, frames, filter: int = -1, slot_bytes: Optional[int] = None) -> Tuple["object", "object"]:
    """Asynchronous form: returns ``(streams, sizes)`` device tensors, ``streams`` uint8 ``[F, slot_bytes]`` and ``sizes``
    int64 ``[F]`` (the length, or minus the needed length where a stream does not fit its slot).  The work is queued on the
    context's stream; ``ctx.sync()`` before another stream reads the tensors."""
    import torch

    _need_context(ctx)
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
    ctx.call("uwip_png_encode", C.byref(b), int(filter), _P(streams.data_ptr()), int(slot_bytes), _P(sizes.data_ptr()))
    return streams, sizes


def encode(ctx: Context, frames, filter: int = -1) -> List[bytes]:
    """``frames``: torch uint8 device tensor ``[F, H, W, 3]`` (BGR) or ``[F, H, W]`` (grey) -> one PNG stream per frame.
    ``filter``: -1 the adaptive choice per row, 0..4 that type on every row.  The slot is the raw frame size; a batch with a
    frame that outgrows it (noise) is encoded once more with ``bound()`` slots."""
    streams, sizes = encode_device(ctx, frames, filter)
    ctx.sync()
    n = sizes.cpu().tolist()
    if any(s < 0 for s in n):
        H, W = int(frames.shape[1]), int(frames.shape[2])
        streams, sizes = encode_device(ctx, frames, filter, bound(H, W, 3 if frames.dim() == 4 else 1))
        ctx.sync()
        n = sizes.cpu().tolist()
    return [streams[f, : n[f]].cpu().numpy().tobytes() for f in range(len(n))]
