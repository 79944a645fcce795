"""cv2.imwrite(".jpg") / cv2.imencode(".jpg") for a batch, on the device (uwip_jpeg_encode, include/uwip.h).

The streams are baseline JFIF -- 4:2:0 for BGR frames, one component for grey ones, the Annex K tables scaled by
``quality`` -- and byte for byte what the CLIs' host codec (cli/jpeg.hpp) writes.  No compute happens here and there is no
CPU path: the frames are a device tensor and the kernels of csrc/jpeg_encode.hip do the work.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

from ._native import _P, Context, UwipError, UWIP_ERR_INVALID, batch_of, lib


def _need_context(ctx):
    if ctx is None or not isinstance(ctx, Context):
        raise UwipError(UWIP_ERR_INVALID, "a Context is needed (no HIP device? there is no CPU fallback)")


def bound(rows: int, cols: int, channels: int) -> int:
    """Worst-case stream length of one frame (``uwip_jpeg_bound``; host only)."""
    return int(lib().uwip_jpeg_bound(int(rows), int(cols), int(channels)))


def encode_device(ctx: Context, frames, quality: int = 95, slot_bytes: Optional[int] = None) -> Tuple["object", "object"]:
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


# ---- decoding (uwip_jpeg_decode, csrc/jpeg_decode.hip) ---------------------------------------------------------------------
BAD_STREAM, SIZE_MISMATCH, HOST_ONLY = -1, -2, -3


def info(stream: bytes) -> Tuple[int, int, int]:
    """``(rows, cols, components)`` of a baseline JPEG stream (``uwip_jpeg_info``; host only).  Raises ``UwipError`` for a
    stream the host decoder's header parse rejects (progressive, truncated header, not a JPEG ...)."""
    r, c, ch = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    buf = (C.c_uint8 * max(len(stream), 1)).from_buffer_copy(bytes(stream) or b"\0")
    rc = lib().uwip_jpeg_info(C.cast(buf, _P), len(stream), C.byref(r), C.byref(c), C.byref(ch))
    if rc != 0:
        raise UwipError(rc, "not a baseline JPEG stream the decoder reads")
    return r.value, c.value, ch.value


def decode_into(ctx: Context, streams: List[bytes], out, sync_rounds: int = -1, unsettled=None):
    """Decodes ``streams`` into the device tensor ``out`` (``[F, H, W, 3]`` BGR or ``[F, H, W]`` grey, any strides with packed
    pixels); returns the int32 device tensor of per-frame statuses.  Asynchronous on the context's stream."""
    import torch

    from ._native import JpegDecodeOpts

    _need_context(ctx)
    if not out.is_cuda:
        raise UwipError(UWIP_ERR_INVALID, "device tensor expected: there is no CPU fallback")
    n = len(streams)
    b = batch_of(out if out.dim() != 3 else out.unsqueeze(-1))
    bufs = [(C.c_uint8 * max(len(s), 1)).from_buffer_copy(bytes(s) or b"\0") for s in streams]
    ptrs = (_P * max(n, 1))(*[C.cast(x, _P) for x in bufs])
    sizes = (C.c_size_t * max(n, 1))(*[len(s) for s in streams])
    status = torch.empty((n,), dtype=torch.int32, device=out.device)
    opts = JpegDecodeOpts(int(sync_rounds), 0, unsettled.data_ptr() if unsettled is not None else None)
    torch.cuda.current_stream(out.device).synchronize()
    ctx.call("uwip_jpeg_decode", ptrs, sizes, n, C.byref(b), C.byref(opts), _P(status.data_ptr()))
    return status


def decode(ctx: Context, streams: List[bytes], channels: int = 3, sync_rounds: int = -1):
    """``cv2.imdecode`` for a batch of equally sized baseline JPEG streams, on the device: returns ``(frames, status)``,
    ``frames`` a uint8 device tensor ``[F, H, W, 3]`` (BGR; a grey stream replicated) or ``[F, H, W]`` (``channels=1``, grey
    streams only) of the size of the first stream that parses (none does: ``UwipError``; no streams: an empty batch),
    ``status`` a list with 0 or ``BAD_STREAM`` / ``SIZE_MISMATCH`` / ``HOST_ONLY`` per frame (the pixels of such a frame are
    unspecified: decode it on the host)."""
    import torch

    _need_context(ctx)
    if channels not in (1, 3):
        raise UwipError(UWIP_ERR_INVALID, "channels must be 1 or 3")
    if len(streams) == 0:
        return torch.empty((0, 0, 0, 3) if channels == 3 else (0, 0, 0), dtype=torch.uint8, device=f"cuda:{ctx.device}"), []
    size = None
    for s in streams:
        try:
            size = info(s)[:2]
            break
        except UwipError:
            continue
    if size is None:
        raise UwipError(UWIP_ERR_INVALID, "no stream of the batch parses: the frame size is unknown")
    H, W = size
    shape = (len(streams), H, W, 3) if channels == 3 else (len(streams), H, W)
    frames = torch.empty(shape, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    status = decode_into(ctx, streams, frames, sync_rounds)
    ctx.sync()
    return frames, status.cpu().tolist()
