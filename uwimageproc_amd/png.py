"""cv2.imwrite(".png") / cv2.imencode(".png") and cv2.imdecode for a batch, on the device (uwip_png_encode / uwip_png_decode,
include/uwip.h).

The streams are lossless PNG -- colour type 2 for BGR frames (RGB in the file), 0 for grey ones, adaptive row filters, a
deflate of runs and per-chunk Huffman codes -- whose pixels are the input's; the bytes are neither OpenCV's nor cli/imgio.hpp's.
Decoding returns the pixels of the CLIs' host reader (imgio::read_png, cli/imgio.hpp) for 8-bit non-interlaced grey, grey +
alpha, RGB and RGBA streams of any encoder.  No compute happens here and there is no CPU path: the frames are a device tensor
and the kernels of csrc/png_encode.hip and csrc/png_decode.hip do the work.
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


# ---- decoding (uwip_png_decode, csrc/png_decode.hip) -----------------------------------------------------------------------
BAD_STREAM, SIZE_MISMATCH = -1, -2


def info(stream: bytes) -> Tuple[int, int, int]:
    """``(rows, cols, channels)`` of a PNG stream the host reader would inflate (``uwip_png_info``; host only); channels is 1
    for grey and grey + alpha, 3 for RGB and RGBA.  Raises ``UwipError`` for anything else (palette, 16 bit, interlaced,
    truncated chunks, not a PNG ...)."""
    r, c, ch = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    buf = (C.c_uint8 * max(len(stream), 1)).from_buffer_copy(bytes(stream) or b"\0")
    rc = lib().uwip_png_info(C.cast(buf, _P), len(stream), C.byref(r), C.byref(c), C.byref(ch))
    if rc != 0:
        raise UwipError(rc, "not a PNG stream the decoder reads")
    return r.value, c.value, ch.value


def decode_into(ctx: Context, streams: List[bytes], out, segmented: int = -1, counts=None, chunk_bytes: int = 0):
    """Decodes ``streams`` into the device tensor ``out`` (``[F, H, W, 3]`` BGR or ``[F, H, W]`` grey, any strides with packed
    pixels); returns the int32 device tensor of per-frame statuses.  ``counts``: an int64 device tensor of 3 that receives the
    units accepted from a parallel pass (segments; with ``segmented=2`` also the chunks of found block starts), the frames that
    took the serial pass, the frames.  ``chunk_bytes``: with ``segmented=2`` the compressed bytes per speculative chunk (256 ..
    1 MiB; 0 the library's choice); the result does not depend on it.  Asynchronous on the context's stream."""
    import torch

    from ._native import PngDecodeOpts

    _need_context(ctx)
    if not out.is_cuda:
        raise UwipError(UWIP_ERR_INVALID, "device tensor expected: there is no CPU fallback")
    n = len(streams)
    b = batch_of(out if out.dim() != 3 else out.unsqueeze(-1))
    bufs = [(C.c_uint8 * max(len(s), 1)).from_buffer_copy(bytes(s) or b"\0") for s in streams]
    ptrs = (_P * max(n, 1))(*[C.cast(x, _P) for x in bufs])
    sizes = (C.c_size_t * max(n, 1))(*[len(s) for s in streams])
    status = torch.empty((n,), dtype=torch.int32, device=out.device)
    opts = PngDecodeOpts(int(segmented), int(chunk_bytes), counts.data_ptr() if counts is not None else None)
    torch.cuda.current_stream(out.device).synchronize()
    ctx.call("uwip_png_decode", ptrs, sizes, n, C.byref(b), C.byref(opts), _P(status.data_ptr()))
    return status


def decode(ctx: Context, streams: List[bytes], channels: int = 3, segmented: int = -1, chunk_bytes: int = 0):
    """``cv2.imdecode`` for a batch of equally sized PNG streams, on the device: returns ``(frames, status)``, ``frames`` a
    uint8 device tensor ``[F, H, W, 3]`` (BGR; a grey stream replicated) or ``[F, H, W]`` (``channels=1``, grey streams only)
    of the size of the first stream that parses (none does: ``UwipError``; no streams: an empty batch), ``status`` a list with
    0 or ``BAD_STREAM`` / ``SIZE_MISMATCH`` per frame (the pixels of such a frame are unspecified).  ``segmented=2`` inflates
    streams of other encoders in parallel from found block starts (``chunk_bytes`` as in ``decode_into``)."""
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
    status = decode_into(ctx, streams, frames, segmented, chunk_bytes=chunk_bytes)
    ctx.sync()
    return frames, status.cpu().tolist()
