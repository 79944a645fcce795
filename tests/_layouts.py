"""Batches laid out the way a cv::Mat ROI or a pitched allocation lays them out, for the tests (a plain helper module: no
fixtures).  uwip_batch_u8 allows any step >= cols * channels, any frame_stride >= step * rows and any base address, and
behind it most kernels have two bodies chosen from the alignment of exactly those three fields; `place` builds every
combination the launchers distinguish, inside a canary-filled buffer.

With rowbytes = W * channels and r16 = rowbytes rounded up to a multiple of 16:

    name     base mod 16   step                         frame_stride
    packed   0             rowbytes                     step * rows
    pad16    0             r16 + 16                     step * rows + 48
    pad8     8             r16 + 8                      step * rows + 8 k, the first k >= 1 that makes it = 8 mod 16
    pad4     4             r16 + 4                      step * rows + 4 k, the first k >= 1 that makes it = 4 mod 16
    odd      5             rowbytes + 13 or + 14 (odd)  step * rows + 1001 or + 1002 (odd)
"""
import numpy as np
import torch

CANARY = 0xA5
GUARD = 4096                      # bytes of canary in front of the first frame and behind the last one (at least)
LAYOUTS = ("packed", "pad16", "pad8", "pad4", "odd")


def _roundup(n, a):
    return (n + a - 1) // a * a


def geometry(layout, rows, rowbytes):
    """(base address mod 16, step, frame_stride) of the table above."""
    r16 = _roundup(rowbytes, 16)
    if layout == "packed":
        return 0, rowbytes, rowbytes * rows
    if layout == "pad16":
        step = r16 + 16
        return 0, step, step * rows + 48
    if layout in ("pad8", "pad4"):
        a = 8 if layout == "pad8" else 4
        step = r16 + a
        fs = step * rows + a
        while fs % 16 != a:
            fs += a
        return a, step, fs
    if layout == "odd":
        step = rowbytes + 13 if (rowbytes + 13) % 2 else rowbytes + 14
        fs = step * rows + 1001 if (step * rows + 1001) % 2 else step * rows + 1002
        return 5, step, fs
    raise ValueError(layout)


def place(frames, layout, device):
    """frames: numpy uint8 [F, H, W] or [F, H, W, 3].  Returns (buf, view): buf is one flat uint8 tensor full of CANARY,
    view a torch.as_strided window of it with the layout's base residue, step and frame_stride, holding the frames."""
    frames = np.array(frames, order="C")              # a copy: the caller's array may be read-only, which torch warns about
    assert frames.dtype == np.uint8 and frames.ndim in (3, 4) and (frames.ndim == 3 or frames.shape[3] == 3)
    F, H, W = frames.shape[:3]
    ch = 3 if frames.ndim == 4 else 1
    rowbytes = W * ch
    res, step, fs = geometry(layout, H, rowbytes)
    extent = (F - 1) * fs + (H - 1) * step + rowbytes
    buf = torch.full((GUARD + 16 + extent + GUARD,), CANARY, dtype=torch.uint8, device=device)
    off = GUARD + (res - (buf.data_ptr() + GUARD)) % 16
    size, stride = ((F, H, W, 3), (fs, step, 3, 1)) if ch == 3 else ((F, H, W), (fs, step, 1))
    view = torch.as_strided(buf, size, stride, off)
    view.copy_(torch.from_numpy(frames).to(device))
    assert view.data_ptr() % 16 == res and off >= GUARD and buf.numel() - (off + extent) >= GUARD
    return buf, view


def place_like(shape, layout, device):
    """A destination batch of the given [F, H, W(, 3)] shape: its frames hold zeros, everything else CANARY."""
    return place(np.zeros(shape, np.uint8), layout, device)


def layout_of(view):
    """(base address mod 16, step, frame_stride) of a placed view."""
    return view.data_ptr() % 16, view.stride(1), view.stride(0)


def assert_only_frames_written(buf, view, before=None):
    """Every byte of buf outside [f, y, 0:rowbytes] of view is still CANARY; with `before` (a copy of buf taken ahead of
    the call, for a batch that is an input only) the whole of buf is unchanged."""
    b = buf.detach().cpu().numpy()
    if before is not None:
        ref = before.detach().cpu().numpy() if isinstance(before, torch.Tensor) else np.asarray(before)
        diff = np.nonzero(b != ref)[0]
        assert diff.size == 0, f"an input batch was written: {diff.size} bytes, the first at offset {int(diff[0])}"
    F, H = view.shape[:2]
    rowbytes = int(np.prod(view.shape[2:]))
    fs, step = view.stride(0), view.stride(1)
    off = view.storage_offset() - buf.storage_offset()
    outside = np.ones(b.size, bool)
    for f in range(F):
        for y in range(H):
            s = off + f * fs + y * step
            outside[s:s + rowbytes] = False
    bad = np.nonzero(outside & (b != CANARY))[0]
    if bad.size:
        p = int(bad[0])
        if p < off:
            where = f"{off - p} bytes before the batch"
        elif p >= off + (F - 1) * fs + (H - 1) * step + rowbytes:
            where = f"{p - (off + (F - 1) * fs + (H - 1) * step + rowbytes)} bytes after the batch"
        else:
            f, r = divmod(p - off, fs)
            y, x = divmod(r, step)
            where = f"the gap behind frame {f}" if y >= H else f"the row padding of frame {f}, row {y}, byte {x}"
        raise AssertionError(f"{bad.size} bytes outside the frames were written, the first in {where}")
