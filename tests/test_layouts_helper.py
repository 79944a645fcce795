"""tests/_layouts.py on the CPU: the layouts are the ones its table promises, uwip_batch_u8 would describe them the same
way, and the canary check sees a single stray byte wherever it lands."""
import numpy as np
import pytest
import torch

import _layouts
from _layouts import CANARY, GUARD, LAYOUTS, assert_only_frames_written, layout_of, place

F, H, W = 3, 7, 37


def _frames(ch):
    rng = np.random.default_rng(ch)
    return rng.integers(0, 256, (F, H, W, 3) if ch == 3 else (F, H, W), dtype=np.uint8)


def _table(layout, rows, rowbytes):
    """The issue's table, restated independently of _layouts.geometry."""
    r16 = -(-rowbytes // 16) * 16
    if layout == "packed":
        return 0, rowbytes, rowbytes * rows, None
    if layout == "pad16":
        return 0, r16 + 16, (r16 + 16) * rows + 48, None
    if layout == "pad8":
        return 8, r16 + 8, None, (8, 8)
    if layout == "pad4":
        return 4, r16 + 4, None, (4, 4)
    return 5, rowbytes + (13 if rowbytes % 2 == 0 else 14), None, None


def _batch_fields(t):
    """batch_of's arithmetic (uwimageproc_amd/_native.py) without its is_cuda assertion."""
    shape, st = list(t.shape), list(t.stride())
    if t.dim() == 3:
        shape, st = shape + [1], st + [1]
    Fn, Hn, Wn, Cn = shape
    assert st[3] == 1 and st[2] == Cn, "pixels must be packed"
    step = st[1] if Hn > 1 else Wn * Cn
    return t.data_ptr(), step, (st[0] if Fn > 1 else step * Hn), Hn, Wn, Cn, Fn


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_place_gives_the_layout_of_the_table(layout, ch):
    frames = _frames(ch)
    rowbytes = W * ch
    buf, view = place(frames, layout, "cpu")
    res, step, fs, mod = _table(layout, H, rowbytes)
    got_res, got_step, got_fs = layout_of(view)
    assert (got_res, got_step) == (res, step)
    if fs is not None:
        assert got_fs == fs
    elif mod is not None:                                   # step * rows + a * k, k >= 1 the first that gives a mod 16
        a, r = mod
        assert got_fs % 16 == r and (got_fs - step * H) % a == 0 and a <= got_fs - step * H <= 16
    else:                                                   # odd
        assert step % 2 == 1 and got_fs % 2 == 1 and got_fs - step * H in (1001, 1002)
    assert (got_res, got_step, got_fs) == _layouts.geometry(layout, H, rowbytes)
    # one flat canary-filled buffer, the frames inside, 4096 bytes of canary on either side
    assert buf.dim() == 1 and buf.dtype == torch.uint8
    assert np.array_equal(view.numpy(), frames)
    off = view.storage_offset()
    end = off + (F - 1) * got_fs + (H - 1) * got_step + rowbytes
    assert off >= GUARD and buf.numel() - end >= GUARD
    assert (buf[:off] == CANARY).all() and (buf[end:] == CANARY).all()
    # what uwip_batch_u8 would say
    data, bstep, bfs, rows, cols, chans, frames_n = _batch_fields(view)
    assert (data % 16, bstep, bfs) == (res, got_step, got_fs)
    assert (rows, cols, chans, frames_n) == (H, W, ch, F)
    assert data == buf.data_ptr() + off
    assert bstep >= cols * chans and bfs >= bstep * rows    # uwip_check_batch's conditions
    assert_only_frames_written(buf, view)
    assert_only_frames_written(buf, view, before=buf.clone())


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_canary_check_fires_on_one_planted_byte(layout, ch):
    buf, view = place(_frames(ch), layout, "cpu")
    rowbytes = W * ch
    _, step, fs = layout_of(view)
    off = view.storage_offset()
    end = off + (F - 1) * fs + (H - 1) * step + rowbytes
    spots = {"just before the batch": off - 1, "just after the batch": end}
    if step > rowbytes:
        spots["row padding"] = off + fs + 2 * step + rowbytes           # first padding byte of frame 1, row 2
        spots["last byte of the row padding"] = off + 3 * step - 1
    if fs > step * H:
        spots["frame gap"] = off + fs + H * step                        # first byte behind frame 1's last row's slot
        spots["last byte of the frame gap"] = off + 2 * fs - 1
    assert layout == "packed" or len(spots) == 6
    for where, p in spots.items():
        before = buf.clone()
        buf[p] = CANARY ^ 1
        with pytest.raises(AssertionError):
            assert_only_frames_written(buf, view)
        with pytest.raises(AssertionError):
            assert_only_frames_written(buf, view, before=before)
        buf[p] = CANARY
        assert_only_frames_written(buf, view, before=before)
    # a byte inside a frame: fine for a destination, a finding for an input
    before = buf.clone()
    view[1, 2, 3] = view[1, 2, 3] ^ 1
    assert_only_frames_written(buf, view)
    with pytest.raises(AssertionError):
        assert_only_frames_written(buf, view, before=before)


def test_working_width_is_640_for_every_source_width(orc):
    """uwip_resize_bgr's destination is lrint(cols * (float)(640 / cols)) wide: 640 for every source width, so there is no
    source shape with an odd working width for test_layouts_gpu.py to use (it takes an odd SOURCE width instead)."""
    assert {orc.resize_dims(100, c)[1] for c in range(1, 8193)} == {640}
