"""CPU: the baseline JPEG writer of the decoder tests (tests/_jpeg_forge.py) against Pillow (libjpeg) alone: nothing of the
library is run here.  Every stream whose reference is Pillow's decode must decode in Pillow; a Pillow stream read by the
forge's reader and written again by the forge decodes to Pillow's own pixels; the forms the forge says it writes are in the
streams."""
import numpy as np
import pytest

import _jpeg_forge as jf
import _jpeg_forge_cases as fc
import _jpeg_streams as js


def test_every_equality_stream_decodes_in_pillow():
    named = fc.equality_streams()
    # 3 sizes x (27 factor triples x 2 intervals + 4 grey factors x 3 intervals) + 3 grey factors up to 4 x 2 intervals
    # + 18 restart + 8 header forms + the long one
    assert len(named) == 3 * (54 + 12) + 6 + 18 + 8 + 1 == 231 and len({n for n, _ in named}) == 231
    for n, f in named:
        grey = f.bpm == 1 and n[0] == "g"
        for channels in ((3, 1) if grey else (3,)):
            a = js.pil_decode(f.stream, channels)                    # raises where libjpeg refuses the stream
            if n[0] in "cg":
                W, H = (int(v) for v in n.split("_")[1].split("x"))
                assert a.shape[:2] == (H, W), n
    # the faults' twins are valid streams too (outside the amplitude bound: only that they decode is asked)
    for n, bad, twin, inside, at in fc.bad_streams():
        assert js.pil_decode(twin.stream).shape == (fc.BH, fc.BW, 3), n


@pytest.mark.parametrize("form", ["420", "444", "422_rst", "grey_opt"])
def test_pillow_coefficients_written_by_the_forge_decode_to_pillows_pixels(form):
    img = js.content(53, 37)
    s = {"420": lambda: js.pil_stream(img, 90, 2), "444": lambda: js.pil_stream(img, 97, 0),
         "422_rst": lambda: js.pil_stream(img, 75, 1, restart_marker_blocks=2),
         "grey_opt": lambda: js.pil_stream(np.ascontiguousarray(img[..., 1]), 85, optimize=True)}[form]()
    r = jf.read_coefs(s)
    assert (r["H"], r["W"]) == (53, 37) and np.abs(r["coefs"][:, 1:]).sum() > 1000
    g = jf.forge(r["W"], r["H"], r["factors"], qt=[r["qt"][0], r["qt"][-1]], coefs=r["coefs"], ri=r["ri"], safe=False)
    assert np.array_equal(js.pil_decode(g.stream), js.pil_decode(s))
    if form != "grey_opt":          # with the Annex K tables the forge writes the very bytes libjpeg wrote
        assert g.stream[g.seg:] == s[js.segment_start(s):]
    # and through other tables, ids and header forms the same pixels still
    kw = dict(one_dht=True, huff_ids=(2, 3), fill=1, sof=0xC1, comp_ids=(10, 11, 12), com_fake_sos=True, q16=True)
    h = jf.forge(r["W"], r["H"], r["factors"], qt=[r["qt"][0], r["qt"][-1]], coefs=r["coefs"], ri=r["ri"], safe=False, **kw)
    assert np.array_equal(js.pil_decode(h.stream), js.pil_decode(s))


def test_reader_returns_what_the_forge_wrote():
    named = fc.equality_colour(37, 53)[::5] + fc.equality_grey(37, 53)[::2] + fc.restart_streams()[::4] + fc.header_streams()
    for n, f in named:
        r = jf.read_coefs(f.stream)
        assert np.array_equal(r["coefs"], f.coefs), n
        assert all(np.array_equal(a, b) for a, b in zip(r["qt"], [f.qt[0], f.qt[1], f.qt[1]])), n


def test_grey_factors_in_sof_do_not_change_libjpegs_pixels():
    """T.81 A.2.2: a scan of one component is not interleaved, whatever factors SOF gives the component."""
    for W, H in fc.SIZES:
        named = dict(fc.equality_grey(W, H))
        for ri in (0, 1, 5):
            ref = js.pil_decode(named[f"g11_{W}x{H}_ri{ri}"].stream, 1)
            assert ref.shape == (H, W)
            for h, v in fc.GREY_FACTORS[1:]:
                assert np.array_equal(js.pil_decode(named[f"g{h}{v}_{W}x{H}_ri{ri}"].stream, 1), ref), (W, H, ri, h, v)
    for n, f in fc.equality_grey_to_4():
        assert np.array_equal(js.pil_decode(f.stream, 1), js.pil_decode(dict(fc.equality_grey(37, 53))["g11" + n[3:]].stream, 1)), n


def test_block_forms_are_in_the_streams():
    """Sparse AC, a coefficient at index 63, DC-only blocks, one, two and three ZRLs, and a ZRL that closes the block."""
    seen = set()
    for n, f in fc.equality_colour(37, 53)[:6]:
        for i, b in enumerate(f.coefs):
            syms = jf.block_symbols(b, 0, bool(f.zrl_close[i]))[1:]
            zrl = sum(1 for s in syms if s[1] == 0xF0)
            if b[63]:
                assert syms[-1][1] not in (0x00, 0xF0)
                seen.add("no EOB")
            elif f.zrl_close[i]:
                assert syms[-1][1] == 0xF0 and 0x00 not in [s[1] for s in syms]
                seen.add("closed by ZRL")
            else:
                assert syms[-1][1] == 0x00
            if not b[1:].any():
                seen.add("DC only")
            if not f.zrl_close[i]:
                seen.add(f"{zrl} ZRL")
        assert np.abs(f.coefs * np.array([f.qt[min(int(c), 1)][jf.ZZ] for c in f.comp])).sum(axis=1).max() <= 1024
    assert seen >= {"no EOB", "closed by ZRL", "DC only", "0 ZRL", "1 ZRL", "2 ZRL", "3 ZRL"}, seen


def test_amplitude_bound_is_asserted():
    c = np.zeros((1, 64), dtype=np.int64)
    c[0, :3] = (60, 30, 20)                      # x 10: 1100
    with pytest.raises(AssertionError):
        jf.forge(8, 8, [(1, 1)], qt=[np.full(64, 10)], coefs=c)
    c[0, 0] = 52                                 # 1020
    jf.forge(8, 8, [(1, 1)], qt=[np.full(64, 10)], coefs=c)


def test_segment_is_stuffed_padded_with_ones_and_restarts_are_cyclic():
    for n, f in fc.restart_streams() + [("long_ri0", fc.long_stream())]:
        assert f.stream[-2:] == b"\xff\xd9"
        seg, ri = f.stream[f.seg:-2], int(n.split("ri")[-1])
        per = ri if 0 < ri < f.nmcu else f.nmcu
        at = [i for i in range(len(seg) - 1) if seg[i] == 0xFF and seg[i + 1] != 0]
        assert [seg[i + 1] for i in at] == [0xD0 + i % 8 for i in range((f.nmcu + per - 1) // per - 1)], n
        assert len(f.ibits) == len(at) + 1
        for a, b, bits in zip([0] + [i + 2 for i in at], at + [len(seg)], f.ibits):
            raw = seg[a:b].replace(b"\xff\x00", b"\xff")
            assert len(raw) == (bits + 7) // 8, n
            pad = 8 * len(raw) - bits
            assert raw[-1] & ((1 << pad) - 1) == (1 << pad) - 1, n
    assert b"\xff\x00" in fc.long_stream().stream[fc.long_stream().seg:]
