"""CPU: the kernels of csrc/png_decode.hip run on host threads (tests/png_decode_emulated.cpp, a stand-alone program built with
the address and undefined-behaviour sanitizers) and must return the host reader's pixels (imgio::read_png, cli/imgio.hpp,
zlib's inflate) for every stream it reads, BAD_STREAM where it does not, and write nothing outside the frame -- through the
segmented pass and through the serial one, which the counters tell apart."""
import numpy as np
import pytest

import _png_decode_streams as pd
from _png_emu import Emu

FILTERS = (0, 1, 2, 3, 4, "mix")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    e = Emu(tmp_path_factory.mktemp("pngd_emu"))

    def run(cases):
        """cases: [(name, stream, channels, segmented)] -> {(name, segmented): dict of the printed fields}"""
        return {(name, seg): v for (name, seg, _), v in e([c + (0,) for c in cases]).items()}
    run.own, run.batch = e.own, e.batch
    return run


def _good(res):
    bad = {k: v for k, v in res.items() if not (v["status"] == 0 and v["host"] and v["equal"] and v["clean"])}
    assert not bad, bad


def test_every_recipe_sample_count_and_filter_on_both_paths(emu):
    cases = []
    for recipe in pd.RECIPES:
        for spp in (1, 2, 3, 4):
            for filt in FILTERS:
                s = pd.stream(pd.content(5, 7, spp), filt, recipe)
                cases += [(f"r_{recipe}_{spp}_{filt}", s, 3, seg) for seg in (0, 1)]
    res = emu(cases)
    _good(res)
    assert all(v["accepted"] == 0 for (n, seg), v in res.items() if seg == 0)


def test_every_shape(emu):
    cases = []
    for H, W in pd.SHAPES[:4]:
        for spp in (1, 2, 3, 4):
            arr = pd.content(H, W, spp, "noise" if spp == 2 else "uw")
            for recipe in ("stored", "fixed", "l9m9", "l6cut1000", "full32k"):
                cases += [(f"s_{H}x{W}_{recipe}_{spp}", pd.stream(arr, "mix", recipe), 3, seg) for seg in (0, 1)]
            cases += [(f"s_{H}x{W}_pil_{spp}", pd.pil_stream(arr), 3, 1), (f"s_{H}x{W}_pilopt_{spp}", pd.pil_stream(arr, optimize=True), 3, 1)]
        g = pd.content(H, W, 1)
        cases += [(f"s_{H}x{W}_grey1", pd.stream(g, "mix", "l1"), 1, 1), (f"s_{H}x{W}_own3", emu.own(pd.content(H, W, 3)), 3, 1),
                  (f"s_{H}x{W}_own1", emu.own(g), 1, 1)]
    _good(emu(cases))


def test_two_and_three_segments_on_both_paths(emu):
    """97 x 113 x 3 is 32980 filtered bytes (two windows), 200 x 333 grey 66800 (three)."""
    rgb, grey, p97 = pd.content(97, 113, 3), pd.content(200, 333, 1), pd.period97()
    cases = []
    for recipe in pd.RECIPES:
        for filt in (FILTERS if recipe == "l9m9" else ("mix", 4)):
            cases += [(f"m_{recipe}_{filt}", pd.stream(rgb, filt, recipe), 3, seg) for seg in (0, 1)]
        cases += [(f"g_{recipe}", pd.stream(grey, "mix", recipe), 3, seg) for seg in ((0, 1) if recipe.startswith("full") else (1,))]
    for filt in (-1, 0, 4):
        cases += [(f"own_rgb_{filt}", emu.own(pd.content(97, 113, 3, seed=filt + 2), filt), 3, seg) for seg in (0, 1)]
    cases += [("own_grey", emu.own(grey), 1, seg) for seg in (0, 1)]
    cases += [("own_p97", emu.own(p97), 3, seg) for seg in (0, 1)]
    cases += [("p97_l9", pd.stream(p97, 0, "l9m9"), 3, seg) for seg in (0, 1)]
    cases += [("p97_sync", pd.stream(p97, 0, "sync32k"), 3, 1), ("p97_full", pd.stream(p97, 0, "full32k"), 3, 1)]
    cases += [("pil_rgb", pd.pil_stream(rgb), 3, 1), ("pil_grey_opt", pd.pil_stream(grey, optimize=True), 1, 1)]
    s = pd.stream(p97, 0, "l9m9")
    assert len(s) < 66800 * 0.55                                 # zlib halves it: the matches reach back a whole period
    res = emu(cases)
    _good(res)
    assert res[("p97_l9", 0)]["maxdist"] >= 32000 and res[("p97_l9", 1)]["maxdist"] >= 32000
    # both paths ran
    for (name, seg), v in res.items():
        if seg == 0:
            assert v["accepted"] == 0 and v["serial"] == 1, (name, v)
    for name, nseg in (("own_rgb_-1", 2), ("own_rgb_0", 2), ("own_rgb_4", 2), ("own_grey", 3), ("own_p97", 3), ("p97_full", 3), ("g_full32k", 3),
                       ("m_full32k_mix", 2)):
        assert res[(name, 1)]["accepted"] == nseg and res[(name, 1)]["serial"] == 0, (name, res[(name, 1)])
    assert res[("p97_sync", 1)]["serial"] == 1 and res[("p97_sync", 1)]["accepted"] < 3          # refused: it reaches back
    assert res[("m_full10k_mix", 1)]["serial"] == 1 and res[("m_full10k_mix", 1)]["accepted"] < 4   # refused: 10000-byte windows
    assert res[("g_full10k", 1)]["serial"] == 1


def test_a_batch_in_one_call_equals_its_streams_alone(emu):
    """Four streams into one 17 x 33 batch, with the segments (1) and the found block starts at 256-byte chunks (2): every
    per-frame base of the plan is non-zero somewhere, and the 16 x 16 stream, which the host refuses (SIZE_MISMATCH), takes no
    room.  Each frame must have the status and the bytes that the same stream gets alone -- the form every other test here
    holds to the host reader -- and nothing else is written."""
    own = emu.own(pd.content(17, 33, 3, "noise")[..., ::-1].copy())
    a, b = pd.idat_span(own)
    assert b - a >= 1700                                        # stored: at least two chunks of 256 bytes
    streams = [own, pd.pil_stream(pd.content(16, 16, 3)), pd.pil_stream(pd.content(17, 33, 2)), own[:len(own) // 2]]
    for seg, cb in ((1, 0), (2, 256)):
        res = emu.batch(streams, 3, 17, 33, seg, cb)
        assert [v["status"] for v in res] == [0, -2, 0, -1], res
        assert all(v["status"] == v["single"] and v["same"] and v["clean"] for v in res), res


def _follows_host(res):
    n_ok = 0
    for k, v in res.items():
        assert v["clean"], (k, v)
        if v["status"] == 0:
            assert v["host"] and v["equal"], (k, v)
            n_ok += 1
        else:
            assert v["status"] == -1 and not v["host"], (k, v)
    return n_ok


def test_damaged_streams_follow_the_host_reader(emu):
    cases = []
    for recipe in ("l9m9", "full32k", "stored", "fixed"):
        arr = pd.content(97, 113, 3) if recipe == "full32k" else pd.content(40, 50, 3)          # two segments; one
        s = pd.stream(arr, "mix", recipe)
        a, b = pd.idat_span(s)
        for i, cut in enumerate((a, a + 1, a + 3, a + (b - a) // 3, a + (b - a) // 2 + 1, b - 5, b - 1)):
            cases += [(f"trunc_{recipe}_{i}", s[:cut], 3, seg) for seg in (0, 1)]
        for seed in range(6):
            rng = np.random.default_rng(seed)
            t = bytearray(s)
            at = int(rng.integers(a, b - 40))
            t[at:at + 32] = rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()
            cases += [(f"noisy_{recipe}_{seed}", bytes(t), 3, seg) for seg in (0, 1)]
        t = bytearray(s)
        t[b - 1] ^= 0x40                                           # the Adler-32's last byte
        cases += [(f"adler_{recipe}", bytes(t), 3, seg) for seg in (0, 1)]
    res = emu(cases)
    _follows_host(res)
    assert all(v["status"] == -1 for (n, _), v in res.items() if n.startswith("adler_") or n.startswith("trunc_"))


def test_every_bit_of_the_zlib_header_and_of_a_dynamic_block_header(emu):
    arr = pd.content(12, 20, 3)
    big = pd.content(40, 50, 3)
    cases = []
    for tag, s, nbytes in (("small", pd.stream(arr, 0, "huffman"), 24), ("big", pd.stream(big, "mix", "l9m9"), 72)):
        a, b = pd.idat_span(s)
        assert (s[a + 2] >> 1) & 3 == 2                            # the first block is dynamic
        for i in range(min(nbytes, b - a - 4)):
            for bit in range(8):
                t = bytearray(s)
                t[a + i] ^= 1 << bit
                cases.append((f"bit_{tag}_{i}_{bit}", bytes(t), 3, 1 if (i + bit) % 2 else 0))
    res = emu(cases)
    n_ok = _follows_host(res)
    assert len(res) > 700 and n_ok < len(res) // 4


def test_ihdr_mutations_and_unsupported_kinds(emu):
    import io
    from PIL import Image
    arr = pd.content(5, 7, 3)
    s = pd.stream(arr, "mix", "l6cut1000")
    at = s.index(b"IHDR") + 4
    cases = []
    for i in range(13):
        for val in sorted({0, 1, 2, 3, 4, 6, 8, 16, s[at + i] ^ 0x01, s[at + i] ^ 0x80} - {s[at + i]}):
            if i in (0, 1, 2, 4, 5, 6):
                continue                                          # a width or height the host reader would try to allocate
            cases.append((f"ihdr_{i}_{val}", s[:at + i] + bytes([val]) + s[at + i + 1:], 3, 1))
    res = emu(cases)
    assert len(res) > 50
    for k, v in res.items():
        assert v["clean"], (k, v)
        assert (v["status"] == 0) == bool(v["host"]), (k, v)
        if v["host"]:
            assert v["equal"], (k, v)
    kinds = []
    img = Image.fromarray(arr)
    for name, im, kw in (("palette", img.convert("P"), {}), ("adam7", img, {"interlace": 1}), ("deep", Image.fromarray(np.arange(35, dtype=np.uint16).reshape(5, 7) * 900), {})):
        buf = io.BytesIO()
        if name == "adam7":
            # Pillow writes no interlaced files: set the IHDR byte of a plain one (the host reader refuses before it inflates)
            t = bytearray(pd.pil_stream(arr))
            t[t.index(b"IHDR") + 4 + 12] = 1
            kinds.append((name, bytes(t), 3, 1))
            continue
        im.save(buf, format="PNG", **kw)
        kinds.append((name, buf.getvalue(), 3, 1))
    res = emu(kinds)
    for k, v in res.items():
        assert v["status"] == -1 and not v["host"] and v["clean"], (k, v)
