"""CPU: the kernels of csrc/jpeg_decode.hip run on host threads (tests/jpeg_decode_emulated.cpp, built with the address and
undefined-behaviour sanitizers) and must return the host decoder's pixels (jpeg::decode, cli/jpeg.hpp) for every stream it
decodes, BAD_STREAM where it does not, and write nothing outside the frame."""
import os
import subprocess

import numpy as np
import pytest

import _emu_build as eb
import _jpeg_forge_cases as fc
import _jpeg_streams as js


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpd_emu")
    exe = eb.build(d, "jpeg_decode.hip", "jpeg_decode_emulated.cpp", "kernels_dec.inc", eb.SANITIZE + ("-fno-sanitize-recover=all",))

    def run(cases, dump=False):
        """cases: [(name, stream, channels, rounds)] -> {(name, rounds): dict of the printed fields}; with `dump` also
        "pixels": the bytes the host decoder returned (None where it refused)"""
        lines = []
        for name, stream, ch, rounds in cases:
            p = str(d / (name + ".jpg"))
            open(p, "wb").write(stream)
            if dump and os.path.exists(p[:-4] + ".host"):
                os.remove(p[:-4] + ".host")
            lines.append(f"{p} {rounds} {ch}" + (f" {p[:-4]}.host" if dump else ""))
        lst = str(d / "list.txt")
        open(lst, "w").write("\n".join(lines) + "\n")
        r = subprocess.run([exe, lst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out = {}
        for ln in r.stdout.splitlines():
            w = ln.split()
            out[(os.path.basename(w[0])[:-4], int(w[1]))] = {"status": int(w[3]), "host": int(w[5]), "equal": int(w[7]), "clean": int(w[9]),
                                                            "unsettled": int(w[11]), "lanes": int(w[13])}
        assert len(out) == len(cases), r.stdout[-3000:]
        for (name, _), v in out.items() if dump else ():
            p = str(d / (name + ".host"))
            v["pixels"] = open(p, "rb").read() if os.path.exists(p) else None
        return out

    def batch(streams, ch, rows, cols, rounds):
        """the streams in one call -> per frame the dict of the printed fields"""
        paths = []
        for i, stream in enumerate(streams):
            paths.append(str(d / f"batch{i}.jpg"))
            open(paths[-1], "wb").write(stream)
        lst = str(d / "batch.txt")
        open(lst, "w").write(f"batch {rounds} {ch} {rows} {cols} " + " ".join(paths) + "\n")
        r = subprocess.run([exe, lst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out = [{"status": int(w[5]), "single": int(w[7]), "same": int(w[9]), "clean": int(w[11])} for w in map(str.split, r.stdout.splitlines())]
        assert len(out) == len(streams), r.stdout[-3000:]
        return out
    run.batch = batch
    return run


def test_every_kind_at_every_round_count(emu):
    cases = [(n, s, ch, r) for n, s, ch in js.kinds() for r in (0, 1, -1)]
    noise = js.content(135, 243, "noise")
    for sub in (0, 2):
        s = js.pil_stream(noise, 100, sub)
        assert b"\xff\x00" in s[js.segment_start(s):]
        cases += [(f"noise_s{sub}", s, 3, r) for r in (0, 1, -1)]
    g = js.pil_stream(np.ascontiguousarray(noise[..., 0]), 100)
    cases += [("noise_grey1", g, 1, r) for r in (0, -1)]
    std = js.pil_stream(js.content(61, 83), 90, 2)
    assert js.strip_dht(std) != std
    cases += [("nodht", js.strip_dht(std), 3, r) for r in (0, -1)]
    res = emu(cases)
    bad = {k: v for k, v in res.items() if not (v["status"] == 0 and v["host"] and v["equal"] and v["clean"])}
    assert not bad, bad
    # the noise frame spans many subsequences, and the sync rounds settle them
    assert res[("noise_s0", -1)]["lanes"] > 100
    assert res[("noise_s0", 0)]["unsettled"] > res[("noise_s0", -1)]["unsettled"]


def test_a_batch_in_one_call_equals_its_streams_alone(emu):
    """Four streams into one 17 x 33 batch: every per-frame base of the plan is non-zero somewhere, and the 16 x 16 stream, which
    the host refuses (SIZE_MISMATCH), takes no room.  Each frame must have the status and the bytes that the same stream gets
    alone -- the form every other test here holds to the host decoder -- and nothing else is written."""
    img = js.content(17, 33)
    s444 = js.pil_stream(img, 95, 0)
    a = js.segment_start(s444)
    streams = [js.pil_stream(img, 95, 2), js.pil_stream(js.content(16, 16), 95, 2), js.pil_stream(np.ascontiguousarray(img[..., 1]), 95),
               s444[:a + (len(s444) - a) // 2]]
    for rounds in (0, -1):
        res = emu.batch(streams, 3, 17, 33, rounds)
        assert [v["status"] for v in res] == [0, -2, 0, 0], res
        assert all(v["status"] == v["single"] and v["same"] and v["clean"] for v in res), res


def test_truncated_streams_follow_the_host_decoder(emu):
    cases, restart = [], set()
    for sub in (0, 1, 2, "grey"):
        for form in ("plain", "rstrows"):
            img = js.content(61, 83)
            s = js.pil_stream(np.ascontiguousarray(img[..., 1]) if sub == "grey" else img, 95, 0 if sub == "grey" else sub, **js.FORMS[form])
            a = js.segment_start(s)
            for i, cut in enumerate((a, a + 1, a + (len(s) - a) // 3, a + (len(s) - a) // 2 + 1, len(s) - 3, len(s) - 2, len(s) - 1)):
                name = f"trunc_s{sub}_{form}_{i}"
                if form != "plain":
                    restart.add(name)
                cases += [(name, s[:cut], 3, r) for r in (0, -1)]
    # the other forms and sizes, at three cut points each
    for H, W in ((61, 83), (17, 33), (16, 16), (135, 243)):
        for sub in (0, 1, 2, "grey"):
            for form in (("optimize", "rstblocks") if (H, W) == (61, 83) else tuple(js.FORMS)):
                if (H, W) == (135, 243) and (sub in (1, "grey") or form in ("optimize", "rstblocks")):
                    continue
                img = js.content(H, W)
                s = js.pil_stream(np.ascontiguousarray(img[..., 1]) if sub == "grey" else img, 95, 0 if sub == "grey" else sub, **js.FORMS[form])
                a = js.segment_start(s)
                for i, cut in enumerate((a + 2, a + (len(s) - a) // 2, len(s) - 2)):
                    name = f"trunc_{H}x{W}_s{sub}_{form}_{i}"
                    if form.startswith("rst"):
                        restart.add(name)
                    cases.append((name, s[:cut], 3, -1))
    res = emu(cases)
    for (name, r), v in res.items():
        assert v["clean"], (name, r, v)
        if v["status"] == 0:
            assert v["host"] and v["equal"], (name, r, v)
        elif v["status"] == -3:
            assert name in restart, (name, r, v)          # fewer RSTn than intervals: the host decoder's business
        else:
            assert v["status"] == -1 and not v["host"], (name, r, v)
    # a stream without restart markers is decoded on the device wherever it is cut
    assert all(v["status"] == 0 for (name, r), v in res.items() if name not in restart)


def test_noise_in_the_segment_is_bad_stream_or_the_host_pixels(emu):
    cases = []
    for sub in (0, 2):
        s = js.pil_stream(js.content(61, 83), 95, sub, optimize=True)
        a = js.segment_start(s)
        for seed in range(6):
            rng = np.random.default_rng(seed)
            t = bytearray(s)
            at = int(rng.integers(a, len(s) - 40))
            noise = rng.integers(0, 255, size=32, dtype=np.uint8)          # no 0xFF: the segment keeps its marker layout
            t[at:at + 32] = noise.tobytes()
            cases += [(f"noisy_s{sub}_{seed}", bytes(t), 3, r) for r in (0, 1, -1)]
    res = emu(cases)
    for (name, r), v in res.items():
        assert v["clean"], (name, r, v)
        if v["host"]:
            assert v["status"] == 0 and v["equal"], (name, r, v)
        else:
            assert v["status"] == -1, (name, r, v)


def test_quantisers_of_255_take_the_64_bit_path(emu):
    s = bytearray(js.pil_stream(js.content(17, 33, "noise"), 100, 0))
    pos, n = 2, 0
    while s[pos + 1] != 0xDA:
        L = (s[pos + 2] << 8) | s[pos + 3]
        if s[pos + 1] == 0xDB:
            q = pos + 4
            while q < pos + 2 + L:
                assert s[q] >> 4 == 0
                s[q + 1:q + 65] = b"\xff" * 64
                q += 65
                n += 1
        pos += 2 + L
    assert n == 2
    res = emu([("q255", bytes(s), 3, r) for r in (0, -1)])
    for k, v in res.items():
        assert v["status"] == 0 and v["host"] and v["equal"] and v["clean"], (k, v)


def test_host_only_streams_are_reported_not_decoded(emu):
    img = js.content(61, 83)
    rst = js.pil_stream(img, 95, 2, restart_marker_rows=1)
    s422 = js.pil_stream(img, 95, 1)
    extra = rst[:-2] + b"\xff\xd7" + rst[-2:]                     # one RSTn more than intervals, before EOI
    cases = [("ho_misplaced", js.misplaced_rst(rst), 3, -1), ("ho_1x2", js.sampled_1x2(s422), 3, -1), ("ho_extra", extra, 3, -1),
             ("ho_ref", rst, 3, -1)]
    res = emu(cases)
    assert res[("ho_ref", -1)]["status"] == 0 and res[("ho_ref", -1)]["equal"]
    for name in ("ho_misplaced", "ho_1x2", "ho_extra"):
        v = res[(name, -1)]
        assert v["status"] == -3 and v["host"] and v["clean"], (name, v)


def test_mutated_headers_are_accepted_or_rejected_as_the_host_decoder_does(emu):
    """jpeg_parse.hpp is the header walk of both decoders: with one header byte changed they must still agree on whether
    the stream decodes (PARSE_BAD is the host decoder's `false`; a host-only stream is one the host decodes), and on the
    pixels where it does."""
    s = js.pil_stream(js.content(17, 33), 90, 2, restart_marker_blocks=3)
    a = js.segment_start(s)
    rng = np.random.default_rng(5)
    marks = [i for i in range(2, a - 1) if s[i] == 0xFF and s[i + 1] not in (0, 0xFF)]
    at = sorted(set(int(v) for v in rng.integers(2, a, size=6)) | {m + d for m in marks for d in (1, 2, 3)} |
                {s.index(b"\xff\xc0") + d for d in range(4, 19)})
    cases = [(f"mut_{i}_{val}", s[:i] + bytes([val]) + s[i + 1:], 3, -1)
             for i in at if i < a for val in sorted({0xFF, s[i] ^ 0x01, s[i] ^ 0x10} - {s[i]})]
    res = emu(cases)
    assert len(res) > 100
    n_bad = 0
    for (name, r), v in res.items():
        assert v["clean"], (name, v)
        if v["status"] == -1:
            assert not v["host"], (name, v)
            n_bad += 1
        elif v["status"] == 0:
            assert v["host"] and v["equal"], (name, v)
        else:
            assert v["status"] in (-2, -3) and v["host"], (name, v)      # a size the batch does not have / host only: both decodable
    assert n_bad > 20


# ---- streams no libjpeg encoder writes (tests/_jpeg_forge.py), against Pillow's decode ------------------------------------------
ROUNDS = (0, 1, -1)


def _equal_pillow(emu, named, channels=3):
    """Emulated kernels == host decoder == Pillow, status 0, at every round count."""
    tag = "" if channels == 3 else "_ch1"
    res = emu([(n + tag, f.stream, channels, r) for n, f in named for r in ROUNDS], dump=True)
    for n, f in named:
        want = js.pil_decode(f.stream, channels)
        for r in ROUNDS:
            v = res[(n + tag, r)]
            assert v["status"] == 0 and v["host"] and v["equal"] and v["clean"], (n, r, {k: x for k, x in v.items() if k != "pixels"})
        host = np.frombuffer(res[(n + tag, -1)]["pixels"], dtype=np.uint8).reshape(want.shape)
        assert np.array_equal(host, want), (n, int(np.abs(host.astype(int) - want).max()), float((host != want).mean()))
    return res


def test_forged_factor_combinations_equal_pillow(emu):
    """The factors are enumerated from the rule of include/uwip.h: 64 triples of (h, v) in 1..2; a component with hmax / h == 1
    and vmax / v == 2 is HOST_ONLY.  hmax = vmax = 2 needs a 2x2 component and allows 2x2, 1x1 and 1x2 beside it: 27 - 8 = 19.
    hmax = 2, vmax = 1: 2x1 and 1x1 with at least one 2x1: 7.  hmax = 1, vmax = 2: all 1x2 (a 1x1 would be 1x2 against it).
    All 1x1.  28, less the triple of 2x2 with its 12 blocks: 27."""
    assert len(fc.device_eligible()) == 27 and [(2, 2)] * 3 not in fc.device_eligible()
    for W, H in fc.SIZES:
        named = fc.equality_colour(W, H)
        assert len(named) == 54
        _equal_pillow(emu, named)


def test_forged_grey_is_one_block_per_mcu_whatever_sof_says(emu):
    for W, H in fc.SIZES:
        named = fc.equality_grey(W, H)
        assert len(named) == 12
        for h, v in fc.GREY_FACTORS[1:]:                # the same bytes but for the factors in SOF
            a, b = dict(named)[f"g11_{W}x{H}_ri5"].stream, dict(named)[f"g{h}{v}_{W}x{H}_ri5"].stream
            assert [i for i in range(len(a)) if a[i] != b[i]] == [a.index(b"\xff\xc0") + 11] and len(a) == len(b)
        _equal_pillow(emu, named)
        _equal_pillow(emu, named, channels=1)
    # factors of 3 and 4, which SOF can hold and no three-component stream may have here
    named = fc.equality_grey_to_4()
    assert len(named) == 6
    _equal_pillow(emu, named)
    _equal_pillow(emu, named, channels=1)


def test_forged_mcu_of_twelve_blocks_is_refused(emu):
    """T.81 B.2.3: an MCU has at most 10 blocks; libjpeg refuses the stream, and so do both decoders."""
    f = fc.twelve_blocks()
    assert f.bpm == 12
    with pytest.raises(Exception):
        js.pil_decode(f.stream)
    res = emu([("twelve", f.stream, 3, r) for r in ROUNDS])
    for r in ROUNDS:
        v = res[("twelve", r)]
        assert v["status"] == -1 and not v["host"] and v["clean"], (r, v)


def test_forged_restart_intervals_equal_pillow(emu):
    named = fc.restart_streams()
    assert len(named) == 18
    for tag in ("420", "422", "444"):
        f = dict(named)[f"r{tag}_ri1"]
        seg = f.stream[f.seg:]
        assert f.nmcu > 9 and seg.count(b"\xff\xd0") >= 2 and b"\xff\xd7" in seg                  # RSTn wraps
        assert f.rst_after_stuffed > 0 and any(b"\xff\x00\xff" + bytes([0xD0 + i]) in seg for i in range(8))
        for ri in (f.nmcu, f.nmcu + 1, 65535):             # an interval that holds every MCU: DRI, and no RSTn
            g = dict(named)[f"r{tag}_ri{ri}"]
            assert b"\xff\xdd" in g.stream[:g.seg] and not any(bytes([0xFF, 0xD0 + i]) in g.stream[g.seg:] for i in range(8))
    _equal_pillow(emu, named)


def test_forged_long_stream_settles_over_the_rounds(emu):
    """One interval of many subsequences: lanes that start in the middle of it read codes that are none, runs past 63 and
    categories above 11 where no symbol starts.  What such a start reads must never become the frame's status."""
    f = fc.long_stream()
    res = _equal_pillow(emu, [("long", f)])
    assert res[("long", -1)]["lanes"] > 100
    assert res[("long", 0)]["unsettled"] > 0 and res[("long", 0)]["status"] == 0 and res[("long", 0)]["equal"]
    assert res[("long", 0)]["unsettled"] > res[("long", 1)]["unsettled"] >= res[("long", -1)]["unsettled"]


def test_forged_header_forms_equal_pillow(emu):
    named = fc.header_streams()
    assert [n for n, _ in named] == ["h_q16", "h_dht23", "h_fill", "h_sof1", "h_ids", "h_com", "h_dri0", "h_all"]
    f = dict(named)["h_all"]
    head = f.stream[:f.seg]
    assert head.index(b"\xff\xda") < f.seg - 14 and b"\xff\xff\xff\xc1" in head and head.count(b"\xff\xdd") == 2 and head.count(b"\xff\xc4") == 1
    _equal_pillow(emu, named)


def test_forged_faults_are_bad_stream_and_their_twins_decode(emu):
    """include/uwip.h, UWIP_JPEG_BAD_STREAM: a DC category above 11, a run past coefficient 63, an undecodable code, a DC
    predictor outside 16 bits.  Each at the first block, behind four subsequences, at the last block and inside a later
    restart interval; the twin is the same stream one step inside the rule (category 11, a run to 63, the longest code,
    a predictor of 32752) and decodes."""
    cases = fc.bad_streams()
    assert len(cases) == 16
    lines = []
    for name, bad, twin, inside, at in cases:
        if name.endswith("_deep"):
            assert bad.pos[at][0] == 0 and bad.pos[at][1] >= 4 * fc.SUB_BITS and twin.pos[at][1] >= 4 * fc.SUB_BITS
        if name.endswith("_last"):
            assert at == len(bad.coefs) - 1
        if name.endswith("_iv5"):
            assert bad.pos[at][0] == 5 and twin.pos[at][0] == 5
        lines += [(name, bad.stream, 3, r) for r in ROUNDS] + [(name + "_twin", twin.stream, 3, r) for r in ROUNDS]
    res = emu(lines, dump=True)
    for name, bad, twin, inside, at in cases:
        for r in ROUNDS:
            v, t = res[(name, r)], res[(name + "_twin", r)]
            assert v["status"] == -1 and not v["host"] and v["clean"], (name, r, v["status"], v["host"], v["clean"])
            assert t["status"] == 0 and t["host"] and t["equal"] and t["clean"], (name, r, t["status"], t["host"], t["equal"], t["clean"])
        if inside:
            want = js.pil_decode(twin.stream)
            assert np.array_equal(np.frombuffer(res[(name + "_twin", -1)]["pixels"], dtype=np.uint8).reshape(want.shape), want), name
