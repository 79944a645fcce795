"""CPU: the found block starts of csrc/png_decode.hip (segmented = 2) run on host threads (tests/png_decode_emulated.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers).  For foreign streams of several deflate blocks
the pixels are the host reader's (imgio::read_png) whatever the chunk size, the serial pass is not needed, and every accepted
chunk starts at a true block start (tests/_png_spec_streams.py walks the stream on its own); streams with nothing to find and
a stream that carries a deflate stream inside stored blocks lose no pixel; damaged streams get the status of mode 1 and of the
host reader."""
import pytest

import _png_spec_streams as sp
from _png_emu import Emu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """cases: [(name, stream, channels, segmented, chunk_bytes)] -> {(name, segmented, chunk_bytes): the printed fields}"""
    return Emu(tmp_path_factory.mktemp("pngd_spec_emu"))


@pytest.fixture(scope="module")
def results(emu):
    S = sp.streams()
    cases = []
    for name, (s, arr) in S.items():
        cases.append((name, s, 3, 1, 0))
        cases += [(name, s, 3, 2, cb) for cb in sp.CHUNKS]
    return S, emu(cases)


def test_pixels_and_statuses_of_every_stream_in_both_modes(results):
    S, res = results
    assert len(res) == len(S) * (1 + len(sp.CHUNKS))
    bad = {k: v for k, v in res.items() if not (v["status"] == 0 and v["host"] and v["equal"] and v["clean"])}
    assert not bad, bad


def test_streams_of_several_blocks_need_no_serial_pass_and_start_at_true_block_starts(results):
    S, res = results
    for name in ("A", "B", "Bp", "C"):
        true = [b[0] for b in sp.blocks(sp.zstream(S[name][0]))]
        for cb in sp.CHUNKS:
            v = res[(name, 2, cb)]
            assert v["serial"] == 0, (name, cb, v)
            assert 2 <= v["accepted"] <= len(true), (name, cb, v, len(true))
            assert v["accepted"] == len(v["starts"]) and v["starts"][0] == 0, (name, cb, v)
            assert len(set(v["starts"])) == len(v["starts"]) and set(v["starts"]) <= set(true), (name, cb, v["starts"], true)
        assert res[(name, 1, 0)]["accepted"] == 1 and res[(name, 1, 0)]["serial"] == 0       # mode 1: one segment, the whole stream


def test_nothing_to_find_and_a_stream_inside_stored_blocks(results):
    S, res = results
    for name in ("D", "Dfixed", "E"):
        true = [b[0] for b in sp.blocks(sp.zstream(S[name][0]))]
        for cb in sp.CHUNKS:
            v = res[(name, 2, cb)]
            assert v["accepted"] + v["serial"] >= 1 and set(v["starts"]) <= set(true), (name, cb, v)
    # E: the chunks that start inside the first stored block's payload find B's blocks there and measure them cleanly; the
    # chain check alone keeps them out.  Two stored blocks: at most the first chunk and one repair are accepted.
    for cb in sp.CHUNKS:
        assert res[("E", 2, cb)]["accepted"] <= 2, res[("E", 2, cb)]
    assert all(st == 0 or st >= 65540 * 8 for st in res[("E", 2, 16384)]["starts"])


def test_damaged_streams_have_the_status_of_mode_1_and_of_the_host_reader(emu):
    cases = []
    for name, s in sp.damaged_a():
        cases += [(name, s, 3, 1, 0), (name, s, 3, 2, 4096)]
    res = emu(cases)
    n_bad = 0
    for (name, seg, cb), v in res.items():
        assert v["clean"], (name, seg, v)
        assert (v["status"] == 0) == bool(v["host"]), (name, seg, v)
        assert v["status"] in (0, -1), (name, seg, v)
        if v["host"]:
            assert v["equal"], (name, seg, v)
        if seg == 2:
            assert v["status"] == res[(name, 1, 0)]["status"], (name, v)
            n_bad += v["status"] != 0
    assert n_bad > 300 and all(res[(n, 2, 4096)]["status"] == -1 for n in ("cut", "filecut", "adler"))
