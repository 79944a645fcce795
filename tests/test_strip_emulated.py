"""CPU: the kernels of csrc/strip.hip run on host threads (tests/strip_emulated.cpp, a stand-alone program built with
-fsanitize=address,undefined -ffp-contract=off) and must give the numpy mirror's chain outputs, canvases and cover planes,
exactly, on cases A-C of tests/_strip_cases.py."""
import subprocess

import numpy as np
import pytest

import _emu_build as eb
import _strip_cases as cases
import _strip_mirror as sm


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip_emu")
    exe = eb.build(d, "strip.hip", "strip_emulated.cpp", flags=eb.SANITIZE + ("-g", "-fno-sanitize-recover=undefined", "-ffp-contract=off"),
                   include=("include",))
    return exe, d


def run_case(emu, name, frames, H, ratio, kw, placements):
    exe, d = emu
    n, h, w = frames.shape[:3]
    max_rows, max_cols, max_scale = kw.get("max_rows", 16384), kw.get("max_cols", 16384), kw.get("max_scale", 4.0)
    fin, fout = str(d / f"{name}.in"), str(d / f"{name}.out")
    with open(fin, "wb") as f:
        f.write(np.array([n, h, w, max_rows, max_cols], np.int32).tobytes())
        f.write(np.array([max_scale], np.float32).tobytes())
        f.write(np.ascontiguousarray(H, np.float64).tobytes())
        f.write(np.ascontiguousarray(ratio, np.float32).tobytes())
        f.write(np.ascontiguousarray(frames).tobytes())
    r = subprocess.run([exe, fin, fout, placements], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    exp = sm.chain(H, ratio, w, h, max_rows, max_cols, max_scale)
    raw = open(fout, "rb").read()
    at = [0]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype, count, at[0])
        at[0] += a.nbytes
        return a

    nseg = int(take(np.int32, 1)[0])
    segs = [tuple(int(v) for v in s[:6]) for s in take(np.int32, 8 * nseg).reshape(nseg, 8)]
    assert segs == exp["segs"]
    G, Gi = take(np.float64, 9 * n).reshape(n, 9), take(np.float64, 9 * n).reshape(n, 9)
    assert np.array_equal(G.view(np.uint64), exp["G"].view(np.uint64)) and np.array_equal(Gi.view(np.uint64), exp["Ginv"].view(np.uint64))
    assert np.array_equal(take(np.int32, n), exp["seg"]) and np.array_equal(take(np.int32, 4 * n).reshape(n, 4), exp["box"])
    mismatches = 0
    for s in segs:
        rows, cols = s[4], s[5]
        for mode in (sm.FEATHER, sm.FIRST, sm.LAST):
            canvas, cover = take(np.uint8, rows * cols * 3).reshape(rows, cols, 3), take(np.uint8, rows * cols).reshape(rows, cols)
            ec, ev = sm.render(frames, exp["Ginv"], s, mode, fill=(7, 99, 200))
            mismatches += int((canvas != ec).sum()) + int((cover != ev).sum())
    assert at[0] == len(raw)
    assert mismatches == 0
    return exp


def test_case_a_every_write_out_body(emu):
    frames, H, ratio, kw = cases.case_a()
    run_case(emu, "a", frames, H, ratio, kw, "all")


def test_case_b_more_frames_than_one_cull_chunk(emu):
    frames, H, ratio, kw = cases.case_b()
    run_case(emu, "b", frames, H, ratio, kw, "rotate")


def test_case_b_identical_positions_saturate_the_cover(emu):
    frames, H, ratio, kw = cases.case_b(identical=True)
    exp = run_case(emu, "b_same", frames, H, ratio, kw, "rotate")
    assert exp["segs"] == [(0, 300, 0, 0, 7, 9)]
    assert (sm.render(frames, exp["Ginv"], exp["segs"][0])[1] == 255).all()


def test_case_c_every_break_rule(emu):
    frames, H, ratio, kw = cases.case_c()
    exp = run_case(emu, "c", frames, H, ratio, kw, "rotate")
    assert tuple(s[0] for s in exp["segs"]) == cases.C_STARTS
