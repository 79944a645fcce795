"""CPU: the gain compensation kernels of csrc/strip.hip -- k_strip_gain_stats, k_strip_gain_solve and the gained
k_strip_render -- run on host threads (tests/strip_gain_emulated.cpp, a stand-alone program built with
-fsanitize=address,undefined -ffp-contract=off) and must give the numpy mirror's statistics, gains, canvases and cover planes,
exactly, on cases A, C, D and E of tests/_strip_gain_cases.py."""
import subprocess

import numpy as np
import pytest

import _emu_build as eb
import _strip_gain_cases as cases
import _strip_gain_mirror as gm
import _strip_mirror as sm


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip_gain_emu")
    exe = eb.build(d, "strip.hip", "strip_gain_emulated.cpp", flags=eb.SANITIZE + ("-g", "-fno-sanitize-recover=undefined", "-ffp-contract=off"),
                   include=("include",))
    return exe, d


@pytest.mark.parametrize("name", ["a", "c", "d", "e"])
def test_kernels_on_host_threads_equal_the_mirror(emu, name):
    exe, d = emu
    (frames, H, ratio, kw), ch, st, gq, g = cases.expected(name)
    n, h, w = frames.shape[:3]
    max_rows, max_cols, max_scale = kw.get("max_rows", 16384), kw.get("max_cols", 16384), kw.get("max_scale", 4.0)
    cfg = gm.DEFAULTS
    fin, fout = str(d / f"{name}.in"), str(d / f"{name}.out")
    with open(fin, "wb") as f:
        f.write(np.array([n, h, w, max_rows, max_cols], np.int32).tobytes())
        f.write(np.array([max_scale, cfg["sigma_n"], cfg["sigma_g"]], np.float32).tobytes())
        f.write(np.array([cfg["lo"], cfg["hi"], cfg["min_pixels"]], np.int32).tobytes())
        f.write(np.ascontiguousarray(H, np.float64).tobytes())
        f.write(np.ascontiguousarray(ratio, np.float32).tobytes())
        f.write(np.ascontiguousarray(frames).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    raw = open(fout, "rb").read()
    at = [0]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype, count, at[0])
        at[0] += a.nbytes
        return a

    nseg = int(take(np.int32, 1)[0])
    segs = [tuple(int(v) for v in s[:6]) for s in take(np.int32, 8 * nseg).reshape(nseg, 8)]
    assert segs == ch["segs"] and np.array_equal(take(np.int32, n), ch["seg"])
    assert np.array_equal(take(np.uint64, 7 * n).reshape(n, 7), st)
    assert np.array_equal(take(np.int32, 3 * n).reshape(n, 3), gq)
    assert np.array_equal(take(np.float64, 3 * n).view(np.uint64), g.reshape(-1).view(np.uint64))       # bit for bit
    exp = cases.expected_render(name)
    for si, s in enumerate(segs):
        rows, cols = s[4], s[5]
        for mode in (sm.FEATHER, sm.FIRST, sm.LAST):
            canvas, cover = take(np.uint8, rows * cols * 3).reshape(rows, cols, 3), take(np.uint8, rows * cols).reshape(rows, cols)
            ec, ev = exp[(si, mode)]
            assert int((canvas != ec).sum()) == 0 and int((cover != ev).sum()) == 0, (si, mode)
    assert at[0] == len(raw)
    if name == "e":
        assert int(st[1][4:].max()) > 2 ** 32, "case E is there for sums beyond 32 bits"
    for k in range(n):                                      # a pair across a break has all-zero statistics
        if k == 0 or ch["seg"][k] != ch["seg"][k - 1]:
            assert not st[k].any()
