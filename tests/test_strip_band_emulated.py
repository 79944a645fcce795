"""CPU: the multi-band kernels of csrc/strip.hip -- k_strip_stack and both instantiations of k_strip_render_bands -- run on host
threads (tests/strip_band_emulated.cpp, a stand-alone program built with -fsanitize=address,undefined -ffp-contract=off) and
must give the numpy mirror's stacks, canvases and cover planes, exactly, on the cases of tests/_strip_band_cases.py."""
import subprocess

import numpy as np
import pytest

import _emu_build as eb
import _strip_band_cases as cases
import _strip_band_mirror as bm


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip_band_emu")
    exe = eb.build(d, "strip.hip", "strip_band_emulated.cpp", flags=eb.SANITIZE + ("-g", "-fno-sanitize-recover=undefined", "-ffp-contract=off"),
                   include=("include",))
    return exe, d


def gains_of(name, n):
    """the gains of a case's gained render: D's solved ones, anything in range for the others"""
    gq = cases.expected(name)[2]
    return gq if gq is not None else np.random.default_rng(53).integers(2048, 8193, (n, 3)).astype(np.int32)


@pytest.mark.parametrize("name", ["a", "c", "d", "f", "g", "h"])
def test_kernels_on_host_threads_equal_the_mirror(emu, name):
    exe, d = emu
    (frames, H, ratio, kw), ch, _, lv = cases.expected(name)
    levels, ramp, _ = cases.RENDER[name]
    n, h, w = frames.shape[:3]
    gq = gains_of(name, n)
    fin, fout = str(d / f"{name}.in"), str(d / f"{name}.out")
    with open(fin, "wb") as f:
        f.write(np.array([n, h, w, kw.get("max_rows", 16384), kw.get("max_cols", 16384)], np.int32).tobytes())
        f.write(np.array([kw.get("max_scale", 4.0)], np.float32).tobytes())
        f.write(np.array([levels, *ramp], np.int32).tobytes())
        f.write(np.ascontiguousarray(H, np.float64).tobytes())
        f.write(np.ascontiguousarray(ratio, np.float32).tobytes())
        f.write(np.ascontiguousarray(gq, np.int32).tobytes())
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
    assert segs == ch["segs"]
    stack = take(np.uint8, levels * n * h * w * 3).reshape(levels, n, h, w, 3)
    assert int((stack != lv[1:levels + 1]).sum()) == 0
    plain, big = cases.expected_render(name) if not cases.RENDER[name][2] else cases.expected_render(name, gains=4096)
    for si, s in enumerate(segs):
        rows, cols = s[4], s[5]
        gained = bm.render(frames, ch["Ginv"], s, levels, ramp, gq, cases.FILL, lv=lv[:levels + 1])
        for exp in (plain[si], gained):
            canvas, cover = take(np.uint8, rows * cols * 3).reshape(rows, cols, 3), take(np.uint8, rows * cols).reshape(rows, cols)
            assert int((canvas != exp[0]).sum()) == 0 and int((cover != exp[1]).sum()) == 0, si
    assert at[0] == len(raw)
    if name == "h":
        assert big > 2 ** 32, "case H is there for numerators beyond 32 bits"
