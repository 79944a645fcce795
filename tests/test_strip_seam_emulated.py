"""CPU: the seam kernels of csrc/strip.hip -- k_strip_seam_cost, both instantiations of k_strip_seam_path and
k_strip_render<UWIP_STRIP_SEAM> with and without gains -- run on host threads (tests/strip_seam_emulated.cpp, a stand-alone
program built with -fsanitize=address,undefined -ffp-contract=off) and must give the numpy mirror's orientations, seams,
totals, canvases and cover planes, exactly, on the cases of tests/_strip_seam_cases.py."""
import subprocess

import numpy as np
import pytest

import _emu_build as eb
import _strip_seam_cases as cases


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip_seam_emu")
    exe = eb.build(d, "strip.hip", "strip_seam_emulated.cpp", flags=eb.SANITIZE + ("-g", "-fno-sanitize-recover=undefined", "-ffp-contract=off"),
                   include=("include",))
    return exe, d


# (case, gained, pairs per round): G in rounds of 7 and A in rounds of 3, so that a round starts inside a segment; A and S also
# with gains they do not have of their own
RUNS = [("a", False, 3), ("a", True, 64), ("c", False, 64), ("d", True, 64), ("f", False, 2), ("g", False, 7), ("s", False, 64),
        ("s", True, 1), ("ow", False, 64), ("oh", False, 5), ("l", False, 64)]


@pytest.mark.parametrize("name,gained,rnd", RUNS)
def test_kernels_on_host_threads_equal_the_mirror(emu, name, gained, rnd):
    exe, d = emu
    (frames, H, ratio, kw), ch, gq, seam, ori, total, _ = cases.expected(name, gained)
    assert (gq is not None) == gained
    n, h, w = frames.shape[:3]
    tag = f"{name}{int(gained)}"
    fin, fout = str(d / f"{tag}.in"), str(d / f"{tag}.out")
    with open(fin, "wb") as f:
        f.write(np.array([n, h, w, kw.get("max_rows", 16384), kw.get("max_cols", 16384)], np.int32).tobytes())
        f.write(np.array([kw.get("max_scale", 4.0)], np.float32).tobytes())
        f.write(np.array([1024, rnd, int(gained)], np.int32).tobytes())
        f.write(np.ascontiguousarray(H, np.float64).tobytes())
        f.write(np.ascontiguousarray(ratio, np.float32).tobytes())
        f.write(np.ascontiguousarray(gq if gained else np.zeros((n, 3)), np.int32).tobytes())
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
    L = max(w, h)
    assert np.array_equal(take(np.int32, n), ori)
    got = take(np.int32, n * L).reshape(n, L)
    assert np.array_equal(got, seam), np.nonzero((got != seam).any(axis=1))[0][:10]
    assert np.array_equal(take(np.uint64, n), total)
    exp = cases.expected_render(name, gained)
    for si, s in enumerate(segs):
        rows, cols = s[4], s[5]
        canvas, cover = take(np.uint8, rows * cols * 3).reshape(rows, cols, 3), take(np.uint8, rows * cols).reshape(rows, cols)
        assert int((canvas != exp[si][0]).sum()) == 0 and int((cover != exp[si][1]).sum()) == 0, si
    assert at[0] == len(raw)
