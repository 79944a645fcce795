"""CPU: the kernels of csrc/png_encode.hip run on host threads (tests/png_encode_emulated.cpp, built with the address and
undefined-behaviour sanitizers) and must write the serial reference encoder's bytes -- sizes, streams, the negative size of a
frame that does not fit, nothing past a slot.  Every stream it leaves is then checked without this project's code: Pillow's
pixels, zlib's inflate against the numpy restatement of the filter rule, and the bound."""
import subprocess

import numpy as np

import _emu_build as eb
import _png_streams as ps


def test_kernels_on_host_threads_equal_the_reference_and_decode(tmp_path):
    exe = eb.build(tmp_path, "png_encode.hip", "png_encode_emulated.cpp", flags=eb.SANITIZE + ("-g", "-fno-sanitize-recover=undefined"), include=())
    out = tmp_path / "streams"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "count 1 of 2 ok" in r.stdout          # the case with a device count below the batch ran

    import uwimageproc_amd as uw
    lines = open(str(out / "manifest.txt")).read().split("\n")[:-1]
    assert len(lines) >= 6 * 8 * 2
    filters = set()
    for line in lines:
        name, raw, rows, cols, nc, filt = line.split()
        rows, cols, nc, filt = int(rows), int(cols), int(nc), int(filt)
        img = np.fromfile(str(out / (raw + ".raw")), dtype=np.uint8).reshape((rows, cols, nc) if nc == 3 else (rows, cols))
        stream = open(str(out / (name + ".png")), "rb").read()
        ps.check_stream(stream, img, filt, uw.png.bound(rows, cols, nc), uw.png.chunk_bytes())
        filters.add(filt)
    assert filters == {-1, 0, 1, 2, 3, 4}
