"""CPU: the kernels of csrc/jpeg_encode.hip run on host threads (tests/jpeg_encode_emulated.cpp) and must write the host
codec's bytes -- sizes, streams, the negative size of a frame that does not fit, and nothing past a slot."""
import subprocess

import _emu_build as eb


def test_kernels_on_host_threads_equal_the_host_codec(tmp_path):
    exe = eb.build(tmp_path, "jpeg_encode.hip", "jpeg_encode_emulated.cpp", flags=eb.SANITIZE + ("-fno-sanitize-recover=all",))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-3000:]
    assert "count 1 of 2 ok" in r.stdout          # the case with a device count below the batch ran
