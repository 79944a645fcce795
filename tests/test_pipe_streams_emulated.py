"""CPU: the kernels of csrc/pipe_streams.hip -- blank, select, gather, carry, table, pack -- run on host threads
(tests/pipe_streams_emulated.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers) and must
give what a serial restatement gives: the list of emitted frames from random ring contents, the gathered and carried pixels,
the offsets of the streams (a negative size in the middle is skipped), the blob byte for byte, and nothing outside any buffer."""
import subprocess

import _emu_build as eb


def test_kernels_on_host_threads_equal_the_serial_restatement(tmp_path):
    exe = eb.build(tmp_path, "pipe_streams.hip", "pipe_streams_emulated.cpp", flags=eb.SANITIZE + ("-g", "-fno-sanitize-recover=undefined"), include=())
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[-4]) >= 50
