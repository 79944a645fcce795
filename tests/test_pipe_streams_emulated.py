"""CPU: the kernels of csrc/pipe_streams.hip -- blank, select, gather, carry, table, pack -- run on host threads
(tests/pipe_streams_emulated.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers) and must
give what a serial restatement gives: the list of emitted frames from random ring contents, the gathered and carried pixels,
the offsets of the streams (a negative size in the middle is skipped), the blob byte for byte, and nothing outside any buffer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernels_on_host_threads_equal_the_serial_restatement(tmp_path):
    src = open(os.path.join(ROOT, "uwimageproc_amd", "csrc", "pipe_streams.hip")).read()
    a, end = src.index("namespace {"), "}  // namespace\n"
    b = src.index(end)
    open(str(tmp_path / "kernels.inc"), "w").write(src[a:b + len(end)])
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(tmp_path), "-I", os.path.join(ROOT, "tests"), "-I", os.path.join(ROOT, "uwimageproc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pipe_streams_emulated.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[-4]) >= 50
