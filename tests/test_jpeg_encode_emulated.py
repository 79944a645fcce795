"""CPU: the kernels of csrc/jpeg_encode.hip run on host threads (tests/jpeg_encode_emulated.cpp) and must write the host
codec's bytes -- sizes, streams, the negative size of a frame that does not fit, and nothing past a slot."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernels_on_host_threads_equal_the_host_codec(tmp_path):
    src = open(os.path.join(ROOT, "uwimageproc_amd", "csrc", "jpeg_encode.hip")).read()
    a, end = src.index("namespace {"), "}  // namespace\n"
    b = src.index(end)
    open(str(tmp_path / "kernels.inc"), "w").write(src[a:b + len(end)])
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-w", "-I", str(tmp_path), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "cli"), "-I", os.path.join(ROOT, "uwimageproc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "jpeg_encode_emulated.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout[-3000:]
