"""One step of every emulation test: cut the first anonymous namespace of a csrc/*.hip unit -- its kernels and its host sequence
-- into an include file, and build the stand-alone harness tests/<harness> over it with the host compiler.  The sanitizers, the
include directories beyond the cut's own and tests/, and the libraries are each module's own flags."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uwimageproc_amd", "csrc")
SANITIZE = ("-fsanitize=address,undefined",)


def build(d, unit, harness, inc="kernels.inc", flags=(), include=("include", "cli"), libs=()):
    """d: a directory (pathlib) for the cut and the program -> the program's path"""
    src = open(os.path.join(CSRC, unit)).read()
    end = "}  // namespace\n"
    a, b = src.index("namespace {"), src.index(end)
    open(str(d / inc), "w").write(src[a:b + len(end)])
    exe = str(d / "emu")
    dirs = [str(d), os.path.join(ROOT, "tests"), CSRC] + [os.path.join(ROOT, i) for i in include]
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-w", *flags, *[a for i in dirs for a in ("-I", i)],
                    os.path.join(ROOT, "tests", harness), "-o", exe, *libs], check=True, timeout=600)
    return exe
