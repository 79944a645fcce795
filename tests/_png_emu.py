"""The emulation harness of the PNG decoder for the two test modules that drive it: tests/png_decode_emulated.cpp, a stand-alone
program built with the address and undefined-behaviour sanitizers, runs the kernels of csrc/png_decode.hip on host threads.
The inflate machinery (csrc/png_inflate.hpp) is included by the harness as it stands; the kernels and the host planning are cut
out of the .hip file (tests/_emu_build.py): its first anonymous namespace, which holds the unit's host sequence as well."""
import os
import subprocess

import _emu_build as eb

FIELDS = (("status", 4), ("host", 6), ("equal", 8), ("clean", 10), ("accepted", 12), ("serial", 14), ("maxdist", 16))


class Emu:
    def __init__(self, d):
        self.d, self.count = d, 0
        self.exe = eb.build(d, "png_decode.hip", "png_decode_emulated.cpp", "kernels_pngd.inc", eb.SANITIZE + ("-fno-sanitize-recover=all",),
                            libs=("-lz",))

    def __call__(self, cases):
        """cases: [(name, stream, channels, segmented, chunk_bytes)] -> {(name, segmented, chunk_bytes): dict of the printed fields}"""
        lines = []
        for name, stream, ch, seg, cb in cases:
            p = str(self.d / (name + ".png"))
            open(p, "wb").write(stream)
            lines.append(f"{p} {seg} {ch} {cb}")
        # the emulation waits at barriers most of the time: four processes side by side, each with a share of the list
        procs = []
        for i in range(4):
            self.count += 1
            lst = str(self.d / f"list{self.count}.txt")
            open(lst, "w").write("\n".join(lines[i::4]) + "\n")
            procs.append(subprocess.Popen([self.exe, lst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        stdout = ""
        for pr in procs:
            o, e = pr.communicate(timeout=1500)
            assert pr.returncode == 0, (o + e)[-3000:]
            stdout += o
        out = {}
        for ln in stdout.splitlines():
            w = ln.split()
            v = {k: int(w[i]) for k, i in FIELDS}
            n = int(w[18])
            v["starts"] = [int(x) for x in w[19:19 + n]]
            v["tried"], v["valid"] = int(w[20 + n]), int(w[22 + n])
            out[(os.path.basename(w[0])[:-4], int(w[1]), int(w[2]))] = v
        assert len(out) == len(cases), stdout[-3000:]
        return out

    def batch(self, streams, ch, rows, cols, seg, cb):
        """the streams in one call -> per frame the dict of the printed fields"""
        paths = []
        for i, stream in enumerate(streams):
            paths.append(str(self.d / f"batch{i}.png"))
            open(paths[-1], "wb").write(stream)
        lst = str(self.d / "batch.txt")
        open(lst, "w").write(f"batch {seg} {ch} {cb} {rows} {cols} " + " ".join(paths) + "\n")
        r = subprocess.run([self.exe, lst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out = [{k: int(w[i]) for k, i in (("status", 6), ("single", 8), ("same", 10), ("clean", 12), ("accepted", 14), ("serial", 16))}
               for w in map(str.split, r.stdout.splitlines())]
        assert len(out) == len(streams), r.stdout[-3000:]
        return out

    def own(self, arr, filt=-1):
        """The library's own encoder (its serial host form) on arr [H, W, 3] BGR or [H, W, 1] grey."""
        H, W, nc = arr.shape
        raw, png = str(self.d / "own.raw"), str(self.d / "own.png")
        arr.tofile(raw)
        subprocess.run([self.exe, "--encode", raw, str(H), str(W), str(nc), str(filt), png], check=True, timeout=300)
        return open(png, "rb").read()
