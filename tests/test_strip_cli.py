"""GPU: `videostrip --strip` writes one blended image per chained segment of the exported key frames and a "Strip:" line per
segment after the report's table; its pixels are Strip.render's for the same key frames, and without the flag the report and
the files are what they are with it, minus the strip."""
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from uwimageproc_amd import Strip, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")


def _load_png(path):
    return np.asarray(Image.open(path).convert("RGB"))[..., ::-1].copy()


def test_videostrip_strip_flag(tmp_path, ctx):
    n, rows, cols = 12, 360, 640
    frames = synth.uw_stream(0, n, rows, cols, step_frac=0.1)
    paths = []
    for i in range(n):
        paths.append(str(tmp_path / f"f{i:03d}.png"))
        Image.fromarray(np.ascontiguousarray(frames[i][..., ::-1])).save(paths[-1])
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    runs = {}
    for name, extra in (("plain", []), ("strip", ["--strip"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([os.path.join(BIN, "videostrip"), *extra, "--png", "-k", "0", "-p", "0.7", lst, "out_"], cwd=str(d),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (d, open(str(d / "out_videostrip_report.txt")).read().splitlines(), sorted(os.listdir(str(d))))
    (pd, prep, pfiles), (sd, srep, sfiles) = runs["plain"], runs["strip"]
    # without the flag: no strip file, no Strip line; with it: the same report and files, plus the strip
    assert not [f for f in pfiles if f.startswith("out_strip_")] and not [l for l in prep if l.startswith("Strip:")]
    lines = [l for l in srep if l.startswith("Strip:")]
    assert [l for l in srep if not l.startswith("Strip:")] == prep and srep[-len(lines):] == lines
    assert [f for f in sfiles if not f.startswith("out_strip_")] == pfiles
    for f in pfiles:
        if f == "out_videostrip_report.txt":          # compared line by line above: it differs by the Strip lines alone
            continue
        assert open(str(pd / f), "rb").read() == open(str(sd / f), "rb").read(), f
    at = prep.index("ID\tFrame\tFilename\tOverlap\tBlur")
    keys = [l.split("\t")[2] for l in prep[at + 1:]]
    assert len(keys) >= 3
    # the same key frames through the Python object
    s = Strip(ctx, rows, cols, batch=1, max_frames=len(keys))
    for k in keys:
        s.add(torch.from_numpy(_load_png(str(pd / k))[None]).cuda())
    segs = s.layout()
    assert len(lines) == len(segs) == len([f for f in sfiles if f.startswith("out_strip_")])
    for i, g in enumerate(segs):
        fn = f"out_strip_{i:03d}.png"
        assert lines[i] == f"Strip:\t{fn}\t{g.first}\t{g.count}\t{g.cols} x {g.rows}"
        assert np.array_equal(_load_png(str(sd / fn)), s.render(i).cpu().numpy())
    assert segs[0].count >= 2 and segs[0].cols > cols         # the key frames did chain into a strip wider than a frame
    s.close()


def test_uwpipe_keyframes_strip_flag(tmp_path, ctx):
    """`uwpipe --keyframes --strip`: the strip of the ENHANCED key frames the program writes, with the Strip lines behind the
    key-frame report's table; without the flag the same files and reports; with --streams it is refused with a message."""
    n, rows, cols, B = 12, 270, 480, 5
    frames = synth.uw_stream(0, n, rows, cols, step_frac=0.1)
    paths = []
    for i in range(n):
        paths.append(str(tmp_path / f"f{i:03d}.png"))
        Image.fromarray(np.ascontiguousarray(frames[i][..., ::-1])).save(paths[-1])
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    runs = {}
    for name, extra in (("plain", []), ("strip", ["--strip", "--strip-mode", "last"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B), "--png", "--guard-s", "--keyframes", "-k", "0", "-p", "0.7", *extra, lst, "out_"],
                           cwd=str(d), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (d, open(str(d / "out_videostrip_report.txt")).read().splitlines(), sorted(os.listdir(str(d))))
    (pd, prep, pfiles), (sd, srep, sfiles) = runs["plain"], runs["strip"]
    assert not [f for f in pfiles if f.startswith("out_strip_")] and not [l for l in prep if l.startswith("Strip:")]
    lines = [l for l in srep if l.startswith("Strip:")]
    assert lines and [l for l in srep if not l.startswith("Strip:")] == prep and srep[-len(lines):] == lines
    assert [f for f in sfiles if not f.startswith("out_strip_")] == pfiles
    for f in pfiles:
        if f != "out_videostrip_report.txt":
            assert open(str(pd / f), "rb").read() == open(str(sd / f), "rb").read(), f
    at = prep.index("ID\tFrame\tFilename\tOverlap\tBlur")
    keys = [l.split("\t")[2] for l in prep[at + 1:]]
    assert len(keys) >= 3
    s = Strip(ctx, rows, cols, batch=1, max_frames=len(keys))
    for k in keys:
        s.add(torch.from_numpy(_load_png(str(pd / k))[None]).cuda())
    segs = s.layout()
    assert len(lines) == len(segs)
    for i, g in enumerate(segs):
        fn = f"out_strip_{i:03d}.png"
        assert lines[i] == f"Strip:\t{fn}\t{g.first}\t{g.count}\t{g.cols} x {g.rows}"
        assert np.array_equal(_load_png(str(sd / fn)), s.render(i, "last").cpu().numpy())
    s.close()
    d = tmp_path / "refused"
    d.mkdir()
    r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B), "--png", "--keyframes", "--streams", "--strip", lst, "out_"], cwd=str(d),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--strip is refused with --streams" in r.stdout
    assert not [f for f in os.listdir(str(d)) if f.startswith("out_strip_")]
