"""GPU: `videostrip --strip --strip-gain` writes strips that differ from the ungained run's and equal Strip.render(gain=True)
for the same key frames; the flag without --strip is refused."""
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


def test_videostrip_strip_gain_flag(tmp_path, ctx):
    n, rows, cols = 12, 360, 640
    frames = synth.uw_stream(0, n, rows, cols, step_frac=0.1).astype(np.float64)
    gains = np.random.default_rng(6).uniform(0.85, 1.15, (n, 1, 1, 3))          # the level steps the compensation is for
    frames = np.clip(np.floor(frames * gains + 0.5), 0, 255).astype(np.uint8)
    paths = []
    for i in range(n):
        paths.append(str(tmp_path / f"f{i:03d}.png"))
        Image.fromarray(np.ascontiguousarray(frames[i][..., ::-1])).save(paths[-1])
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    runs = {}
    for name, extra in (("plain", ["--strip"]), ("gain", ["--strip", "--strip-gain"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([os.path.join(BIN, "videostrip"), *extra, "--png", "-k", "0", "-p", "0.7", lst, "out_"], cwd=str(d),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (d, open(str(d / "out_videostrip_report.txt")).read().splitlines(), sorted(os.listdir(str(d))))
    (pd, prep, pfiles), (gd, grep, gfiles) = runs["plain"], runs["gain"]
    assert prep == grep and pfiles == gfiles                      # the same key frames, the same segments, the same file names
    strips = [f for f in gfiles if f.startswith("out_strip_")]
    assert strips
    for f in pfiles:
        same = open(str(pd / f), "rb").read() == open(str(gd / f), "rb").read()
        assert same != (f in strips) or f == "out_videostrip_report.txt", f
    at = prep.index("ID\tFrame\tFilename\tOverlap\tBlur")
    keys = [l.split("\t")[2] for l in prep[at + 1:] if not l.startswith("Strip:")]
    s = Strip(ctx, rows, cols, batch=1, max_frames=len(keys))
    for k in keys:
        s.add(torch.from_numpy(_load_png(str(pd / k))[None]).cuda())
    segs = s.layout()
    assert len(segs) == len(strips) and segs[0].count >= 2
    s.gains()
    for i in range(len(segs)):
        assert np.array_equal(_load_png(str(gd / f"out_strip_{i:03d}.png")), s.render(i, gain=True).cpu().numpy())
        assert np.array_equal(_load_png(str(pd / f"out_strip_{i:03d}.png")), s.render(i).cpu().numpy())
    s.close()


@pytest.mark.parametrize("prog,args", [("videostrip", ["--png"]), ("uwpipe", ["--png", "--keyframes"])])
def test_strip_gain_without_strip_is_refused(tmp_path, prog, args):
    frames = synth.uw_stream(0, 2, 270, 480, step_frac=0.1)
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / f"f{i}.png"))
        Image.fromarray(np.ascontiguousarray(frames[i][..., ::-1])).save(paths[-1])
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    d = tmp_path / "run"
    d.mkdir()
    r = subprocess.run([os.path.join(BIN, prog), *args, "--strip-gain", lst, "out_"], cwd=str(d), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--strip-gain is refused without --strip" in r.stdout
    assert not [f for f in os.listdir(str(d)) if f.startswith("out_strip_")]
