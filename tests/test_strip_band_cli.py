"""GPU: `videostrip --strip --strip-mode multiband [--strip-gain] [--strip-levels N]` writes the pixels of
Strip.render(mode="multiband") for the same key frames; an unknown mode and levels outside 1..4 are refused."""
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


def _write_list(tmp_path, frames):
    paths = []
    for i in range(len(frames)):
        paths.append(str(tmp_path / f"f{i:03d}.png"))
        Image.fromarray(np.ascontiguousarray(frames[i][..., ::-1])).save(paths[-1])
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return lst


def test_videostrip_multiband(tmp_path, ctx):
    n, rows, cols = 10, 360, 640
    frames = synth.uw_stream(0, n, rows, cols, step_frac=0.1).astype(np.float64)
    gains = np.random.default_rng(6).uniform(0.85, 1.15, (n, 1, 1, 3))
    lst = _write_list(tmp_path, np.clip(np.floor(frames * gains + 0.5), 0, 255).astype(np.uint8))
    runs = {}
    for name, extra in (("band", []), ("band_gain", ["--strip-gain", "--strip-levels", "2"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([os.path.join(BIN, "videostrip"), "--strip", "--strip-mode", "multiband", *extra, "--png", "-k", "0", "-p", "0.7", lst, "out_"],
                           cwd=str(d), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (d, open(str(d / "out_videostrip_report.txt")).read().splitlines(), sorted(os.listdir(str(d))))
    (bd, brep, bfiles), (gd, grep, gfiles) = runs["band"], runs["band_gain"]
    assert brep == grep and bfiles == gfiles                      # the same key frames, segments and file names
    at = brep.index("ID\tFrame\tFilename\tOverlap\tBlur")
    keys = [l.split("\t")[2] for l in brep[at + 1:] if not l.startswith("Strip:")]
    s = Strip(ctx, rows, cols, batch=1, max_frames=len(keys))
    for k in keys:
        s.add(torch.from_numpy(_load_png(str(bd / k))[None]).cuda())
    segs = s.layout()
    assert segs[0].count >= 2 and len(segs) == len([f for f in bfiles if f.startswith("out_strip_")])
    s.gains()
    s.bands()
    for i in range(len(segs)):
        assert np.array_equal(_load_png(str(bd / f"out_strip_{i:03d}.png")), s.render(i, "multiband").cpu().numpy())
    assert not np.array_equal(_load_png(str(bd / "out_strip_000.png")), s.render(0).cpu().numpy())      # not the default mode's strip
    s.bands(levels=2)
    for i in range(len(segs)):
        assert np.array_equal(_load_png(str(gd / f"out_strip_{i:03d}.png")), s.render(i, "multiband", gain=True).cpu().numpy())
    assert not np.array_equal(_load_png(str(gd / "out_strip_000.png")), s.render(0, "multiband").cpu().numpy())
    s.close()


@pytest.mark.parametrize("prog,args", [("videostrip", ["--png"]), ("uwpipe", ["--png", "--keyframes"])])
@pytest.mark.parametrize("extra", [["--strip-mode", "median"], ["--strip-mode", "multiband", "--strip-levels", "5"]])
def test_unknown_mode_and_levels_are_refused(tmp_path, prog, args, extra):
    lst = _write_list(tmp_path, synth.uw_stream(0, 2, 270, 480, step_frac=0.1))
    d = tmp_path / "run"
    d.mkdir()
    r = subprocess.run([os.path.join(BIN, prog), *args, "--strip", *extra, lst, "out_"], cwd=str(d), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--strip-mode: feather, first, last or multiband" in r.stdout
    assert not [f for f in os.listdir(str(d)) if f.startswith("out_strip_")]
