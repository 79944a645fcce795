"""GPU: `videostrip --strip --strip-mode seam [--strip-gain] [--strip-seam-prior N]` writes the numpy mirror's strip
(tests/_strip_seam_mirror.py under the device's own transforms and gains) for the same key frames; a prior outside 0..4096 is
refused, as bad levels are."""
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import _strip_seam_mirror as mm
from uwimageproc_amd import Strip, synth
from uwimageproc_amd import videostrip as vs

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


def test_videostrip_seam(tmp_path, ctx):
    n, rows, cols = 8, 360, 640
    frames = synth.uw_stream(0, n, rows, cols, step_frac=0.1).astype(np.float64)
    gains = np.random.default_rng(6).uniform(0.85, 1.15, (n, 1, 1, 3))
    lst = _write_list(tmp_path, np.clip(np.floor(frames * gains + 0.5), 0, 255).astype(np.uint8))
    runs = {}
    for name, extra in (("seam", []), ("seam_gain", ["--strip-gain", "--strip-seam-prior", "256"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([os.path.join(BIN, "videostrip"), "--strip", "--strip-mode", "seam", *extra, "--png", "-k", "0", "-p", "0.7", lst, "out_"],
                           cwd=str(d), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (d, open(str(d / "out_videostrip_report.txt")).read().splitlines(), sorted(os.listdir(str(d))))
    (bd, brep, bfiles), (gd, grep, gfiles) = runs["seam"], runs["seam_gain"]
    assert brep == grep and bfiles == gfiles                      # the same key frames, segments and file names
    at = brep.index("ID\tFrame\tFilename\tOverlap\tBlur")
    keys = [l.split("\t")[2] for l in brep[at + 1:] if not l.startswith("Strip:")]
    kf = np.stack([_load_png(str(bd / k)) for k in keys])
    d = torch.from_numpy(kf).cuda()
    s = Strip(ctx, rows, cols, batch=1, max_frames=len(keys))
    for k in range(len(keys)):
        s.add(d[k:k + 1])
    segs = s.layout()
    assert segs[0].count >= 2 and len(segs) == len([f for f in bfiles if f.startswith("out_strip_")])
    t = s.transforms()
    stored = vs.resize_bgr(ctx, d).cpu().numpy()
    s.gains()
    gq = s.gain_values()["gq"]
    for run_dir, g, prior in ((bd, None, 1024), (gd, gq, 256)):
        seam, ori, _ = mm.seams(stored, t["G"], t["Ginv"], t["seg"], g, prior)
        for i, seg in enumerate(segs):
            assert np.array_equal(_load_png(str(run_dir / f"out_strip_{i:03d}.png")), mm.render(stored, t["Ginv"], tuple(seg), seam, ori, g)[0]), (g is not None, i)
    assert not np.array_equal(_load_png(str(bd / "out_strip_000.png")), s.render(0).cpu().numpy())        # not the default mode's strip
    assert not np.array_equal(_load_png(str(bd / "out_strip_000.png")), s.render(0, "last").cpu().numpy())
    s.close()


@pytest.mark.parametrize("prog,args", [("videostrip", ["--png"]), ("uwpipe", ["--png", "--keyframes"])])
@pytest.mark.parametrize("prior", ["-1", "4097", "12x", ""])
def test_bad_prior_is_refused(tmp_path, prog, args, prior):
    lst = _write_list(tmp_path, synth.uw_stream(0, 2, 270, 480, step_frac=0.1))
    d = tmp_path / "run"
    d.mkdir()
    r = subprocess.run([os.path.join(BIN, prog), *args, "--strip", "--strip-mode", "seam", "--strip-seam-prior", prior, lst, "out_"], cwd=str(d),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--strip-seam-prior 0..4096" in r.stdout
    assert not [f for f in os.listdir(str(d)) if f.startswith("out_strip_")]


def test_uwpipe_writes_a_seam_strip(tmp_path):
    lst = _write_list(tmp_path, synth.uw_stream(0, 4, 270, 480, step_frac=0.1))
    d = tmp_path / "run"
    d.mkdir()
    r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", "2", "--png", "--guard-s", "--keyframes", "-k", "0", "-p", "0.7", "--strip", "--strip-mode", "seam", lst, "out_"], cwd=str(d),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert [f for f in os.listdir(str(d)) if f.startswith("out_strip_")]
