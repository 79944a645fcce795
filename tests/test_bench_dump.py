"""CPU: bench.py --dump-outputs keeps to its size budget -- the enhanced frames whole when they fit, else every frame at
one fixed seeded set of pixel positions -- and writes float arrays only."""
import importlib
import os
import types

import numpy as np
import torch


def _bench(monkeypatch):
    monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)     # bench.py sets its own at import: restored after the test
    return importlib.import_module("bench")


def _rig(F, H, W, S):
    g = torch.Generator().manual_seed(0)
    Fs = F // S
    pipes = [types.SimpleNamespace(work=torch.randint(0, 256, (Fs, H, W, 3), generator=g, dtype=torch.uint8),
                                   ratio=torch.rand((Fs,), generator=g), params=[(2 * i + 2, 3 * i + 1) for i in range(Fs)])
             for _ in range(S)]
    return types.SimpleNamespace(F=F, H=H, W=W, S=S, Fs=Fs, dev=torch.device("cpu"), pipes=pipes)


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}


def test_dump_whole_frames_when_they_fit(tmp_path, monkeypatch):
    bench = _bench(monkeypatch)
    rig = _rig(6, 9, 11, 3)
    bench.dump_outputs(rig, str(tmp_path))
    out = _load(tmp_path)
    assert set(out) == {"enhanced", "overlap_ratio", "aclahe_params"}
    assert out["enhanced"].dtype == np.float32 and out["overlap_ratio"].dtype == np.float32 and out["aclahe_params"].dtype == np.float64
    assert np.array_equal(out["enhanced"], torch.cat([p.work for p in rig.pipes]).numpy().astype(np.float32))
    assert np.array_equal(out["overlap_ratio"], torch.cat([p.ratio for p in rig.pipes]).numpy())
    assert out["aclahe_params"].shape == (6, 2) and out["aclahe_params"][1].tolist() == [4.0, 4.0]


def test_dump_samples_the_same_pixels_of_every_frame_over_budget(tmp_path, monkeypatch):
    bench = _bench(monkeypatch)
    monkeypatch.setattr(bench, "DUMP_FRAME_BYTES", 4 * 3 * 6 * 20)      # 20 pixels of each of the 6 frames
    rig = _rig(6, 9, 11, 2)
    bench.dump_outputs(rig, str(tmp_path / "a"))
    bench.dump_outputs(rig, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    pix = a["enhanced_pixel_index"]
    assert pix.dtype == np.float64 and pix.shape == (20,) and np.all(np.diff(pix) > 0) and pix.max() < 9 * 11
    frames = torch.cat([p.work for p in rig.pipes]).numpy().reshape(6, 9 * 11, 3)
    assert a["enhanced"].shape == (6, 20, 3) and np.array_equal(a["enhanced"], frames[:, pix.astype(np.int64)].astype(np.float32))
    for name in a:
        assert np.array_equal(a[name], b[name]), name
