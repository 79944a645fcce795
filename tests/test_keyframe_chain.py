"""CPU: the pipe's key-frame chain (csrc/kf_chain.hpp, the code k_kf_chain runs on the device) with its batch / round
scheme, driven on the host by uwip_keyframe_chain_host, equals the reference's selector loop (main.cpp:284-394 as
selector.chain writes it) row for row, and never needs more fallback rounds than the documented bound."""
import ctypes as C
import math
import random

import numpy as np
import pytest

from uwimageproc_amd import selector
from uwimageproc_amd._native import KeyframeConfig, KeyframeRow, lib
from uwimageproc_amd.pipeline import keyframe_chain_host, keyframe_config


def _bound(F, D, k):
    s = k + 1 if k > 0 else min(D, F - 1) + 1
    return (F - 1) // s + 1


def _check(ov, blur, n, batch, minOverlap, kWindow, D):
    recs = [(None, None, float(blur[i]), i) for i in range(n)]
    exp = selector.chain(recs, lambda key, objs: [ov[key[3]][o[3]] for o in objs], minOverlap, kWindow,
                         lookahead=random.choice([1, 3, 8]))
    calls = []

    def overlap(k, f):
        calls.append((k, f))
        return ov[k][f]

    got, rounds = keyframe_chain_host(overlap, lambda f: blur[f], n, batch, minOverlap=minOverlap, kWindow=kWindow, lookback=D)
    assert [(r[0], r[1]) for r in got] == [(e[0], e[1]) for e in exp], (n, batch, minOverlap, kWindow, D, got, exp)
    for g, e in zip(got, exp):
        assert g[3] == pytest.approx(e[2], abs=1e-6) and g[4] == e[3]
    # the index column names the key frame: a trigger's Frame is its index, a window frame's is its index + 1
    for g in got[1:]:
        assert g[1] in (g[2], g[2] + 1) and blur[g[2]] == pytest.approx(g[4], abs=1e-6)
    assert got[0] == (0, 0, 0, 0.0, 0.0)
    assert len(rounds) == -(-n // batch)
    assert max(rounds) <= _bound(batch, D, kWindow), (rounds, batch, D, kWindow)
    assert all(0 <= k < n and 0 <= f < n for k, f in calls)
    return rounds


def _f32(x):
    return float(np.float32(x))


def _pattern(rng, n, kind):
    blur = [rng.choice([rng.random() * 100, float(rng.randint(0, 3))]) for _ in range(n)]   # ties: the strict > rule
    ov = [[0.0] * n for _ in range(n)]
    p_trig = {"dense": 0.8, "sparse": 0.1, "none": 0.0, "mixed": rng.random()}[kind]
    for k in range(n):
        for f in range(n):
            u = rng.random()
            if u < p_trig * 0.3:
                ov[k][f] = -2.0                               # no homography: counts as 0.41
            elif u < p_trig:
                ov[k][f] = rng.choice([rng.random() * 0.7, 0.4, 0.41, 0.5])
            else:
                ov[k][f] = 0.7 + 0.3 * rng.random()
    # the device works in float32, as the reference does (currOverlap, minOverlap, the blur values): the oracle gets the
    # same values
    return [[_f32(v) for v in row] for row in ov], [_f32(b) for b in blur]


def test_chain_matches_reference_random():
    rng = random.Random(1234)
    random.seed(99)
    seen_rounds = 0
    for it in range(2500):
        n = rng.randint(1, 40)
        batch = rng.choice([1, 2, 3, 5, 8, 13, n, n + 3])
        kWindow = rng.choice([0, 1, 2, 3, 11, 50])                 # 50 > F: windows cross several batches
        D = rng.choice([1, 2, 4, 8, 100])
        # not exactly 0.41: there the reference's float compare (0.41f <= 0.41f) and selector.chain's double one differ
        minOverlap = _f32(rng.choice([0.4, 0.5, 0.7, 1.0, -3.0, 0.415, 0.405]))
        ov, blur = _pattern(rng, n, rng.choice(["dense", "sparse", "none", "mixed"]))
        seen_rounds += sum(_check(ov, blur, n, batch, minOverlap, kWindow, D))
    assert seen_rounds > 0          # the fallback rounds were exercised


@pytest.mark.parametrize("spacing", [1, 2, 3, 5, 7, 12, 13])
@pytest.mark.parametrize("batch", [4, 8, 16])
def test_trigger_at_every_spacing(spacing, batch):
    n = 60
    blur = [float((i * 37) % 11) for i in range(n)]
    for kWindow in (0, 1, 2, 11):
        for D in (1, 2, 8):
            # frame f triggers against any key when f is a multiple of `spacing`
            ov = [[(0.1 if f % spacing == 0 else 0.9) for f in range(n)] for _ in range(n)]
            _check(ov, blur, n, batch, 0.4, kWindow, D)
            ov2 = [[(-2.0 if f % spacing == 0 else 0.9) for f in range(n)] for _ in range(n)]
            _check(ov2, blur, n, batch, _f32(0.415), kWindow, D)       # -2.0 -> 0.41 <= 0.415
            rows, _ = keyframe_chain_host(lambda k, f: ov2[k][f], lambda f: blur[f], n, batch, minOverlap=0.405, kWindow=kWindow,
                                          lookback=D)
            assert len(rows) == 1                                 # 0.41 > 0.405: -2.0 is OVERLAP_MIN + 0.01, not minOverlap + 0.01


def test_end_of_stream_inside_a_window():
    n, batch = 10, 4
    blur = [1.0, 2.0, 3.0, 9.0, 4.0, 5.0, 6.0, 7.0, 8.0, 2.0]
    ov = [[0.1 if f == 7 else 0.9 for f in range(n)] for _ in range(n)]
    rows, _ = keyframe_chain_host(lambda k, f: ov[k][f], lambda f: blur[f], n, batch, minOverlap=0.4, kWindow=11, lookback=1)
    # frame 7 triggers, the window holds 8 and 9 when the stream ends: the best so far (8, read count 9) is reported
    assert rows == [(0, 0, 0, 0.0, 0.0), (1, 9, 8, pytest.approx(0.1), 8.0)]


def test_slow_stream_needs_fallback_rounds():
    # no trigger for long runs: after a key change inside a batch, frames further than D from the key need a fallback round
    n, batch = 64, 16
    blur = [float(i % 5) for i in range(n)]
    ov = [[0.1 if f in (5, 30, 41) else 0.9 for f in range(n)] for _ in range(n)]
    rounds = _check(ov, blur, n, batch, 0.4, 0, 1)
    assert sum(rounds) > 0


def test_config_default_and_bound():
    kc = keyframe_config()
    assert kc.minOverlap == pytest.approx(0.4) and kc.kWindow == 11 and kc.lookback >= 1 and kc.max_rows == 4096
    l = lib()
    for F in (1, 2, 7, 64):
        for k in (0, 1, 11):
            for D in (1, 2, 8):
                c = keyframe_config(kWindow=k, lookback=D)
                assert l.uwip_keyframe_max_rounds(C.byref(c), F) == _bound(F, D, k)


def test_bad_configurations_and_null_handles():
    l = lib()
    assert l.uwip_keyframe_config_default(None) != 0
    for bad in (dict(kWindow=-1), dict(lookback=0), dict(max_rows=0), dict(minOverlap=math.nan)):
        c = keyframe_config(**bad)
        assert l.uwip_keyframe_max_rounds(C.byref(c), 8) == -1
        with pytest.raises(Exception):
            keyframe_chain_host(lambda k, f: 0.9, lambda f: 1.0, 8, 4, **bad)
    c = keyframe_config()
    assert l.uwip_keyframe_max_rounds(C.byref(c), 0) == -1
    assert l.uwip_pipe_keyframe_chain(None, C.byref(c)) != 0
    assert l.uwip_pipe_end_of_stream(None, 1) != 0
    n = C.c_int(0)
    assert l.uwip_pipe_keyframes(None, (KeyframeRow * 1)(), 1, C.byref(n)) != 0
    with pytest.raises(Exception):
        keyframe_chain_host(lambda k, f: 0.9, lambda f: 1.0, 8, 0)      # batch 0
    assert C.sizeof(KeyframeRow) == 32 and C.sizeof(KeyframeConfig) == 16
