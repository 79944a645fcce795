"""The overlap detector's keypoint cap on the CPU: oracle/uwip_oracle_overlap.c's detect() == the sort-based restatement of
the rule in _dense_frames.py, exactly, on frames with more candidates than UWIP_MAX_KEYPOINTS = 2048.  This pins the
checker before the device is compared with it (test_overlap_cap_gpu.py).

Measured with the restatement (candidates, then among them: >= the threshold, == the threshold, sharing the threshold's high
16 bits, strictly stronger than the threshold but past the raster cutoff):

| case       | frame                              | shape   | candidates | >= thr | == thr | bin16 | stronger, dropped |
|------------|------------------------------------|---------|------------|--------|--------|-------|-------------------|
| under      | period 7, jitter 60                | 360x640 | 1696       | -      | -      | -     | -                 |
| just_over  | period 10, jitter 60               | 360x640 | 2277       | 2048   | 1      | 15    | 0                 |
| over       | period 8, jitter 60                | 360x640 | 3627       | 2048   | 1      | 17    | 0                 |
| all_tied   | period 10, equal dots              | 360x640 | 2108       | 2108   | 2108   | 2108  | 0                 |
| tied       | period 8, equal dots               | 360x640 | 6708       | 3354   | 3354   | 3354  | 0                 |
| flat       | 90 everywhere                      | 360x640 | 0          | -      | -      | -     | -                 |
| small_tied | period 8, equal dots               | 240x320 | 2128       | 2063   | 999    | 1064  | 15                |
| b2047      | period 8, jitter 5, 1143 dots      | 240x320 | 2047       | -      | -      | -     | -                 |
| b2048      | the same, 1144 dots, last one dimmed | 240x320 | 2048     | -      | -      | -     | -                 |
| b2049      | the same, 1144 dots                | 240x320 | 2049       | 2048   | 1      | 47    | 0                 |

Mutations of detect() in a scratch copy of the oracle, and the cases of test_oracle_equals_restatement that fail on each
(not committed):
  bits[i] >= thr -> >                   : just_over, over, b2049 (one keypoint short); all_tied, tied, small_tied (the tie vanishes)
  no second radix pass, thr = prefix << 16 : just_over, over, small_tied, b2049 (the whole high-16 bin of the threshold passes)
  no nout < 2048 bound, return clamped  : all_tied, tied, small_tied (entries land behind the 2048 the caller owns: the guard
                                          zone of _dense_frames.oracle_detect)"""
import numpy as np
import pytest

import _dense_frames as df


@pytest.mark.parametrize("name", list(df.CASES))
def test_frame_bytes_are_pinned(name):
    fr = df.frame(name)
    assert fr.dtype == np.uint8 and fr.shape == ((360, 640) if name in df.LARGE else (240, 320))
    assert df.crc(fr) == df.CASES[name][1], hex(df.crc(fr))


def test_canvas_bytes_are_pinned():
    assert df.canvas().shape == (400, 700) and df.crc(df.canvas()) == df.CANVAS_CRC


def test_dot_profile_and_placement():
    """the generator's integer table and its centres: period / 2 + k * period, sigma 1.6, +-8 px"""
    assert df._G[0] == 4096 and df._G[16] == round(4096 * np.exp(-64 / (2 * 1.6 ** 2))) and np.all(np.diff(df._G[:15]) < 0)
    one = df.lattice(40, 40, 40, 0, 0).astype(int) - 60           # a single dot at (20, 20)
    assert one[20, 20] == 120 and one[20, 21] == one[21, 20] == one[19, 20] == round(120 * np.exp(-1 / (2 * 1.6 ** 2)))
    assert one[20, 28] == 0 and one[20, 29] == 0 and np.array_equal(one, one.T) and np.array_equal(one[1:, 1:], one[:0:-1, :0:-1])
    odd = df.lattice(21, 21, 7, 0, 0).astype(int)                 # centres 3.5, 10.5, 17.5: symmetric about pixel pairs
    assert odd[3, 3] == odd[3, 4] == odd[4, 4] == odd[10, 11] and odd[3, 3] > odd[3, 2] == odd[3, 5]


def test_select_is_the_rule_on_a_hand_made_list():
    """select() and facts() on lists small enough to check by eye: 2051 candidates in raster order (yi), cap 2048"""
    c = np.zeros(2051, df.CAND)
    c["yi"] = np.arange(2051)
    c["response"] = 2.0
    c["response"][5] = 1.0                         # one weak candidate, 2050 tied: the 2048-th largest is 2.0 ...
    s = df.select(c)
    assert len(s) == 2048 and np.all(s["response"] == 2.0) and 5 not in s["yi"] and s["yi"][-1] == 2048    # ... 2049, 2050 cut off
    two = int(np.float32(2.0).view(np.uint32))
    assert df.facts(c) == dict(total=2051, kept=2048, thr=two, ge=2050, eq=2050, bin16=2050, stronger_dropped=0)
    c["response"][[7, 2050]] = 3.0                 # a stronger one early is kept, a stronger one past the cutoff is dropped
    assert df.facts(c) == dict(total=2051, kept=2048, thr=two, ge=2050, eq=2048, bin16=2048, stronger_dropped=1)
    s = df.select(c)
    assert len(s) == 2048 and 7 in s["yi"] and s["yi"][-1] == 2048
    c["response"][:3] = [1.5, 1.25, 1.75]          # 2047 at or above 2.0: the threshold drops to 1.75, nothing is tied
    assert df.facts(c) == dict(total=2051, kept=2048, thr=int(np.float32(1.75).view(np.uint32)), ge=2048, eq=1, bin16=1,
                               stronger_dropped=0)
    assert np.array_equal(df.select(c)["yi"], np.setdiff1d(np.arange(2051), [0, 1, 5]))
    assert df.select(c[:2048]) is not None and len(df.select(c[:2048])) == 2048 and len(df.select(c[:100])) == 100


@pytest.mark.parametrize("name", list(df.CASES))
def test_oracle_equals_restatement(orc, name):
    c = df.case_candidates(name)
    df.assert_reaches_its_path(name, df.facts(c))
    kps, desc, _ = df.oracle_detect(orc, df.frame(name))         # asserts that nothing lands behind entry 2047
    df.assert_equals_restatement(kps, c)
    assert len(desc) == len(kps) == min(len(c), df.MAXKP)
    k2, d2, _ = orc.detect_describe(df.frame(name))              # the wrapper the GPU tests compare with gives the same
    assert k2.tobytes() == kps.tobytes() and np.array_equal(d2, desc)
    # the refined position lies within one pixel of the lattice position, as the candidate rule demands
    assert np.all(np.abs(kps["x"] - kps["xi"]) <= 1.0) and np.all(np.abs(kps["y"] - kps["yi"]) <= 1.0)


@pytest.mark.parametrize("name,flags", [("over", dict(upright=True)), ("just_over", dict(relative_threshold=True))])
def test_oracle_equals_restatement_under_flags(orc, name, flags):
    """upright touches no candidate; the relative threshold is the fixed one at a contrast factor >= 0.5"""
    kps, _, kc = df.oracle_detect(orc, df.frame(name), **flags)
    assert kc >= 0.5 and df.threshold(kc, flags.get("relative_threshold", False)) == df.DTHRESH
    df.assert_equals_restatement(kps, df.case_candidates(name))
    assert df.threshold(0.25, True) == np.float32(0.001) * np.float32(0.25) and df.threshold(0.25, False) == df.DTHRESH


@pytest.mark.parametrize("dx,dy", [(13, 5), (40, 21)])
def test_crops_are_capped_and_resize_is_the_identity(orc, dx, dy):
    """what the matcher test on the device relies on: both crops exceed the cap, and the 640-wide resize leaves them alone"""
    for o in ((0, 0), (dx, dy)):
        g, c = df.crop(*o), df.crop_candidates(*o)
        assert np.array_equal(orc.resize_gray(df.gray_to_bgr(g)), g)
        assert len(c) > df.MAXKP + 1024
        df.assert_equals_restatement(df.oracle_detect(orc, g)[0], c)
