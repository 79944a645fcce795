"""GPU parity of the overlap detector's keypoint cap: frames with more candidates than UWIP_MAX_KEYPOINTS = 2048, so that the
radix-select chain of csrc/overlap_detect.hip (the histogram filled in k_ov_extrema, k_ov_sel_pick<0>, k_ov_sel_hist<1>,
k_ov_sel_pick<1>, k_ov_count, k_ov_scan_chunks, k_ov_compact) has to choose.  Every comparison is device == oracle, exact, on
keypoints, descriptors and counts; test_overlap_cap_oracle.py pins the oracle to a sort-based restatement of the rule and
holds the table of what each frame exercises.  Each test asserts through that restatement that its frames still reach the
path they are there for."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dense_frames as df
from uwimageproc_amd import videostrip as vs

pytestmark = pytest.mark.gpu

MIXED = ("under", "tied", "flat", "over", "just_over", "all_tied")       # different outcomes side by side in one batch


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(names):
    return _dev(np.stack([df.frame(n) for n in names])[..., None])       # [F, h, w, 1]: 8UC1 planes at the working size


_expected = {}


def _oracle(orc, name, **flags):
    """oracle keypoints / descriptors of a named case, computed once and left unchanged"""
    key = (name,) + tuple(sorted(flags.items()))
    if key not in _expected:
        kps, desc, _ = orc.detect_describe(df.frame(name), **flags)
        kps.setflags(write=False); desc.setflags(write=False)
        _expected[key] = (kps, desc)
    return _expected[key]


def _assert_features_equal(got, exp, what=""):
    (kps, desc), (ek, ed) = got, exp
    assert len(kps) == len(ek) and len(desc) == len(ed), (what, len(kps), len(ek))
    for fld in ("xi", "yi", "level"):
        assert np.array_equal(kps[fld], ek[fld]), (what, fld)
    for fld in ("x", "y", "response", "co", "si"):
        assert np.array_equal(kps[fld], ek[fld]), (what, fld)
    assert np.array_equal(desc, ed), what


def _assert_case(orc, name, got, what="", **flags):
    """the frame reaches its path (restatement), the oracle keeps what the rule keeps, and the device equals the oracle"""
    c = df.case_candidates(name)
    df.assert_reaches_its_path(name, df.facts(c))
    exp = _oracle(orc, name, **flags)
    df.assert_equals_restatement(exp[0], c)
    assert len(got[0]) == min(len(c), df.MAXKP), (what, name)
    _assert_features_equal(got, exp, (what, name))


@pytest.mark.parametrize("name", list(df.CASES))
def test_each_case_alone(ctx, orc, name):
    assert df.crc(df.frame(name)) == df.CASES[name][1]
    f = vs.Features(ctx, 1)
    f.detect(_batch([name]))
    _assert_case(orc, name, f.download(0))
    f.close()


def test_mixed_batch_and_its_reverse(ctx, orc):
    """six 360 x 640 frames in one detect call: under the cap, a large tie, empty, far over, just over, all tied -- the
    selection state of a frame (sel, selhist, counts) next to that of frames with other outcomes; then the reversed order
    into the same feature set"""
    f = vs.Features(ctx, len(MIXED))
    for order in (MIXED, MIXED[::-1]):
        f.detect(_batch(order))
        for s, name in enumerate(order):
            _assert_case(orc, name, f.download(s), ("slot", s))
    f.close()


def test_boundary_batch(ctx, orc):
    """240 x 320: the tie that drops stronger candidates next to frames with exactly 2047, 2048 and 2049 candidates"""
    assert [len(df.case_candidates(n)) for n in df.SMALL[1:]] == [2047, 2048, 2049]
    f = vs.Features(ctx, len(df.SMALL))
    f.detect(_batch(df.SMALL))
    for s, name in enumerate(df.SMALL):
        _assert_case(orc, name, f.download(s), ("slot", s))
    f.close()


def test_workspace_reuse_in_one_slot(ctx, orc):
    """over the cap, under it, empty, over it again, each into slot 0: the selection workspaces survive between the calls and
    may carry nothing over"""
    f = vs.Features(ctx, 1)
    for step, name in enumerate(("over", "under", "flat", "over", "tied", "just_over")):
        f.detect(_batch([name]))
        got = f.download(0)
        if name == "flat":
            assert len(got[0]) == 0
        _assert_case(orc, name, got, ("step", step))
    f.close()


@pytest.mark.parametrize("name,flags", [("over", dict(upright=True)), ("just_over", dict(relative_threshold=True))])
def test_flags_on_a_capped_frame(ctx, orc, name, flags):
    """upright: the same keypoints, (co, si) = (1, 0); relative threshold: at a contrast factor >= 0.5 the threshold is the
    fixed one.  Device == oracle under the same flag."""
    f = vs.Features(ctx, 1)
    f.detect(_batch([name]), **flags)
    got = f.download(0)
    _assert_case(orc, name, got, **flags)
    if flags.get("upright"):
        assert np.all(got[0]["co"] == 1.0) and np.all(got[0]["si"] == 0.0)
        assert not np.array_equal(got[1], _oracle(orc, name)[1])
    else:
        assert orc.detect_describe(df.frame(name), **flags)[2] >= 0.5
        _assert_features_equal(got, _oracle(orc, name))
    f.close()


@pytest.mark.parametrize("dx,dy,ratio", [(13, 5, 0.94077), (40, 21, 0.81239)])
def test_selected_keypoints_through_matcher_and_geometry(ctx, orc, dx, dy, ratio):
    """2048 keypoints that the detector itself selected, on both sides, through kNN, ratio test, RANSAC and overlapArea: two
    crops of one canvas, so the true homography is the translation (dx, dy).  Measured on the oracle: ratio 0.94077 / 0.81239
    (the truth to float precision), 1899 / 1705 inliers."""
    key, obj = df.crop(0, 0), df.crop(dx, dy)
    kb, ob = df.gray_to_bgr(key), df.gray_to_bgr(obj)
    assert df.crc(df.canvas()) == df.CANVAS_CRC
    for g, b, o in ((key, kb, (0, 0)), (obj, ob, (dx, dy))):
        assert np.array_equal(orc.resize_gray(b), g)                     # the resize at 640 columns is the identity
        assert len(df.crop_candidates(*o)) > df.MAXKP + 1024
    f = vs.Features(ctx, 2)
    f.detect(_dev(np.stack([kb, ob])))
    feats = [f.download(s) for s in range(2)]
    for s, (g, o) in enumerate(((key, (0, 0)), (obj, (dx, dy)))):
        ek, ed, _ = orc.detect_describe(g)
        df.assert_equals_restatement(ek, df.crop_candidates(*o))
        _assert_features_equal(feats[s], (ek, ed), ("slot", s))
    res = vs.match_pairs(ctx, f, f, [1], [0], 640, 480, seed=1, want_matches=True)
    idx, dist, info = res["idx"].cpu().numpy()[0], res["dist"].cpu().numpy()[0], res["info"].cpu().numpy()[0]
    (kq, dq), (kt, dt) = feats[1], feats[0]
    eidx, edist = orc.match_knn2(dq, dt)
    assert np.array_equal(idx, eidx) and np.array_equal(dist, edist)
    gq, gt = orc.ratio_test(eidx, edist, len(kt))
    assert info[0] == info[1] == df.MAXKP and info[2] == len(gq)
    ninl, H = orc.find_homography(kq["x"][gq], kq["y"][gq], kt["x"][gt], kt["y"][gt], 640, 360, seed=1)
    assert info[3] == ninl
    Hg = res["H"].cpu().numpy()[0]
    assert np.abs(Hg - H).max() <= 1e-9 * max(1.0, np.abs(H).max())
    er, ecnt = orc.overlapArea(H, 640, 480)
    assert info[4] == ecnt
    r = float(res["ratio"].cpu()[0])
    assert abs(r - er) <= 1e-6
    er2, einfo, _ = orc.calcOverlap(kb, ob, 640, 480, seed=1)
    assert abs(r - er2) <= 1e-6 and list(info[:5]) == einfo
    truth, _ = orc.overlapArea([[1, 0, dx], [0, 1, dy], [0, 0, 1]], 640, 480)
    assert abs(truth - ratio) < 1e-4
    assert abs(r - truth) <= 0.01, (r, truth)                           # the stated acceptance of the overlap ratio
    assert info[3] >= 1500                                              # a matcher fed a wrong keypoint set falls far below
    f.close()


def test_nothing_is_written_past_the_cap(ctx, orc):
    """slot 1 of a two-slot feature set holds a known pattern; the frame with 6708 candidates (3354 of them tied at the
    threshold) goes into slot 0: entry 2048 of slot 0 would be entry 0 of slot 1"""
    c = df.case_candidates("tied")
    assert len(c) > 2 * df.MAXKP and df.facts(c)["ge"] > df.MAXKP
    rng = np.random.default_rng(5)
    K = df.MAXKP
    kps = np.zeros(K, vs.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(8, 632, K), rng.uniform(8, 352, K)
    kps["response"] = rng.uniform(0.001, 0.1, K)
    kps["level"], kps["xi"], kps["yi"] = rng.integers(0, 4, K), rng.integers(8, 632, K), rng.integers(8, 352, K)
    ang = rng.uniform(0, 2 * np.pi, K)
    kps["co"], kps["si"] = np.cos(ang), np.sin(ang)
    desc = rng.integers(0, 256, (K, 64), dtype=np.uint8)
    desc[:, 60] &= 0x3f; desc[:, 61:] = 0
    f = vs.Features(ctx, 2)
    ctx.call("uwip_features_upload", f._h, 1, 360, 640, C.c_void_p(kps.ctypes.data), C.c_void_p(desc.ctypes.data), K)
    f.detect(_batch(["tied"]), first_slot=0)
    _assert_case(orc, "tied", f.download(0))
    k1, d1 = f.download(1)
    assert len(k1) == K and k1.tobytes() == kps.tobytes() and d1.tobytes() == desc.tobytes()
    # the matcher's unpacked copy of slot 1 is intact as well: every row finds itself at distance 0, as the oracle says
    res = vs.match_pairs(ctx, f, f, [1], [1], 640, 480, seed=1, want_matches=True)
    eidx, edist = orc.match_knn2(desc, desc)
    assert np.array_equal(res["idx"].cpu().numpy()[0], eidx) and np.array_equal(res["dist"].cpu().numpy()[0], edist)
    assert np.all(edist[:, 0] == 0)
    f.close()
