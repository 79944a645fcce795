"""The four CLIs (cli/*.cpp over include/uwip.hpp): image I/O round trip on CPU; on the GPU each
tool's output is compared with the oracle chained the same way."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _knee_mirror as knee_mirror   # the scipy mirror of functions.py:49-93 (a checker: lives with the tests)
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cli", "bin")
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from uwimageproc_amd import synth  # noqa: E402


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cli")], check=True)


def _save_png(path, bgr):
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path)


def _load_png(path):
    return np.asarray(Image.open(path).convert("RGB"))[..., ::-1].copy()


def test_cli_builds_and_help_runs_without_gpu(tmp_path):
    _build()
    for tool in ("histretch", "aclahe", "bgdehaze", "videostrip", "uwpipe"):
        r = subprocess.run([os.path.join(BIN, tool), "--help"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "usage" in r.stdout
    # -cuda=0 is refused: there is no CPU implementation in this build
    p = str(tmp_path / "a.png")
    _save_png(p, synth.uw_frame(0, 48, 64))
    r = subprocess.run([os.path.join(BIN, "histretch"), "-c=RGB", "-cuda=0", p, str(tmp_path / "b.png")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "no CPU implementation" in r.stdout


REAL = os.path.join(ROOT, "tests", "golden", "real")


def _write_mjpeg_avi(path, jpegs, fps, width, height):
    """A minimal RIFF AVI with one Motion-JPEG video stream (what `ffmpeg -c:v mjpeg` writes, without the index)."""
    import struct
    def chunk(tag, body):
        return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    def lst(kind, body):
        return chunk(b"LIST", kind + body)
    avih = struct.pack("<14I", int(1e6 / fps), 0, 0, 0x10, len(jpegs), 0, 1, 0, width, height, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII", 0, 0, 0, 0, 1, int(fps), 0, len(jpegs), 0, 0xFFFFFFFF, 0) + struct.pack("<4h", 0, 0, width, height)
    strf = struct.pack("<IiiHHIIiiII", 40, width, height, 1, 24, 0x47504A4D, width * height * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi = lst(b"movi", b"".join(chunk(b"00dc", j) for j in jpegs))
    body = b"AVI " + hdrl + movi
    open(path, "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_jpeg_codec_against_pillow(tmp_path):
    """cli/jpeg.hpp (libjpeg's islow IDCT, fancy upsampling, fixed-point colour; baseline encoder with the Annex K
    tables at cv::imwrite's quality 95): the decoder returns, bit for bit, what Pillow's libjpeg returns for the
    reference's four JPEG files; the encoder's files decode identically in Pillow and in the decoder, and on a photograph
    to exactly what Pillow's own encoder (quality 95, 4:2:0) gives."""
    import io
    _build()
    conv = os.path.join(BIN, "imgconv")
    out = str(tmp_path / "o.png")
    for n in ("in_BUL_T1A_0028.jpg", "in_BUL_T1A_0209.jpg", "in_PIS_T1A_259.jpg", "ref_result_BUL_T1A_0209.jpg"):
        r = subprocess.run([conv, os.path.join(REAL, n), out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout
        assert np.array_equal(_load_png(out), np.asarray(Image.open(os.path.join(REAL, n)).convert("RGB"))[..., ::-1]), n
    photo = np.ascontiguousarray(np.asarray(Image.open(os.path.join(REAL, "in_BUL_T1A_0028.jpg")).convert("RGB"))[:533, :801, ::-1])
    for name, img in (("photo", photo), ("synthetic", synth.uw_stream(0, 1, 270, 483)[0])):
        a, j, b = str(tmp_path / "a.png"), str(tmp_path / "a.jpg"), str(tmp_path / "b.png")
        _save_png(a, img)
        assert subprocess.run([conv, a, j], capture_output=True, timeout=120).returncode == 0
        via_pillow = np.asarray(Image.open(j).convert("RGB"))[..., ::-1]
        assert subprocess.run([conv, j, b], capture_output=True, timeout=120).returncode == 0
        assert np.array_equal(_load_png(b), via_pillow), name                      # our decoder == libjpeg on our stream
        err = np.abs(via_pillow.astype(int) - img.astype(int))
        assert err.mean() < 3.0, (name, err.mean())                               # quality 95
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(buf, format="JPEG", quality=95, subsampling=2)
        theirs = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[..., ::-1]
        d = np.abs(via_pillow.astype(int) - theirs.astype(int))
        if name == "photo":
            assert d.max() == 0                 # same coefficients as libjpeg-turbo's encoder
        else:
            assert (d != 0).mean() < 0.05       # libjpeg-turbo's reciprocal quantiser differs from IJG's division on noise
    # grey: 1-component stream
    g = np.asarray(Image.open(os.path.join(REAL, "in_aclahe_crowd.png")).convert("L"))
    a, j = str(tmp_path / "g.png"), str(tmp_path / "g.jpg")
    Image.fromarray(g).save(a)
    assert subprocess.run([conv, a, j, "grey"], capture_output=True, timeout=120).returncode == 0
    im = Image.open(j)
    assert im.mode == "L" and np.abs(np.asarray(im).astype(int) - g.astype(int)).mean() < 2.0
    # a grey stream whose SOF keeps the 2x2 factors of a colour mode: one block per MCU all the same (T.81 A.2.2), libjpeg's
    # pixels; and Pillow's own grey stream with that one byte of SOF rewritten
    import _jpeg_forge_cases as fc
    forged = dict(fc.equality_grey(37, 53))["g22_37x53_ri0"].stream
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(g[:53, :37])).save(buf, format="JPEG", quality=90)
    own = buf.getvalue()
    sof = own.index(b"\xff\xc0")
    assert own[sof + 9] == 1 and own[sof + 11] == 0x11
    patched = own[:sof + 11] + b"\x22" + own[sof + 12:]
    for name, s in (("forged", forged), ("patched", patched)):
        open(j, "wb").write(s)
        r = subprocess.run([conv, j, out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stdout)
        assert np.array_equal(_load_png(out), np.asarray(Image.open(io.BytesIO(s)).convert("RGB"))[..., ::-1]), name
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(patched))), np.asarray(Image.open(io.BytesIO(own))))


def test_jpeg_header_is_the_one_pillow_writes(tmp_path):
    """The header writer of csrc/jpeg_tables.hpp (shared by the host and the device encoder) against something outside the
    project: the quantisation tables of an `imgconv` stream are the ones Pillow's libjpeg writes at quality 95, and SOI..SOS
    is 623 bytes for a colour stream, 328 for a grey one."""
    import io
    _build()
    conv = os.path.join(BIN, "imgconv")
    colour = synth.uw_stream(0, 1, 17, 33)[0]
    for name, img, hdr in (("colour", colour, 623), ("grey", np.ascontiguousarray(colour[:16, :16, 1]), 328)):
        a, j = str(tmp_path / (name + ".png")), str(tmp_path / (name + ".jpg"))
        pil = Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img[..., ::-1]))
        pil.save(a)
        assert subprocess.run([conv, a, j] + (["grey"] if img.ndim == 2 else []), capture_output=True, timeout=120).returncode == 0
        buf = io.BytesIO()
        pil.save(buf, format="JPEG", quality=95, subsampling=2)
        ours, theirs = Image.open(j), Image.open(io.BytesIO(buf.getvalue()))
        assert ours.size == theirs.size and ours.mode == theirs.mode == ("L" if img.ndim == 2 else "RGB")
        assert {k: list(v) for k, v in ours.quantization.items()} == {k: list(v) for k, v in theirs.quantization.items()}, name
        s = open(j, "rb").read()
        sos = s.index(b"\xff\xda")
        assert sos + 2 + ((s[sos + 2] << 8) | s[sos + 3]) == hdr, name


@pytest.mark.gpu
def test_histretch_cli_config0_640x480_png(tmp_path, orc):
    """BASELINE config 0: histretch on one 640x480 PNG (here through the HIP path)."""
    _build()
    img = synth.uw_frame(0, 480, 640)
    a, b = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    _save_png(a, img)
    r = subprocess.run([os.path.join(BIN, "histretch"), "-c=RGB", "-cuda=1", "-time=1", a, b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Execution Time GPU" in r.stdout and "Applying 3 histretch" in r.stdout
    exp, _ = orc.histretch(img, "RGB")
    assert np.array_equal(_load_png(b), exp)
    # the default -c=r is a no-op and reports the unknown letter (B-1)
    r = subprocess.run([os.path.join(BIN, "histretch"), a, b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "not recognized, skipping" in r.stdout
    assert np.array_equal(_load_png(b), img)


@pytest.mark.gpu
def test_aclahe_and_bgdehaze_cli(tmp_path, orc):
    import dehaze_oracle as dz
    from uwimageproc_amd import aclahe
    _build()
    img = synth.uw_stream(0, 1, 135, 240)[0]
    a, b = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    _save_png(a, img)
    r = subprocess.run([os.path.join(BIN, "aclahe"), a, b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    v = orc.bgr_to_v(img)
    bs, cl = knee_mirror.select_parameters(orc.sweep(v))
    assert f"Block size: {bs}" in r.stdout and f"Clip limit: {cl}" in r.stdout
    assert np.array_equal(_load_png(b), orc.hsv_replace_v(img, orc.clahe(v, float(cl), bs, bs)))
    rows = [l for l in r.stdout.splitlines() if l.count(" ") >= 50]
    assert len(rows) == 5                                             # the 5 x 51 entropy table
    r = subprocess.run([os.path.join(BIN, "bgdehaze"), "--rc", "-w", "15", a, b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    expf = dz.RC_correction(dz.normalize_input(img), 15) * 255.0
    exp = dz.to_u8(expf / 255.0)
    diff = np.abs(_load_png(b).astype(int) - exp.astype(int))
    # cv2.imwrite rounds to nearest even, and the linearly mapped red channel (<= 256 distinct values) sits on exact .5 ties
    # routinely: the bytes may differ by one level exactly where the float value is within 1e-6 of a tie, nowhere else
    assert diff.max() <= 1 and np.all(np.abs(np.abs(expf - np.floor(expf)) - 0.5)[diff != 0] < 1e-6)
    # --histretch chains the stretch in the same run: same bytes as the two tools one after the other
    c, d = str(tmp_path / "dz.png"), str(tmp_path / "dzhs.png")
    for cmd in ([os.path.join(BIN, "bgdehaze"), "-w", "15", a, c], [os.path.join(BIN, "histretch"), "-c=RGB", c, d],
                [os.path.join(BIN, "bgdehaze"), "-w", "15", "--histretch", "RGB", a, b]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(_load_png(b), _load_png(d))


@pytest.mark.gpu
def test_videostrip_cli_selector_and_report(tmp_path, orc):
    """Selector loop (main.cpp:300-394) on a 14-frame 640x480 stream, checked against the same loop
    driven by the oracle's calcOverlap / calcBlur."""
    _build()
    n, k, p = 14, 2, 0.7
    frames = synth.uw_stream(0, n, 480, 640, step_frac=0.05)
    paths = []
    for i in range(n):
        paths.append(str(tmp_path / f"f{i:03d}.png"))
        _save_png(paths[-1], frames[i])
    lst = str(tmp_path / "frames.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    prefix = str(tmp_path / "out_")
    r = subprocess.run([os.path.join(BIN, "videostrip"), "-k", str(k), "-p", str(p), "--png", lst, prefix], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rep = open(prefix + "videostrip_report.txt").read().splitlines()
    hdr = rep.index("ID\tFrame\tFilename\tOverlap\tBlur")
    rows = [l.split("\t") for l in rep[hdr + 1:]]
    # the same loop on the oracle
    exp = [("0", "0")]
    key, nxt, read = frames[0], 1, 1
    while nxt < n:
        f = frames[nxt]; nxt += 1; read += 1
        ov, _, _ = orc.calcOverlap(key, f, 640, 480, seed=1)
        if ov == -2.0:
            ov = 0.41
        if ov <= p:
            best, bestn, bf = orc.calcBlur(f), nxt - 1, f
            eof = False
            for _ in range(k):
                if nxt >= n:
                    eof = True
                    break
                g = frames[nxt]; nxt += 1; read += 1
                b = orc.calcBlur(g)
                if b > best:
                    best, bestn, bf = b, read, g
            key = bf
            exp.append((str(len(exp)), str(bestn)))
            if eof:
                break
    assert [(r_[0], r_[1]) for r_ in rows] == exp, (rows, exp)
    # --gpus N: per-slice extraction on N contexts (both on this box's one GPU), decision chain with look-ahead on GPU 0:
    # the same report, value for value
    for g in (1, 3):
        prefix_g = str(tmp_path / f"g{g}_")
        r = subprocess.run([os.path.join(BIN, "videostrip"), "-k", str(k), "-p", str(p), "--png", "-g", str(g), lst, prefix_g],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        rep_g = open(prefix_g + "videostrip_report.txt").read().splitlines()
        rows_g = [l.split("\t") for l in rep_g[rep_g.index("ID\tFrame\tFilename\tOverlap\tBlur") + 1:]]
        assert [(a[0], a[1], a[3], a[4]) for a in rows_g] == [(a[0], a[1], a[3], a[4]) for a in rows], (g, rows_g, rows)
        for i in range(len(rows)):
            assert np.array_equal(_load_png(prefix_g + f"{i:04d}.png"), _load_png(prefix + f"{i:04d}.png"))
    # the Python mirror of the loop (uwimageproc_amd.videostrip.select_keyframes) agrees with the CLI
    import torch
    import uwimageproc_amd as uw
    from uwimageproc_amd import videostrip as vs
    c = uw.Context(0)
    got = vs.select_keyframes(c, [torch.from_numpy(f).cuda() for f in frames], minOverlap=p, kWindow=k)
    assert [(str(a), str(b)) for a, b, _, _ in got] == exp
    # the multi-GPU form (uwimageproc_amd.selector, SURVEY 8e option 1): features and blur extracted per slice -- here the
    # two slices a 2-rank job would take, one after the other -- then the decision chain on rank 0's GPU with speculative
    # look-ahead: the exported IDs equal the single-GPU CLI's, and so do overlap and blur of every row
    from uwimageproc_amd import selector, sharding
    be = selector.GpuBackend(c, (640, 480), seed=1, lookahead=5)
    recs = []
    for r in range(2):
        a, b = sharding.frame_slice(n, r, 2)
        recs += be.extract(frames[a:b])
    rows2 = selector.chain(recs, be.overlaps, p, k, lookahead=5)
    assert [(str(a), str(b)) for a, b, _, _ in rows2] == exp
    for (_, _, ov2, bl2), (_, _, ov1, bl1) in zip(rows2, got):
        assert abs(ov2 - ov1) <= 1e-6 and abs(bl2 - bl1) <= 1e-6
    rows3 = selector.select_distributed(be, lambda i: frames[i], n, 0, 1, p, k, batch=4, lookahead=3)
    assert [(a, b) for a, b, _, _ in rows3] == [(a, b) for a, b, _, _ in rows2]
    be.close()
    c.close()
    assert len(rows) >= 2 and os.path.exists(prefix + "0000.png") and os.path.exists(prefix + f"{len(rows)-1:04d}.png")
    assert np.array_equal(_load_png(prefix + "0000.png"), frames[0])
    # the same stream as a Motion-JPEG .avi, key frames written as .jpg like the reference (main.cpp:294,377): the frames the
    # tool sees are the DECODED JPEGs, so the expectation is the same loop on those
    import io
    jpegs, dec = [], []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(buf, format="JPEG", quality=92, subsampling=2)
        jpegs.append(buf.getvalue())
        dec.append(np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[..., ::-1]))
    avi = str(tmp_path / "clip.avi")
    _write_mjpeg_avi(avi, jpegs, 25.0, 640, 480)
    prefix2 = str(tmp_path / "avi_")
    r = subprocess.run([os.path.join(BIN, "videostrip"), "-k", str(k), "-p", str(p), avi, prefix2], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rep = open(prefix2 + "videostrip_report.txt").read().splitlines()
    rows2 = [l.split("\t") for l in rep[rep.index("ID\tFrame\tFilename\tOverlap\tBlur") + 1:]]
    exp2 = [("0", "0")]
    key, nxt, read = dec[0], 1, 1
    while nxt < n:
        f = dec[nxt]; nxt += 1; read += 1
        ov, _, _ = orc.calcOverlap(key, f, 640, 480, seed=1)
        if ov == -2.0:
            ov = 0.41
        if ov <= p:
            best, bestn, bf = orc.calcBlur(f), nxt - 1, f
            eof = False
            for _ in range(k):
                if nxt >= n:
                    eof = True
                    break
                g = dec[nxt]; nxt += 1; read += 1
                b = orc.calcBlur(g)
                if b > best:
                    best, bestn, bf = b, read, g
            key = bf
            exp2.append((str(len(exp2)), str(bestn)))
            if eof:
                break
    assert [(r_[0], r_[1]) for r_ in rows2] == exp2, (rows2, exp2)
    first = np.asarray(Image.open(prefix2 + "0000.jpg").convert("RGB"))[..., ::-1]
    assert first.shape == (480, 640, 3) and np.abs(first.astype(int) - dec[0].astype(int)).mean() < 3.0


@pytest.mark.gpu
def test_reference_signature_shims(tmp_path, orc):
    """uw::ref::{calcOverlap, calcBlur, overlapArea, imgChannelStretch, getHistogram}: the reference's names, argument
    order, defaults and globals on a default context (include/uwip.hpp), against the oracle."""
    _build()
    frames = synth.uw_stream(0, 2, 480, 640, step_frac=0.05)
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    _save_png(a, frames[0]); _save_png(b, frames[1])
    r = subprocess.run([os.path.join(BIN, "refshim_check"), a, b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = r.stdout.split()
    got = {tok[i]: tok[i + 1] for i in range(0, 10, 2)}
    ov, _, _ = orc.calcOverlap(frames[0], frames[1], 640, 480, seed=1)
    assert abs(float(got["overlap"]) - ov) <= 1e-5
    assert abs(float(got["blur"]) - orc.calcBlur(frames[1])) <= 1e-3
    assert abs(float(got["area"]) - 1.0) <= 1e-5
    st = frames[1].copy()
    orc.imgChannelStretch(st[:, :, 0], 2, 98)
    assert int(got["stretch"]) == int(st.astype(np.uint64).sum())
    assert float(got["hist0"]) == float((st[:, :, 0] == 0).sum())
    assert tok[-2:] == ["1", "1"]


@pytest.mark.gpu
def test_bgdehaze_cli_on_the_references_photograph(tmp_path):
    """The reference's own use: main.py reads img/BUL_T1A_0209.jpg and writes result/BUL_T1A_0209.jpg (w = 15).  The CLI
    does the same from the same .jpg to a .jpg; against the file the reference's authors saved: the bounds of
    tests/test_real_images.py (first-index tie rule: mean |diff| < 7 levels, correlation > 0.99) plus one more JPEG coding."""
    _build()
    out = str(tmp_path / "out.jpg")
    r = subprocess.run([os.path.join(BIN, "bgdehaze"), "-w", "15", os.path.join(REAL, "in_BUL_T1A_0209.jpg"), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.asarray(Image.open(out).convert("RGB")).astype(int)
    ref = np.asarray(Image.open(os.path.join(REAL, "ref_result_BUL_T1A_0209.jpg")).convert("RGB")).astype(int)
    assert got.shape == ref.shape
    assert np.abs(got - ref).mean() < 7.5
    assert min(np.corrcoef(got[:, :, c].ravel(), ref[:, :, c].ravel())[0, 1] for c in range(3)) > 0.99


def _asan_tool(tmp_path, name, source):
    """A host-only tool over cli/*.hpp built with AddressSanitizer + UBSan (the codecs read untrusted files)."""
    src, exe = str(tmp_path / (name + ".cpp")), str(tmp_path / name)
    open(src, "w").write(source)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "cli"), "-I" + os.path.join(ROOT, "uwimageproc_amd", "csrc"), src, "-o", exe, "-lz"],
                   check=True, timeout=300)
    return exe


def test_hostile_jpeg_and_avi_are_refused_not_crashed(tmp_path):
    """cli/jpeg.hpp and cli/avi.hpp read arbitrary files: over-subscribed Huffman counts, table selectors beyond 3,
    segments shorter than their fields, truncation anywhere and random corruption must end in decode() == false (or a
    decoded image), never in an out-of-bounds access -- checked under ASan/UBSan."""
    import io
    import struct
    conv = _asan_tool(tmp_path, "imgconv_asan", open(os.path.join(ROOT, "cli", "imgconv.cpp")).read())
    env = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:exitcode=99")
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(synth.uw_stream(0, 1, 64, 96)[0][..., ::-1])).save(buf, format="JPEG", quality=90)
    good = buf.getvalue()
    out = str(tmp_path / "o.ppm")

    def run(data, tag):
        p = str(tmp_path / "h.jpg")
        open(p, "wb").write(data)
        r = subprocess.run([conv, p, out], capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode in (0, 1), (tag, r.returncode, r.stderr[-2000:])
        return r.returncode

    assert run(good, "good") == 0

    def seg(marker):
        i = good.index(bytes([0xFF, marker]))
        return i, i + 2 + struct.unpack(">H", good[i + 2:i + 4])[0]

    # (1) DHT whose counts over-subscribe the code space: bits[1] = 5
    a, b = seg(0xC4)
    bad = bytearray(good[a:b]); bad[5] = 5
    assert run(good[:a] + bytes(bad) + good[b:], "dht oversubscribed") == 1
    # (2) SOS table selectors 15/15
    a, b = seg(0xDA)
    bad = bytearray(good[a:b]); bad[6] = 0xFF
    assert run(good[:a] + bytes(bad) + good[b:], "sos selectors") == 1
    # (3) SOF / DRI / SOS whose length field is shorter than the fields read from them, at the end of the file
    a, b = seg(0xC0)
    assert run(good[:a] + b"\xff\xc0\x00\x02", "short sof") == 1
    assert run(good[:a] + b"\xff\xc0\x00\x08" + good[a + 4:a + 10], "sof without components") == 1
    assert run(good[:a] + b"\xff\xdd\x00\x02", "short dri") == 1
    a2, _ = seg(0xDA)
    assert run(good[:a2] + b"\xff\xda\x00\x03\x03", "short sos") == 1
    # (4) truncation at every 7th byte, and seeded random corruption of header and entropy-coded bytes
    for n in range(2, len(good), 7):
        run(good[:n], f"truncated at {n}")
    rng = np.random.default_rng(5)
    for k in range(300):
        d = bytearray(good)
        for _ in range(int(rng.integers(1, 6))):
            d[int(rng.integers(2, len(d)))] = int(rng.integers(0, 256))
        run(bytes(d), f"corrupt {k}")

    # AVI: LIST chunks nested 100 000 deep (12 bytes a level) and a child chunk that overruns its parent LIST
    avi_tool = _asan_tool(tmp_path, "avi_asan", '#include "avi.hpp"\nint main(int c, char **v) { avi::Reader r; bool ok = r.open(v[1]); '
                          'imgio::Image im; for (size_t i = 0; i < r.count(); ++i) r.read(i, im); std::printf("%zu\\n", r.count()); return ok ? 0 : 1; }\n')
    depth = 100000
    body = b"AVI "
    for i in range(depth):
        body += b"LIST" + struct.pack("<I", 4 + 12 * (depth - 1 - i)) + b"rec "
    p = str(tmp_path / "deep.avi")
    open(p, "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)
    r = subprocess.run([avi_tool, p], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 1, r.stderr[-2000:]
    inner = b"00dc" + struct.pack("<I", 4000) + good[:64]           # claims 4000 bytes inside a 76-byte LIST
    body = b"AVI " + b"LIST" + struct.pack("<I", 4 + len(inner)) + b"movi" + inner + b"\0" * 8000
    open(p, "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)
    r = subprocess.run([avi_tool, p], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 1 and r.stdout.strip() == "0", (r.stdout, r.stderr[-2000:])


@pytest.mark.gpu
def test_copier_from_cpp():
    """uw::Copier (include/uwip.hpp over uwip_copier_*): batches uploaded one ahead, stretched, downloaded by ticket from a
    C++ program equal the synchronous path's bytes."""
    _build()
    r = subprocess.run([os.path.join(BIN, "copier_check"), "3", "270", "480", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("copier ok"), r.stdout + r.stderr


@pytest.mark.gpu
def test_uwpipe_cli_whole_chain_over_the_c_pipe(tmp_path, orc):
    """cli/uwpipe.cpp: the four tools as one program over uwip_pipe_step_host -- 5 frames in batches of 2 (the last batch
    padded), the reference's rules (no switch given).  Enhanced frames and the TSV rows equal what the Python caller of the
    same C entry gives for the same batching; frame 1's row equals the oracle's calcOverlap of the written frames."""
    import torch
    from uwimageproc_amd.pipeline import FramePipe
    _build()
    n, B, H, W = 5, 2, 270, 480
    frames = synth.uw_stream(0, n, H, W)
    paths = []
    for i in range(n):
        paths.append(str(tmp_path / f"f{i:03d}.png"))
        _save_png(paths[-1], frames[i])
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    prefix = str(tmp_path / "out_")
    r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B), "--png", lst, prefix], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l.split("\t") for l in open(prefix + "uwpipe_report.txt").read().splitlines() if l[:1].isdigit()]
    assert [int(x[0]) for x in rows] == list(range(n))
    pipe = FramePipe(0, B, H, W)
    exp_out, exp_ratio, exp_par = [], [], []
    for k in range((n + B - 1) // B):
        idx = [min(k * B + j, n - 1) for j in range(B)]
        out, ratio = pipe.run(torch.from_numpy(frames[idx]).cuda())
        torch.cuda.synchronize()
        exp_out += list(out.cpu().numpy()); exp_ratio += list(ratio.cpu().numpy()); exp_par += list(pipe.params)
    pipe.close()
    got = [_load_png(f"{prefix}{i:04d}.png") for i in range(n)]
    for i in range(n):
        assert np.array_equal(got[i], exp_out[i]), i
        assert abs(float(rows[i][2]) - float(exp_ratio[i])) <= 1e-5 * max(1.0, abs(float(exp_ratio[i]))), (i, rows[i])
        assert (int(rows[i][3]), int(rows[i][4])) == tuple(exp_par[i]), i
    er, _, _ = orc.calcOverlap(got[0], got[1], W, H, seed=1)
    assert abs(float(rows[1][2]) - er) <= 1e-5
    # the same frames as a Motion-JPEG .avi with the three opt-in switches: the tool sees the DECODED JPEGs, so the expectation is
    # the Python caller of the same C entry on those, with the same flags (guard_s, min6; relative threshold via the config)
    import io
    import ctypes as C
    jpegs, dec = [], []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(buf, format="JPEG", quality=92, subsampling=2)
        jpegs.append(buf.getvalue())
        dec.append(np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[..., ::-1]))
    dec = np.stack(dec)
    avi = str(tmp_path / "clip.avi")
    _write_mjpeg_avi(avi, jpegs, 25.0, W, H)
    prefix2 = str(tmp_path / "avi_")
    r = subprocess.run([os.path.join(BIN, "uwpipe"), "-b", str(B), "--png", "--guard-s", "--min6", "--relative-threshold", avi, prefix2],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows2 = [l.split("\t") for l in open(prefix2 + "uwpipe_report.txt").read().splitlines() if l[:1].isdigit()]
    pipe = FramePipe(0, B, H, W, guard_s=True, min6=True)
    pipe._cfg.detect_flags = 16                               # UWIP_OVERLAP_RELATIVE_THRESHOLD
    pipe._l.uwip_pipe_destroy(pipe._p); pipe._create()
    for k in range((n + B - 1) // B):
        idx = [min(k * B + j, n - 1) for j in range(B)]
        out, ratio = pipe.run(torch.from_numpy(dec[idx]).cuda())
        torch.cuda.synchronize()
        for j in range(B):
            i = k * B + j
            if i < n:
                assert np.array_equal(_load_png(f"{prefix2}{i:04d}.png"), out[j].cpu().numpy()), i
                assert abs(float(rows2[i][2]) - float(ratio[j])) <= 1e-5 * max(1.0, abs(float(ratio[j]))), (i, rows2[i])
    pipe.close()
