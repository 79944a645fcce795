"""The forged streams of the JPEG decoder tests (tests/_jpeg_forge.py writes them), shared by the CPU tests (emulated kernels
and host decoder) and the GPU tests.  Every stream of an `equality_*` group is inside the amplitude bound of the forge, so
Pillow's decode is its reference; the bad streams and their twins state their own expectation."""
import functools
import itertools

import numpy as np

import _jpeg_forge as jf

SIZES = [(37, 53), (16, 16), (1, 1)]            # W, H
F420, F422, F444 = [(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)]
GREY_FACTORS = [(1, 1), (2, 2), (2, 1), (1, 2)]
# seeds of the interval-1 streams of restart_streams(), chosen so that an interval ends in a stuffed 0xFF before its RSTn
RST_SEEDS = {"420": 2, "422": 4, "444": 2}


def device_eligible():
    """Every (h, v) x 3 with factors 1..2 that the device decodes (include/uwip.h): no component sampled 1x2 against the
    largest factors (hmax / h == 1 and vmax / v == 2: HOST_ONLY), at most 10 blocks per MCU (all 2x2 has 12: BAD_STREAM)."""
    out = []
    for fs in itertools.product([(1, 1), (2, 1), (1, 2), (2, 2)], repeat=3):
        hmax, vmax = max(h for h, _ in fs), max(v for _, v in fs)
        if any(hmax // h == 1 and vmax // v == 2 for h, v in fs) or sum(h * v for h, v in fs) > 10:
            continue
        out.append(list(fs))
    return out


def _name(fs):
    return "".join(f"{h}{v}" for h, v in fs)


@functools.lru_cache(None)
def equality_colour(W, H):
    """[(name, Forged)]: every device-eligible combination with restart interval 0 and 1."""
    return [(f"c{_name(fs)}_{W}x{H}_ri{ri}", jf.forge(W, H, fs, ri=ri, seed=100 * n + ri))
            for n, fs in enumerate(device_eligible()) for ri in (0, 1)]


@functools.lru_cache(None)
def equality_grey(W, H):
    """[(name, Forged)]: one component with each pair of SOF factors and restart interval 0, 1 and 5.  The same seed for the
    four factor pairs: they are one stream but for the SOF byte, and must decode alike."""
    return [(f"g{h}{v}_{W}x{H}_ri{ri}", jf.forge(W, H, [(h, v)], ri=ri, seed=7 + ri)) for h, v in GREY_FACTORS for ri in (0, 1, 5)]


GREY_FACTORS_TO_4 = [(4, 3), (3, 1), (1, 4)]


@functools.lru_cache(None)
def equality_grey_to_4():
    """[(name, Forged)] at 37x53: one component whose SOF factors no three-component stream may have here, 3 and 4 (T.81
    allows 1..4): read as 1x1 all the same.  The streams of equality_grey but for the SOF byte."""
    return [(f"g{h}{v}_37x53_ri{ri}", jf.forge(37, 53, [(h, v)], ri=ri, seed=7 + ri)) for h, v in GREY_FACTORS_TO_4 for ri in (0, 5)]


@functools.lru_cache(None)
def restart_streams():
    """[(name, Forged)] at 37x53: intervals of 1, 2, 7, exactly the MCU count, one more, and 65535 MCUs."""
    out = []
    for tag, fs in (("420", F420), ("422", F422), ("444", F444)):
        nmcu = jf.forge(37, 53, fs).nmcu
        for ri in (1, 2, 7, nmcu, nmcu + 1, 65535):
            out.append((f"r{tag}_ri{ri}", jf.forge(37, 53, fs, ri=ri, seed=RST_SEEDS[tag] if ri == 1 else 1000 + ri)))
    return out


@functools.lru_cache(None)
def long_stream():
    """120x200, 4:2:0, six coefficients of ten non-zero: one interval of many subsequences."""
    q = [np.full(64, 1), np.full(64, 2)]
    return jf.forge(120, 200, F420, qt=q, seed=5, density=0.6, amp=30, kinds=[1, 0, 0, 0, 0, 0, 0])


HEADER_FORMS = {"q16": dict(q16=True), "dht23": dict(one_dht=True, huff_ids=(2, 3)), "fill": dict(fill=2), "sof1": dict(sof=0xC1),
                "ids": dict(comp_ids=(10, 11, 12)), "com": dict(com_fake_sos=True), "dri0": dict(dri_then_zero=True)}


@functools.lru_cache(None)
def header_streams():
    """[(name, Forged)]: each header form alone, and all of them on one stream."""
    q = [np.arange(64) % 16 + 1, np.arange(64) % 13 + 2]
    q[0][63] = 300                   # needs the 16 bits
    forms = dict(HEADER_FORMS, all={k: v for d in HEADER_FORMS.values() for k, v in d.items()})
    return [("h_" + n, jf.forge(37, 53, F420, seed=11, qt=q if kw.get("q16") else None, **kw)) for n, kw in forms.items()]


@functools.lru_cache(None)
def twelve_blocks():
    return jf.forge(37, 53, [(2, 2)] * 3, seed=3)


@functools.lru_cache(None)
def mixed_batch():
    """[(name, Forged, expected status)] at 37x53: factor combinations, grey with SOF factors 2x2, and two bad streams (one
    the parse refuses, one with an undecodable code in its ninth block) between them."""
    col, grey = equality_colour(37, 53), dict(equality_grey(37, 53))
    bad = jf.forge(37, 53, F422, seed=31, hook=jf.ones16(8, False), safe=False)
    out = [(n, f, 0) for n, f in col[::3]]
    out[3:3] = [("twelve", twelve_blocks(), -1), ("g22a", grey["g22_37x53_ri0"], 0)]
    out[9:9] = [("g22b", grey["g22_37x53_ri5"], 0), ("ones16", bad, -1)]
    return out


def equality_streams():
    """Every stream whose reference is Pillow."""
    out = []
    for W, H in SIZES:
        out += equality_colour(W, H) + equality_grey(W, H)
    return out + equality_grey_to_4() + restart_streams() + header_streams() + [("long", long_stream())]


# ---- the four faults of UWIP_JPEG_BAD_STREAM, each at four places, each with its twin one step inside the rule --------------
BW, BH = 96, 88                     # 4:2:0: 36 MCUs of 6 blocks; grey (the same size: one batch): 132 blocks
SUB_BITS = 128 * 8                  # a subsequence of the device decoder


def _behind_four_subsequences(f):
    at = next(i for i, (iv, bit) in enumerate(f.pos) if iv == 0 and bit >= 4 * SUB_BITS)
    assert at < len(f.pos) - 20
    return at


def _ramp(base, factors, blocks, steps, ri):
    """The base stream with the DC of component 0 (q[0] = 1) at 0 everywhere but a climb of 2047 per block over the first
    `steps` of `blocks`, so the predictor reaches steps * 2047, and back down over those that follow.  blocks: consecutive
    blocks of component 0, up to the end of their restart interval (behind it the predictor starts again at 0)."""
    c = base.coefs.copy()
    c[base.comp == 0, 0] = 0
    for j, i in enumerate(blocks):
        c[i, 0] = 2047 * (j + 1 if j < steps else max(0, 2 * steps - 1 - j))
    return jf.forge(BW, BH, factors, qt=base.qt, coefs=c, zrl_close=base.zrl_close, ri=ri, safe=False)


PRED_RI = 6                         # MCUs per interval of the predictor fault's 4:2:0 stream: 24 blocks of component 0


@functools.lru_cache(None)
def bad_streams():
    """[(name, bad Forged, twin Forged, whether the twin is inside the amplitude bound, the block of the fault)].
    Places: the first block; a block behind four subsequences of an interval (its own is the fifth); the last block of the
    stream; a block of interval 5 (counted from 0) of a stream with restart interval 2.  The predictor fault needs 17 blocks of one component
    in one interval, more than two MCUs hold: its fourth place is interval 5 of a 4:2:0 stream with restart interval 6,
    where the other two components have predictors of their own to start again; its other places are on a grey stream.
    A bad stream and its twin hold the same blocks but for the one the hook writes; only a twin inside the bound is forged
    under it, which then checks the block its hook writes as well."""
    with12 = {"dc0": jf.DC_WITH_12, "dc1": jf.DC_WITH_12}
    base = jf.forge(BW, BH, F420, seed=21, density=0.5, amp=30)
    same = dict(qt=base.qt, coefs=base.coefs, zrl_close=base.zrl_close)
    nblk = len(base.coefs)
    places = [("first", 0, 0), ("deep", _behind_four_subsequences(base), 0), ("last", nblk - 1, 0), ("iv5", 5 * 2 * 6 + 4, 2)]
    assert jf.forge(BW, BH, F420, ri=2, **same).pos[64][0] == 5
    out = []
    for place, at, ri in places:
        for fault, bad, twin, tables, inside in (("cat12", jf.dc_category(at, 12), jf.dc_category(at, 11), with12, False),
                                                 ("run64", jf.run_to(at, 64), jf.run_to(at, 63), None, True),
                                                 ("ones16", jf.ones16(at, False), jf.ones16(at, True), None, False)):
            out.append((f"{fault}_{place}", jf.forge(BW, BH, F420, ri=ri, huff=tables, hook=bad, safe=False, **same),
                        jf.forge(BW, BH, F420, ri=ri, huff=tables, hook=twin, safe=inside, **same), inside, at))
    # the 17th difference of +2047 is the fault; the twin climbs 16 steps
    one = [np.ones(64, dtype=np.int64)]
    grey = jf.forge(BW, BH, [(1, 1)], qt=one, seed=22, density=0.5, amp=10)
    n = len(grey.coefs)
    for place, at17 in (("first", 0), ("deep", _behind_four_subsequences(grey)), ("last", n - 17)):
        late = 1 if place == "last" else 0                  # the twin of the last place ends at the last block too
        out.append((f"pred_{place}", _ramp(grey, [(1, 1)], range(at17, n), 17, 0), _ramp(grey, [(1, 1)], range(at17 + late, n), 16, 0),
                    False, at17 + 16))
    col = jf.forge(BW, BH, F420, qt=one + [np.full(64, 3)], seed=23, density=0.5, amp=10)
    assert col.bpm == 6 and col.nmcu == 6 * PRED_RI
    # from the second block of the interval's first MCU to the interval's end, the blocks of component 0
    blocks = [i for i in range(5 * PRED_RI * 6 + 1, 6 * PRED_RI * 6) if col.comp[i] == 0]
    assert len(blocks) == 4 * PRED_RI - 1 and (np.abs(col.coefs[col.comp > 0, 0]) > 0).any()
    out.append(("pred_iv5", _ramp(col, F420, blocks, 17, PRED_RI), _ramp(col, F420, blocks, 16, PRED_RI), False, blocks[16]))
    return out


