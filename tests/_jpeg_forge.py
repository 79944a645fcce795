"""A baseline JPEG writer for the decoder tests (T.81 sequential Huffman, 8 bit), at the level of quantised coefficients: no
DCT, no image.  It writes what no libjpeg encoder does -- any sampling factors per component, any restart interval, any
table ids and header forms, blocks that end without EOB or in a ZRL, and, through a per-block hook, symbols no encoder may
write -- so that the tests can state what a decoder must do with each.  numpy and the standard library only; nothing of the
code under test is read.  `read_coefs` is the forge's own reader, used to take the coefficients of a Pillow stream.

Coefficient blocks are int arrays of 64 in zigzag order, [0] the absolute DC value; quantiser tables are 64 values in natural
(row-major) order."""
import io

import numpy as np


def _zigzag():
    out = []
    for s in range(15):
        cells = [(r, s - r) for r in range(8) if 0 <= s - r < 8]
        out += [r * 8 + c for r, c in (cells if s & 1 else cells[::-1])]
    return out


ZZ = _zigzag()          # ZZ[k]: the natural index of zigzag position k
assert ZZ[:6] == [0, 1, 8, 16, 9, 2] and ZZ[63] == 63 and sorted(ZZ) == list(range(64))


def segments(stream):
    """[(marker, payload offset, payload length)] from SOI up to and including SOS; fill bytes before a marker skipped."""
    out, pos = [], 2
    while True:
        assert stream[pos] == 0xFF, pos
        while stream[pos + 1] == 0xFF:
            pos += 1
        m = stream[pos + 1]
        L = (stream[pos + 2] << 8) | stream[pos + 3]
        out.append((m, pos + 4, L - 2))
        pos += 2 + L
        if m == 0xDA:
            return out, pos


def _dht_tables(stream):
    """{(class, id): (bits[16], vals)} of every DHT table before SOS."""
    t = {}
    for m, a, n in segments(stream)[0]:
        p = a
        while m == 0xC4 and p < a + n:
            bits = list(stream[p + 1:p + 17])
            vals = list(stream[p + 17:p + 17 + sum(bits)])
            t[(stream[p] >> 4, stream[p] & 15)] = (bits, vals)
            p += 17 + sum(bits)
    return t


def _annex_k():
    """The four tables of T.81 Annex K.3, as the DHT segments of a non-optimised libjpeg stream give them."""
    from PIL import Image
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, format="JPEG", quality=75, optimize=False)
    t = _dht_tables(buf.getvalue())
    assert sorted(t) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [len(t[k][1]) for k in sorted(t)] == [12, 12, 162, 162] and t[(0, 0)][0][:9] == [0, 1, 5, 1, 1, 1, 1, 1, 1]
    return {"dc0": t[(0, 0)], "ac0": t[(1, 0)], "dc1": t[(0, 1)], "ac1": t[(1, 1)]}


ANNEX_K = _annex_k()
# the Annex K luminance DC table with one more code, of 10 bits, for the category 12 no baseline stream may use
DC_WITH_12 = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], list(range(13)))


def codes_of(bits, vals):
    """{symbol: (code, length)}: the canonical code of T.81 Annex C."""
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[p]] = (code, l)
            code += 1
            p += 1
        code <<= 1
    return out


def amp_bits(v):
    """(size, the `size` bits that follow the symbol) of a non-zero value (T.81 F.1.2.1)."""
    size = int(abs(v)).bit_length()
    return size, (v if v > 0 else v + (1 << size) - 1)


def block_symbols(blk, pred, zrl_close=False):
    """The symbols of one block: [("dc" | "ac", symbol, extra bits, their count)].  A block whose last coefficient is zero
    ends in EOB, or, with `zrl_close`, in as many ZRLs as run past coefficient 63."""
    size, bits = amp_bits(int(blk[0]) - pred) if int(blk[0]) != pred else (0, 0)
    assert size <= 11, "a DC difference of baseline JPEG has at most 11 bits"
    out, run = [("dc", size, bits, size)], 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(("ac", 0xF0, 0, 0))
            run -= 16
        size, bits = amp_bits(v)
        assert size <= 10, "an AC coefficient of baseline JPEG has at most 10 bits"
        out.append(("ac", (run << 4) | size, bits, size))
        run = 0
    if run:
        out += [("ac", 0xF0, 0, 0)] * ((run + 15) // 16) if zrl_close else [("ac", 0x00, 0, 0)]
    return out


def block_of(syms, pred):
    """The block that the symbols of `block_symbols` or of a hook stand for, [0] absolute from the predictor `pred`; None
    where they stand for none: raw bits, a DC category above 11, a run past coefficient 63."""
    def value(bits, size):
        return bits if size == 0 or bits >> (size - 1) else bits - (1 << size) + 1
    b, k = np.zeros(64, dtype=np.int64), 1
    for s in syms:
        if s[0] == "raw" or (s[0] == "dc" and s[1] > 11):
            return None
        if s[0] == "dc":
            b[0] = pred + value(s[2], s[1])
        elif s[1] == 0x00:
            break
        elif s[1] == 0xF0:
            k += 16
        else:
            k += s[1] >> 4
            if k > 63:
                return None
            b[k] = value(s[2], s[1] & 15)
            k += 1
    return b


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, val, n):
        assert 0 <= val < (1 << n) or n == 0
        self.acc, self.n, self.total = (self.acc << n) | val, self.n + n, self.total + n
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def close(self):
        """pads with 1-bits to a byte, stuffs a zero byte behind every 0xFF"""
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out).replace(b"\xff", b"\xff\x00")


def geometry(W, H, factors):
    """(hmax, vmax, mcux, mcuy, [(component, block row, block column) of each block of an MCU]).  One component: the scan
    is not interleaved (T.81 A.2.2), an MCU is one block whatever the factors."""
    if len(factors) == 1:
        return 1, 1, (W + 7) // 8, (H + 7) // 8, [(0, 0, 0)]
    hmax, vmax = max(h for h, _ in factors), max(v for _, v in factors)
    order = [(c, by, bx) for c, (h, v) in enumerate(factors) for by in range(v) for bx in range(h)]
    return hmax, vmax, (W + 8 * hmax - 1) // (8 * hmax), (H + 8 * vmax - 1) // (8 * vmax), order


# kinds of random block
SPARSE, LAST63, DC_ONLY, ZRL1, ZRL2, ZRL3, ZRL_CLOSE = range(7)


def random_blocks(rng, n, qz, density=0.12, amp=40, kinds=None, safe=True):
    """n blocks for quantisers `qz` (zigzag order) and the flags of those that close in a ZRL.  kinds: the probability of
    each kind of block.  safe: sum |coef * q| <= 1024 over every block."""
    kinds = kinds or [0.4, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]
    blocks, close = np.zeros((n, 64), dtype=np.int64), np.zeros(n, dtype=bool)
    kind = rng.choice(7, size=n, p=kinds)
    for i in range(n):
        b, k = blocks[i], int(kind[i])
        b[0] = int(rng.integers(-300, 301)) // int(qz[0])
        if k in (SPARSE, LAST63, ZRL_CLOSE):
            at = np.flatnonzero(rng.random(63) < density) + 1
            if k == ZRL_CLOSE:
                at = at[at < 60]                    # leaves a zero run at the end for the ZRL to cover
                close[i] = True
            b[at] = rng.integers(1, amp + 1, size=len(at)) * rng.choice([-1, 1], size=len(at))
            if k == LAST63:
                b[63] = int(rng.choice([-1, 1])) * int(rng.integers(1, amp + 1))
        elif k in (ZRL1, ZRL2, ZRL3):
            # one coefficient behind a run of 16 .. 31, 32 .. 47 or 48 .. 62 zeros
            z = {ZRL1: 1, ZRL2: 2, ZRL3: 3}[k]
            b[int(rng.integers(16 * z + 1, min(16 * z + 17, 64)))] = int(rng.choice([-1, 1])) * int(rng.integers(1, amp + 1))
        if safe:
            b[1:] = np.sign(b[1:]) * np.minimum(np.abs(b[1:]), np.maximum(1, 60 // qz[1:]))
            while np.abs(b * qz).sum() > 1024:
                nz = np.flatnonzero(b[1:]) + 1
                big = nz[np.abs(b[nz]) > 1]
                if len(big):
                    b[big] = np.sign(b[big]) * (np.abs(b[big]) // 2)
                else:
                    b[nz[rng.integers(len(nz))]] = 0
    return blocks, close


class Forged:
    """stream; coefs [blocks, 64] in scan order and zigzag order; comp: the component of each block; seg: the offset of the
    entropy-coded segment; pos: (interval, bit offset inside it before stuffing) of each block; ibits: the bits of each interval
    before padding; rst_after_stuffed: the intervals that end in a stuffed 0xFF before their RSTn; nmcu; bpm: blocks per MCU."""


def forge(W, H, factors, *, qt=None, q16=False, huff=None, huff_ids=(0, 1), one_dht=False, ri=0, seed=0, hook=None, coefs=None,
          zrl_close=None, density=0.12, amp=40, kinds=None, safe=True, sof=0xC0, comp_ids=(1, 2, 3), fill=0, com_fake_sos=False,
          dri_then_zero=False):
    """A baseline stream of W x H with the (h, v) factors of 1 or 3 components.
    qt: one or two 64-value tables in natural order (component 0 / the others), default drawn from the seed in 1..16; q16
    writes them with 16-bit precision.  huff: {"dc0", "ac0", "dc1", "ac1"} -> (bits, vals), default Annex K; huff_ids: the DHT
    ids of the two pairs; one_dht: all tables in one DHT segment.  ri: MCUs per restart interval written to DRI (0: no DRI).
    coefs / zrl_close: the blocks in scan order instead of random ones.  hook(i, component, symbols) may return other symbols
    for block i: ("dc" | "ac", symbol, bits, count) or ("raw", bits, count).  safe: assert the amplitude bound under which
    every libjpeg range limit gives the same samples, sum |coef * q| <= 1024 per block (then |sample - 128| <= 256), on
    `coefs` and on the block that the symbols written stand for, so a hook cannot leave it and must write a block.
    Header forms: sof (0xC0 / 0xC1), comp_ids, fill (0xFF bytes before each marker), com_fake_sos (a COM segment that holds
    FF DA), dri_then_zero (a DRI of 3 overridden by a DRI of 0; the stream has no restarts)."""
    rng = np.random.default_rng(seed)
    nc = len(factors)
    assert nc in (1, 3) and all(1 <= h <= 4 and 1 <= v <= 4 for h, v in factors)
    hmax, vmax, mcux, mcuy, order = geometry(W, H, factors)
    nmcu, bpm = mcux * mcuy, len(order)
    if qt is None:
        qt = [rng.integers(1, 17, size=64), rng.integers(1, 17, size=64)]
    qt = [np.asarray(q, dtype=np.int64) for q in qt]
    qt = qt if len(qt) == 2 else [qt[0], qt[0]]
    assert all(q.shape == (64,) and q.min() >= 1 and q.max() <= (65535 if q16 else 255) for q in qt)
    qz = [q[ZZ] for q in qt]
    comp = np.array([c for c, _, _ in order] * nmcu)
    if coefs is None:
        coefs, zrl_close = np.zeros((nmcu * bpm, 64), dtype=np.int64), np.zeros(nmcu * bpm, dtype=bool)
        for t in range(min(nc, 2)):
            sel = np.flatnonzero(np.minimum(comp, 1) == t)
            coefs[sel], zrl_close[sel] = random_blocks(rng, len(sel), qz[t], density, amp, kinds, safe)
    coefs = np.asarray(coefs, dtype=np.int64)
    zrl_close = np.zeros(len(coefs), dtype=bool) if zrl_close is None else zrl_close
    assert coefs.shape == (nmcu * bpm, 64)
    if safe:
        for i in range(len(coefs)):
            assert np.abs(coefs[i] * qz[min(int(comp[i]), 1)]).sum() <= 1024, i
    huff = dict(ANNEX_K, **(huff or {}))
    code = {k: codes_of(*v) for k, v in huff.items()}

    def marker(m, body=b""):
        return b"\xff" * fill + bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + body

    s = b"\xff\xd8"
    if com_fake_sos:
        s += marker(0xFE, b"a comment \xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00 with a scan header in it")
    for t in range(2 if nc == 3 else 1):
        s += marker(0xDB, bytes([(16 if q16 else 0) | t]) + b"".join(int(v).to_bytes(2 if q16 else 1, "big") for v in qz[t]))
    s += marker(sof, b"\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc]) +
                b"".join(bytes([comp_ids[c], (h << 4) | v, min(c, 1)]) for c, (h, v) in enumerate(factors)))
    dht = [bytes([(16 if k[:2] == "ac" else 0) | huff_ids[int(k[2])]]) + bytes(huff[k][0]) + bytes(huff[k][1])
           for k in (("dc0", "ac0", "dc1", "ac1") if nc == 3 else ("dc0", "ac0"))]
    s += marker(0xC4, b"".join(dht)) if one_dht else b"".join(marker(0xC4, d) for d in dht)
    if dri_then_zero:
        assert ri == 0
        s += marker(0xDD, b"\x00\x03") + marker(0xDD, b"\x00\x00")
    elif ri:
        s += marker(0xDD, ri.to_bytes(2, "big"))
    s += marker(0xDA, bytes([nc]) + b"".join(bytes([comp_ids[c], huff_ids[min(c, 1)] * 17]) for c in range(nc)) + b"\x00\x3f\x00")
    f = Forged()
    f.seg, f.pos, f.ibits, f.rst_after_stuffed = len(s), [], [], 0
    per = ri if 0 < ri < nmcu else nmcu
    i = 0
    for first in range(0, nmcu, per):
        w, pred, wpred = _Bits(), [0, 0, 0], [0, 0, 0]
        for _ in range(first, min(first + per, nmcu)):
            for c, _, _ in order:
                t = str(min(c, 1))
                syms = block_symbols(coefs[i], pred[c], bool(zrl_close[i]))
                pred[c] = int(coefs[i][0])
                if hook is not None:
                    syms = hook(i, c, syms) or syms
                if safe:
                    # the bound holds for what is written, a hook's symbols included (wpred: the predictor a decoder has)
                    wb = block_of(syms, wpred[c])
                    assert wb is not None and np.abs(wb * qz[min(c, 1)]).sum() <= 1024, i
                    wpred[c] = int(wb[0])
                f.pos.append((first // per, w.total))
                for kind, a, b, *n in syms:
                    if kind == "raw":
                        w.put(a, b)
                    else:
                        w.put(*code[kind + t][a])
                        w.put(b, n[0])
                i += 1
        f.ibits.append(w.total)
        data = w.close()
        if first + per < nmcu:
            f.rst_after_stuffed += data.endswith(b"\xff\x00")
            data += bytes([0xFF, 0xD0 + (first // per) % 8])
        s += data
    f.stream, f.coefs, f.zrl_close, f.comp, f.nmcu, f.bpm, f.qt = s + b"\xff\xd9", coefs, zrl_close, comp, nmcu, bpm, qt
    return f


# ---- symbols no encoder writes: hooks for one block, each with the twin one step inside the rule ------------------------------
def dc_category(at, cat):
    """Block `at` starts with DC category `cat` and all-one extra bits (the largest difference of the category); EOB."""
    return lambda i, c, syms: [("dc", cat, (1 << cat) - 1, cat), ("ac", 0, 0, 0)] if i == at else None


def run_to(at, k):
    """Block `at`: its own DC, three ZRLs (the next coefficient would be 49), then a run to coefficient k with value 1:
    k = 63 is the last coefficient (the block ends there, no EOB), k = 64 runs past it."""
    assert 49 <= k <= 64
    return lambda i, c, syms: [syms[0]] + [("ac", 0xF0, 0, 0)] * 3 + [("ac", ((k - 49) << 4) | 1, 1, 1)] if i == at else None


assert all(codes_of(*ANNEX_K[t])[0xFA] == (0xFFFE, 16) for t in ("ac0", "ac1"))


def ones16(at, valid):
    """Block `at`: its own DC, then sixteen 1-bits, which are no code of the Annex K tables; the valid twin is their longest
    code 1111111111111110 = (run 15, size 10) with value 1023, then EOB."""
    def hook(i, c, syms):
        if i != at:
            return None
        return [syms[0], ("ac", 0xFA, 1023, 10), ("ac", 0, 0, 0)] if valid else [syms[0], ("raw", 0xFFFF, 16)]
    return hook


# ---- the forge's own reader ------------------------------------------------------------------------------------------------
def read_coefs(stream):
    """A baseline stream -> dict(W, H, factors, qt (natural order, per component), ri, coefs [blocks, 64] in scan and zigzag
    order).  An independent walk of the symbols: tables from the stream's DHT, T.81 F.2.2 decoding."""
    segs, pos = segments(stream)
    qt, ri, comps, tabs = {}, 0, [], {}
    for m, a, n in segs:
        if m == 0xDB:
            p = a
            while p < a + n:
                w = 2 if stream[p] >> 4 else 1
                z = [int.from_bytes(stream[p + 1 + w * k:p + 1 + w * k + w], "big") for k in range(64)]
                q = np.zeros(64, dtype=np.int64)
                q[ZZ] = z
                qt[stream[p] & 15] = q
                p += 1 + 64 * w
        elif m in (0xC0, 0xC1):
            H, W = int.from_bytes(stream[a + 1:a + 3], "big"), int.from_bytes(stream[a + 3:a + 5], "big")
            comps = [(stream[a + 6 + 3 * i], stream[a + 7 + 3 * i] >> 4, stream[a + 7 + 3 * i] & 15, stream[a + 8 + 3 * i]) for i in range(stream[a + 5])]
        elif m == 0xDD:
            ri = int.from_bytes(stream[a:a + 2], "big")
        elif m == 0xDA:
            tabs = {stream[a + 1 + 2 * i]: (stream[a + 2 + 2 * i] >> 4, stream[a + 2 + 2 * i] & 15) for i in range(stream[a])}
    dht = {k: {(l, c): s for s, (c, l) in codes_of(*v).items()} for k, v in _dht_tables(stream).items()}
    factors = [(h, v) for _, h, v, _ in comps]
    _, _, mcux, mcuy, order = geometry(W, H, factors)
    nmcu = mcux * mcuy
    per = ri if 0 < ri < nmcu else nmcu
    # the intervals, unstuffed
    body, ivs, cur, p = stream[pos:], [], bytearray(), 0
    while True:
        if body[p] != 0xFF:
            cur.append(body[p])
            p += 1
        elif body[p + 1] == 0:
            cur.append(0xFF)
            p += 2
        else:
            ivs.append(bytes(cur))
            cur = bytearray()
            if body[p + 1] == 0xD9:
                break
            assert body[p + 1] == 0xD0 + (len(ivs) - 1) % 8
            p += 2
    assert len(ivs) == (nmcu + per - 1) // per
    coefs = []
    for n, iv in enumerate(ivs):
        bits, at, pred = int.from_bytes(iv, "big"), 0, [0, 0, 0]
        total = 8 * len(iv)

        def get(k):
            nonlocal at
            at += k
            assert at <= total
            return (bits >> (total - at)) & ((1 << k) - 1)

        def sym(table):
            c = 0
            for l in range(1, 17):
                c = (c << 1) | get(1)
                if (l, c) in table:
                    return table[(l, c)]
            raise AssertionError("no such code")

        def value(size):
            v = get(size)
            return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1
        for _ in range(min(per, nmcu - n * per)):
            for c, _, _ in order:
                td, ta = tabs[comps[c][0]]
                b = np.zeros(64, dtype=np.int64)
                pred[c] += value(sym(dht[(0, td)]))
                b[0], k = pred[c], 1
                while k < 64:
                    rs = sym(dht[(1, ta)])
                    if rs & 15 == 0:
                        if rs != 0xF0:
                            break
                        k += 16
                        continue
                    k += rs >> 4
                    b[k] = value(rs & 15)
                    k += 1
                coefs.append(b)
    return dict(W=W, H=H, factors=factors, qt=[qt[tq] for _, _, _, tq in comps], ri=ri, coefs=np.array(coefs))
