// The arithmetic of the PNG encoder (png_encode.hip) that is not parallel structure, written ONCE for the device kernels, the
// serial host reference encoder (png_reference.hpp) and the emulation harness: the row filters and their cost, the run-to-token
// rule (zlib's Z_RLE parse), the length symbols, the length-limited Huffman code builder, the 16/17/18 run coding of a code
// length vector, canonical codes in the bit order deflate stores them, the block header, Adler-32 and CRC-32 combination.
// Plain C++ without hipcc; __host__ __device__ under it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DEFLATE_HD __host__ __device__ __forceinline__
#else
#define DEFLATE_HD inline
#endif

namespace uwip_png {

constexpr int kChunk = 32768;           // filtered bytes per independently coded chunk (one deflate block, one IDAT)
constexpr int kNumLL = 286, kNumCL = 19, kEOB = 256;
constexpr int kMaxLLBits = 15, kMaxCLBits = 7;
constexpr uint32_t kAdlerMod = 65521u, kCrcPoly = 0xEDB88320u;
// per chunk: IDAT length, type and CRC (12), the stored block's header (5), the empty stored block behind it (5);
// per frame: signature and IHDR (33), the zlib header (2), the IDAT of the Adler-32 (16), IEND (12)
constexpr int kChunkOverhead = 22, kFrameOverhead = 63;
constexpr int kHeadBytes = 33, kTailBytes = 28;
enum { kStored = 0, kFixed = 1, kDynamic = 2 };

// ---- row filters (PNG 1.2, 6.2 .. 6.6): x the byte, a the byte one pixel to the left, b above, c above left -------------
DEFLATE_HD int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
DEFLATE_HD uint8_t filter_byte(int type, int x, int a, int b, int c)
{
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (uint8_t)(x - pred);
}
// what a filtered byte adds to its row's cost: min(v, 256 - v)
DEFLATE_HD uint32_t filter_cost(uint8_t v) { return v < 128 ? v : 256u - v; }

// ---- tokens: byte k of a run of R equal bytes is a literal (1), starts a match of 3..258 bytes at distance 1, or is covered
// by one (0).  The first byte is a literal, the R - 1 that follow go into matches of 258 while at least 3 are left.
DEFLATE_HD int rle_token(int k, int R)
{
    if (k == 0) return 1;
    const int j = k - 1, grp = j / 258, r = j - grp * 258, rem = R - 1 - grp * 258;
    if (rem < 3) return 1;
    return r == 0 ? (rem < 258 ? rem : 258) : 0;
}

DEFLATE_HD int msb_of(uint32_t v) { return 31 - __builtin_clz(v); }     // v != 0

// the literal/length symbol of a match length 3..258, with its extra bits (RFC 1951, 3.2.5)
DEFLATE_HD void length_symbol(int len, int &sym, int &nextra, uint32_t &extra)
{
    const int l = len - 3;
    nextra = 0; extra = 0;
    if (len == 258) { sym = 285; return; }
    if (l < 8) { sym = 257 + l; return; }
    const int e = msb_of((uint32_t)l) - 2;
    sym = 257 + 4 * e + (l >> e); nextra = e; extra = (uint32_t)l & ((1u << e) - 1u);
}
DEFLATE_HD int ll_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
DEFLATE_HD int fixed_ll_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
DEFLATE_HD uint32_t fixed_ll_code(int sym)
{
    return sym < 144 ? 0x30u + sym : sym < 256 ? 0x190u + (sym - 144) : sym < 280 ? (uint32_t)(sym - 256) : 0xC0u + (sym - 280);
}
// a Huffman code goes into the stream most significant bit first, everything else least significant first
DEFLATE_HD uint32_t rev_bits(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}

// ---- the length-limited Huffman code -------------------------------------------------------------------------------------
// position of symbol i among the used symbols in the order (count, symbol number) ascending; -1 for an unused one
DEFLATE_HD int huff_rank(const uint32_t *freq, int n, int i)
{
    const uint32_t fi = freq[i];
    if (!fi) return -1;
    int r = 0;
    for (int j = 0; j < n; ++j) { const uint32_t fj = freq[j]; r += fj && (fj < fi || (fj == fi && j < i)); }
    return r;
}
// serial form of the sort: order[0..m) and m
DEFLATE_HD int huff_sort(const uint32_t *freq, int n, uint16_t *order)
{
    int m = 0;
    for (int i = 0; i < n; ++i) { const int r = huff_rank(freq, n, i); if (r >= 0) { order[r] = (uint16_t)i; ++m; } }
    return m;
}
// Code lengths for the m used symbols order[0..m) (ascending count): the Huffman tree by the two-queue merge (of two equal
// weights the leaf goes first), depths, the depths above `limit` cut to it, and the Kraft sum brought back to one a unit of
// 2^-limit at a time by moving the deepest leaf above the limit one level down next to a leaf taken from the limit (zlib's
// gen_bitlen repair); then the lengths are dealt out longest to rarest.  iw: m words, node: 2 m halfwords of scratch.
DEFLATE_HD void huff_build(const uint32_t *freq, int n, const uint16_t *order, int m, int limit, uint8_t *len, uint32_t *iw,
                           uint16_t *node)
{
    for (int i = 0; i < n; ++i) len[i] = 0;
    if (m == 0) return;
    if (m == 1) { len[order[0]] = 1; return; }
    int li = 0, ii = 0;
    for (int k = 0; k < m - 1; ++k) {
        uint32_t w = 0;
        for (int s = 0; s < 2; ++s) {
            const bool leaf = li < m && (ii >= k || freq[order[li]] <= iw[ii]);
            if (leaf) { w += freq[order[li]]; node[li] = (uint16_t)(m + k); ++li; }
            else      { w += iw[ii]; node[m + ii] = (uint16_t)(m + k); ++ii; }
        }
        iw[k] = w;
    }
    node[2 * m - 2] = 0;                                   // the root; a parent always has the higher index
    for (int i = 2 * m - 3; i >= 0; --i) node[i] = (uint16_t)(node[node[i]] + 1);
    uint32_t blc[16];
    for (int b = 0; b < 16; ++b) blc[b] = 0;
    for (int i = 0; i < m; ++i) blc[node[i] > limit ? limit : node[i]]++;
    int64_t excess = -((int64_t)1 << limit);
    for (int b = 1; b <= limit; ++b) excess += (int64_t)blc[b] << (limit - b);
    for (; excess > 0; --excess) {
        int bits = limit - 1;
        while (blc[bits] == 0) --bits;
        blc[bits]--; blc[bits + 1] += 2; blc[limit]--;
    }
    int i = 0;
    for (int b = limit; b >= 1; --b)
        for (uint32_t c = 0; c < blc[b]; ++c) len[order[i++]] = (uint8_t)b;
}
// canonical codes from the lengths: table[s] = the code, bit-reversed, | length << 16
DEFLATE_HD void huff_codes(const uint8_t *len, int n, uint32_t *table)
{
    uint32_t blc[17], next[17];
    for (int b = 0; b < 17; ++b) blc[b] = 0;
    for (int i = 0; i < n; ++i) blc[len[i]]++;
    blc[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int b = 1; b < 17; ++b) { code = (code + blc[b - 1]) << 1; next[b] = code; }
    for (int i = 0; i < n; ++i) table[i] = len[i] ? rev_bits(next[len[i]]++, len[i]) | ((uint32_t)len[i] << 16) : 0u;
}

// The run coding of a vector of code lengths, zlib's rule (scan_tree / send_tree): zeros in runs of 3..10 (17) and 11..138
// (18), a repeated length once and then in runs of 3..6 (16), anything shorter as it is.  put(symbol, extra value, extra bits).
template <class Put>
DEFLATE_HD void code_length_runs(const uint8_t *len, int n, Put put)
{
    int prevlen = -1, nextlen = len[0], count = 0, maxc = 7, minc = 4;
    if (nextlen == 0) { maxc = 138; minc = 3; }
    for (int i = 0; i < n; ++i) {
        const int curlen = nextlen;
        nextlen = i + 1 < n ? len[i + 1] : -1;
        if (++count < maxc && curlen == nextlen) continue;
        if (count < minc) { for (int c = 0; c < count; ++c) put(curlen, 0u, 0); }
        else if (curlen != 0) {
            if (curlen != prevlen) { put(curlen, 0u, 0); --count; }
            put(16, (uint32_t)(count - 3), 2);
        } else if (count <= 10) put(17, (uint32_t)(count - 3), 3);
        else put(18, (uint32_t)(count - 11), 7);
        count = 0; prevlen = curlen;
        if (nextlen == 0) { maxc = 138; minc = 3; }
        else if (curlen == nextlen) { maxc = 6; minc = 3; }
        else { maxc = 7; minc = 4; }
    }
}

// what one chunk's block is coded with
struct Codes {
    uint32_t ll[kNumLL];            // literal/length symbol -> reversed code | length << 16
    uint32_t cl[kNumCL];            // the code length code
    uint32_t dist;                  // the code of distance symbol 0 (the only distance there is)
    uint32_t hdr_bits, data_bits;   // BFINAL and BTYPE and the code description; the tokens and the end-of-block code
    int32_t mode, hlit, hclen;
    uint8_t ll_len[kNumLL], cl_len[kNumCL], dist_len;
};
struct Scratch {
    uint32_t iw[kNumLL], clfreq[kNumCL];
    uint16_t order[kNumLL], node[2 * kNumLL], clorder[kNumCL];
};
DEFLATE_HD int cl_order(int i)
{
    constexpr uint8_t o[kNumCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}

// From the counts of a chunk of n bytes (freq[kEOB] = 1 included; s.order[0..m) the used symbols, sorted) to the block type
// and its codes: stored where that is not longer in bytes, else fixed where that is not longer in bits, else dynamic.
DEFLATE_HD void plan_block(const uint32_t *freq, uint32_t nmatch, int n, int m, Scratch &s, Codes &c)
{
    huff_build(freq, kNumLL, s.order, m, kMaxLLBits, c.ll_len, s.iw, s.node);
    c.dist_len = nmatch ? 1 : 0;
    int hlit = kNumLL;
    while (hlit > 257 && c.ll_len[hlit - 1] == 0) --hlit;
    for (int i = 0; i < kNumCL; ++i) s.clfreq[i] = 0;
    uint32_t xbits = 0;
    auto count = [&](int sym, uint32_t, int nx) { s.clfreq[sym]++; xbits += (uint32_t)nx; };
    code_length_runs(c.ll_len, hlit, count);
    code_length_runs(&c.dist_len, 1, count);
    const int mc = huff_sort(s.clfreq, kNumCL, s.clorder);
    huff_build(s.clfreq, kNumCL, s.clorder, mc, kMaxCLBits, c.cl_len, s.iw, s.node);
    int hclen = kNumCL;
    while (hclen > 4 && c.cl_len[cl_order(hclen - 1)] == 0) --hclen;
    uint32_t dyn_hdr = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen + xbits, dyn = 0, fix = 0;
    for (int i = 0; i < kNumCL; ++i) dyn_hdr += s.clfreq[i] * c.cl_len[i];
    for (int i = 0; i < kNumLL; ++i) {
        dyn += freq[i] * (uint32_t)(c.ll_len[i] + ll_extra_bits(i));
        fix += freq[i] * (uint32_t)(fixed_ll_len(i) + ll_extra_bits(i));
    }
    dyn += nmatch * c.dist_len;
    fix += nmatch * 5u;
    const bool use_fixed = 3 + fix <= dyn_hdr + dyn;
    const uint32_t bits = use_fixed ? 3 + fix : dyn_hdr + dyn;
    c.hlit = hlit; c.hclen = hclen;
    if ((uint32_t)(5 + n) <= (bits + 7) / 8) { c.mode = kStored; c.hdr_bits = 0; c.data_bits = 0; return; }
    if (use_fixed) {
        c.mode = kFixed; c.hdr_bits = 3; c.data_bits = fix;
        for (int i = 0; i < kNumLL; ++i) c.ll[i] = rev_bits(fixed_ll_code(i), fixed_ll_len(i)) | ((uint32_t)fixed_ll_len(i) << 16);
        c.dist = 5u << 16;
        return;
    }
    c.mode = kDynamic; c.hdr_bits = dyn_hdr; c.data_bits = dyn;
    huff_codes(c.ll_len, kNumLL, c.ll);
    huff_codes(c.cl_len, kNumCL, c.cl);
    c.dist = (uint32_t)c.dist_len << 16;                      // the one-bit code 0
}

// BFINAL, BTYPE and, for a dynamic block, the description of its codes: put(value, bit count), least significant bit first
template <class Put>
DEFLATE_HD void put_block_header(const Codes &c, bool final, Put put)
{
    put(final ? 1u : 0u, 1);
    put((uint32_t)c.mode, 2);
    if (c.mode != kDynamic) return;
    put((uint32_t)(c.hlit - 257), 5);
    put(0u, 5);                                               // one distance code
    put((uint32_t)(c.hclen - 4), 4);
    for (int i = 0; i < c.hclen; ++i) put(c.cl_len[cl_order(i)], 3);
    auto send = [&](int sym, uint32_t extra, int nx) {
        put(c.cl[sym] & 0xffffu, (int)(c.cl[sym] >> 16));
        if (nx) put(extra, nx);
    };
    code_length_runs(c.ll_len, c.hlit, send);
    code_length_runs(&c.dist_len, 1, send);
}

// one token into put(value, bit count): a literal byte, or a match of `len` bytes at distance 1
template <class Put>
DEFLATE_HD void put_token(const Codes &c, int len, int byte, Put put)
{
    if (len == 1) { put(c.ll[byte] & 0xffffu, (int)(c.ll[byte] >> 16)); return; }
    int sym, nx;
    uint32_t extra;
    length_symbol(len, sym, nx, extra);
    const uint32_t s = c.ll[sym];
    const int sl = (int)(s >> 16), dl = (int)(c.dist >> 16);
    put((s & 0xffffu) | (extra << sl), sl + nx + dl);         // the distance code is dl zero bits
}

// Bits into a window of little-endian 32-bit words, least significant first, from bit `pos` on; words other writers touch
// too are ORed into (Or: atomicOr on the device, a plain |= on one thread).
template <class Or>
struct BitSink {
    uint32_t *w;
    uint32_t wi;
    int nacc;
    uint64_t acc;
    Or orw;
    DEFLATE_HD BitSink(uint32_t *win, uint32_t pos, Or o) : w(win), wi(pos >> 5), nacc((int)(pos & 31)), acc(0), orw(o) {}
    DEFLATE_HD void put(uint32_t v, int n)                    // n <= 32, v < 2^n
    {
        acc |= (uint64_t)v << nacc;
        nacc += n;
        if (nacc >= 32) { orw(&w[wi], (uint32_t)acc); ++wi; acc >>= 32; nacc -= 32; }
    }
    DEFLATE_HD void flush() { if (acc) orw(&w[wi], (uint32_t)acc); acc = 0; }
};

// ---- CRC-32 (reflected, polynomial 0xEDB88320): the register is linear in (start value, message) -----------------------------
DEFLATE_HD uint32_t crc_table_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ kCrcPoly : i >> 1;
    return i;
}
DEFLATE_HD uint32_t crc_byte(uint32_t state, uint8_t b) { return crc_table_entry((state ^ b) & 0xffu) ^ (state >> 8); }
// the CRC-32 of n bytes, bit by bit (headers and trailers; the payloads go through a table)
DEFLATE_HD uint32_t crc_bytes(const uint8_t *p, int n)
{
    uint32_t s = 0xffffffffu;
    for (int i = 0; i < n; ++i) s = crc_byte(s, p[i]);
    return s ^ 0xffffffffu;
}
// a(x) b(x) mod P in the reflected representation (x^0 is bit 31)
DEFLATE_HD uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^(8 n) mod P: what n more message bytes multiply a register by
DEFLATE_HD uint32_t crc_shift_bytes(uint32_t n)
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;              // x^0, x^8
    for (; n; n >>= 1) { if (n & 1u) p = crc_mulmod(p, sq); sq = crc_mulmod(sq, sq); }
    return p;
}
// the register after "IDAT" from the all-ones start
DEFLATE_HD uint32_t crc_idat_state()
{
    uint32_t s = 0xffffffffu;
    s = crc_byte(s, 'I'); s = crc_byte(s, 'D'); s = crc_byte(s, 'A'); s = crc_byte(s, 'T');
    return s;
}
// the CRC of an IDAT chunk from the zero-start register `raw` of its len payload bytes
DEFLATE_HD uint32_t crc_idat(uint32_t raw, uint32_t len) { return crc_mulmod(crc_idat_state(), crc_shift_bytes(len)) ^ raw ^ 0xffffffffu; }

// ---- Adler-32 from per-chunk sums: (A, B) of a chunk of n bytes d[i] are sum d[i] and sum (n - i) d[i], both mod 65521 ------
DEFLATE_HD void adler_append(uint32_t &A, uint32_t &B, uint32_t a, uint32_t b, uint32_t n)
{
    B = (uint32_t)((B + (uint64_t)(n % kAdlerMod) * A + b) % kAdlerMod);
    A = (A + a) % kAdlerMod;
}

DEFLATE_HD void put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// signature and IHDR (33 bytes) of a rows x cols frame of nc channels
DEFLATE_HD void write_head(int rows, int cols, int nc, uint8_t *h)
{
    const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    for (int i = 0; i < 8; ++i) h[i] = sig[i];
    put_be32(h + 8, 13);
    h[12] = 'I'; h[13] = 'H'; h[14] = 'D'; h[15] = 'R';
    put_be32(h + 16, (uint32_t)cols); put_be32(h + 20, (uint32_t)rows);
    h[24] = 8; h[25] = nc == 1 ? 0 : 2; h[26] = 0; h[27] = 0; h[28] = 0;
    put_be32(h + 29, crc_bytes(h + 12, 17));
}
// the IDAT that holds the Adler-32, and IEND (28 bytes)
DEFLATE_HD void write_tail(uint32_t adler, uint8_t *t)
{
    put_be32(t, 4);
    t[4] = 'I'; t[5] = 'D'; t[6] = 'A'; t[7] = 'T';
    put_be32(t + 8, adler);
    put_be32(t + 12, crc_bytes(t + 4, 8));
    put_be32(t + 16, 0);
    t[20] = 'I'; t[21] = 'E'; t[22] = 'N'; t[23] = 'D';
    put_be32(t + 24, crc_bytes(t + 20, 4));
}

// filtered bytes of a frame, its chunks, and the bound on its stream
DEFLATE_HD uint64_t filtered_bytes(int rows, int cols, int nc) { return (uint64_t)rows * ((uint64_t)cols * nc + 1); }
DEFLATE_HD uint64_t chunks_of(uint64_t filtered) { return (filtered + kChunk - 1) / kChunk; }

}  // namespace uwip_png
