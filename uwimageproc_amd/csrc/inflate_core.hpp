// The arithmetic of inflate (RFC 1951) that is not parallel structure, written ONCE for the device loop of png_inflate.hpp,
// the host parse (png_parse.hpp) and the emulation harness: the zlib header rule, the length / distance bases and extra bits,
// the acceptance rules zlib's inflate_table applies to a set of code lengths, the canonical first codes, the look-up entry of
// a code, the slow path for the codes the look-up table does not hold, and the fixed code.  The code-length order, the bit
// reversal, the fixed literal/length lengths and the Adler-32 combination are deflate_core.hpp's.
// Plain C++ without hipcc; __host__ __device__ under it.
#pragma once
#include "deflate_core.hpp"

namespace uwip_inflate {

using uwip_png::cl_order;
using uwip_png::rev_bits;

constexpr int kMaxBits = 15;
constexpr int kMaxLL = 286, kMaxDist = 30;      // zlib: "too many length or distance symbols" above these
constexpr int kFixedLL = 288, kFixedDist = 32;  // the fixed code describes 288 / 32 symbols; 286, 287 / 30, 31 never decode
enum { kCodes = 0, kLens = 1, kDists = 2 };     // what a set of code lengths is for (zlib's CODES, LENS, DISTS)

// CMF, FLG as zlib's inflate checks them behind inflateInit (15 window bits): method 8, CINFO <= 7, FCHECK, no FDICT
DEFLATE_HD bool zlib_header_ok(uint32_t cmf, uint32_t flg)
{
    return ((cmf << 8) + flg) % 31u == 0u && (cmf & 15u) == 8u && (cmf >> 4) <= 7u && (flg & 0x20u) == 0u;
}

// literal/length symbols 257..285 (idx = symbol - 257, 0..28) and distance symbols 0..29 (RFC 1951, 3.2.5), in closed form
DEFLATE_HD uint32_t length_extra(uint32_t idx) { return (idx < 8u || idx == 28u) ? 0u : (idx >> 2) - 1u; }
DEFLATE_HD uint32_t length_base(uint32_t idx)
{
    if (idx < 8u) return 3u + idx;
    if (idx == 28u) return 258u;
    return 3u + ((4u + (idx & 3u)) << ((idx >> 2) - 1u));
}
DEFLATE_HD uint32_t dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }
DEFLATE_HD uint32_t dist_base(uint32_t sym) { return sym < 4u ? 1u + sym : 1u + ((2u + (sym & 1u)) << ((sym >> 1) - 1u)); }

DEFLATE_HD int fixed_len(int i) { return i < kFixedLL ? uwip_png::fixed_ll_len(i) : 5; }      // i: 0..287 literal/length, then 32 distances

// What a set of code lengths decodes with: cnt[l] codes of length l, the first canonical code of each length, where the
// symbols of each length start in the list of symbols sorted by (length, symbol).
struct CodeSet { uint32_t cnt[16], first[16], off[16]; };

// zlib's inflate_table: an over-subscribed set is an error; an incomplete one too, unless it is a literal/length or distance
// set whose only code has one bit; a set without codes builds (every code then fails to decode).  The code-length set without
// codes is refused here at once: with it zlib reads every length as 0 and then misses the end-of-block code.
DEFLATE_HD bool code_set_accepted(const uint32_t *cnt, int kind)
{
    int max = kMaxBits;
    while (max >= 1 && cnt[max] == 0u) --max;
    if (max == 0) return kind != kCodes;
    int left = 1;
    for (int l = 1; l <= kMaxBits; ++l) {
        left <<= 1;
        left -= (int)cnt[l];
        if (left < 0) return false;
    }
    return !(left > 0 && (kind == kCodes || max != 1));
}
DEFLATE_HD void code_set_first(CodeSet &c)
{
    uint32_t code = 0, off = 0;
    c.first[0] = 0; c.off[0] = 0;
    for (int l = 1; l <= kMaxBits; ++l) {
        code = (code + (l > 1 ? c.cnt[l - 1] : 0u)) << 1;
        c.first[l] = code; c.off[l] = off;
        off += c.cnt[l];
    }
}
// a look-up entry: symbol | length << 12; 0: no code of at most `lutbits` bits starts with these bits
DEFLATE_HD uint16_t lut_entry(uint32_t sym, uint32_t len) { return (uint16_t)(sym | (len << 12)); }
// the codes longer than the look-up table: v holds the next bits of the stream, least significant first.  At most 15 - lutbits
// steps; the index into `sorted` is below off[l] + cnt[l], the number of symbols.
DEFLATE_HD bool decode_slow(const CodeSet &c, const uint16_t *sorted, int lutbits, uint32_t v, uint32_t &len, uint32_t &sym)
{
    uint32_t code = rev_bits(v & ((1u << lutbits) - 1u), lutbits);
    for (int l = lutbits + 1; l <= kMaxBits; ++l) {
        code = (code << 1) | ((v >> (l - 1)) & 1u);
        const uint32_t d = code - c.first[l];
        if (d < c.cnt[l]) { sym = sorted[c.off[l] + d]; len = (uint32_t)l; return true; }
    }
    return false;
}

// The screen of a bit position as the start of a dynamic block (png_decode.hip, found block starts), all of it necessary for
// dynamic_header to accept the position: v holds the 17 bits BFINAL, BTYPE, HLIT, HDIST, HCLEN, w the 57 bits behind them
// (up to 19 code lengths of 3 bits).  BTYPE 2, HLIT <= 286 - 257, HDIST <= 30 - 1, and the code-length code complete: the sum
// of 2^(7 - l) over its non-zero lengths l is 2^7, which is what code_set_accepted asks of a kCodes set.
DEFLATE_HD bool dynamic_start_plausible(uint32_t v, uint64_t w)
{
    if (((v >> 1) & 3u) != 2u || ((v >> 3) & 31u) > (uint32_t)(kMaxLL - 257) || ((v >> 8) & 31u) > (uint32_t)(kMaxDist - 1)) return false;
    const uint32_t nc = ((v >> 13) & 15u) + 4u;
    uint32_t sum = 0;
    for (uint32_t i = 0; i < nc; ++i) {
        const uint32_t l = (uint32_t)(w >> (3u * i)) & 7u;
        sum += l ? 128u >> l : 0u;
    }
    return sum == 128u;
}

}  // namespace uwip_inflate
