// The device side of inflate for png_decode.hip: one wavefront reads a deflate stream from a bit position on and hands the
// bytes to a sink.  The bit reader, the decoding tables the lanes build in LDS, a dynamic block's header and ONE loop over
// whole blocks, inflate_run, which every inflating kernel calls: k_pngd_inflate (segments and whole streams), k_pngs_measure
// (search, chunk 0 and repair) and k_pngs_write.  The arithmetic that is not parallel structure is inflate_core.hpp's.
// Device code: under hipcc as it stands, under the host compiler behind tests/hip_on_host.hpp (tests/png_decode_emulated.cpp).
//
// The symbol decode is wave-uniform and serial in the bit stream: every lane decodes the same tokens.  A dynamic block's tables
// are built by the lanes into LDS: a direct look-up table for the short codes, first code / count / sorted symbols for the rest.
//
// What bounds inflate_run on untrusted bytes:
//   (1) the bit position never passes the input's length by more than one token: bits at or behind the last byte read as zeros
//       without a load (peek32), and the first step that leaves the position behind the end fails the run;
//   (2) every token is checked against the window before it is taken (`o + length <= win`), a stored block's length against
//       the window and the input, so a run never produces more than `win` bytes;
//   (3) table indices: look-up indices are masked to the table width; the slow path indexes sorted[off[l] + d] with d < cnt[l],
//       below the symbol count by construction; code lengths are written at have + j < HLIT + HDIST <= 316 < 320; literal/length
//       symbols >= 286 and distance symbols >= 30 are refused before their base is computed; count indices are masked to 0..15;
//   (4) a step consumes at least one bit (a block header 3, a token at least 1) or ends the run: at most 8 x length steps.
// What a sink adds:
//   LengthsOnly  nothing: no store, no LDS token, no barrier, no distance check; a round is a whole block.
//   ByteSink     the bytes into out[0, win).  A match reads its source from out, so a distance beyond the bytes the run has
//                produced fails it (`distance <= o`): every index formed lies in [0, win).
//   ElemSink     16-bit elements into out[0, win): a byte, or kMarker | k for "the byte k + 1 before out[0]".  abs0 bytes of
//                the stream lie before out[0], and a distance beyond them fails the run (`distance <= abs0 + o`).  A source
//                index before out[0] is never read: it becomes the marker, k <= 32 767 since a distance is at most 32 768.
#pragma once
#include "inflate_core.hpp"

namespace uwip_inflate {

constexpr int kLLBits = 10, kDBits = 8, kCLBits = 7;     // look-up widths: literal/length, distance, code length codes
constexpr int kRound = 64;                               // tokens per round of a storing sink: one per lane
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMarker = 0x8000u;

// 32 bits of the input from bit p on, least significant first; bits at or past its last byte are zeros (no load there).
// The second word may lie behind the input: the buffer is 16 bytes longer than its last stream.
__device__ __forceinline__ uint32_t peek32(const uint8_t *src, uint32_t a0, uint32_t len, uint32_t p)
{
    const uint32_t by = p >> 3;
    if (by >= len) return 0u;
    const uint32_t a = a0 + by;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(src) + (a >> 2);
    const uint64_t x = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    uint32_t v = (uint32_t)(x >> ((a & 3u) * 8u + (p & 7u)));
    const uint32_t rem = len * 8u - p;                       // >= 1
    if (rem < 32u) v &= (1u << rem) - 1u;
    return v;
}

struct Tables {
    uint16_t ll[1 << kLLBits], d[1 << kDBits], cl[1 << kCLBits];
    uint16_t ll_sorted[kFixedLL], d_sorted[kFixedDist], cl_sorted[uwip_png::kNumCL];
    CodeSet ll_set, d_set, cl_set;
    uint8_t lens[kFixedLL + kFixedDist], cl_lens[uwip_png::kNumCL + 1];
    uint16_t tlen[kRound], tval[kRound];                     // a round's tokens: length (1: a literal), byte or distance
    uint32_t tout[kRound];                                   // where each goes, from the run's first byte
    uint32_t bad;
};

// The lanes build the decoding tables of n code lengths (each 0..15): false where zlib refuses the set.
__device__ bool build_table(const uint8_t *lens, int n, int kind, int lutbits, uint16_t *lut, uint16_t *sorted, CodeSet &c)
{
    const int lane = (int)threadIdx.x;
    if (lane < 16) c.cnt[lane] = 0u;
    for (int i = lane; i < (1 << lutbits); i += 64) lut[i] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) if (lens[i]) atomicAdd(&c.cnt[lens[i] & 15], 1u);
    __syncthreads();
    if (!code_set_accepted(c.cnt, kind)) return false;       // the same answer in every lane
    if (lane == 0) code_set_first(c);
    __syncthreads();
    if (lane >= 1 && lane <= kMaxBits && c.cnt[lane]) {      // lane l deals out the codes of length l in symbol order
        const uint32_t l = (uint32_t)lane;
        uint32_t code = c.first[l], at = c.off[l];
        for (int s = 0; s < n; ++s) {
            if (lens[s] != l) continue;
            sorted[at++] = (uint16_t)s;                      // at < off[l] + cnt[l] <= n
            if ((int)l <= lutbits)
                for (uint32_t k = rev_bits(code, (int)l); k < (1u << lutbits); k += 1u << l) lut[k] = lut_entry((uint32_t)s, l);
            ++code;
        }
    }
    __syncthreads();
    return true;
}

__device__ __forceinline__ bool decode_sym(const uint16_t *lut, int lutbits, const CodeSet &c, const uint16_t *sorted, uint32_t v,
                                           uint32_t &len, uint32_t &sym)
{
    const uint32_t e = lut[v & ((1u << lutbits) - 1u)];
    if (e) { len = e >> 12; sym = e & 0xFFFu; return true; }
    return decode_slow(c, sorted, lutbits, v, len, sym);
}

// a dynamic block's header from bit pos on: the code lengths into T.lens and the two tables; false: zlib refuses it (or the
// input ends inside it)
__device__ bool dynamic_header(Tables &T, const uint8_t *src, uint32_t a0, uint32_t len, uint32_t &pos)
{
    const uint32_t lane = threadIdx.x, lenbits = len * 8u;
    uint32_t v = peek32(src, a0, len, pos);
    const uint32_t nlen = (v & 31u) + 257u, nd = ((v >> 5) & 31u) + 1u, nc = ((v >> 10) & 15u) + 4u;
    pos += 14u;
    if (pos > lenbits || nlen > (uint32_t)kMaxLL || nd > (uint32_t)kMaxDist) return false;
    if (lane < (uint32_t)uwip_png::kNumCL) T.cl_lens[lane] = 0;
    __syncthreads();
    for (uint32_t i = 0; i < nc; ++i) {                       // nc <= 19
        const uint32_t val = peek32(src, a0, len, pos) & 7u;
        pos += 3u;
        if (lane == 0) T.cl_lens[cl_order((int)i)] = (uint8_t)val;
    }
    if (pos > lenbits) return false;
    __syncthreads();
    if (!build_table(T.cl_lens, uwip_png::kNumCL, kCodes, kCLBits, T.cl, T.cl_sorted, T.cl_set)) return false;
    const uint32_t want = nlen + nd;                          // <= 316
    uint32_t have = 0, prev = 0;
    while (have < want) {
        v = peek32(src, a0, len, pos);
        const uint32_t e = T.cl[v & ((1u << kCLBits) - 1u)];  // every code of this set has at most 7 bits
        if (!e) return false;
        const uint32_t l = e >> 12, sym = e & 0xFFFu;
        pos += l;
        if (sym < 16u) {
            if (lane == 0) T.lens[have] = (uint8_t)sym;
            prev = sym; ++have;
        } else {
            uint32_t rep, val = 0;
            if (sym == 16u) { if (have == 0u) return false; rep = 3u + ((v >> l) & 3u); pos += 2u; val = prev; }
            else if (sym == 17u) { rep = 3u + ((v >> l) & 7u); pos += 3u; }
            else { rep = 11u + ((v >> l) & 127u); pos += 7u; }
            if (have + rep > want) return false;
            for (uint32_t j = lane; j < rep; j += 64u) T.lens[have + j] = (uint8_t)val;
            have += rep; prev = val;
        }
        if (pos > lenbits) return false;
    }
    __syncthreads();
    if (T.lens[256] == 0) return false;                       // no end-of-block code
    if (!build_table(T.lens, (int)nlen, kLens, kLLBits, T.ll, T.ll_sorted, T.ll_set)) return false;
    return build_table(T.lens + nlen, (int)nd, kDists, kDBits, T.d, T.d_sorted, T.d_set);
}

// ---- the sinks (what each adds: the file header) -----------------------------------------------------------------------------
// reach(s, o): how far back a match at output offset o may reach; at(s, q): the element at index q from out[0], q >= -reach.
struct LengthsOnly { static constexpr bool kStores = false; };
struct ByteSink { static constexpr bool kStores = true; uint8_t *out; };
struct ElemSink { static constexpr bool kStores = true; uint16_t *out; uint32_t abs0; };      // abs0: bytes of the stream before out[0]
__device__ __forceinline__ uint32_t reach(const ByteSink &, uint32_t o) { return o; }
__device__ __forceinline__ uint32_t reach(const ElemSink &s, uint32_t o) { return s.abs0 + o; }
__device__ __forceinline__ uint8_t at(const ByteSink &s, int q) { return s.out[q]; }
__device__ __forceinline__ uint16_t at(const ElemSink &s, int q) { return q >= 0 ? s.out[q] : (uint16_t)(kMarker | (uint32_t)(-q - 1)); }

// A round's tokens (T.tlen, T.tval, T.tout; lane i has written token i) into the sink: literals by their lanes, then the
// matches one after the other with the lanes across their elements (distance < length: a period of `distance`).  A match
// whose source may hold elements of a match written since the last barrier waits for them.
template <class S> __device__ __forceinline__ void write_round(Tables &T, const S &sink, uint32_t ntok)
{
    const uint32_t lane = threadIdx.x;
    __syncthreads();
    if (lane < ntok && T.tlen[lane] == 1) sink.out[T.tout[lane]] = T.tval[lane];
    __syncthreads();
    uint32_t dirty = kNone;
    for (uint32_t i = 0; i < ntok; ++i) {
        const uint32_t ml = T.tlen[i];
        if (ml == 1u) continue;
        const uint32_t dist = T.tval[i], to = T.tout[i];
        const int s0 = (int)to - (int)dist;                  // >= -reach(to)
        if (dirty != kNone && s0 + (int)min(ml, dist) > (int)dirty) { __syncthreads(); dirty = kNone; }
        for (uint32_t j = lane; j < ml; j += 64u) sink.out[to + j] = at(sink, s0 + (int)(dist >= ml ? j : j % dist));   // index < to
        dirty = min(dirty, to);
    }
    __syncthreads();
}

// What a run did.  ok: whole blocks were decoded up to `end`; then nbytes were produced, the last block was final (adler_pos:
// the byte behind it, where the Adler-32 lies) or not, and last_empty says whether it was a stored block of length 0.
// maxdist, the largest distance a storing sink has taken, also stands after a failure; so does adler_pos once it is set.
struct InflateRun { uint32_t end, nbytes, adler_pos, maxdist; bool ok, final_blk, last_empty; };

// Whole blocks from the block header at bit `pos` of the input src[a0, a0 + len) up to the first block boundary at or behind bit
// `stop` (kNone: no stop), or through the final block, which needs four bytes behind it; at most `win` bytes.
template <class S>
__device__ __forceinline__ InflateRun inflate_run(Tables &T, const uint8_t *src, uint32_t a0, uint32_t len, uint32_t pos, uint32_t stop,
                                                  const S sink, uint32_t win)
{
    const uint32_t lane = threadIdx.x, lenbits = len * 8u;
    InflateRun r{0u, 0u, 0u, 0u, false, false, false};
    uint32_t o = 0;
    bool last_empty = false;
    for (;;) {
        uint32_t v = peek32(src, a0, len, pos);
        const bool final_blk = v & 1u;
        const uint32_t type = (v >> 1) & 3u;
        pos += 3u;
        if (pos > lenbits || type == 3u) return r;
        if (type == 0u) {
            pos = (pos + 7u) & ~7u;
            if (pos + 32u > lenbits) return r;
            v = peek32(src, a0, len, pos);
            const uint32_t L = v & 0xFFFFu;
            pos += 32u;
            const uint32_t by = pos >> 3;
            if ((L ^ 0xFFFFu) != (v >> 16) || L > len - by || L > win - o) return r;
            if constexpr (S::kStores) {
                for (uint32_t j = lane; j < L; j += 64u) sink.out[o + j] = src[a0 + by + j];
                __syncthreads();
            }
            o += L; pos += L * 8u;
            last_empty = L == 0u;
        } else {
            if (type == 1u) {
                for (uint32_t i = lane; i < (uint32_t)(kFixedLL + kFixedDist); i += 64u) T.lens[i] = (uint8_t)fixed_len((int)i);
                __syncthreads();
                build_table(T.lens, kFixedLL, kLens, kLLBits, T.ll, T.ll_sorted, T.ll_set);
                build_table(T.lens + kFixedLL, kFixedDist, kDists, kDBits, T.d, T.d_sorted, T.d_set);
            } else if (!dynamic_header(T, src, a0, len, pos)) return r;
            for (bool eob = false; !eob;) {
                // a round: every lane decodes its tokens, lane i keeps token i in LDS with its output offset (the running sum
                // of the token lengths), up to kRound of them; a sink that stores nothing takes the whole block
                uint32_t ntok = 0, o_r = o;
                while (!S::kStores || ntok < (uint32_t)kRound) {
                    uint32_t l, sym;
                    v = peek32(src, a0, len, pos);
                    if (!decode_sym(T.ll, kLLBits, T.ll_set, T.ll_sorted, v, l, sym)) return r;
                    pos += l;
                    if (sym < 256u) {
                        if (o_r >= win) return r;
                        if constexpr (S::kStores)
                            if (lane == ntok) { T.tlen[lane] = 1; T.tval[lane] = (uint16_t)sym; T.tout[lane] = o_r; }
                        ++ntok; ++o_r;
                    } else if (sym == 256u) { eob = true; break; }
                    else {
                        if (sym >= (uint32_t)kMaxLL) return r;
                        const uint32_t idx = sym - 257u, eb = length_extra(idx);
                        const uint32_t mlen = length_base(idx) + ((v >> l) & ((1u << eb) - 1u));      // l + eb <= 20 bits of v
                        pos += eb;
                        v = peek32(src, a0, len, pos);
                        uint32_t l2, dsym;
                        if (!decode_sym(T.d, kDBits, T.d_set, T.d_sorted, v, l2, dsym) || dsym >= (uint32_t)kMaxDist) return r;
                        const uint32_t de = dist_extra(dsym), dist = dist_base(dsym) + ((v >> l2) & ((1u << de) - 1u));   // l2 + de <= 28; <= 32768
                        pos += l2 + de;
                        if (mlen > win - o_r) return r;
                        if constexpr (S::kStores) {
                            if (dist > reach(sink, o_r)) return r;
                            r.maxdist = max(r.maxdist, dist);
                            if (lane == ntok) { T.tlen[lane] = (uint16_t)mlen; T.tval[lane] = (uint16_t)dist; T.tout[lane] = o_r; }
                        }
                        ++ntok; o_r += mlen;
                    }
                    if (pos > lenbits) return r;
                }
                if (pos > lenbits) return r;
                if constexpr (S::kStores) write_round(T, sink, ntok);
                o = o_r;
            }
            last_empty = false;
        }
        // a block boundary
        if (final_blk) {
            pos = (pos + 7u) & ~7u;
            r.adler_pos = pos >> 3;
            if (r.adler_pos + 4u > len) return r;            // the Adler-32 follows the last block
            r.final_blk = true;
            break;
        }
        if (pos >= stop) break;
    }
    r.ok = true; r.end = pos; r.nbytes = o; r.last_empty = last_empty;
    return r;
}

}  // namespace uwip_inflate
