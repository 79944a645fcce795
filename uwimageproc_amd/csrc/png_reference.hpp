// uwip_png::encode_host_reference: the PNG stream uwip_png_encode writes, by a plain serial loop over deflate_core.hpp.  It
// exists for the emulation harness (tests/png_encode_emulated.cpp) and cli/pngenc_check to compare bytes against and to
// measure sizes without a device; it is NOT a fallback behind the C ABI.  Host only.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "deflate_core.hpp"

namespace uwip_png {

// the filtered bytes of a frame (rows x (1 + cols * nc)): BGR in, RGB out; filter -1 = per row the type 0..4 with the smallest
// sum of min(v, 256 - v), ties to the lowest type, the row above row 0 taken as zeros
inline void filter_host_reference(const uint8_t *img, int rows, int cols, int nc, size_t step, int filter, std::vector<uint8_t> &out)
{
    const int rb = cols * nc;
    out.assign((size_t)rows * (rb + 1), 0);
    auto sample = [&](const uint8_t *r, int i) -> int {
        if (!r || i < 0) return 0;
        return nc == 3 ? r[i - i % 3 + (2 - i % 3)] : r[i];
    };
    for (int y = 0; y < rows; ++y) {
        const uint8_t *row = img + (size_t)y * step, *up = y ? row - step : nullptr;
        int type = filter;
        if (filter < 0) {
            uint64_t best = 0;
            for (int ty = 0; ty < 5; ++ty) {
                uint64_t cost = 0;
                for (int i = 0; i < rb; ++i)
                    cost += filter_cost(filter_byte(ty, sample(row, i), sample(row, i - nc), sample(up, i), sample(up, i - nc)));
                if (ty == 0 || cost < best) { best = cost; type = ty; }
            }
        }
        uint8_t *dst = &out[(size_t)y * (rb + 1)];
        dst[0] = (uint8_t)type;
        for (int i = 0; i < rb; ++i) dst[1 + i] = filter_byte(type, sample(row, i), sample(row, i - nc), sample(up, i), sample(up, i - nc));
    }
}

// the IDAT payload of chunk c (n bytes at d): the zlib header in front of the first, the block, the empty stored block behind
// every chunk but the last
inline void deflate_chunk_reference(const uint8_t *d, int n, bool first, bool last, std::vector<uint8_t> &payload)
{
    static Codes codes;
    static Scratch scr;
    uint32_t freq[kNumLL] = {0}, nmatch = 0;
    freq[kEOB] = 1;
    auto tokens = [&](auto &&tok) {
        for (int p = 0; p < n;) {
            int q = p + 1;
            while (q < n && d[q] == d[p]) ++q;
            for (int k = 0; k < q - p; ++k) { const int t = rle_token(k, q - p); if (t) tok(t, d[p]); }
            p = q;
        }
    };
    tokens([&](int len, int byte) {
        if (len == 1) { freq[byte]++; return; }
        int sym, nx; uint32_t ex;
        length_symbol(len, sym, nx, ex);
        freq[sym]++; nmatch++;
    });
    const int m = huff_sort(freq, kNumLL, scr.order);
    plan_block(freq, nmatch, n, m, scr, codes);
    const uint32_t hdr0 = first ? 2 : 0;
    std::vector<uint32_t> win((hdr0 + 5 + n + 5 + 3) / 4 + 2, 0u);
    uint8_t *wb = reinterpret_cast<uint8_t *>(win.data());
    if (first) { wb[0] = 0x78; wb[1] = 0x01; }
    uint32_t end_bits;
    if (codes.mode == kStored) {
        wb[hdr0] = last ? 1 : 0;
        wb[hdr0 + 1] = (uint8_t)n; wb[hdr0 + 2] = (uint8_t)(n >> 8); wb[hdr0 + 3] = (uint8_t)~n; wb[hdr0 + 4] = (uint8_t)(~n >> 8);
        std::memcpy(wb + hdr0 + 5, d, (size_t)n);
        end_bits = (hdr0 + 5 + n) * 8;
    } else {
        auto orw = [](uint32_t *p, uint32_t v) { *p |= v; };
        BitSink<decltype(orw)> sink(win.data(), hdr0 * 8, orw);
        auto put = [&](uint32_t v, int nb) { sink.put(v, nb); };
        put_block_header(codes, last, put);
        tokens([&](int len, int byte) { put_token(codes, len, byte, put); });
        put(codes.ll[kEOB] & 0xffffu, (int)(codes.ll[kEOB] >> 16));
        sink.flush();
        end_bits = hdr0 * 8 + codes.hdr_bits + codes.data_bits;
    }
    uint32_t len = (end_bits + 7) / 8;
    if (!last) { len = (end_bits + 3 + 7) / 8 + 4; wb[len - 2] = 0xff; wb[len - 1] = 0xff; }
    payload.assign(wb, wb + len);
}

inline void encode_host_reference(const uint8_t *img, int rows, int cols, int nc, size_t step, int filter, std::vector<uint8_t> &out)
{
    std::vector<uint8_t> filt, payload;
    filter_host_reference(img, rows, cols, nc, step, filter, filt);
    out.resize(kHeadBytes);
    write_head(rows, cols, nc, out.data());
    const uint64_t nch = chunks_of(filt.size());
    uint32_t A = 1, B = 0;
    for (uint64_t c = 0; c < nch; ++c) {
        const uint8_t *d = &filt[c * kChunk];
        const int n = (int)std::min<uint64_t>(kChunk, filt.size() - c * kChunk);
        uint32_t a = 0, b = 0;
        for (int i = 0; i < n; ++i) { a = (a + d[i]) % kAdlerMod; b = (uint32_t)((b + (uint64_t)(n - i) * d[i]) % kAdlerMod); }
        adler_append(A, B, a, b, (uint32_t)n);
        deflate_chunk_reference(d, n, c == 0, c + 1 == nch, payload);
        uint8_t h[8];
        put_be32(h, (uint32_t)payload.size());
        std::memcpy(h + 4, "IDAT", 4);
        out.insert(out.end(), h, h + 8);
        out.insert(out.end(), payload.begin(), payload.end());
        uint32_t s = crc_idat_state();
        for (uint8_t v : payload) s = crc_byte(s, v);
        put_be32(h, s ^ 0xffffffffu);
        out.insert(out.end(), h, h + 4);
    }
    uint8_t tail[kTailBytes];
    write_tail((B << 16) | A, tail);
    out.insert(out.end(), tail, tail + kTailBytes);
}

}  // namespace uwip_png
