// The Annex K tables of baseline JPEG (ITU-T T.81) -- the zig-zag order, the two quantisation tables, the four standard
// Huffman tables -- and what every encoder here derives from them: the quantisers of a quality, the codes of a table, the
// header of a stream.  The one copy: the host codec of the CLIs (cli/jpeg.hpp) and the device codec (jpeg_encode.hip,
// jpeg_parse.hpp) both read these.
#pragma once
#include <cassert>
#include <cstddef>
#include <cstdint>

// the zig-zag order as an initialiser: device code cannot index a namespace-scope host array at run time, so a kernel keeps
// a function-local constexpr array initialised from this
#define UWIP_JPEG_ZIGZAG_INIT                                                                                                  \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

namespace uwip_jpeg {

static const uint8_t ZIGZAG[64] = UWIP_JPEG_ZIGZAG_INIT;

static const uint8_t STD_LUM_Q[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                      69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                      81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92, 95,  98,  112, 100, 103, 99};
static const uint8_t STD_CHR_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                      99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
static const uint8_t DC_LUM_BITS[17] = {0, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t DC_CHR_BITS[17] = {0, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t AC_LUM_BITS[17] = {0, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t AC_LUM_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
static const uint8_t AC_CHR_BITS[17] = {0, 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t AC_CHR_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// (code | size << 16) of every symbol of a table given as BITS / HUFFVAL (T.81 Annex C: codes of one length count up, a longer
// length continues from the doubled next code); a symbol the table does not hold stays 0
inline void build_codes(const uint8_t *bits, const uint8_t *vals, uint32_t *out256)
{
    for (int i = 0; i < 256; ++i) out256[i] = 0;
    uint32_t code = 0;
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l]; ++i, ++p) out256[vals[p]] = code++ | ((uint32_t)l << 16);
        code <<= 1;
    }
}

// the two quantisation tables (luma, chroma; natural order) at a quality of 1..100 (clamped), libjpeg's jpeg_set_quality
inline void scaled_quant(int quality, uint8_t q[2][64])
{
    quality = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int a = (STD_LUM_Q[i] * scale + 50) / 100, b = (STD_CHR_Q[i] * scale + 50) / 100;
        q[0][i] = (uint8_t)(a < 1 ? 1 : (a > 255 ? 255 : a));
        q[1][i] = (uint8_t)(b < 1 ? 1 : (b > 255 ? 255 : b));
    }
}

// SOI .. SOS of a stream of nc components (1: grey; 3: YCbCr 4:2:0), stated on its own
constexpr size_t header_bytes(int nc) { return nc == 3 ? 623 : 328; }

// Writes SOI, APP0 (JFIF), DQT, SOF0, DHT (the standard tables) and SOS into h, which holds header_bytes(nc); returns the length.
inline size_t write_header(int rows, int cols, int nc, const uint8_t q[2][64], uint8_t *h)
{
    size_t n = 0;
    auto put = [&](int v) { h[n++] = (uint8_t)v; };
    auto w16 = [&](int v) { put(v >> 8); put(v); };
    put(0xFF); put(0xD8);
    static const uint8_t jfif[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (uint8_t v : jfif) put(v);
    for (int t = 0; t < (nc == 3 ? 2 : 1); ++t) {
        put(0xFF); put(0xDB); w16(67); put(t);
        for (int i = 0; i < 64; ++i) put(q[t][ZIGZAG[i]]);
    }
    const int hs = nc == 3 ? 2 : 1;
    put(0xFF); put(0xC0); w16(8 + 3 * nc); put(8); w16(rows); w16(cols); put(nc);
    for (int i = 0; i < nc; ++i) { put(i + 1); put(i == 0 ? (hs << 4 | hs) : 0x11); put(i ? 1 : 0); }
    auto dht = [&](int cls_id, const uint8_t *bits, const uint8_t *vals, int cnt) {
        put(0xFF); put(0xC4); w16(19 + cnt); put(cls_id);
        for (int i = 1; i < 17; ++i) put(bits[i]);
        for (int i = 0; i < cnt; ++i) put(vals[i]);
    };
    dht(0x00, DC_LUM_BITS, DC_VALS, 12); dht(0x10, AC_LUM_BITS, AC_LUM_VALS, 162);
    if (nc == 3) { dht(0x01, DC_CHR_BITS, DC_VALS, 12); dht(0x11, AC_CHR_BITS, AC_CHR_VALS, 162); }
    put(0xFF); put(0xDA); w16(6 + 2 * nc); put(nc);
    for (int i = 0; i < nc; ++i) { put(i + 1); put(i ? 0x11 : 0x00); }
    put(0); put(63); put(0);
    assert(n == header_bytes(nc));
    return n;
}

}  // namespace uwip_jpeg
