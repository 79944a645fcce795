// Baseline JPEG (SOF0 / SOF1, 8-bit, Huffman; grey or YCbCr with 1x1 / 2x1 / 2x2 chroma subsampling, restart
// intervals) for the CLIs: the reference reads its test photographs and writes its key frames as .jpg through OpenCV
// (modules/bgdehaze/main.py:16,19; modules/videostrip/src/main.cpp:294,377), and the build image has no codec headers.
//
// The decoder follows the published IJG / libjpeg(-turbo) algorithms step for step so that it returns the pixels
// cv::imread / Pillow return: "islow" integer IDCT (jidctint), "fancy" triangle chroma upsampling (jdsample
// h2v1 / h2v2_fancy_upsample), fixed-point YCbCr -> RGB (jdcolor).  tests/test_cli.py checks it bit for bit against
// Pillow's decode of the reference's four JPEG files.  The encoder is the baseline encoder of the same library:
// RGB -> YCbCr (jccolor), 2x2 chroma downsampling (jcsample), islow forward DCT (jfdctint), the Annex K tables scaled by
// quality (cv::imwrite's default: 95), the standard Huffman tables.  Pixels are BGR-interleaved (cv::Mat), or 1 channel.
//
// What the device codec of the library must do identically is stated once, in uwimageproc_amd/csrc/, and used from here: the
// Annex K tables, the quantiser scaling, the header writer and the encoder's Huffman codes (jpeg_tables.hpp), the header
// parse with the decoder's Huffman tables (jpeg_parse.hpp), one pass of each DCT and the scalar helpers (jpeg_core.hpp).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "jpeg_core.hpp"
#include "jpeg_parse.hpp"
#include "jpeg_tables.hpp"

namespace jpeg {

using namespace uwip_jpeg;

// ---- the slow-but-accurate integer DCT pair (CONST_BITS 13, PASS1_BITS 2): the passes of jpeg_core.hpp over a block ----------
enum { CB = 13, P1 = 2 };

// coef: 64 dequantised coefficients in natural order (|coef| <= 2^20, the decoder clamps: a valid stream stays far
// below); out: 64 samples 0..255
static inline void idct_islow(const int32_t *coef, uint8_t *out, int ostride)
{
    int64_t ws[64], in[8], o[8];
    for (int c = 0; c < 8; ++c) {
        for (int r = 0; r < 8; ++r) in[r] = coef[r * 8 + c];
        idct_pass(in, o);
        for (int r = 0; r < 8; ++r) ws[r * 8 + c] = descale64(o[r], CB - P1);
    }
    for (int r = 0; r < 8; ++r) {
        idct_pass(ws + r * 8, o);
        for (int i = 0; i < 8; ++i) {
            const int64_t s = descale64(o[i], CB + P1 + 3) + 128;
            out[r * ostride + i] = (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
        }
    }
}

// d: 64 samples - 128 in natural order -> 64 coefficients scaled by 8 (jfdctint)
static inline void fdct_islow(int32_t *d)
{
    for (int r = 0; r < 8; ++r) fdct_pass(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7], true);
    for (int c = 0; c < 8; ++c) fdct_pass(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c], false);
}

// ---- decoder ---------------------------------------------------------------------------------------------------------
struct BitReader {
    const uint8_t *p, *end;
    uint32_t acc = 0;
    int nbits = 0;
    bool hit_marker = false;
    void fill()
    {
        while (nbits <= 24) {
            int c = 0;
            if (!hit_marker && p < end) {
                c = *p++;
                if (c == 0xFF) {
                    if (p < end && *p == 0) ++p;
                    else { hit_marker = true; --p; c = 0; }     // a marker: feed zeros, leave it for the caller
                }
            }
            acc |= (uint32_t)c << (24 - nbits);
            nbits += 8;
        }
    }
    int peek(int n) { if (nbits < n) fill(); return (int)(acc >> (32 - n)); }
    void skip(int n) { acc <<= n; nbits -= n; }
    int get(int n) { if (n == 0) return 0; const int v = peek(n); skip(n); return v; }
    void reset() { acc = 0; nbits = 0; hit_marker = false; }
};

static inline int huff_decode(BitReader &br, const DecHuff &h)
{
    const int look = br.peek(9);
    const uint16_t e = h.lookup[look];
    if (e) { br.skip(e >> 8); return e & 255; }
    int code = br.peek(16), l = 10;
    for (; l <= 16; ++l) if ((code >> (16 - l)) <= h.maxcode[l]) break;
    if (l > 16) return -1;
    br.skip(l);
    const int idx = h.valptr[l] + (code >> (16 - l));
    return (idx >= 0 && idx < 256) ? h.vals[idx] : -1;
}

// Returns BGR (channels = 3) or grey (channels = 1, unless force_color) pixels.
inline bool decode(const uint8_t *buf, size_t len, int &rows, int &cols, int &channels, std::vector<uint8_t> &pix, bool force_color)
{
    DecFrame d{};                    // the header: geometry, quantisers and Huffman tables per component
    size_t seg = 0;
    if (parse(buf, len, nullptr, nullptr, nullptr, &d, &seg) == PARSE_BAD) return false;      // PARSE_HOST_ONLY (1x2) decodes here
    const int W = d.W, H = d.H, ncomp = d.ncomp, hmax = d.hmax, vmax = d.vmax;
    std::vector<uint8_t> plane[3];       // per component, MCU-padded: cwb*8 x chb*8
    int pred[3] = {0, 0, 0};
    for (int c = 0; c < ncomp; ++c) plane[c].assign((size_t)d.cwb[c] * 8 * d.chb[c] * 8, 0);
    // ---- the entropy-coded segment
    BitReader br{buf + seg, buf + len};
    int count = 0;
    for (int my = 0; my < d.mcuy; ++my)
        for (int mx = 0; mx < d.mcux; ++mx) {
            if (count == d.ri) {             // never without restarts: d.ri is then the MCU count
                // expect RSTn at the byte position; resynchronise
                br.reset();
                while (br.p + 1 < br.end && !(br.p[0] == 0xFF && br.p[1] >= 0xD0 && br.p[1] <= 0xD7)) ++br.p;
                if (br.p + 1 < br.end) br.p += 2;
                for (int c = 0; c < ncomp; ++c) pred[c] = 0;
                count = 0;
            }
            ++count;
            for (int c = 0; c < ncomp; ++c)
                for (int by = 0; by < d.cv[c]; ++by)
                    for (int bx = 0; bx < d.ch[c]; ++bx) {
                        int32_t blk[64] = {0};
                        const uint16_t *qt = d.qt[c];
                        const int t = huff_decode(br, d.dc[c]);
                        if (t < 0 || t > 11) return false;
                        const int diff = t ? extend(br.get(t), t) : 0;
                        pred[c] += diff;
                        if (pred[c] > 32767 || pred[c] < -32768) return false;     // a valid DC stays within 12 bits
                        blk[0] = (int32_t)clamp_coef((int64_t)pred[c] * qt[0]);
                        for (int k = 1; k < 64;) {
                            const int rs = huff_decode(br, d.ac[c]);
                            if (rs < 0) return false;
                            const int r = rs >> 4, sz = rs & 15;
                            if (sz == 0) { if (r == 15) { k += 16; continue; } break; }
                            k += r;
                            if (k > 63) return false;
                            const int z = ZIGZAG[k];
                            blk[z] = (int32_t)clamp_coef((int64_t)extend(br.get(sz), sz) * qt[z]);
                            ++k;
                        }
                        const int X = (mx * d.ch[c] + bx) * 8, Y = (my * d.cv[c] + by) * 8, stride = d.cwb[c] * 8;
                        idct_islow(blk, &plane[c][(size_t)Y * stride + X], stride);
                    }
        }
    rows = H; cols = W;
    // ---- upsample (fancy, as libjpeg's default) + colour
    auto samp = [&](int c, int x, int y) -> int {     // edge-replicated access inside the downsampled plane
        x = x < 0 ? 0 : (x >= d.cdw[c] ? d.cdw[c] - 1 : x);
        y = y < 0 ? 0 : (y >= d.cdh[c] ? d.cdh[c] - 1 : y);
        return plane[c][(size_t)y * d.cwb[c] * 8 + x];
    };
    auto full = [&](int c, std::vector<uint8_t> &o) {
        o.resize((size_t)W * H);
        const int hx = hmax / d.ch[c], vx = vmax / d.cv[c], dw = d.cdw[c];
        if (hx == 1 && vx == 1) {
            for (int y = 0; y < H; ++y) std::memcpy(&o[(size_t)y * W], &plane[c][(size_t)y * d.cwb[c] * 8], W);
        } else if (hx == 2 && vx == 1) {                      // h2v1_fancy_upsample
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < dw; ++x) {
                    const int s0 = samp(c, x, y);
                    int a, b;
                    if (dw == 1) { a = b = s0; }
                    else if (x == 0) { a = s0; b = (s0 * 3 + samp(c, 1, y) + 2) >> 2; }
                    else if (x == dw - 1) { a = (s0 * 3 + samp(c, x - 1, y) + 1) >> 2; b = s0; }
                    else { a = (s0 * 3 + samp(c, x - 1, y) + 1) >> 2; b = (s0 * 3 + samp(c, x + 1, y) + 2) >> 2; }
                    if (2 * x < W) o[(size_t)y * W + 2 * x] = (uint8_t)a;
                    if (2 * x + 1 < W) o[(size_t)y * W + 2 * x + 1] = (uint8_t)b;
                }
        } else if (hx == 2 && vx == 2) {                      // h2v2_fancy_upsample
            for (int y = 0; y < H; ++y) {
                const int y0 = y >> 1, y1 = (y & 1) ? y0 + 1 : y0 - 1;         // nearer row, farther row
                for (int x = 0; x < dw; ++x) {
                    const int thisc = samp(c, x, y0) * 3 + samp(c, x, y1);
                    int a, b;
                    if (dw == 1) { a = (thisc * 4 + 8) >> 4; b = (thisc * 4 + 7) >> 4; }
                    else {
                        const int lastc = samp(c, x - 1, y0) * 3 + samp(c, x - 1, y1), nextc = samp(c, x + 1, y0) * 3 + samp(c, x + 1, y1);
                        a = x == 0 ? (thisc * 4 + 8) >> 4 : (thisc * 3 + lastc + 8) >> 4;
                        b = x == dw - 1 ? (thisc * 4 + 7) >> 4 : (thisc * 3 + nextc + 7) >> 4;
                    }
                    if (2 * x < W) o[(size_t)y * W + 2 * x] = (uint8_t)a;
                    if (2 * x + 1 < W) o[(size_t)y * W + 2 * x + 1] = (uint8_t)b;
                }
            }
        } else {                                              // 1x2: replicate rows (h1v2 has no fancy form in libjpeg 6b)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) o[(size_t)y * W + x] = (uint8_t)samp(c, x / hx, y / vx);
        }
    };
    std::vector<uint8_t> Y, Cb, Cr;
    full(0, Y);
    if (ncomp == 1) {
        channels = force_color ? 3 : 1;
        pix.resize((size_t)W * H * channels);
        for (size_t i = 0; i < (size_t)W * H; ++i)
            if (channels == 1) pix[i] = Y[i];
            else pix[3 * i] = pix[3 * i + 1] = pix[3 * i + 2] = Y[i];
        return true;
    }
    full(1, Cb); full(2, Cr);
    channels = 3;
    pix.resize((size_t)W * H * 3);
    // jdcolor.c build_ycc_rgb_table: SCALEBITS 16
    // built once, thread-safe (C++11 function-local static: `videostrip -g N` decodes from N worker threads)
    struct YccTables {
        int32_t crr[256], cbb[256], crg[256], cbg[256];
        YccTables() {
            for (int i = 0; i < 256; ++i) {
                const int32_t x = i - 128;
                crr[i] = (int32_t)((91881LL * x + 32768) >> 16);           // FIX(1.40200)
                cbb[i] = (int32_t)((116130LL * x + 32768) >> 16);          // FIX(1.77200)
                crg[i] = (int32_t)(-46802LL * x);                          // FIX(0.71414)
                cbg[i] = (int32_t)(-22554LL * x + 32768);                  // FIX(0.34414) + ONE_HALF
            }
        }
    };
    static const YccTables tab;
    const int32_t *crr = tab.crr, *cbb = tab.cbb, *crg = tab.crg, *cbg = tab.cbg;
    auto clamp8 = [](int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const int y = Y[i], cb = Cb[i], cr = Cr[i];
        pix[3 * i + 2] = clamp8(y + crr[cr]);
        pix[3 * i + 1] = clamp8(y + ((cbg[cb] + crg[cr]) >> 16));
        pix[3 * i + 0] = clamp8(y + cbb[cb]);
    }
    return true;
}

// ---- encoder (baseline, 4:2:0 for colour, standard tables, quality as cv::imwrite: default 95) ----------------------
struct BitWriter {
    std::vector<uint8_t> &out;
    uint32_t acc = 0;
    int n = 0;
    void put(uint32_t code, int size)
    {
        acc = (acc << size) | (code & ((1u << size) - 1));
        n += size;
        while (n >= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            out.push_back(b);
            if (b == 0xFF) out.push_back(0);
            n -= 8;
        }
    }
    void code(uint32_t cs) { put(cs, (int)(cs >> 16)); }      // a symbol of build_codes: code | size << 16 (put masks the size off)
    void flush() { if (n) put(0x7F, 8 - n); }        // pad with ones
};

inline bool encode(const uint8_t *pix, int rows, int cols, int channels, int quality, std::vector<uint8_t> &out)
{
    if (rows <= 0 || cols <= 0 || (channels != 1 && channels != 3)) return false;
    uint8_t q[2][64];
    scaled_quant(quality, q);
    uint32_t dcl[256], dcc[256], acl[256], acc_[256];
    build_codes(DC_LUM_BITS, DC_VALS, dcl); build_codes(DC_CHR_BITS, DC_VALS, dcc);
    build_codes(AC_LUM_BITS, AC_LUM_VALS, acl); build_codes(AC_CHR_BITS, AC_CHR_VALS, acc_);
    const int nc = channels == 3 ? 3 : 1, hs = nc == 3 ? 2 : 1;
    const int mcu = 8 * hs, mcux = (cols + mcu - 1) / mcu, mcuy = (rows + mcu - 1) / mcu;
    const int PW = mcux * mcu, PH = mcuy * mcu;
    // colour conversion (jccolor.c rgb_ycc_convert) into edge-replicated planes
    std::vector<uint8_t> Y((size_t)PW * PH), Cb, Cr;
    if (nc == 3) { Cb.resize((size_t)PW * PH); Cr.resize((size_t)PW * PH); }
    for (int y = 0; y < PH; ++y)
        for (int x = 0; x < PW; ++x) {
            const uint8_t *p = pix + ((size_t)(y < rows ? y : rows - 1) * cols + (x < cols ? x : cols - 1)) * channels;
            if (nc == 1) { Y[(size_t)y * PW + x] = p[0]; continue; }
            const int b = p[0], g = p[1], r = p[2];
            Y[(size_t)y * PW + x] = (uint8_t)((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
            Cb[(size_t)y * PW + x] = (uint8_t)((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16);
            Cr[(size_t)y * PW + x] = (uint8_t)((32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16);
        }
    // h2v2_downsample: 2x2 box with the alternating 1, 2 bias
    std::vector<uint8_t> cb2, cr2;
    const int CW = PW / 2, CH = PH / 2;
    if (nc == 3) {
        cb2.resize((size_t)CW * CH); cr2.resize((size_t)CW * CH);
        for (int y = 0; y < CH; ++y)
            for (int x = 0; x < CW; ++x) {
                const int bias = 1 + (x & 1);
                auto box = [&](const std::vector<uint8_t> &P) {
                    return (uint8_t)((P[(size_t)(2 * y) * PW + 2 * x] + P[(size_t)(2 * y) * PW + 2 * x + 1] + P[(size_t)(2 * y + 1) * PW + 2 * x] +
                                      P[(size_t)(2 * y + 1) * PW + 2 * x + 1] + bias) >> 2);
                };
                cb2[(size_t)y * CW + x] = box(Cb); cr2[(size_t)y * CW + x] = box(Cr);
            }
    }
    out.resize(header_bytes(nc));
    out.resize(write_header(rows, cols, nc, q, out.data()));
    BitWriter bw{out};
    int pred[3] = {0, 0, 0};
    auto block = [&](const uint8_t *P, int stride, const uint8_t *qt, const uint32_t *D, const uint32_t *A, int &pr) {
        int32_t d[64];
        for (int y = 0; y < 8; ++y) for (int x = 0; x < 8; ++x) d[y * 8 + x] = (int32_t)P[(size_t)y * stride + x] - 128;
        fdct_islow(d);
        int zz[64];
        for (int i = 0; i < 64; ++i) {
            const int z = ZIGZAG[i];
            const int32_t qv = (int32_t)qt[z] << 3;
            int32_t t = d[z];
            if (t < 0) { t = -t; t += qv >> 1; t = t >= qv ? t / qv : 0; t = -t; }
            else { t += qv >> 1; t = t >= qv ? t / qv : 0; }
            zz[i] = t;
        }
        int diff = zz[0] - pr;
        pr = zz[0];
        int t = diff < 0 ? -diff : diff, nb = 0;
        while (t) { nb++; t >>= 1; }
        bw.code(D[nb]);
        if (nb) bw.put((uint32_t)(diff < 0 ? diff - 1 : diff), nb);
        int run = 0;
        for (int k = 1; k < 64; ++k) {
            int v = zz[k];
            if (v == 0) { run++; continue; }
            while (run > 15) { bw.code(A[0xF0]); run -= 16; }
            int a = v < 0 ? -v : v, n2 = 0;
            while (a) { n2++; a >>= 1; }
            const int sym = (run << 4) | n2;
            bw.code(A[sym]);
            bw.put((uint32_t)(v < 0 ? v - 1 : v), n2);
            run = 0;
        }
        if (run) bw.code(A[0]);
    };
    for (int my = 0; my < mcuy; ++my)
        for (int mx = 0; mx < mcux; ++mx) {
            for (int by = 0; by < hs; ++by)
                for (int bx = 0; bx < hs; ++bx)
                    block(&Y[(size_t)(my * mcu + by * 8) * PW + mx * mcu + bx * 8], PW, q[0], dcl, acl, pred[0]);
            if (nc == 3) {
                block(&cb2[(size_t)(my * 8) * CW + mx * 8], CW, q[1], dcc, acc_, pred[1]);
                block(&cr2[(size_t)(my * 8) * CW + mx * 8], CW, q[1], dcc, acc_, pred[2]);
            }
        }
    bw.flush();
    out.push_back(0xFF); out.push_back(0xD9);
    return true;
}

}  // namespace jpeg
