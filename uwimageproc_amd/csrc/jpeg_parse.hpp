// The header parse of baseline JPEG, the one copy: SOI .. SOS into the per-frame descriptor that the kernels of the device
// decoder (jpeg_decode.hip) read and that the host decoder of the CLIs (jpeg::decode, cli/jpeg.hpp) decodes from.  Host-only,
// no device needed: uwip_jpeg_info is this parse alone, and tests/jpeg_decode_emulated.cpp feeds the kernels, run on host
// threads, from it.
#pragma once
#include <cstdint>
#include <cstring>
#include "jpeg_tables.hpp"

namespace uwip_jpeg {

// one Huffman table as the decoders read it: 9-bit look-ahead, (length << 8) | symbol, 0 = a longer code; maxcode[l] /
// valptr[l] for l = 10..16 (index 0 unused)
struct DecHuff {
    uint16_t lookup[512];
    int32_t maxcode[17];
    int32_t valptr[17];
    uint8_t vals[256];
};

struct DecFrame {
    int32_t status;                 // what the host parse decided: 0, or one of UWIP_JPEG_*
    int32_t W, H, ncomp, hmax, vmax, mcux, mcuy, nmcu;
    int32_t bpm;                    // blocks per MCU
    int32_t ri, nint;               // MCUs per restart interval (nmcu without DRI), intervals
    int32_t ch[3], cv[3];           // sampling factors
    int32_t cwb[3], chb[3];         // MCU-padded plane size in blocks
    int32_t cdw[3], cdh[3];         // downsampled size in samples
    int32_t coff[3];                // first block of the component inside an MCU
    uint32_t seg_off, seg_len;      // the entropy-coded segment (everything behind SOS) in the uploaded bytes
    uint32_t ubase;                 // the frame's unstuffed bytes
    uint32_t ibase;                 // its first interval (interval arrays hold nint + 1 entries per frame)
    uint32_t sbase, scap;           // its first subsequence; how many it may have
    uint32_t bbase;                 // its first coefficient block
    uint32_t pbase[3];              // its component planes
    uint32_t reserved;              // keeps sizeof(DecFrame) a multiple of 16
    uint16_t qt[3][64];             // quantisers per component, natural order
    DecHuff dc[3], ac[3];           // tables per component
};

// a table as DHT gives it, and the decoding tables built from it (T.81 Annex C, F.2.2.3)
struct HuffSpec {
    uint8_t bits[17] = {0}, vals[256] = {0};
    bool present = false;
    int32_t maxcode[18], valptr[17];
    uint16_t lookup[512];
    // false: the counts do not describe a prefix code (over-subscribed lengths, libjpeg's JERR_BAD_HUFF_TABLE)
    bool build()
    {
        present = false;
        uint8_t huffsize[257];
        uint16_t huffcode[257];
        int p = 0;
        for (int l = 1; l <= 16; ++l) for (int i = 0; i < bits[l]; ++i) { if (p >= 256) return false; huffsize[p++] = (uint8_t)l; }
        huffsize[p] = 0;
        int code = 0, si = huffsize[0];
        p = 0;
        while (huffsize[p]) {
            while (huffsize[p] == si) huffcode[p++] = (uint16_t)code++;
            if (code >= (1 << si)) return false;     // more codes of length si than the prefix tree has room for
            code <<= 1; si++;
        }
        p = 0;
        for (int l = 1; l <= 16; ++l) {
            valptr[l] = 0;
            if (bits[l]) { valptr[l] = p - (int)huffcode[p]; p += bits[l]; maxcode[l] = huffcode[p - 1]; }
            else maxcode[l] = -1;
        }
        maxcode[17] = 0xFFFFF;
        std::memset(lookup, 0, sizeof lookup);
        p = 0;
        for (int l = 1; l <= 9; ++l)
            for (int i = 0; i < bits[l]; ++i, ++p) {
                const int first = huffcode[p] << (9 - l);
                for (int k = 0; k < (1 << (9 - l)); ++k) lookup[first + k] = (uint16_t)((l << 8) | vals[p]);
            }
        present = true;
        return true;
    }
    void to(DecHuff &d) const
    {
        std::memcpy(d.lookup, lookup, sizeof lookup);
        d.maxcode[0] = -1; d.valptr[0] = 0;
        for (int l = 1; l <= 16; ++l) { d.maxcode[l] = maxcode[l]; d.valptr[l] = valptr[l]; }
        std::memcpy(d.vals, vals, 256);
    }
};

inline void std_spec(HuffSpec &t, const uint8_t *bits, const uint8_t *vals, int n)
{
    std::memcpy(t.bits, bits, 17);
    std::memcpy(t.vals, vals, n);
    t.build();
}

enum { PARSE_OK = 0, PARSE_BAD = -1, PARSE_HOST_ONLY = -3 };       // the values of UWIP_JPEG_BAD_STREAM / _HOST_ONLY

// The walk from SOI to the end of SOS.  PARSE_BAD: not the baseline both decoders read (SOF0 / SOF1, 8 bit, 1 or 3 components
// with sampling factors 1 or 2 and at most 10 blocks per MCU, one scan of all components), a malformed segment, a table the
// scan names but no DHT or default gives, or no scan at all.  The factors of a single component, any of 1..4, are taken as
// 1x1.  On PARSE_OK / PARSE_HOST_ONLY (1x2 sampling: the host decoder alone upsamples it) the geometry, the quantisers and
// the tables of `d` are filled in and the entropy-coded segment is buf[*seg .. len).  `d` may be null (uwip_jpeg_info:
// sizes only).
inline int parse(const uint8_t *buf, size_t len, int *rows, int *cols, int *channels, DecFrame *d, size_t *seg)
{
    if (!buf || len < 4 || buf[0] != 0xFF || buf[1] != 0xD8) return PARSE_BAD;
    uint16_t qt[4][64] = {{0}};
    HuffSpec dc[4], ac[4];
    // Motion-JPEG frames may omit DHT: the standard tables apply (overridden by any DHT)
    std_spec(dc[0], DC_LUM_BITS, DC_VALS, 12); std_spec(ac[0], AC_LUM_BITS, AC_LUM_VALS, 162);
    std_spec(dc[1], DC_CHR_BITS, DC_VALS, 12); std_spec(ac[1], AC_CHR_BITS, AC_CHR_VALS, 162);
    struct Comp { int id, h, v, tq, td, ta; } comp[3] = {};
    int ncomp = 0, W = 0, H = 0, restart = 0, hmax = 1, vmax = 1;
    size_t pos = 2;
    bool have_sof = false;
    while (pos + 4 <= len) {
        if (buf[pos] != 0xFF) { ++pos; continue; }
        const int m = buf[pos + 1];
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0xFF) { if (m == 0xFF) --pos; continue; }
        if (m == 0xD9) break;
        if (pos + 2 > len) return PARSE_BAD;
        const size_t L = ((size_t)buf[pos] << 8) | buf[pos + 1];
        if (L < 2 || pos + L > len) return PARSE_BAD;
        const uint8_t *s = buf + pos + 2, *e = buf + pos + L;
        if (m == 0xDB) {
            while (s < e) {
                const int pq = s[0] >> 4, tq = s[0] & 15;
                ++s;
                if (tq > 3 || s + (pq ? 128 : 64) > e) return PARSE_BAD;
                for (int i = 0; i < 64; ++i) { qt[tq][ZIGZAG[i]] = pq ? (uint16_t)((s[0] << 8) | s[1]) : s[0]; s += pq ? 2 : 1; }
            }
        } else if (m == 0xC4) {
            while (s + 17 <= e) {
                const int tc = s[0] >> 4, th = s[0] & 15;
                if (th > 3) return PARSE_BAD;
                HuffSpec &t = tc ? ac[th] : dc[th];
                int n = 0;
                t.bits[0] = 0;
                for (int i = 1; i <= 16; ++i) { t.bits[i] = s[i]; n += s[i]; }
                s += 17;
                if (n > 256 || s + n > e) return PARSE_BAD;
                std::memcpy(t.vals, s, n);
                s += n;
                if (!t.build()) return PARSE_BAD;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (L < 8 || s[0] != 8) return PARSE_BAD;
            H = (s[1] << 8) | s[2]; W = (s[3] << 8) | s[4];
            const int n = s[5];
            if ((n != 1 && n != 3) || W <= 0 || H <= 0 || L < (size_t)(8 + 3 * n)) return PARSE_BAD;
            if (have_sof) return PARSE_BAD;             // one frame per file
            ncomp = n;
            for (int i = 0; i < n; ++i) {
                comp[i].id = s[6 + 3 * i]; comp[i].h = s[7 + 3 * i] >> 4; comp[i].v = s[7 + 3 * i] & 15; comp[i].tq = s[8 + 3 * i] & 3;
                comp[i].td = comp[i].ta = 0;
                // a one-component scan is not interleaved (T.81 A.2.2): one block per MCU, in raster order over ceil(W / 8) x
                // ceil(H / 8) blocks, whatever factors SOF gives the component -- any the format can write (1..4) are read
                // as 1x1, as libjpeg does
                if (n == 1 && comp[0].h >= 1 && comp[0].h <= 4 && comp[0].v >= 1 && comp[0].v <= 4) comp[0].h = comp[0].v = 1;
                if (comp[i].h < 1 || comp[i].h > 2 || comp[i].v < 1 || comp[i].v > 2) return PARSE_BAD;
                hmax = comp[i].h > hmax ? comp[i].h : hmax; vmax = comp[i].v > vmax ? comp[i].v : vmax;
            }
            // T.81 B.2.3: at most 10 blocks in an MCU (three components all 2x2 have 12; libjpeg refuses them too)
            if (n == 3 && comp[0].h * comp[0].v + comp[1].h * comp[1].v + comp[2].h * comp[2].v > 10) return PARSE_BAD;
            have_sof = true;
        } else if (m == 0xC2 || (m >= 0xC5 && m <= 0xCF && m != 0xC8 && m != 0xCC)) {
            return PARSE_BAD;                   // progressive / lossless / arithmetic
        } else if (m == 0xDD) {
            if (L < 4) return PARSE_BAD;
            restart = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!have_sof || L < 3) return PARSE_BAD;
            const int ns = s[0];
            if (ns != ncomp || L < (size_t)(6 + 2 * ns)) return PARSE_BAD;      // one interleaved scan (what baseline encoders write)
            for (int i = 0; i < ns; ++i)
                for (int c = 0; c < ncomp; ++c)
                    if (comp[c].id == s[1 + 2 * i]) { comp[c].td = s[2 + 2 * i] >> 4; comp[c].ta = s[2 + 2 * i] & 15; }
            for (int c = 0; c < ncomp; ++c) if (comp[c].td > 3 || comp[c].ta > 3) return PARSE_BAD;
            for (int c = 0; c < ncomp; ++c) if (!dc[comp[c].td].present || !ac[comp[c].ta].present) return PARSE_BAD;
            pos += L;
            if (rows) *rows = H;
            if (cols) *cols = W;
            if (channels) *channels = ncomp;
            if (seg) *seg = pos;
            if (!d) return PARSE_OK;
            d->W = W; d->H = H; d->ncomp = ncomp; d->hmax = hmax; d->vmax = vmax;
            d->mcux = (W + 8 * hmax - 1) / (8 * hmax); d->mcuy = (H + 8 * vmax - 1) / (8 * vmax);
            d->nmcu = d->mcux * d->mcuy;
            d->bpm = 0;
            bool host_only = false;
            for (int c = 0; c < ncomp; ++c) {
                d->ch[c] = comp[c].h; d->cv[c] = comp[c].v;
                d->cwb[c] = d->mcux * comp[c].h; d->chb[c] = d->mcuy * comp[c].v;
                d->cdw[c] = (W * comp[c].h + hmax - 1) / hmax; d->cdh[c] = (H * comp[c].v + vmax - 1) / vmax;
                d->coff[c] = d->bpm;
                d->bpm += comp[c].h * comp[c].v;
                std::memcpy(d->qt[c], qt[comp[c].tq], sizeof d->qt[c]);
                dc[comp[c].td].to(d->dc[c]); ac[comp[c].ta].to(d->ac[c]);
                if (hmax / comp[c].h == 1 && vmax / comp[c].v == 2) host_only = true;       // 1x2: rows replicated, host only
            }
            d->ri = (restart > 0 && restart < d->nmcu) ? restart : d->nmcu;
            d->nint = (d->nmcu + d->ri - 1) / d->ri;
            return host_only ? PARSE_HOST_ONLY : PARSE_OK;
        }
        pos += L;
    }
    return PARSE_BAD;       // no scan
}

}  // namespace uwip_jpeg
