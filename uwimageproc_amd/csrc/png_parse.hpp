// The chunk walk and the IHDR rules of imgio::read_png (cli/imgio.hpp), stated once for uwip_png_info, uwip_png_decode, the
// emulation harness and cli/pngdec_check: which streams the host reader starts to inflate, where their IDAT payloads lie, and
// where the zlib stream may be cut into segments for the device.  No CRC is checked, the host reader checks
// none.  Host only.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "inflate_core.hpp"

namespace uwip_pngd {

enum { PARSE_OK = 0, PARSE_BAD = -1 };      // UWIP_PNG_BAD_STREAM

struct Span { size_t off, len; };           // an IDAT payload inside the file
struct Parsed {
    uint32_t W = 0, H = 0;
    int spp = 0;                            // samples per pixel: 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA
    size_t zlen = 0;                        // bytes of the zlib stream: the IDAT payloads up to IEND, concatenated
    std::vector<Span> idat;
    std::vector<size_t> cuts;               // offsets in the zlib stream where an IDAT starts behind 00 00 FF FF, ascending
};

inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// read_png's walk: the signature, chunks while twelve bytes are left, a chunk that overruns the file is the end of the
// decode, the last IHDR counts, IEND stops the walk.  IHDR's thirteen bytes are read whatever its length field says (the
// host reader does), so they have to lie inside the file.  Then the IHDR rules and the zlib header.
inline int parse(const uint8_t *buf, size_t len, Parsed &p)
{
    static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    p = Parsed();
    if (!buf || len < 33 || std::memcmp(buf, sig, 8) != 0) return PARSE_BAD;
    size_t pos = 8;
    int depth = 0, ctype = 0, interlace = 0;
    uint8_t tail[4] = {1, 1, 1, 1};         // the last four bytes of the zlib stream so far
    uint8_t head[2] = {0, 0};
    while (pos + 12 <= len) {
        const uint32_t n = be32(buf + pos);
        const uint8_t *type = buf + pos + 4, *d = buf + pos + 8;
        if (pos + 12 + (size_t)n > len) return PARSE_BAD;
        if (!std::memcmp(type, "IHDR", 4)) {
            if (pos + 8 + 13 > len) return PARSE_BAD;
            p.W = be32(d); p.H = be32(d + 4); depth = d[8]; ctype = d[9]; interlace = d[12];
        } else if (!std::memcmp(type, "IDAT", 4)) {
            if (n) {
                if (p.zlen > 2 && tail[0] == 0 && tail[1] == 0 && tail[2] == 0xFF && tail[3] == 0xFF) p.cuts.push_back(p.zlen);
                for (uint32_t i = 0; i < n && p.zlen + i < 2; ++i) head[p.zlen + i] = d[i];
                for (uint32_t i = n > 4 ? n - 4 : 0; i < n; ++i) { tail[0] = tail[1]; tail[1] = tail[2]; tail[2] = tail[3]; tail[3] = d[i]; }
                p.idat.push_back({pos + 8, (size_t)n});
                p.zlen += n;
            }
        } else if (!std::memcmp(type, "IEND", 4)) break;
        pos += 12 + (size_t)n;
    }
    if (depth != 8 || interlace != 0 || p.W == 0 || p.H == 0) return PARSE_BAD;
    p.spp = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (!p.spp) return PARSE_BAD;
    if (p.zlen < 2 || !uwip_inflate::zlib_header_ok(head[0], head[1])) return PARSE_BAD;
    return PARSE_OK;
}

// the IHDR rules alone, for uwip_png_info: the size and the channels (1 grey, 3 colour) of a stream read_png would inflate
inline int info(const uint8_t *buf, size_t len, int *rows, int *cols, int *channels)
{
    Parsed p;
    if (parse(buf, len, p) != PARSE_OK || p.W > 0x7fffffffu || p.H > 0x7fffffffu) return PARSE_BAD;
    *rows = (int)p.H; *cols = (int)p.W; *channels = p.spp <= 2 ? 1 : 3;
    return PARSE_OK;
}

// the zlib stream into dst (p.zlen bytes)
inline void gather(const uint8_t *buf, const Parsed &p, uint8_t *dst)
{
    for (const Span &s : p.idat) { std::memcpy(dst, buf + s.off, s.len); dst += s.len; }
}

}  // namespace uwip_pngd
