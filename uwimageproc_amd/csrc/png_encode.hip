// PNG encoding of a batch on the device: cv::imwrite(".png") without the trip to the host.  Lossless: colour type 0 (grey) or 2
// (BGR in, RGB in the file), 8 bit, no interlace, adaptive or forced row filters, and a zlib stream whose deflate is zlib's
// Z_RLE parse (runs at distance 1) with one block per 32 KiB chunk of filtered bytes, each with its own length-limited Huffman
// codes, or stored / fixed where that is not longer.  Every chunk ends on a byte (an empty stored block follows all but the
// last) and becomes one IDAT, so no word and no CRC is shared between workgroups; the Adler-32 has an IDAT of its own.  All
// arithmetic is deflate_core.hpp (shared with the serial host reference, png_reference.hpp, which writes the same bytes).
//   k_png_filter    one workgroup per row: the five costs (filter -1), the type byte and the filtered row into "png.filtered"
//                   -- from the source rows alone, so rows are independent;
//   k_png_deflate   one workgroup per chunk, 128 bytes per thread: run starts by neighbour comparison, every run's ends across
//                   the threads, tokens in closed form from the offset within the run (rle_token); histogram in LDS; the codes
//                   (sort by rank in parallel, tree and header by one thread); per-thread bit lengths, scan, codes ORed into an
//                   LDS window at their bit offsets; the window's CRC from per-thread slices combined with x^(8 S) mod P; the
//                   window goes to the chunk's staging area by plain stores, with its length, CRC and Adler sums;
//   k_png_finish    one workgroup per frame: offsets of the IDATs, the stream length, the Adler-32 from the chunk sums;
//   k_png_assemble  signature, IHDR, the IDATs, the Adler IDAT, IEND and the size -- or minus the size and nothing else.
#include "uwip_internal.hpp"
#include "device_utils.hpp"
#include "deflate_core.hpp"
#include <cstring>

namespace {

using namespace uwip_png;

constexpr int kSeg = kChunk / 256;                       // filtered bytes per thread of k_png_deflate
constexpr int kWinBytes = 2 + 5 + kChunk + 5;            // zlib header, stored block, empty stored block: the longest payload
constexpr int kWinWords = (kWinBytes + 3) / 4 + 2;
constexpr int kStageBytes = (kWinBytes + 15) / 16 * 16;  // per chunk in "png.staging"

struct PGeo {
    int rows, cols, nc, nch;        // nch: chunks per frame
    size_t step, fs;
    uint64_t total;                 // filtered bytes per frame
    size_t fstride;                 // bytes between the frames of "png.filtered": nch * kChunk
};
// per chunk, from k_png_deflate
struct ChunkOut { uint32_t size, crc, a, b; };

__global__ __launch_bounds__(256) void k_png_filter(const uint8_t *__restrict__ img, PGeo g, int filter, uint8_t *__restrict__ filt,
                                                    const int32_t *__restrict__ nsel)
{
    __shared__ uint32_t s_scan[8];
    if (nsel && (int)blockIdx.y >= *nsel) return;                // uniform over the workgroup, ahead of every barrier
    const int y = blockIdx.x, f = blockIdx.y, nc = g.nc, rb = g.cols * g.nc;
    const uint8_t *row = img + (size_t)f * g.fs + (size_t)y * g.step, *up = y ? row - g.step : nullptr;
    auto sample = [&](const uint8_t *r, int i) -> int {        // byte i of the row as the file has it (RGB)
        if (!r || i < 0) return 0;
        return nc == 3 ? r[i - i % 3 + (2 - i % 3)] : r[i];
    };
    int type = filter;
    if (filter < 0) {
        uint32_t cost[5] = {0, 0, 0, 0, 0};
        for (int i = threadIdx.x; i < rb; i += 256) {
            const int x = sample(row, i), a = sample(row, i - nc), b = sample(up, i), c = sample(up, i - nc);
#pragma unroll
            for (int ty = 0; ty < 5; ++ty) cost[ty] += filter_cost(filter_byte(ty, x, a, b, c));
        }
        uint32_t best = 0;
#pragma unroll
        for (int ty = 0; ty < 5; ++ty) {
            const uint32_t s = block256_sum_u32(cost[ty], s_scan);
            if (ty == 0 || s < best) { best = s; type = ty; }
        }
    }
    uint8_t *dst = filt + (size_t)f * g.fstride + (size_t)y * ((size_t)rb + 1);
    if (threadIdx.x == 0) dst[0] = (uint8_t)type;
    for (int i = threadIdx.x; i < rb; i += 256)
        dst[1 + i] = filter_byte(type, sample(row, i), sample(row, i - nc), sample(up, i), sample(up, i - nc));
}

// The tokens that start in [b0, b1) of a chunk of n bytes: tok(length or 1, byte).  s_in: where the run that reaches into b0
// starts; e_out: where the run that leaves through b1 ends.
template <class Tok>
__device__ __forceinline__ void walk_tokens(const uint8_t *__restrict__ d, int n, int b0, int b1, int s_in, int e_out, Tok tok)
{
    for (int p = b0; p < b1;) {
        const int v = d[p];
        int q = p + 1;
        while (q < b1 && d[q] == v) ++q;
        const int S = (p == b0 && b0 > 0 && d[b0 - 1] == v) ? s_in : p;
        const int E = (q == b1 && b1 < n && d[b1] == v) ? e_out : q;
        for (int i = p; i < q; ++i) {
            const int t = rle_token(i - S, E - S);
            if (t) tok(t, v);
        }
        p = q;
    }
}

__global__ __launch_bounds__(256) void k_png_deflate(const uint8_t *__restrict__ filt, PGeo g, uint8_t *__restrict__ stage,
                                                     ChunkOut *__restrict__ cout, const int32_t *__restrict__ nsel)
{
    if (nsel && (int)blockIdx.y >= *nsel) return;
    __shared__ uint32_t s_freq[kNumLL], s_win[kWinWords], s_crc[256], s_tab[256], s_scan[8], s_nmatch;
    __shared__ int s_ls[256], s_fs[256];
    __shared__ Codes s_codes;
    __shared__ Scratch s_scr;
    const int t = threadIdx.x, c = blockIdx.x, f = blockIdx.y;
    auto orw = [](uint32_t *p, uint32_t v) { if (v) atomicOr(p, v); };
    const uint64_t base = (uint64_t)c * kChunk;
    const int n = (int)min((uint64_t)kChunk, g.total - base);
    const bool first = c == 0, last = c == g.nch - 1;
    const uint8_t *d = filt + (size_t)f * g.fstride + base;
    for (int i = t; i < kNumLL; i += 256) s_freq[i] = i == kEOB ? 1u : 0u;
    for (int i = t; i < kWinWords; i += 256) s_win[i] = 0u;
    s_tab[t] = crc_table_entry((uint32_t)t);
    if (t == 0) s_nmatch = 0u;
    // run starts: the last and the first one of this thread's bytes; the chunk's Adler sums
    const int b0 = min(t * kSeg, n), b1 = min(b0 + kSeg, n);
    int ls = -1, fst = n;
    uint32_t sa = 0, sb = 0;
    for (int p = b0; p < b1; ++p) {
        if (p == 0 || d[p] != d[p - 1]) { ls = p; if (fst == n) fst = p; }
        sa += d[p];
        sb += (uint32_t)(n - p) * d[p];                       // < 128 * 32768 * 255
    }
    s_ls[t] = ls; s_fs[t] = fst;
    const uint32_t adler_a = block256_sum_u32(sa % kAdlerMod, s_scan) % kAdlerMod;
    const uint32_t adler_b = block256_sum_u32(sb % kAdlerMod, s_scan) % kAdlerMod;    // (the sums' barriers publish s_ls, s_fs)
    int s_in = 0, e_out = n;
    for (int j = t - 1; j >= 0; --j) if (s_ls[j] >= 0) { s_in = s_ls[j]; break; }
    for (int j = t + 1; j < 256; ++j) if (s_fs[j] < n) { e_out = s_fs[j]; break; }
    // histogram
    uint32_t nm = 0;
    walk_tokens(d, n, b0, b1, s_in, e_out, [&](int len, int byte) {
        int sym = byte;
        if (len != 1) { int nx; uint32_t ex; length_symbol(len, sym, nx, ex); ++nm; }
        atomicAdd(&s_freq[sym], 1u);
    });
    if (nm) atomicAdd(&s_nmatch, nm);
    __syncthreads();
    // the codes: the sort in parallel, the rest by one thread
    uint32_t used = 0;
    for (int i = t; i < kNumLL; i += 256) {
        const int r = huff_rank(s_freq, kNumLL, i);
        if (r >= 0) { s_scr.order[r] = (uint16_t)i; ++used; }
    }
    const int m = (int)block256_sum_u32(used, s_scan);
    if (t == 0) plan_block(s_freq, s_nmatch, n, m, s_scr, s_codes);
    __syncthreads();
    const uint32_t hdr0 = first ? 2u : 0u;
    uint8_t *wb = reinterpret_cast<uint8_t *>(s_win);
    uint32_t end_bits;
    if (s_codes.mode == kStored) {                            // uniform over the workgroup
        if (t == 0) {
            if (first) { wb[0] = 0x78; wb[1] = 0x01; }
            wb[hdr0] = last ? 1 : 0;
            wb[hdr0 + 1] = (uint8_t)n; wb[hdr0 + 2] = (uint8_t)(n >> 8); wb[hdr0 + 3] = (uint8_t)~n; wb[hdr0 + 4] = (uint8_t)(~n >> 8);
        }
        for (int p = t; p < n; p += 256) wb[hdr0 + 5 + p] = d[p];
        end_bits = (hdr0 + 5 + (uint32_t)n) * 8;
    } else {
        uint32_t bits = 0;
        walk_tokens(d, n, b0, b1, s_in, e_out, [&](int len, int byte) { put_token(s_codes, len, byte, [&](uint32_t, int nb) { bits += (uint32_t)nb; }); });
        const uint32_t inc = block256_incl_scan_u32(bits, s_scan);
        const uint32_t data0 = hdr0 * 8 + s_codes.hdr_bits;
        if (t == 0) {
            if (first) atomicOr(&s_win[0], 0x0178u);
            BitSink<decltype(orw)> hs(s_win, hdr0 * 8, orw);
            put_block_header(s_codes, last, [&](uint32_t v, int nb) { hs.put(v, nb); });
            hs.flush();
        }
        BitSink<decltype(orw)> sink(s_win, data0 + inc - bits, orw);
        walk_tokens(d, n, b0, b1, s_in, e_out, [&](int len, int byte) { put_token(s_codes, len, byte, [&](uint32_t v, int nb) { sink.put(v, nb); }); });
        if (t == 255) sink.put(s_codes.ll[kEOB] & 0xffffu, (int)(s_codes.ll[kEOB] >> 16));
        sink.flush();
        end_bits = data0 + s_codes.data_bits;
    }
    uint32_t len = (end_bits + 7) / 8;
    if (!last) len = (end_bits + 3 + 7) / 8 + 4;              // BFINAL 0, BTYPE 00, to the byte, LEN 0000, NLEN FFFF
    __syncthreads();
    if (t == 0 && !last) { wb[len - 2] = 0xff; wb[len - 1] = 0xff; }
    __syncthreads();
    // CRC: thread t takes bytes [t S, (t + 1) S) of the payload padded IN FRONT with zeros to 256 S bytes (zeros in front do not
    // change a zero-start register), then pairs of neighbours: left x^(8 S d) + right
    const uint32_t S = (len + 255) / 256, pad = 256 * S - len;
    uint32_t r = 0;
    for (uint32_t q = t * S; q < (t + 1) * S; ++q)
        if (q >= pad) r = s_tab[(r ^ wb[q - pad]) & 0xffu] ^ (r >> 8);
    s_crc[t] = r;
    uint32_t shift = crc_shift_bytes(S);
    for (int dd = 1; dd < 256; dd <<= 1) {
        __syncthreads();
        if ((t & (2 * dd - 1)) == 0) s_crc[t] = crc_mulmod(s_crc[t], shift) ^ s_crc[t + dd];
        shift = crc_mulmod(shift, shift);
    }
    uint32_t *dst = reinterpret_cast<uint32_t *>(stage + ((size_t)f * g.nch + c) * kStageBytes);
    for (uint32_t i = t; i < (len + 3) / 4; i += 256) dst[i] = s_win[i];
    if (t == 0) {
        ChunkOut o;
        o.size = len; o.crc = crc_idat(s_crc[0], len); o.a = adler_a; o.b = adler_b;
        cout[(size_t)f * g.nch + c] = o;
    }
}

// per frame: where each IDAT starts behind signature and IHDR, the stream length, the Adler-32
__global__ __launch_bounds__(256) void k_png_finish(const ChunkOut *__restrict__ cout, PGeo g, uint64_t *__restrict__ coff,
                                                    int64_t *__restrict__ needed, uint32_t *__restrict__ adler,
                                                    const int32_t *__restrict__ nsel)
{
    __shared__ uint32_t s_scan[8], s_tot[2];
    const int f = blockIdx.x, t = threadIdx.x;
    if (nsel && f >= *nsel) return;
    uint64_t off = 0;
    uint32_t A = 1, myb = 0;                                  // A: the Adler A in front of this tile
    for (int cb = 0; cb < g.nch; cb += 256) {
        const int i = cb + t;
        const bool in = i < g.nch;
        const ChunkOut o = in ? cout[(size_t)f * g.nch + i] : ChunkOut{0, 0, 0, 0};
        const uint32_t v = in ? 12u + o.size : 0u;
        const uint32_t inc = block256_incl_scan_u32(v, s_scan), inca = block256_incl_scan_u32(o.a, s_scan);
        if (in) {
            coff[(size_t)f * g.nch + i] = off + inc - v;
            const uint32_t n = (uint32_t)min((uint64_t)kChunk, g.total - (uint64_t)i * kChunk);
            const uint32_t pa = (A + inca - o.a) % kAdlerMod;          // A in front of chunk i
            myb = (myb + (n % kAdlerMod) * pa % kAdlerMod + o.b) % kAdlerMod;
        }
        if (t == 255) { s_tot[0] = inc; s_tot[1] = inca; }
        __syncthreads();
        off += s_tot[0];
        A = (A + s_tot[1]) % kAdlerMod;
    }
    const uint32_t B = block256_sum_u32(myb, s_scan) % kAdlerMod;
    if (t == 0) {
        needed[f] = (int64_t)(kHeadBytes + off + kTailBytes);
        adler[f] = (B << 16) | A;
    }
}

__global__ __launch_bounds__(256) void k_png_assemble(const uint8_t *__restrict__ stage, const ChunkOut *__restrict__ cout,
                                                      const uint64_t *__restrict__ coff, PGeo g, const uint8_t *__restrict__ head,
                                                      const int64_t *__restrict__ needed, const uint32_t *__restrict__ adler,
                                                      uint8_t *__restrict__ streams, size_t slot_bytes, int64_t *__restrict__ sizes,
                                                      const int32_t *__restrict__ nsel)
{
    __shared__ uint8_t s_tail[kTailBytes];
    const int c = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    if (nsel && f >= *nsel) {                                   // not selected: size 0, nothing written
        if (c == 0 && t == 0) sizes[f] = 0;
        return;
    }
    const int64_t need = needed[f];
    const bool fits = (uint64_t)need <= (uint64_t)slot_bytes;
    if (c == 0 && t == 0) sizes[f] = fits ? need : -need;
    if (!fits) return;                                        // a status, not a fault: nothing of this frame is written
    uint8_t *out = streams + (size_t)f * slot_bytes;
    if (c == 0) {
        if (t == 0) write_tail(adler[f], s_tail);
        __syncthreads();
        if (t < kHeadBytes) out[t] = head[t];
        if (t < kTailBytes) out[need - kTailBytes + t] = s_tail[t];
    }
    const ChunkOut o = cout[(size_t)f * g.nch + c];
    uint8_t *p = out + kHeadBytes + coff[(size_t)f * g.nch + c];
    if (t < 4) p[t] = (uint8_t)(o.size >> (24 - 8 * t));
    else if (t < 8) p[t] = (uint8_t)"IDAT"[t - 4];
    else if (t < 12) p[8 + o.size + (t - 8)] = (uint8_t)(o.crc >> (24 - 8 * (t - 8)));
    const uint8_t *src = stage + ((size_t)f * g.nch + c) * kStageBytes;
    for (uint32_t i = t; i < o.size; i += 256) p[8 + i] = src[i];
}

bool png_geometry(int rows, int cols, int channels)
{
    return rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535 && (channels == 1 || channels == 3);
}

PGeo geometry_of(int rows, int cols, int nc, size_t step, size_t fs)
{
    PGeo g;
    g.rows = rows; g.cols = cols; g.nc = nc; g.step = step; g.fs = fs;
    g.total = filtered_bytes(rows, cols, nc);
    g.nch = (int)chunks_of(g.total);
    g.fstride = (size_t)g.nch * kChunk;
    return g;
}

// uwip_png_encode_dev behind its argument checks and the cached head, on either back end (uwip_device; the host threads of
// tests/hip_on_host.hpp): the working arrays and every launch.  head: signature and IHDR where the kernels read them; d_count:
// null, or the device's frame count.
template <class BE>
void encode_sequence(BE &be, const uint8_t *img, const PGeo &g, int F, int filter, const uint8_t *head, uint8_t *d_streams, size_t slot_bytes,
                     int64_t *d_sizes, const int32_t *d_count)
{
    using dim3 = typename BE::dim3;                           // HIP's on the device, its stand-in on host threads
    const size_t nchunks = (size_t)F * g.nch;
    uint8_t *filt = be.template array<uint8_t>("png.filtered", (size_t)F * g.fstride);
    uint8_t *stage = be.template array<uint8_t>("png.staging", nchunks * kStageBytes);
    ChunkOut *cout = be.template array<ChunkOut>("png.chunkout", nchunks);
    uint64_t *coff = be.template array<uint64_t>("png.coff", nchunks);
    int64_t *needed = be.template array<int64_t>("png.needed", (size_t)F);
    uint32_t *adler = be.template array<uint32_t>("png.adler", (size_t)F);
    be.launch("k_png_filter", k_png_filter, dim3(g.rows, F), 256, img, g, filter, filt, d_count);
    be.launch("k_png_deflate", k_png_deflate, dim3(g.nch, F), 256, filt, g, stage, cout, d_count);
    be.launch("k_png_finish", k_png_finish, dim3(F), 256, cout, g, coff, needed, adler, d_count);
    be.launch("k_png_assemble", k_png_assemble, dim3(g.nch, F), 256, stage, cout, coff, g, head, needed, adler, d_streams, slot_bytes, d_sizes,
              d_count);
}

}  // namespace

UWIP_API size_t uwip_png_bound(int rows, int cols, int channels)
{
    if (!png_geometry(rows, cols, channels)) return 0;
    const uint64_t fb = filtered_bytes(rows, cols, channels);
    return (size_t)(fb + chunks_of(fb) * kChunkOverhead + kFrameOverhead);
}

UWIP_API int uwip_png_chunk_bytes(void) { return kChunk; }

UWIP_API int uwip_png_encode(uwip_ctx *ctx, const uwip_batch_u8 *frames, int filter, uint8_t *d_streams, size_t slot_bytes,
                             int64_t *d_sizes)
{
    return uwip_png_encode_dev(ctx, frames, filter, d_streams, slot_bytes, d_sizes, nullptr);
}

int uwip_png_encode_dev(uwip_ctx *ctx, const uwip_batch_u8 *frames, int filter, uint8_t *d_streams, size_t slot_bytes,
                        int64_t *d_sizes, const int32_t *d_count)
{
    if (!ctx) {                                               // no context: because there is no device, or a plain bad argument
        int ndev = 0;
        return (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) ? UWIP_ERR_HIP : UWIP_ERR_INVALID;
    }
    int rc = uwip_check_batch(ctx, frames, 0);
    if (rc) return rc;
    const int F = frames->frames;
    if (F == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, frames->rows >= 1 && frames->cols >= 1, "empty frame");
    UWIP_REQUIRE(ctx, frames->rows <= 65535 && frames->cols <= 65535, "at most 65535 rows / columns");
    UWIP_REQUIRE(ctx, F <= 65535, "at most 65535 frames per call");
    UWIP_REQUIRE(ctx, filter >= -1 && filter <= 4, "filter must be -1 (adaptive) or 0..4");
    UWIP_REQUIRE(ctx, d_sizes != nullptr, "null sizes");
    UWIP_REQUIRE(ctx, d_streams != nullptr || slot_bytes == 0, "null streams");

    const PGeo g = geometry_of(frames->rows, frames->cols, frames->channels, frames->step, frames->frame_stride);

    char key[96];
    std::snprintf(key, sizeof key, "png.head.%dx%dx%d", g.rows, g.cols, g.nc);
    const void *d_head = uwip_table_find(ctx, key, nullptr);
    if (!d_head) {
        uint8_t h[kHeadBytes];
        write_head(g.rows, g.cols, g.nc, h);
        d_head = uwip_table_put(ctx, key, h, sizeof h);
        if (!d_head) return UWIP_ERR_HIP;
    }
    uwip_device dev(ctx);
    encode_sequence(dev, static_cast<const uint8_t *>(frames->data), g, F, filter, static_cast<const uint8_t *>(d_head), d_streams, slot_bytes,
                    d_sizes, d_count);
    return dev.finish();
}

UWIP_API int uwip_png_encode_host(uwip_ctx *ctx, const uwip_batch_u8 *frames, int filter, uint8_t *h_streams, size_t slot_bytes,
                                  int64_t *h_sizes)
{
    if (!ctx) return uwip_png_encode(ctx, frames, filter, nullptr, 0, nullptr);
    return uwip_encode_to_host(ctx, frames, filter, h_streams, slot_bytes, h_sizes, uwip_png_encode, "png.streams", "png.sizes");
}
