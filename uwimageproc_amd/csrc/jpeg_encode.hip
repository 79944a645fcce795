// Baseline JPEG encoding of a batch on the device: cv::imwrite(".jpg") without the trip to the host.
// The arithmetic follows jpeg::encode of cli/jpeg.hpp (the host codec the CLIs write their files with) step for step, so
// the streams are the same bytes: rgb_ycc conversion, 2x2 chroma box with the alternating 1, 2 bias, jfdctint (jpeg_core.hpp,
// shared with the host), the division quantiser, the Annex K Huffman tables and the header (jpeg_tables.hpp, shared), byte
// stuffing.  Everything but the DC difference and the bit position of a block is
// independent per 8x8 block, so the frame goes through five streaming stages:
//   k_jpeg_transform  one thread per block: samples (edge-replicated to the MCU-padded size) -> FDCT -> quantised
//                     coefficients, zig-zag order, int16, in the workspace "jpeg.coef";
//   k_jpeg_bits       one thread per block: entropy-coded bit length (DC category from the previous block of the same
//                     component); exclusive scan inside the workgroup, workgroup sums out;
//   k_jpeg_scan_bits  one workgroup per frame: exclusive scan of the workgroup sums (64-bit), the frame's bit total;
//   k_jpeg_emit       128 blocks per workgroup: every block's codes go to its bit offset in an LDS window (ds_or), the window
//                     goes to the unstuffed buffer -- a word two workgroups share by atomicOr on a word zeroed beforehand
//                     (k_jpeg_zero_shared), every other word by a plain store; the last byte is padded with one-bits.  The
//                     same pass counts the window's 0xFF bytes, so the stream length is exact also for a frame whose unstuffed
//                     stream does not fit its slot (nothing of such a frame is stored);
//   k_jpeg_ffcount    0xFF bytes per 4 KiB chunk of the unstuffed buffer; k_jpeg_finish scans them and fixes the length;
//   k_jpeg_assemble   header, stuffed bytes, FF D9 and the length into the frame's slot.
// The unstuffed buffer keeps the stream as big-endian 32-bit words: byte k is bits 31-8(k&3) .. 24-8(k&3) of word k / 4.
#include "uwip_internal.hpp"
#include "device_utils.hpp"
#include "jpeg_core.hpp"
#include "jpeg_tables.hpp"
#include <cstring>

namespace {

using uwip_jpeg::fdct_pass;

constexpr int kBitsWG = 256;        // blocks per workgroup of k_jpeg_bits (one thread each)
constexpr int kEmitWG = 128;        // blocks per workgroup of k_jpeg_emit
// the longest a block can get: DC code (<= 11 bits, chroma category 11) + 11 magnitude bits, 63 x (16-bit AC code + 10
// magnitude bits) = 1660 bits
constexpr int kMaxBlockBits = 22 + 63 * 26;
constexpr int kWinWords = (kEmitWG * kMaxBlockBits + 31) / 32 + 2;
constexpr int kChunk = 4096;        // bytes of unstuffed stream per workgroup of the stuffing passes (16 per thread)
constexpr int kHdrMax = 640;        // SOI .. SOS is 623 bytes for colour, 328 for grey

// per (geometry, quality) constants, a cached device table: the quantisers, then the header
struct JpegConst {
    int32_t qv[2][64];              // q << 3 in zig-zag order (luma, chroma)
    uint32_t hdr_len;
    uint8_t hdr[kHdrMax];
};
// the Huffman tables, code | size << 16 per symbol
struct JpegHuff {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

struct Geo {
    int rows, cols, nc;             // nc = 1 (grey) or 3 (4:2:0)
    int mcux, nblk;                 // MCUs per row; blocks per frame in scan order
    size_t step, fs;
};

// where block b of the scan lies: component (0 = Y, 1 = Cb, 2 = Cr) and the top-left luma pixel of what it covers
__device__ __forceinline__ void block_place(const Geo &g, int b, int &comp, int &x0, int &y0)
{
    if (g.nc == 1) {
        comp = 0; x0 = (b % g.mcux) * 8; y0 = (b / g.mcux) * 8;
        return;
    }
    const int mcu = b / 6, k = b - mcu * 6;
    const int mx = mcu % g.mcux, my = mcu / g.mcux;
    if (k < 4) { comp = 0; x0 = mx * 16 + (k & 1) * 8; y0 = my * 16 + (k >> 1) * 8; }
    else       { comp = k - 3; x0 = mx * 16; y0 = my * 16; }
}

// index of the previous block of the same component in scan order, -1 for the first
__device__ __forceinline__ int block_prev(const Geo &g, int b)
{
    if (g.nc == 1) return b - 1;
    const int k = b % 6;
    if (k >= 1 && k <= 3) return b - 1;
    if (b < 6) return -1;
    return k == 0 ? b - 3 : b - 6;
}

__global__ __launch_bounds__(256) void k_jpeg_transform(const uint8_t *__restrict__ img, Geo g, const JpegConst *__restrict__ cst,
                                                        int16_t *__restrict__ coef, const int32_t *__restrict__ nsel)
{
    __shared__ int32_t s_qv[2][64];
    if (nsel && (int)blockIdx.y >= *nsel) return;                        // uniform over the workgroup, ahead of every barrier
    if (threadIdx.x < 128) s_qv[threadIdx.x >> 6][threadIdx.x & 63] = cst->qv[threadIdx.x >> 6][threadIdx.x & 63];
    __syncthreads();
    const int b = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (b >= g.nblk) return;
    int comp, x0, y0;
    block_place(g, b, comp, x0, y0);
    const uint8_t *src = img + (size_t)f * g.fs;
    int32_t d[64];
    if (g.nc == 1) {
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint8_t *row = src + (size_t)min(y0 + y, g.rows - 1) * g.step;
#pragma unroll
            for (int x = 0; x < 8; ++x) d[y * 8 + x] = (int32_t)row[min(x0 + x, g.cols - 1)] - 128;
        }
    } else if (comp == 0) {
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint8_t *row = src + (size_t)min(y0 + y, g.rows - 1) * g.step;
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const uint8_t *p = row + (size_t)min(x0 + x, g.cols - 1) * 3;
                const int bl = p[0], gr = p[1], rd = p[2];
                d[y * 8 + x] = ((19595 * rd + 38470 * gr + 7471 * bl + 32768) >> 16) - 128;
            }
        }
    } else {
        // jccolor's Cb / Cr per pixel (8 bits each), then h2v2_downsample's box
        const int cr_ = comp == 2;
        const int kr = cr_ ? 32768 : -11059, kg = cr_ ? -27439 : -21709, kb = cr_ ? -5329 : 32768;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint8_t *r0 = src + (size_t)min(y0 + 2 * y, g.rows - 1) * g.step;
            const uint8_t *r1 = src + (size_t)min(y0 + 2 * y + 1, g.rows - 1) * g.step;
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const size_t xa = (size_t)min(x0 + 2 * x, g.cols - 1) * 3, xb = (size_t)min(x0 + 2 * x + 1, g.cols - 1) * 3;
                auto c = [&](const uint8_t *p) {
                    return (kr * (int)p[2] + kg * (int)p[1] + kb * (int)p[0] + (128 << 16) + 32767) >> 16;
                };
                d[y * 8 + x] = ((c(r0 + xa) + c(r0 + xb) + c(r1 + xa) + c(r1 + xb) + 1 + (x & 1)) >> 2) - 128;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
        fdct_pass(d[r * 8], d[r * 8 + 1], d[r * 8 + 2], d[r * 8 + 3], d[r * 8 + 4], d[r * 8 + 5], d[r * 8 + 6], d[r * 8 + 7], true);
#pragma unroll
    for (int c = 0; c < 8; ++c)
        fdct_pass(d[c], d[8 + c], d[16 + c], d[24 + c], d[32 + c], d[40 + c], d[48 + c], d[56 + c], false);
    const int32_t *qv = s_qv[comp ? 1 : 0];
    constexpr uint8_t ZZ[64] = UWIP_JPEG_ZIGZAG_INIT;
    uint32_t pk[32];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int32_t q = qv[i];
        int32_t t = d[ZZ[i]];
        const bool neg = t < 0;
        t = (neg ? -t : t) + (q >> 1);
        t = t >= q ? t / q : 0;
        const uint32_t v = (uint32_t)(neg ? -t : t) & 0xffffu;
        if (i & 1) pk[i >> 1] |= v << 16; else pk[i >> 1] = v;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(coef + ((size_t)f * g.nblk + b) * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = make_uint4(pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]);
}

__device__ __forceinline__ void load_huff(const JpegHuff *__restrict__ h, uint32_t (*s_dc)[16], uint32_t (*s_ac)[256])
{
    for (int i = threadIdx.x; i < 512; i += blockDim.x) s_ac[i >> 8][i & 255] = h->ac[i >> 8][i & 255];
    if (threadIdx.x < 32) s_dc[threadIdx.x >> 4][threadIdx.x & 15] = h->dc[threadIdx.x >> 4][threadIdx.x & 15];
}

__device__ __forceinline__ int nbits_of(int v) { return 32 - __clz(v < 0 ? -v : v); }     // __clz(0) = 32

// The entropy coding of one block, in the order jpeg::encode's `block` lambda puts it: put(value, bit count) per code.
template <class Put>
__device__ __forceinline__ void code_block(const int16_t *__restrict__ coef, const Geo &g, int f, int b, const uint32_t (*s_dc)[16],
                                           const uint32_t (*s_ac)[256], Put put)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(coef + ((size_t)f * g.nblk + b) * 64);
    uint32_t pk[32];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = src[i];
        pk[4 * i] = v.x; pk[4 * i + 1] = v.y; pk[4 * i + 2] = v.z; pk[4 * i + 3] = v.w;
    }
    const int tb = (g.nc == 3 && b % 6 >= 4) ? 1 : 0;
    const int pb = block_prev(g, b);
    const int pred = pb < 0 ? 0 : (int)coef[((size_t)f * g.nblk + pb) * 64];
    const int diff = (int)(int16_t)(pk[0] & 0xffffu) - pred;
    const int nb = nbits_of(diff);
    const uint32_t dcs = s_dc[tb][nb];
    put(((dcs & 0xffffu) << nb) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u)), (int)(dcs >> 16) + nb);
    const uint32_t zrl = s_ac[tb][0xF0];
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = (int)(int16_t)((pk[k >> 1] >> ((k & 1) * 16)) & 0xffffu);
        if (v == 0) { run++; continue; }
        while (run > 15) { put(zrl & 0xffffu, (int)(zrl >> 16)); run -= 16; }
        const int n2 = nbits_of(v);
        const uint32_t s = s_ac[tb][(run << 4) | n2];
        put(((s & 0xffffu) << n2) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n2) - 1u)), (int)(s >> 16) + n2);
        run = 0;
    }
    if (run) { const uint32_t s = s_ac[tb][0]; put(s & 0xffffu, (int)(s >> 16)); }
}

__global__ __launch_bounds__(kBitsWG) void k_jpeg_bits(const int16_t *__restrict__ coef, Geo g, const JpegHuff *__restrict__ huff,
                                                       uint32_t *__restrict__ blkoff, uint32_t *__restrict__ wgsum, int nwg,
                                                       const int32_t *__restrict__ nsel)
{
    __shared__ uint32_t s_dc[2][16], s_ac[2][256], s_scan[8];
    if (nsel && (int)blockIdx.y >= *nsel) return;
    load_huff(huff, s_dc, s_ac);
    __syncthreads();
    const int b = blockIdx.x * kBitsWG + threadIdx.x, f = blockIdx.y;
    uint32_t bits = 0;
    if (b < g.nblk) code_block(coef, g, f, b, s_dc, s_ac, [&](uint32_t, int n) { bits += (uint32_t)n; });
    const uint32_t inc = block256_incl_scan_u32(bits, s_scan);
    if (b < g.nblk) blkoff[(size_t)f * g.nblk + b] = inc - bits;
    if (threadIdx.x == kBitsWG - 1) wgsum[(size_t)f * nwg + blockIdx.x] = inc;
}

// exclusive scan of in[0..n) into 64-bit out[0..n) by one 256-thread workgroup; the total, in every thread
__device__ uint64_t scan_excl_u64(const uint32_t *__restrict__ in, uint64_t *__restrict__ out, int n, uint32_t *s_scan)
{
    uint64_t carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        const uint32_t v = i < n ? in[i] : 0u;
        const uint32_t inc = block256_incl_scan_u32(v, s_scan);
        if (i < n) out[i] = carry + inc - v;
        if (threadIdx.x == 255) s_scan[4] = inc;
        __syncthreads();
        carry += s_scan[4];
    }
    return carry;
}

__global__ __launch_bounds__(256) void k_jpeg_scan_bits(const uint32_t *__restrict__ wgsum, uint64_t *__restrict__ wgbase,
                                                        uint64_t *__restrict__ totbits, int nwg, const int32_t *__restrict__ nsel)
{
    __shared__ uint32_t s_scan[8];
    const int f = blockIdx.x;
    if (nsel && f >= *nsel) return;
    const uint64_t t = scan_excl_u64(wgsum + (size_t)f * nwg, wgbase + (size_t)f * nwg, nwg, s_scan);
    if (threadIdx.x == 0) totbits[f] = t;
}

struct Offs {
    const uint32_t *blkoff;
    const uint64_t *wgbase, *totbits;
    int nwg;                        // workgroups of k_jpeg_bits per frame
};
// bit offset of block b of frame f (b == nblk: the frame's total)
__device__ __forceinline__ uint64_t bit_offset(const Offs &o, const Geo &g, int f, int b)
{
    if (b >= g.nblk) return o.totbits[f];
    return o.wgbase[(size_t)f * o.nwg + b / kBitsWG] + o.blkoff[(size_t)f * g.nblk + b];
}
// the unstuffed stream of a frame is stored only when it can fit the slot at all (stuffing only adds)
__device__ __forceinline__ bool stores(uint64_t totbits, uint32_t hdr_len, size_t slot_bytes)
{
    return (uint64_t)hdr_len + (totbits + 7) / 8 + 2 <= (uint64_t)slot_bytes;
}

// zero the words two emit workgroups share, ahead of their atomicOr
__global__ void k_jpeg_zero_shared(Geo g, Offs o, const JpegConst *__restrict__ cst, size_t slot_bytes, uint32_t *__restrict__ ubuf,
                                   size_t ustride, int nwg_emit, const int32_t *__restrict__ nsel)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (w < 1 || w >= nwg_emit) return;
    if (nsel && f >= *nsel) return;
    if (!stores(o.totbits[f], cst->hdr_len, slot_bytes)) return;
    const uint64_t o0 = bit_offset(o, g, f, w * kEmitWG);
    if (o0 & 31) ubuf[(size_t)f * ustride + (size_t)(o0 >> 5)] = 0u;
}

__global__ __launch_bounds__(kEmitWG) void k_jpeg_emit(const int16_t *__restrict__ coef, Geo g, const JpegHuff *__restrict__ huff, Offs o,
                                                       const JpegConst *__restrict__ cst, size_t slot_bytes,
                                                       uint32_t *__restrict__ ubuf, size_t ustride, uint32_t *__restrict__ ffemit,
                                                       uint32_t *__restrict__ notff, int nwg_emit, const int32_t *__restrict__ nsel)
{
    __shared__ uint32_t s_dc[2][16], s_ac[2][256], s_win[kWinWords], s_cnt;
    if (nsel && (int)blockIdx.y >= *nsel) return;
    load_huff(huff, s_dc, s_ac);
    const int w = blockIdx.x, f = blockIdx.y;
    const int b0 = w * kEmitWG, b1 = min(b0 + kEmitWG, g.nblk);
    const bool last = b1 == g.nblk;
    const uint64_t o0 = bit_offset(o, g, f, b0), o1 = bit_offset(o, g, f, b1);
    const uint64_t o1p = last ? (o1 + 7) & ~(uint64_t)7 : o1;        // BitWriter::flush pads the last byte with ones
    const uint64_t wbase = o0 >> 5;
    const int nw = (int)(((o1p + 31) >> 5) - wbase);                 // <= kWinWords by kMaxBlockBits
    for (int i = threadIdx.x; i < nw; i += kEmitWG) s_win[i] = 0u;
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    const int b = b0 + (int)threadIdx.x;
    if (b < b1) {
        const uint32_t p = (uint32_t)(bit_offset(o, g, f, b) - wbase * 32);
        int wi = (int)(p >> 5), nacc = (int)(p & 31);
        uint32_t acc = 0u;
        code_block(coef, g, f, b, s_dc, s_ac, [&](uint32_t v, int n) {       // n <= 27, v < 2^n
            if (n == 0) return;
            const int room = 32 - nacc;
            if (n < room) { acc |= v << (room - n); nacc += n; return; }
            atomicOr(&s_win[wi], acc | (v >> (n - room)));
            ++wi;
            nacc = n - room;
            acc = nacc ? v << (32 - nacc) : 0u;
        });
        if (nacc) atomicOr(&s_win[wi], acc);
    }
    __syncthreads();
    if (threadIdx.x == 0 && o1p != o1) {
        const uint32_t p = (uint32_t)(o1 - wbase * 32), n = (uint32_t)(o1p - o1);
        s_win[p >> 5] |= ((1u << n) - 1u) << (32 - (p & 31) - n);
    }
    __syncthreads();
    auto byte_at = [&](uint64_t j) {                                  // byte j of the frame's unstuffed stream
        const uint32_t r = (uint32_t)(j - wbase * 4);
        return (s_win[r >> 2] >> (24 - 8 * (r & 3))) & 0xffu;
    };
    // 0xFF bytes: the bytes that lie wholly in this workgroup's bits are counted here; a byte shared with a neighbour is
    // 0xFF when no party says that its bits of it are not all ones (notff[w]: the byte in which workgroup w starts)
    uint32_t cnt = 0;
    for (uint64_t j = ((o0 + 7) >> 3) + threadIdx.x; j < (o1p >> 3); j += kEmitWG) cnt += byte_at(j) == 0xffu;
    if (threadIdx.x == 0) {
        if (o0 & 7) {
            const uint64_t end = min(o1p, (o0 | 7) + 1);
            const uint32_t n = (uint32_t)(end - o0), m = ((1u << n) - 1u) << (8 - (uint32_t)(o0 & 7) - n);
            if ((byte_at(o0 >> 3) & m) != m) notff[(size_t)f * (nwg_emit + 1) + w] = 1u;
        }
        if (o1p & 7) {
            const uint32_t n = (uint32_t)(o1p & 7), m = ((1u << n) - 1u) << (8 - n);
            if ((byte_at(o1p >> 3) & m) != m) notff[(size_t)f * (nwg_emit + 1) + w + 1] = 1u;
        }
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&ffemit[f], s_cnt);
    if (!stores(o.totbits[f], cst->hdr_len, slot_bytes)) return;
    uint32_t *dst = ubuf + (size_t)f * ustride + (size_t)wbase;
    for (int i = threadIdx.x; i < nw; i += kEmitWG) {
        const bool shared = (i == 0 && (o0 & 31)) || (i == nw - 1 && (o1p & 31) && !last);
        if (shared) atomicOr(&dst[i], s_win[i]);
        else dst[i] = s_win[i];
    }
}

// the 16 unstuffed bytes of thread t of chunk c: how many are 0xFF (and the bytes themselves, stream order, in v)
__device__ __forceinline__ uint32_t chunk_ff(const uint32_t *__restrict__ ubuf_f, uint64_t s, uint64_t ubytes, uint4 &v)
{
    v = *reinterpret_cast<const uint4 *>(ubuf_f + (s >> 2));
    const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) cnt += (s + k < ubytes) && ((wv[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu) == 0xffu;
    return cnt;
}

__global__ __launch_bounds__(256) void k_jpeg_ffcount(const uint32_t *__restrict__ ubuf, size_t ustride, const uint64_t *__restrict__ totbits,
                                                      const JpegConst *__restrict__ cst, size_t slot_bytes, uint32_t *__restrict__ chunkcnt,
                                                      int nchunk, const int32_t *__restrict__ nsel)
{
    __shared__ uint32_t s_scan[8];
    const int c = blockIdx.x, f = blockIdx.y;
    if (nsel && f >= *nsel) return;
    const uint64_t tb = totbits[f], ubytes = (tb + 7) / 8;
    const uint64_t s = (uint64_t)c * kChunk + threadIdx.x * 16;
    uint32_t cnt = 0;
    if (stores(tb, cst->hdr_len, slot_bytes) && (uint64_t)c * kChunk < ubytes) {        // uniform over the workgroup
        uint4 v;
        if (s < ubytes) cnt = chunk_ff(ubuf + (size_t)f * ustride, s, ubytes, v);
    }
    const uint32_t sum = block256_sum_u32(cnt, s_scan);
    if (threadIdx.x == 0) chunkcnt[(size_t)f * nchunk + c] = sum;
}

// per frame: scan of the chunk counts, and the stream length from the emit pass's count
__global__ __launch_bounds__(256) void k_jpeg_finish(const uint32_t *__restrict__ chunkcnt, uint64_t *__restrict__ chunkbase, int nchunk, Geo g,
                                                     Offs o, const JpegConst *__restrict__ cst, const uint32_t *__restrict__ ffemit,
                                                     const uint32_t *__restrict__ notff, int nwg_emit, int64_t *__restrict__ needed,
                                                     const int32_t *__restrict__ nsel)
{
    __shared__ uint32_t s_scan[8];
    const int f = blockIdx.x;
    if (nsel && f >= *nsel) return;
    (void)scan_excl_u64(chunkcnt + (size_t)f * nchunk, chunkbase + (size_t)f * nchunk, nchunk, s_scan);
    uint32_t cnt = 0;
    for (int w = 1 + (int)threadIdx.x; w < nwg_emit; w += 256)
        cnt += (bit_offset(o, g, f, w * kEmitWG) & 7) && !notff[(size_t)f * (nwg_emit + 1) + w];
    const uint32_t shared_ff = block256_sum_u32(cnt, s_scan);
    if (threadIdx.x == 0)
        needed[f] = (int64_t)cst->hdr_len + (int64_t)((o.totbits[f] + 7) / 8) + (int64_t)ffemit[f] + (int64_t)shared_ff + 2;
}

__global__ __launch_bounds__(256) void k_jpeg_assemble(const uint32_t *__restrict__ ubuf, size_t ustride, const uint64_t *__restrict__ totbits,
                                                       const uint64_t *__restrict__ chunkbase, int nchunk, const JpegConst *__restrict__ cst,
                                                       const int64_t *__restrict__ needed, uint8_t *__restrict__ streams, size_t slot_bytes,
                                                       int64_t *__restrict__ sizes, const int32_t *__restrict__ nsel)
{
    __shared__ uint32_t s_scan[8];
    const int c = blockIdx.x, f = blockIdx.y;
    if (nsel && f >= *nsel) {                                            // not selected: size 0, nothing written
        if (c == 0 && threadIdx.x == 0) sizes[f] = 0;
        return;
    }
    const int64_t need = needed[f];
    const bool fits = (uint64_t)need <= (uint64_t)slot_bytes;
    if (c == 0 && threadIdx.x == 0) sizes[f] = fits ? need : -need;
    if (!fits) return;                                                 // a status, not a fault: nothing of this frame is written
    uint8_t *out = streams + (size_t)f * slot_bytes;
    const uint32_t hl = cst->hdr_len;
    if (c == 0) {
        for (uint32_t i = threadIdx.x; i < hl; i += 256) out[i] = cst->hdr[i];
        if (threadIdx.x == 0) { out[need - 2] = 0xFF; out[need - 1] = 0xD9; }
    }
    const uint64_t ubytes = (totbits[f] + 7) / 8;
    if ((uint64_t)c * kChunk >= ubytes) return;
    const uint64_t s = (uint64_t)c * kChunk + threadIdx.x * 16;
    uint4 v = make_uint4(0, 0, 0, 0);
    const uint32_t cnt = s < ubytes ? chunk_ff(ubuf + (size_t)f * ustride, s, ubytes, v) : 0u;
    const uint32_t inc = block256_incl_scan_u32(cnt, s_scan);
    if (s >= ubytes) return;
    uint64_t d = (uint64_t)hl + s + chunkbase[(size_t)f * nchunk + c] + (inc - cnt);
    const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t by = (wv[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu;
        if (s + k < ubytes) {
            out[d++] = (uint8_t)by;
            if (by == 0xffu) out[d++] = 0;
        }
    }
}

int clamp_quality(int q) { return q < 1 ? 1 : (q > 100 ? 100 : q); }

// the quantisers and SOI .. SOS for (rows, cols, nc, quality)
void build_const(int rows, int cols, int nc, int quality, JpegConst &c)
{
    uint8_t q[2][64];
    uwip_jpeg::scaled_quant(quality, q);
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) c.qv[t][i] = (int32_t)q[t][uwip_jpeg::ZIGZAG[i]] << 3;
    static_assert(kHdrMax >= uwip_jpeg::header_bytes(3), "JpegConst::hdr holds the longer header");
    c.hdr_len = (uint32_t)uwip_jpeg::write_header(rows, cols, nc, q, c.hdr);
}

int blocks_of(int rows, int cols, int nc, int *mcux_out)
{
    const int mcu = nc == 3 ? 16 : 8;
    const int mcux = (cols + mcu - 1) / mcu, mcuy = (rows + mcu - 1) / mcu;
    if (mcux_out) *mcux_out = mcux;
    return mcux * mcuy * (nc == 3 ? 6 : 1);
}

// the Annex K tables as the kernels read them
void build_huff(JpegHuff &h)
{
    using namespace uwip_jpeg;
    std::memset(&h, 0, sizeof h);
    uint32_t t[256];
    build_codes(DC_LUM_BITS, DC_VALS, t); std::memcpy(h.dc[0], t, sizeof h.dc[0]);
    build_codes(DC_CHR_BITS, DC_VALS, t); std::memcpy(h.dc[1], t, sizeof h.dc[1]);
    build_codes(AC_LUM_BITS, AC_LUM_VALS, h.ac[0]);
    build_codes(AC_CHR_BITS, AC_CHR_VALS, h.ac[1]);
}

// uwip_jpeg_encode_dev behind its argument checks and table caches, on either back end (uwip_device; the host threads of
// tests/hip_on_host.hpp): the working arrays and every launch.  huff / cst: the tables where the kernels read them; d_count:
// null, or the device's frame count.
template <class BE>
void encode_sequence(BE &be, const uint8_t *img, const Geo &g, int F, const JpegHuff *huff, const JpegConst *cst, uint8_t *d_streams,
                     size_t slot_bytes, int64_t *d_sizes, const int32_t *d_count)
{
    using dim3 = typename BE::dim3;                           // HIP's on the device, its stand-in on host threads
    const int nwg_bits = (int)uwip_cdiv((size_t)g.nblk, kBitsWG), nwg_emit = (int)uwip_cdiv((size_t)g.nblk, kEmitWG);
    // the unstuffed stream of a frame is kept only when it fits the slot, so the slot bounds its buffer as well
    const size_t ubound = ((size_t)g.nblk * kMaxBlockBits + 7) / 8;
    const size_t ucap = slot_bytes < ubound ? slot_bytes : ubound;
    const size_t ustride = ((ucap + 15) / 16) * 4 + 8;                   // words; a multiple of 4: uint4 loads
    const int nchunk = ucap ? (int)uwip_cdiv(ucap, kChunk) : 1;
    const size_t nf = (size_t)F;

    int16_t *coef = be.template array<int16_t>("jpeg.coef", nf * g.nblk * 64);
    uint32_t *ubuf = be.template array<uint32_t>("jpeg.unstuffed", nf * ustride);
    uint32_t *blkoff = be.template array<uint32_t>("jpeg.blkoff", nf * g.nblk);
    uint32_t *wgsum = be.template array<uint32_t>("jpeg.wgsum", nf * nwg_bits);
    uint64_t *wgbase = be.template array<uint64_t>("jpeg.wgbase", nf * nwg_bits);
    uint64_t *totbits = be.template array<uint64_t>("jpeg.totbits", nf);
    uint32_t *chunkcnt = be.template array<uint32_t>("jpeg.chunkcnt", nf * nchunk);
    uint64_t *chunkbase = be.template array<uint64_t>("jpeg.chunkbase", nf * nchunk);
    int64_t *needed = be.template array<int64_t>("jpeg.needed", nf);
    uint32_t *ffemit = be.template array<uint32_t>("jpeg.ffemit", nf);
    uint32_t *notff = be.template array<uint32_t>("jpeg.notff", nf * (nwg_emit + 1));
    be.fill(ffemit, 0, nf * sizeof(uint32_t));
    be.fill(notff, 0, nf * (nwg_emit + 1) * sizeof(uint32_t));

    const Offs o{blkoff, wgbase, totbits, nwg_bits};
    be.launch("k_jpeg_transform", k_jpeg_transform, dim3(nwg_bits, F), 256, img, g, cst, coef, d_count);
    be.launch("k_jpeg_bits", k_jpeg_bits, dim3(nwg_bits, F), kBitsWG, coef, g, huff, blkoff, wgsum, nwg_bits, d_count);
    be.launch("k_jpeg_scan_bits", k_jpeg_scan_bits, dim3(F), 256, wgsum, wgbase, totbits, nwg_bits, d_count);
    be.launch("k_jpeg_zero_shared", k_jpeg_zero_shared, dim3(uwip_cdiv((size_t)nwg_emit, 256), F), 256, g, o, cst, slot_bytes, ubuf, ustride,
              nwg_emit, d_count);
    be.launch("k_jpeg_emit", k_jpeg_emit, dim3(nwg_emit, F), kEmitWG, coef, g, huff, o, cst, slot_bytes, ubuf, ustride, ffemit, notff, nwg_emit,
              d_count);
    be.launch("k_jpeg_ffcount", k_jpeg_ffcount, dim3(nchunk, F), 256, ubuf, ustride, totbits, cst, slot_bytes, chunkcnt, nchunk, d_count);
    be.launch("k_jpeg_finish", k_jpeg_finish, dim3(F), 256, chunkcnt, chunkbase, nchunk, g, o, cst, ffemit, notff, nwg_emit, needed, d_count);
    be.launch("k_jpeg_assemble", k_jpeg_assemble, dim3(nchunk, F), 256, ubuf, ustride, totbits, chunkbase, nchunk, cst, needed, d_streams,
              slot_bytes, d_sizes, d_count);
}

}  // namespace

UWIP_API size_t uwip_jpeg_bound(int rows, int cols, int channels)
{
    if (rows < 1 || cols < 1 || rows > 65535 || cols > 65535 || (channels != 1 && channels != 3)) return 0;
    const size_t nblk = (size_t)blocks_of(rows, cols, channels, nullptr);
    return uwip_jpeg::header_bytes(channels) + 2 * ((nblk * kMaxBlockBits + 7) / 8) + 2;
}

UWIP_API int uwip_jpeg_encode(uwip_ctx *ctx, const uwip_batch_u8 *frames, int quality, uint8_t *d_streams, size_t slot_bytes,
                              int64_t *d_sizes)
{
    return uwip_jpeg_encode_dev(ctx, frames, quality, d_streams, slot_bytes, d_sizes, nullptr);
}

int uwip_jpeg_encode_dev(uwip_ctx *ctx, const uwip_batch_u8 *frames, int quality, uint8_t *d_streams, size_t slot_bytes,
                         int64_t *d_sizes, const int32_t *d_count)
{
    int rc = uwip_check_batch(ctx, frames, 0);
    if (rc) return rc;
    const int F = frames->frames;
    if (F == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, frames->rows >= 1 && frames->cols >= 1, "empty frame");
    UWIP_REQUIRE(ctx, frames->rows <= 65535 && frames->cols <= 65535, "JPEG holds at most 65535 rows / columns");
    UWIP_REQUIRE(ctx, F <= 65535, "at most 65535 frames per call");
    UWIP_REQUIRE(ctx, d_sizes != nullptr, "null sizes");
    UWIP_REQUIRE(ctx, d_streams != nullptr || slot_bytes == 0, "null streams");
    quality = clamp_quality(quality);

    Geo g;
    g.rows = frames->rows; g.cols = frames->cols; g.nc = frames->channels;
    g.step = frames->step; g.fs = frames->frame_stride;
    g.nblk = blocks_of(g.rows, g.cols, g.nc, &g.mcux);

    const void *d_huff = uwip_table_find(ctx, "jpeg.huff", nullptr);
    if (!d_huff) {
        std::vector<JpegHuff> h(1);
        build_huff(h[0]);
        d_huff = uwip_table_put(ctx, "jpeg.huff", h.data(), sizeof(JpegHuff));
        if (!d_huff) return UWIP_ERR_HIP;
    }
    char key[96];
    std::snprintf(key, sizeof key, "jpeg.const.%dx%dx%d.q%d", g.rows, g.cols, g.nc, quality);
    const void *d_cst = uwip_table_find(ctx, key, nullptr);
    if (!d_cst) {
        std::vector<JpegConst> c(1);
        std::memset(c.data(), 0, sizeof(JpegConst));
        build_const(g.rows, g.cols, g.nc, quality, c[0]);
        d_cst = uwip_table_put(ctx, key, c.data(), sizeof(JpegConst));
        if (!d_cst) return UWIP_ERR_HIP;
    }
    const JpegHuff *huff = static_cast<const JpegHuff *>(d_huff);
    const JpegConst *cst = static_cast<const JpegConst *>(d_cst);

    uwip_device dev(ctx);
    encode_sequence(dev, static_cast<const uint8_t *>(frames->data), g, F, huff, cst, d_streams, slot_bytes, d_sizes, d_count);
    return dev.finish();
}

UWIP_API int uwip_jpeg_encode_host(uwip_ctx *ctx, const uwip_batch_u8 *frames, int quality, uint8_t *h_streams, size_t slot_bytes,
                                   int64_t *h_sizes)
{
    return uwip_encode_to_host(ctx, frames, quality, h_streams, slot_bytes, h_sizes, uwip_jpeg_encode, "jpeg.streams", "jpeg.sizes");
}
