// PNG decoding of a batch on the device: imgio::read_png (cli/imgio.hpp, the reader of the CLIs) without the host inflate and
// without raw pixels on the link.  Where the status is 0 the pixels are the host reader's byte for byte, and the status is 0
// exactly where the host reader returns true and the size fits.  The chunk walk, the IHDR rules and the zlib header are checked
// on the host (png_parse.hpp, the host reader's walk); the IDAT payloads and one descriptor per frame and segment are uploaded.
// The stages, all on the context's stream, none waits for the host:
//   k_pngd_inflate  one wavefront per segment runs the one inflate loop of png_inflate.hpp (inflate_run: wave-uniform symbol
//                   decode, rounds of up to 64 tokens through LDS, then all lanes write the round) with the byte sink: inflated
//                   bytes go to the frame's workspace; back references read from there.
//                   Launch 0 decodes the segments the host parse proposed (cuts at IDAT boundaries behind 00 00 FF FF; segment
//                   i assumed to start at inflated offset i * 32768); launch 1, one wavefront per frame, accepts a frame all of
//                   whose segments report success and decodes every other frame again from its first byte.
//   k_pngs_*        segmented = 2 only, between the two launches: the found block starts for streams without such cuts, with
//                   their own header and loop bounds further down; a frame they accept is not decoded again by launch 1.
//   k_pngd_adler    (a, b) sums of every 32 KiB piece of the inflated bytes, 128 bytes per thread;
//   k_pngd_unfilter one wavefront per frame: the pieces' sums into the Adler-32 and its comparison with the stream's (a
//                   mismatch is UWIP_PNG_BAD_STREAM), then the row filters undone in place, 64 rows at a time on the diagonal:
//                   lane L has row r0 + L and is one pixel behind lane L - 1, whose last result (through LDS) is "up", whose
//                   result before that "upper left"; the band's first row reads the row above from memory;
//   k_pngd_color    one thread per pixel: the type byte and alpha dropped, RGB -> BGR or grey replicated, the caller's layout.
// What bounds the inflate loop on untrusted bytes, and what each of its three sinks adds, is stated once, with the loop, in
// png_inflate.hpp; what bounds the loops around it (the search, the chain walk, the marker passes) further down.
#include "uwip_internal.hpp"
#include "device_utils.hpp"
#include "png_inflate.hpp"
#include "png_parse.hpp"
#include <cstring>

namespace {

using namespace uwip_inflate;
using uwip_png::kAdlerMod;
using uwip_png::kChunk;

constexpr int kBand = 64;                                // rows per pass of the unfilter: one per lane
constexpr int kPngBad = -1;                              // UWIP_PNG_BAD_STREAM

struct PFrame {                 // per frame, from the host parse
    int32_t status, spp;
    uint32_t zoff, zlen;        // its zlib stream in the uploaded bytes
    uint32_t seg0, nseg;        // its segments of launch 0 (nseg 0: none, launch 1 decodes it)
    uint32_t chunk0, nchunks;   // found block starts: its chunk records (nchunks + kRepairs of them); nchunks < 2: not on that path
};
struct PSeg { uint32_t frame, idx, off, len; };          // input bytes [off, off + len) of the frame's stream
struct PRes { uint32_t ok, adler_pos, maxdist, pad; };   // per segment, then per frame: adler_pos in the frame's stream
struct PGeoD { int rows, cols; uint32_t ws_stride, npieces; };
// found block starts (segmented = 2): a chunk's measured run of whole blocks, and a frame's walk along the chain of them
struct PChunk { uint32_t start, end, nbytes, flags, out_off, adler_pos, tries, pad; };   // bits behind the zlib header; flags: kChunk*; tries: candidates decoded
struct PSpecFrame {
    uint32_t open, ok;          // still walking the chain; accepted (a later kernel that finds anything amiss takes it back)
    uint32_t end, out;          // the accepted chain ends at this bit and has produced this many bytes
    uint32_t nacc, nrep;        // accepted chunks (their records in order: PBufs::order), repair passes used
    uint32_t repair;            // the record the next repair pass measures from `end` into; kNone: nothing asked for
    uint32_t adler_pos;         // of an accepted frame: where the Adler-32 lies, in bytes behind the zlib header
};

struct PBufs {
    const PFrame *fr;
    const PSeg *seg;
    const uint8_t *src;
    uint8_t *ws;                // per frame ws_stride bytes: the inflated bytes, unfiltered in place
    PRes *res;                  // [nsegtot + frames]
    uint32_t *asum;             // [frames][npieces][2]
    int32_t *status;
    unsigned long long *counts; // segments accepted in launch 0, frames launch 1 decoded, frames
    uint32_t nsegtot, nframes;
    // found block starts; all null / 0 in the other modes
    PSpecFrame *spec = nullptr;
    PChunk *chunk = nullptr;
    uint32_t *order = nullptr;
    uint16_t *sym = nullptr;    // per frame ws_stride elements: a byte, or 0x8000 | k: the byte k + 1 before the chunk's first
    uint32_t chunk_bits = 0;
};

__device__ __forceinline__ uint32_t frame_total(const PGeoD &g, int spp) { return (uint32_t)g.rows * (1u + (uint32_t)g.cols * (uint32_t)spp); }

// pass 0: block s is segment s.  pass 1: block f is frame f -- accepted from its segments, or decoded again as a whole.
__global__ __launch_bounds__(64) void k_pngd_inflate(PBufs B, PGeoD g, int pass)
{
    __shared__ Tables T;
    const uint32_t lane = threadIdx.x;
    uint32_t f, a0, len, win, rslot;
    uint8_t *out;
    bool lastseg;
    if (pass == 0) {
        const PSeg sg = B.seg[blockIdx.x];
        f = sg.frame;
        const PFrame fr = B.fr[f];
        const uint32_t total = frame_total(g, fr.spp), base = sg.idx * (uint32_t)kChunk;
        rslot = blockIdx.x;
        lastseg = sg.idx + 1u == fr.nseg;
        if ((uint64_t)sg.idx * (uint64_t)kChunk > (uint64_t)total) {                                   // its window lies behind the frame: refused
            if (lane == 0) B.res[rslot] = PRes{0u, 0u, 0u, 0u};
            return;
        }
        a0 = fr.zoff + sg.off; len = sg.len;
        win = lastseg ? total - base : min((uint32_t)kChunk, total - base);
        out = B.ws + (size_t)f * g.ws_stride + base;
    } else {
        f = blockIdx.x;
        const PFrame fr = B.fr[f];
        rslot = B.nsegtot + f;
        if (f == 0u && lane == 0u) B.counts[2] = B.nframes;
        if (fr.status != 0) {
            if (lane == 0) { B.status[f] = fr.status; B.res[rslot] = PRes{0u, 0u, 0u, 0u}; }
            return;
        }
        if (B.spec && B.spec[f].ok) {                         // accepted from found block starts: its bytes are in the workspace
            if (lane == 0) {
                B.status[f] = 0;
                B.res[rslot] = PRes{1u, 2u + B.spec[f].adler_pos, 0u, 0u};
                atomicAdd(&B.counts[0], (unsigned long long)B.spec[f].nacc);
            }
            return;
        }
        if (fr.nseg) {
            if (lane == 0) T.bad = 0u;
            __syncthreads();
            uint32_t nb = 0;
            for (uint32_t s = lane; s < fr.nseg; s += 64u) nb += B.res[fr.seg0 + s].ok ? 0u : 1u;
            if (nb) atomicAdd(&T.bad, nb);
            __syncthreads();
            const uint32_t bad = T.bad;
            if (bad == 0u || fr.nseg == 1u) {                 // one segment is the whole stream: its answer stands
                if (lane == 0) {
                    B.status[f] = bad ? kPngBad : 0;
                    B.res[rslot] = B.res[fr.seg0 + fr.nseg - 1u];
                }
                return;
            }
        }
        if (lane == 0) atomicAdd(&B.counts[1], 1ull);
        a0 = fr.zoff + 2u; len = fr.zlen - 2u;                // zlen >= 2: the host parse read the zlib header
        win = frame_total(g, fr.spp);
        out = B.ws + (size_t)f * g.ws_stride;
        lastseg = true;
    }
    // A segment that is not the last reports success only if it ended exactly at its input's last bit, behind an empty stored
    // block that was not final; the last segment, or the whole stream, only if it ended with the final block.  Both only with
    // exactly their window produced (and ByteSink: no match reached before the segment's own first byte).
    const uint32_t lenbits = len * 8u;
    const InflateRun r = inflate_run(T, B.src, a0, len, 0u, lastseg ? kNone : lenbits, ByteSink{out}, win);
    const bool ok = r.ok && r.nbytes == win && (lastseg ? r.final_blk : !r.final_blk && r.last_empty && r.end == lenbits);
    if (lane == 0) {
        B.res[rslot] = PRes{ok ? 1u : 0u, a0 - B.fr[f].zoff + r.adler_pos, r.maxdist, 0u};
        if (pass == 0) { if (ok) atomicAdd(&B.counts[0], 1ull); }
        else B.status[f] = ok ? 0 : kPngBad;
    }
}

__global__ __launch_bounds__(256) void k_pngd_adler(PBufs B, PGeoD g)
{
    __shared__ uint32_t s_scan[8];
    const int f = blockIdx.y, t = threadIdx.x;
    if (B.status[f] != 0) return;
    const uint32_t total = frame_total(g, B.fr[f].spp), base = blockIdx.x * (uint32_t)kChunk;
    if (base >= total) return;
    const int n = (int)min((uint32_t)kChunk, total - base);
    const uint8_t *d = B.ws + (size_t)f * g.ws_stride + base;
    const int b0 = min(t * (kChunk / 256), n), b1 = min(b0 + kChunk / 256, n);
    uint32_t sa = 0, sb = 0;
    for (int p = b0; p < b1; ++p) { sa += d[p]; sb += (uint32_t)(n - p) * d[p]; }          // < 128 * 32768 * 255
    const uint32_t a = block256_sum_u32(sa % kAdlerMod, s_scan) % kAdlerMod;
    const uint32_t b = block256_sum_u32(sb % kAdlerMod, s_scan) % kAdlerMod;
    if (t == 0) { uint32_t *q = B.asum + ((size_t)f * g.npieces + blockIdx.x) * 2; q[0] = a; q[1] = b; }
}

__global__ __launch_bounds__(64) void k_pngd_unfilter(PBufs B, PGeoD g)
{
    __shared__ uint32_t s_px[2][kBand];
    __shared__ uint32_t s_bad;
    const int f = blockIdx.x, lane = threadIdx.x;
    if (B.status[f] != 0) return;
    const PFrame fr = B.fr[f];
    const int spp = fr.spp, rows = g.rows, cols = g.cols;
    const uint32_t total = frame_total(g, spp);
    if (lane == 0) {
        uint32_t A = 1, Bs = 0;
        for (uint32_t p = 0; p * (uint32_t)kChunk < total; ++p) {
            const uint32_t *q = B.asum + ((size_t)f * g.npieces + p) * 2;
            uwip_png::adler_append(A, Bs, q[0], q[1], min((uint32_t)kChunk, total - p * (uint32_t)kChunk));
        }
        const uint8_t *z = B.src + fr.zoff + B.res[B.nsegtot + f].adler_pos;       // four bytes inside the stream (checked)
        const uint32_t stored = ((uint32_t)z[0] << 24) | ((uint32_t)z[1] << 16) | ((uint32_t)z[2] << 8) | z[3];
        s_bad = stored != ((Bs << 16) | A);
    }
    __syncthreads();
    if (s_bad) {                                                                   // written behind the barrier: every lane has read it
        if (lane == 0) B.status[f] = kPngBad;
        return;
    }
    uint8_t *ws = B.ws + (size_t)f * g.ws_stride;
    const size_t rstride = (size_t)cols * spp + 1;
    for (int r0 = 0; r0 < rows; r0 += kBand) {
        const int y = r0 + lane;
        const bool active = y < rows;
        uint8_t *row = ws + (size_t)(active ? y : 0) * rstride + 1;
        int ft = active ? row[-1] : 0;
        if (ft > 4) ft = 0;                                                        // the host loop's default
        const uint8_t *up = (lane == 0 && r0 > 0) ? row - rstride : nullptr;
        uint32_t a = 0, c = 0;                                                     // the pixel to the left, the one above it
        const int nsteps = cols + min(kBand, rows - r0) - 1;
        for (int s = 0; s < nsteps; ++s) {
            const int x = s - lane;
            uint32_t res = 0;
            if (active && x >= 0 && x < cols) {
                uint32_t b = 0;
                if (lane > 0) b = s_px[(s - 1) & 1][lane - 1];
                else if (up) for (int k = 0; k < spp; ++k) b |= (uint32_t)up[(size_t)x * spp + k] << (8 * k);
                for (int k = 0; k < spp; ++k) {
                    const int av = (a >> (8 * k)) & 255, bv = (b >> (8 * k)) & 255, cv = (c >> (8 * k)) & 255;
                    int v = row[(size_t)x * spp + k];
                    v += ft == 1 ? av : ft == 2 ? bv : ft == 3 ? (av + bv) >> 1 : ft == 4 ? uwip_png::paeth(av, bv, cv) : 0;
                    row[(size_t)x * spp + k] = (uint8_t)v;
                    res |= (uint32_t)(v & 255) << (8 * k);
                }
                a = res; c = b;
            }
            s_px[s & 1][lane] = res;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void k_pngd_color(PBufs B, PGeoD g, uint8_t *out, size_t step, size_t fs, int channels)
{
    const int f = blockIdx.y;
    if (B.status[f] != 0) return;
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= (uint32_t)g.rows * (uint32_t)g.cols) return;
    const int spp = B.fr[f].spp;
    const uint32_t y = q / (uint32_t)g.cols, x = q - y * (uint32_t)g.cols;
    const uint8_t *s = B.ws + (size_t)f * g.ws_stride + (size_t)y * ((size_t)g.cols * spp + 1) + 1 + (size_t)x * spp;
    uint8_t *p = out + (size_t)f * fs + (size_t)y * step + (size_t)x * channels;
    if (channels == 1) p[0] = s[0];                                                // grey streams only (the host's rule)
    else if (spp <= 2) p[0] = p[1] = p[2] = s[0];
    else { p[0] = s[2]; p[1] = s[1]; p[2] = s[0]; }
}

// ---- found block starts (segmented = 2) ------------------------------------------------------------------------
// A stream without flush points is cut into chunks of chunk_bytes compressed bytes.  Kernels, each one launch, no workgroup
// waits for another -- the order between chunks comes from the kernel boundaries alone:
//   k_pngs_begin    one thread per frame: which frames take this path (good, at least two chunks, not accepted from segments);
//   k_pngs_measure  one wavefront per (chunk, frame).  Chunk 0 starts behind the zlib header.  Every other chunk looks for
//                   the first bit of its range that passes as the start of a dynamic block: the lanes screen kScreen x 64
//                   positions a round in registers (dynamic_start_plausible), the first that passes gets dynamic_header, and
//                   from there the wavefront decodes lengths only (inflate_run without a sink) through whole blocks up to the
//                   first block boundary at or behind the end of its range.  A decode that fails discards the candidate and
//                   the search goes on one bit later.  The record: start bit, end bit, bytes produced.
//                   As a repair pass (one wavefront per frame) it measures from the accepted chain's end, any block type;
//   k_pngs_verify   one thread per frame walks the chain: the chunk whose range holds the chain's end is accepted iff it
//                   starts exactly there, and gets the chain's byte count as its output offset; otherwise a repair pass is
//                   asked for (kRepairs of them per call), and the frame is given up when they are spent;
//   k_pngs_write    one wavefront per accepted chunk decodes again, the same loop with the element sink: 16-bit elements;
//   k_pngs_window   one workgroup per frame, the chunks in order: the markers in a chunk's last 32 768 elements become bytes;
//   k_pngs_resolve  one workgroup per accepted chunk: elements to bytes in the frame's workspace.
// What bounds the loops around inflate_run on untrusted bytes: the search position only grows and ends at the chunk's range,
// and at most kMaxTries candidates of a chunk get the full decode; a measured run may not produce more than the frame's bytes
// (its window); verify accepts a chunk only inside the frame (out_off + nbytes <= total, total <= ws_stride), each acceptance
// moves to a later range, so its loop takes at most nchunks steps; the window of k_pngs_write is the chunk's measured length;
// k_pngs_window and k_pngs_resolve form a source index only where k + 1 <= out_off, and their element loops run over measured
// lengths.
constexpr uint32_t kChunkValid = 1u, kChunkFinal = 2u;
constexpr int kRepairs = 4;                              // repair passes per call
constexpr int kScreen = 4;                               // bit positions a lane screens per round
constexpr int kMaxTries = 256;                           // candidates of one chunk that get the full decode
constexpr uint32_t kSpecChunkDefault = 16384;            // chunk_bytes 0

__global__ __launch_bounds__(64) void k_pngs_begin(PBufs B)
{
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= B.nframes) return;
    const PFrame fr = B.fr[f];
    bool open = fr.status == 0 && fr.nchunks >= 2u;
    if (open && fr.nseg) {                                   // its segments ran: accepted there, it is finished
        uint32_t bad = 0;
        for (uint32_t s = 0; s < fr.nseg; ++s) bad += B.res[fr.seg0 + s].ok ? 0u : 1u;
        open = bad != 0u;
    }
    B.spec[f] = PSpecFrame{open ? 1u : 0u, 0u, 0u, 0u, 0u, 0u, kNone, 0u};
}

// repair 0: block (c, f) is chunk c of frame f.  repair 1: block (0, f) measures from the chain's end, where verify asked for it.
__global__ __launch_bounds__(64) void k_pngs_measure(PBufs B, PGeoD g, int repair)
{
    __shared__ Tables T;
    __shared__ uint32_t s_first[2];
    const uint32_t lane = threadIdx.x, f = blockIdx.y;
    const PFrame fr = B.fr[f];
    const PSpecFrame sp = B.spec[f];
    if (!sp.open) return;
    uint32_t c = blockIdx.x, lo, slot;
    if (repair) {
        if (sp.repair == kNone) return;
        lo = sp.end; c = lo / B.chunk_bits; slot = sp.repair;
    } else {
        if (c >= fr.nchunks) return;
        lo = c * B.chunk_bits; slot = c;
    }
    const uint32_t a0 = fr.zoff + 2u, len = fr.zlen - 2u, lenbits = len * 8u, total = frame_total(g, fr.spp);
    const uint32_t hi = min((c + 1u) * B.chunk_bits, lenbits);
    const uint8_t *src = B.src;
    InflateRun r{0u, 0u, 0u, 0u, false, false, false};
    uint32_t start = lo;
    int tries = 0;
    if (repair || c == 0u) r = inflate_run(T, src, a0, len, lo, hi, LengthsOnly{}, total);
    else {
        uint32_t p = lo;
        int par = 0;
        while (p < hi && tries < kMaxTries) {
            if (lane == 0) s_first[par] = kNone;
            __syncthreads();
            uint32_t mine = kNone;
            for (int j = 0; j < kScreen && mine == kNone; ++j) {
                const uint32_t q = p + lane + 64u * (uint32_t)j;
                if (q >= hi) break;
                const uint32_t v = peek32(src, a0, len, q);
                const uint64_t w = (uint64_t)peek32(src, a0, len, q + 17u) | ((uint64_t)peek32(src, a0, len, q + 49u) << 32);
                if (dynamic_start_plausible(v, w)) mine = q;
            }
            if (mine != kNone) atomicMin(&s_first[par], mine);
            __syncthreads();
            const uint32_t q = s_first[par];
            par ^= 1;
            if (q == kNone) { p += 64u * (uint32_t)kScreen; continue; }
            ++tries;
            r = inflate_run(T, src, a0, len, q, hi, LengthsOnly{}, total);      // the screen saw BTYPE 2 at q: a dynamic block
            if (r.ok) { start = q; break; }
            p = q + 1u;
        }
    }
    if (lane == 0)
        B.chunk[fr.chunk0 + slot] = PChunk{start, r.end, r.nbytes, r.ok ? (kChunkValid | (r.final_blk ? kChunkFinal : 0u)) : 0u, 0u, r.adler_pos, (uint32_t)tries, 0u};
}

__global__ __launch_bounds__(64) void k_pngs_verify(PBufs B, PGeoD g)
{
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= B.nframes) return;
    PSpecFrame sp = B.spec[f];
    if (!sp.open) return;
    const PFrame fr = B.fr[f];
    const uint32_t total = frame_total(g, fr.spp);
    PChunk *ch = B.chunk + fr.chunk0;
    uint32_t *order = B.order + fr.chunk0;
    sp.open = 0u;                                            // unless a repair is asked for below
    for (;;) {                                               // an accepted chunk ends in a later range (or the stream): <= nchunks steps
        const bool repaired = sp.repair != kNone;
        uint32_t slot = sp.repair;
        sp.repair = kNone;
        if (!repaired) {
            slot = sp.end / B.chunk_bits;
            if (slot >= fr.nchunks) break;
        }
        const PChunk k = ch[slot];
        if (!(k.flags & kChunkValid) || k.start != sp.end) {  // nothing starts where the chain ends
            if (!repaired && sp.nrep < (uint32_t)kRepairs) { sp.repair = fr.nchunks + sp.nrep; ++sp.nrep; sp.open = 1u; }
            break;
        }
        if (k.nbytes > total - sp.out || sp.nacc >= fr.nchunks + (uint32_t)kRepairs) break;
        ch[slot].out_off = sp.out;
        order[sp.nacc++] = slot;
        sp.end = k.end; sp.out += k.nbytes;
        if (k.flags & kChunkFinal) {
            sp.ok = sp.out == total ? 1u : 0u;
            sp.adler_pos = k.adler_pos;
            break;
        }
    }
    B.spec[f] = sp;
}

__global__ __launch_bounds__(64) void k_pngs_write(PBufs B, PGeoD g)
{
    __shared__ Tables T;
    const uint32_t f = blockIdx.y;
    const PSpecFrame sp = B.spec[f];
    if (!sp.ok || blockIdx.x >= sp.nacc) return;
    const PFrame fr = B.fr[f];
    const PChunk k = B.chunk[fr.chunk0 + B.order[fr.chunk0 + blockIdx.x]];
    uint16_t *out = B.sym + (size_t)f * g.ws_stride + k.out_off;
    const InflateRun r = inflate_run(T, B.src, fr.zoff + 2u, fr.zlen - 2u, k.start, k.end, ElemSink{out, k.out_off}, k.nbytes);
    if (!(r.ok && r.end == k.end && r.nbytes == k.nbytes) && threadIdx.x == 0) B.spec[f].ok = 0u;
}

__global__ __launch_bounds__(256) void k_pngs_window(PBufs B, PGeoD g)
{
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    const PSpecFrame sp = B.spec[f];
    if (!sp.ok) return;
    const PFrame fr = B.fr[f];
    uint16_t *sym = B.sym + (size_t)f * g.ws_stride;
    bool bad = false;
    for (uint32_t i = 0; i < sp.nacc; ++i) {
        const PChunk k = B.chunk[fr.chunk0 + B.order[fr.chunk0 + i]];
        // a marker's source lies in the 32 768 bytes before this chunk: in the last 32 768 elements of earlier chunks, all bytes by now
        for (uint32_t e = (k.nbytes > (uint32_t)kChunk ? k.nbytes - (uint32_t)kChunk : 0u) + t; e < k.nbytes; e += 256u) {
            const uint32_t v = sym[k.out_off + e];
            if (!(v & kMarker)) continue;
            const uint32_t back = (v & 0x7FFFu) + 1u;
            const uint32_t s = back <= k.out_off ? sym[k.out_off - back] : (uint32_t)kMarker;
            if (s & kMarker) bad = true;
            else sym[k.out_off + e] = (uint16_t)s;
        }
        __syncthreads();
    }
    if (bad) B.spec[f].ok = 0u;
}

__global__ __launch_bounds__(256) void k_pngs_resolve(PBufs B, PGeoD g)
{
    const uint32_t f = blockIdx.y, t = threadIdx.x;
    const PSpecFrame sp = B.spec[f];
    if (!sp.ok || blockIdx.x >= sp.nacc) return;
    const PFrame fr = B.fr[f];
    const PChunk k = B.chunk[fr.chunk0 + B.order[fr.chunk0 + blockIdx.x]];
    const uint16_t *sym = B.sym + (size_t)f * g.ws_stride;
    uint8_t *out = B.ws + (size_t)f * g.ws_stride + k.out_off;
    bool bad = false;
    for (uint32_t e = t; e < k.nbytes; e += 256u) {
        uint32_t v = sym[k.out_off + e];
        if (v & kMarker) {
            const uint32_t back = (v & 0x7FFFu) + 1u;
            v = back <= k.out_off ? sym[k.out_off - back] : (uint32_t)kMarker;
            if (v & kMarker) bad = true;
        }
        out[e] = (uint8_t)v;
    }
    if (bad) B.spec[f].ok = 0u;
}

// ---- the host side ----------------------------------------------------------------------------------------------------------
struct PPlan {
    size_t src_bytes = 0, nseg = 0;
    bool too_large = false;
};

// the per-frame workspace comes from the batch's geometry at four samples per pixel, never from an IHDR
size_t ws_bytes(int rows, int cols) { return (((size_t)rows * ((size_t)cols * 4 + 1)) + 15) & ~(size_t)15; }

// a frame's descriptor and segments from its parse; segmented: one segment per proposed cut and one behind the last
void plan_frame(PFrame &d, const uwip_pngd::Parsed &p, int rows, int cols, int segmented, std::vector<PSeg> &segs, int f, PPlan &pl)
{
    d.zoff = (uint32_t)pl.src_bytes; d.zlen = (uint32_t)p.zlen;
    pl.src_bytes += (p.zlen + 31) & ~(size_t)15;
    d.seg0 = (uint32_t)segs.size(); d.nseg = 0;
    if (segmented == 1 || (segmented == 2 && !p.cuts.empty())) {      // 2: a stream without cuts is left to the found block starts
        size_t at = 2;
        uint32_t i = 0;
        for (size_t c : p.cuts) { segs.push_back(PSeg{(uint32_t)f, i++, (uint32_t)at, (uint32_t)(c - at)}); at = c; }
        segs.push_back(PSeg{(uint32_t)f, i++, (uint32_t)at, (uint32_t)(p.zlen - at)});
        d.nseg = i;
    }
    if (pl.src_bytes >= ((size_t)1 << 31)) pl.too_large = true;
}

// ---- the host side of the found block starts ----
// chunk_bytes 0 is the library's choice; the records of frame f: nchunks for its chunks, kRepairs behind them
uint32_t spec_chunk_bytes(int32_t asked) { return asked ? (uint32_t)asked : kSpecChunkDefault; }
void spec_plan_frame(PFrame &d, uint32_t chunk_bytes, size_t &nslots, uint32_t &maxslots)
{
    const size_t len = d.zlen - 2u;
    d.nchunks = (uint32_t)((len + chunk_bytes - 1) / chunk_bytes);
    d.chunk0 = (uint32_t)nslots;
    if (d.nchunks < 2u) { d.nchunks = 0u; return; }
    nslots += d.nchunks + kRepairs;
    maxslots = std::max(maxslots, d.nchunks + (uint32_t)kRepairs);
}
// the records of the found block starts share one buffer: a PSpecFrame per frame, then per chunk record a PChunk, then its place
// in the chain's order, and 16 spare bytes.  The one statement of that layout: the byte count and the pointers both come from it
struct SpecLayout {
    size_t chunk, order, bytes;
    SpecLayout(size_t n, size_t nslots)
        : chunk(n * sizeof(PSpecFrame)), order(chunk + nslots * sizeof(PChunk)), bytes(order + nslots * sizeof(uint32_t) + 16) {}
};
size_t spec_meta_bytes(size_t n, size_t nslots) { return SpecLayout(n, nslots).bytes; }
void spec_bind(PBufs &B, void *meta, void *sym, size_t n, size_t nslots, uint32_t chunk_bytes)
{
    const SpecLayout l(n, nslots);
    uint8_t *m = static_cast<uint8_t *>(meta);
    B.spec = reinterpret_cast<PSpecFrame *>(m);
    B.chunk = reinterpret_cast<PChunk *>(m + l.chunk);
    B.order = reinterpret_cast<uint32_t *>(m + l.order);
    B.sym = static_cast<uint16_t *>(sym);
    B.chunk_bits = chunk_bytes * 8u;
}

// uwip_png_decode behind the upload, on either back end (uwip_device; the host threads of tests/hip_on_host.hpp): the working
// arrays, their first values and every launch of the three modes.  fr / seg / src: the descriptors, the nsegtot segments of
// launch 0 and the zlib streams, where the kernels read them; nslots / maxslots: the chunk records of the found block starts
// over the batch and the most a frame has (spec_plan_frame), 0 where no frame takes that path.
template <class BE>
void decode_sequence(BE &be, const PFrame *fr, const PSeg *seg, const uint8_t *src, size_t nsegtot, size_t nslots, uint32_t maxslots,
                     uint32_t chunk_bytes, int n, const uwip_batch_u8 &out, int32_t *d_status, void *d_counts)
{
    using dim3 = typename BE::dim3;                           // HIP's on the device, its stand-in on host threads
    const size_t wsb = ws_bytes(out.rows, out.cols);
    PGeoD g;
    g.rows = out.rows; g.cols = out.cols; g.ws_stride = (uint32_t)wsb; g.npieces = (uint32_t)((wsb + kChunk - 1) / kChunk);
    PBufs B;
    B.fr = fr; B.seg = seg; B.src = src; B.status = d_status;
    B.nsegtot = (uint32_t)nsegtot; B.nframes = (uint32_t)n;
    B.ws = be.template array<uint8_t>("pngdec.inflated", (size_t)n * wsb + 16);
    B.counts = be.template array<unsigned long long>("pngdec.counts", 3);
    B.res = be.template array<PRes>("pngdec.res", nsegtot + n);
    B.asum = be.template array<uint32_t>("pngdec.asum", (size_t)n * g.npieces * 2);
    if (nslots) {                                             // only where the found block starts are used
        spec_bind(B, be.template array<uint8_t>("pngdec.chunks", spec_meta_bytes((size_t)n, nslots)),
                  be.template array<uint16_t>("pngdec.symbols", (size_t)n * wsb), (size_t)n, nslots, chunk_bytes);
    }
    be.fill(B.counts, 0, 3 * sizeof(unsigned long long));
    if (nsegtot) be.launch("k_pngd_inflate_segments", k_pngd_inflate, dim3((unsigned)nsegtot), 64, B, g, 0);
    if (nslots) {
        const unsigned nb = uwip_cdiv((size_t)n, 64);
        be.launch("k_pngs_begin", k_pngs_begin, dim3(nb), 64, B);
        be.launch("k_pngs_measure", k_pngs_measure, dim3(maxslots - kRepairs, n), 64, B, g, 0);
        be.launch("k_pngs_verify", k_pngs_verify, dim3(nb), 64, B, g);
        for (int r = 0; r < kRepairs; ++r) {
            be.launch("k_pngs_measure_repair", k_pngs_measure, dim3(1, n), 64, B, g, 1);
            be.launch("k_pngs_verify", k_pngs_verify, dim3(nb), 64, B, g);
        }
        be.launch("k_pngs_write", k_pngs_write, dim3(maxslots, n), 64, B, g);
        be.launch("k_pngs_window", k_pngs_window, dim3(n), 256, B, g);
        be.launch("k_pngs_resolve", k_pngs_resolve, dim3(maxslots, n), 256, B, g);
    }
    be.launch("k_pngd_inflate", k_pngd_inflate, dim3(n), 64, B, g, 1);
    be.launch("k_pngd_adler", k_pngd_adler, dim3(g.npieces, n), 256, B, g);
    be.launch("k_pngd_unfilter", k_pngd_unfilter, dim3(n), 64, B, g);
    be.launch("k_pngd_color", k_pngd_color, dim3(uwip_cdiv((size_t)out.rows * out.cols, 256), n), 256, B, g, static_cast<uint8_t *>(out.data),
              out.step, out.frame_stride, out.channels);
    if (d_counts) be.copy(d_counts, B.counts, 3 * sizeof(unsigned long long));
}

}  // namespace

UWIP_API int uwip_png_info(const uint8_t *buf, size_t len, int32_t *rows, int32_t *cols, int32_t *channels)
{
    if (!buf || !rows || !cols || !channels) return UWIP_ERR_INVALID;
    int r = 0, c = 0, ch = 0;
    if (uwip_pngd::info(buf, len, &r, &c, &ch) != uwip_pngd::PARSE_OK) return UWIP_ERR_UNSUPPORTED;
    *rows = r; *cols = c; *channels = ch;
    return UWIP_OK;
}

UWIP_API int uwip_png_decode(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                             const uwip_png_decode_opts *opts, int32_t *d_status)
{
    const int mode = opts ? opts->segmented : -1, asked = opts ? opts->chunk_bytes : 0;
    const bool opts_ok = mode >= -1 && mode <= 2 && (asked == 0 || (mode == 2 && asked >= 256 && asked <= (1 << 20)));
    if (!ctx) {                                               // no context: because there is no device, or a plain bad argument
        if (!opts_ok) return UWIP_ERR_INVALID;
        int ndev = 0;
        return (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) ? UWIP_ERR_HIP : UWIP_ERR_INVALID;
    }
    int rc = uwip_check_batch(ctx, out, 0);
    if (rc) return rc;
    UWIP_REQUIRE(ctx, opts_ok, "segmented must be -1, 0, 1 or 2; chunk_bytes 0, or 256 .. 1 MiB with segmented 2");
    rc = uwip_check_streams(ctx, h_streams, h_sizes, n, out, d_status);
    if (rc || n == 0) return rc;
    UWIP_REQUIRE(ctx, out->rows <= 65535 && out->cols <= 65535, "at most 65535 rows / columns");
    const int segmented = mode < 0 ? 1 : mode;
    const uint32_t chunk_bytes = spec_chunk_bytes(asked);
    const size_t wsb = ws_bytes(out->rows, out->cols);
    UWIP_REQUIRE(ctx, wsb < ((size_t)1 << 31), "frame too large");

    std::vector<uwip_pngd::Parsed> parsed((size_t)n);
    std::vector<PFrame> fr((size_t)n);
    std::vector<PSeg> segs;
    PPlan pl;
    size_t nslots = 0;                                        // chunk records of the found block starts
    uint32_t maxslots = 0;
    for (int f = 0; f < n; ++f) {
        PFrame &d = fr[f];
        std::memset(&d, 0, sizeof d);
        uwip_pngd::Parsed &p = parsed[f];
        d.status = uwip_pngd::parse(h_streams[f], h_sizes[f], p);
        if (d.status == 0 && ((int64_t)p.H != out->rows || (int64_t)p.W != out->cols || (p.spp >= 3 && out->channels == 1)))
            d.status = UWIP_PNG_SIZE_MISMATCH;
        d.spp = d.status == 0 ? p.spp : 1;
        if (d.status == 0) {
            plan_frame(d, p, out->rows, out->cols, segmented, segs, f, pl);
            if (segmented == 2) spec_plan_frame(d, chunk_bytes, nslots, maxslots);
        }
    }
    UWIP_REQUIRE(ctx, !pl.too_large && segs.size() < ((size_t)1 << 24) && nslots < ((size_t)1 << 24), "batch too large for one call");

    // The page-locked staging buffer holds the descriptors, the segments, then the zlib streams.  It is free again once the
    // previous call's upload has finished: poll that event (the stream is not drained) before the buffer is touched.
    static_assert(sizeof(PFrame) % 16 == 0 && sizeof(PSeg) == 16, "the streams follow the descriptors at a 16-byte boundary");
    if (!ctx->pngd_ev) UWIP_HIP(ctx, hipEventCreateWithFlags(&ctx->pngd_ev, hipEventDisableTiming));
    else UWIP_HIP(ctx, uwip_event_wait(ctx->pngd_ev, 200));
    const size_t nsegtot = segs.size(), hdr = (size_t)n * sizeof(PFrame) + nsegtot * sizeof(PSeg);
    const size_t in_bytes = hdr + pl.src_bytes + 16;
    uint8_t *h_in = static_cast<uint8_t *>(uwip_host_ws(ctx, "pngdec.in", in_bytes));
    if (!h_in) return UWIP_ERR_NOMEM;
    std::memcpy(h_in, fr.data(), (size_t)n * sizeof(PFrame));
    if (nsegtot) std::memcpy(h_in + (size_t)n * sizeof(PFrame), segs.data(), nsegtot * sizeof(PSeg));
    for (int f = 0; f < n; ++f)
        if (fr[f].status == 0) uwip_pngd::gather(h_streams[f], parsed[f], h_in + hdr + fr[f].zoff);
    std::memset(h_in + hdr + pl.src_bytes, 0, 16);

    uint8_t *d_in = static_cast<uint8_t *>(uwip_ws(ctx, "pngdec.in", in_bytes));
    if (!d_in) return UWIP_ERR_NOMEM;
    UWIP_HIP(ctx, hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    UWIP_HIP(ctx, hipEventRecord(ctx->pngd_ev, ctx->stream));

    uwip_device dev(ctx);
    decode_sequence(dev, reinterpret_cast<const PFrame *>(d_in), reinterpret_cast<const PSeg *>(d_in + (size_t)n * sizeof(PFrame)), d_in + hdr,
                    nsegtot, nslots, maxslots, chunk_bytes, n, *out, d_status, opts ? opts->d_counts : nullptr);
    return dev.finish();
}

UWIP_API int uwip_png_decode_host(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                                  const uwip_png_decode_opts *opts, int32_t *h_status)
{
    if (!ctx) return uwip_png_decode(ctx, h_streams, h_sizes, n, out, opts, nullptr);
    return uwip_decode_to_host(ctx, h_streams, h_sizes, n, out, opts, h_status, uwip_png_decode, "pngdec.status");
}
