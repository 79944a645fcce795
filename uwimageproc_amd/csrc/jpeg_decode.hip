// Baseline JPEG decoding of a batch on the device: cv::imread / cv::imdecode without the host codec and without raw pixels on
// the link.  The arithmetic follows jpeg::decode of cli/jpeg.hpp (the host codec of the CLIs) step for step, so a frame with
// status 0 holds the same bytes: Huffman decoding with the host's rule for bits past the end of a segment (zeros), the
// clamped dequantisation and jidctint in 64-bit temporaries (jpeg_core.hpp, shared with the host), jdsample's fancy h2v1 /
// h2v2 upsampling, jdcolor's fixed point.  The header is parsed on the host (jpeg_parse.hpp, the host decoder's parse); only the entropy-coded segments and one descriptor per frame are
// uploaded.  The stages, all on the context's stream, none waits for the host:
//   k_jpd_unstuff   one workgroup per frame, 4 KiB per step (count, scan, copy with a running base): FF 00 -> FF, RSTn taken
//                   out and its place recorded as the start of the next restart interval, stop at any other marker; then
//                   the subsequences per interval (128 bytes each, at least one) by a scan over the intervals.  A restart
//                   layout other than ceil(MCUs / Ri) - 1 markers in cyclic order is UWIP_JPEG_HOST_ONLY.
//   k_jpd_round     one lane per subsequence.  Round 0 decodes from the first bit of the subsequence in state (block 0 of
//                   the MCU, coefficient 0), writes nothing, and records the state (bit, block in MCU, zig-zag index) it
//                   left with and the blocks it completed.  A sync round decodes again from the state the lane before left
//                   with, unless that is the state the lane last started from (exit states are double-buffered).
//   k_jpd_check     a lane is settled when it last started from its predecessor's exit state; lane 0 of an interval starts
//                   from a known state, so everything before the first unsettled lane of an interval is the true decode.
//   k_jpd_cleanup   one lane per interval walks on serially from that first unsettled lane (sync_rounds 0: the whole
//                   interval): correct whether or not the stream synchronised.
//   k_jpd_blkscan   segmented scan of the completed blocks: the block each lane starts in.
//   k_jpd_write     every lane decodes once more from its true entry state and writes the quantised coefficients, int16,
//                   natural order, DC as the difference; an undecodable code, a DC category above 11 or a run past
//                   coefficient 63 before the interval's last block is UWIP_JPEG_BAD_STREAM.
//   k_jpd_dc        segmented scan of the DC differences per component and interval, with the host's 16-bit range check.
//   k_jpd_idct      one thread per block into the MCU-padded component planes.
//   k_jpd_color     one thread per pixel: upsampling, YCbCr -> BGR, the caller's layout.
// Speculative passes stop at the end of the subsequence plus one symbol (<= 31 bits) and report an undecodable code only as
// "unsettled"; all table indices are masked or checked; a bit position at or past the interval's last byte reads zeros
// without touching memory.
#include "uwip_internal.hpp"
#include "device_utils.hpp"
#include "jpeg_core.hpp"
#include "jpeg_parse.hpp"
#include <cstring>

namespace {

using uwip_jpeg::DecFrame;
using uwip_jpeg::DecHuff;
using uwip_jpeg::clamp_coef;
using uwip_jpeg::descale64;
using uwip_jpeg::extend;
using uwip_jpeg::idct_pass;

constexpr int kSubBytes = 128;                  // subsequence length (the device JPEG decoder)
constexpr uint32_t kSubBits = kSubBytes * 8;
constexpr int kDefaultRounds = 8;
constexpr uint64_t kInvalid = ~0ull;            // exit state of a lane that met an undecodable code
constexpr int kStBad = -1, kStHostOnly = -3;    // UWIP_JPEG_BAD_STREAM, UWIP_JPEG_HOST_ONLY

struct DecBufs {
    const DecFrame *fr;
    const uint8_t *src;             // the uploaded segments
    uint8_t *ubuf;                  // unstuffed bytes
    uint32_t *istart, *isub, *ifirst;       // per interval: first unstuffed byte, first subsequence, first unsettled lane
    uint64_t *exit0, *exit1, *entry;        // per subsequence: exit state (two buffers), the entry state last decoded from
    uint32_t *cnt, *sblk, *sint;            // per subsequence: blocks completed, first block, interval
    int16_t *coef;
    uint8_t *planes;
    int32_t *status;
    int32_t *err;                   // per frame: non-zero once a kernel found the stream undecodable (merged into status last)
    unsigned long long *stats;      // [2]: unsettled lanes after the sync rounds, lanes
};

__device__ __forceinline__ uint64_t pack_state(uint32_t p, uint32_t b, uint32_t k) { return ((uint64_t)p << 32) | (b << 8) | k; }

// ---- unstuffing ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_jpd_unstuff(DecBufs B)
{
    __shared__ uint32_t s_scan[8], s_term, s_tot, s_bad;
    const int f = blockIdx.x;
    const DecFrame &d = B.fr[f];
    const int32_t st0 = d.status;
    if (threadIdx.x == 0) { B.status[f] = st0; s_bad = 0u; }
    if (st0 != 0) return;
    const uint8_t *in = B.src + d.seg_off;
    const uint32_t n = d.seg_len, nint = (uint32_t)d.nint;
    uint8_t *out = B.ubuf + d.ubase;
    uint32_t *istart = B.istart + d.ibase, *isub = B.isub + d.ibase;
    if (threadIdx.x == 0) istart[0] = 0u;
    uint32_t kept = 0, rsts = 0;
    bool bad = false;
    for (uint32_t base = 0; base < n; base += 4096u) {
        if (threadIdx.x == 0) s_term = 0xFFFFFFFFu;
        __syncthreads();
        const uint32_t p0 = base + threadIdx.x * 16u;
        uint8_t b[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) {
            const uint32_t i = p0 + (uint32_t)k;                     // byte i - 1
            b[k] = (i >= 1u && i - 1u < n) ? in[i - 1u] : (uint8_t)(i == 0u ? 0x00 : 0x01);      // past the end: a marker follows
        }
        uint32_t isrst = 0, drop = 0, tpos = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 1; k <= 16; ++k) {
            const uint32_t i = p0 + (uint32_t)k - 1u;
            const uint8_t c = b[k], pv = b[k - 1], nx = b[k + 1];
            const bool r = c == 0xFF && (nx & 0xF8) == 0xD0;
            if (i < n && c == 0xFF && nx != 0 && !r && tpos == 0xFFFFFFFFu) tpos = i;
            if (r) isrst |= 1u << k;
            if (r || (pv == 0xFF && (c == 0 || (c & 0xF8) == 0xD0))) drop |= 1u << k;
        }
        if (tpos != 0xFFFFFFFFu) atomicMin(&s_term, tpos);
        __syncthreads();
        const uint32_t term = s_term, lim = min(n, term);
        uint32_t nk = 0, nr = 0;
#pragma unroll
        for (int k = 1; k <= 16; ++k) {
            const uint32_t i = p0 + (uint32_t)k - 1u;
            if (i < lim) { nk += !((drop >> k) & 1u); nr += (isrst >> k) & 1u; }
        }
        const uint32_t pk = nk | (nr << 16);
        const uint32_t inc = block256_incl_scan_u32(pk, s_scan);
        uint32_t ko = kept + ((inc - pk) & 0xFFFFu), ro = rsts + ((inc - pk) >> 16);
#pragma unroll
        for (int k = 1; k <= 16; ++k) {
            const uint32_t i = p0 + (uint32_t)k - 1u;
            if (i < lim && ((isrst >> k) & 1u)) {
                if (ro + 1u < nint) { istart[ro + 1u] = ko; if ((uint32_t)(b[k + 1] & 7) != (ro & 7u)) bad = true; }
                else bad = true;
                ++ro;
            } else if (i < lim && !((drop >> k) & 1u)) out[ko++] = b[k];
        }
        if (threadIdx.x == 255) s_tot = inc;
        __syncthreads();
        kept += s_tot & 0xFFFFu; rsts += s_tot >> 16;
        if (term != 0xFFFFFFFFu) break;
    }
    if (bad) atomicOr(&s_bad, 1u);
    __syncthreads();
    if (s_bad || rsts + 1u != nint) {
        if (threadIdx.x == 0) B.status[f] = kStHostOnly;
        return;
    }
    if (threadIdx.x == 0) istart[nint] = kept;
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < nint; i0 += 256u) {
        const uint32_t i = i0 + threadIdx.x;
        uint32_t ns = 0;
        if (i < nint) { const uint32_t len = istart[i + 1] - istart[i]; ns = max(1u, (len + kSubBytes - 1u) / kSubBytes); }
        const uint32_t inc = block256_incl_scan_u32(ns, s_scan);
        if (i < nint) isub[i] = carry + inc - ns;
        if (threadIdx.x == 255) s_tot = inc;
        __syncthreads();
        carry += s_tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) isub[nint] = min(carry, d.scap);          // carry <= scap by construction (plan_layout)
}

// ---- entropy decoding -----------------------------------------------------------------------------------------------------
struct Tabs { DecHuff dc[3], ac[3]; };

__device__ __forceinline__ void load_tabs(const DecFrame &d, Tabs &t)
{
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&d.dc[0]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&t);
    for (uint32_t i = threadIdx.x; i < sizeof(Tabs) / 4; i += blockDim.x) dst[i] = src[i];
}

// 32 bits of the interval from bit p on; bits at or past its last byte are zeros (no load there)
__device__ __forceinline__ uint32_t fetch32(const uint8_t *ubuf, uint32_t a0, uint32_t len, uint32_t p)
{
    const uint32_t by = p >> 3;
    if (by >= len) return 0u;
    const uint32_t a = a0 + by;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(ubuf) + (a >> 2);
    const uint64_t x = ((uint64_t)__builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);
    uint32_t v = (uint32_t)((x << ((a & 3u) * 8u + (p & 7u))) >> 32);
    const uint32_t rem = len - by;
    if (rem < 5u) {
        const uint32_t valid = rem * 8u - (p & 7u);              // 1 .. 32
        if (valid < 32u) v &= ~0u << (32u - valid);
    }
    return v;
}

// jpeg::huff_decode on the top bits of v: the code length, the symbol; false for an undecodable code
__device__ __forceinline__ bool huff(const DecHuff &h, uint32_t v, uint32_t &len, uint32_t &sym)
{
    const uint32_t e = h.lookup[v >> 23];
    if (e) { len = e >> 8; sym = e & 255u; return true; }
    const int code = (int)(v >> 16);
    int l = 10;
    for (; l <= 16; ++l) if ((code >> (16 - l)) <= h.maxcode[l]) break;
    if (l > 16) return false;
    const int idx = h.valptr[l] + (code >> (16 - l));
    if (idx < 0 || idx > 255) return false;
    len = (uint32_t)l; sym = h.vals[idx];
    return true;
}

// Decodes symbols from state `st` while the bit position is before `ebit` (WRITE: and, in the last subsequence of an interval,
// on into the zeros behind it) and, WRITE, the block is before `limit`.  Returns the exit state, kInvalid after an undecodable
// symbol; nblk: WRITE: the first block on entry, the block reached on exit; else the blocks completed.
template <bool WRITE>
__device__ uint64_t decode_run(const Tabs &t, const DecFrame &d, const uint8_t *ubuf, uint32_t a0, uint32_t len, uint64_t st,
                               uint32_t ebit, bool last, uint32_t &nblk, uint32_t limit, int16_t *coef)
{
    constexpr uint8_t ZZ[64] = UWIP_JPEG_ZIGZAG_INIT;
    uint32_t p = (uint32_t)(st >> 32), b = ((uint32_t)st >> 8) & 0xFFu, k = (uint32_t)st & 0xFFu;
    const uint32_t bpm = (uint32_t)d.bpm, lenbits = len * 8u;
    // the blocks of an MCU at which components 1 and 2 start (one component: never), in registers for the symbol loop
    const uint32_t c1 = d.ncomp == 3 ? (uint32_t)d.coff[1] : 0xFFu, c2 = d.ncomp == 3 ? (uint32_t)d.coff[2] : 0xFFu;
    if (b >= bpm || k > 63u) return kInvalid;
    uint32_t blk = WRITE ? nblk : 0u;
    while ((p < ebit || (WRITE && last)) && (!WRITE || blk < limit)) {
        const int c = b >= c1 ? (b >= c2 ? 2 : 1) : 0;
        const uint32_t v = fetch32(ubuf, a0, len, p);
        uint32_t l, s;
        bool done = false;
        if (k == 0u) {
            if (!huff(t.dc[c], v, l, s) || s > 11u) return kInvalid;
            if (WRITE) coef[(size_t)blk * 64] = (int16_t)(s ? extend((int)((v << l) >> (32u - s)), (int)s) : 0);
            p += l + s;
            k = 1u;
        } else {
            if (!huff(t.ac[c], v, l, s)) return kInvalid;
            const uint32_t r = s >> 4, sz = s & 15u;
            p += l + sz;
            if (sz == 0u) {
                if (r == 15u) { k += 16u; done = k > 63u; }
                else done = true;
            } else {
                k += r;
                if (k > 63u) return kInvalid;
                if (WRITE) coef[(size_t)blk * 64 + ZZ[k]] = (int16_t)extend((int)((v << l) >> (32u - sz)), (int)sz);
                ++k;
                done = k > 63u;
            }
        }
        if (done) { k = 0u; b = b + 1u == bpm ? 0u : b + 1u; ++blk; }
        if (WRITE && p > lenbits) p = lenbits;              // behind the end everything reads as zeros: keep p from wrapping
    }
    nblk = blk;
    return pack_state(p, b, k);
}

struct Lane { uint32_t i, j, nsub, a0, len; };      // interval, subsequence within it, its subsequences, its bytes

__device__ __forceinline__ void lane_interval(const DecBufs &B, const DecFrame &d, uint32_t i, Lane &L)
{
    const uint32_t *istart = B.istart + d.ibase, *isub = B.isub + d.ibase;
    L.i = i;
    L.nsub = isub[i + 1] - isub[i];
    L.a0 = d.ubase + istart[i];
    L.len = istart[i + 1] - istart[i];
}

__global__ __launch_bounds__(256) void k_jpd_round(DecBufs B, int round)
{
    __shared__ Tabs s_t;
    const int f = blockIdx.y;
    if (B.status[f] != 0) return;
    const DecFrame &d = B.fr[f];
    load_tabs(d, s_t);
    __syncthreads();
    const uint32_t *isub = B.isub + d.ibase;
    const uint32_t nint = (uint32_t)d.nint, s = blockIdx.x * 256u + threadIdx.x;
    if (s >= isub[nint]) return;
    const size_t gs = (size_t)d.sbase + s;
    const uint64_t *ein = (round & 1) ? B.exit0 : B.exit1;
    uint64_t *eout = (round & 1) ? B.exit1 : B.exit0;
    uint32_t i;
    if (round == 0) {
        uint32_t lo = 0, hi = nint;                      // the last interval that starts at or before lane s
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (isub[mid] <= s) lo = mid; else hi = mid; }
        i = lo;
        B.sint[gs] = i;
    } else i = min(B.sint[gs], nint - 1u);
    Lane L;
    lane_interval(B, d, i, L);
    L.j = s - isub[i];
    uint64_t st;
    if (round == 0) st = pack_state(L.j * kSubBits, 0u, 0u);
    else {
        if (L.j == 0u) { eout[gs] = ein[gs]; return; }
        st = ein[gs - 1];
        if (st == B.entry[gs] || st == kInvalid) { eout[gs] = ein[gs]; return; }
    }
    const uint32_t ebit = L.j + 1u == L.nsub ? L.len * 8u : min((L.j + 1u) * kSubBits, L.len * 8u);
    uint32_t nb = 0;
    const uint64_t ex = decode_run<false>(s_t, d, B.ubuf, L.a0, L.len, st, ebit, false, nb, 0u, nullptr);
    B.entry[gs] = st;
    eout[gs] = ex;
    B.cnt[gs] = ex == kInvalid ? 0u : nb;
}

__global__ __launch_bounds__(256) void k_jpd_check(DecBufs B, int rounds)
{
    __shared__ uint32_t s_n[2];             // this workgroup's unsettled lanes, lanes: one global atomic each
    const int f = blockIdx.y;
    if (B.status[f] != 0) return;
    if (threadIdx.x < 2) s_n[threadIdx.x] = 0u;
    __syncthreads();
    const DecFrame &d = B.fr[f];
    const uint32_t *isub = B.isub + d.ibase;
    const uint32_t nint = (uint32_t)d.nint, s = blockIdx.x * 256u + threadIdx.x;
    if (s < isub[nint]) {
        const size_t gs = (size_t)d.sbase + s;
        const uint32_t i = min(B.sint[gs], nint - 1u), j = s - isub[i];
        const uint64_t *ex = (rounds & 1) ? B.exit1 : B.exit0;
        atomicAdd(&s_n[1], 1u);
        if (j != 0u && ex[gs - 1] != B.entry[gs]) {
            atomicMin(&B.ifirst[d.ibase + i], j);
            atomicAdd(&s_n[0], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_n[threadIdx.x]) atomicAdd(&B.stats[threadIdx.x], (unsigned long long)s_n[threadIdx.x]);
}

__global__ __launch_bounds__(64) void k_jpd_cleanup(DecBufs B, int rounds)
{
    __shared__ Tabs s_t;
    const int f = blockIdx.y;
    if (B.status[f] != 0) return;
    const DecFrame &d = B.fr[f];
    load_tabs(d, s_t);
    __syncthreads();
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= (uint32_t)d.nint) return;
    const uint32_t first = B.ifirst[d.ibase + i];
    Lane L;
    lane_interval(B, d, i, L);
    if (first == 0u || first >= L.nsub) return;
    uint64_t *ex = (rounds & 1) ? B.exit1 : B.exit0;
    const size_t g0 = (size_t)d.sbase + B.isub[d.ibase + i];
    for (uint32_t j = first; j < L.nsub; ++j) {
        const uint64_t st = ex[g0 + j - 1];
        if (st == kInvalid) {                                        // the lane before stops the decode: nothing follows it
            for (; j < L.nsub; ++j) { ex[g0 + j] = kInvalid; B.cnt[g0 + j] = 0u; }
            break;
        }
        if (st == B.entry[g0 + j]) continue;
        const uint32_t ebit = j + 1u == L.nsub ? L.len * 8u : min((j + 1u) * kSubBits, L.len * 8u);
        uint32_t nb = 0;
        const uint64_t e = decode_run<false>(s_t, d, B.ubuf, L.a0, L.len, st, ebit, false, nb, 0u, nullptr);
        B.entry[g0 + j] = st;
        ex[g0 + j] = e;
        B.cnt[g0 + j] = e == kInvalid ? 0u : nb;
    }
}

// inclusive segmented scan over the 256 threads of a workgroup (head: the element starts a segment); `carry` is the running
// value of the segment open at the end of the previous call, updated for the next
__device__ int64_t block256_seg_scan(int64_t v, bool head, int64_t &carry, int64_t *s_v, uint32_t *s_h)
{
    const uint32_t t = threadIdx.x;
    uint32_t h = head ? 1u : 0u;
    for (uint32_t off = 1; off < 256u; off <<= 1) {
        s_v[t] = v; s_h[t] = h;
        __syncthreads();
        if (t >= off && !h) { v += s_v[t - off]; h = s_h[t - off]; }
        __syncthreads();
    }
    if (!h) v += carry;
    s_v[t] = v;
    __syncthreads();
    carry = s_v[255];
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(256) void k_jpd_blkscan(DecBufs B)
{
    __shared__ int64_t s_v[256];
    __shared__ uint32_t s_h[256];
    const int f = blockIdx.x;
    if (B.status[f] != 0) return;
    const DecFrame &d = B.fr[f];
    const uint32_t *isub = B.isub + d.ibase;
    const uint32_t nint = (uint32_t)d.nint, ns = isub[nint];
    int64_t carry = 0;
    for (uint32_t s0 = 0; s0 < ns; s0 += 256u) {
        const uint32_t s = s0 + threadIdx.x;
        uint32_t c = 0;
        bool head = false;
        if (s < ns) {
            const size_t gs = (size_t)d.sbase + s;
            c = B.cnt[gs];
            head = s == isub[min(B.sint[gs], nint - 1u)];
        }
        const int64_t inc = block256_seg_scan((int64_t)c, head, carry, s_v, s_h);
        if (s < ns) B.sblk[(size_t)d.sbase + s] = (uint32_t)min(inc - (int64_t)c, (int64_t)0x7FFFFFFF);
    }
}

__global__ __launch_bounds__(256) void k_jpd_write(DecBufs B, int rounds)
{
    __shared__ Tabs s_t;
    const int f = blockIdx.y;
    if (B.status[f] != 0) return;
    const DecFrame &d = B.fr[f];
    load_tabs(d, s_t);
    __syncthreads();
    const uint32_t *isub = B.isub + d.ibase;
    const uint32_t nint = (uint32_t)d.nint, s = blockIdx.x * 256u + threadIdx.x;
    if (s >= isub[nint]) return;
    const size_t gs = (size_t)d.sbase + s;
    const uint32_t i = min(B.sint[gs], nint - 1u);
    Lane L;
    lane_interval(B, d, i, L);
    L.j = s - isub[i];
    const uint64_t *ex = (rounds & 1) ? B.exit1 : B.exit0;
    const uint64_t st = L.j == 0u ? pack_state(0u, 0u, 0u) : ex[gs - 1];
    if (st == kInvalid) return;
    const uint32_t mcus = min((uint32_t)d.ri, (uint32_t)d.nmcu - i * (uint32_t)d.ri), limit = mcus * (uint32_t)d.bpm;
    uint32_t blk = B.sblk[gs];
    if (blk >= limit) return;
    const bool last = L.j + 1u == L.nsub;
    const uint32_t ebit = last ? L.len * 8u : min((L.j + 1u) * kSubBits, L.len * 8u);
    int16_t *coef = B.coef + ((size_t)d.bbase + (size_t)i * d.ri * d.bpm) * 64;
    const uint64_t e = decode_run<true>(s_t, d, B.ubuf, L.a0, L.len, st, ebit, last, blk, limit, coef);
    if (e == kInvalid) B.err[f] = 1;
}

// ---- DC prediction --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_jpd_dc(DecBufs B)
{
    __shared__ int64_t s_v[256];
    __shared__ uint32_t s_h[256];
    const int c = blockIdx.x, f = blockIdx.y;
    if (B.status[f] != 0) return;
    const DecFrame &d = B.fr[f];
    if (c >= d.ncomp) return;
    const uint32_t hv = (uint32_t)(d.ch[c] * d.cv[c]), n = (uint32_t)d.nmcu * hv, bpm = (uint32_t)d.bpm, ri = (uint32_t)d.ri;
    int16_t *coef = B.coef + (size_t)d.bbase * 64;
    int64_t carry = 0;
    bool bad = false;
    for (uint32_t n0 = 0; n0 < n; n0 += 256u) {
        const uint32_t q = n0 + threadIdx.x;
        int64_t v = 0;
        bool head = false;
        size_t g = 0;
        if (q < n) {
            const uint32_t mcu = q / hv, jj = q - mcu * hv;
            g = ((size_t)mcu * bpm + (uint32_t)d.coff[c] + jj) * 64;
            v = coef[g];
            head = jj == 0u && mcu % ri == 0u;
        }
        const int64_t pred = block256_seg_scan(v, head, carry, s_v, s_h);
        if (q < n) {
            if (pred > 32767 || pred < -32768) bad = true;
            coef[g] = (int16_t)pred;
        }
    }
    if (bad) B.err[f] = 1;
}

// ---- inverse DCT ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_jpd_idct(DecBufs B)
{
    const int f = blockIdx.y;
    if (B.status[f] != 0 || B.err[f] != 0) return;
    const DecFrame &d = B.fr[f];
    const uint32_t g = blockIdx.x * 64u + threadIdx.x, bpm = (uint32_t)d.bpm;
    if (g >= (uint32_t)d.nmcu * bpm) return;
    const uint32_t mcu = g / bpm, b = g - mcu * bpm;
    const int c = (d.ncomp == 3 && b >= (uint32_t)d.coff[1]) ? (b >= (uint32_t)d.coff[2] ? 2 : 1) : 0;
    const uint32_t jj = b - (uint32_t)d.coff[c], bx = jj % (uint32_t)d.ch[c], by = jj / (uint32_t)d.ch[c];
    const uint32_t mx = mcu % (uint32_t)d.mcux, my = mcu / (uint32_t)d.mcux;
    const size_t stride = (size_t)d.cwb[c] * 8;
    uint8_t *dst = B.planes + d.pbase[c] + (size_t)((my * d.cv[c] + by) * 8u) * stride + (size_t)(mx * d.ch[c] + bx) * 8u;
    const int16_t *src = B.coef + ((size_t)d.bbase + g) * 64;
    const uint16_t *qt = d.qt[c];
    int64_t ws[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) ws[i] = clamp_coef((int64_t)src[i] * (int64_t)qt[i]);
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int64_t in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = ws[r * 8 + col];
        idct_pass(in, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r * 8 + col] = descale64(o[r], 13 - 2);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int64_t in[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) in[i] = ws[r * 8 + i];
        idct_pass(in, o);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t sv = descale64(o[i], 13 + 2 + 3) + 128;
            const uint32_t u = (uint32_t)(sv < 0 ? 0 : (sv > 255 ? 255 : sv));
            if (i < 4) lo |= u << (8 * i); else hi |= u << (8 * (i - 4));
        }
        uint32_t *row = reinterpret_cast<uint32_t *>(dst + (size_t)r * stride);          // 8-byte aligned: plane bases are
        row[0] = lo; row[1] = hi;
    }
}

// ---- upsampling and colour --------------------------------------------------------------------------------------------------
// the full-resolution sample (x, y) of component c: jpeg::decode's `full`
__device__ __forceinline__ int full_sample(const DecFrame &d, const uint8_t *planes, int c, int x, int y)
{
    const uint8_t *pl = planes + d.pbase[c];
    const int stride = d.cwb[c] * 8, dw = d.cdw[c], dh = d.cdh[c];
    auto samp = [&](int sx, int sy) -> int {
        sx = sx < 0 ? 0 : (sx >= dw ? dw - 1 : sx);
        sy = sy < 0 ? 0 : (sy >= dh ? dh - 1 : sy);
        return pl[(size_t)sy * stride + sx];
    };
    const int hx = d.hmax / d.ch[c], vx = d.vmax / d.cv[c];
    if (hx == 1) return samp(x, y);                          // vx == 2 is host only
    const int xs = x >> 1;
    if (vx == 1) {                                           // h2v1_fancy_upsample
        const int s0 = samp(xs, y);
        if (x & 1) return xs == dw - 1 ? s0 : (s0 * 3 + samp(xs + 1, y) + 2) >> 2;
        return xs == 0 ? s0 : (s0 * 3 + samp(xs - 1, y) + 1) >> 2;
    }
    const int y0 = y >> 1, y1 = (y & 1) ? y0 + 1 : y0 - 1;  // h2v2_fancy_upsample
    const int thisc = samp(xs, y0) * 3 + samp(xs, y1);
    if (x & 1) {
        if (xs == dw - 1) return (thisc * 4 + 7) >> 4;
        return (thisc * 3 + samp(xs + 1, y0) * 3 + samp(xs + 1, y1) + 7) >> 4;
    }
    if (xs == 0) return (thisc * 4 + 8) >> 4;
    return (thisc * 3 + samp(xs - 1, y0) * 3 + samp(xs - 1, y1) + 8) >> 4;
}

__global__ __launch_bounds__(256) void k_jpd_color(DecBufs B, uint8_t *out, size_t step, size_t fs, int rows, int cols, int channels)
{
    const int f = blockIdx.y;
    if (B.status[f] != 0) return;
    if (B.err[f] != 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) B.status[f] = kStBad;
        return;
    }
    const DecFrame &d = B.fr[f];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (d.W != cols || d.H != rows || q >= (uint32_t)rows * (uint32_t)cols) return;
    const int y = (int)(q / (uint32_t)cols), x = (int)(q - (uint32_t)y * (uint32_t)cols);
    uint8_t *p = out + (size_t)f * fs + (size_t)y * step + (size_t)x * channels;
    const int Y = full_sample(d, B.planes, 0, x, y);
    if (channels == 1) { p[0] = (uint8_t)Y; return; }
    if (d.ncomp == 1) { p[0] = p[1] = p[2] = (uint8_t)Y; return; }
    const int cb = full_sample(d, B.planes, 1, x, y) - 128, cr = full_sample(d, B.planes, 2, x, y) - 128;
    auto clamp8 = [](int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
    p[2] = clamp8(Y + ((91881 * cr + 32768) >> 16));                                     // jdcolor, SCALEBITS 16
    p[1] = clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    p[0] = clamp8(Y + ((116130 * cb + 32768) >> 16));
}

// ---- the host side ----------------------------------------------------------------------------------------------------------
struct DecPlan {
    size_t src_bytes = 0, ubuf_bytes = 0, nintv = 0, nsub = 0, nblk = 0, plane_bytes = 0;
    uint32_t max_sub = 0, max_int = 0, max_blk = 0;
    bool too_large = false;
};

// where every frame's pieces lie in the shared buffers; seg_len is set by the caller.  A frame the host already gave a status
// takes no room.
void plan_layout(DecFrame *fr, int F, DecPlan &pl)
{
    for (int f = 0; f < F; ++f) {
        DecFrame &d = fr[f];
        if (d.status != 0) continue;
        d.seg_off = (uint32_t)pl.src_bytes; pl.src_bytes += ((size_t)d.seg_len + 31) & ~(size_t)15;
        d.ubase = (uint32_t)pl.ubuf_bytes; pl.ubuf_bytes += ((size_t)d.seg_len + 31) & ~(size_t)15;
        d.ibase = (uint32_t)pl.nintv; pl.nintv += (size_t)d.nint + 1;
        d.scap = d.seg_len / kSubBytes + (uint32_t)d.nint + 1u;
        d.sbase = (uint32_t)pl.nsub; pl.nsub += d.scap;
        const size_t nb = (size_t)d.nmcu * d.bpm;
        d.bbase = (uint32_t)pl.nblk; pl.nblk += nb;
        for (int c = 0; c < d.ncomp; ++c) { d.pbase[c] = (uint32_t)pl.plane_bytes; pl.plane_bytes += (size_t)d.cwb[c] * d.chb[c] * 64; }
        if (d.scap > pl.max_sub) pl.max_sub = d.scap;
        if ((uint32_t)d.nint > pl.max_int) pl.max_int = (uint32_t)d.nint;
        if (nb > pl.max_blk) pl.max_blk = (uint32_t)nb;
        if (pl.src_bytes >= (1u << 31) || pl.nblk >= (1u << 30) || pl.plane_bytes >= (1ull << 32) || pl.nsub >= (1u << 31)) pl.too_large = true;
    }
}

int rounds_of(int sync_rounds) { return sync_rounds < 0 ? kDefaultRounds : (sync_rounds > 64 ? 64 : sync_rounds); }

// uwip_jpeg_decode behind the upload, on either back end (uwip_device; the host threads of tests/hip_on_host.hpp): the working
// arrays, their first values and every launch.  fr / src: the planned descriptors and the segments, where the kernels read them.
template <class BE>
void decode_sequence(BE &be, const DecFrame *fr, const uint8_t *src, const DecPlan &pl, int n, int rounds, const uwip_batch_u8 &out,
                     int32_t *d_status, void *d_unsettled)
{
    using dim3 = typename BE::dim3;                           // HIP's on the device, its stand-in on host threads
    const size_t ni = pl.nintv + 1, ns = pl.nsub + 1, ncoef = (pl.nblk + 1) * 64;
    DecBufs B;
    B.fr = fr; B.src = src; B.status = d_status;
    B.ubuf = be.template array<uint8_t>("jpegdec.unstuffed", pl.ubuf_bytes + 16);
    B.istart = be.template array<uint32_t>("jpegdec.istart", ni);
    B.isub = be.template array<uint32_t>("jpegdec.isub", ni);
    B.ifirst = be.template array<uint32_t>("jpegdec.ifirst", ni);
    B.exit0 = be.template array<uint64_t>("jpegdec.exit0", ns);
    B.exit1 = be.template array<uint64_t>("jpegdec.exit1", ns);
    B.entry = be.template array<uint64_t>("jpegdec.entry", ns);
    B.cnt = be.template array<uint32_t>("jpegdec.cnt", ns);
    B.sblk = be.template array<uint32_t>("jpegdec.sblk", ns);
    B.sint = be.template array<uint32_t>("jpegdec.sint", ns);
    B.coef = be.template array<int16_t>("jpegdec.coef", ncoef);
    B.planes = be.template array<uint8_t>("jpegdec.planes", pl.plane_bytes + 16);
    B.err = be.template array<int32_t>("jpegdec.err", (size_t)n);
    B.stats = be.template array<unsigned long long>("jpegdec.stats", 2);
    be.fill(B.err, 0, (size_t)n * sizeof(int32_t));
    be.fill(B.stats, 0, 2 * sizeof(unsigned long long));
    be.fill(B.ifirst, 0xFF, ni * sizeof(uint32_t));
    be.fill(B.coef, 0, ncoef * sizeof(int16_t));

    const unsigned gsub = uwip_cdiv(pl.max_sub ? pl.max_sub : 1, 256), gint = uwip_cdiv(pl.max_int ? pl.max_int : 1, 64);
    const unsigned gblk = uwip_cdiv(pl.max_blk ? pl.max_blk : 1, 64), gpix = uwip_cdiv((size_t)out.rows * out.cols, 256);
    be.launch("k_jpd_unstuff", k_jpd_unstuff, dim3(n), 256, B);
    for (int r = 0; r <= rounds; ++r) be.launch(r ? "k_jpd_round_sync" : "k_jpd_round", k_jpd_round, dim3(gsub, n), 256, B, r);
    be.launch("k_jpd_check", k_jpd_check, dim3(gsub, n), 256, B, rounds);
    be.launch("k_jpd_cleanup", k_jpd_cleanup, dim3(gint, n), 64, B, rounds);
    be.launch("k_jpd_blkscan", k_jpd_blkscan, dim3(n), 256, B);
    be.launch("k_jpd_write", k_jpd_write, dim3(gsub, n), 256, B, rounds);
    be.launch("k_jpd_dc", k_jpd_dc, dim3(3, n), 256, B);
    be.launch("k_jpd_idct", k_jpd_idct, dim3(gblk, n), 64, B);
    be.launch("k_jpd_color", k_jpd_color, dim3(gpix, n), 256, B, static_cast<uint8_t *>(out.data), out.step, out.frame_stride, out.rows,
              out.cols, out.channels);
    if (d_unsettled) be.copy(d_unsettled, B.stats, 2 * sizeof(unsigned long long));
}

}  // namespace

UWIP_API int uwip_jpeg_info(const uint8_t *buf, size_t len, int32_t *rows, int32_t *cols, int32_t *channels)
{
    if (!buf || !rows || !cols || !channels) return UWIP_ERR_INVALID;
    int r = 0, c = 0, ch = 0;
    if (uwip_jpeg::parse(buf, len, &r, &c, &ch, nullptr, nullptr) == uwip_jpeg::PARSE_BAD) return UWIP_ERR_UNSUPPORTED;
    *rows = r; *cols = c; *channels = ch;
    return UWIP_OK;
}

UWIP_API int uwip_jpeg_decode(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                              const uwip_jpeg_decode_opts *opts, int32_t *d_status)
{
    int rc = uwip_check_batch(ctx, out, 0);
    if (rc) return rc;
    rc = uwip_check_streams(ctx, h_streams, h_sizes, n, out, d_status);
    if (rc || n == 0) return rc;
    const int rounds = rounds_of(opts ? opts->sync_rounds : -1);

    // The page-locked staging buffer holds the descriptors, then the segments.  It is free again once the previous call's
    // upload has finished: poll that event (the stream is not drained) before the buffer is touched -- or grown, which frees it.
    static_assert(sizeof(DecFrame) % 16 == 0, "the segments follow the descriptors at a 16-byte boundary");
    static_assert(sizeof(DecFrame) == 9056, "the kernels and the host decoder read one layout");
    if (!ctx->jpd_ev) UWIP_HIP(ctx, hipEventCreateWithFlags(&ctx->jpd_ev, hipEventDisableTiming));
    else UWIP_HIP(ctx, uwip_event_wait(ctx->jpd_ev, 200));
    const size_t hdr = (size_t)n * sizeof(DecFrame);
    size_t in_bytes = hdr + 16;                     // a segment is at most its stream
    for (int f = 0; f < n; ++f) in_bytes += (h_sizes[f] + 31) & ~(size_t)15;
    uint8_t *h_in = static_cast<uint8_t *>(uwip_host_ws(ctx, "jpegdec.in", in_bytes));
    if (!h_in) return UWIP_ERR_NOMEM;
    DecFrame *fr = reinterpret_cast<DecFrame *>(h_in);          // parsed straight into staging
    std::vector<size_t> seg((size_t)n, 0);
    for (int f = 0; f < n; ++f) {
        DecFrame &d = fr[f];
        std::memset(&d, 0, sizeof d);
        int r = 0, c = 0, ch = 0;
        d.status = uwip_jpeg::parse(h_streams[f], h_sizes[f], &r, &c, &ch, &d, &seg[f]);
        if (d.status == 0 && (r != out->rows || c != out->cols || (ch == 3 && out->channels == 1))) d.status = UWIP_JPEG_SIZE_MISMATCH;
        if (d.status == 0) d.seg_len = (uint32_t)(h_sizes[f] - seg[f]);
    }
    DecPlan pl;
    plan_layout(fr, n, pl);
    UWIP_REQUIRE(ctx, !pl.too_large, "batch too large for one call");

    uint8_t *d_in = static_cast<uint8_t *>(uwip_ws(ctx, "jpegdec.in", in_bytes));
    if (!d_in) return UWIP_ERR_NOMEM;
    for (int f = 0; f < n; ++f)
        if (fr[f].status == 0 && fr[f].seg_len) std::memcpy(h_in + hdr + fr[f].seg_off, h_streams[f] + seg[f], fr[f].seg_len);
    UWIP_HIP(ctx, hipMemcpyAsync(d_in, h_in, hdr + pl.src_bytes, hipMemcpyHostToDevice, ctx->stream));
    UWIP_HIP(ctx, hipEventRecord(ctx->jpd_ev, ctx->stream));

    uwip_device dev(ctx);
    decode_sequence(dev, reinterpret_cast<const DecFrame *>(d_in), d_in + hdr, pl, n, rounds, *out, d_status, opts ? opts->d_unsettled : nullptr);
    return dev.finish();
}

UWIP_API int uwip_jpeg_decode_host(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                                   const uwip_jpeg_decode_opts *opts, int32_t *h_status)
{
    return uwip_decode_to_host(ctx, h_streams, h_sizes, n, out, opts, h_status, uwip_jpeg_decode, "jpegdec.status");
}
