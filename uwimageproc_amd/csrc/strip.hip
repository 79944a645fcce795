// Strip mosaic (include/uwip.h, "strip mosaic"): the key frames of main.cpp:368-381, chained by the
// homographies of videostrip.cpp:270 and rendered into one canvas per segment.
//   k_strip_chain    one lane runs strip_core.hpp's chain() over the appended H / ratio arrays;
//   k_strip_render   canvas-centric gather: a workgroup owns a 64 x 16 tile, collects the frames whose box meets it (in
//                    chunks of kCullChunk, compacted in LDS together with their inverse transforms), every thread keeps
//                    integer accumulators for its four pixels, the tile is assembled in LDS and written row by row;
//   k_strip_store    the injected form's copy of frames into the store;
//   k_strip_gain_stats  gain compensation, the measurement: a workgroup owns a 64 x 16 tile of frame k, samples frame k - 1 at the
//                    same plane points, keeps the count and the six sums of the valid pixels in registers, reduces them in
//                    LDS and adds them to stats[k] with one 64-bit atomic per quantity;
//   k_strip_gain_solve  one lane runs strip_core.hpp's gain_solve() over the statistics;
//   k_strip_stack    multi-band blending, the frames' stacks: one level of every frame per launch, the tile and its halo in LDS;
//   k_strip_render_bands  the gather of k_strip_render, one pixel per thread, blending the stacks' bands (UWIP_STRIP_MULTIBAND).
// Everything inside the anonymous namespace is also compiled by the host compiler and run on host threads by
// tests/strip_emulated.cpp (no HIP-only intrinsics in there).
#include "uwip_internal.hpp"
#include "strip_core.hpp"
#include <algorithm>
#include <cstring>

namespace {
constexpr int kTileW = 64, kTileH = 16, kRenderThreads = 256;
constexpr int kPix = kTileW * kTileH / kRenderThreads;      // pixels per thread: rows ly, ly + 4, ly + 8, ly + 12 of one column
constexpr int kCullChunk = 256;                              // frames tested (and at most listed) per pass of the cull list
constexpr int kTileRowBytes = kTileW * 3;

struct StripRender {
    const uint8_t *store;                 // [frames][h][w][3]
    size_t fstride;
    int32_t w, h;
    const double *Ginv;                   // [frames][9]
    const int32_t *box;                   // [frames][4]
    int32_t first, count;                 // the segment's frames
    int32_t x0, y0, rows, cols;           // the segment's canvas
    uint8_t *canvas;
    size_t step;
    uint8_t *cover;                       // [rows][cols] or null
    uint8_t fill[4];
    int32_t vec;                          // bytes per store of the write-out: 16, 4 or 1
    const int32_t *gq = nullptr;          // [frames][3] gains in 1/4096 for k_strip_render<MODE, true>; null = none
};

struct StripGainStats {
    const uint8_t *store;                 // [frames][h][w][3]
    size_t fstride;
    int32_t w, h;
    const double *G, *Ginv;               // [frames][9]
    const int32_t *seg;                   // [frames]
    uwip_sm::GainParams P;
    unsigned long long *stats;            // [frames][7], cleared before the launch
    int32_t tiles_x;                      // tiles per row of tiles: blockIdx.x = tile, blockIdx.y = frame
};

__global__ __launch_bounds__(64) void k_strip_chain(uwip_sm::ChainParams P, const double *H, const float *ratio, int32_t n,
                                                    uwip_sm::ChainOut o, double *fb)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uwip_sm::chain(P, H, ratio, n, o, fb);
}

__global__ __launch_bounds__(256) void k_strip_store(const uint8_t *src, size_t step, size_t fs, int32_t rows, int32_t rowbytes,
                                                     uint8_t *dst)
{
    const int32_t x = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x), y = (int32_t)blockIdx.y;
    const size_t f = blockIdx.z;
    if (x < rowbytes && y < rows) dst[(f * rows + y) * (size_t)rowbytes + x] = src[f * fs + (size_t)y * step + x];
}

// Frame k = blockIdx.y against frame k - 1.  A thread's four pixels give at most 4 x 255 x 1024, a workgroup's 1024 pixels at
// most 2^28.0: 32-bit sums up to the workgroup, 64-bit ones beyond it.
__global__ __launch_bounds__(kRenderThreads) void k_strip_gain_stats(StripGainStats a)
{
    __shared__ uint32_t s_sum[uwip_sm::kGainStats][kRenderThreads];
    const int32_t k = (int32_t)blockIdx.y;
    if (k == 0 || a.seg[k] != a.seg[k - 1]) return;        // the first frame of a segment has no partner (uniform: no barrier yet)
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t tx0 = ((int32_t)blockIdx.x % a.tiles_x) * kTileW, ty0 = ((int32_t)blockIdx.x / a.tiles_x) * kTileH;
    const int32_t x = tx0 + (tid & (kTileW - 1)), ly = tid / kTileW;
    const uint8_t *fk = a.store + (size_t)k * a.fstride, *fp = a.store + (size_t)(k - 1) * a.fstride;
    double G[9], Ap[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { G[i] = a.G[9 * (size_t)k + i]; Ap[i] = a.Ginv[9 * (size_t)(k - 1) + i]; }
    uint32_t sum[uwip_sm::kGainStats];
#pragma unroll
    for (int q = 0; q < uwip_sm::kGainStats; ++q) sum[q] = 0;
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int32_t y = ty0 + ly + j * (kRenderThreads / kTileW);
        int32_t Pa[3], Pb[3];
        if (x >= a.w || y >= a.h || !uwip_sm::gain_pixel(a.P, fk, fp, G, Ap, x, y, a.w, a.h, Pa, Pb)) continue;
        sum[0] += 1u;
#pragma unroll
        for (int c = 0; c < 3; ++c) { sum[1 + c] += (uint32_t)Pa[c]; sum[4 + c] += (uint32_t)Pb[c]; }
    }
#pragma unroll
    for (int q = 0; q < uwip_sm::kGainStats; ++q) s_sum[q][tid] = sum[q];
    __syncthreads();
    for (int32_t s = kRenderThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < uwip_sm::kGainStats; ++q) s_sum[q][tid] += s_sum[q][tid + s];
        }
        __syncthreads();
    }
    if (tid < uwip_sm::kGainStats && s_sum[tid][0]) atomicAdd(a.stats + uwip_sm::kGainStats * (size_t)k + tid, (unsigned long long)s_sum[tid][0]);
}

__global__ __launch_bounds__(64) void k_strip_gain_solve(uwip_sm::GainParams P, const unsigned long long *stats, const int32_t *seg, int32_t n,
                                                         int32_t *gq, double *g, double *scr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uwip_sm::gain_solve(P, reinterpret_cast<const uint64_t *>(stats), seg, n, gq, g, scr);
}

// GAIN: every sample is multiplied by its frame's gain (a.gq) before it is blended; false is the kernel without gains
template <int MODE, bool GAIN = false>
__global__ __launch_bounds__(kRenderThreads) void k_strip_render(StripRender a)
{
    __shared__ double s_A[kCullChunk][9];
    __shared__ int32_t s_idx[kCullChunk];
    __shared__ int32_t s_gq[GAIN ? kCullChunk : 1][3];
    __shared__ uint32_t s_n;
    __shared__ uint32_t s_tile[kTileH * kTileRowBytes / 4];
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t tx0 = (int32_t)blockIdx.x * kTileW, ty0 = (int32_t)blockIdx.y * kTileH;
    const int32_t tx1 = min(tx0 + kTileW, a.cols) - 1, ty1 = min(ty0 + kTileH, a.rows) - 1;
    const int32_t lx = tid & (kTileW - 1), ly = tid / kTileW;
    const int32_t X = tx0 + lx;
    const double px = (double)(X + a.x0);

    // FEATHER: num / den; FIRST / LAST: the winner's index in den and its P in num
    int64_t num[kPix][3], den[kPix];
    uint32_t cnt[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) { num[j][0] = num[j][1] = num[j][2] = 0; den[j] = MODE == UWIP_STRIP_FEATHER ? 0 : -1; cnt[j] = 0; }

    for (int32_t base = 0; base < a.count; base += kCullChunk) {
        __syncthreads();                                   // the previous chunk's list has been read by everyone
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (int32_t k = base + tid; k < min(base + kCullChunk, a.count); k += kRenderThreads) {
            const int32_t g = a.first + k;
            const int32_t *b = a.box + 4 * (size_t)g;
            if (b[0] <= tx1 && b[2] >= tx0 && b[1] <= ty1 && b[3] >= ty0) {
                const uint32_t slot = atomicAdd(&s_n, 1u);
                s_idx[slot] = g;
                for (int i = 0; i < 9; ++i) s_A[slot][i] = a.Ginv[9 * (size_t)g + i];
                if (GAIN) for (int c = 0; c < 3; ++c) s_gq[slot][c] = a.gq[3 * (size_t)g + c];
            }
        }
        __syncthreads();
        const int32_t n = (int32_t)s_n;
        if (X > tx1) continue;                             // a column beyond the canvas: nothing to accumulate (barriers stay uniform)
        for (int32_t e = 0; e < n; ++e) {
            double A[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) A[i] = s_A[e][i];
            const int32_t g = s_idx[e];
            const uint8_t *f = a.store + (size_t)g * a.fstride;
            int32_t gq[3] = {4096, 4096, 4096};
            if (GAIN) for (int c = 0; c < 3; ++c) gq[c] = s_gq[e][c];
#pragma unroll
            for (int j = 0; j < kPix; ++j) {
                const int32_t Y = ty0 + ly + j * (kRenderThreads / kTileW);
                if (Y > ty1) continue;
                uwip_sm::Tap t;
                if (!uwip_sm::sample(A, px, (double)(Y + a.y0), a.w, a.h, t)) continue;
                cnt[j] += 1u;
                if (MODE != UWIP_STRIP_FEATHER) {
                    const bool wins = den[j] < 0 || (MODE == UWIP_STRIP_LAST ? g > den[j] : g < den[j]);
                    if (!wins) continue;
                    den[j] = g;
                }
                const uint8_t *r0 = f + ((size_t)t.y * a.w) * 3, *r1 = f + ((size_t)t.y1 * a.w) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    int32_t P = uwip_sm::bilinear(t, r0[t.x * 3 + c], r0[t.x1 * 3 + c], r1[t.x * 3 + c], r1[t.x1 * 3 + c]);
                    if (GAIN) P = uwip_sm::apply_gain(P, gq[c]);
                    if (MODE == UWIP_STRIP_FEATHER) num[j][c] += (int64_t)t.q * P;
                    else num[j][c] = P;
                }
                if (MODE == UWIP_STRIP_FEATHER) den[j] += t.q;
            }
        }
    }

    // the tile in LDS, then its rows out contiguously
    uint8_t *tile = reinterpret_cast<uint8_t *>(s_tile);
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int32_t r = ly + j * (kRenderThreads / kTileW), Y = ty0 + r;
        if (X > tx1 || Y > ty1) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t v = a.fill[c];
            if (MODE == UWIP_STRIP_FEATHER) {
                if (den[j] > 0) v = (uint8_t)((num[j][c] + 512 * den[j]) / (1024 * den[j]));
            } else if (den[j] >= 0) {
                v = (uint8_t)((num[j][c] + 512) >> 10);
            }
            tile[r * kTileRowBytes + lx * 3 + c] = v;
        }
        if (a.cover) a.cover[(size_t)Y * a.cols + X] = (uint8_t)(cnt[j] > 255u ? 255u : cnt[j]);
    }
    __syncthreads();
    const int32_t th = ty1 - ty0 + 1, nb = (tx1 - tx0 + 1) * 3;       // rows of this tile, bytes of each
    uint8_t *out = a.canvas + (size_t)ty0 * a.step + (size_t)tx0 * 3;
    if (a.vec == 16) {
        constexpr int U = kTileRowBytes / 16;
        for (int32_t i = tid; i < kTileH * U; i += kRenderThreads) {
            const int32_t r = i / U, at = (i % U) * 16;
            if (r >= th || at >= nb) continue;
            uint8_t *p = out + (size_t)r * a.step + at;
            const uint32_t *s = s_tile + (r * kTileRowBytes + at) / 4;
            if (at + 16 <= nb) *reinterpret_cast<uint4 *>(p) = make_uint4(s[0], s[1], s[2], s[3]);
            else for (int32_t q = at; q < nb; ++q) out[(size_t)r * a.step + q] = tile[r * kTileRowBytes + q];
        }
    } else if (a.vec == 4) {
        constexpr int U = kTileRowBytes / 4;
        for (int32_t i = tid; i < kTileH * U; i += kRenderThreads) {
            const int32_t r = i / U, at = (i % U) * 4;
            if (r >= th || at >= nb) continue;
            uint8_t *p = out + (size_t)r * a.step + at;
            if (at + 4 <= nb) *reinterpret_cast<uint32_t *>(p) = s_tile[(r * kTileRowBytes + at) / 4];
            else for (int32_t q = at; q < nb; ++q) out[(size_t)r * a.step + q] = tile[r * kTileRowBytes + q];
        }
    } else {
        for (int32_t i = tid; i < kTileH * kTileRowBytes; i += kRenderThreads) {
            const int32_t r = i / kTileRowBytes, at = i % kTileRowBytes;
            if (r < th && at < nb) out[(size_t)r * a.step + at] = tile[i];
        }
    }
}

// ---- multi-band blending ------------------------------------------------------------------------------------------------------
struct StripStack {
    const uint8_t *in;                    // [frames][h][w][3]: level l
    uint8_t *out;                         // [frames][h][w][3]: level l + 1
    size_t fstride;
    int32_t w, h, s;                      // s = 2^l: the distance of the taps
    int32_t tiles_x;                      // tiles per row of tiles: blockIdx.x = tile, blockIdx.y = frame
    int32_t vec;                          // 4: both bases, the frame stride and 3 w are multiples of 4 (whole words); 1: bytes
};

struct StripBands {
    StripRender r;                        // as k_strip_render takes it
    const uint8_t *bands;                 // [levels][bcount][h][w][3]: levels 1 .. levels of every frame
    size_t lstride;                       // bcount x fstride
    uwip_sm::BandParams P;
};

constexpr int kStackRows = kTileH + 4 * 8;                          // the tile and a halo of 2 s rows, at s = 8
constexpr int kStackRowWords = (kTileRowBytes + 12 * 8) / 4;       // and of 6 s bytes on either side (s = 1: 2 more, to a word)
constexpr int kBandTileH = kRenderThreads / kTileW;                 // the multiband render's tile: 64 x 4, one pixel per thread

// Level l + 1 of every frame from level l.  A frame's rows are bytes here: the taps of a byte lie 3 s bytes apart, and beyond a
// row's ends each byte takes its own channel of the first / last pixel.  The tile's rows with their halo go into LDS from a
// start that is a multiple of 4 bytes, as whole words wherever a word lies inside the row.
__global__ __launch_bounds__(kRenderThreads) void k_strip_stack(StripStack a)
{
    __shared__ uint32_t s_in[kStackRows * kStackRowWords];
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t tx0 = ((int32_t)blockIdx.x % a.tiles_x) * kTileW, ty0 = ((int32_t)blockIdx.x / a.tiles_x) * kTileH;
    const uint8_t *in = a.in + (size_t)blockIdx.y * a.fstride;
    uint8_t *out = a.out + (size_t)blockIdx.y * a.fstride;
    const int32_t s = a.s, pad = (6 * s) & 3, rb = 3 * a.w;
    const int32_t Ba = tx0 * 3 - 6 * s - pad;                                      // the row byte of LDS byte 0: a multiple of 4
    const int32_t rw = (kTileRowBytes + 12 * s + pad + 3) / 4, rows = kTileH + 4 * s;
    for (int32_t i = tid; i < rows * rw; i += kRenderThreads) {
        const int32_t r = i / rw, j = i % rw, B = Ba + 4 * j;
        const uint8_t *row = in + (size_t)uwip_sm::clampi(ty0 - 2 * s + r, 0, a.h - 1) * rb;
        uint32_t v = 0;
        if (a.vec == 4 && B >= 0 && B + 4 <= rb) {
            v = *reinterpret_cast<const uint32_t *>(row + B);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v |= (uint32_t)row[uwip_sm::stack_clamp_byte(B + q, a.w)] << (8 * q);
        }
        s_in[r * kStackRowWords + j] = v;
    }
    __syncthreads();
    const uint8_t *lds = reinterpret_cast<const uint8_t *>(s_in);
    const int32_t th = min(kTileH, a.h - ty0), nb = min(kTileRowBytes, rb - tx0 * 3);   // rows of this tile, bytes of each
    constexpr int U = kTileRowBytes / 4;
    for (int32_t i = tid; i < kTileH * U; i += kRenderThreads) {
        const int32_t r = i / U, at = (i % U) * 4;
        if (r >= th || at >= nb) continue;
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int32_t sum = 0;
#pragma unroll
            for (int ii = 0; ii < 5; ++ii) {
                const uint8_t *p = lds + (r + ii * s) * (kStackRowWords * 4) + pad + at + q;
                int32_t rs = 0;
#pragma unroll
                for (int jj = 0; jj < 5; ++jj) rs += uwip_sm::stack_k(jj) * (int32_t)p[3 * s * jj];
                sum += uwip_sm::stack_k(ii) * rs;
            }
            v |= (uint32_t)uwip_sm::stack_round(sum) << (8 * q);
        }
        uint8_t *p = out + (size_t)(ty0 + r) * rb + (size_t)tx0 * 3 + at;
        if (a.vec == 4 && at + 4 <= nb) {
            *reinterpret_cast<uint32_t *>(p) = v;
        } else {
            for (int32_t q = 0; q < 4 && at + q < nb; ++q) p[q] = (uint8_t)(v >> (8 * q));
        }
    }
}

// UWIP_STRIP_MULTIBAND: the gather of k_strip_render with one pixel per thread on a 64 x 4 tile and two passes over the listed
// frames -- the first finds the pixel's largest feather weight (and its cover count), the second samples every level a frame
// has a weight in and accumulates the bands' sums and the residual's.  A frame whose band weights are all zero costs the
// residual level's taps alone.
template <bool GAIN>
__global__ __launch_bounds__(kRenderThreads) void k_strip_render_bands(StripBands b)
{
    __shared__ double s_A[kCullChunk][9];
    __shared__ int32_t s_idx[kCullChunk];
    __shared__ int32_t s_gq[GAIN ? kCullChunk : 1][3];
    __shared__ uint32_t s_n;
    __shared__ uint32_t s_tile[kBandTileH * kTileRowBytes / 4];
    constexpr int L = uwip_sm::kBandLevels;
    const StripRender &a = b.r;
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t tx0 = (int32_t)blockIdx.x * kTileW, ty0 = (int32_t)blockIdx.y * kBandTileH;
    const int32_t tx1 = min(tx0 + kTileW, a.cols) - 1, ty1 = min(ty0 + kBandTileH, a.rows) - 1;
    const int32_t lx = tid & (kTileW - 1), ly = tid / kTileW;
    const int32_t X = tx0 + lx, Y = ty0 + ly;
    const bool inside = X <= tx1 && Y <= ty1;
    const double px = (double)(X + a.x0), py = (double)(Y + a.y0);
    const int32_t levels = b.P.levels;

    int64_t N[L][3], W[L], NL[3] = {0, 0, 0}, WL = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) { N[l][0] = N[l][1] = N[l][2] = 0; W[l] = 0; }
    int32_t qmax = 0;
    uint32_t cnt = 0;

    for (int pass = 0; pass < 2; ++pass) {
        for (int32_t base = 0; base < a.count; base += kCullChunk) {
            __syncthreads();                               // the previous chunk's list has been read by everyone
            if (tid == 0) s_n = 0;
            __syncthreads();
            for (int32_t k = base + tid; k < min(base + kCullChunk, a.count); k += kRenderThreads) {
                const int32_t g = a.first + k;
                const int32_t *bx = a.box + 4 * (size_t)g;
                if (bx[0] <= tx1 && bx[2] >= tx0 && bx[1] <= ty1 && bx[3] >= ty0) {
                    const uint32_t slot = atomicAdd(&s_n, 1u);
                    s_idx[slot] = g;
                    for (int i = 0; i < 9; ++i) s_A[slot][i] = a.Ginv[9 * (size_t)g + i];
                    if (GAIN) for (int c = 0; c < 3; ++c) s_gq[slot][c] = a.gq[3 * (size_t)g + c];
                }
            }
            __syncthreads();
            const int32_t n = (int32_t)s_n;
            if (!inside) continue;                         // a pixel beyond the canvas: nothing to accumulate (barriers stay uniform)
            for (int32_t e = 0; e < n; ++e) {
                double A[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) A[i] = s_A[e][i];
                uwip_sm::Tap t;
                if (!uwip_sm::sample(A, px, py, a.w, a.h, t)) continue;
                if (pass == 0) {
                    qmax = t.q > qmax ? t.q : qmax;
                    cnt += 1u;
                    continue;
                }
                const int32_t g = s_idx[e];
                int32_t gq[3] = {4096, 4096, 4096};
                if (GAIN) for (int c = 0; c < 3; ++c) gq[c] = s_gq[e][c];
                int32_t wl[L];
#pragma unroll
                for (int l = 0; l < L; ++l) wl[l] = l < levels ? uwip_sm::band_weight(t.q, qmax, b.P.ramp[l]) : 0;
                const size_t o0 = ((size_t)t.y * a.w) * 3, o1 = ((size_t)t.y1 * a.w) * 3;
                int32_t prev[3] = {0, 0, 0};               // S[l - 1], when level l - 1 has a weight
#pragma unroll
                for (int l = 0; l <= L; ++l) {
                    if (l > levels) continue;
                    const bool last = l == levels;
                    const bool need = last || wl[l < L ? l : L - 1] > 0 || (l > 0 && wl[l - 1] > 0);
                    if (!need) continue;
                    const uint8_t *f = l == 0 ? a.store + (size_t)g * a.fstride : b.bands + (size_t)(l - 1) * b.lstride + (size_t)g * a.fstride;
                    const uint8_t *r0 = f + o0, *r1 = f + o1;
                    int32_t S[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        S[c] = uwip_sm::bilinear(t, r0[t.x * 3 + c], r0[t.x1 * 3 + c], r1[t.x * 3 + c], r1[t.x1 * 3 + c]);
                        if (GAIN) S[c] = uwip_sm::apply_gain(S[c], gq[c]);
                    }
                    if (l > 0 && wl[l - 1] > 0) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) N[l - 1][c] += (int64_t)wl[l - 1] * (int64_t)(prev[c] - S[c]);
                        W[l - 1] += wl[l - 1];
                    }
                    if (last) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) NL[c] += (int64_t)t.q * S[c];
                        WL += t.q;
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) prev[c] = S[c];
                }
            }
        }
    }

    uint8_t *tile = reinterpret_cast<uint8_t *>(s_tile);
    if (inside) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t v = a.fill[c];
            if (cnt > 0u) {
                int64_t bsum = 0;
#pragma unroll
                for (int l = 0; l < L; ++l) if (l < levels) bsum += uwip_sm::band_term(N[l][c], W[l]);
                v = uwip_sm::band_pixel(NL[c], WL, bsum);
            }
            tile[ly * kTileRowBytes + lx * 3 + c] = v;
        }
        if (a.cover) a.cover[(size_t)Y * a.cols + X] = (uint8_t)(cnt > 255u ? 255u : cnt);
    }
    __syncthreads();
    const int32_t th = ty1 - ty0 + 1, nb = (tx1 - tx0 + 1) * 3;       // rows of this tile, bytes of each
    uint8_t *out = a.canvas + (size_t)ty0 * a.step + (size_t)tx0 * 3;
    if (a.vec == 16) {
        constexpr int U = kTileRowBytes / 16;
        for (int32_t i = tid; i < kBandTileH * U; i += kRenderThreads) {
            const int32_t r = i / U, at = (i % U) * 16;
            if (r >= th || at >= nb) continue;
            uint8_t *p = out + (size_t)r * a.step + at;
            const uint32_t *s = s_tile + (r * kTileRowBytes + at) / 4;
            if (at + 16 <= nb) *reinterpret_cast<uint4 *>(p) = make_uint4(s[0], s[1], s[2], s[3]);
            else for (int32_t q = at; q < nb; ++q) out[(size_t)r * a.step + q] = tile[r * kTileRowBytes + q];
        }
    } else if (a.vec == 4) {
        constexpr int U = kTileRowBytes / 4;
        for (int32_t i = tid; i < kBandTileH * U; i += kRenderThreads) {
            const int32_t r = i / U, at = (i % U) * 4;
            if (r >= th || at >= nb) continue;
            uint8_t *p = out + (size_t)r * a.step + at;
            if (at + 4 <= nb) *reinterpret_cast<uint32_t *>(p) = s_tile[(r * kTileRowBytes + at) / 4];
            else for (int32_t q = at; q < nb; ++q) out[(size_t)r * a.step + q] = tile[r * kTileRowBytes + q];
        }
    } else {
        for (int32_t i = tid; i < kBandTileH * kTileRowBytes; i += kRenderThreads) {
            const int32_t r = i / kTileRowBytes, at = i % kTileRowBytes;
            if (r < th && at < nb) out[(size_t)r * a.step + at] = tile[i];
        }
    }
}
}  // namespace

struct uwip_strip {
    uwip_ctx *ctx = nullptr;
    uwip_strip_config cfg{};
    std::string err;
    int form = 0;                          // 0: no frame yet; 1: resized, detected, matched; 2: injected, stored as given
    int w = 0, h = 0;                      // geometry of the stored frames (the working size, or rows x cols when injected)
    int count = 0, last_n = 0;
    bool have_prev = false;
    uint8_t *store = nullptr;
    size_t store_bytes = 0;
    uint8_t *block = nullptr;              // the chain's arrays, one allocation
    double *H = nullptr, *G = nullptr, *Ginv = nullptr, *fb = nullptr;
    float *ratio = nullptr;
    int32_t *seg = nullptr, *box = nullptr, *nseg = nullptr;
    uwip_strip_segment *segs = nullptr;
    uwip_features *feats = nullptr;
    std::vector<int32_t> pq, pt;
    std::vector<uwip_strip_segment> h_segs;    // the last layout
    int laid = -1;                         // frame count the last layout saw (-1: none)
    int cursor = 0;                        // next segment uwip_strip_layout returns
    unsigned long long *stats = nullptr;   // [max_frames][7]: the pairs' statistics (in the block)
    int32_t *gq = nullptr;                 // [max_frames][3]
    double *g = nullptr;                   // [max_frames][3]
    bool gained = false;                   // gains computed or set since the last layout (an add, a reset, a new layout: dropped)
    uint8_t *bands = nullptr;              // [levels][band_count][h][w][3]: the frames' stacks, allocated by uwip_strip_bands
    size_t bands_bytes = 0;
    int band_count = 0;                    // frames the stacks were built for
    uwip_sm::BandParams band{};            // levels 0: no stacks (an add, a reset: dropped; a new layout keeps them)

    int fail(int code, const char *what) { err = what; return code; }
    int from_ctx(int rc) { if (rc) err = ctx->err; return rc; }
};

static bool strip_config_ok(const uwip_strip_config &c)
{
    return c.rows >= 2 && c.cols >= 2 && c.rows <= 32768 && c.cols <= 32768 && c.batch >= 1 && c.batch <= 4094 && c.max_frames >= 1 &&
           c.max_canvas_rows >= 1 && c.max_canvas_cols >= 1 && c.max_canvas_rows <= 32768 && c.max_canvas_cols <= 32768 &&
           c.max_scale >= 1.0f && c.max_scale <= 1024.0f && c.videoWidth >= 0 && c.videoHeight >= 0;
}

UWIP_API int uwip_strip_config_default(uwip_strip_config *cfg, int rows, int cols)
{
    if (!cfg || rows < 2 || cols < 2) return UWIP_ERR_INVALID;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->rows = rows; cfg->cols = cols;
    cfg->batch = 16; cfg->max_frames = 1024;
    cfg->max_canvas_rows = cfg->max_canvas_cols = 16384;
    cfg->max_scale = 4.0f;
    cfg->seed = 1;
    return UWIP_OK;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

UWIP_API int uwip_strip_create(uwip_ctx *ctx, const uwip_strip_config *cfg, uwip_strip **out)
{
    if (!ctx || !out) return UWIP_ERR_INVALID;
    *out = nullptr;
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, cfg != nullptr && strip_config_ok(*cfg), "bad strip configuration");
    uwip_strip *s = new uwip_strip;
    s->ctx = ctx; s->cfg = *cfg;
    const size_t N = (size_t)cfg->max_frames;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
    const size_t o_H = take(72 * N), o_G = take(72 * N), o_Gi = take(72 * N), o_fb = take(32 * N), o_ratio = take(4 * N), o_seg = take(4 * N),
                 o_box = take(16 * N), o_segs = take(sizeof(uwip_strip_segment) * N), o_nseg = take(4),
                 o_stats = take(8 * uwip_sm::kGainStats * N), o_gq = take(12 * N), o_g = take(24 * N);
    void *d = nullptr;
    int rc = uwip_malloc(ctx, off, &d);
    if (!rc) rc = uwip_features_create(ctx, cfg->batch + 1, &s->feats);
    if (rc) {
        if (d) uwip_free(ctx, d);
        delete s;
        return rc;
    }
    s->block = (uint8_t *)d;
    s->H = (double *)(s->block + o_H); s->G = (double *)(s->block + o_G); s->Ginv = (double *)(s->block + o_Gi);
    s->fb = (double *)(s->block + o_fb); s->ratio = (float *)(s->block + o_ratio); s->seg = (int32_t *)(s->block + o_seg);
    s->box = (int32_t *)(s->block + o_box); s->segs = (uwip_strip_segment *)(s->block + o_segs); s->nseg = (int32_t *)(s->block + o_nseg);
    s->stats = (unsigned long long *)(s->block + o_stats); s->gq = (int32_t *)(s->block + o_gq); s->g = (double *)(s->block + o_g);
    s->pq.resize(cfg->batch); s->pt.resize(cfg->batch);
    for (int i = 0; i < cfg->batch; ++i) { s->pq[i] = i + 1; s->pt[i] = i; }
    *out = s;
    return UWIP_OK;
}

UWIP_API int uwip_strip_destroy(uwip_strip *s)
{
    if (!s) return UWIP_OK;
    if (uwip_enter(s->ctx) == UWIP_OK) (void)uwip_stream_wait(s->ctx);
    if (s->feats) uwip_features_destroy(s->feats);
    if (s->store) uwip_free(s->ctx, s->store);
    if (s->bands) uwip_free(s->ctx, s->bands);
    if (s->block) uwip_free(s->ctx, s->block);
    delete s;
    return UWIP_OK;
}

UWIP_API int uwip_strip_reset(uwip_strip *s)
{
    if (!s) return UWIP_ERR_INVALID;
    s->form = 0; s->count = 0; s->last_n = 0; s->have_prev = false; s->laid = -1; s->cursor = 0; s->gained = false;
    s->h_segs.clear();
    s->band.levels = 0;
    if (s->bands) {                                        // the stacks' store goes with the frames: a strip that asks again pays again
        if (uwip_enter(s->ctx) == UWIP_OK) (void)uwip_stream_wait(s->ctx);
        uwip_free(s->ctx, s->bands);
        s->bands = nullptr; s->bands_bytes = 0;
    }
    return UWIP_OK;
}

UWIP_API int uwip_strip_count(const uwip_strip *s, int *n)
{
    if (!s || !n) return UWIP_ERR_INVALID;
    *n = s->count;
    return UWIP_OK;
}

UWIP_API const char *uwip_strip_last_error(const uwip_strip *s) { return s ? s->err.c_str() : "null strip"; }

UWIP_API int uwip_strip_add(uwip_strip *s, const uwip_batch_u8 *frames, const double *d_H_inject, const float *d_ratio_inject)
{
    if (!s) return UWIP_ERR_INVALID;
    uwip_ctx *ctx = s->ctx;
    const uwip_strip_config &c = s->cfg;
    int rc = uwip_check_batch(ctx, frames, 3);
    if (rc) return s->from_ctx(rc);
    if (frames->rows != c.rows || frames->cols != c.cols) return s->fail(UWIP_ERR_INVALID, "uwip_strip_add: not the configured frame geometry");
    if (frames->frames < 1 || frames->frames > c.batch) return s->fail(UWIP_ERR_INVALID, "uwip_strip_add: 1..batch frames per call");
    if ((d_H_inject == nullptr) != (d_ratio_inject == nullptr)) return s->fail(UWIP_ERR_INVALID, "uwip_strip_add: inject both H and ratio, or neither");
    const int form = d_H_inject ? 2 : 1, n = frames->frames;
    if (s->form && s->form != form) return s->fail(UWIP_ERR_INVALID, "uwip_strip_add: matched and injected frames do not mix in one strip");
    if ((int64_t)s->count + n > c.max_frames) return s->fail(UWIP_ERR_INVALID, "uwip_strip_add: more than max_frames frames");
    if (!s->form) {
        // the first frame decides the store's geometry; the store is allocated here, once per form (a strip that is reset keeps it)
        int w = c.cols, h = c.rows;
        if (form == 1 && (rc = uwip_overlap_working_size(c.rows, c.cols, &h, &w))) return s->fail(rc, "uwip_overlap_working_size");
        if (w > c.max_canvas_cols || h > c.max_canvas_rows) return s->fail(UWIP_ERR_INVALID, "uwip_strip_add: a frame is larger than the largest canvas");
        const size_t need = (size_t)w * h * 3 * (size_t)c.max_frames;
        if (need > s->store_bytes) {
            if (s->store) {
                UWIP_HIP(ctx, uwip_stream_wait(ctx));
                uwip_free(ctx, s->store);
                s->store = nullptr; s->store_bytes = 0;
            }
            void *d = nullptr;
            if ((rc = uwip_malloc(ctx, need, &d))) return s->from_ctx(rc);
            s->store = (uint8_t *)d; s->store_bytes = need;
        }
        s->w = w; s->h = h;
    }
    const size_t fbytes = (size_t)s->w * s->h * 3;
    uwip_batch_u8 dst;
    dst.data = s->store + (size_t)s->count * fbytes; dst.step = (size_t)s->w * 3; dst.frame_stride = fbytes;
    dst.rows = s->h; dst.cols = s->w; dst.channels = 3; dst.frames = n;
    if (form == 1) {
        // cv::resize(frame, res_frame, Size(), f, f), main.cpp:242,311: the frames the homographies refer to
        if ((rc = uwip_resize_bgr(ctx, frames, &dst))) return s->from_ctx(rc);
        if (!s->have_prev) {
            // a strip's first frame is its own predecessor, as the pipe's first frame is its own key frame (main.cpp:284-297):
            // it is detected into slot 0 and again into slot 1, and the pair (1, 0) yields an H[0] the chain never reads.
            // Deliberate: one pair list and one launch shape for every add, for one extra detect per strip
            uwip_batch_u8 first = *frames;
            first.frames = 1;
            if ((rc = uwip_overlap_detect_ex(ctx, &first, s->feats, 0, c.detect_flags))) return s->from_ctx(rc);
        } else if ((rc = uwip_features_copy(ctx, s->feats, s->last_n, s->feats, 0))) {
            return s->from_ctx(rc);
        }
        if ((rc = uwip_overlap_detect_ex(ctx, frames, s->feats, 1, c.detect_flags))) return s->from_ctx(rc);
        rc = uwip_overlap_match_ex(ctx, s->feats, s->feats, s->pq.data(), s->pt.data(), n, c.videoWidth ? c.videoWidth : c.cols,
                                   c.videoHeight ? c.videoHeight : c.rows, c.seed, c.match_flags, s->ratio + s->count, nullptr,
                                   s->H + 9 * (size_t)s->count, nullptr, nullptr);
        if (rc) return s->from_ctx(rc);
    } else {
        const int32_t rowbytes = s->w * 3;
        {
            uwip_kscope ks(ctx, "k_strip_store");
            k_strip_store<<<dim3(uwip_cdiv((size_t)rowbytes, 256), (unsigned)s->h, (unsigned)n), 256, 0, ctx->stream>>>(
                (const uint8_t *)frames->data, frames->step, frames->frame_stride, s->h, rowbytes, (uint8_t *)dst.data);
            UWIP_HIP(ctx, hipGetLastError());
        }
        UWIP_HIP(ctx, hipMemcpyAsync(s->H + 9 * (size_t)s->count, d_H_inject, 72 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
        UWIP_HIP(ctx, hipMemcpyAsync(s->ratio + s->count, d_ratio_inject, 4 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    }
    s->form = form; s->have_prev = true; s->last_n = n; s->count += n; s->gained = false; s->band.levels = 0;
    return UWIP_OK;
}

static uwip_sm::ChainParams chain_params(int w, int h, int max_rows, int max_cols, float max_scale)
{
    uwip_sm::ChainParams P;
    P.w = w; P.h = h; P.max_rows = max_rows; P.max_cols = max_cols; P.max_scale = (double)max_scale;
    return P;
}

// run the chain over what has been added and fetch the segments, unless the last layout is still current
static int strip_lay_out(uwip_strip *s)
{
    uwip_ctx *ctx = s->ctx;
    if (s->laid == s->count) return UWIP_OK;
    s->h_segs.clear();
    s->gained = false;
    if (s->count > 0) {
        uwip_sm::ChainOut o;
        o.G = s->G; o.Ginv = s->Ginv; o.seg = s->seg; o.box = s->box; o.segs = s->segs; o.nseg = s->nseg;
        {
            uwip_kscope ks(ctx, "k_strip_chain");
            k_strip_chain<<<1, 64, 0, ctx->stream>>>(chain_params(s->w, s->h, s->cfg.max_canvas_rows, s->cfg.max_canvas_cols, s->cfg.max_scale),
                                                     s->H, s->ratio, s->count, o, s->fb);
            UWIP_HIP(ctx, hipGetLastError());
        }
        int32_t nseg = 0;
        int rc = uwip_memcpy_d2h(ctx, &nseg, s->nseg, 4);
        if (rc) return rc;
        if (nseg < 1 || nseg > s->count) return ctx->fail(UWIP_ERR_HIP, "k_strip_chain left no segment count");
        s->h_segs.resize(nseg);
        if ((rc = uwip_memcpy_d2h(ctx, s->h_segs.data(), s->segs, sizeof(uwip_strip_segment) * (size_t)nseg))) return rc;
    }
    s->laid = s->count;
    return UWIP_OK;
}

UWIP_API int uwip_strip_layout(uwip_strip *s, uwip_strip_segment *h_segs, int cap, int *n)
{
    if (!s) return UWIP_ERR_INVALID;
    if (!h_segs || !n || cap < 1) return s->fail(UWIP_ERR_INVALID, "uwip_strip_layout: h_segs, n and cap >= 1");
    *n = 0;
    if (int rc_e = uwip_enter(s->ctx)) return s->from_ctx(rc_e);
    if (s->laid != s->count) s->cursor = 0;                 // frames were added: the listing starts over
    if (int rc = strip_lay_out(s)) return s->from_ctx(rc);
    const int total = (int)s->h_segs.size(), at = std::min(s->cursor, total), k = std::min(cap, total - at);
    std::copy(s->h_segs.begin() + at, s->h_segs.begin() + at + k, h_segs);
    *n = k;
    s->cursor = k == cap ? at + k : 0;
    return UWIP_OK;
}

UWIP_API int uwip_strip_transforms(uwip_strip *s, double *h_G, double *h_Ginv, int32_t *h_seg, int32_t *h_box)
{
    if (!s) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(s->ctx)) return s->from_ctx(rc_e);
    if (s->laid != s->count) return s->fail(UWIP_ERR_INVALID, "uwip_strip_transforms: call uwip_strip_layout first");
    const size_t N = (size_t)s->count;
    int rc = UWIP_OK;
    if (!rc && h_G) rc = uwip_memcpy_d2h(s->ctx, h_G, s->G, 72 * N);
    if (!rc && h_Ginv) rc = uwip_memcpy_d2h(s->ctx, h_Ginv, s->Ginv, 72 * N);
    if (!rc && h_seg) rc = uwip_memcpy_d2h(s->ctx, h_seg, s->seg, 4 * N);
    if (!rc && h_box) rc = uwip_memcpy_d2h(s->ctx, h_box, s->box, 16 * N);
    return s->from_ctx(rc);
}

UWIP_API int uwip_strip_render(uwip_strip *s, int segment, int mode, const uint8_t *fill, const uwip_batch_u8 *canvas, uint8_t *d_cover)
{
    if (!s) return UWIP_ERR_INVALID;
    uwip_ctx *ctx = s->ctx;
    int rc = uwip_check_batch(ctx, canvas, 3);
    if (rc) return s->from_ctx(rc);
    if (s->laid != s->count || s->count == 0) return s->fail(UWIP_ERR_INVALID, "uwip_strip_render: call uwip_strip_layout first");
    if (segment < 0 || segment >= (int)s->h_segs.size()) return s->fail(UWIP_ERR_INVALID, "uwip_strip_render: no such segment");
    const bool gain = (mode & UWIP_STRIP_GAIN) != 0;
    mode &= ~UWIP_STRIP_GAIN;
    if (mode != UWIP_STRIP_FEATHER && mode != UWIP_STRIP_FIRST && mode != UWIP_STRIP_LAST && mode != UWIP_STRIP_MULTIBAND)
        return s->fail(UWIP_ERR_INVALID, "uwip_strip_render: unknown mode");
    if (mode == UWIP_STRIP_MULTIBAND && (s->band.levels == 0 || s->band_count != s->count))
        return s->fail(UWIP_ERR_INVALID, "uwip_strip_render: UWIP_STRIP_MULTIBAND without uwip_strip_bands since the last add");
    if (gain && !s->gained) return s->fail(UWIP_ERR_INVALID, "uwip_strip_render: UWIP_STRIP_GAIN without uwip_strip_gains or uwip_strip_set_gains since the last layout");
    const uwip_strip_segment &g = s->h_segs[segment];
    if (canvas->frames != 1 || canvas->rows != g.rows || canvas->cols != g.cols)
        return s->fail(UWIP_ERR_INVALID, "uwip_strip_render: the canvas is not one frame of the segment's rows x cols");
    StripRender a;
    a.store = s->store; a.fstride = (size_t)s->w * s->h * 3; a.w = s->w; a.h = s->h;
    a.Ginv = s->Ginv; a.box = s->box; a.first = g.first; a.count = g.count;
    a.x0 = g.x0; a.y0 = g.y0; a.rows = g.rows; a.cols = g.cols;
    a.canvas = (uint8_t *)canvas->data; a.step = canvas->step; a.cover = d_cover;
    for (int c = 0; c < 3; ++c) a.fill[c] = fill ? fill[c] : 0;
    a.fill[3] = 0;
    // the tile's rows start at multiples of 192 bytes from the row's start: base and step decide the store width
    const uintptr_t al = (uintptr_t)canvas->data | (uintptr_t)canvas->step;
    a.vec = al % 16 == 0 ? 16 : (al % 4 == 0 ? 4 : 1);
    if (mode == UWIP_STRIP_MULTIBAND) {
        StripBands b;
        b.r = a; b.bands = s->bands; b.lstride = (size_t)s->band_count * a.fstride; b.P = s->band;
        const dim3 bgrid(uwip_cdiv((size_t)g.cols, kTileW), uwip_cdiv((size_t)g.rows, kBandTileH));
        if (gain) {
            b.r.gq = s->gq;
            uwip_kscope ks(ctx, "k_strip_render_bands_gain");
            k_strip_render_bands<true><<<bgrid, kRenderThreads, 0, ctx->stream>>>(b);
            UWIP_HIP(ctx, hipGetLastError());
            return UWIP_OK;
        }
        uwip_kscope ks(ctx, "k_strip_render_bands");
        k_strip_render_bands<false><<<bgrid, kRenderThreads, 0, ctx->stream>>>(b);
        UWIP_HIP(ctx, hipGetLastError());
        return UWIP_OK;
    }
    const dim3 grid(uwip_cdiv((size_t)g.cols, kTileW), uwip_cdiv((size_t)g.rows, kTileH));
    if (gain) {
        a.gq = s->gq;
        uwip_kscope ks(ctx, "k_strip_render_gain");
        if (mode == UWIP_STRIP_FEATHER) k_strip_render<UWIP_STRIP_FEATHER, true><<<grid, kRenderThreads, 0, ctx->stream>>>(a);
        else if (mode == UWIP_STRIP_FIRST) k_strip_render<UWIP_STRIP_FIRST, true><<<grid, kRenderThreads, 0, ctx->stream>>>(a);
        else k_strip_render<UWIP_STRIP_LAST, true><<<grid, kRenderThreads, 0, ctx->stream>>>(a);
        UWIP_HIP(ctx, hipGetLastError());
        return UWIP_OK;
    }
    uwip_kscope ks(ctx, "k_strip_render");
    if (mode == UWIP_STRIP_FEATHER) k_strip_render<UWIP_STRIP_FEATHER><<<grid, kRenderThreads, 0, ctx->stream>>>(a);
    else if (mode == UWIP_STRIP_FIRST) k_strip_render<UWIP_STRIP_FIRST><<<grid, kRenderThreads, 0, ctx->stream>>>(a);
    else k_strip_render<UWIP_STRIP_LAST><<<grid, kRenderThreads, 0, ctx->stream>>>(a);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

// ---- multi-band blending ------------------------------------------------------------------------------------------------------
UWIP_API int uwip_strip_bands_config_default(uwip_strip_bands_config *cfg)
{
    if (!cfg) return UWIP_ERR_INVALID;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->levels = 4;
    for (int l = 0; l < 4; ++l) cfg->ramp[l] = 1 << l;
    return UWIP_OK;
}

static bool bands_config_ok(const uwip_strip_bands_config &c)
{
    if (c.levels < 1 || c.levels > uwip_sm::kBandLevels) return false;
    for (int l = 0; l < c.levels; ++l) if (c.ramp[l] < 1 || c.ramp[l] > 4096) return false;
    return true;
}

UWIP_API int uwip_strip_bands(uwip_strip *s, const uwip_strip_bands_config *cfg)
{
    if (!s) return UWIP_ERR_INVALID;
    uwip_ctx *ctx = s->ctx;
    if (int rc_e = uwip_enter(ctx)) return s->from_ctx(rc_e);
    uwip_strip_bands_config c;
    if (cfg) c = *cfg; else uwip_strip_bands_config_default(&c);
    if (!bands_config_ok(c)) return s->fail(UWIP_ERR_INVALID, "uwip_strip_bands: levels 1..4, ramp[l] 1..4096 for l < levels");
    if (s->count == 0) return s->fail(UWIP_ERR_INVALID, "uwip_strip_bands: no frame");
    const size_t fstride = (size_t)s->w * s->h * 3, lstride = fstride * (size_t)s->count, need = lstride * (size_t)c.levels;
    if (need > s->bands_bytes) {
        if (s->bands) {
            if (hipError_t e = uwip_stream_wait(ctx)) return s->from_ctx(ctx->fail(UWIP_ERR_HIP, "uwip_stream_wait", hipGetErrorString(e)));
            uwip_free(ctx, s->bands);
            s->bands = nullptr; s->bands_bytes = 0; s->band.levels = 0;
        }
        void *d = nullptr;
        if (int rc = uwip_malloc(ctx, need, &d)) return s->from_ctx(rc);
        s->bands = (uint8_t *)d; s->bands_bytes = need;
    }
    StripStack a;
    a.fstride = fstride; a.w = s->w; a.h = s->h;
    a.tiles_x = (int32_t)uwip_cdiv((size_t)s->w, kTileW);
    a.vec = (s->w * 3) % 4 == 0 ? 4 : 1;                    // the stores' bases are allocations: rows of whole words decide
    const dim3 grid((unsigned)a.tiles_x * uwip_cdiv((size_t)s->h, kTileH), (unsigned)s->count);
    for (int l = 0; l < c.levels; ++l) {
        a.in = l == 0 ? s->store : s->bands + (size_t)(l - 1) * lstride;
        a.out = s->bands + (size_t)l * lstride;
        a.s = 1 << l;
        static const char *const names[uwip_sm::kBandLevels] = {"k_strip_stack_1", "k_strip_stack_2", "k_strip_stack_4", "k_strip_stack_8"};
        uwip_kscope ks(ctx, names[l]);                      // the profile keeps the levels apart, by their tap distance
        k_strip_stack<<<grid, kRenderThreads, 0, ctx->stream>>>(a);
        if (hipError_t e = hipGetLastError()) { s->band.levels = 0; return s->from_ctx(ctx->fail(UWIP_ERR_HIP, "k_strip_stack", hipGetErrorString(e))); }
    }
    s->band.levels = c.levels;
    for (int l = 0; l < uwip_sm::kBandLevels; ++l) s->band.ramp[l] = l < c.levels ? c.ramp[l] : 1;
    s->band_count = s->count;
    return UWIP_OK;
}

UWIP_API int uwip_strip_band_level(uwip_strip *s, int frame, int level, uint8_t *h_out)
{
    if (!s) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(s->ctx)) return s->from_ctx(rc_e);
    if (!h_out) return s->fail(UWIP_ERR_INVALID, "uwip_strip_band_level: h_out");
    if (s->band.levels == 0 || s->band_count != s->count) return s->fail(UWIP_ERR_INVALID, "uwip_strip_band_level: no stacks since the last add");
    if (frame < 0 || frame >= s->count || level < 1 || level > s->band.levels) return s->fail(UWIP_ERR_INVALID, "uwip_strip_band_level: no such frame or level");
    const size_t fstride = (size_t)s->w * s->h * 3;
    return s->from_ctx(uwip_memcpy_d2h(s->ctx, h_out, s->bands + ((size_t)(level - 1) * s->band_count + frame) * fstride, fstride));
}

UWIP_API int uwip_strip_stack_host(const uint8_t *frame, int w, int h, int levels, uint8_t *out)
{
    if (!frame || !out || w < 1 || h < 1 || w > 32768 || h > 32768 || levels < 1 || levels > uwip_sm::kBandLevels) return UWIP_ERR_INVALID;
    const size_t fstride = (size_t)w * h * 3;
    for (int l = 0; l < levels; ++l) {
        const uint8_t *in = l == 0 ? frame : out + (size_t)(l - 1) * fstride;
        uint8_t *o = out + (size_t)l * fstride;
        for (int y = 0; y < h; ++y)
            for (int B = 0; B < 3 * w; ++B) o[(size_t)y * w * 3 + B] = uwip_sm::stack_byte(in, w, h, 1 << l, y, B);
    }
    return UWIP_OK;
}

// ---- gain compensation ----------------------------------------------------------------------------------------------------
UWIP_API int uwip_strip_gain_config_default(uwip_strip_gain_config *cfg)
{
    if (!cfg) return UWIP_ERR_INVALID;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->sigma_n = 10.0f; cfg->sigma_g = 0.1f;
    cfg->lo = 5; cfg->hi = 250; cfg->min_pixels = 64;
    return UWIP_OK;
}

static bool gain_config_ok(const uwip_strip_gain_config &c)
{
    return c.sigma_n > 0.0f && c.sigma_g > 0.0f && c.sigma_n <= 3.0e38f && c.sigma_g <= 3.0e38f && c.lo >= 0 && c.hi <= 255 && c.lo <= c.hi &&
           c.min_pixels >= 1;
}

static uwip_sm::GainParams gain_params(const uwip_strip_gain_config *cfg)
{
    uwip_strip_gain_config c;
    if (cfg) c = *cfg; else uwip_strip_gain_config_default(&c);
    uwip_sm::GainParams P;
    P.sigma_n = (double)c.sigma_n; P.sigma_g = (double)c.sigma_g; P.lo = c.lo; P.hi = c.hi; P.min_pixels = c.min_pixels;
    return P;
}

UWIP_API int uwip_strip_gains(uwip_strip *s, const uwip_strip_gain_config *cfg)
{
    if (!s) return UWIP_ERR_INVALID;
    uwip_ctx *ctx = s->ctx;
    if (int rc_e = uwip_enter(ctx)) return s->from_ctx(rc_e);
    if (cfg && !gain_config_ok(*cfg)) return s->fail(UWIP_ERR_INVALID, "uwip_strip_gains: sigma_n, sigma_g > 0, 0 <= lo <= hi <= 255, min_pixels >= 1");
    if (s->laid != s->count || s->count == 0) return s->fail(UWIP_ERR_INVALID, "uwip_strip_gains: call uwip_strip_layout first");
    const uwip_sm::GainParams P = gain_params(cfg);
    const size_t N = (size_t)s->count;
    if (hipError_t e = hipMemsetAsync(s->stats, 0, 8 * uwip_sm::kGainStats * N, ctx->stream)) return s->from_ctx(ctx->fail(UWIP_ERR_HIP, "hipMemsetAsync", hipGetErrorString(e)));
    StripGainStats a;
    a.store = s->store; a.fstride = (size_t)s->w * s->h * 3; a.w = s->w; a.h = s->h;
    a.G = s->G; a.Ginv = s->Ginv; a.seg = s->seg; a.P = P; a.stats = s->stats;
    a.tiles_x = (int32_t)uwip_cdiv((size_t)s->w, kTileW);
    {
        uwip_kscope ks(ctx, "k_strip_gain_stats");
        k_strip_gain_stats<<<dim3((unsigned)a.tiles_x * uwip_cdiv((size_t)s->h, kTileH), (unsigned)s->count), kRenderThreads, 0, ctx->stream>>>(a);
        if (hipError_t e = hipGetLastError()) return s->from_ctx(ctx->fail(UWIP_ERR_HIP, "k_strip_gain_stats", hipGetErrorString(e)));
    }
    {
        uwip_kscope ks(ctx, "k_strip_gain_solve");
        k_strip_gain_solve<<<1, 64, 0, ctx->stream>>>(P, s->stats, s->seg, s->count, s->gq, s->g, s->fb);     // fb: free once the chain has run
        if (hipError_t e = hipGetLastError()) return s->from_ctx(ctx->fail(UWIP_ERR_HIP, "k_strip_gain_solve", hipGetErrorString(e)));
    }
    s->gained = true;
    return UWIP_OK;
}

UWIP_API int uwip_strip_gain_values(uwip_strip *s, int32_t *h_gq, double *h_g, uint64_t *h_stats)
{
    if (!s) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(s->ctx)) return s->from_ctx(rc_e);
    if (s->laid != s->count || !s->gained) return s->fail(UWIP_ERR_INVALID, "uwip_strip_gain_values: no gains since the last layout");
    const size_t N = (size_t)s->count;
    int rc = UWIP_OK;
    if (!rc && h_gq) rc = uwip_memcpy_d2h(s->ctx, h_gq, s->gq, 12 * N);
    if (!rc && h_g) rc = uwip_memcpy_d2h(s->ctx, h_g, s->g, 24 * N);
    if (!rc && h_stats) rc = uwip_memcpy_d2h(s->ctx, h_stats, s->stats, 8 * uwip_sm::kGainStats * N);
    return s->from_ctx(rc);
}

UWIP_API int uwip_strip_set_gains(uwip_strip *s, const int32_t *h_gq)
{
    if (!s) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(s->ctx)) return s->from_ctx(rc_e);
    if (!h_gq) return s->fail(UWIP_ERR_INVALID, "uwip_strip_set_gains: h_gq");
    if (s->laid != s->count || s->count == 0) return s->fail(UWIP_ERR_INVALID, "uwip_strip_set_gains: call uwip_strip_layout first");
    const size_t N = (size_t)s->count;
    std::vector<double> g(3 * N);
    for (size_t i = 0; i < 3 * N; ++i) {
        if (h_gq[i] < 1024 || h_gq[i] > 16384) return s->fail(UWIP_ERR_INVALID, "uwip_strip_set_gains: a gain outside 1024..16384");
        g[i] = (double)h_gq[i] / 4096.0;
    }
    // the taps of injected gains: g = gq / 4096, no statistics
    int rc = uwip_memcpy_h2d(s->ctx, s->gq, h_gq, 12 * N);
    if (!rc) rc = uwip_memcpy_h2d(s->ctx, s->g, g.data(), 24 * N);
    if (rc) return s->from_ctx(rc);
    if (hipError_t e = hipMemsetAsync(s->stats, 0, 8 * uwip_sm::kGainStats * N, s->ctx->stream)) return s->from_ctx(s->ctx->fail(UWIP_ERR_HIP, "hipMemsetAsync", hipGetErrorString(e)));
    s->gained = true;
    return UWIP_OK;
}

UWIP_API int uwip_strip_gain_solve_host(const uint64_t *h_stats, const int32_t *h_seg, int n, const uwip_strip_gain_config *cfg, int32_t *h_gq,
                                        double *h_g)
{
    if (n < 0 || (n > 0 && (!h_stats || !h_seg)) || (cfg && !gain_config_ok(*cfg))) return UWIP_ERR_INVALID;
    const size_t N = (size_t)n;
    std::vector<double> g(3 * N), scr(3 * N);
    std::vector<int32_t> gq(3 * N);
    uwip_sm::gain_solve(gain_params(cfg), h_stats, h_seg, n, gq.data(), g.data(), scr.data());
    if (h_gq) std::copy(gq.begin(), gq.end(), h_gq);
    if (h_g) std::copy(g.begin(), g.end(), h_g);
    return UWIP_OK;
}

UWIP_API int uwip_strip_chain_host(int w, int h, int max_canvas_rows, int max_canvas_cols, float max_scale, const double *h_H,
                                   const float *h_ratio, int n, double *h_G, double *h_Ginv, int32_t *h_seg, int32_t *h_box,
                                   uwip_strip_segment *h_segs, int cap, int *n_segs)
{
    if (w < 2 || h < 2 || w > 32768 || h > 32768 || max_canvas_rows < h || max_canvas_cols < w || max_canvas_rows > 32768 ||
        max_canvas_cols > 32768 || !(max_scale >= 1.0f) || max_scale > 1024.0f || n < 0 || (n > 0 && (!h_H || !h_ratio)) || !n_segs ||
        cap < 0 || (cap > 0 && !h_segs))
        return UWIP_ERR_INVALID;
    const size_t N = (size_t)n;
    std::vector<double> G(9 * N), Ginv(9 * N), fb(4 * N);
    std::vector<int32_t> seg(N), box(4 * N);
    std::vector<uwip_strip_segment> segs(N);
    int32_t nseg = 0;
    uwip_sm::ChainOut o;
    o.G = G.data(); o.Ginv = Ginv.data(); o.seg = seg.data(); o.box = box.data(); o.segs = segs.data(); o.nseg = &nseg;
    uwip_sm::chain(chain_params(w, h, max_canvas_rows, max_canvas_cols, max_scale), h_H, h_ratio, n, o, fb.data());
    if (h_G) std::copy(G.begin(), G.end(), h_G);
    if (h_Ginv) std::copy(Ginv.begin(), Ginv.end(), h_Ginv);
    if (h_seg) std::copy(seg.begin(), seg.end(), h_seg);
    if (h_box) std::copy(box.begin(), box.end(), h_box);
    std::copy(segs.begin(), segs.begin() + std::min(nseg, cap), h_segs ? h_segs : segs.data());
    *n_segs = nseg;
    return UWIP_OK;
}
