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
//   k_strip_render_bands  the gather of k_strip_render, one pixel per thread, blending the stacks' bands (UWIP_STRIP_MULTIBAND);
//   k_strip_seam_cost  seams, the measurement: the tile of k_strip_gain_stats, one cost per pixel of frame k against frame k - 1,
//                    written in the order the path reads it (transposed through LDS when the path runs along x);
//   k_strip_seam_path  one workgroup per pair runs strip_core.hpp's seam_step() over the steps, the states in parallel, E double-
//                    buffered in LDS, back pointers of 2 bits in LDS or in global scratch; one lane walks back.
//   k_strip_render<UWIP_STRIP_SEAM> paints every frame over the ones below it on its side of its seam.
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

// what k_strip_render<UWIP_STRIP_SEAM> takes besides: the seams stay in global memory (a wave's 64 pixels read neighbouring entries)
struct StripSeams {
    const int32_t *seam = nullptr;        // [frames][L]: each frame's seam against the one before
    const int32_t *orient = nullptr;      // [frames]: axis | sign of each seam
    int32_t L = 0;
};

constexpr int kSeamRound = 64;                               // pairs whose costs the scratch holds at a time
constexpr int kSeamStates = (uwip_sm::kSeamMaxSide + kRenderThreads - 1) / kRenderThreads;    // most states a thread of the path owns
constexpr int kSeamBackLdsWords = 15360;                     // back pointers kept in LDS: 60 KB (360 x 640 / 16 words are 57.6 KB)
constexpr int kSeamCostPad = kTileW + 4;                     // the transposed read's 16 rows x 4 columns: 64 different banks

struct StripSeam {
    const uint8_t *store;                 // [frames][h][w][3]
    size_t fstride;
    int32_t w, h;
    const double *G, *Ginv;               // [frames][9]
    const int32_t *seg;                   // [frames]
    const int32_t *gq;                    // [frames][3] or null
    uwip_sm::SeamParams P;
    int32_t k0;                           // the round's first frame: blockIdx.y (cost) / blockIdx.x (path) = frame - k0 = the slot
    int32_t tiles_x;
    uint32_t *cost;                       // [round][T][S]
    uint32_t *back;                       // [round][back_stride] words of back pointers for k_strip_seam_path<false>
    size_t back_stride;
    int32_t *orient;                      // [frames]
    int32_t *seam;                        // [frames][L]
    int32_t L;                            // max(w, h)
    unsigned long long *total;            // [frames]
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

// Frame k = k0 + blockIdx.y against frame k - 1: the cost of every pixel of the tile, into cost[slot] in path order [t][s].
// Axis 1 (t = y, s = x): a wave's 64 pixels of a row are 64 consecutive entries.  Axis 0 (t = x, s = y): the tile goes through
// LDS and comes out as 64 runs of 16 consecutive entries.
__global__ __launch_bounds__(kRenderThreads) void k_strip_seam_cost(StripSeam a)
{
    __shared__ uint32_t s_c[kTileH][kSeamCostPad];
    __shared__ int32_t s_orient;
    const int32_t k = a.k0 + (int32_t)blockIdx.y;
    if (k == 0 || a.seg[k] != a.seg[k - 1]) return;        // the first frame of a segment has no seam (uniform: no barrier yet)
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t tx0 = ((int32_t)blockIdx.x % a.tiles_x) * kTileW, ty0 = ((int32_t)blockIdx.x / a.tiles_x) * kTileH;
    const int32_t lx = tid & (kTileW - 1), ly = tid / kTileW, x = tx0 + lx;
    if (tid == 0) {
        s_orient = uwip_sm::seam_orient(a.G + 9 * (size_t)(k - 1), a.Ginv + 9 * (size_t)k, a.w, a.h);
        if (blockIdx.x == 0) a.orient[k] = s_orient;
    }
    __syncthreads();
    const int32_t axis = uwip_sm::seam_axis(s_orient);
    const uint8_t *fk = a.store + (size_t)k * a.fstride, *fp = a.store + (size_t)(k - 1) * a.fstride;
    const int32_t *gk = a.gq ? a.gq + 3 * (size_t)k : nullptr, *gp = a.gq ? a.gq + 3 * (size_t)(k - 1) : nullptr;
    uint32_t *C = a.cost + (size_t)blockIdx.y * ((size_t)a.w * a.h);
    double G[9], Ap[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { G[i] = a.G[9 * (size_t)k + i]; Ap[i] = a.Ginv[9 * (size_t)(k - 1) + i]; }
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int32_t r = ly + j * (kRenderThreads / kTileW), y = ty0 + r;
        const bool in = x < a.w && y < a.h;
        const uint32_t c = in ? uwip_sm::seam_cost(a.P, fk, fp, G, Ap, gk, gp, axis, x, y, a.w, a.h) : 0u;
        if (axis) { if (in) C[(size_t)y * a.w + x] = c; }
        else s_c[r][lx] = c;
    }
    if (axis) return;                                      // uniform
    __syncthreads();
    for (int32_t i = tid; i < kTileW * kTileH; i += kRenderThreads) {
        const int32_t cx = i / kTileH, cy = i % kTileH;
        if (tx0 + cx < a.w && ty0 + cy < a.h) C[(size_t)(tx0 + cx) * a.h + (ty0 + cy)] = s_c[cy][cx];
    }
}

// The pair of frame k = k0 + blockIdx.x: T sequential steps, a thread owns the states tid, tid + 256, ...  The back pointer of
// (t, s) is bits 2 (t & 15) of word [t >> 4][s]: a thread collects 16 steps of a state in a register, so no two threads share
// a word.  LDS_BACK: the words are in LDS (the launch code has checked that they fit), otherwise in a.back.
template <bool LDS_BACK>
__global__ __launch_bounds__(kRenderThreads) void k_strip_seam_path(StripSeam a)
{
    __shared__ uint32_t s_E[2][uwip_sm::kSeamMaxSide + 1];
    __shared__ uint32_t s_back[LDS_BACK ? kSeamBackLdsWords : 1];
    const int32_t k = a.k0 + (int32_t)blockIdx.x, tid = (int32_t)threadIdx.x;
    int32_t *seam = a.seam + (size_t)k * a.L;
    if (k == 0 || a.seg[k] != a.seg[k - 1]) {              // a segment's first frame: no seam (uniform)
        for (int32_t i = tid; i < a.L; i += kRenderThreads) seam[i] = -1;
        if (tid == 0) { a.orient[k] = 0; a.total[k] = 0; }
        return;
    }
    const int32_t axis = uwip_sm::seam_axis(a.orient[k]);
    const int32_t T = axis ? a.h : a.w, S = axis ? a.w : a.h;
    const uint32_t *C = a.cost + (size_t)blockIdx.x * ((size_t)a.w * a.h);
    uint32_t *back = LDS_BACK ? s_back : a.back + (size_t)blockIdx.x * a.back_stride;
    uint32_t acc[kSeamStates], next[kSeamStates];
#pragma unroll
    for (int j = 0; j < kSeamStates; ++j) {
        const int32_t s = tid + j * kRenderThreads;
        acc[j] = 0; next[j] = 0;
        if (s < S) {
            s_E[0][s] = C[s];
            if (T > 1) next[j] = C[(size_t)S + s];
        }
    }
    __syncthreads();
    for (int32_t t = 1; t < T; ++t) {
        const uint32_t *prev = s_E[(t - 1) & 1];
        uint32_t *cur = s_E[t & 1];
        const bool flush = (t & 15) == 15 || t == T - 1;
#pragma unroll
        for (int j = 0; j < kSeamStates; ++j) {
            const int32_t s = tid + j * kRenderThreads;
            if (s >= S) continue;
            const uint32_t c = next[j];
            if (t + 1 < T) next[j] = C[(size_t)(t + 1) * S + s];       // the next step's cost is on its way during this one
            uint32_t bp;
            cur[s] = uwip_sm::seam_step(prev, S, s, c, bp);
            acc[j] |= bp << (2 * (t & 15));
            if (flush) { back[(size_t)(t >> 4) * S + s] = acc[j]; acc[j] = 0; }
        }
        __syncthreads();                                   // E[t] is complete; E[t - 1] may be overwritten by step t + 1
    }
    for (int32_t i = T + tid; i < a.L; i += kRenderThreads) seam[i] = -1;
    if (tid != 0) return;
    const uint32_t *last = s_E[(T - 1) & 1];
    int32_t s = 0;
    for (int32_t i = 1; i < S; ++i) if (last[i] < last[s]) s = i;
    a.total[k] = last[s];
    for (int32_t t = T - 1; t >= 0; --t) {
        seam[t] = s;
        if (t > 0) s = uwip_sm::seam_back(s, (back[(size_t)(t >> 4) * S + s] >> (2 * (t & 15))) & 3u);
    }
}

// GAIN: every sample is multiplied by its frame's gain (a.gq) before it is blended; false is the kernel without gains.
// UWIP_STRIP_SEAM keeps two candidates per pixel -- the largest covering frame on its own side of its seam (den, num) and the
// smallest covering frame (lo, nlo) -- so the result does not depend on the order of the tile's listing.
template <int MODE, bool GAIN = false>
__global__ __launch_bounds__(kRenderThreads) void k_strip_render(StripRender a, StripSeams q = StripSeams())
{
    __shared__ double s_A[kCullChunk][9];
    __shared__ int32_t s_idx[kCullChunk];
    __shared__ int32_t s_gq[GAIN ? kCullChunk : 1][3];
    __shared__ int32_t s_or[MODE == UWIP_STRIP_SEAM ? kCullChunk : 1];       // the listed frames' orient; -1: the segment's first
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
    int32_t lo[kPix], nlo[kPix][3];                       // UWIP_STRIP_SEAM alone
#pragma unroll
    for (int j = 0; j < kPix; ++j) { num[j][0] = num[j][1] = num[j][2] = 0; den[j] = MODE == UWIP_STRIP_FEATHER ? 0 : -1; cnt[j] = 0; }
    if (MODE == UWIP_STRIP_SEAM) {
#pragma unroll
        for (int j = 0; j < kPix; ++j) { lo[j] = -1; nlo[j][0] = nlo[j][1] = nlo[j][2] = 0; }
    }

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
                if (MODE == UWIP_STRIP_SEAM) s_or[slot] = g == a.first ? -1 : q.orient[g];
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
                if (MODE == UWIP_STRIP_SEAM) {
                    const int32_t o = s_or[e];
                    const bool best = o >= 0 && g > den[j] &&
                                      uwip_sm::seam_side(o, q.seam + (size_t)g * q.L, t.x + (t.fx >= 16), t.y + (t.fy >= 16));
                    const bool lowest = lo[j] < 0 || g < lo[j];
                    if (!best && !lowest) continue;
                    const uint8_t *r0 = f + ((size_t)t.y * a.w) * 3, *r1 = f + ((size_t)t.y1 * a.w) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        int32_t P = uwip_sm::bilinear(t, r0[t.x * 3 + c], r0[t.x1 * 3 + c], r1[t.x * 3 + c], r1[t.x1 * 3 + c]);
                        if (GAIN) P = uwip_sm::apply_gain(P, gq[c]);
                        if (best) num[j][c] = P;
                        if (lowest) nlo[j][c] = P;
                    }
                    if (best) den[j] = g;
                    if (lowest) lo[j] = g;
                    continue;
                }
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
            } else if (MODE == UWIP_STRIP_SEAM && lo[j] >= 0) {
                v = (uint8_t)((nlo[j][c] + 512) >> 10);
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
    uint8_t *seam_block = nullptr;         // seam [max_frames][max(w, h)], orient [max_frames], total [max_frames]: allocated by
    int32_t *seam = nullptr, *orient = nullptr;    // uwip_strip_seams / uwip_strip_set_seams, freed by reset and destroy
    unsigned long long *total = nullptr;
    uint8_t *seam_scratch = nullptr;       // the costs of a round of pairs, and their back pointers where LDS cannot hold them
    size_t seam_scratch_bytes = 0;
    bool seamed = false;                   // seams found or set since the last layout and the last gains (dropped as the gains are)

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
    if (s->seam_block) uwip_free(s->ctx, s->seam_block);
    if (s->seam_scratch) uwip_free(s->ctx, s->seam_scratch);
    if (s->block) uwip_free(s->ctx, s->block);
    delete s;
    return UWIP_OK;
}

UWIP_API int uwip_strip_reset(uwip_strip *s)
{
    if (!s) return UWIP_ERR_INVALID;
    s->form = 0; s->count = 0; s->last_n = 0; s->have_prev = false; s->laid = -1; s->cursor = 0; s->gained = false;
    s->h_segs.clear();
    s->band.levels = 0; s->seamed = false;
    if (s->bands || s->seam_block || s->seam_scratch) {    // these stores go with the frames: a strip that asks again pays again
        if (uwip_enter(s->ctx) == UWIP_OK) (void)uwip_stream_wait(s->ctx);
        if (s->bands) uwip_free(s->ctx, s->bands);
        if (s->seam_block) uwip_free(s->ctx, s->seam_block);
        if (s->seam_scratch) uwip_free(s->ctx, s->seam_scratch);
        s->bands = nullptr; s->bands_bytes = 0;
        s->seam_block = nullptr; s->seam = s->orient = nullptr; s->total = nullptr;
        s->seam_scratch = nullptr; s->seam_scratch_bytes = 0;
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
    s->form = form; s->have_prev = true; s->last_n = n; s->count += n; s->gained = false; s->seamed = false; s->band.levels = 0;
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
    s->gained = false; s->seamed = false;
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
    if (mode != UWIP_STRIP_FEATHER && mode != UWIP_STRIP_FIRST && mode != UWIP_STRIP_LAST && mode != UWIP_STRIP_MULTIBAND && mode != UWIP_STRIP_SEAM)
        return s->fail(UWIP_ERR_INVALID, "uwip_strip_render: unknown mode");
    if (mode == UWIP_STRIP_SEAM && !s->seamed)
        return s->fail(UWIP_ERR_INVALID, "uwip_strip_render: UWIP_STRIP_SEAM without uwip_strip_seams or uwip_strip_set_seams since the last layout and gains");
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
    if (mode == UWIP_STRIP_SEAM) {
        StripSeams q;
        q.seam = s->seam; q.orient = s->orient; q.L = std::max(s->w, s->h);
        if (gain) a.gq = s->gq;
        uwip_kscope ks(ctx, gain ? "k_strip_render_seam_gain" : "k_strip_render_seam");
        if (gain) k_strip_render<UWIP_STRIP_SEAM, true><<<grid, kRenderThreads, 0, ctx->stream>>>(a, q);
        else k_strip_render<UWIP_STRIP_SEAM><<<grid, kRenderThreads, 0, ctx->stream>>>(a, q);
        UWIP_HIP(ctx, hipGetLastError());
        return UWIP_OK;
    }
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
    s->gained = true; s->seamed = false;
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
    s->gained = true; s->seamed = false;
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

// ---- seams ----------------------------------------------------------------------------------------------------------------
UWIP_API int uwip_strip_seam_config_default(uwip_strip_seam_config *cfg)
{
    if (!cfg) return UWIP_ERR_INVALID;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->prior = 1024;
    return UWIP_OK;
}

// seam, orient and total of every frame the strip can hold, one allocation
static int seam_arrays(uwip_strip *s)
{
    if (s->seam_block) return UWIP_OK;
    const size_t N = (size_t)s->cfg.max_frames, L = (size_t)std::max(s->w, s->h);
    const size_t o_total = 0, o_seam = align256(8 * N), o_orient = o_seam + align256(4 * L * N);
    void *d = nullptr;
    if (int rc = uwip_malloc(s->ctx, o_orient + align256(4 * N), &d)) return rc;
    s->seam_block = (uint8_t *)d;
    s->total = (unsigned long long *)(s->seam_block + o_total); s->seam = (int32_t *)(s->seam_block + o_seam); s->orient = (int32_t *)(s->seam_block + o_orient);
    return UWIP_OK;
}

UWIP_API int uwip_strip_seams(uwip_strip *s, const uwip_strip_seam_config *cfg)
{
    if (!s) return UWIP_ERR_INVALID;
    uwip_ctx *ctx = s->ctx;
    if (int rc_e = uwip_enter(ctx)) return s->from_ctx(rc_e);
    if (cfg && (cfg->prior < 0 || cfg->prior > 4096)) return s->fail(UWIP_ERR_INVALID, "uwip_strip_seams: prior 0..4096");
    if (s->laid != s->count || s->count == 0) return s->fail(UWIP_ERR_INVALID, "uwip_strip_seams: call uwip_strip_layout first");
    if (std::max(s->w, s->h) > uwip_sm::kSeamMaxSide) return s->fail(UWIP_ERR_INVALID, "uwip_strip_seams: stored frames of at most 1023 x 1023");
    const size_t wh = (size_t)s->w * s->h;
    const size_t back_words = std::max((size_t)uwip_cdiv((size_t)s->w, 16) * s->h, (size_t)uwip_cdiv((size_t)s->h, 16) * s->w);   // either axis
    const bool lds_back = back_words <= (size_t)kSeamBackLdsWords;
    const size_t round = (size_t)std::min(kSeamRound, s->cfg.max_frames);
    const size_t o_back = align256(4 * wh * round), need = o_back + (lds_back ? 0 : align256(4 * back_words * round));
    if (need > s->seam_scratch_bytes) {
        void *d = nullptr;                                   // the new block first: a failure leaves the strip as it was
        if (int rc = uwip_malloc(ctx, need, &d)) return s->from_ctx(rc);
        if (s->seam_scratch) {
            if (hipError_t e = uwip_stream_wait(ctx)) { uwip_free(ctx, d); return s->from_ctx(ctx->fail(UWIP_ERR_HIP, "uwip_stream_wait", hipGetErrorString(e))); }
            uwip_free(ctx, s->seam_scratch);
        }
        s->seam_scratch = (uint8_t *)d; s->seam_scratch_bytes = need;
    }
    if (int rc = seam_arrays(s)) return s->from_ctx(rc);
    StripSeam a;
    a.store = s->store; a.fstride = wh * 3; a.w = s->w; a.h = s->h;
    a.G = s->G; a.Ginv = s->Ginv; a.seg = s->seg; a.gq = s->gained ? s->gq : nullptr;
    a.P.prior = cfg ? cfg->prior : 1024;
    a.tiles_x = (int32_t)uwip_cdiv((size_t)s->w, kTileW);
    a.cost = (uint32_t *)s->seam_scratch; a.back = lds_back ? nullptr : (uint32_t *)(s->seam_scratch + o_back); a.back_stride = back_words;
    a.orient = s->orient; a.seam = s->seam; a.L = std::max(s->w, s->h); a.total = s->total;
    s->seamed = false;
    for (int k0 = 0; k0 < s->count; k0 += (int)round) {    // a round's costs are read by its paths before the next round's are written: one stream
        const unsigned nr = (unsigned)std::min((int)round, s->count - k0);
        a.k0 = k0;
        {
            uwip_kscope ks(ctx, "k_strip_seam_cost");
            k_strip_seam_cost<<<dim3((unsigned)a.tiles_x * uwip_cdiv((size_t)s->h, kTileH), nr), kRenderThreads, 0, ctx->stream>>>(a);
            if (hipError_t e = hipGetLastError()) return s->from_ctx(ctx->fail(UWIP_ERR_HIP, "k_strip_seam_cost", hipGetErrorString(e)));
        }
        uwip_kscope ks(ctx, "k_strip_seam_path");
        if (lds_back) k_strip_seam_path<true><<<nr, kRenderThreads, 0, ctx->stream>>>(a);
        else k_strip_seam_path<false><<<nr, kRenderThreads, 0, ctx->stream>>>(a);
        if (hipError_t e = hipGetLastError()) return s->from_ctx(ctx->fail(UWIP_ERR_HIP, "k_strip_seam_path", hipGetErrorString(e)));
    }
    s->seamed = true;
    return UWIP_OK;
}

UWIP_API int uwip_strip_seam_values(uwip_strip *s, int32_t *h_seam, int32_t *h_orient, uint64_t *h_total)
{
    if (!s) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(s->ctx)) return s->from_ctx(rc_e);
    if (s->laid != s->count || !s->seamed) return s->fail(UWIP_ERR_INVALID, "uwip_strip_seam_values: no seams since the last layout and gains");
    const size_t N = (size_t)s->count, L = (size_t)std::max(s->w, s->h);
    int rc = UWIP_OK;
    if (!rc && h_seam) rc = uwip_memcpy_d2h(s->ctx, h_seam, s->seam, 4 * L * N);
    if (!rc && h_orient) rc = uwip_memcpy_d2h(s->ctx, h_orient, s->orient, 4 * N);
    if (!rc && h_total) rc = uwip_memcpy_d2h(s->ctx, h_total, s->total, 8 * N);
    if (!rc && !h_seam && !h_orient && !h_total) rc = uwip_sync(s->ctx);
    return s->from_ctx(rc);
}

UWIP_API int uwip_strip_set_seams(uwip_strip *s, const int32_t *h_seam, const int32_t *h_orient)
{
    if (!s) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(s->ctx)) return s->from_ctx(rc_e);
    if (!h_seam || !h_orient) return s->fail(UWIP_ERR_INVALID, "uwip_strip_set_seams: h_seam and h_orient");
    if (s->laid != s->count || s->count == 0) return s->fail(UWIP_ERR_INVALID, "uwip_strip_set_seams: call uwip_strip_layout first");
    const size_t N = (size_t)s->count, L = (size_t)std::max(s->w, s->h);
    std::vector<int32_t> seam(L * N, -1), orient(N, 0);
    std::vector<uint64_t> total(N, 0);
    for (const uwip_strip_segment &g : s->h_segs)
        for (int k = g.first + 1; k < g.first + g.count; ++k) {          // a segment's first frame has no seam: its entries are not read
            const int32_t o = h_orient[k];
            if (o < 0 || o > 3) return s->fail(UWIP_ERR_INVALID, "uwip_strip_set_seams: an orient outside 0..3");
            const int32_t T = uwip_sm::seam_axis(o) ? s->h : s->w, S = uwip_sm::seam_axis(o) ? s->w : s->h;
            for (int32_t t = 0; t < T; ++t) {
                const int32_t v = h_seam[L * (size_t)k + t];
                if (v < 0 || v > S) return s->fail(UWIP_ERR_INVALID, "uwip_strip_set_seams: a seam entry outside 0..states");
                seam[L * (size_t)k + t] = v;
            }
            orient[k] = o;
        }
    if (int rc = seam_arrays(s)) return s->from_ctx(rc);
    int rc = uwip_memcpy_h2d(s->ctx, s->seam, seam.data(), 4 * L * N);
    if (!rc) rc = uwip_memcpy_h2d(s->ctx, s->orient, orient.data(), 4 * N);
    if (!rc) rc = uwip_memcpy_h2d(s->ctx, s->total, total.data(), 8 * N);
    if (rc) return s->from_ctx(rc);
    s->seamed = true;
    return UWIP_OK;
}

UWIP_API int uwip_strip_seam_path_host(const uint32_t *cost, int steps, int states, int32_t *seam, uint64_t *total)
{
    if (!cost || !seam || !total || steps < 1 || states < 1 || steps > uwip_sm::kSeamMaxSide || states > uwip_sm::kSeamMaxSide) return UWIP_ERR_INVALID;
    const size_t n = (size_t)steps * states;
    for (size_t i = 0; i < n; ++i) if (cost[i] > uwip_sm::kSeamOutside) return UWIP_ERR_INVALID;
    std::vector<uint32_t> E(2 * (size_t)states);
    std::vector<uint8_t> back(n);
    *total = uwip_sm::seam_path(cost, steps, states, seam, E.data(), back.data());
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
