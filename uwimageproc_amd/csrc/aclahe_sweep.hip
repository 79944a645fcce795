// The 5 x 51 sweep of ACLAHE (aclahe.cpp:160-193) for gfx950:
//   k_clahe_sweep     a block owns interpolation cells, keeps 17 clip limits'
//                     packed LUTs and 17 output histograms in LDS, and never
//                     writes the 255 intermediate images
//   k_entropy         aclaheEntropy (aclahe.cpp:228-248) on 256-bin counts.
// The tile histograms and LUT rows come from clahe.hip's launchers (clahe_internal.hpp).
#include "clahe_internal.hpp"

int uwip_launch_hist_internal(uwip_ctx *ctx, const uwip_batch_u8 *img, uint32_t *d_hist);

namespace {

// ---- C3: the sweep, one interpolation cell (chunk) at a time ------------------
constexpr int SWEEP_GROUP = 17;    // clip limits per block (51 = 3 x 17)

struct CellItem {
    int cx, cy;       // cell indices in [0,gx] x [0,gy]
    int x0, x1;       // pixel columns [x0,x1)
    int r0, r1;       // pixel rows    [r0,r1)
    int pad0, pad1;
};

// Same-bin LDS atomics from one wave serialise, and neighbouring pixels of a smooth underwater frame land in
// few bins: the output histograms are therefore replicated SWEEP_REP times, keyed by the thread index modulo
// SWEEP_REP.  A block is 512 threads; packed LUTs (17 KB) + 3 replicas of 16-bit counters (27 KB) + the tail
// histograms (8 KB, below) = 52 KB of LDS, three blocks per CU (measured: 2 replicas x 4 blocks and 4 replicas x 2
// blocks are both slower).
constexpr int SWEEP_THREADS = 512;
constexpr int SWEEP_REP = 3;
constexpr int SWEEP_HROWS = (SWEEP_GROUP + 1) / 2;   // two clip limits share a word: 16-bit counters (a block sees < 65536 pixels)
constexpr int SWEEP_SPREAD = 8;    // multiple of SWEEP_THREADS / 64
constexpr int SWEEP_RSTRIDE = SWEEP_HROWS * 256 + 8;   // +8 words: equal bins of different replicas fall in different LDS banks
// A clip limit at or above the tallest bin of a cell's four tiles clips nothing: the 17 limits of a group therefore give
// `nd` different LUTs followed by 17 - nd repeats of the last one (clip limits grow with their index).  The repeats are
// never evaluated: the pixel's output under limit nd-1 is counted ONCE, in a tail histogram T[nd-1], and the flush adds
// T[0..c] to H[c].  (T[16] does not exist: nd = 17 has no repeats.)  One copy, 16-bit counter pairs like H.
constexpr int SWEEP_TROWS = (SWEEP_GROUP - 1) / 2;
// Whole groups of repeats are not even walked: when limit 16 (33) already clips nothing in a cell, every limit of group 1
// (2) gives the outputs of limit 0, the unclipped LUT.  The block of group 0 counts those once more in G and adds G to
// the rows of groups 1 / 2 at flush time; the blocks of groups 1 / 2 skip the cell.  G lives in the one counter slot H
// leaves free (the high half of row 8: 17 limits in 18 slots): replica 0 for cells where groups 1 and 2 repeat, replica 1
// for cells where only group 2 does.
constexpr size_t SWEEP_LDS_WORDS = (size_t)SWEEP_GROUP * 256 + (size_t)SWEEP_REP * SWEEP_RSTRIDE + (size_t)SWEEP_TROWS * 256;
static_assert(SWEEP_REP >= 2 && (SWEEP_GROUP & 1) == 1 && SWEEP_LDS_WORDS * 4 + 128 <= 54528, "three blocks per CU (tools/ubench/lds_occ.hip: 54528 B is the most LDS a block of three may hold)");
// clahe_blend -> RNE, clamped byte; pk = TL | TR << 8 | BL << 16 | BR << 24
__device__ __forceinline__ uint32_t sweep_eval(uint32_t pk, float xa1, float xa, float ya1, float ya)
{
    const float res = clahe_blend(pk & 255u, (pk >> 8) & 255u, (pk >> 16) & 255u, pk >> 24, xa1, xa, ya1, ya);
    return __builtin_amdgcn_cvt_pk_u8_f32(res, 0, 0u);     // RNE + clamp
}

// s_pack by grey level: limits 0 .. 15 of the group as [256 grey][4 quads][4 limits] dwords (64 B per grey level, one
// ds_read_b128 per quad of limits), limit 16 in a [256] row of its own behind them (read only where nd == 17).
// A ds_read_b128 is served in 16 slots of 16 B per 256-B row; unswizzled, quad q of grey v sits in slot (4v + q) mod 16, which
// depends on v mod 4 only.  Quad q of grey v is therefore stored at quad position q ^ ((v >> 2) & 3): the slot depends on
// v mod 16.  sweep_quad0(v) ^ q is the uint4 index of quad q (the pack stage and the reads both use it).
constexpr int SWEEP_QUADS = (SWEEP_GROUP - 1) / 4;
constexpr int SWEEP_ROW16 = SWEEP_QUADS * 4 * 256;          // dword offset of limit 16's row
static_assert(SWEEP_GROUP == 4 * SWEEP_QUADS + 1 && (SWEEP_QUADS + 1) * 64 <= SWEEP_THREADS, "four quads and one row; one pack task per thread");
__device__ __forceinline__ uint32_t sweep_quad0(uint32_t v) { return v * 4u + ((v >> 2) & 3u); }

// clip limits 0 .. N-1 of one pixel from their packed tuples: the evaluations interleave
template <int N>
__device__ __forceinline__ void sweep_run(const uint32_t *pk, uint32_t *my_hist, float xa1, float xa, float ya1, float ya)
{
    // Limits 2j and 2j + 1 share a counter word (low / high half).  Where a pixel's two outputs agree -- neighbouring limits
    // often blend the same four LUT entries -- ONE atomic adds to both halves, and the second one runs only for the lanes that
    // differ (fewer active lanes = fewer same-bank collisions in the LDS pipe, the kernel's other limit).
    uint32_t o[N > 0 ? N : 1];
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = sweep_eval(pk[i], xa1, xa, ya1, ya);
#pragma unroll
    for (int i = 0; i + 1 < N; i += 2) {
        const bool same = o[i] == o[i + 1];
        atomicAdd(&my_hist[(i >> 1) * 256 + o[i]], same ? 0x10001u : 1u);
        if (!same) atomicAdd(&my_hist[(i >> 1) * 256 + o[i + 1]], 65536u);
    }
    if constexpr ((N & 1) != 0) atomicAdd(&my_hist[((N - 1) >> 1) * 256 + o[N - 1]], 1u);
}

// one pixel of a cell with ns = 4 NQ + R < 16: quads 0 .. NQ go out together, limits 0 .. ns-1 are counted in H and limit ns
// (position R of quad NQ) in the tail
template <int NQ, int R>
__device__ __forceinline__ void sweep_pixel(const uint4 *pack4, uint32_t q0, uint32_t *my_hist, uint32_t *s_tail, uint32_t *s_g, bool g_sep,
                                            bool g_last, float xa1, float xa, float ya1, float ya)
{
    constexpr int NS = 4 * NQ + R;
    uint32_t pk[4 * (NQ + 1)];
#pragma unroll
    for (int i = 0; i <= NQ; ++i) {
        const uint4 q = pack4[q0 ^ (uint32_t)i];
        pk[4 * i] = q.x; pk[4 * i + 1] = q.y; pk[4 * i + 2] = q.z; pk[4 * i + 3] = q.w;
    }
    if (g_sep) atomicAdd(&s_g[sweep_eval(pk[0], xa1, xa, ya1, ya)], 65536u);
    sweep_run<NS>(pk, my_hist, xa1, xa, ya1, ya);
    const uint32_t o_last = sweep_eval(pk[NS], xa1, xa, ya1, ya);
    atomicAdd(&s_tail[(NS >> 1) * 256 + o_last], (NS & 1) ? 65536u : 1u);
    if (g_last) atomicAdd(&s_g[o_last], 65536u);
}

__global__ __launch_bounds__(SWEEP_THREADS) void k_clahe_sweep(const uint8_t *__restrict__ src, size_t step,
                                                     size_t fstride, int gx, int gy, float inv_tw,
                                                     float inv_th,
                                                     const uint8_t *__restrict__ luts /*[F][tiles][51][256]*/,
                                                     const CellItem *__restrict__ items, int nitems,
                                                     int items_per_block,
                                                     uint32_t *__restrict__ out_hist /*[F][51][256]*/,
                                                     size_t out_fs, const uint32_t *__restrict__ tile_max /*[F][tiles]*/,
                                                     ClipList cl)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_sweep[];
    uint32_t *s_pack = s_sweep;                                   // [256][SWEEP_QUADS][4] swizzled + [256] for limit 16 (sweep_quad0)
    uint32_t *s_hist = s_sweep + SWEEP_GROUP * 256;               // [SWEEP_REP][SWEEP_HROWS][256], two 16-bit counters per word
    uint32_t *s_tail = s_hist + SWEEP_REP * SWEEP_RSTRIDE;        // [SWEEP_TROWS][256], same packing
    const int tid = threadIdx.x;
    const int cg = blockIdx.y, f = blockIdx.z;
    const int clip_g1 = cl.clip[SWEEP_GROUP - 1], clip_g2 = cl.clip[2 * SWEEP_GROUP - 1];
    const int tiles = gx * gy;
    const uint32_t *tmax = tile_max + (size_t)f * tiles;
    const int i0 = blockIdx.x * items_per_block, i1 = min(nitems, i0 + items_per_block);
    if (cg != 0) {
        // nothing to do when every cell of this block repeats limit 0 throughout the group (block-uniform)
        const uint32_t clip_prev = (uint32_t)(cg == 1 ? clip_g1 : clip_g2);
        bool any = false;
        for (int it = i0; it < i1; ++it) {
            const CellItem ci = items[it];
            const int tx1 = max(ci.cx - 1, 0), tx2 = min(ci.cx, gx - 1), ty1 = max(ci.cy - 1, 0), ty2 = min(ci.cy, gy - 1);
            any = any || clip_prev < max(max(tmax[ty1 * gx + tx1], tmax[ty1 * gx + tx2]), max(tmax[ty2 * gx + tx1], tmax[ty2 * gx + tx2]));
        }
        if (!any) return;
    }
    for (int i = tid; i < SWEEP_REP * SWEEP_RSTRIDE + SWEEP_TROWS * 256; i += SWEEP_THREADS) s_hist[i] = 0;
    uint32_t *my_hist = s_hist + (tid % SWEEP_REP) * SWEEP_RSTRIDE;
    const uint8_t *fb = src + (size_t)f * fstride;
    const uint8_t *L = luts + ((size_t)f * tiles * SWEEP_NCL + (size_t)cg * SWEEP_GROUP) * 256;      // + (tile * 51 + c) * 256
    for (int it = i0; it < i1; ++it) {
        const CellItem ci = items[it];
        const int tx1 = max(ci.cx - 1, 0), tx2 = min(ci.cx, gx - 1);
        const int ty1 = max(ci.cy - 1, 0), ty2 = min(ci.cy, gy - 1);
        const uint32_t cellmax = max(max(tmax[ty1 * gx + tx1], tmax[ty1 * gx + tx2]), max(tmax[ty2 * gx + tx1], tmax[ty2 * gx + tx2]));
        const bool rep1 = (uint32_t)clip_g1 >= cellmax, rep2 = (uint32_t)clip_g2 >= cellmax;   // rep1 implies rep2
        if ((cg == 1 && rep1) || (cg == 2 && rep2)) continue;            // counted by the block of group 0 (block-uniform)
        const bool g_any = cg == 0 && rep2, g_both = cg == 0 && rep1;
        uint32_t *s_g = s_hist + (g_both ? 0 : SWEEP_RSTRIDE) + (SWEEP_HROWS - 1) * 256;
        __syncthreads();
        // nd = how many of the group's 17 limits have LUTs of their own in this cell: limit c repeats limit c-1 once
        // limit c-1 is at or above the tallest bin of the four tiles (both are then the unclipped LUT), and the limits
        // grow with c, so the distinct ones come first.  (Block-uniform; small tiles, where two limits that still clip
        // round to one integer, evaluate such a pair twice: harmless.)
        int nd = 1;
        for (int c = 1; c < SWEEP_GROUP; ++c) nd += (uint32_t)cl.clip[cg * SWEEP_GROUP + c - 1] < cellmax ? 1 : 0;
        const int ns = nd - 1;                                     // limits 0 .. ns-1 go to H, limit ns to T[ns]
        // A thread takes four grey levels of one quad of limits (wave w: quad w; wave 4: limit 16 where nd == 17): per limit one
        // dword from each of the four tiles' LUTs, byte-transposed by v_perm into four packed entries
        // (TL | TR << 8 | BL << 16 | BR << 24), then one 16-byte LDS write per grey level.  Quads >= ceil(nd / 4) are never read.
        {
            const int qd = tid >> 6, v4 = tid & 63;
            const int nq = min((nd + 3) >> 2, SWEEP_QUADS);
            const bool row16 = qd == SWEEP_QUADS && nd == SWEEP_GROUP;
            if (qd < nq || row16) {
                uint32_t e[4][4] = {};                                   // [grey 4 v4 + k][limit 4 qd + j]
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j > 0 && row16) break;
                    const uint32_t *Lc = reinterpret_cast<const uint32_t *>(L + (size_t)(qd * 4 + j) * 256);
                    const uint32_t a = Lc[((size_t)ty1 * gx + tx1) * (SWEEP_NCL * 64) + v4];
                    const uint32_t b = Lc[((size_t)ty1 * gx + tx2) * (SWEEP_NCL * 64) + v4];
                    const uint32_t cc = Lc[((size_t)ty2 * gx + tx1) * (SWEEP_NCL * 64) + v4];
                    const uint32_t d = Lc[((size_t)ty2 * gx + tx2) * (SWEEP_NCL * 64) + v4];
                    const uint32_t t0 = __builtin_amdgcn_perm(b, a, 0x05010400u), t1 = __builtin_amdgcn_perm(b, a, 0x07030602u);
                    const uint32_t u0 = __builtin_amdgcn_perm(d, cc, 0x05010400u), u1 = __builtin_amdgcn_perm(d, cc, 0x07030602u);
                    e[0][j] = __builtin_amdgcn_perm(u0, t0, 0x05040100u); e[1][j] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
                    e[2][j] = __builtin_amdgcn_perm(u1, t1, 0x05040100u); e[3][j] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
                }
                if (row16) {
                    reinterpret_cast<uint4 *>(s_pack + SWEEP_ROW16)[v4] = make_uint4(e[0][0], e[1][0], e[2][0], e[3][0]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        reinterpret_cast<uint4 *>(s_pack)[sweep_quad0((uint32_t)(4 * v4 + k)) ^ (uint32_t)qd] = make_uint4(e[k][0], e[k][1], e[k][2], e[k][3]);
                }
            }
        }
        __syncthreads();
        // with rep1 the last distinct limit is the unclipped LUT itself: its output is reused for G
        const bool g_last = g_both && nd < SWEEP_GROUP;
        const bool g_sep = g_any && !g_last;
        const int w = ci.x1 - ci.x0;
        const int npix = w * (ci.r1 - ci.r0);
        const float inv_w = 1.0f / (float)w;
        // pixel p of the cell -> (x, y); the byte for the NEXT iteration is requested before this one's 17
        // evaluations so its latency hides behind them
        // (p < 2^16, w < 2^16, rows * step < 2^31: 24-bit multiplies and a 32-bit byte offset are exact and full rate,
        // where the 32 x 32 and 64-bit forms are quarter rate)
        auto locate = [&](int p, int &x, int &y) {
            int q = (int)(((float)p + 0.5f) * inv_w);
            int r = p - (int)__umul24((unsigned)q, (unsigned)w);
            if (r < 0) { q--; r += w; }
            if (r >= w) { q++; r -= w; }
            x = ci.x0 + r; y = ci.r0 + q;
        };
        const uint32_t step24 = (uint32_t)step;
        auto pix_at = [&](int x, int y) { return (uint32_t)fb[__umul24((unsigned)y, step24) + (unsigned)x]; };
        int xn = 0, yn = 0;
        uint32_t vnext = 0;
        // The 64 pixels of one LDS-atomic instruction are SWEEP_SPREAD apart (lane i of wave w takes pixel
        // SWEEP_SPREAD*i + w + 8m of every 64*SWEEP_SPREAD), so fewer of them fall into the same output bin than 64
        // neighbours of a smooth frame would.
        constexpr int MS = SWEEP_SPREAD / (SWEEP_THREADS / 64);
        auto pix_of = [&](int t) { return (t / MS) * (64 * SWEEP_SPREAD) + (tid & 63) * SWEEP_SPREAD + (tid >> 6) + (SWEEP_THREADS / 64) * (t % MS); };
        static_assert(MS == 1, "consecutive pixels of a thread are SWEEP_THREADS apart");
        // Whole groups of SWEEP_THREADS pixels go by the spread mapping (a permutation of the group); the remainder of the
        // cell (npix mod 512 pixels) is taken contiguously, one pixel per thread from thread 0 on, so that only
        // ceil(rem / 64) waves run the last round instead of all eight with a few lanes each (a 61 x 34 cell of the 32 x 32
        // grid has 4 whole groups + 26 pixels: 5 rounds for every wave became 4 + one wave's).
        const int nfull = npix / SWEEP_THREADS, rem = npix - nfull * SWEEP_THREADS;
        const int ntot = nfull + (tid < rem ? 1 : 0);
        int t = 0;
        if (ntot > 0) { locate(nfull > 0 ? pix_of(0) : tid, xn, yn); vnext = pix_at(xn, yn); }
        // a thread's next pixel is SWEEP_THREADS further along the cell: step (x, y) instead of dividing again
        const int dq = SWEEP_THREADS / w, dr = SWEEP_THREADS - dq * w;     // wave-uniform
        for (; t < ntot;) {
            const int x = xn, y = yn;
            const uint32_t v = vnext;
            ++t;
            if (t < ntot) {
                if (t < nfull) {
                    xn += dr; yn += dq;
                    if (xn >= ci.x1) { xn -= w; yn++; }
                } else {
                    locate(nfull * SWEEP_THREADS + tid, xn, yn);          // the remainder pixel
                }
                vnext = pix_at(xn, yn);
            }
            const float txf = (float)x * inv_tw - 0.5f;
            const float xa = txf - floorf(txf), xa1 = 1.0f - xa;
            const float tyf = (float)y * inv_th - 0.5f;
            const float ya = tyf - floorf(tyf), ya1 = 1.0f - ya;
            const uint4 *pack4 = reinterpret_cast<const uint4 *>(s_pack);
            const uint32_t q0 = sweep_quad0(v);
            if (nd == SWEEP_GROUP) {
                // every clip limit has its own LUTs: four quads and limit 16's row, all into H
                uint32_t pk[SWEEP_GROUP];
                pk[SWEEP_GROUP - 1] = s_pack[SWEEP_ROW16 + v];
#pragma unroll
                for (int i = 0; i < SWEEP_QUADS; ++i) {
                    const uint4 q = pack4[q0 ^ (uint32_t)i];
                    pk[4 * i] = q.x; pk[4 * i + 1] = q.y; pk[4 * i + 2] = q.z; pk[4 * i + 3] = q.w;
                }
                if (g_sep) atomicAdd(&s_g[sweep_eval(pk[0], xa1, xa, ya1, ya)], 65536u);
                sweep_run<SWEEP_GROUP>(pk, my_hist, xa1, xa, ya1, ya);
                continue;
            }
            // ns < 16 (block-uniform): straight-line code per number of quads and position of the last distinct limit
#define SWEEP_PIXEL(NQ, R) sweep_pixel<NQ, R>(pack4, q0, my_hist, s_tail, s_g, g_sep, g_last, xa1, xa, ya1, ya); break
            switch (ns) {
            case 0: SWEEP_PIXEL(0, 0);
            case 1: SWEEP_PIXEL(0, 1);
            case 2: SWEEP_PIXEL(0, 2);
            case 3: SWEEP_PIXEL(0, 3);
            case 4: SWEEP_PIXEL(1, 0);
            case 5: SWEEP_PIXEL(1, 1);
            case 6: SWEEP_PIXEL(1, 2);
            case 7: SWEEP_PIXEL(1, 3);
            case 8: SWEEP_PIXEL(2, 0);
            case 9: SWEEP_PIXEL(2, 1);
            case 10: SWEEP_PIXEL(2, 2);
            case 11: SWEEP_PIXEL(2, 3);
            case 12: SWEEP_PIXEL(3, 0);
            case 13: SWEEP_PIXEL(3, 1);
            case 14: SWEEP_PIXEL(3, 2);
            default: SWEEP_PIXEL(3, 3);
            }
#undef SWEEP_PIXEL
        }
    }
    __syncthreads();
    uint32_t *out = out_hist + (size_t)f * out_fs + (size_t)cg * SWEEP_GROUP * 256;
    // H[c] + T[0] + ... + T[min(c, 15)], one thread per grey level walking up the clip limits
    if (tid < 256) {
        uint32_t run = 0;
#pragma unroll
        for (int c = 0; c < SWEEP_GROUP; ++c) {
            const int sh = (c & 1) * 16;
            if (c < SWEEP_GROUP - 1) run += (s_tail[(c >> 1) * 256 + tid] >> sh) & 0xffffu;
            uint32_t sum = run;
#pragma unroll
            for (int r = 0; r < SWEEP_REP; ++r) sum += (s_hist[r * SWEEP_RSTRIDE + (c >> 1) * 256 + tid] >> sh) & 0xffffu;
            if (sum) atomicAdd(&out[c * 256 + tid], sum);
        }
        if (cg == 0) {
            const uint32_t g1 = s_hist[(SWEEP_HROWS - 1) * 256 + tid] >> 16;
            const uint32_t g2 = g1 + (s_hist[SWEEP_RSTRIDE + (SWEEP_HROWS - 1) * 256 + tid] >> 16);
            if (g1) for (int c = SWEEP_GROUP; c < 2 * SWEEP_GROUP; ++c) atomicAdd(&out[c * 256 + tid], g1);
            if (g2) for (int c = 2 * SWEEP_GROUP; c < 3 * SWEEP_GROUP; ++c) atomicAdd(&out[c * 256 + tid], g2);
        }
    }
}

// ---- C2: entropy of 256-bin counts ---------------------------------------------
__global__ __launch_bounds__(256) void k_entropy(const uint32_t *__restrict__ hist, int rows,
                                                 int cols, float *__restrict__ out)
{
    __shared__ double s_term[256];
    const int v = threadIdx.x;
    const size_t h = blockIdx.x;
    s_term[v] = entropy_term(hist[h * 256 + v], rows, cols);
    __syncthreads();
    if (v == 0) {
        float e = 0.0f;
        for (int i = 0; i < 256; ++i) e = (float)((double)e + s_term[i]);
        out[h] = -e;
    }
}

}  // namespace

UWIP_API int uwip_entropy(uwip_ctx *ctx, const uwip_batch_u8 *src, float *d_entropy)
{
    int rc = uwip_check_batch(ctx, src, 1);
    if (rc) return rc;
    if (src->frames == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, d_entropy != nullptr, "null output");
    UWIP_REQUIRE(ctx, !uwip_batch_empty(src), "entropy of an empty image");
    uint32_t *d_hist = (uint32_t *)uwip_ws(ctx, "entropy.hist", sizeof(uint32_t) * 256 * (size_t)src->frames);
    if (!d_hist) return UWIP_ERR_NOMEM;
    rc = uwip_launch_hist_internal(ctx, src, d_hist);
    if (rc) return rc;
    uwip_kscope ks(ctx, "k_entropy");
    k_entropy<<<src->frames, 256, 0, ctx->stream>>>(d_hist, src->rows, src->cols, d_entropy);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

UWIP_API int uwip_aclahe_sweep_hist(uwip_ctx *ctx, const uwip_batch_u8 *src, int residual_rule, float *d_entropy, uint32_t *d_hist_tap)
{
    int rc = uwip_check_batch(ctx, src, 1);
    if (rc) return rc;
    if (src->frames == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, d_entropy != nullptr, "null output");
    UWIP_REQUIRE(ctx, !uwip_batch_empty(src), "sweep of an empty image");
    UWIP_REQUIRE(ctx, src->frames <= 65535, "too many frames for one launch");
    // k_clahe_sweep counts in 16-bit LDS counters: a block must see < 65536 pixels, and its smallest work item is one
    // row of an interpolation cell (at most a tile wide)
    UWIP_REQUIRE(ctx, src->cols <= 65535, "image too wide for the sweep");
    // ... and addresses a pixel of a frame by a 32-bit byte offset formed with a 24-bit multiply
    UWIP_REQUIRE(ctx, src->step < (1u << 24) && (uint64_t)src->rows * src->step < (1ull << 32), "frame too large for the sweep");
    const int F = src->frames;
    const size_t out_fs = (size_t)5 * SWEEP_NCL * 256;
    uint32_t *d_out = (uint32_t *)uwip_ws(ctx, "sweep.outhist", sizeof(uint32_t) * out_fs * F);
    uint32_t *hbuf[2] = {(uint32_t *)uwip_ws(ctx, "clahe.tilehist", sizeof(uint32_t) * 256 * (size_t)CLAHE_MAX_TILES * F),
                         (uint32_t *)uwip_ws(ctx, "clahe.tilehist2", sizeof(uint32_t) * 256 * (size_t)CLAHE_MAX_TILES * F)};
    uint8_t *d_luts = (uint8_t *)uwip_ws(ctx, "sweep.luts", SWEEP_LUTS_FRAME_BYTES * F);
    uint32_t *d_tmax = (uint32_t *)uwip_ws(ctx, "sweep.tilemax", sizeof(uint32_t) * (size_t)CLAHE_MAX_TILES * F);
    if (!d_out || !hbuf[0] || !hbuf[1] || !d_luts || !d_tmax) return UWIP_ERR_NOMEM;
    UWIP_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(uint32_t) * out_fs * F, ctx->stream));
    // finest grid first: a coarser unpadded grid sums the tile histograms of the grid twice as fine
    ClaheGeom finer{};
    bool finer_has_hists = false;
    for (int gi = ACLAHE_NBS - 1; gi >= 0; --gi) {
        const int gsz = ACLAHE_BS[gi];
        const ClaheGeom g = make_geom(src->rows, src->cols, gsz, gsz);
        uint32_t *d_hists = hbuf[gi & 1];
        const bool nested = gi < ACLAHE_NBS - 1 && finer.gx == 2 * g.gx && finer.gy == 2 * g.gy && finer.pc == finer.cols && finer.pr == finer.rows &&
                            g.pc == g.cols && g.pr == g.rows && finer.tw * 2 == g.tw && finer.th * 2 == g.th;
        ClipList cl{};
        cl.n = 0;
        for (float c = 0.0f; c <= 25.0f; c += 0.5f) cl.clip[cl.n++] = clip_from_limit((double)c, g.area);
        if (nested && finer_has_hists) {
            rc = uwip_clahe_launch_tilehist_merge(ctx, hbuf[(gi + 1) & 1], g, F, d_hists);
            if (rc) return rc;
            finer_has_hists = true;
        } else if (uwip_clahe_band_ok(src, g)) {
            // histograms and the 51 LUT rows of every tile in one launch; the histograms stay in LDS
            rc = uwip_clahe_launch_band(ctx, src, g, nullptr, F, cl.clip, cl.n, nullptr, residual_rule, d_luts, d_tmax);
            if (rc) return rc;
            finer_has_hists = false;
        } else {
            rc = uwip_clahe_launch_tilehist(ctx, src, g, nullptr, F, d_hists);
            if (rc) return rc;
            finer_has_hists = true;
        }
        finer = g;
        if (finer_has_hists) {
            rc = uwip_clahe_launch_lut(ctx, g, d_hists, cl.clip, cl.n, nullptr, F, residual_rule, d_luts, d_tmax);
            if (rc) return rc;
        }
        // work items: interpolation cells cut into row chunks of <= ~16K pixels (cached per geometry)
        char key[96];
        snprintf(key, sizeof key, "cells:%d:%d:%d", g.rows, g.cols, gsz);
        size_t bytes = 0;
        const void *d_tab = uwip_table_find(ctx, key, &bytes);
        if (!d_tab) {
            std::vector<int> xs, ys;
            cell_starts(g.cols, g.gx, g.inv_tw, xs);
            cell_starts(g.rows, g.gy, g.inv_th, ys);
            std::vector<CellItem> items;
            for (int cy = 0; cy <= g.gy; ++cy) {
                for (int cx = 0; cx <= g.gx; ++cx) {
                    const int w = xs[cx + 1] - xs[cx], h = ys[cy + 1] - ys[cy];
                    if (w <= 0 || h <= 0) continue;
                    const int rows_per = std::max(1, 16384 / w);
                    for (int r = ys[cy]; r < ys[cy + 1]; r += rows_per) {
                        CellItem ci{};
                        ci.cx = cx; ci.cy = cy; ci.x0 = xs[cx]; ci.x1 = xs[cx + 1];
                        ci.r0 = r; ci.r1 = std::min(r + rows_per, ys[cy + 1]);
                        items.push_back(ci);
                    }
                }
            }
            bytes = items.size() * sizeof(CellItem);
            d_tab = uwip_table_put(ctx, key, items.data(), bytes);
            if (!d_tab) return UWIP_ERR_NOMEM;
        }
        const CellItem *d_items = (const CellItem *)d_tab;
        const int nitems = (int)(bytes / sizeof(CellItem));
        const int cell_px = std::max(1, g.tw * g.th);
        const int ipb = std::max(1, std::min(32, 32768 / cell_px));   // <= 32768 pixels per block: the 16-bit LDS counters cannot overflow
        dim3 grid(uwip_cdiv(nitems, ipb), SWEEP_NCL / SWEEP_GROUP, (unsigned)F);
        uwip_kscope ks(ctx, "k_clahe_sweep");
        const size_t sweep_lds = sizeof(uint32_t) * SWEEP_LDS_WORDS;
        rc = uwip_lds_optin(ctx, "k_clahe_sweep", (const void *)k_clahe_sweep, sweep_lds);
        if (rc) return rc;
        k_clahe_sweep<<<grid, SWEEP_THREADS, sweep_lds, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, g.gx,
                                                     g.gy, g.inv_tw, g.inv_th, d_luts, d_items, nitems, ipb,
                                                     d_out + (size_t)gi * SWEEP_NCL * 256, out_fs, d_tmax, cl);
        UWIP_HIP(ctx, hipGetLastError());
    }
    {
        uwip_kscope ks(ctx, "k_entropy");
        k_entropy<<<F * 5 * SWEEP_NCL, 256, 0, ctx->stream>>>(d_out, src->rows, src->cols, d_entropy);
        UWIP_HIP(ctx, hipGetLastError());
    }
    if (d_hist_tap) UWIP_HIP(ctx, hipMemcpyAsync(d_hist_tap, d_out, sizeof(uint32_t) * out_fs * F, hipMemcpyDeviceToDevice, ctx->stream));
    return UWIP_OK;
}

UWIP_API int uwip_aclahe_sweep(uwip_ctx *ctx, const uwip_batch_u8 *src, int residual_rule, float *d_entropy)
{
    return uwip_aclahe_sweep_hist(ctx, src, residual_rule, d_entropy, nullptr);
}
