// What the units of the CLAHE / ACLAHE path share (clahe.hip, aclahe_sweep.hip, aclahe_auto.hip): the tile geometry, the clip
// list, the block sizes ACLAHE searches, the arithmetic that must read the same wherever it is evaluated (clip limit ->
// integer clip, the LUT rows of a tile, cv::CLAHE's bilinear blend, the entropy term), the interpolation's per-frame
// descriptor, the workspace sizes two units must agree on and the launchers that cross a unit boundary.
// All float32 arithmetic keeps OpenCV's operation order (every unit is compiled with -ffp-contract=off).
#pragma once
#include "uwip_internal.hpp"
#include "device_utils.hpp"
#include <algorithm>
#include <cmath>

// host-side geometry and launch shape: plain types, they appear in the signatures of the launchers below
struct ClaheGeom {
    int rows, cols, gx, gy, tw, th, pc, pr, area;
    float inv_tw, inv_th, lutScale;
};

// launch shape of the interpolation for one geometry: column parts per strip, threads along x, rows per strip and the
// cells (KB of LDS) a block can touch
struct ApplyShape { int xs, TX, max_rows, lds_cells; };

namespace {      // internal linkage on purpose: kernels take ClipList and ApplyFrame, and every unit keeps the same kernel names

inline ClaheGeom make_geom(int rows, int cols, int gx, int gy)
{
    ClaheGeom g{};
    g.rows = rows; g.cols = cols; g.gx = gx; g.gy = gy;
    g.pc = cols; g.pr = rows;
    if (!(cols % gx == 0 && rows % gy == 0)) {      // both pads, as cv::CLAHE does
        g.pr = rows + (gy - (rows % gy));
        g.pc = cols + (gx - (cols % gx));
    }
    g.tw = g.pc / gx; g.th = g.pr / gy;
    g.area = g.tw * g.th;
    g.inv_tw = 1.0f / (float)g.tw;
    g.inv_th = 1.0f / (float)g.th;
    g.lutScale = (float)255 / (float)g.area;
    return g;
}

// cv::CLAHE's integer clip of a tile of `area` pixels (0: no clipping), on the host and in the kernels that derive it
// from device-side parameters
__host__ __device__ inline int clip_from_limit(double clipLimit, int area)
{
    int clip = 0;
    if (clipLimit > 0.0) {
        clip = (int)(clipLimit * area / 256);
        clip = clip > 1 ? clip : 1;
    }
    return clip;
}

// first coordinate p in [0, n] whose cell index floor(p*inv - 0.5f) + 1 is >= c
// (cell index is non-decreasing in p).  Same float32 expression as the kernels.
inline int cell_of(int p, float inv) { return (int)floorf((float)p * inv - 0.5f) + 1; }

inline void cell_starts(int n, int g, float inv, std::vector<int> &starts)
{
    starts.assign(g + 2, n);
    int p = 0;
    for (int c = 0; c <= g; ++c) {
        while (p < n && cell_of(p, inv) < c) ++p;
        starts[c] = p;
    }
    starts[g + 1] = n;
    // cells beyond the last occupied one are empty: starts stay at n
    for (int c = g; c >= 0; --c) starts[c] = std::min(starts[c], starts[c + 1]);
}

// the integer clips of one launch, a kernel parameter (n = 1: one clip, or per-frame clips read from device memory)
struct ClipList {
    int n;
    int clip[51];
};

// the grid sizes ACLAHE searches (aclahe.cpp:161); group k of the per-frame launches = block size ACLAHE_BS[k]
constexpr int ACLAHE_NBS = 5;
constexpr int ACLAHE_BS[ACLAHE_NBS] = {2, 4, 8, 16, 32};
constexpr int CLAHE_MAX_TILES = 32 * 32;      // the finest of them: what the per-grid workspaces are sized for
constexpr int SWEEP_NCL = 51;                 // clip limits 0, 0.5, ..., 25  (aclahe.cpp:181)
// tiles of the grids 2, 4, 8, 16, 32 one after the other: offsets 0, 4, 20, 84, 340 = (4^(k+1) - 4) / 3, 1364 per frame
constexpr int EXACT_TILES = 1364;
constexpr int exact_tile_off(int k) { return ((4 << (2 * k)) - 4) / 3; }
constexpr bool exact_tiles_match_list()
{
    int off = 0;
    for (int k = 0; k < ACLAHE_NBS; ++k) {
        if (exact_tile_off(k) != off) return false;
        off += ACLAHE_BS[k] * ACLAHE_BS[k];
    }
    return off == EXACT_TILES && ACLAHE_BS[ACLAHE_NBS - 1] * ACLAHE_BS[ACLAHE_NBS - 1] == CLAHE_MAX_TILES;
}
static_assert(exact_tiles_match_list(), "exact_tile_off / EXACT_TILES / CLAHE_MAX_TILES follow ACLAHE_BS");
// workspace "sweep.luts", per frame: the sweep's [tiles][51][256] LUT rows of one grid; the exact block-size search borrows
// it for its [EXACT_TILES][256] rows of all five
constexpr size_t SWEEP_LUTS_FRAME_BYTES = (size_t)256 * CLAHE_MAX_TILES * SWEEP_NCL;
constexpr size_t EXACT_LUTS_FRAME_BYTES = (size_t)256 * EXACT_TILES;
static_assert(EXACT_LUTS_FRAME_BYTES <= SWEEP_LUTS_FRAME_BYTES, "the exact search's LUT rows fit the sweep's workspace");

// (TL*xa1 + TR*xa)*ya1 + (BL*xa1 + BR*xa)*ya: cv::CLAHE's blend of the four neighbouring tiles' LUT values -- OpenCV's four
// products, three sums and order (no FMA: -ffp-contract=off); the caller rounds to nearest even and clamps (v_cvt_pk_u8_f32).
// Plain f32 operations: on gfx950 a v_pk_mul/add_f32 costs 2.6x a v_mul/add_f32 (tools/ubench/valu_rate.hip: 2.97 vs
// 1.14 ns per wave-instruction), so the two-rows-per-packed-pair form lost.
__device__ __forceinline__ float clahe_blend(uint32_t TL, uint32_t TR, uint32_t BL, uint32_t BR, float xa1, float xa, float ya1, float ya)
{
    const float top = (float)TL * xa1 + (float)TR * xa;
    const float bot = (float)BL * xa1 + (float)BR * xa;
    return top * ya1 + bot * ya;
}

// one term of aclaheEntropy (aclahe.cpp:241-247): p * log2(p + 0.00001), p = count / pixels in float32, the product in
// float64; the caller accumulates serially, e = (float)((double)e + term)
__device__ __forceinline__ double entropy_term(uint32_t count, int rows, int cols)
{
    const float p = (float)count / (float)(cols * rows);
    return (double)p * log2((double)p + 0.00001);
}

// residual -> stepr | magic << 9 (clahe_lut_rows); header-local: every unit that inlines clahe_lut_rows keeps its own copy
struct SteprTab { uint32_t v[256]; };
constexpr SteprTab make_stepr_tab()
{
    SteprTab t{};
    for (int r = 0; r < 256; ++r) {
        const uint32_t stepr = r ? (256u / (uint32_t)r > 1u ? 256u / (uint32_t)r : 1u) : 1u;
        t.v[r] = stepr | ((65536u / stepr + 1u) << 9);
    }
    return t;
}
static __device__ const SteprTab D_STEPR = make_stepr_tab();

// ---- C1b: clip, redistribute, cumulative LUT --------------------------------
// One wave per (tile, frame); lane l owns bins 4l..4l+3 and the wave walks all clip limits with shuffle-only
// reductions and scans (no barriers).  Arithmetic is cv::CLAHE's: integer clip / redistribute, then
// lut = sat_u8(rne(float(cumsum) * lutScale)).
// the wave-level body: h0 = this lane's four bins of the tile's histogram; writes the tile's ncl LUT rows (256 B each, lane l
// the bytes 4l .. 4l+3) from `out` on and, optionally, the tallest bin
__device__ __forceinline__ void clahe_lut_rows(const int (&h0)[4], int lane, float lutScale, const ClipList &cl, int frame_clip /*< 0: none*/,
                                               int rule, uint8_t *__restrict__ out, uint32_t *__restrict__ tile_max_out)
{
    const int ncl = cl.n;
    // the tile's tallest bin: a clip limit at or above it clips nothing (cv::CLAHE clips bins > limit only), so its LUT is
    // the unclipped one -- computed once here, and k_clahe_sweep never evaluates such limits
    int m = max(max(h0[0], h0[1]), max(h0[2], h0[3]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d));
    if (tile_max_out && lane == 0) *tile_max_out = (uint32_t)m;
    auto lut_word = [&](const int h[4]) {
        const int p0 = h[0], p1 = p0 + h[1], p2 = p1 + h[2], p3 = p2 + h[3];
        const int off = (int)wave_incl_scan_u32((uint32_t)p3) - p3;
        // sum * lutScale lies in [0, 255.0001]: v_cvt_pk_u8_f32 (round to nearest even, clamp, byte insert) is sat_u8_rne there
        uint32_t wv = __builtin_amdgcn_cvt_pk_u8_f32((float)(off + p0) * lutScale, 0, 0u);
        wv = __builtin_amdgcn_cvt_pk_u8_f32((float)(off + p1) * lutScale, 1, wv);
        wv = __builtin_amdgcn_cvt_pk_u8_f32((float)(off + p2) * lutScale, 2, wv);
        return __builtin_amdgcn_cvt_pk_u8_f32((float)(off + p3) * lutScale, 3, wv);
    };
    uint32_t w_unclipped = 0;
    bool have_unclipped = false;                 // computed when the first limit that clips nothing asks for it
    for (int c = 0; c < ncl; ++c) {
        const int clip = frame_clip >= 0 ? frame_clip : cl.clip[c];
        uint32_t w;
        if (!(clip > 0 && clip < m)) {                                 // wave-uniform
            if (!have_unclipped) { w_unclipped = lut_word(h0); have_unclipped = true; }
            w = w_unclipped;
        } else {
            int h[4] = {h0[0], h0[1], h0[2], h0[3]};
            int excess = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { excess += max(h[k] - clip, 0); h[k] = min(h[k], clip); }
            excess = (int)wave_sum_u32((uint32_t)excess);
            const int batch = excess >> 8;
            const int residual = excess & 255;
            // stepr = max(256 / residual, 1) and, for v / stepr with v < 256 without a per-lane integer division, the
            // multiplier m = floor(2^16 / stepr) + 1 (q = (v * m) >> 16 is exact here: v * (m * stepr - 2^16) <= 255 * 256 <
            // 2^16) -- both from a 256-entry table indexed by the wave-uniform residual instead of two division sequences
            // per clip limit
            const uint32_t sm = D_STEPR.v[__builtin_amdgcn_readfirstlane(residual)];
            const int stepr = (int)(sm & 511u);
            const uint32_t magic = sm >> 9;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int v = lane * 4 + k;
                h[k] += batch;
                if (residual != 0) {
                    if (rule == 0) {                                                           // OpenCV 3.4.x
                        const uint32_t q = __umul24((uint32_t)v, magic) >> 16;
                        if (__umul24(q, (uint32_t)stepr) == (uint32_t)v && (int)q < residual) h[k]++;
                    } else if (v < residual) h[k]++;                                           // OpenCV 3.2
                }
            }
            w = lut_word(h);
        }
        *reinterpret_cast<uint32_t *>(out + (size_t)c * 256 + lane * 4) = w;
    }
}

// ---- C1c: bilinear LUT interpolation, strip per block -------------------------
// strips[s] = (cy, r0, r1, unused): rows [r0,r1) all have floor(y*inv_th-0.5)+1 == cy.
// One launch may mix tile grids (the per-frame parameters of the aclahe stage): a per-frame descriptor then
// replaces the launch-wide geometry, so that 64 frames stay ONE long launch instead of one short launch per grid size.
struct ApplyFrame {
    const int4 *strips;     // this frame's strip list
    const uint8_t *luts;    // its tile LUTs [gy * gx][256]
    int fr;                 // frame index in src / dst
    int nstrips, gx, gy, TX, xs;    // xs: column parts per strip
    float inv_tw, inv_th;
};

inline int check_grid(uwip_ctx *ctx, int gx, int gy)
{
    UWIP_REQUIRE(ctx, gx >= 1 && gy >= 1 && gx <= 62 && gy <= 128, "tile grid must be in [1,62] x [1,128]");
    return UWIP_OK;
}

}  // namespace

// clahe.hip: the launchers the ACLAHE units share with the CLAHE entry points.  clip / ncl: the clip list of the launch
// (null: all zero -- the per-frame clips d_frame_clip are used); d_nf (optional): frames that take part, in device memory.
int uwip_clahe_launch_tilehist(uwip_ctx *ctx, const uwip_batch_u8 *src, const ClaheGeom &g, const int *d_frame_map, int nf,
                               uint32_t *d_hists, const int *d_nf = nullptr);
// histograms of g's grid from those of the grid twice as fine (neither padded)
int uwip_clahe_launch_tilehist_merge(uwip_ctx *ctx, const uint32_t *d_child, const ClaheGeom &g, int nf, uint32_t *d_hists);
int uwip_clahe_launch_lut(uwip_ctx *ctx, const ClaheGeom &g, const uint32_t *d_hists, const int *clip, int ncl, const int *d_frame_clip,
                          int nf, int rule, uint8_t *d_luts, uint32_t *d_tile_max = nullptr, const int *d_nf = nullptr);
// tile histograms + LUT rows in one launch where uwip_clahe_band_ok
bool uwip_clahe_band_ok(const uwip_batch_u8 *src, const ClaheGeom &g);
int uwip_clahe_launch_band(uwip_ctx *ctx, const uwip_batch_u8 *src, const ClaheGeom &g, const int *d_frame_map, int nf, const int *clip,
                           int ncl, const int *d_frame_clip, int rule, uint8_t *d_luts, uint32_t *d_tile_max, const int *d_nf = nullptr);
ApplyShape uwip_clahe_apply_shape(const ClaheGeom &g);
// strip table for (rows, gy, th, max_rows): built once per geometry and cached
int uwip_clahe_build_strips(uwip_ctx *ctx, const ClaheGeom &g, int max_rows, const int4 **d_strips, int *nstrips);
// all frames of a batch in ONE interpolation launch, each with its own geometry (d_desc: ApplyFrame [nf], device memory)
int uwip_clahe_launch_apply_mixed(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, const void *d_desc, int nf,
                                  int max_blocks, int max_cells);
