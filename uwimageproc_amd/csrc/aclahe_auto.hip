// The driver of the aclahe stage for gfx950: sweep -> parameter choice -> exact block-size
// search -> per-frame CLAHE.
//   k_aclahe_exact_bs  the block-size search at a clip limit outside the swept grid, one block per (flagged frame, grid)
//   k_pf_prepare       the launch of the per-frame CLAHE derived from device-side parameters
// The sweep is aclahe_sweep.hip, the parameter choice aclahe_select.cpp / aclahe_device.hip, the CLAHE kernels clahe.hip.
#include "clahe_internal.hpp"
#include <cstdlib>

namespace {

// ---- the block-size search at a clip limit OUTSIDE the swept grid, on the device (ACLAHE.py:102-112) -----------------------
// A knee index d >= 26 makes d itself (the reference uses the index as a clip limit) leave the sweep's 0 .. 25: the five
// entropies at that clip limit are then evaluated for the frame.  It takes a degenerate fit to get here, so
// this is written for correctness, not speed: one block per (flagged frame, grid) -- tile histograms by global atomics into
// the (frame, grid) slice of the tile-histogram workspace, LUT rows by clahe_lut_rows, the CLAHE output of every pixel
// (cv::CLAHE's float32 blend, the operations of k_clahe_apply) counted into a 256-bin LDS histogram without being stored,
// aclaheEntropy (k_entropy's operations); the last of a frame's five blocks to finish (an arrival counter in the spare field
// of the frame's parameter record) rewrites the frame's BS.  Blocks of unflagged frames exit at once.  Worst case (every
// frame of a batch flagged: tests/test_clahe_gpu.py measures it) ~13 ms at 1080p -- round 4 walked the five grids in ONE
// block per frame: 63 ms.
struct ExactGrids {
    int g[5], tw[5], th[5], pc[5], pr[5], area[5];
    float inv_tw[5], inv_th[5], lutScale[5];
};
__global__ __launch_bounds__(512) void k_aclahe_exact_bs(const uint8_t *__restrict__ src, size_t step, size_t fstride, int rows, int cols,
                                                        ExactGrids G, int rule, int32_t *__restrict__ par /*[F][4]*/,
                                                        uint32_t *__restrict__ hist_ws /*[F][1364][256]*/, uint8_t *__restrict__ lut_ws /*[F][1364][256]*/,
                                                        float *__restrict__ ent_ws /*[F][5]*/)
{
    const int f = blockIdx.x;
    if (par[4 * f + 2] != 1) return;             // (the last block of a flagged frame writes 2 only after all five have read this)
    __shared__ uint32_t s_out[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = par[4 * f + 1];
    const uint8_t *plane = src + (size_t)f * fstride;
    {
        const int k = blockIdx.y;
        uint32_t *hist = hist_ws + ((size_t)f * EXACT_TILES + exact_tile_off(k)) * 256;
        uint8_t *lut = lut_ws + ((size_t)f * EXACT_TILES + exact_tile_off(k)) * 256;
        const int gx = G.g[k], gy = G.g[k], tiles = gx * gy, tw = G.tw[k], th = G.th[k], pc = G.pc[k], pr = G.pr[k];
        for (int i = tid; i < tiles * 256; i += 512) hist[i] = 0;
        if (tid < 256) s_out[tid] = 0;
        __threadfence();
        __syncthreads();
        for (int i = tid; i < pc * pr; i += 512) {
            const int y = i / pc, x = i - y * pc;
            const uint32_t v = plane[(size_t)reflect101(y, rows) * step + reflect101(x, cols)];
            atomicAdd(&hist[((y / th) * gx + x / tw) * 256 + v], 1u);
        }
        __threadfence();
        __syncthreads();
        const int clip = clip_from_limit((double)d, G.area[k]);
        ClipList cl;
        cl.n = 1;
        for (int t = wave; t < tiles; t += 8) {
            const uint4 hv = *reinterpret_cast<const uint4 *>(hist + (size_t)t * 256 + lane * 4);
            const int h0[4] = {(int)hv.x, (int)hv.y, (int)hv.z, (int)hv.w};
            clahe_lut_rows(h0, lane, G.lutScale[k], cl, clip, rule, lut + (size_t)t * 256, nullptr);
        }
        __threadfence();
        __syncthreads();
        const float inv_tw = G.inv_tw[k], inv_th = G.inv_th[k];
        for (int i = tid; i < rows * cols; i += 512) {
            const int y = i / cols, x = i - y * cols;
            const uint32_t v = plane[(size_t)y * step + x];
            const float txf = (float)x * inv_tw - 0.5f, tyf = (float)y * inv_th - 0.5f;
            const float flx = floorf(txf), fly = floorf(tyf);
            const float xa = txf - flx, xa1 = 1.0f - xa, ya = tyf - fly, ya1 = 1.0f - ya;
            const int tx1 = max((int)flx, 0), tx2 = min((int)flx + 1, gx - 1), ty1 = max((int)fly, 0), ty2 = min((int)fly + 1, gy - 1);
            const uint32_t TL = lut[(size_t)(ty1 * gx + tx1) * 256 + v], TR = lut[(size_t)(ty1 * gx + tx2) * 256 + v];
            const uint32_t BL = lut[(size_t)(ty2 * gx + tx1) * 256 + v], BR = lut[(size_t)(ty2 * gx + tx2) * 256 + v];
            const float res = clahe_blend(TL, TR, BL, BR, xa1, xa, ya1, ya);
            atomicAdd(&s_out[__builtin_amdgcn_cvt_pk_u8_f32(res, 0, 0u)], 1u);
        }
        __syncthreads();
        if (tid == 0) {                                // aclaheEntropy, aclahe.cpp:241-247
            float e = 0.0f;
            for (int i = 0; i < 256; ++i) e = (float)((double)e + entropy_term(s_out[i], rows, cols));
            ent_ws[(size_t)f * 5 + k] = -e;
            __threadfence();
            if (atomicAdd(&par[4 * f + 3], 1) == 4) {              // the last of the frame's five blocks
                __threadfence();
                int w = 0;
                float best = 0.f;
                for (int q = 0; q < 5; ++q) {
                    const float h = (float)(_Float16)__hip_atomic_load(&ent_ws[(size_t)f * 5 + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (q == 0 || h >= best) { best = h; w = q; }  // last maximum wins (ACLAHE.py:118-124)
                }
                par[4 * f + 0] = G.g[w];
                par[4 * f + 3] = 0;
                par[4 * f + 2] = 2;                                  // evaluated
            }
        }
    }
}

// ---- the final CLAHE of the aclahe stage launched from DEVICE-side parameters (round 4) -------------------------------------
// The parameter choice is made on the device (aclahe_device.hip); to launch the per-frame CLAHE without bringing {BS, CL}
// back, everything the host used to derive from them is derived here: the frames are grouped by block size (group k =
// block size 2, 4, 8, 16, 32, frame order kept), every group gets its frame map, clip limits and frame count, every frame
// its interpolation descriptor.  The host then launches the tile-histogram / LUT kernels of ALL five grids over the whole
// batch -- a block whose frame index is beyond its group's count exits at once -- and the one mixed interpolation launch.
struct PfGrids {
    const int4 *strips[5];
    uint8_t *luts[5];
    int *map[5], *clip[5];
    int nstrips[5], g[5], TX[5], xs[5], area[5], tiles[5];
    float inv_tw[5], inv_th[5];
};
__global__ void k_pf_prepare(const int32_t *__restrict__ par /*[F][4] = BS, CL, ..*/, int F, PfGrids G, int *__restrict__ count /*[5]*/,
                             ApplyFrame *__restrict__ desc)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int cnt[5] = {0, 0, 0, 0, 0};
    for (int f = 0; f < F; ++f) {                   // a sub-batch: a serial walk keeps every group in frame order
        const int bs = par[4 * f], cl = par[4 * f + 1];
        int k = ACLAHE_NBS - 1;                      // the group of block size bs (none of the list: the last)
#pragma unroll
        for (int q = ACLAHE_NBS - 2; q >= 0; --q) if (bs == ACLAHE_BS[q]) k = q;
        int i = 0;
#pragma unroll
        for (int q = 0; q < 5; ++q) if (q == k) i = cnt[q]++;
        G.map[k][i] = f;
        G.clip[k][i] = clip_from_limit((double)cl, G.area[k]);
        ApplyFrame a;
        a.strips = G.strips[k]; a.luts = G.luts[k] + (size_t)i * G.tiles[k] * 256; a.fr = f;
        a.nstrips = G.nstrips[k]; a.gx = G.g[k]; a.gy = G.g[k]; a.TX = G.TX[k]; a.xs = G.xs[k];
        a.inv_tw = G.inv_tw[k]; a.inv_th = G.inv_th[k];
        desc[f] = a;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) count[q] = cnt[q];
}

// the exact block-size search (one predicated launch; see k_aclahe_exact_bs) of the frames the [F][4] record "auto.par"
// flags, for every form of uwip_aclahe_auto_ex.  Async (h_par = NULL): launched unconditionally behind the device choice.
// Synchronous (h_par = the host copy of the record): only when some frame is flagged -- the record goes up first when the
// host made it (upload; field 3, the kernel's arrival counter, is 0), and comes back before the call returns.
int aclahe_exact_bs_device(uwip_ctx *ctx, const uwip_batch_u8 *src, int residual_rule, int32_t *h_par, bool upload)
{
    const int F = src->frames;
    bool any = !h_par;
    for (int f = 0; !any && f < F; ++f) any = h_par[4 * f + 2] != 0;
    if (!any) return UWIP_OK;
    ExactGrids G{};
    for (int k = 0; k < 5; ++k) {
        const ClaheGeom g = make_geom(src->rows, src->cols, ACLAHE_BS[k], ACLAHE_BS[k]);
        G.g[k] = ACLAHE_BS[k]; G.tw[k] = g.tw; G.th[k] = g.th; G.pc[k] = g.pc; G.pr[k] = g.pr; G.area[k] = g.area;
        G.inv_tw[k] = g.inv_tw; G.inv_th[k] = g.inv_th; G.lutScale[k] = g.lutScale;
    }
    int32_t *d_par = (int32_t *)uwip_ws(ctx, "auto.par", sizeof(int32_t) * 4 * (size_t)F);
    uint32_t *d_hists = (uint32_t *)uwip_ws(ctx, "clahe.tilehist", sizeof(uint32_t) * 256 * (size_t)EXACT_TILES * F);
    uint8_t *d_luts = (uint8_t *)uwip_ws(ctx, "sweep.luts", SWEEP_LUTS_FRAME_BYTES * F);      // borrowed: >= EXACT_LUTS_FRAME_BYTES * F (clahe_internal.hpp)
    float *d_ent = (float *)uwip_ws(ctx, "auto.exact_ent", sizeof(float) * 5 * (size_t)F);
    if (!d_par || !d_hists || !d_luts || !d_ent) return UWIP_ERR_NOMEM;
    if (upload) UWIP_HIP(ctx, hipMemcpyAsync(d_par, h_par, sizeof(int32_t) * 4 * (size_t)F, hipMemcpyHostToDevice, ctx->stream));
    {
        uwip_kscope ks(ctx, "k_aclahe_exact_bs");
        k_aclahe_exact_bs<<<dim3(F, 5), 512, 0, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, src->rows,
                                                               src->cols, G, residual_rule, d_par, d_hists, d_luts, d_ent);
        UWIP_HIP(ctx, hipGetLastError());
    }
    if (!h_par) return UWIP_OK;
    UWIP_HIP(ctx, hipMemcpyAsync(h_par, d_par, sizeof(int32_t) * 4 * (size_t)F, hipMemcpyDeviceToHost, ctx->stream));
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    return UWIP_OK;
}

// createCLAHE(CL, (BS, BS)).apply per frame with {BS, CL} read from device memory (d_par [F][4]): no host wait, no copy
int clahe_per_frame_device(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, const int32_t *d_par, int residual_rule)
{
    int rc = uwip_check_pair(ctx, src, dst);
    if (rc) return rc;
    if (uwip_batch_empty(src)) return UWIP_OK;
    const int F = src->frames;
    ClaheGeom g[5];
    ApplyShape sh[5];
    PfGrids G{};
    size_t lut_bytes = 0;
    for (int k = 0; k < 5; ++k) {
        rc = check_grid(ctx, ACLAHE_BS[k], ACLAHE_BS[k]);
        if (rc) return rc;
        g[k] = make_geom(src->rows, src->cols, ACLAHE_BS[k], ACLAHE_BS[k]);
        sh[k] = uwip_clahe_apply_shape(g[k]);
        lut_bytes += (size_t)ACLAHE_BS[k] * ACLAHE_BS[k] * 256 * F;
    }
    uint32_t *d_hists = (uint32_t *)uwip_ws(ctx, "clahe.tilehist", sizeof(uint32_t) * 256 * (size_t)CLAHE_MAX_TILES * F);
    uint8_t *d_luts = (uint8_t *)uwip_ws(ctx, "clahe.pfd.luts", lut_bytes);
    int *d_ints = (int *)uwip_ws(ctx, "clahe.pfd.ints", sizeof(int) * (10 * (size_t)F + 8));
    ApplyFrame *d_desc = (ApplyFrame *)uwip_ws(ctx, "clahe.pf.desc", sizeof(ApplyFrame) * (size_t)F);
    if (!d_hists || !d_luts || !d_ints || !d_desc) return UWIP_ERR_NOMEM;
    int *d_count = d_ints + 10 * (size_t)F;
    int max_blocks = 0, max_cells = 0;
    size_t loff = 0;
    for (int k = 0; k < 5; ++k) {
        const int4 *d_strips = nullptr;
        int nstrips = 0;
        rc = uwip_clahe_build_strips(ctx, g[k], sh[k].max_rows, &d_strips, &nstrips);
        if (rc) return rc;
        G.strips[k] = d_strips; G.nstrips[k] = nstrips; G.g[k] = ACLAHE_BS[k]; G.TX[k] = sh[k].TX; G.xs[k] = sh[k].xs;
        G.area[k] = g[k].area; G.tiles[k] = ACLAHE_BS[k] * ACLAHE_BS[k]; G.inv_tw[k] = g[k].inv_tw; G.inv_th[k] = g[k].inv_th;
        G.luts[k] = d_luts + loff;
        loff += (size_t)G.tiles[k] * 256 * F;
        G.map[k] = d_ints + (size_t)k * F;
        G.clip[k] = d_ints + (size_t)(5 + k) * F;
        max_blocks = std::max(max_blocks, nstrips * sh[k].xs);
        max_cells = std::max(max_cells, sh[k].lds_cells);
    }
    {
        uwip_kscope ks(ctx, "k_pf_prepare");
        k_pf_prepare<<<1, 64, 0, ctx->stream>>>(d_par, F, G, d_count, d_desc);
        UWIP_HIP(ctx, hipGetLastError());
    }
    for (int k = 0; k < 5; ++k) {
        if (uwip_clahe_band_ok(src, g[k])) {
            rc = uwip_clahe_launch_band(ctx, src, g[k], G.map[k], F, nullptr, 1, G.clip[k], residual_rule, G.luts[k], nullptr, d_count + k);
            if (rc) return rc;
        } else {
            rc = uwip_clahe_launch_tilehist(ctx, src, g[k], G.map[k], F, d_hists, d_count + k);
            if (rc) return rc;
            rc = uwip_clahe_launch_lut(ctx, g[k], d_hists, nullptr, 1, G.clip[k], F, residual_rule, G.luts[k], nullptr, d_count + k);
            if (rc) return rc;
        }
    }
    return uwip_clahe_launch_apply_mixed(ctx, src, dst, d_desc, F, max_blocks, max_cells);
}

}  // namespace

int uwip_aclahe_select_internal(const float *h_entropy, int frames, int32_t *h_bs, int32_t *h_cl, int32_t *h_knee,
                                int32_t *h_need_eval);
extern "C" int uwip_aclahe_select_device(uwip_ctx *ctx, const float *d_entropy, int frames, int32_t *d_par, int32_t *d_knee);

// C3 + C4 + the final apply in one call: sweep -> parameter choice -> exact block-size search -> per-frame CLAHE.
// This is the whole "aclahe" stage of the pipe.  h_bs / h_cl receive the chosen parameters.
UWIP_API int uwip_aclahe_auto_ex(uwip_ctx *ctx, const uwip_batch_u8 *img, const uwip_batch_u8 *dst, int residual_rule, unsigned flags,
                                 int32_t *h_bs, int32_t *h_cl)
{
    int rc = uwip_check_pair(ctx, img, dst);
    if (rc) return rc;
    if (img->frames == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, !uwip_batch_empty(img), "aclahe of an empty image");
    UWIP_REQUIRE(ctx, (flags & ~(unsigned)(UWIP_ACLAHE_PREFILTER | UWIP_ACLAHE_HOST_SELECT | UWIP_ACLAHE_ASYNC)) == 0, "unknown flag");
    UWIP_REQUIRE(ctx, !(flags & UWIP_ACLAHE_ASYNC) || (!h_bs && !h_cl), "UWIP_ACLAHE_ASYNC: the parameters are fetched with uwip_aclahe_last_params");
    const int F = img->frames;
    // a call that fails leaves "no parameters recorded" (not the previous call's): recorded only after the last launch succeeded
    ctx->aclahe_last_n = 0;
    ctx->aclahe_last_on_device = false;
    ctx->aclahe_last_host.clear();
    // Where the choice is made.  Default: on the device (no table copy, no host computation: 0.25 CPU-seconds per 512-frame
    // step and rank otherwise) -- except for batches of a few frames, where latency is what matters (the paced 4K@60 stream
    // runs one frame per call): a curve takes one wavefront 1.3 ms on the device (a serial dependent chain of float64
    // divisions and square roots at one instruction per ~9 cycles) and a host core 0.15 ms.  UWIP_ACLAHE_SELECT=host|device
    // or the flag force one form; both give the same parameters bit for bit.
    static const int env_sel = [] { const char *e = getenv("UWIP_ACLAHE_SELECT"); return !e ? 0 : ((*e == 'h' || *e == 'H') ? 1 : ((*e == 'd' || *e == 'D') ? 2 : 0)); }();
    const bool host_select = (flags & UWIP_ACLAHE_HOST_SELECT) || env_sel == 1 || (env_sel == 0 && F <= 4);
    // ParametrosACLAHE searches its parameters on imgfilt = GaussianBlur(img, (3,3), 0) (ACLAHE.py:15: the sweep :40-47 and
    // the block-size search :102-112 both run on it); the final createCLAHE(CL,(BS,BS)).apply takes the unfiltered image
    // (python/main.py:19-20).  The C++ driver (aclahe.cpp:152-187) sweeps the unfiltered plane: flags = 0.
    uwip_batch_u8 filt = *img;
    if (flags & UWIP_ACLAHE_PREFILTER) {
        uint8_t *fb = (uint8_t *)uwip_ws(ctx, "auto.blur", (size_t)img->rows * img->cols * F);
        if (!fb) return UWIP_ERR_NOMEM;
        filt.data = fb; filt.step = (size_t)img->cols; filt.frame_stride = (size_t)img->rows * img->cols;
        rc = uwip_GaussianBlur3(ctx, img, &filt, residual_rule);
        if (rc) return rc;
    }
    const uwip_batch_u8 *src = &filt;
    float *d_ent = (float *)uwip_ws(ctx, "auto.entropy", sizeof(float) * 255 * F);
    if (!d_ent) return UWIP_ERR_NOMEM;
    rc = uwip_aclahe_sweep(ctx, src, residual_rule, d_ent);
    if (rc) return rc;
    int32_t *d_par = nullptr;
    if (!host_select) {
        // the choice on the device (aclahe_device.hip) into the record d_par [F][4] = {BS, CL, need, 0}
        d_par = (int32_t *)uwip_ws(ctx, "auto.par", sizeof(int32_t) * 4 * (size_t)F);
        if (!d_par) return UWIP_ERR_NOMEM;
        rc = uwip_aclahe_select_device(ctx, d_ent, F, d_par, nullptr);
        if (rc) return rc;
        if (flags & UWIP_ACLAHE_ASYNC) {
            // nothing comes back to the host: the exact search and the launch of the final CLAHE from the device-side
            // parameters (clahe_per_frame_device) are queued behind the sweep, and the call returns
            rc = aclahe_exact_bs_device(ctx, src, residual_rule, nullptr, false);
            if (rc) return rc;
            rc = clahe_per_frame_device(ctx, img, dst, d_par, residual_rule);
            if (rc) return rc;
            ctx->aclahe_last_n = F;
            ctx->aclahe_last_on_device = true;
            return UWIP_OK;
        }
    }
    // the synchronous forms: the choice in the same record on the host
    int32_t *par = (int32_t *)uwip_host_ws(ctx, "auto.dpar", sizeof(int32_t) * 4 * (size_t)F);
    if (!par) return UWIP_ERR_NOMEM;
    if (!host_select) {
        // only the record comes back -- the launch geometry of the final CLAHE depends on it
        UWIP_HIP(ctx, hipMemcpyAsync(par, d_par, sizeof(int32_t) * 4 * (size_t)F, hipMemcpyDeviceToHost, ctx->stream));
        UWIP_HIP(ctx, uwip_stream_wait(ctx));
    } else {
        float *h_ent = (float *)uwip_host_ws(ctx, "auto.entropy", sizeof(float) * 255 * F);
        if (!h_ent) return UWIP_ERR_NOMEM;
        UWIP_HIP(ctx, hipMemcpyAsync(h_ent, d_ent, sizeof(float) * 255 * F, hipMemcpyDeviceToHost, ctx->stream));
        UWIP_HIP(ctx, uwip_stream_wait(ctx));            // host decision point (ACLAHE.py:66-129)
        std::vector<int32_t> sel(3 * (size_t)F);         // BS, CL, need
        rc = uwip_aclahe_select_internal(h_ent, F, sel.data(), sel.data() + F, nullptr, sel.data() + 2 * F);
        if (rc) return ctx->fail(rc, "aclahe select");
        const int force = uwip_test_force_cl();          // as uwip_aclahe_select_device applies it
        for (int f = 0; f < F; ++f) {
            par[4 * f] = sel[f];
            par[4 * f + 1] = force >= 0 ? force : sel[F + f];
            par[4 * f + 2] = force >= 0 ? (2 * force > 50) : sel[2 * F + f];
            par[4 * f + 3] = 0;
        }
    }
    rc = aclahe_exact_bs_device(ctx, src, residual_rule, par, host_select);
    if (rc) return rc;
    std::vector<int32_t> bs(F);
    std::vector<double> clip(F);
    for (int f = 0; f < F; ++f) { bs[f] = par[4 * f]; clip[f] = (double)par[4 * f + 1]; }
    if (h_bs) for (int f = 0; f < F; ++f) h_bs[f] = par[4 * f];
    if (h_cl) for (int f = 0; f < F; ++f) h_cl[f] = par[4 * f + 1];
    rc = uwip_clahe_per_frame(ctx, img, dst, clip.data(), bs.data(), residual_rule);
    if (rc) return rc;
    ctx->aclahe_last_host.assign(par, par + 4 * (size_t)F);
    ctx->aclahe_last_n = F;
    return UWIP_OK;
}

// the parameters of the most recent uwip_aclahe_auto_ex on this context (waits for the stream when they are still on the device)
UWIP_API int uwip_aclahe_last_params(uwip_ctx *ctx, int32_t *h_bs, int32_t *h_cl, int frames)
{
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    if (frames == 0 && ctx->aclahe_last_n == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, ctx->aclahe_last_n > 0, "no parameters recorded (no uwip_aclahe_auto_ex yet, or the last one failed)");
    UWIP_REQUIRE(ctx, frames == ctx->aclahe_last_n, "frame count differs from the last uwip_aclahe_auto_ex");
    UWIP_REQUIRE(ctx, h_bs && h_cl, "null output");
    const int32_t *h = ctx->aclahe_last_host.data();
    if (ctx->aclahe_last_on_device) {
        const int32_t *d_par = (const int32_t *)uwip_ws(ctx, "auto.par", sizeof(int32_t) * 4 * (size_t)frames);
        int32_t *hp = (int32_t *)uwip_host_ws(ctx, "auto.dpar", sizeof(int32_t) * 4 * (size_t)frames);
        if (!d_par || !hp) return UWIP_ERR_NOMEM;
        UWIP_HIP(ctx, hipMemcpyAsync(hp, d_par, sizeof(int32_t) * 4 * (size_t)frames, hipMemcpyDeviceToHost, ctx->stream));
        UWIP_HIP(ctx, uwip_stream_wait(ctx));
        h = hp;
    } else {
        UWIP_REQUIRE(ctx, ctx->aclahe_last_host.size() == 4 * (size_t)frames, "no parameters recorded");
    }
    for (int f = 0; f < frames; ++f) { h_bs[f] = h[4 * f]; h_cl[f] = h[4 * f + 1]; }
    return UWIP_OK;
}

UWIP_API int uwip_aclahe_auto(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, int residual_rule,
                              int32_t *h_bs, int32_t *h_cl)
{
    return uwip_aclahe_auto_ex(ctx, src, dst, residual_rule, 0u, h_bs, h_cl);
}
