// The two 8-bit plane operations in front of the aclahe stage's sweep, for gfx950:
//   k_bgr_to_v    the V plane of a BGR image (max of the three channels)
//   k_gauss3_u8   cv2.GaussianBlur(img, (3,3), 0), ParametrosACLAHE's prefilter (ACLAHE.py:15)
#include "uwip_internal.hpp"
#include "device_utils.hpp"
#include <algorithm>

namespace {

// ---- BGR -> V (max) -------------------------------------------------------
__global__ __launch_bounds__(256) void k_bgr_to_v(const uint8_t *__restrict__ src, size_t sstep,
                                                  size_t sfs, uint8_t *__restrict__ dst,
                                                  size_t dstep, size_t dfs, int rows, int cols,
                                                  int vec)
{
    const int f = blockIdx.z;
    const int y = blockIdx.y;
    const uint8_t *s = src + (size_t)f * sfs + (size_t)y * sstep;
    uint8_t *d = dst + (size_t)f * dfs + (size_t)y * dstep;
    const int groups = (cols + 15) / 16;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int x0 = g * 16;
        if (vec && x0 + 16 <= cols) {
            const uint4 a = *reinterpret_cast<const uint4 *>(s + (size_t)x0 * 3);
            const uint4 b = *reinterpret_cast<const uint4 *>(s + (size_t)x0 * 3 + 16);
            const uint4 c = *reinterpret_cast<const uint4 *>(s + (size_t)x0 * 3 + 32);
            const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b0 = 3 * i, b1 = 3 * i + 1, b2 = 3 * i + 2;
                const uint32_t B = (w[b0 >> 2] >> ((b0 & 3) * 8)) & 255u;
                const uint32_t G = (w[b1 >> 2] >> ((b1 & 3) * 8)) & 255u;
                const uint32_t R = (w[b2 >> 2] >> ((b2 & 3) * 8)) & 255u;
                o[i >> 2] |= max(max(B, G), R) << ((i & 3) * 8);
            }
            *reinterpret_cast<uint4 *>(d + x0) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            for (int x = x0; x < min(x0 + 16, cols); ++x) {
                const uint8_t B = s[3 * x], G = s[3 * x + 1], R = s[3 * x + 2];
                d[x] = max(max(B, G), R);
            }
        }
    }
}

// ---- cv2.GaussianBlur(img, (3,3), 0) on an 8-bit plane (ACLAHE.py:15) ------------------------------------
// ksize 3 with sigma <= 0 takes OpenCV's fixed table [0.25, 0.5, 0.25]; BORDER_DEFAULT = REFLECT_101.  Both passes are
// exact in fixed point, so the result is (sum of the 3x3 window weighted 1 2 1 / 2 4 2 / 1 2 1) / 16 rounded:
//   rule 0 (OpenCV 3.4.x, bit-exact 8-bit path: ufixedpoint16 -> uchar adds one half and truncates): round half UP
//   rule 1 (OpenCV 3.2, float rows/columns + cvRound): round half to EVEN.   parity unpinned (OpenCV-internal).
constexpr int GS3_ROWS = 8;      // rows per block row of the aligned path
template <bool VEC>
__global__ __launch_bounds__(256) void k_gauss3_u8(const uint8_t *__restrict__ src, size_t sstep, size_t sfs,
                                                   uint8_t *__restrict__ dst, size_t dstep, size_t dfs, int rows, int cols, int rule)
{
    const int f = blockIdx.z, y = blockIdx.y;
    const int ym = rows == 1 ? 0 : (y == 0 ? 1 : y - 1), yp = rows == 1 ? 0 : (y == rows - 1 ? rows - 2 : y + 1);
    const uint8_t *r0 = src + (size_t)f * sfs + (size_t)ym * sstep, *r1 = src + (size_t)f * sfs + (size_t)y * sstep,
                  *r2 = src + (size_t)f * sfs + (size_t)yp * sstep;
    uint8_t *d = dst + (size_t)f * dfs + (size_t)y * dstep;
    auto finish = [&](int s) -> uint32_t {                     // s = window sum, <= 16 * 255
        int q = (s + 8) >> 4;                                  // half up
        if (rule == 1 && (s & 15) == 8) q = ((s >> 4) & 1) ? (s >> 4) + 1 : (s >> 4);      // tie -> even
        return (uint32_t)q;
    };
    if (VEC) {
        // four pixels per thread and GS3_ROWS rows per block row: the horizontal 1 2 1 sums of a row (three dwords: the
        // thread's own and its two neighbours') are formed once and serve the three output rows they touch -- the window
        // sum is an exact integer, so horizontal-then-vertical equals vertical-then-horizontal
        const int n4 = cols >> 2;
        const int y0 = blockIdx.y * GS3_ROWS, y1 = min(y0 + GS3_ROWS, rows);
        const uint8_t *base = src + (size_t)f * sfs;
        for (int g = blockIdx.x * 256 + threadIdx.x; g < n4; g += gridDim.x * 256) {
            const int gl = g == 0 ? 0 : g - 1, gr = g == n4 - 1 ? g : g + 1;
            // h[k] = s[x-1] + 2 s[x] + s[x+1] of the row's pixels x = 4g + k, reflect-101 at the row ends
            auto hrow = [&](int yy, uint32_t (&hh)[4]) {
                const uint32_t *p = reinterpret_cast<const uint32_t *>(base + (size_t)yy * sstep);
                const uint32_t a = p[g], l = p[gl], q = p[gr];
                const uint32_t c0 = a & 255u, c1 = (a >> 8) & 255u, c2 = (a >> 16) & 255u, c3 = a >> 24;
                const uint32_t cm = g == 0 ? c1 : l >> 24, cp = g == n4 - 1 ? c2 : q & 255u;
                hh[0] = cm + 2u * c0 + c1; hh[1] = c0 + 2u * c1 + c2; hh[2] = c1 + 2u * c2 + c3; hh[3] = c2 + 2u * c3 + cp;
            };
            auto refl = [&](int yy) { return rows == 1 ? 0 : (yy < 0 ? 1 : (yy >= rows ? rows - 2 : yy)); };
            uint32_t ha[4], hb[4], hc[4];
            hrow(refl(y0 - 1), ha);
            hrow(y0, hb);
            for (int yy = y0; yy < y1; ++yy) {
                hrow(refl(yy + 1), hc);
                uint32_t o = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) o |= finish((int)(ha[k] + 2u * hb[k] + hc[k])) << (8 * k);
                reinterpret_cast<uint32_t *>(dst + (size_t)f * dfs + (size_t)yy * dstep)[g] = o;
#pragma unroll
                for (int k = 0; k < 4; ++k) { ha[k] = hb[k]; hb[k] = hc[k]; }
            }
        }
        return;
    }
    for (int x = blockIdx.x * 256 + threadIdx.x; x < cols; x += gridDim.x * 256) {
        const int xm = cols == 1 ? 0 : (x == 0 ? 1 : x - 1), xp = cols == 1 ? 0 : (x == cols - 1 ? cols - 2 : x + 1);
        const int v0 = r0[xm] + 2 * r0[x] + r0[xp], v1 = r1[xm] + 2 * r1[x] + r1[xp], v2 = r2[xm] + 2 * r2[x] + r2[xp];
        d[x] = (uint8_t)finish(v0 + 2 * v1 + v2);
    }
}

}  // namespace

UWIP_API int uwip_bgr_to_v(uwip_ctx *ctx, const uwip_batch_u8 *bgr, const uwip_batch_u8 *v)
{
    int rc = uwip_check_batch(ctx, bgr, 3);
    if (rc) return rc;
    rc = uwip_check_batch(ctx, v, 1);
    if (rc) return rc;
    UWIP_REQUIRE(ctx, bgr->rows == v->rows && bgr->cols == v->cols && bgr->frames == v->frames, "shape mismatch");
    if (uwip_batch_empty(bgr)) return UWIP_OK;
    const int groups = (bgr->cols + 15) / 16;
    dim3 grid(uwip_cdiv(groups, 256), (unsigned)bgr->rows, (unsigned)bgr->frames);
    UWIP_REQUIRE(ctx, bgr->rows <= 65535 && bgr->frames <= 65535, "too many rows/frames for one launch");
    const int vec = uwip_aligned_for(bgr, 16) && uwip_aligned_for(v, 16);
    uwip_kscope ks(ctx, "k_bgr_to_v");
    k_bgr_to_v<<<grid, 256, 0, ctx->stream>>>((const uint8_t *)bgr->data, bgr->step, bgr->frame_stride,
                                              (uint8_t *)v->data, v->step, v->frame_stride, bgr->rows, bgr->cols, vec);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

UWIP_API int uwip_GaussianBlur3(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, int rounding_rule)
{
    int rc = uwip_check_pair(ctx, src, dst);
    if (rc) return rc;
    if (uwip_batch_empty(src)) return UWIP_OK;
    UWIP_REQUIRE(ctx, src->data != dst->data, "GaussianBlur3 cannot run in place");
    UWIP_REQUIRE(ctx, src->frames <= 65535 && src->rows <= 65535, "batch too large for one launch");
    uwip_kscope ks(ctx, "k_gauss3_u8");
    const bool vec = src->cols >= 8 && src->cols % 4 == 0 && uwip_aligned_for(src, 4) && uwip_aligned_for(dst, 4);
    const dim3 grid(std::min(uwip_cdiv(vec ? src->cols / 4 : src->cols, 256), 64u), vec ? uwip_cdiv(src->rows, GS3_ROWS) : (unsigned)src->rows, (unsigned)src->frames);
    if (vec)
        k_gauss3_u8<true><<<grid, 256, 0, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, (uint8_t *)dst->data, dst->step,
                                                        dst->frame_stride, src->rows, src->cols, rounding_rule);
    else
        k_gauss3_u8<false><<<grid, 256, 0, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, (uint8_t *)dst->data, dst->step,
                                                         dst->frame_stride, src->rows, src->cols, rounding_rule);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}
