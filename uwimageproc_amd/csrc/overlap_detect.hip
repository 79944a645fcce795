// videostrip overlap path, detection: resize -> gray -> non-linear scale space (Gaussian + FED diffusion) -> determinant of
// the Hessian -> extrema -> at most MAXKP keypoints: the first MAXKP in (level, y, x) raster order among the candidates whose
// response is >= the MAXKP-th largest (DESIGN.md "overlap stage"); and calcBlur, which shares the fused resize + gray kernel.
#include "overlap_internal.hpp"
#include "device_utils.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int BORDER = 8;
constexpr float DTHRESH = 0.001f;
constexpr float KC_REF = 0.5f;       // contrast factor at and above which the detector threshold is DTHRESH itself

const float H_SIGMA[NLEV] = {1.6f, 2.2627417f, 3.2f, 4.5254834f};
const int H_SSIZE[NLEV] = {2, 3, 5, 7};      // overlap_describe.hip's D_SSIZE holds the same values

struct ConvK {
    int ks;
    float k[16];
};

// ---- resize (INTER_LINEAR, 8UC3, fixed point) + BGR2GRAY + /255 ---------------------------
__global__ __launch_bounds__(256) void k_ov_resize_gray(const uint8_t *__restrict__ src, size_t step, size_t fs,
                                                       int rows, int cols, int oh, int ow,
                                                       const int *__restrict__ xo, const short *__restrict__ xa,
                                                       const short *__restrict__ xb, const int *__restrict__ yo,
                                                       const short *__restrict__ ya, const short *__restrict__ yb,
                                                       uint8_t *__restrict__ gray, float *__restrict__ L0)
{
    const int f = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const uint8_t *b = src + (size_t)f * fs;
    const int sy = yo[y], sy1 = sy + 1 < rows ? sy + 1 : sy;
    const uint8_t *r0 = b + (size_t)sy * step, *r1 = b + (size_t)sy1 * step;
    const int sx = xo[x], sx1 = sx + 1 < cols ? sx + 1 : sx;
    const int a0 = xa[x], a1 = xb[x], b0 = ya[y], b1 = yb[y];
    int px[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int S0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
        const int S1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        px[c] = min(max(v, 0), 255);
    }
    const int g = (px[0] * 1868 + px[1] * 9617 + px[2] * 4899 + 8192) >> 14;
    const size_t o = ((size_t)f * oh + y) * ow + x;
    gray[o] = (uint8_t)g;
    L0[o] = (float)g / 255.0f;
}

// cv::resize(frame, res_frame, Size(), f, f) alone (main.cpp:242,287,311): the 8UC3 result the reference hands to
// calcOverlap and calcBlur.  Same fixed-point arithmetic as the fused kernel above.
__global__ __launch_bounds__(256) void k_ov_resize_bgr(const uint8_t *__restrict__ src, size_t step, size_t fs, int rows, int cols,
                                                      int oh, int ow, const int *__restrict__ xo, const short *__restrict__ xa,
                                                      const short *__restrict__ xb, const int *__restrict__ yo,
                                                      const short *__restrict__ ya, const short *__restrict__ yb,
                                                      uint8_t *__restrict__ dst, size_t dstep, size_t dfs)
{
    const int f = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const uint8_t *b = src + (size_t)f * fs;
    const int sy = yo[y], sy1 = sy + 1 < rows ? sy + 1 : sy;
    const uint8_t *r0 = b + (size_t)sy * step, *r1 = b + (size_t)sy1 * step;
    const int sx = xo[x], sx1 = sx + 1 < cols ? sx + 1 : sx;
    const int a0 = xa[x], a1 = xb[x], b0 = ya[y], b1 = yb[y];
    uint8_t *o = dst + (size_t)f * dfs + (size_t)y * dstep + (size_t)x * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int S0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
        const int S1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        o[c] = (uint8_t)min(max(v, 0), 255);
    }
}

// gray u8 (already at working size) -> L0
__global__ void k_ov_gray_to_L0(const uint8_t *__restrict__ gray, float *__restrict__ L0, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) L0[i] = (float)gray[i] / 255.0f;
}

// ---- separable Gaussian, reflect-101 border ----------------------------------------------
// Both passes of the separable Gaussian in one launch: a block owns a 64 x 16 output tile, stages the tile + halo once
// (reflect-101 applied to the global indices), convolves along x into a second LDS plane (tile rows + halo rows) and
// along y out of it.  Every output goes through the same multiplies and adds in the same order as the two-pass form
// (the intermediate row of image row reflect101(y) is what the y pass of the two-pass form reads there).
constexpr int CV_TW = 64, CV_TH = 16, CV_RMAX = 7;
// KS = the kernel size when it is one of the usual ones (5 for sigma 1, 9 for sigma 1.6: loops unrolled, the staging index a
// constant division), 0 = any odd size up to 2 CV_RMAX + 1 at run time.
template <int KS>
__global__ __launch_bounds__(256) void k_ov_conv2(const float *__restrict__ in, float *__restrict__ out, int h, int w, ConvK K)
{
    __shared__ float s_in[(CV_TH + 2 * CV_RMAX) * (CV_TW + 2 * CV_RMAX)];
    __shared__ float s_tmp[(CV_TH + 2 * CV_RMAX) * CV_TW];
    const int f = blockIdx.z, x0 = blockIdx.x * CV_TW, y0 = blockIdx.y * CV_TH;
    const float *I = in + (size_t)f * h * w;
    const int ks = KS ? KS : K.ks;
    const int r = ks / 2, RW = CV_TW + 2 * r, RH = CV_TH + 2 * r;
    const bool inside = x0 - r >= 0 && y0 - r >= 0 && x0 - r + RW <= w && y0 - r + RH <= h;     // block-uniform
    if (inside) {
        const float *base = I + (size_t)(y0 - r) * w + (x0 - r);
        for (int i = threadIdx.x; i < RH * RW; i += 256) {
            const int ry = i / RW, rx = i - ry * RW;
            s_in[i] = base[(size_t)ry * w + rx];
        }
    } else {
        for (int i = threadIdx.x; i < RH * RW; i += 256) {
            const int ry = i / RW, rx = i - ry * RW;
            s_in[i] = I[(size_t)reflect101(y0 - r + ry, h) * w + reflect101(x0 - r + rx, w)];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RH * CV_TW; i += 256) {
        const int ry = i / CV_TW, tx = i - ry * CV_TW;
        const float *row = s_in + ry * RW + tx;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < ks; ++k) acc = acc + K.k[k] * row[k];
        s_tmp[i] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CV_TH * CV_TW; i += 256) {
        const int ty = i / CV_TW, tx = i - ty * CV_TW;
        const float *col = s_tmp + ty * CV_TW + tx;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < ks; ++k) acc = acc + K.k[k] * col[k * CV_TW];
        const int x = x0 + tx, y = y0 + ty;
        if (x < w && y < h) out[((size_t)f * h + y) * w + x] = acc;
    }
}
template <class... A>
static void launch_conv2(int ks, dim3 grid, hipStream_t st, A... a)
{
    switch (ks) {
    case 5: k_ov_conv2<5><<<grid, 256, 0, st>>>(a...); break;
    case 7: k_ov_conv2<7><<<grid, 256, 0, st>>>(a...); break;
    case 9: k_ov_conv2<9><<<grid, 256, 0, st>>>(a...); break;
    case 11: k_ov_conv2<11><<<grid, 256, 0, st>>>(a...); break;
    default: k_ov_conv2<0><<<grid, 256, 0, st>>>(a...); break;
    }
}

// INSIDE: the caller knows that the 3 x 3 neighbourhood lies in the image (block-uniform test): no border rule
template <bool INSIDE = false>
__device__ __forceinline__ void scharr_at(const float *I, int h, int w, int y, int x, float &gx, float &gy)
{
    const int ym = INSIDE ? y - 1 : reflect101(y - 1, h), yp = INSIDE ? y + 1 : reflect101(y + 1, h),
              xm = INSIDE ? x - 1 : reflect101(x - 1, w), xp = INSIDE ? x + 1 : reflect101(x + 1, w);
    const float a0 = I[(size_t)ym * w + xm], a1 = I[(size_t)ym * w + x], a2 = I[(size_t)ym * w + xp];
    const float b0 = I[(size_t)y * w + xm], b2 = I[(size_t)y * w + xp];
    const float c0 = I[(size_t)yp * w + xm], c1 = I[(size_t)yp * w + x], c2 = I[(size_t)yp * w + xp];
    float t0 = 3.0f * (a2 - a0), t1 = 10.0f * (b2 - b0), t2 = 3.0f * (c2 - c0);
    gx = (t0 + t1) + t2;
    t0 = 3.0f * (c0 - a0); t1 = 10.0f * (c1 - a1); t2 = 3.0f * (c2 - a2);
    gy = (t0 + t1) + t2;
}

// ---- contrast factor: 70th percentile of the gradient-magnitude histogram ------------------
// PASS 0: per-frame max (float bits as uint, values >= 0).  PASS 1: 300-bin histogram.
constexpr int KC_ROWS = 8;      // groups of four rows per block of k_ov_kc
template <int PASS>
__global__ __launch_bounds__(256) void k_ov_kc(const float *__restrict__ Lsm, int h, int w, uint32_t *__restrict__ hmax_bits,
                                              uint32_t *__restrict__ hist /*[F][304]*/)
{
    // gradient magnitudes of a smooth frame crowd into a few low bins: KC_REP copies of the histogram keyed by the lane,
    // 304 + 1 words apart (equal bins of neighbouring copies in different banks), so that one atomic instruction rarely
    // sends many lanes to one word
    constexpr int KC_REP = 8, KC_STRIDE = 305;
    __shared__ uint32_t s_hist[PASS == 1 ? KC_REP * KC_STRIDE : 1];
    const int f = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const float *I = Lsm + (size_t)f * h * w;
    if (PASS == 1) {
        for (int i = threadIdx.x; i < KC_REP * KC_STRIDE; i += 256) s_hist[i] = 0;
        __syncthreads();
    }
    const float hmax = PASS == 1 ? __uint_as_float(hmax_bits[f]) : 0.0f;
    uint32_t bmax = 0;
    // a block walks KC_ROWS groups of four rows: its 300 global atomics (one partial maximum) are paid once per 64 x 32
    // pixels -- at one group per block 900 blocks of a frame queued on the same few hundred L2 words
#pragma unroll 2
    for (int ry = 0; ry < KC_ROWS; ++ry) {
        const int y = (blockIdx.y * KC_ROWS + ry) * 4 + (threadIdx.x >> 6);
        const bool in = x >= 1 && x < w - 1 && y >= 1 && y < h - 1;
        float m = 0.0f;
        if (in) {
            float gx, gy;
            scharr_at<true>(I, h, w, y, x, gx, gy);      // in: x +- 1, y +- 1 are pixels of the image
            m = sqrtf(gx * gx + gy * gy);
        }
        if (PASS == 0) bmax = max(bmax, __float_as_uint(m));
        else if (in && m != 0.0f && hmax != 0.0f) {
            int nbin = (int)floorf(300.0f * (m / hmax));
            if (nbin >= 300) nbin = 299;
            atomicAdd(&s_hist[(threadIdx.x & (KC_REP - 1)) * KC_STRIDE + nbin], 1u);
            // npoints = the sum of the bins (k_ov_kc_final): a counter word of its own would take every lane through one address
        }
    }
    if (PASS == 0) {
        uint32_t b = bmax;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, d, 64));
        // one partial per block, reduced by k_ov_kc_max (hundreds of blocks polling one word of a frame serialise
        // on a single L2 channel; max is exact whatever the order)
        __shared__ uint32_t s_mx[4];
        if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = b;
        __syncthreads();
        if (threadIdx.x == 0)
            hist[((size_t)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = max(max(s_mx[0], s_mx[1]), max(s_mx[2], s_mx[3]));
    } else {
        __syncthreads();
        for (int i = threadIdx.x; i < 300; i += 256) {
            uint32_t c = 0;
#pragma unroll
            for (int r = 0; r < KC_REP; ++r) c += s_hist[r * KC_STRIDE + i];
            if (c) atomicAdd(&hist[(size_t)f * 304 + i], c);
        }
    }
}

__global__ __launch_bounds__(256) void k_ov_kc_max(const uint32_t *__restrict__ part, int nb, uint32_t *__restrict__ hmax_bits)
{
    __shared__ uint32_t s_mx[4];
    const int f = blockIdx.x;
    uint32_t b = 0;
    for (int i = threadIdx.x; i < nb; i += 256) b = max(b, part[(size_t)f * nb + i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, d, 64));
    if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) hmax_bits[f] = max(max(s_mx[0], s_mx[1]), max(s_mx[2], s_mx[3]));
}

__global__ void k_ov_kc_final(const uint32_t *__restrict__ hmax_bits, const uint32_t *__restrict__ hist, float *__restrict__ kc, int F)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float hmax = __uint_as_float(hmax_bits[f]);
    if (hmax == 0.0f) { kc[f] = 0.03f; return; }
    const uint32_t *hh = hist + (size_t)f * 304;
    int npoints = 0;
    for (int k = 0; k < 300; ++k) npoints += (int)hh[k];
    const int nthreshold = (int)((float)npoints * 0.7f);
    int k = 0, nelements = 0;
    for (k = 0; nelements < nthreshold && k < 300; k++) nelements += (int)hh[k];
    kc[f] = nelements < nthreshold ? 0.03f : hmax * ((float)k / 300.0f);
}

// (the Perona-Malik g2 conductivity is written by k_ov_deriv1, which reads the same smoothed plane)

// ---- explicit FED diffusion steps ---------------------------------------------------------------
// One step at one pixel: L + tau / 2 * (((xpos - xneg) + ypos) - yneg), xpos = (c + c_x+1) * (L_x+1 - L), xneg = (c_x-1 + c) *
// (L - L_x-1) and the same along y, in this order (the oracle's).  The neighbour of a pixel on the image border is the pixel
// itself (edge-clamped index).
constexpr int FD_TW = 64, FD_TH = 16;      // the output tile of a block
__device__ __forceinline__ float fed_px(float Lc, float Lxm, float Lxp, float Lym, float Lyp, float cc, float cxm, float cxp,
                                        float cym, float cyp, float step)
{
    const float xpos = (cc + cxp) * (Lxp - Lc);
    const float xneg = (cxm + cc) * (Lc - Lxm);
    const float ypos = (cc + cyp) * (Lyp - Lc);
    const float yneg = (cym + cc) * (Lc - Lym);
    float d = xpos - xneg;
    d = d + ypos;
    d = d - yneg;
    return Lc + step * d;
}

// NS consecutive FED steps in one launch (NS <= FDN_MAX): the tile + NS halo pixels of L and of the conductivity are staged
// once (edge-clamped loads), every step shrinks the valid region by one pixel, ping-ponging between two LDS planes.  A
// neighbour index is clamped INSIDE THE IMAGE before it is turned into a plane index (the border rule above), so values
// computed at out-of-image halo positions are never read.  Every output goes through fed_px NS times on the values NS
// whole-image passes of one step would give it; the planes travel through L2 / HBM once instead of NS times.
constexpr int FDN_MAX = 4;
struct FedTaus { float t[FDN_MAX]; };
template <int NS>
__global__ __launch_bounds__(256) void k_ov_fedn(const float *__restrict__ Lin, const float *__restrict__ cin, float *__restrict__ out,
                                                int h, int w, FedTaus taus)
{
    constexpr int W2 = FD_TW + 2 * NS, H2 = FD_TH + 2 * NS;
    __shared__ float s_c[H2 * W2], s_A[H2 * W2], s_B[H2 * W2];
    const int f = blockIdx.z, x0 = blockIdx.x * FD_TW - NS, y0 = blockIdx.y * FD_TH - NS;   // image coordinates of plane (0, 0)
    const float *L = Lin + (size_t)f * h * w, *c = cin + (size_t)f * h * w;
    for (int i = threadIdx.x; i < H2 * W2; i += 256) {
        const int ry = i / W2, rx = i - ry * W2;
        const int y = min(max(y0 + ry, 0), h - 1), x = min(max(x0 + rx, 0), w - 1);
        s_A[i] = L[(size_t)y * w + x];
        s_c[i] = c[(size_t)y * w + x];
    }
    __syncthreads();
    float *src = s_A, *dst = s_B;
    // a plane that lies inside the image (three tiles in four at 640 x 360) needs no border rule: neighbours are +-1, +-W2
    const bool inside = x0 >= 0 && y0 >= 0 && x0 + W2 <= w && y0 + H2 <= h;      // block-uniform
#pragma unroll
    for (int k = 1; k <= NS; ++k) {
        const float step = 0.5f * taus.t[k - 1];
        const int RW = W2 - 2 * k, RH = H2 - 2 * k;          // region of this step: plane coordinates [k, W2 - k) x [k, H2 - k)
        if (inside) {
            for (int i = threadIdx.x; i < RH * RW; i += 256) {
                const int q = i / RW;
                const int o = (q + k) * W2 + (i - q * RW) + k;
                const float v = fed_px(src[o], src[o - 1], src[o + 1], src[o - W2], src[o + W2], s_c[o], s_c[o - 1], s_c[o + 1],
                                       s_c[o - W2], s_c[o + W2], step);
                if (k < NS) dst[o] = v;
                else out[((size_t)f * h + (y0 + q + k)) * w + x0 + (i - q * RW) + k] = v;
            }
        } else
        for (int i = threadIdx.x; i < RH * RW; i += 256) {
            const int ry = i / RW + k, rx = i - (i / RW) * RW + k;
            const int x = x0 + rx, y = y0 + ry;
            const int xm = min(max(x - 1, 0), w - 1) - x0, xp = min(max(x + 1, 0), w - 1) - x0;
            const int ym = min(max(y - 1, 0), h - 1) - y0, yp = min(max(y + 1, 0), h - 1) - y0;
            // an out-of-image position has its neighbour indices clamped onto in-plane positions as well (|delta| <= 1 from
            // a clamped coordinate): harmless, its value is never used
            const int o = ry * W2 + rx;
            const int oxm = ry * W2 + min(max(xm, 0), W2 - 1), oxp = ry * W2 + min(max(xp, 0), W2 - 1);
            const int oym = min(max(ym, 0), H2 - 1) * W2 + rx, oyp = min(max(yp, 0), H2 - 1) * W2 + rx;
            const float v = fed_px(src[o], src[oxm], src[oxp], src[oym], src[oyp], s_c[o], s_c[oxm], s_c[oxp], s_c[oym], s_c[oyp], step);
            if (k < NS) dst[o] = v;
            else if (x < w && y < h) out[((size_t)f * h + y) * w + x] = v;   // k == NS: the region is the tile itself
        }
        if (k < NS) {
            __syncthreads();
            float *t = src; src = dst; dst = t;
        }
    }
}

// ---- scale-s first derivative (taps at -s, 0, +s) ------------------------------------------------
template <bool INSIDE = false>
__device__ __forceinline__ float deriv_at(const float *I, int h, int w, int y, int x, int s, bool along_x)
{
    const float wgt = 10.0f / 3.0f;
    const float norm = 1.0f / (2.0f * (float)s * (wgt + 2.0f));
    const float wn = wgt * norm;
    const int ym = INSIDE ? y - s : reflect101(y - s, h), yp = INSIDE ? y + s : reflect101(y + s, h);
    const int xm = INSIDE ? x - s : reflect101(x - s, w), xp = INSIDE ? x + s : reflect101(x + s, w);
    float t0, t1, t2;
    if (along_x) {
        t0 = norm * (I[(size_t)ym * w + xp] - I[(size_t)ym * w + xm]);
        t1 = wn * (I[(size_t)y * w + xp] - I[(size_t)y * w + xm]);
        t2 = norm * (I[(size_t)yp * w + xp] - I[(size_t)yp * w + xm]);
    } else {
        t0 = norm * (I[(size_t)yp * w + xm] - I[(size_t)ym * w + xm]);
        t1 = wn * (I[(size_t)yp * w + x] - I[(size_t)ym * w + x]);
        t2 = norm * (I[(size_t)yp * w + xp] - I[(size_t)ym * w + xp]);
    }
    return (t0 + t1) + t2;
}

// also writes the Perona-Malik conductivity of the same smoothed plane when `flow` is given (k_ov_flow's arithmetic: the
// two kernels read the same plane, one launch and one read of it instead of two)
__global__ __launch_bounds__(256) void k_ov_deriv1(const float *__restrict__ Lsm, float2 *__restrict__ Lxy, int h, int w, int s,
                                                  const float *__restrict__ kc, float *__restrict__ flow)
{
    const int f = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const float *I = Lsm + (size_t)f * h * w;
    const size_t o = ((size_t)f * h + y) * w + x;
    // block-uniform: every tap of the block's 64 x 4 pixels lies in the image (s >= 1 covers the Scharr taps too)
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    const bool inside = bx0 - s >= 0 && bx0 + 63 + s < w && by0 - s >= 0 && by0 + 3 + s < h;
    float gx, gy;
    // (Lx, Ly) as ONE float2 plane: k_ov_ldet and k_ov_describe want both at the same positions -- one gather instead of two
    if (inside) {
        Lxy[o] = make_float2(deriv_at<true>(I, h, w, y, x, s, true), deriv_at<true>(I, h, w, y, x, s, false));
        if (flow) scharr_at<true>(I, h, w, y, x, gx, gy);
    } else {
        Lxy[o] = make_float2(deriv_at(I, h, w, y, x, s, true), deriv_at(I, h, w, y, x, s, false));
        if (flow) scharr_at(I, h, w, y, x, gx, gy);
    }
    if (flow) {
        const float k = kc[f];
        const float inv_k = 1.0f / (k * k);
        flow[o] = 1.0f / (1.0f + (gx * gx + gy * gy) * inv_k);
    }
}

// second derivatives of one pixel from the (Lx, Ly) plane: Lxx = d/dx of Lx, Lyy = d/dy of Ly, Lxy = d/dy of Lx -- deriv_at's
// operations on eight float2 taps (the four corner taps serve all three, the two d/dy centre taps serve Lyy and Lxy)
template <bool INSIDE>
__device__ __forceinline__ void second_derivs(const float2 *P, int h, int w, int y, int x, int s, float &lxx, float &lyy, float &lxy)
{
    const float wgt = 10.0f / 3.0f;
    const float norm = 1.0f / (2.0f * (float)s * (wgt + 2.0f));
    const float wn = wgt * norm;
    const int ym = INSIDE ? y - s : reflect101(y - s, h), yp = INSIDE ? y + s : reflect101(y + s, h);
    const int xm = INSIDE ? x - s : reflect101(x - s, w), xp = INSIDE ? x + s : reflect101(x + s, w);
    const float2 mm = P[(size_t)ym * w + xm], m0 = P[(size_t)ym * w + x], mp = P[(size_t)ym * w + xp];
    const float2 zm = P[(size_t)y * w + xm], zp = P[(size_t)y * w + xp];
    const float2 pm = P[(size_t)yp * w + xm], p0 = P[(size_t)yp * w + x], pp = P[(size_t)yp * w + xp];
    float t0 = norm * (mp.x - mm.x), t1 = wn * (zp.x - zm.x), t2 = norm * (pp.x - pm.x);
    lxx = (t0 + t1) + t2;
    t0 = norm * (pm.y - mm.y); t1 = wn * (p0.y - m0.y); t2 = norm * (pp.y - mp.y);
    lyy = (t0 + t1) + t2;
    t0 = norm * (pm.x - mm.x); t1 = wn * (p0.x - m0.x); t2 = norm * (pp.x - mp.x);
    lxy = (t0 + t1) + t2;
}
__global__ __launch_bounds__(256) void k_ov_ldet(const float2 *__restrict__ Lxy, float *__restrict__ Ldet, int h, int w, int s)
{
    const int f = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const float2 *P = Lxy + (size_t)f * h * w;
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    const bool inside = bx0 - s >= 0 && bx0 + 63 + s < w && by0 - s >= 0 && by0 + 3 + s < h;     // block-uniform
    float lxx, lyy, lxy;
    if (inside) second_derivs<true>(P, h, w, y, x, s, lxx, lyy, lxy);
    else second_derivs<false>(P, h, w, y, x, s, lxx, lyy, lxy);
    const float ss = (float)(s * s), s4 = ss * ss;
    Ldet[((size_t)f * h + y) * w + x] = (lxx * lyy - lxy * lxy) * s4;
}

// ---- extrema: candidate response map over all levels ------------------------------------------------
// Ldet: [NLEV][F][h][w] (each level a dense batch); cand: [F][NLEV][h][w], response or 0
// The detector threshold is relative to the frame's contrast factor k (det of the Hessian scales with contrast squared;
// raw frames of turbid water have no response above a fixed 1e-3): DTHRESH * min(1, (k / KC_REF)^2), in the oracle's
// operations (UWIP_OVERLAP_RELATIVE_THRESHOLD); `fixed` keeps DTHRESH (the default).
// One block = a 64 x 8 tile of ALL levels: the four level tiles + 1 halo pixel are staged in LDS once (coalesced rows), and
// every comparison of the 3 x 3 x 3 test and the sub-pixel check reads LDS -- the dense map of every level is read once
// (x 1.29 for the halo) instead of once plus 26 scattered neighbour loads wherever any lane of a wave passes the threshold.
constexpr int EX_TW = 64, EX_TH = 8, EX_PW = EX_TW + 2, EX_PH = EX_TH + 2;
__global__ __launch_bounds__(256) void k_ov_extrema(const float *__restrict__ Ldet, float *__restrict__ cand, int h, int w, int F,
                                                   const float *__restrict__ kc, int fixed, uint32_t *__restrict__ selhist)
{
    __shared__ float s_D[NLEV][EX_PH * EX_PW];
    const int f = blockIdx.z, x0 = blockIdx.x * EX_TW, y0 = blockIdx.y * EX_TH;
    const size_t n = (size_t)h * w;
    for (int i = threadIdx.x; i < EX_PH * EX_PW; i += 256) {
        const int ry = i / EX_PW, rx = i - ry * EX_PW;
        const int gy = y0 - 1 + ry, gx = x0 - 1 + rx;
        const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;       // positions outside are never compared (BORDER >= 1)
#pragma unroll
        for (int lv = 0; lv < NLEV; ++lv) s_D[lv][i] = in ? Ldet[((size_t)lv * F + f) * n + (size_t)gy * w + gx] : 0.0f;
    }
    __syncthreads();
    const float kr = kc[f] / KC_REF;
    float ks = kr * kr;
    if (!(ks < 1.0f)) ks = 1.0f;
    const float dthr = fixed ? DTHRESH : DTHRESH * ks;
    const int tx = threadIdx.x & 63, x = x0 + tx;
#pragma unroll
    for (int k = 0; k < EX_TH / 4; ++k) {
        const int ty = (threadIdx.x >> 6) + 4 * k, y = y0 + ty;
        if (x >= w || y >= h) continue;
        const bool inb = x >= BORDER && x < w - BORDER && y >= BORDER && y < h - BORDER;
        const int c = (ty + 1) * EX_PW + tx + 1;
#pragma unroll
        for (int lv = 0; lv < NLEV; ++lv) {
            const float *D = s_D[lv];
            float out = 0.0f;
            const float v = D[c];
            bool ok = inb && v > dthr;
            if (ok) {
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx)
                        if ((dx != 0 || dy != 0) && !(v > D[c + dy * EX_PW + dx])) ok = false;
            }
            if (ok) {
#pragma unroll
                for (int o = -1; o <= 1; o += 2) {
                    const int l2 = lv + o;
                    if (l2 < 0 || l2 >= NLEV) continue;
                    const float *E = s_D[l2];
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx)
                            if (!(v > E[c + dy * EX_PW + dx])) ok = false;
                }
            }
            if (ok) {
                // candidates that the sub-pixel refinement would discard are dropped here, so that
                // the top-K selection sees exactly the oracle's candidate list
                const float vxp = D[c + 1], vxm = D[c - 1];
                const float vyp = D[c + EX_PW], vym = D[c - EX_PW];
                const float Dx = 0.5f * (vxp - vxm), Dy = 0.5f * (vyp - vym);
                const float Dxx = (vxp + vxm) - 2.0f * v, Dyy = (vyp + vym) - 2.0f * v;
                const float Dxy = 0.25f * (D[c + EX_PW + 1] + D[c - EX_PW - 1]) - 0.25f * (D[c + EX_PW - 1] + D[c - EX_PW + 1]);
                const float det = Dxx * Dyy - Dxy * Dxy;
                if (det == 0.0f) ok = false;
                else {
                    const float ox = -(Dyy * Dx - Dxy * Dy) / det, oy = -(Dxx * Dy - Dxy * Dx) / det;
                    if (!(fabsf(ox) <= 1.0f && fabsf(oy) <= 1.0f)) ok = false;
                }
                if (ok) {
                    out = v;
                    // first pass of the top-K radix select (k_ov_sel_hist<0>'s histogram of the high 16 response bits) counted
                    // here: candidates are a few thousand per frame, and the dense map is read once less
                    atomicAdd(&selhist[(size_t)f * 65536 + (__float_as_uint(v) >> 16)], 1u);
                }
            }
            cand[((size_t)f * NLEV + lv) * n + (size_t)y * w + x] = out;
        }
    }
}

// ---- top-K selection: 2-pass radix select on the float bit patterns ---------------------------------
// hist: [F][65536]; sel: [F][4] = {prefix, remaining, total, threshold_bits}
template <int PASS>
__global__ __launch_bounds__(256) void k_ov_sel_hist(const float *__restrict__ cand, size_t n4, uint32_t *__restrict__ hist,
                                                    const uint32_t *__restrict__ sel)
{
    const int f = blockIdx.y;
    const float *c = cand + (size_t)f * n4;
    const uint32_t prefix = PASS == 1 ? sel[(size_t)f * 4] : 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const uint32_t b = __float_as_uint(c[i]);
        if (b == 0) continue;
        if (PASS == 1 && (b >> 16) != prefix) continue;
        atomicAdd(&hist[(size_t)f * 65536 + (PASS == 0 ? (b >> 16) : (b & 0xffffu))], 1u);
    }
}

// one block per frame: walk the 65536 bins from the top until `remaining` candidates are covered
template <int PASS>
__global__ __launch_bounds__(256) void k_ov_sel_pick(const uint32_t *__restrict__ hist, uint32_t *__restrict__ sel)
{
    __shared__ uint32_t s_sum[256];
    __shared__ uint32_t s_scratch[8];
    const int f = blockIdx.x, t = threadIdx.x;
    const uint32_t *hh = hist + (size_t)f * 65536;
    // thread t owns bins [65535 - 256 t - 255, 65535 - 256 t] (descending order across threads)
    uint32_t mine = 0;
    const int top = 65535 - 256 * t;
    for (int b = top; b > top - 256; --b) mine += hh[b];
    const uint32_t incl = block256_incl_scan_u32(mine, s_scratch);
    s_sum[t] = incl;
    __syncthreads();
    uint32_t *s = sel + (size_t)f * 4;
    const uint32_t total = s_sum[255];
    uint32_t remaining = PASS == 0 ? (uint32_t)MAXKP : s[1];
    if (PASS == 0 && t == 0) s[2] = total;
    if (PASS == 0 && total <= (uint32_t)MAXKP) {
        if (t == 0) { s[0] = 0; s[1] = 0; s[3] = 1u; }      // accept every candidate (bits >= 1)
        return;
    }
    if (PASS == 1 && s[3] == 1u && s[2] <= (uint32_t)MAXKP) return;
    const uint32_t before = incl - mine;
    if (before < remaining && incl >= remaining) {
        // the K-th strongest lies in this thread's 256 bins
        uint32_t acc = before;
        int b = top;
        for (; b > top - 256; --b) {
            if (acc + hh[b] >= remaining) break;
            acc += hh[b];
        }
        if (PASS == 0) { s[0] = (uint32_t)b; s[1] = remaining - acc; }
        else { s[3] = (s[0] << 16) | (uint32_t)b; }
    }
}

// ---- ordered compaction + sub-pixel refinement ---------------------------------------------------------
constexpr int CMP_CHUNK = 1024;
// One WAVE per chunk of CMP_CHUNK map entries (ballot + popcount: no LDS, no barrier)
__global__ __launch_bounds__(256) void k_ov_count(const float *__restrict__ cand, size_t n4, const uint32_t *__restrict__ sel,
                                                 uint32_t *__restrict__ counts, int nchunks)
{
    const int f = blockIdx.y, ch = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ch >= nchunks) return;
    const uint32_t thr = sel[(size_t)f * 4 + 3];
    const float *c = cand + (size_t)f * n4;
    uint32_t tot = 0;
#pragma unroll 4
    for (int k = 0; k < CMP_CHUNK / 64; ++k) {
        const size_t i = (size_t)ch * CMP_CHUNK + (size_t)k * 64 + lane;
        bool flag = false;
        if (i < n4) {
            const uint32_t b = __float_as_uint(c[i]);
            flag = b != 0 && b >= thr;
        }
        tot += (uint32_t)__popcll(__ballot(flag));
    }
    if (lane == 0) counts[(size_t)f * nchunks + ch] = tot;
}

__global__ __launch_bounds__(256) void k_ov_scan_chunks(uint32_t *__restrict__ counts, int nchunks, int32_t *__restrict__ nkp)
{
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t carry;
    const int f = blockIdx.x;
    uint32_t *c = counts + (size_t)f * nchunks;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nchunks; base += 256) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < nchunks ? c[i] : 0u;
        const uint32_t incl = block256_incl_scan_u32(v, scratch);
        const uint32_t off = carry;
        if (i < nchunks) c[i] = off + incl - v;       // exclusive offset
        __syncthreads();
        if (threadIdx.x == 255) carry = off + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) nkp[f] = (int32_t)min(carry, (uint32_t)MAXKP);
}

__global__ __launch_bounds__(256) void k_ov_compact(const float *__restrict__ cand, const float *__restrict__ Ldet, int h, int w,
                                                   const uint32_t *__restrict__ sel, const uint32_t *__restrict__ offsets,
                                                   int nchunks, Keypoint *__restrict__ kps, int F)
{
    const int f = blockIdx.y, ch = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ch >= nchunks) return;
    const size_t n = (size_t)h * w, n4 = n * NLEV;
    const uint32_t thr = sel[(size_t)f * 4 + 3];
    const float *c = cand + (size_t)f * n4;
    uint32_t base = offsets[(size_t)f * nchunks + ch];          // wave-uniform: entries selected before this chunk
    for (int k = 0; k < CMP_CHUNK / 64 && base < (uint32_t)MAXKP; ++k) {
        const size_t i = (size_t)ch * CMP_CHUNK + (size_t)k * 64 + lane;
        bool flag = false;
        float v = 0.0f;
        if (i < n4) {
            v = c[i];
            const uint32_t b = __float_as_uint(v);
            flag = b != 0 && b >= thr;
        }
        const unsigned long long mask = __ballot(flag);
        const uint32_t pos = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        base += (uint32_t)__popcll(mask);
        if (flag && pos < (uint32_t)MAXKP) {
            const int lv = (int)(i / n);
            const size_t r = i - (size_t)lv * n;
            const int y = (int)(r / w), x = (int)(r - (size_t)y * w);
            const float *D = Ldet + ((size_t)lv * F + f) * n;
            const float vxp = D[(size_t)y * w + x + 1], vxm = D[(size_t)y * w + x - 1];
            const float vyp = D[(size_t)(y + 1) * w + x], vym = D[(size_t)(y - 1) * w + x];
            const float Dx = 0.5f * (vxp - vxm), Dy = 0.5f * (vyp - vym);
            const float Dxx = (vxp + vxm) - 2.0f * v, Dyy = (vyp + vym) - 2.0f * v;
            const float Dxy = 0.25f * (D[(size_t)(y + 1) * w + x + 1] + D[(size_t)(y - 1) * w + x - 1]) -
                              0.25f * (D[(size_t)(y + 1) * w + x - 1] + D[(size_t)(y - 1) * w + x + 1]);
            const float det = Dxx * Dyy - Dxy * Dxy;
            const float ox = -(Dyy * Dx - Dxy * Dy) / det, oy = -(Dxx * Dy - Dxy * Dx) / det;
            Keypoint kp;
            kp.x = (float)x + ox; kp.y = (float)y + oy; kp.response = v;
            kp.level = lv; kp.xi = x; kp.yi = y; kp.co = 1.0f; kp.si = 0.0f;
            kps[(size_t)f * MAXKP + pos] = kp;
        }
    }
}

// ---- V5 calcBlur: gray -> Laplacian (aperture 3, saturated to u8) -> population stddev ---------------------------
__global__ __launch_bounds__(256) void k_ov_blur(const uint8_t *__restrict__ gray, int h, int w, double *__restrict__ part /*[F][nb][2]*/)
{
    __shared__ double scratch[8];
    const int f = blockIdx.y;
    const uint8_t *g = gray + (size_t)f * h * w;
    const size_t n = (size_t)h * w;
    double s = 0.0, s2 = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i - (size_t)y * w);
        const int ym = reflect101(y - 1, h), yp = reflect101(y + 1, h), xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
        int v = 2 * (g[(size_t)ym * w + xm] + g[(size_t)ym * w + xp] + g[(size_t)yp * w + xm] + g[(size_t)yp * w + xp]) - 8 * g[(size_t)y * w + x];
        v = min(max(v, 0), 255);
        s += v; s2 += (double)v * v;
    }
    // integer-valued sums: exact in double, so the reduction order is immaterial
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s = wave_sum_f64(s); s2 = wave_sum_f64(s2);
    if (lane == 0) { scratch[wave] = s; scratch[4 + wave] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = part + ((size_t)f * gridDim.x + blockIdx.x) * 2;
        o[0] = scratch[0] + scratch[1] + scratch[2] + scratch[3];
        o[1] = scratch[4] + scratch[5] + scratch[6] + scratch[7];
    }
}

__global__ void k_ov_blur_final(const double *__restrict__ part, int nb, double npix, float *__restrict__ out, int F)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double s = 0, s2 = 0;
    for (int k = 0; k < nb; ++k) { s += part[((size_t)f * nb + k) * 2]; s2 += part[((size_t)f * nb + k) * 2 + 1]; }
    const double mean = s / npix;
    const double var = s2 / npix - mean * mean;
    out[f] = (float)sqrt(var < 0 ? 0 : var);
}

// ---- host side: filter taps, FED step sizes, resize tables, workspaces, the launch sequence ---------------------------------
ConvK gauss_kernel(float sigma)
{
    ConvK K{};
    int ks = (int)std::ceil(2.0 * (1.0 + ((double)sigma - 0.8) / 0.3));
    if ((ks & 1) == 0) ks++;
    const int r = ks / 2;
    double sum = 0, tmp[32];
    for (int i = 0; i < ks; ++i) { tmp[i] = std::exp(-((double)(i - r) * (i - r)) / (2.0 * (double)sigma * (double)sigma)); sum += tmp[i]; }
    K.ks = ks;
    for (int i = 0; i < ks; ++i) K.k[i] = (float)(tmp[i] / sum);
    return K;
}

int fed_taus(float T, float *tau)
{
    const double tau_max = 0.25;
    int n = (int)(std::ceil(std::sqrt(3.0 * (double)T / tau_max + 0.25) - 0.5 - 1.0e-8) + 0.5);
    if (n < 1) n = 1;
    const double scale = 3.0 * (double)T / (tau_max * (double)(n * (n + 1)));
    const double c = 1.0 / (4.0 * (double)n + 2.0), d = scale * tau_max / 2.0;
    for (int k = 0; k < n; ++k) {
        const double hh = std::cos(3.14159265358979323846 * (2.0 * (double)k + 1.0) * c);
        tau[k] = (float)(d / (hh * hh));
    }
    return n;
}

void resize_dims(int rows, int cols, int target_w, int *orows, int *ocols)
{
    const float f = (float)target_w / (float)cols;                 // hResizeFactor (main.cpp:242)
    *ocols = (int)std::lrint((double)cols * (double)f);
    *orows = (int)std::lrint((double)rows * (double)f);
}

struct ResizeTab {
    std::vector<int> ofs;
    std::vector<short> c0, c1;
};

void resize_tab(int ssize, int dsize, ResizeTab &t)
{
    t.ofs.resize(dsize); t.c0.resize(dsize); t.c1.resize(dsize);
    const double scale = 1.0 / ((double)dsize / (double)ssize);
    for (int d = 0; d < dsize; ++d) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        int sx = (int)std::floor(fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= ssize - 1) { fx = 0; sx = ssize - 1; }
        t.ofs[d] = sx;
        const long r0 = std::lrintf((1.0f - fx) * 2048.0f), r1 = std::lrintf(fx * 2048.0f);
        t.c0[d] = (short)std::min<long>(r0, 32767);
        t.c1[d] = (short)std::min<long>(r1, 32767);
    }
}

// device table: [ofs int32 x d][c0 int16 x d][c1 int16 x d]
const void *resize_table(uwip_ctx *ctx, int ssize, int dsize)
{
    char key[64];
    snprintf(key, sizeof key, "resize:%d:%d", ssize, dsize);
    const void *d = uwip_table_find(ctx, key, nullptr);
    if (d) return d;
    ResizeTab t;
    resize_tab(ssize, dsize, t);
    std::vector<uint8_t> buf((size_t)dsize * 8);
    memcpy(buf.data(), t.ofs.data(), (size_t)dsize * 4);
    memcpy(buf.data() + (size_t)dsize * 4, t.c0.data(), (size_t)dsize * 2);
    memcpy(buf.data() + (size_t)dsize * 6, t.c1.data(), (size_t)dsize * 2);
    return uwip_table_put(ctx, key, buf.data(), buf.size());
}

dim3 grid2d(int w, int h, int z) { return dim3(uwip_cdiv(w, 64), uwip_cdiv(h, 4), (unsigned)z); }

struct OvWork {
    uint8_t *gray;
    float *L0, *Lsm, *flow, *ping, *Lt, *Ldet, *cand, *kc;
    float2 *Lxy;       // (Lx, Ly) interleaved, [NLEV][F][h][w]
    uint32_t *hmax, *khist, *selhist, *sel, *counts;
};

int alloc_work(uwip_ctx *ctx, int F, int h, int w, OvWork *W)
{
    const size_t n = (size_t)h * w;
    const int nchunks = (int)((n * NLEV + CMP_CHUNK - 1) / CMP_CHUNK);
    W->gray = (uint8_t *)uwip_ws(ctx, "ov.gray", n * F);
    W->L0 = (float *)uwip_ws(ctx, "ov.L0", n * F * 4);
    W->Lsm = (float *)uwip_ws(ctx, "ov.Lsm", n * F * 4);
    W->flow = (float *)uwip_ws(ctx, "ov.flow", n * F * 4);
    W->ping = (float *)uwip_ws(ctx, "ov.ping", n * F * 4);
    W->Lt = (float *)uwip_ws(ctx, "ov.Lt", n * F * 4 * NLEV);
    W->Lxy = (float2 *)uwip_ws(ctx, "ov.Lxy", n * F * 8 * NLEV);
    W->Ldet = (float *)uwip_ws(ctx, "ov.Ldet", n * F * 4 * NLEV);
    W->cand = (float *)uwip_ws(ctx, "ov.cand", n * F * 4 * NLEV);
    W->kc = (float *)uwip_ws(ctx, "ov.kc", sizeof(float) * F);
    W->hmax = (uint32_t *)uwip_ws(ctx, "ov.hmax", sizeof(uint32_t) * F);
    W->khist = (uint32_t *)uwip_ws(ctx, "ov.khist", sizeof(uint32_t) * 304 * F);
    W->selhist = (uint32_t *)uwip_ws(ctx, "ov.selhist", sizeof(uint32_t) * 65536 * F);
    W->sel = (uint32_t *)uwip_ws(ctx, "ov.sel", sizeof(uint32_t) * 4 * F);
    W->counts = (uint32_t *)uwip_ws(ctx, "ov.counts", sizeof(uint32_t) * nchunks * F);
    if (!W->gray || !W->L0 || !W->Lsm || !W->flow || !W->ping || !W->Lt || !W->Lxy || !W->Ldet || !W->cand ||
        !W->kc || !W->hmax || !W->khist || !W->selhist || !W->sel || !W->counts)
        return UWIP_ERR_NOMEM;
    return UWIP_OK;
}

// Level images are stored level-major, [NLEV][F][h][w]: every level is itself a dense batch, so the per-level
// kernels write their results in place (no staging copies).
// detect + describe every frame whose gray/L0 already sit in W (working size h x w)
int detect_describe(uwip_ctx *ctx, OvWork &W, int F, int h, int w, uwip_features *ft, int first_slot, int upright, int fixed_thr)
{
    const size_t n = (size_t)h * w, lvl = n * F;
    const dim3 g = grid2d(w, h, F);
    ctx->ov_last_frames = F;
    {
        uwip_kscope ks(ctx, "k_ov_scale_space");
        const ConvK K0 = gauss_kernel(H_SIGMA[0]), K1 = gauss_kernel(1.0f);
        UWIP_REQUIRE(ctx, K0.ks / 2 <= CV_RMAX && K1.ks / 2 <= CV_RMAX && (K0.ks & 1) && (K1.ks & 1), "Gaussian kernel too wide for k_ov_conv2");
        const dim3 gc(uwip_cdiv(w, CV_TW), uwip_cdiv(h, CV_TH), (unsigned)F);
        launch_conv2(K0.ks, gc, ctx->stream, (const float *)W.L0, W.Lt, h, w, K0);
        for (int lv = 0; lv < NLEV; ++lv) {
            float *Lt = W.Lt + lv * lvl;
            launch_conv2(K1.ks, gc, ctx->stream, (const float *)Lt, W.Lsm, h, w, K1);
            if (lv == 0) {
                const dim3 gk(g.x, uwip_cdiv(g.y, KC_ROWS), g.z);
                const int nbk = (int)(gk.x * gk.y);
                uint32_t *kpart = (uint32_t *)uwip_ws(ctx, "ov.kcpart", sizeof(uint32_t) * nbk * F);
                if (!kpart) return UWIP_ERR_NOMEM;
                k_ov_kc<0><<<gk, 256, 0, ctx->stream>>>(W.Lsm, h, w, W.hmax, kpart);
                k_ov_kc_max<<<F, 256, 0, ctx->stream>>>(kpart, nbk, W.hmax);
                UWIP_HIP(ctx, hipMemsetAsync(W.khist, 0, sizeof(uint32_t) * 304 * F, ctx->stream));
                k_ov_kc<1><<<gk, 256, 0, ctx->stream>>>(W.Lsm, h, w, W.hmax, W.khist);
                k_ov_kc_final<<<uwip_cdiv(F, 64), 64, 0, ctx->stream>>>(W.hmax, W.khist, W.kc, F);
            }
            const int s = H_SSIZE[lv];
            k_ov_deriv1<<<g, 256, 0, ctx->stream>>>(W.Lsm, W.Lxy + lv * lvl, h, w, s, W.kc, lv + 1 < NLEV ? W.flow : nullptr);
            k_ov_ldet<<<g, 256, 0, ctx->stream>>>(W.Lxy + lv * lvl, W.Ldet + lv * lvl, h, w, s);
            if (lv + 1 < NLEV) {
                const float e0 = 0.5f * H_SIGMA[lv] * H_SIGMA[lv], e1 = 0.5f * H_SIGMA[lv + 1] * H_SIGMA[lv + 1];
                float taus[32];
                const int nt = fed_taus(e1 - e0, taus);
                // up to FDN_MAX steps per launch, split as evenly as possible (8 -> 4 + 4, 6 -> 3 + 3, 4 -> 4); ping-pong
                // between Lt[lv+1] and a scratch plane so that the last launch lands in Lt[lv+1]
                float *next = W.Lt + (lv + 1) * lvl;
                const float *src = Lt;
                const int nl = (nt + FDN_MAX - 1) / FDN_MAX;
                const dim3 gf(uwip_cdiv(w, FD_TW), uwip_cdiv(h, FD_TH), (unsigned)F);
                for (int j = 0, k = 0; j < nl; ++j) {
                    float *dst = ((nl - j) & 1) ? next : W.ping;
                    const int ns = (nt - k + (nl - j) - 1) / (nl - j);
                    FedTaus tk;
                    for (int q = 0; q < FDN_MAX; ++q) tk.t[q] = q < ns ? taus[k + q] : 0.0f;
                    // H_SIGMA's three transitions take 4, 6 and 8 steps: only these two sizes occur.  Another sigma table wants
                    // its own instantiation, not k_ov_fedn<4> with padded zero taus.
                    UWIP_REQUIRE(ctx, ns == 3 || ns == 4, "no k_ov_fedn instantiation for this number of FED steps per launch");
                    if (ns == 3) k_ov_fedn<3><<<gf, 256, 0, ctx->stream>>>(src, W.flow, dst, h, w, tk);
                    else k_ov_fedn<4><<<gf, 256, 0, ctx->stream>>>(src, W.flow, dst, h, w, tk);
                    k += ns;
                    src = dst;
                }
            }
        }
        UWIP_HIP(ctx, hipGetLastError());
    }
    const size_t n4 = n * NLEV;
    const int nchunks = (int)((n4 + CMP_CHUNK - 1) / CMP_CHUNK);
    Keypoint *kps = ft->d_kp + (size_t)first_slot * MAXKP;
    int32_t *nkp = ft->d_n + first_slot;
    {
        uwip_kscope ks(ctx, "k_ov_detect");
        UWIP_HIP(ctx, hipMemsetAsync(W.selhist, 0, sizeof(uint32_t) * 65536 * F, ctx->stream));
        k_ov_extrema<<<dim3(uwip_cdiv(w, EX_TW), uwip_cdiv(h, EX_TH), (unsigned)F), 256, 0, ctx->stream>>>(W.Ldet, W.cand, h, w, F, W.kc, fixed_thr, W.selhist);
        k_ov_sel_pick<0><<<F, 256, 0, ctx->stream>>>(W.selhist, W.sel);
        UWIP_HIP(ctx, hipMemsetAsync(W.selhist, 0, sizeof(uint32_t) * 65536 * F, ctx->stream));
        k_ov_sel_hist<1><<<dim3(64, F), 256, 0, ctx->stream>>>(W.cand, n4, W.selhist, W.sel);
        k_ov_sel_pick<1><<<F, 256, 0, ctx->stream>>>(W.selhist, W.sel);
        k_ov_count<<<dim3(uwip_cdiv(nchunks, 4), F), 256, 0, ctx->stream>>>(W.cand, n4, W.sel, W.counts, nchunks);
        k_ov_scan_chunks<<<F, 256, 0, ctx->stream>>>(W.counts, nchunks, nkp);
        k_ov_compact<<<dim3(uwip_cdiv(nchunks, 4), F), 256, 0, ctx->stream>>>(W.cand, W.Ldet, h, w, W.sel, W.counts, nchunks, kps, F);
        UWIP_HIP(ctx, hipGetLastError());
    }
    return uwip_overlap_describe(ctx, W.Lt, W.Lxy, h, w, F, ft, first_slot, upright);
}

}  // namespace

UWIP_API int uwip_overlap_working_size(int rows, int cols, int *orows, int *ocols)
{
    if (!orows || !ocols || rows <= 0 || cols <= 0) return UWIP_ERR_INVALID;
    resize_dims(rows, cols, TW, orows, ocols);
    return UWIP_OK;
}

// frames: full-resolution BGR (resized to 640 wide inside, main.cpp:242,311) or, when `already_gray`
// is set, 8UC1 planes already at the working size.  Fills slots [first_slot, first_slot+frames).
UWIP_API int uwip_overlap_detect(uwip_ctx *ctx, const uwip_batch_u8 *frames, uwip_features *feats, int first_slot)
{
    return uwip_overlap_detect_ex(ctx, frames, feats, first_slot, 0u);
}

UWIP_API int uwip_overlap_detect_ex(uwip_ctx *ctx, const uwip_batch_u8 *frames, uwip_features *feats, int first_slot, unsigned flags)
{
    int rc = uwip_check_batch(ctx, frames, 0);
    if (rc) return rc;
    UWIP_REQUIRE(ctx, (flags & ~(unsigned)(UWIP_OVERLAP_UPRIGHT | UWIP_OVERLAP_FIXED_THRESHOLD | UWIP_OVERLAP_RELATIVE_THRESHOLD)) == 0, "unknown flag");
    UWIP_REQUIRE(ctx, (flags & (UWIP_OVERLAP_FIXED_THRESHOLD | UWIP_OVERLAP_RELATIVE_THRESHOLD)) != (UWIP_OVERLAP_FIXED_THRESHOLD | UWIP_OVERLAP_RELATIVE_THRESHOLD),
                 "UWIP_OVERLAP_FIXED_THRESHOLD and UWIP_OVERLAP_RELATIVE_THRESHOLD exclude each other");
    UWIP_REQUIRE(ctx, feats != nullptr && feats->ctx == ctx, "feature set belongs to another context");
    UWIP_REQUIRE(ctx, first_slot >= 0 && first_slot + frames->frames <= feats->capacity, "feature set too small");
    if (frames->frames == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, !uwip_batch_empty(frames), "empty image");           // calcOverlap returns -1 there
    const int F = frames->frames;
    int h, w;
    if (frames->channels == 3) resize_dims(frames->rows, frames->cols, TW, &h, &w);
    else { h = frames->rows; w = frames->cols; }
    UWIP_REQUIRE(ctx, h >= 2 * BORDER + 3 && w >= 2 * BORDER + 3, "working image too small");
    UWIP_REQUIRE(ctx, feats->w == 0 || (feats->w == w && feats->h == h), "feature set holds frames of another size");
    OvWork W;
    rc = alloc_work(ctx, F, h, w, &W);
    if (rc) return rc;
    const size_t n = (size_t)h * w;
    if (frames->channels == 3) {
        const uint8_t *tx = (const uint8_t *)resize_table(ctx, frames->cols, w);
        const uint8_t *ty = (const uint8_t *)resize_table(ctx, frames->rows, h);
        if (!tx || !ty) return UWIP_ERR_NOMEM;
        uwip_kscope ks(ctx, "k_ov_resize_gray");
        k_ov_resize_gray<<<grid2d(w, h, F), 256, 0, ctx->stream>>>(
            (const uint8_t *)frames->data, frames->step, frames->frame_stride, frames->rows, frames->cols, h, w,
            (const int *)tx, (const short *)(tx + (size_t)w * 4), (const short *)(tx + (size_t)w * 6),
            (const int *)ty, (const short *)(ty + (size_t)h * 4), (const short *)(ty + (size_t)h * 6), W.gray, W.L0);
        UWIP_HIP(ctx, hipGetLastError());
    } else {
        for (int f = 0; f < F; ++f)
            UWIP_HIP(ctx, hipMemcpy2DAsync(W.gray + (size_t)f * n, (size_t)w, (const uint8_t *)frames->data + (size_t)f * frames->frame_stride,
                                           frames->step, (size_t)w, (size_t)h, hipMemcpyDeviceToDevice, ctx->stream));
        k_ov_gray_to_L0<<<uwip_cdiv(n * F, 256), 256, 0, ctx->stream>>>(W.gray, W.L0, n * F);
        UWIP_HIP(ctx, hipGetLastError());
    }
    feats->w = w; feats->h = h;
    feats->frames = std::max(feats->frames, first_slot + F);
    return detect_describe(ctx, W, F, h, w, feats, first_slot, (flags & UWIP_OVERLAP_UPRIGHT) ? 1 : 0,
                           (flags & UWIP_OVERLAP_RELATIVE_THRESHOLD) ? 0 : 1);
}

// scale-space tap for tests: level images of slot-0 work buffers after the last detect call
UWIP_API int uwip_overlap_debug_level(uwip_ctx *ctx, int frame, int level, int rows, int cols, float *h_Lt, float *h_Lx,
                                      float *h_Ly, float *h_Ldet, float *h_kcontrast)
{
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, level >= 0 && level < NLEV && frame >= 0, "bad level/frame");
    const size_t n = (size_t)rows * cols;
    auto get = [&](const char *name) -> float * {
        auto it = ctx->ws.find(name);
        return it == ctx->ws.end() ? nullptr : (float *)it->second.ptr;
    };
    float *Lt = get("ov.Lt"), *Lxy = get("ov.Lxy"), *Ld = get("ov.Ldet"), *kc = get("ov.kc");
    UWIP_REQUIRE(ctx, Lt && Lxy && Ld && kc, "no detect call yet");
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    UWIP_REQUIRE(ctx, frame < ctx->ov_last_frames, "frame beyond the last detect batch");
    const size_t off = ((size_t)level * ctx->ov_last_frames + frame) * n;
    if (h_Lt) UWIP_HIP(ctx, hipMemcpy(h_Lt, Lt + off, n * 4, hipMemcpyDeviceToHost));
    if (h_Lx || h_Ly) {        // the derivative pair is one interleaved plane on the device
        std::vector<float> xy(2 * n);
        UWIP_HIP(ctx, hipMemcpy(xy.data(), Lxy + 2 * off, n * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            if (h_Lx) h_Lx[i] = xy[2 * i];
            if (h_Ly) h_Ly[i] = xy[2 * i + 1];
        }
    }
    if (h_Ldet) UWIP_HIP(ctx, hipMemcpy(h_Ldet, Ld + off, n * 4, hipMemcpyDeviceToHost));
    if (h_kcontrast) UWIP_HIP(ctx, hipMemcpy(h_kcontrast, kc + frame, 4, hipMemcpyDeviceToHost));
    return UWIP_OK;
}

// calcBlur(Mat frame), videostrip.cpp:170-184, per frame of a BGR batch ALREADY at the working size
// (the reference calls it on res_frame, main.cpp:338,355): d_blur [frames].
UWIP_API int uwip_calcBlur(uwip_ctx *ctx, const uwip_batch_u8 *frames, float *d_blur)
{
    int rc = uwip_check_batch(ctx, frames, 3);
    if (rc) return rc;
    if (frames->frames == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, !uwip_batch_empty(frames) && d_blur, "empty image or null output");
    const int F = frames->frames, h = frames->rows, w = frames->cols;
    const size_t n = (size_t)h * w;
    uint8_t *gray = (uint8_t *)uwip_ws(ctx, "blur.gray", n * F);
    float *L0 = (float *)uwip_ws(ctx, "blur.L0", n * F * 4);
    const int nb = 64;
    double *part = (double *)uwip_ws(ctx, "blur.part", sizeof(double) * 2 * nb * F);
    if (!gray || !L0 || !part) return UWIP_ERR_NOMEM;
    const uint8_t *tx = (const uint8_t *)resize_table(ctx, w, w), *ty = (const uint8_t *)resize_table(ctx, h, h);
    if (!tx || !ty) return UWIP_ERR_NOMEM;
    uwip_kscope ks(ctx, "k_ov_blur");
    // identity "resize" = the fused BGR2GRAY pass
    k_ov_resize_gray<<<grid2d(w, h, F), 256, 0, ctx->stream>>>((const uint8_t *)frames->data, frames->step, frames->frame_stride, h, w, h, w,
                                                              (const int *)tx, (const short *)(tx + (size_t)w * 4), (const short *)(tx + (size_t)w * 6),
                                                              (const int *)ty, (const short *)(ty + (size_t)h * 4), (const short *)(ty + (size_t)h * 6),
                                                              gray, L0);
    k_ov_blur<<<dim3(nb, F), 256, 0, ctx->stream>>>(gray, h, w, part);
    k_ov_blur_final<<<uwip_cdiv(F, 64), 64, 0, ctx->stream>>>(part, nb, (double)n, d_blur, F);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

// cv::resize(frame, res_frame, cv::Size(), hResizeFactor, hResizeFactor), main.cpp:242,287,311 (INTER_LINEAR, 8UC3):
// dst must have the size uwip_overlap_working_size gives for src.
UWIP_API int uwip_resize_bgr(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst)
{
    int rc = uwip_check_batch(ctx, src, 3);
    if (rc) return rc;
    rc = uwip_check_batch(ctx, dst, 3);
    if (rc) return rc;
    UWIP_REQUIRE(ctx, src->frames == dst->frames, "frame count mismatch");
    if (src->frames == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, !uwip_batch_empty(src), "empty image");
    int oh = 0, ow = 0;
    resize_dims(src->rows, src->cols, TW, &oh, &ow);
    UWIP_REQUIRE(ctx, dst->rows == oh && dst->cols == ow, "dst is not the working size of src (uwip_overlap_working_size)");
    const uint8_t *tx = (const uint8_t *)resize_table(ctx, src->cols, ow), *ty = (const uint8_t *)resize_table(ctx, src->rows, oh);
    if (!tx || !ty) return UWIP_ERR_NOMEM;
    uwip_kscope ks(ctx, "k_ov_resize_bgr");
    k_ov_resize_bgr<<<grid2d(ow, oh, src->frames), 256, 0, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, src->rows, src->cols, oh, ow,
                                                                        (const int *)tx, (const short *)(tx + (size_t)ow * 4), (const short *)(tx + (size_t)ow * 6),
                                                                        (const int *)ty, (const short *)(ty + (size_t)oh * 4), (const short *)(ty + (size_t)oh * 6),
                                                                        (uint8_t *)dst->data, dst->step, dst->frame_stride);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}
