// videostrip overlap path, geometry: ratio test -> RANSAC homography -> least-squares refit -> overlapArea, one block per pair.
#include "overlap_internal.hpp"
#include "device_utils.hpp"

namespace {

constexpr int RANSAC_ITERS = 512;

// ---- ratio test + RANSAC homography + overlapArea, one block per pair ---------------------------------------
__device__ __forceinline__ uint32_t hash32(uint32_t a)
{
    a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
    return a;
}

// 8 x 8 Gaussian elimination with partial pivoting, the oracle's operations in the oracle's order -- but with every index
// a compile-time constant: the pivot row is swapped in by selects against each candidate row instead of A[p][k], so the
// 72 doubles live in registers.  (Indexed by the run-time pivot the array sat in scratch memory, and two of these solves
// per thread were half of k_ov_geometry's 0.4 ms.)  Columns left of the pivot column are never read again, so the swap
// and the elimination skip them.
__device__ __forceinline__ bool solve8(double (&A)[8][9])
{
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int p = c;
        double best = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double v = fabs(A[r][c]);
            if (v > best) { best = v; p = r; }          // strict: the first of equal maxima, as `p` walks in the oracle
        }
        if (!(best > 1e-12)) return false;
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const bool sw = p == r;
#pragma unroll
            for (int k = c; k < 9; ++k) {
                const double a = A[c][k], b = A[r][k];
                A[c][k] = sw ? b : a;
                A[r][k] = sw ? a : b;
            }
        }
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] / A[c][c];
#pragma unroll
            for (int k = c; k < 9; ++k) A[r][k] = A[r][k] - f * A[c][k];
        }
    }
#pragma unroll
    for (int r = 7; r >= 0; --r) {
        double s = A[r][8];
#pragma unroll
        for (int k = r + 1; k < 8; ++k) s = s - A[r][k] * A[k][8];
        A[r][8] = s / A[r][r];
    }
    return true;
}

__device__ __forceinline__ bool is_inlier(const double *H, double x, double y, double X, double Y)
{
    const double wv = H[6] * x + H[7] * y + H[8];
    const double px = (H[0] * x + H[1] * y + H[2]) / wv, py = (H[3] * x + H[4] * y + H[5]) / wv;
    const double ex = px - X, ey = py - Y;
    return (ex * ex + ey * ey) <= 9.0;
}

__device__ bool clip_line(long long W, long long Hh, long long &x1, long long &y1, long long &x2, long long &y2)
{
    const long long right = W - 1, bottom = Hh - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

constexpr int MASK_WORDS = TW / 32;     // 20 words per row

__device__ void draw_line(uint32_t *mask, long long x1, long long y1, long long x2, long long y2)
{
    if (!clip_line(TW, TH, x1, y1, x2, y2)) return;
    if (x2 < x1) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
    int dx = (int)(x2 - x1), dy = (int)(y2 - y1);
    const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
    dx = dx < 0 ? -dx : dx; dy = dy < 0 ? -dy : dy;
    int x = (int)x1, y = (int)y1;
    if (dy > dx) {
        int err = dy - (dx + dx);
        for (int i = 0; i <= dy; ++i) {
            mask[y * MASK_WORDS + (x >> 5)] |= 1u << (x & 31);
            const int m = err < 0;
            err += -(dx + dx) + (m ? dy + dy : 0);
            y += sy;
            if (m) x += sx;
        }
    } else {
        int err = dx - (dy + dy);
        for (int i = 0; i <= dx; ++i) {
            mask[y * MASK_WORDS + (x >> 5)] |= 1u << (x & 31);
            const int m = err < 0;
            err += -(dy + dy) + (m ? dx + dx : 0);
            x += sx;
            if (m) y += sy;
        }
    }
}

// scanline part of cv::fillConvexPoly (shift 0): per-row span ends into span[y] = (xx1, xx2) or (1, 0)
__device__ void fill_spans(const long long vx[4], const long long vy[4], short2 *span)
{
    const int XY_SHIFT = 16;
    const long long XY_ONE = 1 << XY_SHIFT;
    const int npts = 4;
    struct { int idx, di; long long x, dx; int ye; } edge[2];
    const int delta1 = (int)(XY_ONE >> 1), delta2 = (int)(XY_ONE >> 1);
    int imin = 0, edges = npts;
    long long xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    for (int i = 0; i < npts; ++i) {
        if (vy[i] < ymin) { ymin = vy[i]; imin = i; }
        if (vy[i] > ymax) ymax = vy[i];
        if (vx[i] > xmax) xmax = vx[i];
        if (vx[i] < xmin) xmin = vx[i];
    }
    if ((int)xmax < 0 || (int)ymax < 0 || (int)xmin >= TW || (int)ymin >= TH) return;
    if (ymax > TH - 1) ymax = TH - 1;
    int y = (int)ymin;
    edge[0].idx = edge[1].idx = imin;
    edge[0].ye = edge[1].ye = y;
    edge[0].di = 1; edge[1].di = npts - 1;
    edge[0].x = edge[1].x = -XY_ONE;
    edge[0].dx = edge[1].dx = 0;
    do {
        for (int i = 0; i < 2; ++i) {
            if (y >= edge[i].ye) {
                int idx0 = edge[i].idx;
                const int di = edge[i].di;
                int idx = idx0 + di;
                if (idx >= npts) idx -= npts;
                for (; edges-- > 0;) {
                    const int ty = (int)vy[idx];
                    if (ty > y) {
                        const long long xs = vx[idx0] << XY_SHIFT, xe = vx[idx] << XY_SHIFT;
                        edge[i].ye = ty;
                        edge[i].dx = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));
                        edge[i].x = xs;
                        edge[i].idx = idx;
                        break;
                    }
                    idx0 = idx;
                    idx += di;
                    if (idx >= npts) idx -= npts;
                }
            }
        }
        if (edges < 0) break;
        if (y >= 0) {
            int left = 0, right = 1;
            if (edge[0].x > edge[1].x) { left = 1; right = 0; }
            int xx1 = (int)((edge[left].x + delta1) >> XY_SHIFT);
            int xx2 = (int)((edge[right].x + delta2) >> XY_SHIFT);
            if (xx2 >= 0 && xx1 < TW) {
                if (xx1 < 0) xx1 = 0;
                if (xx2 >= TW) xx2 = TW - 1;
                span[y] = make_short2((short)xx1, (short)xx2);
            }
        }
        edge[0].x += edge[0].dx;
        edge[1].x += edge[1].dx;
    } while (++y <= (int)ymax);
}

// overlapArea(H), videostrip.cpp:291-319.  Must be called by the whole 256-thread block.
__device__ float overlap_area_block(const double *H, int videoW, int videoH, uint32_t *s_mask /*[TH*MASK_WORDS]*/,
                                    short2 *s_span /*[TH]*/, uint32_t *scratch, int *ov_out)
{
    __shared__ float s_f[8];
    for (int i = threadIdx.x; i < TH * MASK_WORDS; i += 256) s_mask[i] = 0;
    for (int i = threadIdx.x; i < TH; i += 256) s_span[i] = make_short2(1, 0);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float px[4] = {0, (float)TW, (float)TW, 0}, py[4] = {0, 0, (float)TH, (float)TH};
        long long vx[4], vy[4];
        for (int i = 0; i < 4; ++i) {
            const double x = px[i], y = py[i];
            double wv = x * H[6] + y * H[7] + H[8];
            float fx = 0.0f, fy = 0.0f;
            if (fabs(wv) > 2.220446049250313e-16) {
                wv = 1.0 / wv;
                fx = (float)((x * H[0] + y * H[1] + H[2]) * wv);
                fy = (float)((x * H[3] + y * H[4] + H[5]) * wv);
            }
            s_f[i] = fx; s_f[4 + i] = fy;
            vx[i] = (long long)__float2int_rn(fx);
            vy[i] = (long long)__float2int_rn(fy);
        }
        for (int i = 0; i < 4; ++i) {
            const int p = (i + 3) % 4;
            draw_line(s_mask, vx[p], vy[p], vx[i], vy[i]);
        }
        fill_spans(vx, vy, s_span);
    }
    __syncthreads();
    uint32_t cnt = 0;
    for (int i = threadIdx.x; i < TH * MASK_WORDS; i += 256) {
        const int y = i / MASK_WORDS, wd = i - y * MASK_WORDS;
        uint32_t m = s_mask[i];
        const short2 sp = s_span[y];
        const int lo = max((int)sp.x, wd * 32), hi = min((int)sp.y, wd * 32 + 31);
        if (lo <= hi) {
            const int nb = hi - lo + 1;
            const uint32_t bitsm = nb == 32 ? 0xffffffffu : (((1u << nb) - 1u) << (lo & 31));
            m |= bitsm;
        }
        cnt += __popc(m);
    }
    const uint32_t ov = block256_sum_u32(cnt, scratch);
    if (ov_out) *ov_out = (int)ov;
    double a00 = 0;
    for (int i = 0; i < 4; ++i) {
        const int p = (i + 3) % 4;
        a00 += (double)s_f[p] * s_f[4 + i] - (double)s_f[4 + p] * s_f[i];
    }
    const float area1 = (float)(videoW * videoH), area2 = (float)fabs(a00 * 0.5), cur = (float)ov;
    return cur / (area1 + area2 - cur);
}

constexpr int NSUM = 44;

__global__ __launch_bounds__(256) void k_ov_geometry(const Keypoint *__restrict__ qkp, const Keypoint *__restrict__ tkp,
                                                    const int32_t *__restrict__ qn, const int32_t *__restrict__ tn,
                                                    const int32_t *__restrict__ pair_q, const int32_t *__restrict__ pair_t,
                                                    const int32_t *__restrict__ m_idx, const int32_t *__restrict__ m_dist,
                                                    int w, int h, int videoW, int videoH, uint32_t seed, int min_inliers,
                                                    float *__restrict__ ratio, int32_t *__restrict__ info /*[P][8]*/,
                                                    double *__restrict__ Hout /*[P][9]*/,
                                                    const int32_t *__restrict__ d_npairs /*null: every launched pair*/)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_raw[];
    // carve: good points 4 x MAXKP floats (32 KB) | inlier flags MAXKP (2 KB) | mask (38.4 KB) | spans (1.9 KB)
    float *s_ox = reinterpret_cast<float *>(s_raw), *s_oy = s_ox + MAXKP, *s_sx = s_oy + MAXKP, *s_sy = s_sx + MAXKP;
    uint8_t *s_inl = reinterpret_cast<uint8_t *>(s_sy + MAXKP);
    uint32_t *s_mask = reinterpret_cast<uint32_t *>(s_inl + MAXKP);
    short2 *s_span = reinterpret_cast<short2 *>(s_mask + TH * MASK_WORDS);
    __shared__ uint32_t scratch[16];
    __shared__ int s_best_cnt[256], s_best_it[256];
    __shared__ double s_H[9];
    __shared__ double s_g[4][NSUM];
    __shared__ int s_ng;

    const int p = blockIdx.x, tid = threadIdx.x;
    if (d_npairs && p >= *d_npairs) return;
    const int fq = pair_q[p], ft = pair_t[p];
    const int nq = qn[fq], nt = tn[ft];
    const Keypoint *KQ = qkp + (size_t)fq * MAXKP, *KT = tkp + (size_t)ft * MAXKP;
    const int32_t *mi = m_idx + (size_t)p * MAXKP * 2, *md = m_dist + (size_t)p * MAXKP * 2;
    int32_t *inf = info + (size_t)p * 8;

    // ratio test (videostrip.cpp:233-242; last query skipped, B-12), order-preserving compaction
    if (tid == 0) s_ng = 0;
    __syncthreads();
    const int limit = (nt >= 2 && nq >= 1) ? nq - 1 : 0;
    for (int base = 0; base < limit; base += 256) {
        const int k = base + tid;
        uint32_t good = 0;
        if (k < limit) good = ((double)md[k * 2] < 0.8 * (double)md[k * 2 + 1]) ? 1u : 0u;
        const uint32_t incl = block256_incl_scan_u32(good, scratch);
        const int off = s_ng;
        if (good) {
            const int pos = off + (int)(incl - 1);
            const Keypoint a = KQ[k], b = KT[mi[k * 2]];
            s_ox[pos] = a.x; s_oy[pos] = a.y; s_sx[pos] = b.x; s_sy[pos] = b.y;
        }
        __syncthreads();
        if (tid == 255) s_ng = off + (int)incl;
        __syncthreads();
    }
    const int ng = s_ng;
    if (tid == 0) { inf[0] = nq; inf[1] = nt; inf[2] = ng; inf[3] = 0; inf[4] = 0; }
    if (ng < 4) {                                    // "Not enough good matches" -> -2.0 (videostrip.cpp:252-256)
        if (tid == 0) ratio[p] = -2.0f;
        return;
    }
    // 512 hypotheses, 2 per thread
    int my_cnt = 0, my_it = 0x7fffffff;
    for (int rep = 0; rep < RANSAC_ITERS / 256; ++rep) {
        const int it = rep * 256 + tid;
        int pick[4];
        for (int j = 0; j < 4; ++j) {
            uint32_t attempt = 0;
            for (;;) {
                const uint32_t r = hash32(seed ^ hash32((uint32_t)(it * 4 + j + 1) + attempt * 0x9e3779b9u));
                const int c = (int)(r % (uint32_t)ng);
                bool dup = false;
                for (int m = 0; m < j; ++m) dup = dup || (pick[m] == c);
                if (!dup || attempt >= 16) { pick[j] = c; break; }
                attempt++;
            }
        }
        double A[8][9];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double x = s_ox[pick[j]], y = s_oy[pick[j]], X = s_sx[pick[j]], Y = s_sy[pick[j]];
            double *r0 = A[2 * j], *r1 = A[2 * j + 1];
            r0[0] = x; r0[1] = y; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -x * X; r0[7] = -y * X; r0[8] = X;
            r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = x; r1[4] = y; r1[5] = 1; r1[6] = -x * Y; r1[7] = -y * Y; r1[8] = Y;
        }
        if (!solve8(A)) continue;
        double Hc[9];
#pragma unroll
        for (int k = 0; k < 8; ++k) Hc[k] = A[k][8];
        Hc[8] = 1.0;
        int cnt = 0;
        for (int i = 0; i < ng; ++i) cnt += is_inlier(Hc, s_ox[i], s_oy[i], s_sx[i], s_sy[i]) ? 1 : 0;
        if (cnt > my_cnt) { my_cnt = cnt; my_it = it; }      // it increases: keeps the first maximum
    }
    s_best_cnt[tid] = my_cnt; s_best_it[tid] = my_it;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            const int oc = s_best_cnt[tid + s], oi = s_best_it[tid + s];
            if (oc > s_best_cnt[tid] || (oc == s_best_cnt[tid] && oi < s_best_it[tid])) { s_best_cnt[tid] = oc; s_best_it[tid] = oi; }
        }
        __syncthreads();
    }
    const int best = s_best_cnt[0], best_it = s_best_it[0];
    if (best < min_inliers) {                         // H.empty() -> -2.0 (videostrip.cpp:272)
        if (tid == 0) ratio[p] = -2.0f;
        return;
    }
    if (tid == 0) {
        // rebuild the winning hypothesis
        int pick[4];
        for (int j = 0; j < 4; ++j) {
            uint32_t attempt = 0;
            for (;;) {
                const uint32_t r = hash32(seed ^ hash32((uint32_t)(best_it * 4 + j + 1) + attempt * 0x9e3779b9u));
                const int c = (int)(r % (uint32_t)ng);
                bool dup = false;
                for (int m = 0; m < j; ++m) dup = dup || (pick[m] == c);
                if (!dup || attempt >= 16) { pick[j] = c; break; }
                attempt++;
            }
        }
        double A[8][9];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double x = s_ox[pick[j]], y = s_oy[pick[j]], X = s_sx[pick[j]], Y = s_sy[pick[j]];
            double *r0 = A[2 * j], *r1 = A[2 * j + 1];
            r0[0] = x; r0[1] = y; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -x * X; r0[7] = -y * X; r0[8] = X;
            r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = x; r1[4] = y; r1[5] = 1; r1[6] = -x * Y; r1[7] = -y * Y; r1[8] = Y;
        }
        solve8(A);
        for (int k = 0; k < 8; ++k) s_H[k] = A[k][8];
        s_H[8] = 1.0;
        inf[3] = best;
    }
    __syncthreads();
    for (int i = tid; i < ng; i += 256) s_inl[i] = is_inlier(s_H, s_ox[i], s_oy[i], s_sx[i], s_sy[i]) ? 1 : 0;
    __syncthreads();
    // least-squares refit in fixed-normalised coordinates; summation order = the oracle's
    const double cx = 0.5 * (double)w, cy = 0.5 * (double)h, sN = 0.5 * (double)w;
    double part[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) part[k] = 0.0;
    for (int i = tid; i < ng; i += 256) {
        if (!s_inl[i]) continue;
        const double x = ((double)s_ox[i] - cx) / sN, y = ((double)s_oy[i] - cy) / sN;
        const double X = ((double)s_sx[i] - cx) / sN, Y = ((double)s_sy[i] - cy) / sN;
        const double a[8] = {x, y, 1, 0, 0, 0, -x * X, -y * X}, b[8] = {0, 0, 0, x, y, 1, -x * Y, -y * Y};
        int k = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = r; c < 8; ++c) { part[k] = part[k] + (a[r] * a[c] + b[r] * b[c]); k++; }
#pragma unroll
        for (int r = 0; r < 8; ++r) { part[k] = part[k] + (a[r] * X + b[r] * Y); k++; }
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        double v = part[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
        if ((tid & 63) == 0) s_g[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double A[8][9];
        int k = 0;
        for (int r = 0; r < 8; ++r)
            for (int c = r; c < 8; ++c) {
                const double t = ((s_g[0][k] + s_g[1][k]) + s_g[2][k]) + s_g[3][k];
                A[r][c] = t; A[c][r] = t; k++;
            }
        for (int r = 0; r < 8; ++r) { A[r][8] = ((s_g[0][k] + s_g[1][k]) + s_g[2][k]) + s_g[3][k]; k++; }
        int ok = solve8(A) ? 1 : 0;
        if (ok) {
            const double hn[9] = {A[0][8], A[1][8], A[2][8], A[3][8], A[4][8], A[5][8], A[6][8], A[7][8], 1.0};
            double M[9], R[9];
            for (int r = 0; r < 3; ++r) {
                M[r * 3 + 0] = hn[r * 3 + 0] / sN;
                M[r * 3 + 1] = hn[r * 3 + 1] / sN;
                M[r * 3 + 2] = (hn[r * 3 + 2] - hn[r * 3 + 0] * (cx / sN)) - hn[r * 3 + 1] * (cy / sN);
            }
            for (int c = 0; c < 3; ++c) {
                R[0 * 3 + c] = sN * M[0 * 3 + c] + cx * M[2 * 3 + c];
                R[1 * 3 + c] = sN * M[1 * 3 + c] + cy * M[2 * 3 + c];
                R[2 * 3 + c] = M[2 * 3 + c];
            }
            if (R[8] == 0.0 || R[8] != R[8]) ok = 0;
            else for (int i = 0; i < 9; ++i) s_H[i] = R[i] / R[8];
        }
        (void)ok;
        if (Hout) for (int i = 0; i < 9; ++i) Hout[(size_t)p * 9 + i] = s_H[i];
    }
    __syncthreads();
    int ov = 0;
    const float r = overlap_area_block(s_H, videoW, videoH, s_mask, s_span, scratch, &ov);
    if (tid == 0) { ratio[p] = r; inf[4] = ov; }
}

// standalone overlapArea on a list of homographies
__global__ __launch_bounds__(256) void k_ov_area_only(const double *__restrict__ Hs, int videoW, int videoH, float *__restrict__ ratio,
                                                     int32_t *__restrict__ ovc)
{
    __shared__ uint32_t s_mask[TH * MASK_WORDS];
    __shared__ short2 s_span[TH];
    __shared__ uint32_t scratch[16];
    __shared__ double s_H[9];
    if (threadIdx.x < 9) s_H[threadIdx.x] = Hs[(size_t)blockIdx.x * 9 + threadIdx.x];
    __syncthreads();
    int ov = 0;
    const float r = overlap_area_block(s_H, videoW, videoH, s_mask, s_span, scratch, &ov);
    if (threadIdx.x == 0) { ratio[blockIdx.x] = r; if (ovc) ovc[blockIdx.x] = ov; }
}

}  // namespace

int uwip_overlap_geometry(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft, const int32_t *d_pq, const int32_t *d_pt,
                          const int32_t *d_npairs, int npairs, const int32_t *m_idx, const int32_t *m_dist, int videoWidth,
                          int videoHeight, uint32_t seed, int min_inliers, float *d_ratio, int32_t *info, double *d_H)
{
    uwip_kscope ks(ctx, "k_ov_geometry");
    const size_t lds = (size_t)MAXKP * 16 + MAXKP + (size_t)TH * MASK_WORDS * 4 + (size_t)TH * 4;
    int rc = uwip_lds_optin(ctx, "k_ov_geometry", (const void *)k_ov_geometry, lds);
    if (rc) return rc;
    k_ov_geometry<<<npairs, 256, lds, ctx->stream>>>(fq->d_kp, ft->d_kp, fq->d_n, ft->d_n, d_pq, d_pt, m_idx, m_dist,
                                                    fq->w, fq->h, videoWidth, videoHeight, seed, min_inliers, d_ratio, info, d_H, d_npairs);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

// overlapArea(Mat H), videostrip.cpp:291-319, for n homographies (device, row-major 3x3 doubles)
UWIP_API int uwip_overlapArea(uwip_ctx *ctx, const double *d_H, int n, int videoWidth, int videoHeight, float *d_ratio,
                              int32_t *d_count)
{
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, n >= 0, "negative count");
    if (n == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, d_H && d_ratio, "null buffer");
    uwip_kscope ks(ctx, "k_ov_area_only");
    k_ov_area_only<<<n, 256, 0, ctx->stream>>>(d_H, videoWidth, videoHeight, d_ratio, d_count);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}
