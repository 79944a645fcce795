// The arithmetic of the strip mosaic, stated ONCE for the device (strip.hip: k_strip_chain, k_strip_render, k_strip_gain_stats,
// k_strip_gain_solve, k_strip_stack, k_strip_render_bands, k_strip_seam_cost, k_strip_seam_path), the host (uwip_strip_chain_host,
// uwip_strip_gain_solve_host, uwip_strip_stack_host, uwip_strip_seam_path_host) and the emulation harnesses
// (tests/strip_emulated.cpp, tests/strip_gain_emulated.cpp, tests/strip_band_emulated.cpp, tests/strip_seam_emulated.cpp).
// tests/_strip_mirror.py, tests/_strip_gain_mirror.py, tests/_strip_band_mirror.py and tests/_strip_seam_mirror.py restate it
// in numpy and take nothing from here; the tests compare the two bit for bit, which is why
//   - every coordinate is float64, products and sums are separate operations (the library and the harness are built with
//     -ffp-contract=off), sums are written ((a*x) + (b*y)) + c, and divisions are IEEE divisions;
//   - everything after the source position (u, v) is integer arithmetic.
// Conventions: pixel centres at integer coordinates; frames are w x h BGR; H_k takes frame k onto frame k - 1 (the matcher's
// d_H with query = k, train = k - 1, videostrip.cpp:270); G_k takes frame k onto the plane of its segment, which is the
// coordinate system of the segment's first frame.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/uwip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STRIP_HD __host__ __device__
#else
#define STRIP_HD
#endif

namespace uwip_sm {

struct ChainParams {
    int32_t w, h;                         // geometry of the stored frames
    int32_t max_rows, max_cols;           // largest canvas of one segment
    double  max_scale;                    // a frame's mapped area stays within (w-1)(h-1) / s^2 ... (w-1)(h-1) * s^2
};

// what the chain writes ([n] frames; segs holds one entry per segment, at most n)
struct ChainOut {
    double  *G, *Ginv;                    // [n][9]
    int32_t *seg;                         // [n]
    int32_t *box;                         // [n][4] = x0, y0, x1, y1 on the segment's canvas (inclusive, grown by 1, clamped)
    uwip_strip_segment *segs;
    int32_t *nseg;
};

STRIP_HD inline bool finite_d(double v) { return v - v == 0.0; }

// adjugate of G times the sign of its determinant: the projective inverse with a positive denominator wherever G's own
// denominator is positive.  Not divided by the determinant (a homography's scale is free).
STRIP_HD inline void adjugate_signed(const double *G, double *A)
{
    A[0] = (G[4] * G[8]) - (G[5] * G[7]);
    A[1] = (G[2] * G[7]) - (G[1] * G[8]);
    A[2] = (G[1] * G[5]) - (G[2] * G[4]);
    A[3] = (G[5] * G[6]) - (G[3] * G[8]);
    A[4] = (G[0] * G[8]) - (G[2] * G[6]);
    A[5] = (G[2] * G[3]) - (G[0] * G[5]);
    A[6] = (G[3] * G[7]) - (G[4] * G[6]);
    A[7] = (G[1] * G[6]) - (G[0] * G[7]);
    A[8] = (G[0] * G[4]) - (G[1] * G[3]);
    const double det = ((G[0] * A[0]) + (G[1] * A[3])) + (G[2] * A[6]);
    const double s = det < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 9; ++i) A[i] = A[i] * s;
}

// Break rules 2-4 on a candidate G: maps the four pixel-centre corners; q = x0..x3, y0..y3.  false = start a new segment.
STRIP_HD inline bool quad_ok(const ChainParams &P, const double *G, double *qx, double *qy)
{
    for (int i = 0; i < 9; ++i) if (!finite_d(G[i])) return false;
    const double cx[4] = {0.0, (double)(P.w - 1), (double)(P.w - 1), 0.0};
    const double cy[4] = {0.0, 0.0, (double)(P.h - 1), (double)(P.h - 1)};
    for (int i = 0; i < 4; ++i) {
        const double d = ((G[6] * cx[i]) + (G[7] * cy[i])) + G[8];
        if (!(d > 0.0)) return false;
        qx[i] = (((G[0] * cx[i]) + (G[1] * cy[i])) + G[2]) / d;
        qy[i] = (((G[3] * cx[i]) + (G[4] * cy[i])) + G[5]) / d;
        if (!finite_d(qx[i]) || !finite_d(qy[i])) return false;
    }
    // rule 3: strictly convex, the input's orientation (every cross product of consecutive edges > 0)
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3, k = (i + 2) & 3;
        const double ax = qx[j] - qx[i], ay = qy[j] - qy[i], bx = qx[k] - qx[j], by = qy[k] - qy[j];
        const double c = (ax * by) - (ay * bx);
        if (!(c > 0.0)) return false;
    }
    // rule 4: shoelace area
    double s = 0.0;
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        s = s + ((qx[i] * qy[j]) - (qx[j] * qy[i]));
    }
    const double area = 0.5 * s, a0 = (double)(P.w - 1) * (double)(P.h - 1), s2 = P.max_scale * P.max_scale;
    if (!(area >= a0 / s2) || !(area <= a0 * s2)) return false;
    return true;
}

// integer box (as doubles: a candidate may lie anywhere) of a mapped quad
STRIP_HD inline void quad_box(const double *qx, const double *qy, double *b)
{
    double x0 = qx[0], x1 = qx[0], y0 = qy[0], y1 = qy[0];
    for (int i = 1; i < 4; ++i) {
        x0 = qx[i] < x0 ? qx[i] : x0; x1 = qx[i] > x1 ? qx[i] : x1;
        y0 = qy[i] < y0 ? qy[i] : y0; y1 = qy[i] > y1 ? qy[i] : y1;
    }
    b[0] = floor(x0); b[1] = floor(y0); b[2] = ceil(x1); b[3] = ceil(y1);
}

STRIP_HD inline int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The chain: sequential over the frames.  H [n][9], ratio [n] (entry 0 of both is not read: frame 0 starts segment 0).
// `fb` is scratch of [n][4] doubles (each frame's box on its segment's plane, until the segment closes).
STRIP_HD inline void chain(const ChainParams &P, const double *H, const float *ratio, int32_t n, const ChainOut &o, double *fb)
{
    const double I9[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    int32_t nseg = 0, first = 0;
    double sb[4] = {0.0, 0.0, 0.0, 0.0};         // the open segment's box
    double Gp[9];
    auto close = [&](int32_t end) {
        uwip_strip_segment &s = o.segs[nseg];
        s.first = first; s.count = end - first;
        s.x0 = (int32_t)sb[0]; s.y0 = (int32_t)sb[1];
        s.cols = (int32_t)(sb[2] - sb[0]) + 1; s.rows = (int32_t)(sb[3] - sb[1]) + 1;
        s.reserved[0] = s.reserved[1] = 0;
        for (int32_t k = first; k < end; ++k) {
            o.seg[k] = nseg;
            o.box[4 * k + 0] = clampi((int32_t)fb[4 * k + 0] - 1 - s.x0, 0, s.cols - 1);
            o.box[4 * k + 1] = clampi((int32_t)fb[4 * k + 1] - 1 - s.y0, 0, s.rows - 1);
            o.box[4 * k + 2] = clampi((int32_t)fb[4 * k + 2] + 1 - s.x0, 0, s.cols - 1);
            o.box[4 * k + 3] = clampi((int32_t)fb[4 * k + 3] + 1 - s.y0, 0, s.rows - 1);
        }
        ++nseg;
    };
    for (int32_t k = 0; k < n; ++k) {
        double G[9], qx[4], qy[4], b[4], nb[4];
        bool joined = false;
        if (k > first && ratio[k] != -2.0f) {                        // rule 1
            const double *Hk = H + 9 * (size_t)k;
            double M[9];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    M[3 * i + j] = ((Gp[3 * i] * Hk[j]) + (Gp[3 * i + 1] * Hk[3 + j])) + (Gp[3 * i + 2] * Hk[6 + j]);
            for (int i = 0; i < 9; ++i) G[i] = M[i] / M[8];
            if (quad_ok(P, G, qx, qy)) {                             // rules 2-4
                quad_box(qx, qy, b);
                nb[0] = b[0] < sb[0] ? b[0] : sb[0]; nb[1] = b[1] < sb[1] ? b[1] : sb[1];
                nb[2] = b[2] > sb[2] ? b[2] : sb[2]; nb[3] = b[3] > sb[3] ? b[3] : sb[3];
                joined = ((nb[2] - nb[0]) + 1.0 <= (double)P.max_cols) && ((nb[3] - nb[1]) + 1.0 <= (double)P.max_rows);   // rule 5
            }
        }
        if (!joined) {
            if (k > first) close(k);
            first = k;
            for (int i = 0; i < 9; ++i) G[i] = I9[i];
            b[0] = 0.0; b[1] = 0.0; b[2] = (double)(P.w - 1); b[3] = (double)(P.h - 1);
            for (int i = 0; i < 4; ++i) nb[i] = b[i];
        }
        for (int i = 0; i < 4; ++i) { sb[i] = nb[i]; fb[4 * (size_t)k + i] = b[i]; }
        for (int i = 0; i < 9; ++i) { Gp[i] = G[i]; o.G[9 * (size_t)k + i] = G[i]; }
        adjugate_signed(G, o.Ginv + 9 * (size_t)k);
    }
    if (n > 0) close(n);
    *o.nseg = nseg;
}

// ---- the sample: canvas pixel -> source taps --------------------------------------------------------------------------
struct Tap {
    int32_t x, y, x1, y1;                 // the four taps' columns and rows
    int32_t fx, fy;                       // 5-bit fractions
    int32_t q;                            // feather weight: 1 + distance of the nearest pixel to the frame's border
};

// plane point (px, py) under A = Ginv of a w x h frame; false = not covered
STRIP_HD inline bool sample(const double *A, double px, double py, int32_t w, int32_t h, Tap &t)
{
    const double d = ((A[6] * px) + (A[7] * py)) + A[8];
    if (!(d > 0.0)) return false;
    const double u = (((A[0] * px) + (A[1] * py)) + A[2]) / d;
    const double v = (((A[3] * px) + (A[4] * py)) + A[5]) / d;
    if (!(fabs(u) < 1048576.0) || !(fabs(v) < 1048576.0)) return false;
    const int32_t U = (int32_t)floor((u * 32.0) + 0.5), V = (int32_t)floor((v * 32.0) + 0.5);
    if (U < 0 || U > 32 * (w - 1) || V < 0 || V > 32 * (h - 1)) return false;
    t.x = U >> 5; t.fx = U & 31; t.x1 = t.x + 1 < w - 1 ? t.x + 1 : w - 1;
    t.y = V >> 5; t.fy = V & 31; t.y1 = t.y + 1 < h - 1 ? t.y + 1 : h - 1;
    const int32_t xn = (U + 16) >> 5, yn = (V + 16) >> 5;
    int32_t m = xn < w - 1 - xn ? xn : w - 1 - xn;
    m = yn < m ? yn : m;
    m = h - 1 - yn < m ? h - 1 - yn : m;
    t.q = 1 + m;
    return true;
}

// P = sum of the four taps times their 10-bit weights, 0 .. 255 * 1024
STRIP_HD inline int32_t bilinear(const Tap &t, int32_t p00, int32_t p10, int32_t p01, int32_t p11)
{
    return (32 - t.fx) * (32 - t.fy) * p00 + t.fx * (32 - t.fy) * p10 + (32 - t.fx) * t.fy * p01 + t.fx * t.fy * p11;
}

// ---- gain compensation from the overlaps of consecutive frames (Brown & Lowe 2007, section 6) ----------------------------
// One gain per frame and colour channel, from the pairs (k - 1, k) inside a segment alone: the normal equations are
// tridiagonal.  k_strip_gain_stats measures the pairs, gain_solve() solves, apply_gain() is the render's multiply.
struct GainParams {
    double  sigma_n, sigma_g;             // the paper's error and gain deviations, in 8-bit levels / as a factor
    int32_t lo, hi;                       // a pixel counts when all six of its values lie in 1024 lo .. 1024 hi
    int32_t min_pixels;                   // a pair with fewer valid pixels counts as having none
};
constexpr int kGainStats = 7;             // N, Sa[3], Sb[3] per frame: its pair with the frame before

// pixel (x, y) of a frame under its G -> the point on the segment's plane; false = no such point
STRIP_HD inline bool gain_point(const double *G, double x, double y, double &px, double &py)
{
    const double d = ((G[6] * x) + (G[7] * y)) + G[8];
    if (!(d > 0.0)) return false;
    px = (((G[0] * x) + (G[1] * y)) + G[2]) / d;
    py = (((G[3] * x) + (G[4] * y)) + G[5]) / d;
    return finite_d(px) && finite_d(py);
}

// One pixel of frame k against frame k - 1: fk / fp are the two frames (w x h BGR, packed), G of frame k, Ap = Ginv of frame
// k - 1.  Pb = 1024 x the pixel, Pa = the bilinear sample of frame k - 1 at the same plane point; false = not a valid pixel.
STRIP_HD inline bool gain_pixel(const GainParams &P, const uint8_t *fk, const uint8_t *fp, const double *G, const double *Ap,
                                int32_t x, int32_t y, int32_t w, int32_t h, int32_t *Pa, int32_t *Pb)
{
    double px, py;
    Tap t;
    if (!gain_point(G, (double)x, (double)y, px, py)) return false;
    if (!sample(Ap, px, py, w, h, t)) return false;
    const uint8_t *b = fk + ((size_t)y * w + x) * 3;
    const uint8_t *r0 = fp + ((size_t)t.y * w) * 3, *r1 = fp + ((size_t)t.y1 * w) * 3;
    const int32_t lo = 1024 * P.lo, hi = 1024 * P.hi;
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        Pb[c] = 1024 * (int32_t)b[c];
        Pa[c] = bilinear(t, r0[t.x * 3 + c], r0[t.x1 * 3 + c], r1[t.x * 3 + c], r1[t.x1 * 3 + c]);
        ok = ok && Pa[c] >= lo && Pa[c] <= hi && Pb[c] >= lo && Pb[c] <= hi;
    }
    return ok;
}

STRIP_HD inline int32_t gain_quantise(double g)
{
    const double v = floor((g * 4096.0) + 0.5);
    if (!finite_d(v)) return 4096;
    return v < 1024.0 ? 1024 : (v > 16384.0 ? 16384 : (int32_t)v);
}

// The solve: stats [n][7] (a segment's first frame: zeros), seg [n] -> gq [n][3] (gains in 1/4096, 1024 .. 16384), g [n][3].
// `scr` is scratch of [n][3] doubles (diag, off, rhs of one segment and channel; the elimination overwrites diag and rhs).
STRIP_HD inline void gain_solve(const GainParams &P, const uint64_t *stats, const int32_t *seg, int32_t n, int32_t *gq, double *g,
                                double *scr)
{
    const double wN = 1.0 / (P.sigma_n * P.sigma_n), wg = 1.0 / (P.sigma_g * P.sigma_g);
    for (int32_t first = 0; first < n;) {
        int32_t end = first + 1;
        while (end < n && seg[end] == seg[first]) ++end;
        const int32_t m = end - first;
        double *diag = scr, *off = scr + m, *rhs = scr + 2 * (size_t)m;
        for (int c = 0; c < 3; ++c) {
            for (int32_t i = 0; i < m; ++i) { diag[i] = 0.0; off[i] = 0.0; rhs[i] = 0.0; }
            for (int32_t i = 1; i < m; ++i) {                        // the pair (a, b) = (i - 1, i)
                const uint64_t *st = stats + kGainStats * (size_t)(first + i);
                if (st[0] < (uint64_t)P.min_pixels) continue;        // counts as N = 0: the pair adds nothing
                const double Nd = (double)st[0];
                const double A = (double)st[1 + c] / (Nd * 1024.0), B = (double)st[4 + c] / (Nd * 1024.0);
                diag[i - 1] = diag[i - 1] + (Nd * (((A * A) * wN) + wg));
                diag[i] = diag[i] + (Nd * (((B * B) * wN) + wg));
                off[i - 1] = -(Nd * ((A * B) * wN));
                rhs[i - 1] = rhs[i - 1] + (Nd * wg);
                rhs[i] = rhs[i] + (Nd * wg);
            }
            for (int32_t i = 0; i < m; ++i) if (diag[i] == 0.0) { diag[i] = 1.0; rhs[i] = 1.0; }
            // Thomas elimination: forwards (diag becomes c, rhs becomes e), then backwards
            for (int32_t i = 1; i < m; ++i) {
                const double mul = off[i - 1] / diag[i - 1];
                diag[i] = diag[i] - (mul * off[i - 1]);
                rhs[i] = rhs[i] - (mul * rhs[i - 1]);
            }
            double *go = g + 3 * (size_t)first + c;
            go[3 * (size_t)(m - 1)] = rhs[m - 1] / diag[m - 1];
            for (int32_t i = m - 2; i >= 0; --i) go[3 * (size_t)i] = (rhs[i] - (off[i] * go[3 * (size_t)(i + 1)])) / diag[i];
            for (int32_t i = 0; i < m; ++i) gq[3 * (size_t)(first + i) + c] = gain_quantise(go[3 * (size_t)i]);
        }
        first = end;
    }
}

// P (0 .. 255 * 1024) times a gain in 1/4096, saturating: 261120 x 16384 + 2048 < 2^32
STRIP_HD inline int32_t apply_gain(int32_t P, int32_t gq)
{
    const uint32_t v = ((uint32_t)P * (uint32_t)gq + 2048u) >> 12;
    return (int32_t)(v < 255u * 1024u ? v : 255u * 1024u);
}

// ---- multi-band blending (Brown & Lowe 2007, section 7) ------------------------------------------------------------------
// Every frame carries an undecimated (a trous) stack in its own coordinates: level 0 is the frame, level l + 1 is level l under
// (1, 4, 6, 4, 1) x (1, 4, 6, 4, 1) / 256 with taps 2^l pixels apart, borders clamped, one rounding per level.  The render
// samples every level at the frame's one tap, blends the differences of consecutive levels with a ramp of ramp[l] feather units
// behind the best frame, and the last level with the feather weights themselves.
constexpr int kBandLevels = 4;            // most levels of a stack

struct BandParams {
    int32_t levels;                       // 1 .. kBandLevels
    int32_t ramp[kBandLevels];            // 1 .. 4096 each
};

STRIP_HD inline int32_t stack_k(int i) { return i == 2 ? 6 : ((i == 1 || i == 3) ? 4 : 1); }

// A frame's rows as bytes: byte B of a row of 3 w bytes, B anywhere -> the byte the clamp reads (its own channel of the row's
// first or last pixel)
STRIP_HD inline int32_t stack_clamp_byte(int32_t B, int32_t w)
{
    if (B < 0) return ((B % 3) + 3) % 3;
    if (B >= 3 * w) return 3 * (w - 1) + B % 3;
    return B;
}

STRIP_HD inline uint8_t stack_round(int32_t sum) { return (uint8_t)((sum + 128) >> 8); }

// byte B of row y of the next level, from the level `in` (w x h BGR, packed) with taps s pixels apart
STRIP_HD inline uint8_t stack_byte(const uint8_t *in, int32_t w, int32_t h, int32_t s, int32_t y, int32_t B)
{
    int32_t sum = 0;
    for (int i = 0; i < 5; ++i) {
        const uint8_t *row = in + (size_t)clampi(y + (i - 2) * s, 0, h - 1) * w * 3;
        int32_t r = 0;
        for (int j = 0; j < 5; ++j) r += stack_k(j) * (int32_t)row[stack_clamp_byte(B + 3 * s * (j - 2), w)];
        sum += stack_k(i) * r;
    }
    return stack_round(sum);
}

// a / b towards minus infinity, b > 0
STRIP_HD inline int64_t floor_div(int64_t a, int64_t b)
{
    const int64_t q = a / b;
    return (a % b) < 0 ? q - 1 : q;
}

STRIP_HD inline int32_t band_weight(int32_t q, int32_t qmax, int32_t ramp)
{
    const int32_t v = (q - qmax) + ramp;
    return v > 0 ? v : 0;
}

// one band's share of a pixel: the rounded quotient of its weighted differences, N = sum w D, W = sum w >= 1
STRIP_HD inline int64_t band_term(int64_t N, int64_t W) { return floor_div(2 * N + W, 2 * W); }

// the pixel: NL = sum q S[levels], WL = sum q > 0, b = the sum of the bands' terms
STRIP_HD inline uint8_t band_pixel(int64_t NL, int64_t WL, int64_t b)
{
    const int64_t v = floor_div(NL + (b + 512) * WL, 1024 * WL);
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- seams found in the overlaps of consecutive frames ----------------------------------------------------------------------
// Frame k of a segment (not its first) has one seam against frame k - 1, in frame k's own pixel grid: the path through the
// overlap along which the two (gained) frames differ least, one dynamic programme per pair.  seam_orient() picks the axis the
// path runs along, seam_cost() is one entry of the pair's cost, seam_step() one state of one step of the programme, seam_path()
// the whole of it, seam_side() the render's question.  Costs are exact integers below 2^22 (kSeamOutside where the pair has no
// sample), so with at most 1023 steps every path total stays below 2^32.
struct SeamParams { int32_t prior; };     // 0 .. 4096: cost, in 1/1024 grey levels, per pixel of imbalance between the two frames' margins
constexpr uint32_t kSeamOutside = 1u << 22;
constexpr int32_t kSeamMaxSide = 1023;    // the largest stored frame side a seam is computed for

// orient = axis | (sign < 0 ? 2 : 0).  axis 0: the seam is a function of x (steps t = x, states s = y); axis 1: of y.
STRIP_HD inline int32_t seam_axis(int32_t orient) { return orient & 1; }
STRIP_HD inline int32_t seam_sign(int32_t orient) { return (orient & 2) ? -1 : 1; }

// Gp = G of frame k - 1, A = Ginv of frame k: the direction from k - 1's centre to k's centre, in k's coordinates
STRIP_HD inline int32_t seam_orient(const double *Gp, const double *A, int32_t w, int32_t h)
{
    const double cx = (double)(w - 1) * 0.5, cy = (double)(h - 1) * 0.5;
    double dx = 0.0, dy = 0.0, px, py;
    if (gain_point(Gp, cx, cy, px, py)) {
        const double d = ((A[6] * px) + (A[7] * py)) + A[8];
        if (d > 0.0) {
            const double u = (((A[0] * px) + (A[1] * py)) + A[2]) / d;
            const double v = (((A[3] * px) + (A[4] * py)) + A[5]) / d;
            if (finite_d(u) && finite_d(v)) { dx = cx - u; dy = cy - v; }
        }
    }
    if (fabs(dy) >= fabs(dx)) return dy >= 0.0 ? 0 : 2;
    return dx >= 0.0 ? 1 : 3;
}

// C of pixel (x, y) of frame k: fk / fp are frames k and k - 1 (w x h BGR, packed), G of frame k, Ap = Ginv of frame k - 1,
// gk / gp their gains in 1/4096 (null: 4096)
STRIP_HD inline uint32_t seam_cost(const SeamParams &P, const uint8_t *fk, const uint8_t *fp, const double *G, const double *Ap,
                                   const int32_t *gk, const int32_t *gp, int32_t axis, int32_t x, int32_t y, int32_t w, int32_t h)
{
    double px, py;
    Tap t;
    if (!gain_point(G, (double)x, (double)y, px, py)) return kSeamOutside;
    if (!sample(Ap, px, py, w, h, t)) return kSeamOutside;
    const uint8_t *b = fk + ((size_t)y * w + x) * 3;
    const uint8_t *r0 = fp + ((size_t)t.y * w) * 3, *r1 = fp + ((size_t)t.y1 * w) * 3;
    int32_t D = 0;
    for (int c = 0; c < 3; ++c) {
        const int32_t Pb = apply_gain(1024 * (int32_t)b[c], gk ? gk[c] : 4096);
        const int32_t Pa = apply_gain(bilinear(t, r0[t.x * 3 + c], r0[t.x1 * 3 + c], r1[t.x * 3 + c], r1[t.x1 * 3 + c]), gp ? gp[c] : 4096);
        D += Pa > Pb ? Pa - Pb : Pb - Pa;
    }
    const int32_t xn = t.x + (t.fx >= 16), yn = t.y + (t.fy >= 16);
    const int32_t S = axis ? w : h, s = axis ? x : y, sp = axis ? xn : yn;
    const int32_t ak = s < S - 1 - s ? s : S - 1 - s, ap = sp < S - 1 - sp ? sp : S - 1 - sp;
    return (uint32_t)(D + P.prior * (ak > ap ? ak - ap : ap - ak));
}

// One state of one step: E[t][s] from E[t - 1] (`prev`, S states) and c = C[t][s]; bp = 0, 1, 2 for the predecessor s, s - 1,
// s + 1 (ties in that order)
STRIP_HD inline uint32_t seam_step(const uint32_t *prev, int32_t S, int32_t s, uint32_t c, uint32_t &bp)
{
    uint32_t m = prev[s];
    bp = 0;
    if (s > 0 && prev[s - 1] < m) { m = prev[s - 1]; bp = 1; }
    if (s + 1 < S && prev[s + 1] < m) { m = prev[s + 1]; bp = 2; }
    return c + m;
}

STRIP_HD inline int32_t seam_back(int32_t s, uint32_t bp) { return bp == 1 ? s - 1 : (bp == 2 ? s + 1 : s); }

// The path: cost [T][S] -> seam [T], the total.  E [2][S] and back [T][S] (2 bits used of each byte) are scratch.
STRIP_HD inline uint64_t seam_path(const uint32_t *cost, int32_t T, int32_t S, int32_t *seam, uint32_t *E, uint8_t *back)
{
    for (int32_t s = 0; s < S; ++s) E[s] = cost[s];
    for (int32_t t = 1; t < T; ++t) {
        const uint32_t *prev = E + (size_t)((t - 1) & 1) * S;
        uint32_t *cur = E + (size_t)(t & 1) * S;
        for (int32_t s = 0; s < S; ++s) {
            uint32_t bp;
            cur[s] = seam_step(prev, S, s, cost[(size_t)t * S + s], bp);
            back[(size_t)t * S + s] = (uint8_t)bp;
        }
    }
    const uint32_t *last = E + (size_t)((T - 1) & 1) * S;
    int32_t s = 0;
    for (int32_t i = 1; i < S; ++i) if (last[i] < last[s]) s = i;
    const uint64_t total = last[s];
    for (int32_t t = T - 1; t >= 0; --t) {
        seam[t] = s;
        if (t > 0) s = seam_back(s, back[(size_t)t * S + s]);
    }
    return total;
}

// does frame k take the pixel whose nearest source pixel is (xn, yn)?  seam = frame k's row of seams
STRIP_HD inline bool seam_side(int32_t orient, const int32_t *seam, int32_t xn, int32_t yn)
{
    const int32_t t = seam_axis(orient) ? yn : xn, s = seam_axis(orient) ? xn : yn;
    return seam_sign(orient) * (s - seam[t]) >= 0;
}

}  // namespace uwip_sm
