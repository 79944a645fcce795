// The arithmetic of baseline JPEG that the host codec of the CLIs (cli/jpeg.hpp) and the device codec (jpeg_encode.hip,
// jpeg_decode.hip) must perform identically, written ONCE for both: one pass of the slow-but-accurate integer DCT pair of
// libjpeg (jidctint / jfdctint, CONST_BITS 13, PASS1_BITS 2), its descaling, the sign extension of a Huffman-coded magnitude
// and the clamp of a dequantised coefficient.  Plain C++ without hipcc; __host__ __device__ under it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

namespace uwip_jpeg {

constexpr int32_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                  F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

JPEG_HD int32_t descale(int32_t x, int n) { return (x + (1 << (n - 1))) >> n; }
JPEG_HD int64_t descale64(int64_t x, int n) { return (x + ((int64_t)1 << (n - 1))) >> n; }

// the value of a t-bit magnitude field v (T.81 F.2.2.1 EXTEND)
JPEG_HD int extend(int v, int t) { return v < (1 << (t - 1)) ? v - (1 << t) + 1 : v; }

// a dequantised coefficient, |v| <= 2^20: a valid stream stays far below, and idct_pass cannot overflow on a corrupt one
JPEG_HD int64_t clamp_coef(int64_t v) { return v > (1 << 20) ? (1 << 20) : (v < -(1 << 20) ? -(1 << 20) : v); }

// One pass of jidctint over 8 values, before its descaling (columns: by 13 - 2; rows: by 13 + 2 + 3, then + 128 and the clamp
// to 0..255).  64-bit temporaries: the same values as libjpeg's 32-bit ones on a valid stream, and no signed overflow for
// |in| <= 2^20 (first pass) and for what the first pass can return (second pass).
JPEG_HD void idct_pass(const int64_t in[8], int64_t o[8])
{
    int64_t z2 = in[2], z3 = in[6];
    int64_t z1 = (z2 + z3) * F0541;
    int64_t tmp2 = z1 + z3 * (-F1847), tmp3 = z1 + z2 * F0765;
    int64_t tmp0 = (in[0] + in[4]) * (1 << 13), tmp1 = (in[0] - in[4]) * (1 << 13);
    const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int64_t z4 = tmp1 + tmp3;
    const int64_t z5 = (z3 + z4) * F1175;
    tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3; o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1; o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}

// One pass of jfdctint over 8 values in place: first the rows (samples - 128 in, results scaled up by 4), then the columns
// (coefficients scaled by 8 out).
JPEG_HD void fdct_pass(int32_t &p0, int32_t &p1, int32_t &p2, int32_t &p3, int32_t &p4, int32_t &p5, int32_t &p6, int32_t &p7,
                       const bool rows)
{
    int32_t tmp0 = p0 + p7, tmp7 = p0 - p7, tmp1 = p1 + p6, tmp6 = p1 - p6;
    int32_t tmp2 = p2 + p5, tmp5 = p2 - p5, tmp3 = p3 + p4, tmp4 = p3 - p4;
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int sh = rows ? 13 - 2 : 13 + 2;
    if (rows) { p0 = (tmp10 + tmp11) * 4; p4 = (tmp10 - tmp11) * 4; }
    else      { p0 = descale(tmp10 + tmp11, 2); p4 = descale(tmp10 - tmp11, 2); }
    int32_t z1 = (tmp12 + tmp13) * F0541;
    p2 = descale(z1 + tmp13 * F0765, sh); p6 = descale(z1 + tmp12 * (-F1847), sh);
    z1 = tmp4 + tmp7;
    int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int32_t z5 = (z3 + z4) * F1175;
    tmp4 *= F0298; tmp5 *= F2053; tmp6 *= F3072; tmp7 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
    z3 += z5; z4 += z5;
    p7 = descale(tmp4 + z1 + z3, sh); p5 = descale(tmp5 + z2 + z4, sh);
    p3 = descale(tmp6 + z2 + z3, sh); p1 = descale(tmp7 + z1 + z4, sh);
}

}  // namespace uwip_jpeg
