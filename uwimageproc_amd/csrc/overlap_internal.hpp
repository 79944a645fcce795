// What the units of the videostrip overlap path share (overlap.hip, overlap_{detect,describe,match,geometry}.hip): the sizes
// of a feature set, the keypoint record, the feature-set object and the launchers that cross unit boundaries.
#pragma once
#include "uwip_internal.hpp"

namespace {      // internal linkage on purpose: kernels take Keypoint by pointer, and every unit keeps the same kernel names

constexpr int NLEV = 4;
constexpr int MAXKP = 2048;
constexpr int DESC_BYTES = 64;     // packed bits
constexpr int DESC_K = 512;        // unpacked 0/1 bytes for the i8 MFMA
constexpr int DESC_NIBW = 64;      // the same 512 bits as FP4 E2M1 nibbles: 64 dwords = 256 bytes (the f8f6f4 MFMA operand)
constexpr int TW = 640, TH = 480;  // TARGET_WIDTH / TARGET_HEIGHT (videostrip.hpp:48-49)

struct Keypoint {
    float x, y, response;
    int32_t level, xi, yi;
    float co, si;        // unit vector of the dominant orientation ((1, 0): upright)
};

// 8 descriptor bits -> 8 FP4 E2M1 nibbles (bit j -> nibble j): 0 -> 0b0000 = 0.0, 1 -> 0b0010 = 1.0
__device__ __forceinline__ uint32_t desc_byte_to_nibbles(uint32_t x)
{
    x = (x | (x << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return x << 1;
}

}  // namespace

// The opaque feature set: everything calcOverlap caches in `struct keyframe`
// (videostrip.hpp:62-68: keypoints + descriptors of a frame), for a batch of frames.
struct uwip_features {
    uwip_ctx *ctx = nullptr;
    int capacity = 0;      // frames
    int frames = 0;        // valid frames
    int w = 0, h = 0;      // working (640-wide) size
    Keypoint *d_kp = nullptr;      // [capacity][MAXKP]
    uint8_t *d_desc = nullptr;     // [capacity][MAXKP][64]   packed
    int8_t *d_bits = nullptr;      // [capacity][MAXKP][512]  0/1 bytes (i8 MFMA operand)
    uint32_t *d_nib = nullptr;     // [capacity][MAXKP][64]   0/1 as FP4 E2M1 nibbles, 0x0 / 0x2 = 0.0 / 1.0 (f8f6f4 MFMA operand)
    int32_t *d_pop = nullptr;      // [capacity][MAXKP]       popcounts
    int32_t *d_n = nullptr;        // [capacity]              keypoint counts
};

// overlap_describe.hip: orientation + descriptor of the keypoints in slots [first_slot, first_slot + F) of `ft`, from the
// level images Lt and the derivative pairs Lxy ([NLEV][F][h][w] each) of the same F frames
int uwip_overlap_describe(uwip_ctx *ctx, const float *Lt, const float2 *Lxy, int h, int w, int F, uwip_features *ft, int first_slot,
                          int upright);
// overlap_match.hip: kNN(2) of every query slot d_pq[p] of `fq` against the train slot d_pt[p] of `ft` -> m_idx / m_dist
// [npairs][MAXKP][2]; d_npairs (null: all npairs): a pair count in device memory, blocks at or beyond it return at once
int uwip_overlap_knn(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft, const int32_t *d_pq, const int32_t *d_pt,
                     const int32_t *d_npairs, int npairs, int32_t *m_idx, int32_t *m_dist);
// overlap_geometry.hip: ratio test + RANSAC homography + overlapArea of the same pairs from that kNN(2) result -> d_ratio
// [npairs], info [npairs][8], d_H (may be null) [npairs][9]
int uwip_overlap_geometry(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft, const int32_t *d_pq, const int32_t *d_pt,
                          const int32_t *d_npairs, int npairs, const int32_t *m_idx, const int32_t *m_dist, int videoWidth,
                          int videoHeight, uint32_t seed, int min_inliers, float *d_ratio, int32_t *info, double *d_H);
