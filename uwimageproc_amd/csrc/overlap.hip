// videostrip overlap path for gfx950.
//
// calcOverlap (modules/videostrip/src/videostrip.cpp:192-289) = resize ->
// gray -> detect+describe -> brute-force kNN(2) -> ratio test -> RANSAC
// homography -> overlapArea.  The reference delegates detect/describe/match to
// OpenCV-contrib SURF + L2 BFMatcher; BASELINE.json's north_star replaces them
// with an AKAZE-style detector, binary descriptors and a Hamming matcher whose
// dense distance matrix runs on MFMA.  The algorithm is specified in
// DESIGN.md ("overlap stage") and restated independently in
// oracle/uwip_oracle_overlap.c; every float kernel here keeps that
// specification's operation order (-ffp-contract=off), so keypoints,
// descriptors and matches are bit-exact against the oracle.
//
// Everything is batched: one launch covers all frames (grid.z), because a
// 640x360 working image is far too small to fill 256 CUs on its own.
//
// This unit holds the feature-set object and the matching entry points; the stages live in overlap_detect.hip,
// overlap_describe.hip, overlap_match.hip and overlap_geometry.hip (overlap_internal.hpp: what they share).
#include "overlap_internal.hpp"
#include <cstring>
#include <new>

namespace {
constexpr int MIN_INLIERS = 4;       // default = the reference's rule: whatever findHomography returns for >= 4 good matches
                                     // (videostrip.cpp:252-272), i.e. any hypothesis with >= 4 inliers
constexpr int MIN_INLIERS_STRICT = 6;   // UWIP_OVERLAP_MIN6 (uwip_overlap_match_ex): fewer inliers = no homography (-2.0): four chance
                                        // matches always fit one
}  // namespace

// ---- exported entry points -------------------------------------------------------------------------------------

UWIP_API int uwip_features_create(uwip_ctx *ctx, int max_frames, uwip_features **out)
{
    if (!ctx || !out) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, max_frames >= 1 && max_frames <= 4096, "max_frames must be in [1,4096]");
    uwip_features *f = new (std::nothrow) uwip_features();
    if (!f) return UWIP_ERR_NOMEM;
    f->ctx = ctx; f->capacity = max_frames;
    const size_t K = (size_t)max_frames * MAXKP;
    if (hipMalloc(&f->d_kp, K * sizeof(Keypoint)) != hipSuccess || hipMalloc(&f->d_desc, K * DESC_BYTES) != hipSuccess ||
        hipMalloc(&f->d_bits, K * DESC_K) != hipSuccess || hipMalloc(&f->d_nib, K * DESC_NIBW * 4) != hipSuccess ||
        hipMalloc(&f->d_pop, K * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&f->d_n, sizeof(int32_t) * max_frames) != hipSuccess) {
        (void)hipFree(f->d_kp); (void)hipFree(f->d_desc); (void)hipFree(f->d_bits); (void)hipFree(f->d_nib); (void)hipFree(f->d_pop); (void)hipFree(f->d_n);
        delete f;
        return ctx->fail(UWIP_ERR_NOMEM, "feature set hipMalloc");
    }
    uwip_trace_range(ctx, "device", "features.kp", f->d_kp, K * sizeof(Keypoint));
    uwip_trace_range(ctx, "device", "features.desc", f->d_desc, K * DESC_BYTES);
    uwip_trace_range(ctx, "device", "features.bits", f->d_bits, K * DESC_K);
    uwip_trace_range(ctx, "device", "features.pop", f->d_pop, K * sizeof(int32_t));
    (void)hipMemsetAsync(f->d_n, 0, sizeof(int32_t) * max_frames, ctx->stream);
    (void)hipMemsetAsync(f->d_bits, 0, K * DESC_K, ctx->stream);
    (void)hipMemsetAsync(f->d_nib, 0, K * DESC_NIBW * 4, ctx->stream);
    (void)hipMemsetAsync(f->d_pop, 0, K * sizeof(int32_t), ctx->stream);
    *out = f;
    return UWIP_OK;
}

UWIP_API int uwip_features_destroy(uwip_features *f)
{
    if (!f) return UWIP_OK;
    (void)hipSetDevice(f->ctx->device);
    (void)uwip_stream_wait(f->ctx);
    (void)hipFree(f->d_kp); (void)hipFree(f->d_desc); (void)hipFree(f->d_bits); (void)hipFree(f->d_nib); (void)hipFree(f->d_pop); (void)hipFree(f->d_n);
    delete f;
    return UWIP_OK;
}

// tap for tests: one slot's keypoints / packed descriptors to the host
UWIP_API int uwip_features_download(uwip_ctx *ctx, const uwip_features *feats, int slot, void *h_kps /*[2048] 32-byte records*/,
                                    uint8_t *h_desc /*[2048][64]*/, int32_t *h_count)
{
    if (!ctx || !feats) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, slot >= 0 && slot < feats->capacity, "slot out of range");
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    if (h_count) UWIP_HIP(ctx, hipMemcpy(h_count, feats->d_n + slot, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (h_kps) UWIP_HIP(ctx, hipMemcpy(h_kps, feats->d_kp + (size_t)slot * MAXKP, sizeof(Keypoint) * MAXKP, hipMemcpyDeviceToHost));
    if (h_desc) UWIP_HIP(ctx, hipMemcpy(h_desc, feats->d_desc + (size_t)slot * MAXKP * DESC_BYTES, (size_t)MAXKP * DESC_BYTES, hipMemcpyDeviceToHost));
    return UWIP_OK;
}

// The opposite direction: fill one slot from host keypoints / packed descriptors (the reference's `struct keyframe`
// has public keypoints / descriptors members that a caller may fill itself, videostrip.hpp:62-68); also how the
// matcher is measured on a full 2048 x 2048 descriptor set.  Rows >= count are zeroed.
namespace {
__global__ __launch_bounds__(256) void k_ov_unpack_desc(const uint8_t *__restrict__ desc, int count, int8_t *__restrict__ bits,
                                                       uint32_t *__restrict__ nib, int32_t *__restrict__ pop)
{
    const int k = blockIdx.x;                         // keypoint
    const int t = threadIdx.x;                        // 2 bits per thread -> 512
    const uint8_t *d = desc + (size_t)k * DESC_BYTES;
    const bool live = k < count;
    const int b0 = live ? (d[(2 * t) >> 3] >> ((2 * t) & 7)) & 1 : 0, b1 = live ? (d[(2 * t + 1) >> 3] >> ((2 * t + 1) & 7)) & 1 : 0;
    bits[(size_t)k * DESC_K + 2 * t] = (int8_t)b0;
    bits[(size_t)k * DESC_K + 2 * t + 1] = (int8_t)b1;
    if (t < DESC_NIBW) nib[(size_t)k * DESC_NIBW + t] = live ? desc_byte_to_nibbles(d[t]) : 0u;
    __shared__ int s_c[4];
    int c = b0 + b1;
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) c += __shfl_xor(c, sft, 64);
    if ((t & 63) == 0) s_c[t >> 6] = c;
    __syncthreads();
    if (t == 0) pop[k] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
}
}  // namespace

UWIP_API int uwip_features_upload(uwip_ctx *ctx, uwip_features *feats, int slot, int rows, int cols, const void *h_kps,
                                  const uint8_t *h_desc, int32_t count)
{
    if (!ctx || !feats) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, feats->ctx == ctx, "feature set of another context");
    UWIP_REQUIRE(ctx, slot >= 0 && slot < feats->capacity, "slot out of range");
    UWIP_REQUIRE(ctx, count >= 0 && count <= MAXKP, "count out of range");
    UWIP_REQUIRE(ctx, rows > 0 && cols > 0 && (feats->w == 0 || (feats->w == cols && feats->h == rows)), "working size mismatch");
    UWIP_REQUIRE(ctx, count == 0 || (h_kps && h_desc), "null buffer");
    feats->w = cols; feats->h = rows;
    uint8_t *stage = (uint8_t *)uwip_ws(ctx, "ov.upload.desc", (size_t)MAXKP * DESC_BYTES);
    if (!stage) return UWIP_ERR_NOMEM;
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    if (count) {
        UWIP_HIP(ctx, hipMemcpy(stage, h_desc, (size_t)count * DESC_BYTES, hipMemcpyHostToDevice));
        UWIP_HIP(ctx, hipMemcpy(feats->d_kp + (size_t)slot * MAXKP, h_kps, sizeof(Keypoint) * (size_t)count, hipMemcpyHostToDevice));
        UWIP_HIP(ctx, hipMemcpy(feats->d_desc + (size_t)slot * MAXKP * DESC_BYTES, h_desc, (size_t)count * DESC_BYTES, hipMemcpyHostToDevice));
    }
    UWIP_HIP(ctx, hipMemcpy(feats->d_n + slot, &count, sizeof(int32_t), hipMemcpyHostToDevice));
    k_ov_unpack_desc<<<MAXKP, 256, 0, ctx->stream>>>(stage, count, feats->d_bits + (size_t)slot * MAXKP * DESC_K,
                                                     feats->d_nib + (size_t)slot * MAXKP * DESC_NIBW, feats->d_pop + (size_t)slot * MAXKP);
    UWIP_HIP(ctx, hipGetLastError());
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    return UWIP_OK;
}

// The matcher and the geometry on pair lists already in device memory: d_pq / d_pt [npairs] slot indices.  d_npairs
// (null: all npairs) is a count the device itself wrote: the launches cover npairs pairs, the blocks at or beyond the count
// return at once (the key-frame chain's fallback rounds, kf_chain.hpp).
static int launch_match(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft, const int32_t *d_pq, const int32_t *d_pt,
                        const int32_t *d_npairs, int npairs, int videoWidth, int videoHeight, uint32_t seed, int min_inliers,
                        float *d_ratio, int32_t *info, double *d_H, int32_t *m_idx, int32_t *m_dist)
{
    if (int rc = uwip_overlap_knn(ctx, fq, ft, d_pq, d_pt, d_npairs, npairs, m_idx, m_dist)) return rc;
    return uwip_overlap_geometry(ctx, fq, ft, d_pq, d_pt, d_npairs, npairs, m_idx, m_dist, videoWidth, videoHeight, seed, min_inliers,
                                 d_ratio, info, d_H);
}

// match query slots against train slots and turn each pair into an overlap ratio.
// h_pair_q / h_pair_t: host arrays of slot indices (query = object frame, train = key frame).
// d_ratio [npairs]: overlap ratio or -2.0 (videostrip.cpp:252-256,272).  d_info (may be NULL) [npairs][8]:
// nkp_obj, nkp_key, ngood, ninliers, overlap pixel count.  d_H (may be NULL) [npairs][9].
// d_match_idx / d_match_dist (may be NULL) [npairs][2048][2]: the kNN(2) result.
UWIP_API int uwip_overlap_match(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft, const int32_t *h_pair_q,
                                const int32_t *h_pair_t, int npairs, int videoWidth, int videoHeight, uint32_t seed,
                                float *d_ratio, int32_t *d_info, double *d_H, int32_t *d_match_idx, int32_t *d_match_dist)
{
    return uwip_overlap_match_ex(ctx, fq, ft, h_pair_q, h_pair_t, npairs, videoWidth, videoHeight, seed, 0u, d_ratio, d_info, d_H,
                                 d_match_idx, d_match_dist);
}

UWIP_API int uwip_overlap_match_ex(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft, const int32_t *h_pair_q,
                                   const int32_t *h_pair_t, int npairs, int videoWidth, int videoHeight, uint32_t seed, unsigned flags,
                                   float *d_ratio, int32_t *d_info, double *d_H, int32_t *d_match_idx, int32_t *d_match_dist)
{
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, (flags & ~(unsigned)(UWIP_OVERLAP_MIN4 | UWIP_OVERLAP_MIN6)) == 0, "unknown flag");
    UWIP_REQUIRE(ctx, (flags & (UWIP_OVERLAP_MIN4 | UWIP_OVERLAP_MIN6)) != (UWIP_OVERLAP_MIN4 | UWIP_OVERLAP_MIN6), "UWIP_OVERLAP_MIN4 and UWIP_OVERLAP_MIN6 exclude each other");
    const int min_inliers = (flags & UWIP_OVERLAP_MIN6) ? MIN_INLIERS_STRICT : MIN_INLIERS;
    UWIP_REQUIRE(ctx, fq && ft && fq->ctx == ctx && ft->ctx == ctx, "bad feature sets");
    UWIP_REQUIRE(ctx, npairs >= 0 && npairs <= 65535, "npairs out of range");
    if (npairs == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, h_pair_q && h_pair_t && d_ratio, "null buffer");
    UWIP_REQUIRE(ctx, fq->w == ft->w && fq->h == ft->h && fq->w > 0, "feature sets of different working sizes");
    for (int p = 0; p < npairs; ++p)
        UWIP_REQUIRE(ctx, h_pair_q[p] >= 0 && h_pair_q[p] < fq->capacity && h_pair_t[p] >= 0 && h_pair_t[p] < ft->capacity, "pair slot out of range");
    int32_t *h_pairs = (int32_t *)uwip_host_ws(ctx, "ov.pairs", sizeof(int32_t) * 2 * (size_t)npairs);
    int32_t *d_pairs = (int32_t *)uwip_ws(ctx, "ov.pairs", sizeof(int32_t) * 2 * (size_t)npairs);
    int32_t *m_idx = d_match_idx ? d_match_idx : (int32_t *)uwip_ws(ctx, "ov.midx", sizeof(int32_t) * 2 * MAXKP * (size_t)npairs);
    int32_t *m_dist = d_match_dist ? d_match_dist : (int32_t *)uwip_ws(ctx, "ov.mdist", sizeof(int32_t) * 2 * MAXKP * (size_t)npairs);
    int32_t *info = d_info ? d_info : (int32_t *)uwip_ws(ctx, "ov.info", sizeof(int32_t) * 8 * (size_t)npairs);
    if (!h_pairs || !d_pairs || !m_idx || !m_dist || !info) return UWIP_ERR_NOMEM;
    // the same pair list as last time (every batch of a stream: frame i against frame i - 1) is already in d_pairs: nothing
    // to stage, and the host does not have to wait for the stream before reusing the pinned buffer
    const bool same = ctx->ov_pairs_dev == d_pairs && ctx->ov_pairs_host.size() == 2 * (size_t)npairs &&
                      memcmp(ctx->ov_pairs_host.data(), h_pair_q, sizeof(int32_t) * npairs) == 0 &&
                      memcmp(ctx->ov_pairs_host.data() + npairs, h_pair_t, sizeof(int32_t) * npairs) == 0;
    if (!same) {
        UWIP_HIP(ctx, uwip_stream_wait(ctx));          // pinned staging reuse
        memcpy(h_pairs, h_pair_q, sizeof(int32_t) * npairs);
        memcpy(h_pairs + npairs, h_pair_t, sizeof(int32_t) * npairs);
        UWIP_HIP(ctx, hipMemcpyAsync(d_pairs, h_pairs, sizeof(int32_t) * 2 * (size_t)npairs, hipMemcpyHostToDevice, ctx->stream));
        ctx->ov_pairs_host.assign(h_pairs, h_pairs + 2 * (size_t)npairs);
        ctx->ov_pairs_dev = d_pairs;
    }
    return launch_match(ctx, fq, ft, d_pairs, d_pairs + npairs, nullptr, npairs, videoWidth, videoHeight, seed, min_inliers, d_ratio,
                        info, d_H, m_idx, m_dist);
}

// keep a frame's cached keypoints/descriptors (what `struct keyframe` holds) in another slot
UWIP_API int uwip_features_copy(uwip_ctx *ctx, const uwip_features *src, int src_slot, uwip_features *dst, int dst_slot)
{
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, src && dst && src->ctx == ctx && dst->ctx == ctx, "bad feature sets");
    UWIP_REQUIRE(ctx, src_slot >= 0 && src_slot < src->capacity && dst_slot >= 0 && dst_slot < dst->capacity, "slot out of range");
    UWIP_REQUIRE(ctx, dst->w == 0 || (dst->w == src->w && dst->h == src->h), "feature sets of different working sizes");
    if (src == dst && src_slot == dst_slot) return UWIP_OK;
    dst->w = src->w; dst->h = src->h;
    const size_t s = (size_t)src_slot * MAXKP, d = (size_t)dst_slot * MAXKP;
    UWIP_HIP(ctx, hipMemcpyAsync(dst->d_kp + d, src->d_kp + s, sizeof(Keypoint) * MAXKP, hipMemcpyDeviceToDevice, ctx->stream));
    UWIP_HIP(ctx, hipMemcpyAsync(dst->d_desc + d * DESC_BYTES, src->d_desc + s * DESC_BYTES, (size_t)MAXKP * DESC_BYTES, hipMemcpyDeviceToDevice, ctx->stream));
    UWIP_HIP(ctx, hipMemcpyAsync(dst->d_bits + d * DESC_K, src->d_bits + s * DESC_K, (size_t)MAXKP * DESC_K, hipMemcpyDeviceToDevice, ctx->stream));
    UWIP_HIP(ctx, hipMemcpyAsync(dst->d_nib + d * DESC_NIBW, src->d_nib + s * DESC_NIBW, (size_t)MAXKP * DESC_NIBW * 4, hipMemcpyDeviceToDevice, ctx->stream));
    UWIP_HIP(ctx, hipMemcpyAsync(dst->d_pop + d, src->d_pop + s, sizeof(int32_t) * MAXKP, hipMemcpyDeviceToDevice, ctx->stream));
    UWIP_HIP(ctx, hipMemcpyAsync(dst->d_n + dst_slot, src->d_n + src_slot, sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    return UWIP_OK;
}

// ---- the key-frame chain's device-side entry points (pipe.cpp, kf_chain.hpp) -------------------------------------

int uwip_overlap_match_dev(uwip_ctx *ctx, const uwip_features *f, const int32_t *d_pq, const int32_t *d_pt, const int32_t *d_npairs,
                           int npairs, int videoWidth, int videoHeight, uint32_t seed, unsigned flags, float *d_ratio, int32_t *d_info,
                           int32_t *m_idx, int32_t *m_dist)
{
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, f && f->ctx == ctx && f->w > 0, "bad feature set");
    UWIP_REQUIRE(ctx, npairs >= 0 && npairs <= 65535, "npairs out of range");
    UWIP_REQUIRE(ctx, d_pq && d_pt && d_ratio && d_info && m_idx && m_dist, "null buffer");
    if (npairs == 0) return UWIP_OK;
    const int min_inliers = (flags & UWIP_OVERLAP_MIN6) ? MIN_INLIERS_STRICT : MIN_INLIERS;
    return launch_match(ctx, f, f, d_pq, d_pt, d_npairs, npairs, videoWidth, videoHeight, seed, min_inliers, d_ratio, d_info, nullptr,
                        m_idx, m_dist);
}

size_t uwip_overlap_match_scratch_bytes(int npairs) { return sizeof(int32_t) * 2 * MAXKP * (size_t)npairs; }

namespace {
// job j = blockIdx.y copies slot src[j] to slot dst_j (src[j] < 0: nothing); the slot indices come from device memory
__global__ __launch_bounds__(256) void k_kf_slot_copy(Keypoint *kp, uint8_t *desc, int8_t *bits, uint32_t *nib, int32_t *pop,
                                                      int32_t *nkp, int capacity, const int32_t *__restrict__ src, int dst0, int dst1)
{
    const int s = src[blockIdx.y], d = blockIdx.y == 0 ? dst0 : dst1;
    if (s < 0 || s >= capacity || s == d) return;
    struct Part { uint4 *base; size_t n16; };        // per-slot bytes / 16 of each array
    const Part parts[5] = {{reinterpret_cast<uint4 *>(kp), sizeof(Keypoint) * MAXKP / 16},
                           {reinterpret_cast<uint4 *>(desc), (size_t)MAXKP * DESC_BYTES / 16},
                           {reinterpret_cast<uint4 *>(bits), (size_t)MAXKP * DESC_K / 16},
                           {reinterpret_cast<uint4 *>(nib), (size_t)MAXKP * DESC_NIBW * 4 / 16},
                           {reinterpret_cast<uint4 *>(pop), (size_t)MAXKP * 4 / 16}};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (int a = 0; a < 5; ++a) {
        const uint4 *from = parts[a].base + (size_t)s * parts[a].n16;
        uint4 *to = parts[a].base + (size_t)d * parts[a].n16;
        for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < parts[a].n16; k += stride) to[k] = from[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) nkp[d] = nkp[s];
}
}  // namespace

int uwip_features_copy_dev(uwip_ctx *ctx, uwip_features *f, const int32_t *d_src, int dst0, int dst1)
{
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, f && f->ctx == ctx, "bad feature set");
    UWIP_REQUIRE(ctx, dst0 >= 0 && dst0 < f->capacity && dst1 >= 0 && dst1 < f->capacity && dst0 != dst1, "slot out of range");
    uwip_kscope ks(ctx, "k_kf_slot_copy");
    k_kf_slot_copy<<<dim3(64, 2), 256, 0, ctx->stream>>>(f->d_kp, f->d_desc, f->d_bits, f->d_nib, f->d_pop, f->d_n, f->capacity, d_src,
                                                       dst0, dst1);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}
