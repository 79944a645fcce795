// Internal definitions shared by the HIP translation units of libuwip.so.
// gfx950 (MI355X) only: wave = 64 lanes, 160 KiB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
#include "../../include/uwip.h"
#include "kf_chain.hpp"

#define UWIP_API extern "C" __attribute__((visibility("default")))

struct uwip_prof_rec {
    std::string name;
    double total_ms = 0.0;
    uint64_t launches = 0;
};

struct uwip_ws_buf {
    void *ptr = nullptr;
    size_t bytes = 0;
};

struct uwip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // named, grow-only device workspaces: no hipMalloc in steady state
    std::map<std::string, uwip_ws_buf> ws;
    // named pinned host staging buffers
    std::map<std::string, uwip_ws_buf> hs;
    // immutable device tables keyed by their geometry (strip / cell lists)
    std::map<std::string, uwip_ws_buf> tables;
    // kernels whose > 64 KiB dynamic-LDS opt-in (hipFuncSetAttribute) has been made on this device
    std::map<std::string, bool> lds_optin;
    int ov_last_frames = 0;        // batch size of the most recent uwip_overlap_detect (debug taps)
    // the parameters the most recent uwip_aclahe_auto_ex chose: on the host (the synchronous forms) or still on the device
    // (UWIP_ACLAHE_ASYNC: workspace "auto.par", [n][4] int32) -- uwip_aclahe_last_params
    int aclahe_last_n = 0;
    bool aclahe_last_on_device = false;
    std::vector<int32_t> aclahe_last_host;      // [n][4] = BS, CL, need, 0 (the layout of "auto.par")
    // the pair list uwip_overlap_match last uploaded (a stream of batches sends the same one every time: no re-upload,
    // and no host wait for the staging buffer)
    std::vector<int32_t> ov_pairs_host;
    const void *ov_pairs_dev = nullptr;
    // profiling
    bool prof = false;
    std::vector<uwip_prof_rec> prof_recs;
    std::map<std::string, int> prof_index;
    struct pending_t { int rec; hipEvent_t a, b; };
    std::vector<pending_t> prof_pending;
    std::vector<hipEvent_t> event_pool;
    // host waits: an event recorded behind the stream's work and polled with sleeps in between, so the calling thread
    // does not burn a core until the stream has drained (hipStreamSynchronize / hipEventSynchronize spin on this runtime,
    // blocking-sync events included: eight sub-batch threads of a rank burned eight cores, measured host_cpu_s_per_step
    // 1.59 s per 0.177 s step); UWIP_CTX_SPIN_WAIT keeps the spinning wait
    hipEvent_t wait_ev = nullptr;
    // uwip_jpeg_decode: recorded behind the upload out of the page-locked staging buffer, polled before the next call refills it
    hipEvent_t jpd_ev = nullptr;
    hipEvent_t pngd_ev = nullptr;               // the same for uwip_png_decode's staging buffer
    bool spin_wait = false;

    int fail(int code, const char *what, const char *detail = nullptr)
    {
        err = what;
        if (detail) { err += ": "; err += detail; }
        return code;
    }
};

// Wait on the host until everything queued on the context's stream has finished (sleeping, see uwip_ctx::wait_ev).
hipError_t uwip_stream_wait(uwip_ctx *ctx);
hipError_t uwip_event_wait(hipEvent_t ev, int max_sleep_us);      // hipEventQuery + nanosleep back-off (ctx.hip)
void *uwip_ws(uwip_ctx *ctx, const char *name, size_t bytes);       // nullptr on failure (ctx->err set)
void *uwip_host_ws(uwip_ctx *ctx, const char *name, size_t bytes);  // pinned host
// Cached immutable device table: uploaded once (blocking) the first time `key` is seen.
const void *uwip_table_find(uwip_ctx *ctx, const std::string &key, size_t *bytes);
const void *uwip_table_put(uwip_ctx *ctx, const std::string &key, const void *host, size_t bytes);
int uwip_prof_flush(uwip_ctx *ctx);
// UWIP_TRACE_ALLOC=1: report an allocation's address range on stderr (attributing a GPU fault address to a buffer)
void uwip_trace_range(const uwip_ctx *ctx, const char *kind, const char *name, const void *p, size_t bytes);
// colorspace.hip: in-place 8-bit BGR -> HSV -> BGR (an HSV letter of histretch)
int uwip_hsv_roundtrip(uwip_ctx *ctx, const uwip_batch_u8 *img);
// winfilter15.hip: 15x15 window max and/or min of interleaved 3-channel u8 frames -> planar [F][3][H][W]
bool uwip_winfilter15_ok(const uint8_t *img, size_t step, size_t fs, int H, int W, int w);
// stats (optional, both filters only): stats[f*stride + {0..3}] = min, max of all channels, min, max of channel 2,
// by atomicMin / atomicMax onto the caller's 255 / 0 initial values
int uwip_winfilter15(uwip_ctx *ctx, const uint8_t *img, size_t step, size_t fs, int F, int H, int W, uint8_t *out_max,
                     uint8_t *out_min, int *stats = nullptr, int stats_stride = 0, unsigned long long *redsum = nullptr);
// guided_filter_ws.hip: the wave-strip guided filter (guide u8 x3, P [F][np][H][W] -> Q, AB [F*np][4][H][W] scratch)
// Optional 8-bit source of p (bgdehaze's transmission): plane ip of frame f is max(1 - normv(m) / B_ip, tmin) of the u8
// plane m = planes[(f * nplanes + ip)][H][W], and 1 where the w x w window around the pixel leaves the image;
// B_ip = sc[f * sc_stride + b_off + ip], normv by the frame's gnorm pair.
struct uwip_gf_pu8 {
    const uint8_t *planes = nullptr;
    int nplanes = 0;
    const double *sc = nullptr;
    int sc_stride = 0, b_off = 0;
    double tmin = 0.0;
    int w = 0, pad = 0;
};
// Optional fused scene recovery (bgdehaze D5) in the second kernel: Q receives J_ip = (normv(I_ip) - B_ip) / q + B_ip
// instead of q, and part[(z * nb + block) * 3 + {0,1,2}] the per-block min / max / sum of J (z = f * np + ip; `part` and
// `nb` are filled in by uwip_gf_wave_strip).  Aligned path only.
struct uwip_gf_recover {
    const double *sc = nullptr;
    int sc_stride = 0, b_off = 0;
    double *part = nullptr;
    int nb = 0;
};
// true when the 8-bit p source can be used for this geometry (aligned rows, W and r multiples of 4, np = 2)
bool uwip_gf_pu8_ok(const uint8_t *guide, size_t step, size_t fs, const uint8_t *planes, int np, int W, int r);
int uwip_gf_wave_strip(uwip_ctx *ctx, const uint8_t *guide, size_t step, size_t fs, const int *gnorm, int gstride,
                       const double *P, double *Q, double *AB, int F, int np, int H, int W, int r, double eps,
                       const uwip_gf_pu8 *pu8 = nullptr, uwip_gf_recover *rec = nullptr);
// Test / measurement hooks (UWIP_ACLAHE_TEST_FORCE_CL, UWIP_DIAG_GF_ONLY) are dead unless the process was started with
// UWIP_TEST_HOOKS=1 in its environment: read ONCE, at the first call; a product process never looks at the hook variables.
inline bool uwip_test_hooks()
{
    static const bool on = [] { const char *e = std::getenv("UWIP_TEST_HOOKS"); return e && *e == '1'; }();
    return on;
}
// UWIP_ACLAHE_TEST_FORCE_CL: the clip limit (a knee index) the aclahe stage's choice gives every frame, -1 when unset.  A
// knee index >= 26 takes a degenerate fit: the tests force one to reach the exact block-size search.  Read at
// every call (a test sets it around one call).
inline int uwip_test_force_cl()
{
    const char *e = uwip_test_hooks() ? std::getenv("UWIP_ACLAHE_TEST_FORCE_CL") : nullptr;
    return e && *e ? std::atoi(e) : -1;
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (context, kernel)
int uwip_lds_optin(uwip_ctx *ctx, const char *name, const void *func, size_t bytes);
// overlap.hip, for the key-frame chain (kf_chain.hpp): uwip_overlap_match_ex on a pair list already in device memory, d_pq /
// d_pt [npairs] slots of `f` (query, train); d_npairs (null: all npairs) a pair count the device wrote, blocks at or beyond
// it return at once.  m_idx / m_dist: caller scratch of uwip_overlap_match_scratch_bytes(npairs) bytes each.
int uwip_overlap_match_dev(uwip_ctx *ctx, const uwip_features *f, const int32_t *d_pq, const int32_t *d_pt, const int32_t *d_npairs,
                           int npairs, int videoWidth, int videoHeight, uint32_t seed, unsigned flags, float *d_ratio, int32_t *d_info,
                           int32_t *m_idx, int32_t *m_dist);
size_t uwip_overlap_match_scratch_bytes(int npairs);
// copy slot d_src[0] to slot dst0 and slot d_src[1] to slot dst1 of `f`; the source slots are read on the device (< 0: no copy)
int uwip_features_copy_dev(uwip_ctx *ctx, uwip_features *f, const int32_t *d_src, int dst0, int dst1);
// kf_chain.hip: one walker call of the key-frame chain (kf_chain.hpp) on the device
int uwip_kf_walk(uwip_ctx *ctx, const uwip_kf::Batch &b, uwip_kf::State *d_state, const uwip_kf::Bufs &u, int round);

// jpeg_encode.hip / png_encode.hip: uwip_jpeg_encode / uwip_png_encode with a frame count the device wrote.  d_count (null:
// all frames) is read by every kernel: a frame at or beyond it returns at once and reports size 0.
int uwip_jpeg_encode_dev(uwip_ctx *ctx, const uwip_batch_u8 *frames, int quality, uint8_t *d_streams, size_t slot_bytes,
                         int64_t *d_sizes, const int32_t *d_count);
int uwip_png_encode_dev(uwip_ctx *ctx, const uwip_batch_u8 *frames, int filter, uint8_t *d_streams, size_t slot_bytes,
                        int64_t *d_sizes, const int32_t *d_count);
// pipe_streams.hip: the kernels of uwip_pipe_step_streams between decoders, stages and encoders (pipe_streams.hpp)
namespace uwip_ps { struct Step; }
int uwip_ps_blank(uwip_ctx *ctx, uint8_t *d_frames, int F, size_t frame_bytes, const int32_t *d_status);
int uwip_ps_select_gather(uwip_ctx *ctx, const uwip_ps::Step &s);
int uwip_ps_pack(uwip_ctx *ctx, const uwip_ps::Step &s, const int64_t *d_sizes, const float *d_ratio, const int32_t *d_par,
                 const uint8_t *d_slots, size_t slot_bytes, uint8_t *d_table, uint8_t *d_blob);

#define UWIP_HIP(ctx, expr)                                                         \
    do {                                                                             \
        hipError_t e__ = (expr);                                                     \
        if (e__ != hipSuccess) return (ctx)->fail(UWIP_ERR_HIP, #expr, hipGetErrorString(e__)); \
    } while (0)

#define UWIP_REQUIRE(ctx, cond, msg)                                   \
    do {                                                               \
        if (!(cond)) return (ctx)->fail(UWIP_ERR_INVALID, msg, #cond); \
    } while (0)

// RAII launch bracket: when profiling is on, records events around a kernel.
struct uwip_kscope {
    uwip_ctx *ctx;
    int rec = -1;
    hipEvent_t a = nullptr, b = nullptr;
    uwip_kscope(uwip_ctx *c, const char *name);
    ~uwip_kscope();
};

// The back end that a codec's host sequence is written against: the sequences (function templates in the first anonymous
// namespace of jpeg_encode.hip, jpeg_decode.hip, png_encode.hip and png_decode.hip) take no context, only this -- the device
// here, host threads in tests/hip_on_host.hpp, where the emulation harnesses run the same text under the sanitizers.  The first
// failure sticks: every later operation does nothing, and the entry point returns finish().
struct uwip_device {
    using dim3 = ::dim3;
    uwip_ctx *ctx;
    int rc = UWIP_OK;
    explicit uwip_device(uwip_ctx *c) : ctx(c) {}
    // `count` elements of T, the named workspace: valid until the context's next call of the same entry point
    template <class T> T *array(const char *name, size_t count)
    {
        if (rc) return nullptr;
        T *p = static_cast<T *>(uwip_ws(ctx, name, count * sizeof(T)));
        if (!p) rc = UWIP_ERR_NOMEM;
        return p;
    }
    void fill(void *p, int value, size_t bytes) { if (!rc) hip(hipMemsetAsync(p, value, bytes, ctx->stream), "hipMemsetAsync"); }
    void copy(void *dst, const void *src, size_t bytes)          // device to device
    {
        if (!rc) hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync");
    }
    // name: what the profile calls this launch (not always the kernel's own name)
    template <class... P, class... A> void launch(const char *name, void (*kernel)(P...), dim3 grid, unsigned block, A... args)
    {
        if (rc) return;
        uwip_kscope ks(ctx, name);
        kernel<<<grid, block, 0, ctx->stream>>>(static_cast<P>(args)...);
    }
    int finish()
    {
        if (!rc) hip(hipGetLastError(), "hipGetLastError()");
        return rc;
    }
    void hip(hipError_t e, const char *what) { if (e != hipSuccess) rc = ctx->fail(UWIP_ERR_HIP, what, hipGetErrorString(e)); }
};

// First statement of every entry point that allocates, copies or launches: makes the context's device the calling
// thread's current one (hipSetDevice is thread-local state; a second host thread or a device != 0 would otherwise
// hipMalloc / launch on whatever device that thread last used).
static inline int uwip_enter(uwip_ctx *ctx)
{
    if (!ctx) return UWIP_ERR_INVALID;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return ctx->fail(UWIP_ERR_HIP, "hipSetDevice", hipGetErrorString(e));
    return UWIP_OK;
}

static inline int uwip_check_batch(uwip_ctx *ctx, const uwip_batch_u8 *b, int channels /*0=any*/)
{
    if (int rc0 = uwip_enter(ctx)) return rc0;
    UWIP_REQUIRE(ctx, b != nullptr, "null batch");
    UWIP_REQUIRE(ctx, b->rows >= 0 && b->cols >= 0 && b->frames >= 0, "negative extent");
    UWIP_REQUIRE(ctx, b->channels == 1 || b->channels == 3, "channels must be 1 or 3");
    if (channels) UWIP_REQUIRE(ctx, b->channels == channels, "wrong channel count");
    UWIP_REQUIRE(ctx, b->step >= (size_t)b->cols * b->channels, "step smaller than a row");
    if (b->frames > 1) UWIP_REQUIRE(ctx, b->frame_stride >= b->step * (size_t)b->rows, "frame_stride smaller than a frame");
    if ((size_t)b->rows * b->cols * b->frames > 0) UWIP_REQUIRE(ctx, b->data != nullptr, "null data");
    UWIP_REQUIRE(ctx, (uint64_t)b->rows * (uint64_t)b->cols < (1ull << 31), "frame too large");
    return UWIP_OK;
}

static inline bool uwip_batch_empty(const uwip_batch_u8 *b)
{
    return (size_t)b->rows * b->cols * b->frames == 0;
}

// two single-channel batches of one shape
static inline int uwip_check_pair(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst)
{
    int rc = uwip_check_batch(ctx, src, 1);
    if (rc) return rc;
    rc = uwip_check_batch(ctx, dst, 1);
    if (rc) return rc;
    UWIP_REQUIRE(ctx, src->rows == dst->rows && src->cols == dst->cols && src->frames == dst->frames,
                 "src/dst shape mismatch");
    return UWIP_OK;
}

// base address, row step and (with more than one frame) frame stride are multiples of `a` bytes
static inline bool uwip_aligned_for(const uwip_batch_u8 *b, size_t a)
{
    return ((uintptr_t)b->data % a == 0) && (b->step % a == 0) && (b->frames <= 1 || b->frame_stride % a == 0);
}

static inline unsigned uwip_cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// ---- what the JPEG and the PNG codec's entry points share --------------------------------------------------------------------
// uwip_jpeg_decode / uwip_png_decode: the checks on (h_streams, h_sizes, n, out, d_status); n == 0 passes, the caller returns
static inline int uwip_check_streams(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                                     const int32_t *d_status)
{
    UWIP_REQUIRE(ctx, n >= 0 && n <= 65535, "at most 65535 frames per call");
    UWIP_REQUIRE(ctx, out->frames == n, "the batch must hold one frame per stream");
    if (n == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, h_streams != nullptr && h_sizes != nullptr && d_status != nullptr, "null argument");
    UWIP_REQUIRE(ctx, out->rows >= 1 && out->cols >= 1, "empty frame");
    for (int f = 0; f < n; ++f) UWIP_REQUIRE(ctx, h_streams[f] != nullptr || h_sizes[f] == 0, "null stream");
    for (int f = 0; f < n; ++f) UWIP_REQUIRE(ctx, h_sizes[f] < ((size_t)1 << 28), "a stream of 256 MiB or more");
    return UWIP_OK;
}

// uwip_*_decode_host: the device form into the workspace `ws_status`, the statuses down, wait
template <class Opts>
static inline int uwip_decode_to_host(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                                      const Opts *opts, int32_t *h_status,
                                      int (*decode)(uwip_ctx *, const uint8_t *const *, const size_t *, int, const uwip_batch_u8 *, const Opts *, int32_t *),
                                      const char *ws_status)
{
    if (int rc = uwip_enter(ctx)) return rc;
    UWIP_REQUIRE(ctx, n >= 0 && (h_status != nullptr || n == 0), "null status");
    if (n == 0) return UWIP_OK;
    int32_t *d_status = static_cast<int32_t *>(uwip_ws(ctx, ws_status, (size_t)n * sizeof(int32_t)));
    if (!d_status) return UWIP_ERR_NOMEM;
    int rc = decode(ctx, h_streams, h_sizes, n, out, opts, d_status);
    if (rc) return rc;
    UWIP_HIP(ctx, hipMemcpyAsync(h_status, d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    return UWIP_OK;
}

// uwip_*_encode_host: the device form into the workspaces `ws_streams` / `ws_sizes`, the sizes down, wait, one copy per positive
// size, wait
static inline int uwip_encode_to_host(uwip_ctx *ctx, const uwip_batch_u8 *frames, int param, uint8_t *h_streams, size_t slot_bytes,
                                      int64_t *h_sizes, int (*encode)(uwip_ctx *, const uwip_batch_u8 *, int, uint8_t *, size_t, int64_t *),
                                      const char *ws_streams, const char *ws_sizes)
{
    int rc = uwip_check_batch(ctx, frames, 0);
    if (rc) return rc;
    const int F = frames->frames;
    if (F == 0) return UWIP_OK;
    UWIP_REQUIRE(ctx, h_sizes != nullptr, "null sizes");
    UWIP_REQUIRE(ctx, h_streams != nullptr || slot_bytes == 0, "null streams");
    uint8_t *d_out = static_cast<uint8_t *>(uwip_ws(ctx, ws_streams, (size_t)F * slot_bytes + 16));
    int64_t *d_sizes = static_cast<int64_t *>(uwip_ws(ctx, ws_sizes, (size_t)F * sizeof(int64_t)));
    if (!d_out || !d_sizes) return UWIP_ERR_NOMEM;
    rc = encode(ctx, frames, param, d_out, slot_bytes, d_sizes);
    if (rc) return rc;
    UWIP_HIP(ctx, hipMemcpyAsync(h_sizes, d_sizes, (size_t)F * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    for (int f = 0; f < F; ++f)
        if (h_sizes[f] > 0)
            UWIP_HIP(ctx, hipMemcpyAsync(h_streams + (size_t)f * slot_bytes, d_out + (size_t)f * slot_bytes, (size_t)h_sizes[f],
                                         hipMemcpyDeviceToHost, ctx->stream));
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    return UWIP_OK;
}
