/*
 * uwip.h -- C ABI of the MI355X-native (gfx950) implementation of the
 * uwimageproc per-frame hot path:  bgdehaze -> histretch -> aclahe ->
 * videostrip-overlap.
 *
 * The reference has no FFI/plugin layer: its only seam is ordinary C++ calls
 * into modules/common/preprocessing.h and modules/videostrip/include/
 * videostrip.hpp, switched at compile time by USE_GPU and at run time by
 * -cuda=0/1 (modules/histretch/src/histretch.cpp:72,121-141).  The `...GPU`
 * twins there (imgChannelStretchGPU, calcOverlapGPU, calcBlurGPU) are the
 * precedent for an accelerator back end behind the same call sites; this
 * header is what such a back end binds to.  Every entry point cites the
 * reference interface it replaces.  INTEGRATION.md shows the reference-side
 * stubs.
 *
 * Conventions
 *   - plain C: opaque context, raw pointers, sizes; no C++/torch types.
 *   - every function returns an int status (UWIP_OK == 0); the message for
 *     the last failure is uwip_last_error(ctx).
 *   - images are batches of equally sized 8-bit frames in DEVICE memory,
 *     described by uwip_batch_u8, whose (data, step, rows, cols, channels)
 *     map field-for-field onto a cv::Mat of type CV_8UC1 / CV_8UC3
 *     (BGR interleaved, as cv::imread returns).  frames == 1 is one cv::Mat.
 *   - pointers named d_* are device pointers, h_* host pointers.
 *   - work is enqueued on the context's HIP stream and is asynchronous
 *     unless the function has a host-side result; uwip_sync() drains it.
 *   - there is NO CPU fallback: without a HIP device every compute entry
 *     point fails with UWIP_ERR_HIP.
 */
#ifndef UWIP_H
#define UWIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UWIP_OK               0
#define UWIP_ERR_INVALID      1   /* bad argument / shape */
#define UWIP_ERR_HIP          2   /* HIP runtime failure (incl. no device) */
#define UWIP_ERR_UNSUPPORTED  3   /* valid request outside the hot path */
#define UWIP_ERR_NOMEM        4

typedef struct uwip_ctx uwip_ctx;

/* One batch of frames in device memory (cv::Mat fields + batch extent). */
typedef struct uwip_batch_u8 {
    void   *data;          /* device pointer: frame 0, row 0 (cv::Mat::data) */
    size_t  step;          /* bytes between rows (cv::Mat::step)             */
    size_t  frame_stride;  /* bytes between consecutive frames               */
    int32_t rows, cols;    /* cv::Mat::rows / cols                           */
    int32_t channels;      /* 1 (CV_8UC1) or 3 (CV_8UC3, BGR)                */
    int32_t frames;        /* batch size (1 == a single cv::Mat)             */
} uwip_batch_u8;

/* ---- context, memory, profiling -------------------------------------- */

/* Replaces cuda::getCudaEnabledDeviceCount / cuda::setDevice(0)
 * (histretch.cpp:122-134, videostrip/src/main.cpp:188).  `stream` may be a
 * caller-owned hipStream_t (e.g. the framework's current stream) or NULL to
 * let the context create its own. */
int uwip_device_count(int *count);
int uwip_ctx_create(int device, void *stream, uwip_ctx **out);
/* Same with flags.  UWIP_CTX_STREAM_GIVEN: `stream` is used as it is even when
 * it is NULL -- the handle of the device's default ("null") stream is 0, which
 * uwip_ctx_create cannot tell from "no stream given"; a host framework whose
 * current stream is the default one (torch's is, until a side stream is made
 * current) passes this flag so that its own work and the library's stay in one
 * stream order.
 *
 * Threading: a uwip_ctx (and every uwip_features made from it) is
 * single-threaded -- one host thread at a time may be inside calls on it; the
 * library keeps no state outside contexts, so different contexts may be used
 * from different threads concurrently (one context per host thread / stream,
 * as bench.py does).  Every entry point makes the context's device current for
 * the calling thread (hipSetDevice) before it allocates, copies or launches. */
#define UWIP_CTX_STREAM_GIVEN 1u
/* Host waits.  Wherever the library waits on the host for its stream (uwip_sync, the ACLAHE parameter choice, staging
 * reuse, the copier's lanes) the calling thread polls an event with sleeps in between (20 ... 200 us) by default:
 * hipStreamSynchronize and hipEventSynchronize spin on this runtime -- also on hipEventBlockingSync events; only the
 * process-wide hipDeviceScheduleBlockingSync device flag makes them sleep, which is the host application's to set --
 * and a rank with eight sub-batch threads then burns eight cores doing nothing (measured: 1.59 CPU-seconds per 0.177 s
 * step), which a node's CPU quota does not have for eight ranks.  UWIP_CTX_SPIN_WAIT (or the environment variable
 * UWIP_SPIN_WAIT=1) keeps the spinning wait: up to 200 us less wake-up latency per wait for one core per waiting thread. */
#define UWIP_CTX_SPIN_WAIT 2u
int uwip_ctx_create_ex(int device, void *stream, unsigned flags, uwip_ctx **out);
int uwip_ctx_destroy(uwip_ctx *ctx);
const char *uwip_last_error(const uwip_ctx *ctx);
const char *uwip_version(void);
int uwip_sync(uwip_ctx *ctx);

/* Replaces GpuMat::upload / download (histretch.cpp:174-175,212-213). */
int uwip_malloc(uwip_ctx *ctx, size_t bytes, void **d_ptr);
int uwip_free(uwip_ctx *ctx, void *d_ptr);
int uwip_memcpy_h2d(uwip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int uwip_memcpy_d2h(uwip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* The same transfers enqueued on the context's stream without waiting
 * (GpuMat::upload / download with a cuda::Stream): the host buffer must be
 * page-locked -- take it from uwip_host_alloc (cuda::HostMem, PAGE_LOCKED) --
 * and stay untouched until uwip_sync().  This is the host-buffer front end of
 * the timed region of histretch.cpp:165-216 (upload ... download). */
int uwip_host_alloc(uwip_ctx *ctx, size_t bytes, void **h_ptr);
int uwip_host_free(uwip_ctx *ctx, void *h_ptr);
int uwip_memcpy_h2d_async(uwip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int uwip_memcpy_d2h_async(uwip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);

/* Copy engine for a stream of frame batches (the double-buffered form of
 * GpuMat::upload ... download around the timed region, histretch.cpp:165-216;
 * SURVEY.md section 7 "PCIe feed").  One per device / rank: an upload lane and a
 * download lane, each a host thread with a stream of its own that serves the
 * first queued request whose dependency has completed (requests that depend on
 * the same context are served in their order, and so are two requests of which
 * one writes bytes -- host or device -- the other reads or writes; one whose
 * stream is still busy does not hold back the ready requests of other
 * contexts).  A request with `after` != NULL starts once
 * everything queued on that context's stream AT THE TIME OF THE CALL has
 * finished (the lane waits for it on the host, so a copy is only handed to the
 * DMA engine when it can run: no hardware queue ever holds a barrier packet
 * that waits for a copy or for another stream -- with more streams than the
 * runtime has hardware queues such packets stall unrelated kernels).  A ticket
 * names the request: uwip_copier_wait blocks the calling host thread until
 * that copy has completed (ticket 0: returns at once), after which the host
 * buffer may be reused (upload) or read (download), and the device buffer may
 * be read by kernels queued from then on.  Requests may come from any thread.
 * uwip_copier_create leaves the caller's current HIP device as it found it.
 * Failure is sticky: after the first HIP error in a lane every later submit /
 * wait / query returns UWIP_ERR_HIP (uwip_copier_last_error says what failed;
 * queued requests are completed without copying so that no waiter blocks) and
 * the copier must be destroyed and created anew -- there is no reset. */
typedef struct uwip_copier uwip_copier;
int uwip_copier_create(int device, uwip_copier **out);
int uwip_copier_destroy(uwip_copier *c);                 /* drains both lanes first */
int uwip_copier_upload(uwip_copier *c, uwip_ctx *after, void *d_dst, const void *h_src, size_t bytes, uint64_t *ticket);
int uwip_copier_download(uwip_copier *c, uwip_ctx *after, void *h_dst, const void *d_src, size_t bytes, uint64_t *ticket);
int uwip_copier_wait(uwip_copier *c, uint64_t ticket);
int uwip_copier_query(uwip_copier *c, uint64_t ticket, int *done);
const char *uwip_copier_last_error(const uwip_copier *c);

/* Per-kernel hipEvent timing on the context's stream (replaces the
 * getTickCount stopwatch, histretch.cpp:165,257-261).  Enabling it brackets
 * every kernel launch with events; totals are read back per kernel name. */
int uwip_prof_enable(uwip_ctx *ctx, int on);
int uwip_prof_reset(uwip_ctx *ctx);
int uwip_prof_count(uwip_ctx *ctx, int *n);
int uwip_prof_get(uwip_ctx *ctx, int index, char *name, size_t name_cap,
                  double *total_ms, uint64_t *launches);

/* ---- histretch (H1-H4) ------------------------------------------------- */

/* numChannel / numSpace, preprocessing.cpp:147-161 (host, pure). */
int uwip_numChannel(char c);
int uwip_numSpace(char c);

/* getHistogram, preprocessing.cpp:25-34 (cv::calcHist, 256 bins), for every
 * frame and channel of the batch in one pass.  d_hist: [frames][channels][256]
 * uint32 counts (the reference stores the same counts as CV_32F). */
int uwip_getHistogram(uwip_ctx *ctx, const uwip_batch_u8 *img, uint32_t *d_hist);

/* Percentile search + stretch LUT, preprocessing.cpp:82-100, for `nplanes`
 * histograms of rows*cols-pixel planes.  d_lut: [nplanes][256] bytes;
 * d_bounds (may be NULL): [nplanes][2] int32 = (lower, higher) bins. */
int uwip_stretch_lut(uwip_ctx *ctx, const uint32_t *d_hist, int nplanes, int rows, int cols,
                     int lo, int hi, uint8_t *d_lut, int32_t *d_bounds);

/* In-place LUT application (the fused `img += b; img *= m`,
 * preprocessing.cpp:99-100).  d_lut: [frames][channels][256]. */
int uwip_apply_lut(uwip_ctx *ctx, const uwip_batch_u8 *img, const uint8_t *d_lut);

/* imgChannelStretch(Mat, Mat, lo, hi), preprocessing.cpp:74-105, on lane
 * `channel` of every frame, in place (the reference passes the same Mat as
 * input and output). */
int uwip_imgChannelStretch(uwip_ctx *ctx, const uwip_batch_u8 *img, int channel, int lo, int hi);

/* The per-letter loop of histretch.cpp:217-254 on BGR frames, in place:
 * for each letter in order, stretch plane numChannel(letter).  Unknown
 * letters are skipped as the reference does.  Letters of the other colour
 * spaces -- HSV ('H','S','V'), HLS ('h','s','l'), Lab ('L','a','b'), YCrCb
 * ('Y','C','X') -- do what the reference's code does with them (SURVEY.md
 * B-3): the stretch lands in a split copy and the image receives the 8-bit
 * colour round trip cvtColor(BGR2xxx) -> cvtColor(xxx2BGR), applied in letter
 * order between the BGR letters' stretches.
 * uwip_histretch_ex with UWIP_HISTRETCH_FIXED_ORDER runs the evident intent
 * instead: convert (histretch.cpp:232), split / stretch / MERGE (:234-236,
 * :240), then convert back (:238) -- the stretch is kept.
 * The 8-bit conversions restate OpenCV 3.x's color.cpp (parity unpinned).  Lab -> BGR exists in two forms there: OpenCV
 * 3.4.x (the version INSTALL.md:47-63 pins) converts 8-bit Lab with the integer Lab2RGBinteger, OpenCV 3.2 (the version the
 * module READMEs name) with the float Lab2RGB_f + inverse-gamma spline.  Default = 3.4.x, as for CLAHE's residual rule and
 * the 3 x 3 blur's rounding; UWIP_HISTRETCH_OPENCV32 / opencv_rule = 1 selects the 3.2 form. */
#define UWIP_HISTRETCH_FIXED_ORDER 1u
#define UWIP_HISTRETCH_OPENCV32    2u
int uwip_histretch_ex(uwip_ctx *ctx, const uwip_batch_u8 *img, const char *letters, int lo, int hi,
                      unsigned flags);
/* cv::cvtColor(src, dst, COLOR_BGR2{HSV,HLS,Lab,YCrCb}) (to_bgr = 0) or COLOR_{..}2BGR (to_bgr = 1) on 8UC3 batches;
 * space = uwip_numSpace's index 1..4 (histretch.cpp:155-156).  dst may alias src. */
int uwip_cvtColor(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, int space, int to_bgr);
/* opencv_rule: 0 = OpenCV 3.4.x, 1 = OpenCV 3.2 (only COLOR_Lab2BGR differs). */
int uwip_cvtColor_ex(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, int space, int to_bgr, int opencv_rule);
int uwip_histretch(uwip_ctx *ctx, const uwip_batch_u8 *img, const char *letters, int lo, int hi);

/* ---- aclahe (C1-C4) ----------------------------------------------------- */

/* V plane of cvtColor(BGR2HSV)+split, aclahe.cpp:152-154 (V = max(B,G,R)). */
int uwip_bgr_to_v(uwip_ctx *ctx, const uwip_batch_u8 *bgr, const uwip_batch_u8 *v);

/* cv::CLAHE::{setClipLimit,setTilesGridSize,apply}, aclahe.cpp:184-187, on
 * 8UC1 planes.  residual_rule: 0 = OpenCV 3.4.x, 1 = OpenCV 3.2. */
int uwip_clahe(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst,
               double clipLimit, int gx, int gy, int residual_rule);
/* Same with per-frame parameters (host arrays of length src->frames), the
 * "for resulting CL/BS, apply classic clahe" step of aclahe.cpp:215. */
int uwip_clahe_per_frame(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst,
                         const double *h_clipLimit, const int32_t *h_grid, int residual_rule);
/* Tile LUT stage tap for parity tests: d_luts [frames][gy*gx][256]. */
int uwip_clahe_luts(uwip_ctx *ctx, const uwip_batch_u8 *src, double clipLimit, int gx, int gy,
                    int residual_rule, uint8_t *d_luts);

/* aclaheEntropy, aclahe.cpp:228-248: d_entropy [frames] float. */
int uwip_entropy(uwip_ctx *ctx, const uwip_batch_u8 *src, float *d_entropy);

/* The sweep of aclahe.cpp:160-193: grid in {2,4,8,16,32} x clip limit in
 * {0,0.5,...,25}; d_entropy: [frames][5][51] float (clean table). */
int uwip_aclahe_sweep(uwip_ctx *ctx, const uwip_batch_u8 *src, int residual_rule,
                      float *d_entropy);
/* The same with a tap (may be NULL): d_hist [frames][5][51][256] uint32, the histogram of the CLAHE output of every
 * (grid, clip limit) -- what calcHist sees at aclahe.cpp:236 -- for exact parity checks of the sweep. */
int uwip_aclahe_sweep_hist(uwip_ctx *ctx, const uwip_batch_u8 *src, int residual_rule,
                           float *d_entropy, uint32_t *d_hist);

/* Parameter choice of modules/aclahe/python/ACLAHE.py:66-129 (host, pure; the
 * reference does it with scipy, functions.py:49-93; the C++ module stops at
 * comment stubs, aclahe.cpp:209-218).
 * uwip_aclahe_knee: DerivadaY + DerivadaX + Curvatura on one 49-sample curve
 *   (h_xs49 = clip limits 0.5..24.5, h_ys49 = entropies) -> arg-max index, or
 *   -1 where scipy's curve_fit would raise.
 * uwip_aclahe_select: h_entropy [frames][5][51] (the sweep table) -> per frame
 *   h_bs (block size) and h_cl (clip limit = the largest of the five knee
 *   indices, used as a clip limit as the reference does); h_knee (may be NULL)
 *   [frames][5].  When 2*CL lies outside the swept grid the BS choice falls
 *   back to the last swept clip limit; uwip_aclahe_auto evaluates it exactly
 *   (on the device, whichever form made the choice). */
int uwip_aclahe_knee(const float *h_xs49, const float *h_ys49, int32_t *index);
/* The same choice made ON THE DEVICE, from the table the sweep leaves in HBM (no copy to the host, no host computation):
 * one wavefront per (frame, block size) runs the knee stage -- the same source as uwip_aclahe_select
 * (csrc/lm_core.hpp), the 49 samples of a curve on 49 lanes, MINPACK's summation order kept, so host and device agree
 * bit for bit -- and one thread per frame the choice of ACLAHE.py:92-125.
 *   d_entropy  device, [frames][5][51] (uwip_aclahe_sweep's output)
 *   d_par      device, [frames][4] int32 = {BS, CL, need_eval, 0}; need_eval = 1 when 2 * CL lies outside the swept grid
 *              (BS then comes from the last swept clip limit; uwip_aclahe_auto_ex evaluates such frames exactly, in every
 *              form by the same device kernel, k_aclahe_exact_bs)
 *   d_knee     device, [frames][5] int32, may be NULL: the five knee indices (-1 where curve_fit would raise) */
int uwip_aclahe_select_device(uwip_ctx *ctx, const float *d_entropy, int frames, int32_t *d_par, int32_t *d_knee);
/* The persistent host pool uwip_aclahe_select spreads its frames over (one per process, created on first use):
 * its size is the CPU budget of this rank minus the calling thread, at most 16 -- budget = min(CPUs in the affinity
 * mask, cgroup CPU quota) / ranks on the node (UWIP_RANKS_ON_NODE, else the launcher's LOCAL_WORLD_SIZE, else 1);
 * UWIP_HOST_THREADS overrides the size.  Any argument may be NULL. */
int uwip_host_pool_info(int *workers, double *cpu_budget, int *ranks_on_node);
int uwip_aclahe_select(const float *h_entropy, int frames, int32_t *h_bs, int32_t *h_cl,
                       int32_t *h_knee);

/* The whole aclahe stage on 8UC1 planes: sweep (aclahe.cpp:160-193), parameter
 * choice (ACLAHE.py:66-129) and the final createCLAHE(CL,(BS,BS)).apply
 * (python/main.py:19-20).  h_bs / h_cl (may be NULL): the chosen parameters.
 * Synchronises the stream once (the choice is a host decision). */
int uwip_aclahe_auto(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst,
                     int residual_rule, int32_t *h_bs, int32_t *h_cl);
/* The (BS, CL) the most recent uwip_aclahe_auto / uwip_aclahe_auto_ex on this context chose, h_bs / h_cl [frames] (frames =
 * that call's frame count).  After a UWIP_ACLAHE_ASYNC call this waits for the stream and copies them from the device. */
int uwip_aclahe_last_params(uwip_ctx *ctx, int32_t *h_bs, int32_t *h_cl, int frames);
/* cv2.GaussianBlur(img, (3,3), 0) on 8UC1 planes, ACLAHE.py:15 (fixed [1 2 1]/4 kernel, BORDER_REFLECT_101; rounding of
 * the /16: rule 0 = half up, OpenCV 3.4.x's 8-bit fixed-point path; rule 1 = half to even, OpenCV 3.2's float path).
 * Not in place. */
int uwip_GaussianBlur3(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, int rounding_rule);
/* The two forms of the aclahe stage the reference holds:
 *   flags = 0                      the C++ driver, modules/aclahe/src/aclahe.cpp:152-187: the sweep runs on the plane itself
 *                                  (= uwip_aclahe_auto);
 *   flags = UWIP_ACLAHE_PREFILTER  ParametrosACLAHE, modules/aclahe/python/ACLAHE.py:9-129: the sweep (:40-47) and the
 *                                  block-size search (:102-112) run on GaussianBlur(img,(3,3),0) (:15), the final
 *                                  createCLAHE(CL,(BS,BS)).apply on the unfiltered image (python/main.py:19-20). */
#define UWIP_ACLAHE_PREFILTER 1u
/*   UWIP_ACLAHE_HOST_SELECT        the parameter choice by uwip_aclahe_select on the host (the sweep table is copied to
 *                                  page-locked memory, the host pool fits the curves) instead of uwip_aclahe_select_device,
 *                                  which is the default for batches of more than 4 frames (smaller ones take the host form
 *                                  for its latency: 0.15 ms per curve on a core against 1.3 ms on one wavefront); same
 *                                  parameters -- the two forms agree bit for bit.  Environment UWIP_ACLAHE_SELECT=host |
 *                                  device forces one form process-wide. */
#define UWIP_ACLAHE_HOST_SELECT 2u
/*   UWIP_ACLAHE_ASYNC              nothing comes back to the host and the call does not wait: the choice is made on the device,
 *                                  the exact block-size search is queued behind it unconditionally (blocks of frames whose
 *                                  clip limit stays in the swept grid exit), and the final per-frame CLAHE is launched from
 *                                  the device-side parameters (the kernels of all five grids are launched over the batch,
 *                                  blocks of frames that chose another grid exit).  h_bs / h_cl must be NULL;
 *                                  uwip_aclahe_last_params fetches the parameters later (it waits for the stream).  Same
 *                                  image, same parameters as the other forms.  Batches the library gives to the host form
 *                                  (<= 4 frames, UWIP_ACLAHE_SELECT=host) run synchronously under this flag too.
 * In every form a frame whose clip limit leaves the swept grid gets its exact block-size search from the same device kernel;
 * the synchronous forms launch it (and wait for it once more) only when some frame of the batch needs it. */
#define UWIP_ACLAHE_ASYNC 4u
int uwip_aclahe_auto_ex(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst,
                        int residual_rule, unsigned flags, int32_t *h_bs, int32_t *h_cl);

/* "transform back image" (aclahe.cpp:216 stub): cvtColor(BGR2HSV), replace V by
 * v_new (the CLAHE'd plane), cvtColor(HSV2BGR), all 8-bit.  bgr_out may alias bgr. */
int uwip_hsv_replace_v(uwip_ctx *ctx, const uwip_batch_u8 *bgr, const uwip_batch_u8 *v_new,
                       const uwip_batch_u8 *bgr_out);

/* ---- bgdehaze (D1-D6) ---------------------------------------------------- */
/* All real-valued results are float64, as in the reference.  The input is the
 * uint8 BGR frame cv2.imread returns; normI = (I - min)/(max - min)
 * (modules/bgdehaze/main.py:17) is formed inside. */

/* Background_light(normI, w), BGDehaze.py:14-26.  d_B: [frames][3] (BGR);
 * d_idx (may be NULL): [frames][2] row-major pixel indices of the two minima.
 * Ties take the first index (the reference's order is unspecified, B-9). */
int uwip_dehaze_background_light(uwip_ctx *ctx, const uwip_batch_u8 *in, int w, double *d_B,
                                 int32_t *d_idx);

/* transmission_map(normI, 15) with B injected, BGDehaze.py:28-37.
 * d_B: [frames][3]; d_t: [frames][2][rows][cols] (blue, green), before the
 * 0.2 clamp. */
int uwip_dehaze_transmission(uwip_ctx *ctx, const uwip_batch_u8 *in, const double *d_B, double *d_t);

/* guided_filter(I, p, r, eps), guidedfilter.py:54-103, for the guide form both
 * call sites use: an 8-bit 3-channel image normalised by its global min/max.
 * d_p, d_q: [frames][rows][cols].  Needs rows, cols >= 2r+1. */
int uwip_guided_filter(uwip_ctx *ctx, const uwip_batch_u8 *guide, const double *d_p, int r, double eps,
                       double *d_q);

/* generate_results(), modules/bgdehaze/main.py:14-20: uint8 BGR in -> uint8
 * BGR out.  flags: UWIP_DEHAZE_FULL runs adaptiveExp_map (BGDehaze.py:71-89),
 * without it the chain stops after RC_correction (:59-69).  As written, a 0/0
 * in the exposure map S (:83) turns the whole frame into NaN -> black
 * (SURVEY.md B-11); that is reproduced unless UWIP_DEHAZE_GUARD_S is set, which
 * substitutes S = 1 there (a documented deviation).
 * `out` may be NULL when only taps are wanted.
 * Optional taps / injection (device pointers, may be NULL):
 *   d_B_inject   [frames][3]              use this background light (parity tests)
 *   d_refined_t  [frames][2][rows][cols]  refined_t (:39-48)
 *   d_float_out  [frames][rows][cols][3]  the float64 image before *255 */
#define UWIP_DEHAZE_FULL     1
#define UWIP_DEHAZE_GUARD_S  2
int uwip_dehaze(uwip_ctx *ctx, const uwip_batch_u8 *in, const uwip_batch_u8 *out, int w, int flags,
                const double *d_B_inject, double *d_refined_t, double *d_float_out);

/* bgdehaze -> histretch chained on one batch (BASELINE.json configs[2]; the reference runs the two tools back to back
 * over files: modules/bgdehaze/main.py:14-20, then modules/histretch/src/histretch.cpp:218-254 on its output).  Same
 * result as uwip_dehaze(in, out, ...) followed by uwip_histretch_ex(out, ...); with UWIP_DEHAZE_FULL the kernel
 * that writes the dehazed bytes also counts them, so the stretch starts from a finished histogram instead of
 * reading the image once more. */
int uwip_dehaze_histretch(uwip_ctx *ctx, const uwip_batch_u8 *in, const uwip_batch_u8 *out, int w, int dehaze_flags,
                          const char *letters, int lo, int hi, unsigned histretch_flags);

/* ---- videostrip overlap (V1-V5) -------------------------------------------- */
/* calcOverlap(keyframe*, Mat), modules/videostrip/src/videostrip.cpp:192-289, split
 * at the point where the reference caches a key frame's keypoints/descriptors in
 * `struct keyframe` (videostrip.hpp:62-68; kframe->new_img, :209-213):
 *   uwip_overlap_detect   resize to 640 wide (main.cpp:242,311) + BGR2GRAY + detect + describe
 *                         for a batch of frames, into slots of an opaque feature set;
 *   uwip_overlap_match    kNN(2) match (:229-231), ratio test (:233-242), homography (:270),
 *                         overlapArea (:280) for a list of (object slot, key slot) pairs.
 * The detector/descriptor/matcher are the AKAZE-style / M-LDB / Hamming design that
 * BASELINE.json's north_star names in place of the reference's OpenCV-contrib SURF +
 * L2 matcher (DESIGN.md "overlap stage"); the dense distance matrix runs on i8 MFMA. */
typedef struct uwip_features uwip_features;

/* At most this many keypoints per frame.  A frame with more candidates keeps the FIRST UWIP_MAX_KEYPOINTS, in (level, y, x)
 * raster order, of the candidates whose response is >= the UWIP_MAX_KEYPOINTS-th largest response.  Without ties at that
 * threshold these are the strongest; with ties the cutoff falls in raster order, and a candidate late in that order is
 * dropped even where it is strictly stronger than the threshold (DESIGN.md "overlap stage"). */
#define UWIP_MAX_KEYPOINTS 2048
/* keypoint record returned by uwip_features_download (32 bytes) */
typedef struct uwip_keypoint {
    float   x, y;        /* sub-pixel position in the 640-wide working image */
    float   response;    /* scale-normalised determinant of the Hessian */
    int32_t level;       /* evolution level 0..3 */
    int32_t xi, yi;      /* integer extremum position */
    float   co, si;      /* unit vector of the dominant orientation ((1, 0) with UWIP_OVERLAP_UPRIGHT) */
} uwip_keypoint;

int uwip_features_create(uwip_ctx *ctx, int max_frames, uwip_features **out);
int uwip_features_destroy(uwip_features *feats);
/* copy one slot's cached keypoints/descriptors (kframe->keypoints/descriptors) to another slot */
int uwip_features_copy(uwip_ctx *ctx, const uwip_features *src, int src_slot, uwip_features *dst,
                       int dst_slot);
/* working size for a rows x cols frame: cv::resize(frame, Size(), f, f), f = 640/cols */
int uwip_overlap_working_size(int rows, int cols, int *orows, int *ocols);
/* cv::resize(frame, res_frame, Size(), f, f) by itself (main.cpp:242,287,311; INTER_LINEAR, 8UC3 fixed point): the frame
 * the reference hands to calcBlur (main.cpp:338,355).  dst: rows x cols of uwip_overlap_working_size. */
int uwip_resize_bgr(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst);
/* frames: full-resolution CV_8UC3 BGR (resized inside) or CV_8UC1 planes already at the
 * working size.  Fills slots [first_slot, first_slot + frames->frames). */
int uwip_overlap_detect(uwip_ctx *ctx, const uwip_batch_u8 *frames, uwip_features *feats, int first_slot);
/* Same with flags.  By default keypoints carry a dominant orientation and the descriptor is sampled in the keypoint's own
 * frame, as the reference's SURF::create(400) is oriented (upright = false, videostrip.cpp:206-208): the overlap ratio
 * holds under any in-plane rotation of the camera.  UWIP_OVERLAP_UPRIGHT skips the orientation estimate (SURF's
 * `upright` parameter): rotation tolerance then ends near 20 degrees. */
#define UWIP_OVERLAP_UPRIGHT 1u
/* The detector threshold is FIXED by default (1e-3 on the scale-normalised determinant of the Hessian), as SURF's
 * hessianThreshold is in the reference (SURF::create(400), videostrip.cpp:200,206).  UWIP_OVERLAP_RELATIVE_THRESHOLD (opt-in, a
 * DEVIATION): the threshold follows the frame's own contrast, 1e-3 * min(1, (k / 0.5)^2), k = the frame's contrast factor
 * (70th percentile of the gradient magnitude).  The response scales with the square of the contrast, and raw frames of
 * turbid water -- what the reference's videostrip is run on -- have none above a fixed threshold (the reference's own
 * photograph PIS_T1A_259: no keypoint at all at 1e-3, so calcOverlap answers -2.0 whatever the motion; 130 keypoints with
 * the relative one).  It also finds a few dozen "keypoints" in pure sensor noise: combine it with UWIP_OVERLAP_MIN6.
 * (Rounds 3-4 had the relative threshold as the default; UWIP_OVERLAP_FIXED_THRESHOLD is still accepted and names the
 * default.) */
#define UWIP_OVERLAP_FIXED_THRESHOLD 2u
#define UWIP_OVERLAP_RELATIVE_THRESHOLD 16u
int uwip_overlap_detect_ex(uwip_ctx *ctx, const uwip_batch_u8 *frames, uwip_features *feats, int first_slot, unsigned flags);
/* parity taps: one slot's keypoints (uwip_keypoint[2048]) / packed 64-byte descriptors; and the
 * scale-space images of frame `frame` of the most recent uwip_overlap_detect call (host buffers
 * of rows*cols floats, any may be NULL). */
int uwip_features_download(uwip_ctx *ctx, const uwip_features *feats, int slot, void *h_kps,
                           uint8_t *h_desc, int32_t *h_count);
/* the opposite direction: fill one slot from host keypoints (uwip_keypoint[count]) and packed
 * descriptors ([count][64]); the reference's `struct keyframe` members are public and caller-fillable
 * (videostrip.hpp:62-68).  rows/cols: the working size the keypoints refer to. */
int uwip_features_upload(uwip_ctx *ctx, uwip_features *feats, int slot, int rows, int cols,
                         const void *h_kps, const uint8_t *h_desc, int32_t count);
int uwip_overlap_debug_level(uwip_ctx *ctx, int frame, int level, int rows, int cols, float *h_Lt,
                             float *h_Lx, float *h_Ly, float *h_Ldet, float *h_kcontrast);
/* h_pair_q / h_pair_t: host arrays of slot indices (query = object frame in fq, train = key
 * frame in ft).  d_ratio [npairs]: the overlap ratio, or -2.0 when fewer than 4 good matches
 * survive or no homography is found (videostrip.cpp:252-256,272).  videoWidth / videoHeight
 * are the reference's globals (main.cpp:238-239).  Optional device outputs:
 * d_info [npairs][8] = {nkp_obj, nkp_key, ngood, ninliers, overlap pixels, 0,0,0};
 * d_H [npairs][9]; d_match_idx / d_match_dist [npairs][2048][2] (the kNN(2) result). */
int uwip_overlap_match(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft,
                       const int32_t *h_pair_q, const int32_t *h_pair_t, int npairs, int videoWidth,
                       int videoHeight, uint32_t seed, float *d_ratio, int32_t *d_info, double *d_H,
                       int32_t *d_match_idx, int32_t *d_match_dist);
/* Same with flags.  The default is the reference's rule (videostrip.cpp:252-256,270-272): -2.0 only when fewer than 4 good
 * matches survive the ratio test or no homography is found; whatever findHomography returns for >= 4 good matches is
 * used -- i.e. any hypothesis with >= 4 inliers (any solvable sample of four good matches) yields an overlap value.
 * UWIP_OVERLAP_MIN6 (opt-in, a DEVIATION from the reference): a homography supported by fewer than 6 RANSAC inliers is
 * reported as none (-2.0) -- four matches always fit one exactly, and with the contrast-relative detector threshold two
 * frames of pure sensor noise now and then produce four chance matches.  (Rounds 3-4 had the two the other way round:
 * UWIP_OVERLAP_MIN4 is still accepted and now names the default.) */
#define UWIP_OVERLAP_MIN4 4u
#define UWIP_OVERLAP_MIN6 8u
int uwip_overlap_match_ex(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft,
                          const int32_t *h_pair_q, const int32_t *h_pair_t, int npairs, int videoWidth,
                          int videoHeight, uint32_t seed, unsigned flags, float *d_ratio, int32_t *d_info,
                          double *d_H, int32_t *d_match_idx, int32_t *d_match_dist);
/* overlapArea(Mat H), videostrip.cpp:291-319, for n row-major 3x3 double homographies. */
int uwip_overlapArea(uwip_ctx *ctx, const double *d_H, int n, int videoWidth, int videoHeight,
                     float *d_ratio, int32_t *d_count);
/* calcBlur(Mat frame), videostrip.cpp:170-184, on BGR frames (the reference passes the
 * resized frame, main.cpp:338,355): d_blur [frames]. */
int uwip_calcBlur(uwip_ctx *ctx, const uwip_batch_u8 *frames, float *d_blur);

/* ---- the whole per-frame chain ----------------------------------------------------------------------------- */
/* bgdehaze -> histretch -> aclahe -> videostrip-overlap on batches of frames, as ONE object: what the reference runs as
 * four tools back to back over files -- modules/bgdehaze/main.py:14-20, modules/histretch/src/histretch.cpp:217-254,
 * modules/aclahe/src/aclahe.cpp:152-218 (+ python/ACLAHE.py:9-129, python/main.py:19-20), modules/videostrip/src/
 * main.cpp:300-394 (calcOverlap of every frame against its predecessor, videostrip.cpp:192-289).  A pipe owns what the
 * chain carries from step to step: the V planes, the feature slots (slot 0 = the previous batch's last frame, i.e. the
 * `struct keyframe` cache of videostrip.hpp:62-68 carried across batches), the pair list, a throttle (at most
 * `max_in_flight` steps queued on the stream: nothing in a step waits on the host, so an unthrottled caller would queue
 * without bound), and -- for the host-buffer form -- two source and two result buffers in device memory with their copy
 * tickets (GpuMat::upload ... download around the timed region, histretch.cpp:165-216, double-buffered).
 * Stage definitions: dehaze = uwip_dehaze(w, dehaze_flags); histretch = uwip_histretch_ex(letters, lo, hi,
 * histretch_flags) (the two chained through uwip_dehaze_histretch when both run); aclahe = uwip_bgr_to_v +
 * uwip_aclahe_auto_ex(residual_rule, aclahe_flags) + uwip_hsv_replace_v; overlap = uwip_overlap_detect_ex(detect_flags)
 * + uwip_overlap_match_ex(videoWidth, videoHeight, seed, match_flags) of frame i against frame i - 1 (frame 0 against the
 * previous batch's last frame; in the very first batch against itself, main.cpp:284-297 takes the first frame as key frame).
 * uwip_pipe_config_default fills in the REFERENCE's rules: letters "RGB", 2 / 98 percent, w = 15, UWIP_DEHAZE_FULL (S
 * unguarded, BGDehaze.py:83), UWIP_ACLAHE_PREFILTER | UWIP_ACLAHE_ASYNC, OpenCV 3.4.x rounding, >= 4 good matches
 * (videostrip.cpp:252-272), videoWidth x videoHeight = cols x rows (main.cpp:238-239), seed 1, two steps in flight.
 * A pipe is bound to the context it was made from (its stream, its thread rule); destroy it before the context. */
typedef struct uwip_pipe uwip_pipe;
typedef struct uwip_pipe_config {
    int32_t  frames, rows, cols;       /* batch geometry of every step: `frames` CV_8UC3 BGR frames of rows x cols */
    char     letters[16];              /* histretch -c letters, NUL-terminated */
    int32_t  lo, hi;                   /* histretch percentiles */
    int32_t  w;                        /* bgdehaze window */
    uint32_t dehaze_flags;             /* UWIP_DEHAZE_* */
    uint32_t histretch_flags;          /* UWIP_HISTRETCH_* */
    int32_t  residual_rule;            /* 0 = OpenCV 3.4.x, 1 = OpenCV 3.2 (CLAHE redistribution, 3x3 blur rounding) */
    uint32_t aclahe_flags;             /* UWIP_ACLAHE_* */
    uint32_t detect_flags;             /* UWIP_OVERLAP_UPRIGHT | UWIP_OVERLAP_RELATIVE_THRESHOLD */
    uint32_t match_flags;              /* UWIP_OVERLAP_MIN6 */
    int32_t  videoWidth, videoHeight;  /* the reference's globals; 0 = cols / rows */
    uint32_t seed;                     /* RANSAC seed */
    int32_t  max_in_flight;            /* steps queued before uwip_pipe_step waits for the oldest (>= 1) */
    void    *d_staging;                /* host-buffer form: caller-owned device memory of uwip_pipe_staging_bytes() bytes,
                                          or NULL = the pipe allocates it at the first uwip_pipe_step_host.  Layout:
                                          src[2][frames][rows][cols][3] u8, work[2][...] u8, ratio[2][frames] f32 (256-byte
                                          aligned), info[2][frames][8] i32 */
} uwip_pipe_config;
int uwip_pipe_config_default(uwip_pipe_config *cfg, int frames, int rows, int cols);
size_t uwip_pipe_staging_bytes(const uwip_pipe_config *cfg);
/* copier: the copy engine the host-buffer form uses (shared by all pipes of a rank), or NULL = the pipe makes its own at
 * the first uwip_pipe_step_host. */
int uwip_pipe_create(uwip_ctx *ctx, const uwip_pipe_config *cfg, uwip_copier *copier, uwip_pipe **out);
int uwip_pipe_destroy(uwip_pipe *p);          /* drains the stream and the pipe's outstanding copies first */
const char *uwip_pipe_last_error(const uwip_pipe *p);
/* One step on frames resident in device memory: in -> out (distinct buffers of the configured geometry), d_ratio [frames]
 * f32 = the overlap ratio of every frame against its predecessor (-2.0 / the value, videostrip.cpp:252-289), d_info (may
 * be NULL) [frames][8] as uwip_overlap_match.  Asynchronous: returns when the step is queued (after waiting, if need be,
 * until fewer than max_in_flight earlier steps are unfinished); uwip_pipe_sync drains. */
int uwip_pipe_step(uwip_pipe *p, const uwip_batch_u8 *in, const uwip_batch_u8 *out, float *d_ratio, int32_t *d_info);
/* The same, stage by stage (parity tests tap the chain between stages; a tool runs a part of it): `stages` is a mask of
 * UWIP_PIPE_*.  Without UWIP_PIPE_DEHAZE `in` is ignored (may be NULL) and `out` is processed in place; d_ratio / d_info
 * are used by UWIP_PIPE_OVERLAP only.  Not throttled. */
#define UWIP_PIPE_DEHAZE    1u
#define UWIP_PIPE_HISTRETCH 2u
#define UWIP_PIPE_ACLAHE    4u
#define UWIP_PIPE_OVERLAP   8u
#define UWIP_PIPE_ALL       15u
int uwip_pipe_stages(uwip_pipe *p, unsigned stages, const uwip_batch_u8 *in, const uwip_batch_u8 *out, float *d_ratio,
                     int32_t *d_info);
/* One step from / to page-locked host memory (uwip_host_alloc): h_in -> upload -> the four stages -> download -> h_out
 * (frames) and, when h_ratio != NULL, h_ratio [frames] f32.  h_prefetch (may be NULL) is the NEXT step's h_in: its upload
 * is requested now and runs under this step's kernels.  Returns without waiting for the device; tickets[0] = the upload of
 * h_in (h_in may be refilled once it is complete), tickets[1] = the download of the frames (they leave as soon as the
 * aclahe stage is done, under the overlap kernels), tickets[2] = the download of the ratios (0 when h_ratio is NULL):
 * uwip_pipe_wait blocks the calling thread until that copy is complete.  The call itself waits (on the host, sleeping) for
 * the upload of h_in and for the download of the step before last, whose device buffer it reuses. */
int uwip_pipe_step_host(uwip_pipe *p, const void *h_in, void *h_out, float *h_ratio, const void *h_prefetch,
                        uint64_t tickets[3]);
int uwip_pipe_wait(uwip_pipe *p, uint64_t ticket);
int uwip_pipe_sync(uwip_pipe *p);             /* the stream and every outstanding copy of this pipe */
/* Forget the carried key frame: the next step's frame 0 is its own key frame again (a new video). */
int uwip_pipe_reset(uwip_pipe *p);
/* (BS, CL) the aclahe stage of the most recent step chose, h_bs / h_cl [frames] (waits for the stream). */
int uwip_pipe_last_params(uwip_pipe *p, int32_t *h_bs, int32_t *h_cl);
/* Device pointers of the most recent step's results, for callers that chain further device work: the V planes the
 * aclahe stage left ([frames][rows][cols] u8, the unfiltered V of the stretched frames), and -- host-buffer form -- the
 * frames / ratios / info of that step inside the staging area.  Any argument may be NULL. */
int uwip_pipe_device_results(uwip_pipe *p, const uint8_t **d_v, const uint8_t **d_frames, const float **d_ratio,
                             const int32_t **d_info);

/* ---- key-frame mode: videostrip's selector on the enhanced frames ---------------------------------------------------
 * Opt-in per pipe (uwip_pipe_keyframe_chain); without it the overlap stage compares every frame with its predecessor, as
 * above.  In key-frame mode the overlap stage runs main.cpp:284-394 over the stream of frames it is given, across steps:
 * stream frame 0 is the first key frame (row (0, 0, 0.0, 0.0)); every later frame outside a refinement window gets
 * calcOverlap(key, frame); -2.0 counts as OVERLAP_MIN + 0.01 = 0.41 (:321-329); a result <= minOverlap opens a window: the
 * trigger and the next kWindow frames are candidates by calcBlur(resize(frame)) alone, a later one replaces the best only
 * when its blur is strictly greater, and the best becomes the new key frame (:335-381).  "Frame" keeps the reference's
 * numbering: a trigger that stays best reports its 0-based stream index (:340), a window frame the 1-based count of frames
 * read (:364).  When the stream ends inside a window the row is written with the best candidate so far.
 * Every decision is made on the device, behind the matcher: the step never waits on the host (key-frame mode).
 * d_ratio[i] is frame i's raw calcOverlap against the key it was compared with (-2.0: no homography; NaN: not compared --
 * a window frame, stream frame 0, a frame past `valid`); d_info[i][0..4] as uwip_overlap_match for that pair, d_info[i][5]
 * the key's stream index (-1: not compared).  The host form's h_ratio follows the same rule. */
typedef struct uwip_keyframe_config {
    float   minOverlap;   /* -p, default 0.4 (videostrip.hpp:50) */
    int32_t kWindow;      /* -k, default 11 (videostrip.hpp:51); 0 = no refinement */
    int32_t lookback;     /* D >= 1: frames i - 1..i - D of the batch are matched against frame i ahead of the decisions;
                             a pure performance knob, the results are identical for every D */
    int32_t max_rows;     /* capacity of the pipe's row ring (>= 1), default 4096 */
} uwip_keyframe_config;
typedef struct uwip_keyframe_row {      /* 32 bytes */
    int32_t id, frame;                  /* report ID and "Frame" (main.cpp:381) */
    int32_t index;                      /* 0-based stream index of the key frame: which enhanced frame to write */
    float   overlap, blur;              /* trigger overlap (after -2.0 -> 0.41), best blur (0, 0 in row 0) */
    int32_t reserved[3];
} uwip_keyframe_row;
int uwip_keyframe_config_default(uwip_keyframe_config *kc);          /* 0.4, 11, lookback 8, 4096 rows */
/* Switch the pipe to key-frame mode (or re-configure it): before the first step or right after uwip_pipe_reset.  Waits for
 * the stream (it re-allocates the feature slots and uploads the fixed pair list). */
int uwip_pipe_keyframe_chain(uwip_pipe *p, const uwip_keyframe_config *kc);
/* The NEXT step that runs the overlap stage is the stream's last, and only its first `valid` frames (1..frames) are real (a
 * caller that pads its last batch by repeating a frame passes the real count).  In key-frame mode only those frames enter
 * the chain: the padding is not compared (NaN ratios) and a window still open is closed with its best so far.  In the
 * predecessor mode `valid` changes nothing in that step: every frame, padding included, is matched against its predecessor
 * as before.  In both modes the pipe starts a new stream after that step, as after a reset. */
int uwip_pipe_end_of_stream(uwip_pipe *p, int valid);
/* Rows closed since the last call, up to `cap` of them (*n = how many; call again while *n == cap).  Waits for the stream.
 * An error when the caller fell more than max_rows rows behind (those rows are gone: the call says so instead of dropping
 * them silently) or when a batch was not resolved within the round bound (reported once; the chain then stays stopped until
 * the next stream begins). */
int uwip_pipe_keyframes(uwip_pipe *p, uwip_keyframe_row *h_rows, int cap, int *n);
/* The same decision chain with the same batch / round scheme on the host, the overlaps and blurs coming from callbacks:
 * overlap(user, key, frame) = calcOverlap of stream frame `frame` against stream frame `key`, blur(user, frame) =
 * calcBlur(resize(frame)).  n_frames frames in batches of `batch`, the last one holding the rest (end of stream).  Writes up
 * to `cap` rows (*n_rows = all rows) and, when `rounds` != NULL, the fallback rounds each batch used ([ceil(n_frames /
 * batch)]).  No device needed: the tests check the device chain's logic against the reference loop with it. */
typedef float (*uwip_kf_overlap_fn)(void *user, int32_t key, int32_t frame);
typedef float (*uwip_kf_blur_fn)(void *user, int32_t frame);
int uwip_keyframe_chain_host(const uwip_keyframe_config *kc, int n_frames, int batch, uwip_kf_overlap_fn overlap,
                             uwip_kf_blur_fn blur, void *user, uwip_keyframe_row *rows, int cap, int *n_rows, int32_t *rounds);
/* The fallback-round bound R a pipe queues per step (key-frame mode): (frames - 1) / s + 1 with s = kWindow + 1,
 * or s = min(lookback, frames - 1) + 1 when kWindow = 0.  -1 for a bad configuration. */
int uwip_keyframe_max_rounds(const uwip_keyframe_config *kc, int frames);

/* ---- writing the frames: baseline JPEG on the device ---------------------------------------------------------------
 * cv::imwrite(".jpg") for a batch, on the device (cli/jpeg.hpp is the host form; same bytes): baseline JFIF with the Annex K
 * tables scaled by `quality` (clamped to 1..100; cv::imwrite's default is 95), 4:2:0 for 3-channel BGR frames, one component
 * for 1-channel frames; any step / frame_stride / alignment, rows and cols 1..65535.
 * uwip_jpeg_bound: the worst-case stream length of one frame, 0 for a bad geometry (host, pure, no device needed).  Derivation
 *   from the code lengths: a block holds one DC code (the longest standard one has 11 bits, chroma category 11) with at most
 *   11 magnitude bits and 63 AC coefficients of at most a 16-bit code and 10 magnitude bits each -- a ZRL only replaces
 *   coefficients that are zero and an EOB only follows a shorter block -- so at most 22 + 63 * 26 = 1660 bits; the scan has
 *   ceil(rows / m) * ceil(cols / m) MCUs of 6 blocks (m = 16, colour) or 1 block (m = 8, grey); every byte may be 0xFF and
 *   stuffed, hence twice ceil(blocks * 1660 / 8); plus the header (623 bytes colour, 328 grey) and FF D9.
 * uwip_jpeg_encode: asynchronous on the context's stream.  Frame f's stream starts at d_streams + f * slot_bytes and
 *   d_sizes[f] is its length; a frame whose stream is longer than slot_bytes writes nothing and reports -(needed length) -- a
 *   status, not an error: the other frames of the batch are unaffected.  The library's workspace for the unstuffed stream is
 *   bounded by slot_bytes per frame as well.
 * uwip_jpeg_encode_host: the same into host memory (frame f at h_streams + f * slot_bytes): encodes, waits, and copies only
 *   the bytes each stream uses. */
size_t uwip_jpeg_bound(int rows, int cols, int channels);
int uwip_jpeg_encode(uwip_ctx *ctx, const uwip_batch_u8 *frames, int quality, uint8_t *d_streams, size_t slot_bytes,
                     int64_t *d_sizes);
int uwip_jpeg_encode_host(uwip_ctx *ctx, const uwip_batch_u8 *frames, int quality, uint8_t *h_streams, size_t slot_bytes,
                          int64_t *h_sizes);

/* ---- writing the frames: PNG on the device -------------------------------------------------------------------------------
 * cv::imwrite(".png") for a batch, on the device: lossless; the bytes differ from OpenCV's and from cli/imgio.hpp's, the pixels
 * do not.  8-bit frames with 1 channel (colour type 0) or 3 channels (BGR in, RGB in the file, colour type 2); any step /
 * frame_stride / alignment, rows and cols 1..65535.  No interlace, no ancillary chunks: signature, IHDR, IDATs, IEND.
 * filter: -1 is the adaptive choice, made per row: choose the type 0..4 whose filtered row has the smallest sum of
 *   min(v, 256 - v) over its bytes; ties go to the lowest type number; row 0 uses the same rule with the row above taken as
 *   zeros.  0..4 forces that type on every row.
 * The zlib stream: the filtered bytes (rows x (1 + cols * channels)) are cut into chunks of uwip_png_chunk_bytes() = 32768
 *   bytes and each chunk is coded on its own.  Tokens are zlib's Z_RLE parse: the first byte of a run is a literal, the equal
 *   bytes that follow are matches at distance 1 of length 3..258, leftovers shorter than 3 are literals.  Each chunk is one
 *   deflate block: stored (BTYPE 00) where that is not longer in bytes, else fixed (01) where that is not longer in bits, else
 *   dynamic (10) with a literal/length code limited to 15 bits and a code-length code limited to 7.  Every chunk but the last
 *   ends with an empty stored block (00 00 FF FF), the last block carries BFINAL; one IDAT per chunk, then one IDAT with the
 *   Adler-32 of the filtered bytes.
 * uwip_png_bound: the worst-case stream length of one frame, 0 for a bad geometry (host, pure, no device needed).  Derivation:
 *   a chunk is never longer than its stored form, 5 bytes of block header and its bytes, plus the 5 bytes of the empty stored
 *   block (3 bits, padding, LEN, NLEN) and the 12 of its IDAT's length, type and CRC: filtered bytes + 22 per chunk; per frame
 *   signature and IHDR (33), the zlib header (2), the Adler-32's IDAT (16) and IEND (12): 63.
 * uwip_png_encode: asynchronous on the context's stream.  Frame f's stream starts at d_streams + f * slot_bytes and d_sizes[f]
 *   is its length; a frame whose stream is longer than slot_bytes writes nothing and reports -(needed length) -- a status, not
 *   an error: the other frames of the batch are unaffected.  Without a device it fails with UWIP_ERR_HIP.
 * uwip_png_encode_host: the same into host memory (frame f at h_streams + f * slot_bytes): encodes, waits, and copies only
 *   the bytes each stream uses. */
size_t uwip_png_bound(int rows, int cols, int channels);
int uwip_png_chunk_bytes(void);
int uwip_png_encode(uwip_ctx *ctx, const uwip_batch_u8 *frames, int filter, uint8_t *d_streams, size_t slot_bytes,
                    int64_t *d_sizes);
int uwip_png_encode_host(uwip_ctx *ctx, const uwip_batch_u8 *frames, int filter, uint8_t *h_streams, size_t slot_bytes,
                         int64_t *h_sizes);

/* ---- reading the frames: baseline JPEG on the device ---------------------------------------------------------------
 * cv::imread / cv::imdecode for a batch, on the device (jpeg::decode of cli/jpeg.hpp is the host form; where the status is 0,
 * the same pixels byte for byte, the host decoder's rules for a truncated segment included: bits past the end, or past a
 * marker that is no RSTn, read as zeros).  Baseline (SOF0 / SOF1, 8 bit, Huffman), one scan of all components, 1 or 3
 * components, restart intervals; Motion-JPEG frames without DHT use the Annex K tables.  Three components are interleaved,
 * have sampling factors 1..2 and at most 10 blocks per MCU (T.81 B.2.3: all three sampled 2x2 is refused).  One component
 * is not interleaved (T.81 A.2.2): its MCU is one block, in raster order over ceil(cols / 8) x ceil(rows / 8) blocks, and
 * the factors its SOF gives, any of 1..4, are read as 1x1, as libjpeg does; such a stream is never HOST_ONLY for its factors.
 * uwip_jpeg_info: the header parse alone (host, pure, no device needed): rows, cols and the component count (1 or 3) of a
 *   stream jpeg::decode would start to decode; UWIP_ERR_UNSUPPORTED where its parse fails (not 8 bit, progressive and the
 *   other non-baseline SOFs, more than one SOF, a component count other than 1 or 3, three components with sampling factors
 *   outside 1..2 or more than 10 blocks per MCU, short segments, no scan).  The factors of a single component do not
 *   matter: any that SOF can hold, 1..4, are read.
 * uwip_jpeg_decode: parses the n streams on the host, copies their entropy-coded segments through page-locked staging owned
 *   by the library to the device on the context's stream, queues the kernels and returns without waiting (reuse of the
 *   staging buffer waits, polling an event, for the previous call's upload only).  `out` is a device batch of n frames with 3
 *   channels (BGR; a one-component stream is replicated) or 1 channel (one-component streams only); any step, frame_stride
 *   and alignment.  d_status[f] (device) is 0 or one of the codes below -- a status, not an error: the other frames are
 *   complete, and the pixels of a frame with a negative status are unspecified but stay inside its slot.  A caller decodes
 *   such a frame on the host and uploads it into its slot.
 *     UWIP_JPEG_BAD_STREAM     jpeg::decode returns false: parse errors, an undecodable Huffman code, a DC category above 11,
 *                              a DC predictor outside 16 bits, a run past coefficient 63
 *     UWIP_JPEG_SIZE_MISMATCH  the SOF size is not out->rows x out->cols, or a colour stream goes into a 1-channel batch
 *     UWIP_JPEG_HOST_ONLY      the host decoder reads the stream, the device does not: one of three components sampled 1x2
 *                              against the largest factors, or an entropy-coded segment whose markers before the first
 *                              non-RST marker are not exactly ceil(MCUs / Ri) - 1 RSTn in cyclic order
 *   opts (NULL: the defaults): sync_rounds is the number of synchronisation rounds of the entropy decoder, -1 the
 *   library's choice, 0 none (one lane per restart interval decodes serially); d_unsettled, when not NULL, receives two
 *   64-bit counts on the device: subsequences still unsettled after the rounds, subsequences in all.
 * uwip_jpeg_decode_host: the same, waits, and returns the status array in host memory. */
#define UWIP_JPEG_BAD_STREAM    (-1)
#define UWIP_JPEG_SIZE_MISMATCH (-2)
#define UWIP_JPEG_HOST_ONLY     (-3)
typedef struct uwip_jpeg_decode_opts {
    int32_t sync_rounds;
    int32_t reserved;             /* 0 */
    uint64_t *d_unsettled;
} uwip_jpeg_decode_opts;
int uwip_jpeg_info(const uint8_t *buf, size_t len, int32_t *rows, int32_t *cols, int32_t *channels);
int uwip_jpeg_decode(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                     const uwip_jpeg_decode_opts *opts, int32_t *d_status);
int uwip_jpeg_decode_host(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                          const uwip_jpeg_decode_opts *opts, int32_t *h_status);

/* ---- reading the frames: PNG on the device ---------------------------------------------------------------------------
 * cv::imread / cv::imdecode of a .png for a batch, on the device (imgio::read_png of cli/imgio.hpp is the host form and the
 * contract: where the status is 0 the pixels are its pixels byte for byte, and the status is 0 exactly where it returns true
 * and the size fits).  8 bit, no interlace, colour types 0 / 2 / 4 / 6: alpha is dropped, RGB becomes BGR, grey is replicated
 * into a 3-channel batch.  Chunk CRCs are not checked (the host reader checks none).  The zlib stream is the concatenation of
 * the IDAT payloads up to IEND and must pass what zlib's uncompress passes: the header check (method 8, CINFO <= 7, FCHECK, no
 * FDICT), zlib's rules for sets of code lengths (an over-subscribed set is refused, an incomplete one allowed only as zlib
 * allows it, the end-of-block code must be present, HLIT <= 286, HDIST <= 30), no distance beyond the bytes already produced,
 * a final block, the Adler-32, and an inflated length of exactly rows * (1 + cols * samples).  Bytes behind the stream's end
 * are ignored; a filter type above 4 behaves as type 0, as in the host loop.
 * uwip_png_info: the chunk walk, the IHDR rules and the zlib header alone (host, pure, no device needed): rows, cols and the
 *   channels (1 for colour types 0 / 4, 3 for 2 / 6) of a stream read_png would inflate; UWIP_ERR_UNSUPPORTED otherwise
 *   (palette, other depths, interlace, a chunk that overruns the file, no IDAT ...).
 * uwip_png_decode: parses the n streams on the host, copies their IDAT payloads through page-locked staging owned by the
 *   library to the device on the context's stream, queues the kernels and returns without waiting (reuse of the staging
 *   buffer waits, polling an event, for the previous call's upload only).  `out` is a device batch of n frames with 3 channels
 *   or 1 channel (grey streams only); any step, frame_stride and alignment.  The workspace is sized from `out` at four
 *   samples per pixel, never from an IHDR.  d_status[f] (device) is 0 or one of the codes below -- a status, not an error:
 *   the other frames are complete, and the pixels of a frame with a negative status are unspecified but stay inside its slot.
 *     UWIP_PNG_BAD_STREAM     read_png returns false
 *     UWIP_PNG_SIZE_MISMATCH  the IHDR size is not out->rows x out->cols, or a colour stream (types 2 / 6) goes into a
 *                             1-channel batch
 *   opts (NULL: the defaults): segmented 1 (and -1, the library's choice) first inflates the segments between the IDAT
 *   boundaries that follow an empty stored block (00 00 FF FF), one wavefront each, segment i at inflated offset
 *   i * uwip_png_chunk_bytes(), and accepts a frame only when every segment proves the assumption; every other
 *   frame, and with segmented 0 every frame, is inflated from its first byte by one wavefront.  segmented 2 puts a pass between
 *   the two for streams without such boundaries (any other encoder's): every good frame the segments did not finish and whose
 *   zlib stream is longer than chunk_bytes is cut into chunks of chunk_bytes compressed bytes, one wavefront per chunk looks
 *   for the first bit that parses as the start of a dynamic block and measures the blocks from there, and a frame is accepted
 *   only when the measured chunks form one chain from the zlib header to the final block that produces exactly the frame's
 *   bytes; the chunks are then inflated in parallel.  A frame not accepted there takes the one-wavefront pass,
 *   which alone decides a bad status.  The pixels and statuses depend neither on segmented nor on chunk_bytes.  d_counts, when
 *   not NULL, receives three 64-bit counts on the device: units accepted from a parallel pass (segments, and with segmented 2
 *   the chunks of the frames accepted from found block starts), frames that took the serial pass, frames in all.  Without a
 *   device the call fails with UWIP_ERR_HIP (UWIP_ERR_INVALID where opts itself is out of range).
 * uwip_png_decode_host: the same, waits, and returns the status array in host memory. */
#define UWIP_PNG_BAD_STREAM    (-1)
#define UWIP_PNG_SIZE_MISMATCH (-2)
typedef struct uwip_png_decode_opts {
    int32_t   segmented;   /* -1 library's choice (= 1), 0 one wavefront per stream only, 1 try IDAT-boundary segments first,
                              2 those segments, then found block starts for the frames they do not finish */
    int32_t   chunk_bytes; /* segmented 2: compressed bytes per speculative chunk, 256 .. 1 MiB; 0 the library's choice (and
                              0 in every other mode) */
    uint64_t *d_counts;    /* may be NULL; device, 3 x u64 */
} uwip_png_decode_opts;
int uwip_png_info(const uint8_t *buf, size_t len, int32_t *rows, int32_t *cols, int32_t *channels);
int uwip_png_decode(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                    const uwip_png_decode_opts *opts, int32_t *d_status);
int uwip_png_decode_host(uwip_ctx *ctx, const uint8_t *const *h_streams, const size_t *h_sizes, int n, const uwip_batch_u8 *out,
                         const uwip_png_decode_opts *opts, int32_t *h_status);

/* ---- the pipe on files: compressed frames in, compressed (key) frames out, no host wait ----------------------------------
 * A step that takes a batch of .jpg / .png streams and later hands back the finished .jpg / .png streams of exactly the frames
 * asked for -- every good frame (UWIP_EMIT_ALL) or the key frames whose rows closed in that step (UWIP_EMIT_KEYFRAMES) -- so that
 * only compressed bytes cross the link.  Decode, the four stages, the selection of the frames, the gather of their pixels, the
 * encoders and the packing of the streams are queued on the context's stream; nothing waits for the walker's decisions
 * (DESIGN.md 7c).
 * uwip_pipe_streams_config: format UWIP_STREAM_JPEG / UWIP_STREAM_PNG; quality as uwip_jpeg_encode clamps it, 0 means 95;
 *   png_filter -1..4 as uwip_png_encode; emit UWIP_EMIT_ALL / UWIP_EMIT_KEYFRAMES; slot_bytes per emitted frame, 0 = the raw
 *   frame size rows * cols * 3; depth = the steps whose results stay collectable, >= 2.  uwip_pipe_streams_config_default: JPEG,
 *   95, -1, UWIP_EMIT_ALL, 0, 2.
 * uwip_pipe_streams: before the first step or right after uwip_pipe_reset; allocates what the mode needs (it waits for the
 *   stream).  UWIP_EMIT_KEYFRAMES on a pipe that is not in key-frame mode (uwip_pipe_keyframe_chain comes first) is
 *   UWIP_ERR_INVALID.  A pipe that has been given a streams configuration takes its steps of one stream through
 *   uwip_pipe_step_streams only: the raw-pixel entries do not feed the carried frame.
 * uwip_pipe_step_streams: n must be the pipe's `frames`.  JPEG and PNG inputs may be mixed: they are told apart by the PNG
 *   signature, run by run.  The call parses the streams and copies them through the decoders' staging (uwip_jpeg_decode /
 *   uwip_png_decode), so the caller's buffers are free when it returns; it then queues decode -> the four stages -> selection ->
 *   encode -> pack and returns without waiting for the device.  *ticket names the step's result.  The throttle (max_in_flight)
 *   applies as in uwip_pipe_step.  Results live in `depth` slots used in turn: a step whose slot still holds a result that has
 *   not been collected is refused with UWIP_ERR_INVALID (nothing is queued), not silently lost.  uwip_pipe_end_of_stream,
 *   uwip_pipe_keyframes, uwip_pipe_last_params and uwip_pipe_reset keep their meaning; after uwip_pipe_end_of_stream(valid) only
 *   the first `valid` frames of the step are emitted under UWIP_EMIT_ALL (the padding is not a frame of the stream).
 *   A frame with a negative decoder status is zero-filled on the device before the chain, so the step is deterministic; its
 *   status is reported, and under UWIP_EMIT_ALL it is not emitted (no entry, no bytes); its neighbours are untouched.  A caller
 *   that wants a host fallback decodes the frame itself and uses the raw-pixel entries.
 * uwip_pipe_collect: the only call that waits, and only for that step.  h_status [frames]: the decoders' statuses; h_ratio
 *   [frames] (may be NULL): the step's ratios (uwip_pipe_step's d_ratio); h_outs [cap]: one uwip_stream_out per emitted frame
 *   -- `index` the 0-based stream index of the frame, `row_id` the key-frame row's ID (-1 with UWIP_EMIT_ALL), `size` its bytes
 *   or -(needed) when the stream outgrew its slot (such a frame is absent from the blob), `offset` its position in the blob --
 *   in row order (key frames) or frame order (all); *n_outs their number (at most frames + 1).  h_blob receives the emitted
 *   streams back to back, *blob_bytes of them.  When cap or blob_cap is too small the call fails with UWIP_ERR_INVALID, reports
 *   *n_outs and *blob_bytes, and the result stays collectable.  A result can be collected once.
 * uwip_pipe_result_params: (BS, CL) the aclahe stage chose in the step `ticket` names, h_bs / h_cl [frames]; waits for that step
 *   only (uwip_pipe_last_params gives the most recent step's and waits for the stream).  Before the result is collected.
 * The stream of an emitted frame is byte for byte what uwip_jpeg_encode / uwip_png_encode give for that enhanced frame with the
 * same quality / filter and slot. */
#define UWIP_STREAM_JPEG    0
#define UWIP_STREAM_PNG     1
#define UWIP_EMIT_ALL       0
#define UWIP_EMIT_KEYFRAMES 1
typedef struct uwip_pipe_streams_config {
    int32_t format;        /* UWIP_STREAM_JPEG / UWIP_STREAM_PNG */
    int32_t quality;       /* JPEG: 1..100 (clamped), 0 = 95 */
    int32_t png_filter;    /* PNG: -1 adaptive, 0..4 */
    int32_t emit;          /* UWIP_EMIT_ALL / UWIP_EMIT_KEYFRAMES */
    size_t  slot_bytes;    /* per emitted frame; 0 = rows * cols * 3 */
    int32_t depth;         /* >= 2 */
    int32_t reserved;      /* 0 */
} uwip_pipe_streams_config;
typedef struct uwip_stream_out {        /* 24 bytes */
    int32_t index, row_id;
    int64_t size, offset;
} uwip_stream_out;
int uwip_pipe_streams_config_default(uwip_pipe_streams_config *cfg);
int uwip_pipe_streams(uwip_pipe *p, const uwip_pipe_streams_config *cfg);
int uwip_pipe_step_streams(uwip_pipe *p, const uint8_t *const *h_streams, const size_t *h_sizes, int n, uint64_t *ticket);
int uwip_pipe_collect(uwip_pipe *p, uint64_t ticket, int32_t *h_status, float *h_ratio, uwip_stream_out *h_outs, int cap,
                      int *n_outs, uint8_t *h_blob, size_t blob_cap, size_t *blob_bytes);
int uwip_pipe_result_params(uwip_pipe *p, uint64_t ticket, int32_t *h_bs, int32_t *h_cl);

/* ---- strip mosaic: the key frames warped and blended into one image ------------------------------------------------
 * The reference calls videostrip "automatic frame extraction for 2D mosaic" and stops at the frame list (main.cpp:368-381
 * writes the key frame and its row); the homography calcOverlap computes per pair (findHomography, videostrip.cpp:270) is
 * used for overlapArea alone (:280).  A strip continues from there: it keeps the frames it is given at the working size
 * (cv::resize to 640 wide, main.cpp:242,311), matches every frame against its predecessor with the matcher's d_H output,
 * chains the homographies (G_0 = I, G_k = G_{k-1} H_k, normalised), lays out one canvas per SEGMENT -- a frame that cannot be
 * chained (no homography, a degenerate or implausible one, a canvas beyond the limit) starts a new one -- and renders a
 * segment by a gather over the canvas: every pixel samples every frame that covers it, bilinearly with 5-bit fractions.
 * The arithmetic is stated once in csrc/strip_core.hpp and is exact: coordinates in float64 without
 * fused operations, everything behind the source position in integers.
 * A quick look, not a mosaic: working resolution only; exposure compensation as one gain per frame and channel from the
 * overlaps of CONSECUTIVE frames of a segment (uwip_strip_gains, below), seams found in those same overlaps
 * (uwip_strip_seams, below) and multi-band blending along the feather weights, not along the found seams (uwip_strip_bands,
 * below) -- no pairs that are not consecutive, no bundle adjustment, no loop closure.
 * A strip is bound to the context it was made from (its stream, its thread rule); destroy it before the context. */
typedef struct uwip_strip uwip_strip;
typedef struct uwip_strip_config {
    int32_t  rows, cols;                 /* geometry of the BGR frames handed to uwip_strip_add */
    int32_t  batch, max_frames;          /* most frames per add; capacity of the strip (frames are kept at working size) */
    int32_t  max_canvas_rows, max_canvas_cols;   /* default 16384 x 16384 */
    float    max_scale;                  /* default 4 */
    uint32_t detect_flags, match_flags, seed;    /* as uwip_pipe_config; defaults = the reference's rules, seed 1 */
    int32_t  videoWidth, videoHeight;    /* 0 = cols / rows */
} uwip_strip_config;
typedef struct uwip_strip_segment { int32_t first, count, x0, y0, rows, cols, reserved[2]; } uwip_strip_segment;
#define UWIP_STRIP_FEATHER 0   /* weights 1 + distance to the frame's border, the default */
#define UWIP_STRIP_FIRST   1   /* the covering frame with the smallest index */
#define UWIP_STRIP_LAST    2   /* the covering frame with the largest index */
int uwip_strip_config_default(uwip_strip_config *cfg, int rows, int cols);       /* batch 16, 1024 frames */
int uwip_strip_create(uwip_ctx *ctx, const uwip_strip_config *cfg, uwip_strip **out);
int uwip_strip_destroy(uwip_strip *s);          /* drains the stream first */
int uwip_strip_reset(uwip_strip *s);            /* forget every frame: a new video */
int uwip_strip_count(const uwip_strip *s, int *n);
const char *uwip_strip_last_error(const uwip_strip *s);
/* Append frames->frames (1..batch) frames of the configured geometry, the key frames main.cpp:368-381 writes.  The frames are
 * resized into the strip's store (uwip_resize_bgr), detected into feature slots 1..n (slot 0 carries the previous call's last
 * frame, the `struct keyframe` cache of videostrip.hpp:62-68), matched (i, i - 1) in one launch (videostrip.cpp:229-270), and
 * the pairs' H and ratio are appended.  With d_H_inject [n][9] f64 and d_ratio_inject [n] f32 (device; both or neither) detect
 * and match are skipped and those are appended instead, and the frames are stored AS GIVEN, without the resize: injected
 * homographies are in the coordinates of the frames they come with (the parity hook, as uwip_dehaze's d_B_inject).  A strip
 * takes one of the two forms from its first add until uwip_strip_reset.  Entry 0 of a strip's first add is not read.
 * Asynchronous.  More than max_frames frames in total: UWIP_ERR_INVALID, and nothing is queued. */
int uwip_strip_add(uwip_strip *s, const uwip_batch_u8 *frames, const double *d_H_inject, const float *d_ratio_inject);
/* Chain and lay out what has been added (k_strip_chain), wait, and return the segments, up to `cap` (>= 1) of them per call
 * (*n = how many; call again while *n == cap for the following ones -- a call that returns fewer ends the listing, and
 * the next call starts from segment 0 again; so does the first call after an add). */
int uwip_strip_layout(uwip_strip *s, uwip_strip_segment *h_segs, int cap, int *n);
/* Parity tap, after uwip_strip_layout: h_G / h_Ginv [count][9] f64, h_seg [count] i32, h_box [count][4] i32 (x0, y0, x1, y1 on
 * the segment's canvas, inclusive); any may be NULL.  Waits for the stream. */
int uwip_strip_transforms(uwip_strip *s, double *h_G, double *h_Ginv, int32_t *h_seg, int32_t *h_box);
/* Render one segment of the last layout into `canvas`: one frame, 3 channels, the segment's rows x cols, any step / base.
 * fill [3] (NULL = black) is what uncovered pixels take; d_cover (may be NULL) [rows][cols] u8, packed: the number of frames
 * that cover each pixel, saturating at 255.  Asynchronous. */
int uwip_strip_render(uwip_strip *s, int segment, int mode, const uint8_t *fill, const uwip_batch_u8 *canvas, uint8_t *d_cover);
/* The chain by itself on the host (csrc/strip_core.hpp, the source k_strip_chain runs), no device needed: what
 * uwip_keyframe_chain_host is to the selector.  w x h: the stored frames; h_H [n][9], h_ratio [n]; outputs as
 * uwip_strip_transforms and uwip_strip_layout (h_segs: up to cap entries, *n_segs = all). */
int uwip_strip_chain_host(int w, int h, int max_canvas_rows, int max_canvas_cols, float max_scale, const double *h_H,
                          const float *h_ratio, int n, double *h_G, double *h_Ginv, int32_t *h_seg, int32_t *h_box,
                          uwip_strip_segment *h_segs, int cap, int *n_segs);
/* Gain compensation (Brown & Lowe 2007, section 6, restricted to the consecutive pairs of a segment; csrc/strip_core.hpp,
 * DESIGN.md section 7d).  The key frames are enhanced one by one, so two of the same sea floor differ in level and colour
 * balance; one gain per frame and channel, solved from the means of the pairs' overlaps, takes the steps out of the seams.
 *   measure  for every pixel of frame k (not a segment's first) the sample of frame k - 1 at the same plane point; a pixel
 *            counts when it is covered and all six values (1024 x 8-bit levels) lie in 1024 lo .. 1024 hi; stats[k] = the
 *            count and the sums of the three samples and of the three pixels, seven uint64 (zeros for a first frame);
 *   solve    per segment and channel the tridiagonal system of the paper's error with deviations sigma_n (levels) and
 *            sigma_g (gain), pairs of fewer than min_pixels pixels left out, in float64; gq = the gain in 1/4096,
 *            clamped to 1024..16384 (0.25..4);
 *   apply    uwip_strip_render with mode | UWIP_STRIP_GAIN multiplies every sample by its frame's gain, saturating at 255,
 *            before it is blended; the cover plane is unchanged, and so is every render without the bit. */
typedef struct uwip_strip_gain_config { float sigma_n, sigma_g; int32_t lo, hi, min_pixels, reserved[3]; } uwip_strip_gain_config;
#define UWIP_STRIP_GAIN 0x100     /* OR into uwip_strip_render's mode */
int uwip_strip_gain_config_default(uwip_strip_gain_config *cfg);     /* sigma_n 10, sigma_g 0.1, lo 5, hi 250, min_pixels 64 */
/* Measure and solve (k_strip_gain_stats, k_strip_gain_solve) for the frames of the last layout.  cfg NULL = the defaults;
 * sigma_* <= 0, lo > hi, lo or hi outside 0..255 or min_pixels < 1: UWIP_ERR_INVALID.  Without a uwip_strip_layout since the
 * last add: UWIP_ERR_INVALID, nothing is queued.  Asynchronous.  An add, a reset or a new layout (the first
 * uwip_strip_layout after an add; listing the same layout again keeps them) drops the gains, and mode | UWIP_STRIP_GAIN
 * without gains is UWIP_ERR_INVALID. */
int uwip_strip_gains(uwip_strip *s, const uwip_strip_gain_config *cfg);
/* Parity tap: h_gq [count][3] i32, h_g [count][3] f64 (the solution before it is quantised), h_stats [count][7] u64; any may be
 * NULL.  Waits for the stream.  After uwip_strip_set_gains: g = gq / 4096 and the statistics are zero. */
int uwip_strip_gain_values(uwip_strip *s, int32_t *h_gq, double *h_g, uint64_t *h_stats);
/* Inject gains instead (host, [count][3], each 1024..16384), after a layout: the parity hook of the gained render. */
int uwip_strip_set_gains(uwip_strip *s, const int32_t *h_gq);
/* The solve by itself on the host (the source k_strip_gain_solve runs), no device needed: h_stats [n][7], h_seg [n] as
 * uwip_strip_transforms returns it, cfg NULL = the defaults -> h_gq [n][3], h_g [n][3] (either may be NULL). */
int uwip_strip_gain_solve_host(const uint64_t *h_stats, const int32_t *h_seg, int n, const uwip_strip_gain_config *cfg,
                               int32_t *h_gq, double *h_g);
/* Multi-band blending (Brown & Lowe 2007, section 7; csrc/strip_core.hpp): low frequencies are blended
 * over a wide zone and high frequencies over a narrow one, so levels join smoothly while texture stays sharp where two
 * misregistered frames meet.  No pyramid of the canvas: every frame carries an undecimated stack in its own coordinates.
 *   stack    level 0 is the stored frame; level l + 1 = level l under (1, 4, 6, 4, 1) x (1, 4, 6, 4, 1) with taps 2^l pixels
 *            apart, borders clamped: (sum + 128) >> 8, one rounding per level, u8;
 *   render   a covering frame k has one tap and one feather weight q_k (those of the other modes); S[k][l] = the bilinear
 *            sample of its level l (times the frame's gain with UWIP_STRIP_GAIN), D[k][l] = S[k][l] - S[k][l+1]; the band
 *            weight w[k][l] = max(0, q_k - max_k q_k + ramp[l]) is a ramp of ramp[l] feather units behind the best frame
 *            (1: winner takes all, ties share); b = sum_l round(sum_k w D / sum_k w), the last level is blended with the
 *            weights q_k themselves, out = clamp(floor((sum q S[levels] + (b + 512) sum q) / (1024 sum q)), 0, 255).
 * A pixel that one frame covers is what UWIP_STRIP_FIRST gives; the cover plane is that of the other modes. */
typedef struct uwip_strip_bands_config { int32_t levels; int32_t ramp[4]; int32_t reserved[3]; } uwip_strip_bands_config;
#define UWIP_STRIP_MULTIBAND 3    /* uwip_strip_render's mode, alone or with UWIP_STRIP_GAIN; uwip_strip_bands first */
int uwip_strip_bands_config_default(uwip_strip_bands_config *cfg);   /* levels 4, ramps 1, 2, 4, 8 */
/* Build the stacks of every frame added so far (k_strip_stack, one launch per level) and keep the ramps for the renders.
 * cfg NULL = the defaults; levels outside 1..4, a ramp[l] for l < levels outside 1..4096, or no frame: UWIP_ERR_INVALID, nothing
 * is queued.  The stacks' store (levels x count x rows x cols x 3 bytes of the stored geometry) is allocated here, not at
 * uwip_strip_create, and freed by uwip_strip_reset and uwip_strip_destroy; a failed allocation returns UWIP_ERR_NOMEM and
 * leaves the strip as it was, without stacks.  Asynchronous.  An add or a reset drops the stacks (UWIP_STRIP_MULTIBAND without
 * them is UWIP_ERR_INVALID); a new layout keeps them: they depend on the frames alone. */
int uwip_strip_bands(uwip_strip *s, const uwip_strip_bands_config *cfg);
/* Parity tap: level 1..levels of a frame's stack, h_out [rows][cols][3] u8 of the stored geometry, packed.  Waits for the
 * stream. */
int uwip_strip_band_level(uwip_strip *s, int frame, int level, uint8_t *h_out);
/* The stack by itself on the host (the source k_strip_stack runs), no device needed: frame [h][w][3] u8 packed, levels 1..4
 * -> out [levels][h][w][3].  A null pointer, w or h outside 1..32768 or levels outside 1..4: UWIP_ERR_INVALID. */
int uwip_strip_stack_host(const uint8_t *frame, int w, int h, int levels, uint8_t *out);
/* Seams found in the images (csrc/strip_core.hpp): the other modes decide from geometry alone where one
 * key frame ends and the next begins, and cut through whatever moved between the two.  Frame k of a segment, other than its
 * first, has one seam against frame k - 1, in frame k's own pixel grid: the path through the overlap along which the two
 * frames differ least, one dynamic programme per pair.
 *   orient   the direction (dx, dy) from frame k - 1's centre to frame k's, in k's coordinates; |dy| >= |dx|: axis 0, the seam is
 *            a function of x (steps t = x, T = cols; states s = y, S = rows), else axis 1 (t = y, s = x); sign +1 when the
 *            larger component is >= 0, else -1; orient = axis | (sign < 0 ? 2 : 0);
 *   cost     C[t][s] = sum_c |Pa[c] - Pb[c]| + prior |a_k - a_p| for a pixel of frame k that frame k - 1 covers (Pb = 1024 x
 *            the pixel, Pa = the bilinear sample of k - 1, both times their frame's gain when the strip has gains; a = the
 *            distance along the state axis to the nearer border, a_p of k - 1's nearest pixel), 1 << 22 elsewhere;
 *   path     E[0] = C[0], E[t][s] = C[t][s] + min(E[t-1][s], E[t-1][s-1], E[t-1][s+1]), ties in that order; the end is the
 *            smallest s among the minima of E[T-1]; seam[t] in 0..S-1 by walking back, total = the path's cost;
 *   render   UWIP_STRIP_SEAM: frame k takes a pixel whose nearest source pixel is (t, s) iff sign (s - seam_k[t]) >= 0 (a
 *            segment's first frame: never); the winner is the largest covering k that takes it, else the smallest covering k;
 *            out = (P + 512) >> 10 of the winner, as FIRST and LAST.  The cover plane is that of the other modes.
 * Frames larger than 1023 in either direction (of the stored geometry) are refused: path totals stay below 2^32. */
typedef struct uwip_strip_seam_config { int32_t prior; int32_t reserved[3]; } uwip_strip_seam_config;   /* prior 0..4096 */
#define UWIP_STRIP_SEAM 4         /* uwip_strip_render's mode, alone or with UWIP_STRIP_GAIN; uwip_strip_seams first */
int uwip_strip_seam_config_default(uwip_strip_seam_config *cfg);     /* prior 1024: one grey level per pixel of imbalance */
/* Find the seams of the frames of the last layout (k_strip_seam_cost, k_strip_seam_path; pairs in rounds of 64), with the
 * strip's gains if it has any.  cfg NULL = the defaults; a prior outside 0..4096, no layout since the last add, or a stored
 * frame beyond 1023 x 1023: UWIP_ERR_INVALID, nothing is queued.  The scratch (64 pairs' costs: 4 bytes per pixel) is
 * allocated here and kept until uwip_strip_reset / uwip_strip_destroy; a failed allocation returns UWIP_ERR_NOMEM and leaves the
 * strip as it was.  Asynchronous.  An add, a reset, a new layout, uwip_strip_gains and uwip_strip_set_gains drop the seams, and
 * UWIP_STRIP_SEAM without seams is UWIP_ERR_INVALID. */
int uwip_strip_seams(uwip_strip *s, const uwip_strip_seam_config *cfg);
/* Parity tap: h_seam [count][max(cols, rows)] i32 of the stored geometry (entries 0..T-1 of a row are the seam, the others and
 * a segment's first frame -1), h_orient [count] i32, h_total [count] u64 (a first frame: 0); any may be NULL.  Waits for the
 * stream. */
int uwip_strip_seam_values(uwip_strip *s, int32_t *h_seam, int32_t *h_orient, uint64_t *h_total);
/* Inject seams instead (host, laid out as the tap's), after a layout: the parity hook of the render.  Entries 0..T-1 of a frame
 * that is not its segment's first must lie in 0..S (S with sign +1: the frame takes nothing) and its orient in 0..3, else
 * UWIP_ERR_INVALID and the strip's seams stay as they were; a first frame's entries are not read.  Totals read 0 afterwards. */
int uwip_strip_set_seams(uwip_strip *s, const int32_t *h_seam, const int32_t *h_orient);
/* The path by itself on the host (the source k_strip_seam_path steps through), no device needed: cost [steps][states], each
 * entry at most 1 << 22, steps and states 1..1023 -> seam [steps], *total.  Anything else: UWIP_ERR_INVALID, nothing is
 * written. */
int uwip_strip_seam_path_host(const uint32_t *cost, int steps, int states, int32_t *seam, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif /* UWIP_H */
