// uwip.hpp -- C++ host shim over the C ABI (include/uwip.h) with the reference's own
// function names and argument meaning, on a cv::Mat-shaped POD (uw::Mat).  When the
// reference is built against OpenCV, a cv::Mat maps onto uw::Mat field for field
// (data, step, rows, cols, channels); see INTEGRATION.md.  Host buffers go in and out;
// device staging is internal.  There is no CPU path: every call needs a HIP device.
//
//   modules/common/preprocessing.h:38,66,112,115   getHistogram, imgChannelStretch, numChannel, numSpace
//   modules/videostrip/include/videostrip.hpp:62-68,84,98,118   keyframe, calcOverlap, calcBlur, overlapArea
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "uwip.h"

namespace uw {

struct Mat {                      // the cv::Mat fields this path uses (8-bit, 1 or 3 channels, BGR)
    uint8_t *data = nullptr;
    size_t step = 0;
    int rows = 0, cols = 0, chans = 0;
    bool empty() const { return !data || rows <= 0 || cols <= 0; }
    int channels() const { return chans; }
};

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

class Context {
public:
    explicit Context(int device = 0)
    {
        int rc = uwip_ctx_create(device, nullptr, &ctx_);
        if (rc != UWIP_OK) throw Error(rc, "uwip_ctx_create failed: no HIP device (there is no CPU fallback)");
    }
    // a view of a context the caller owns (a program written against the C ABI that uses one of the classes below)
    explicit Context(uwip_ctx *borrowed) : ctx_(borrowed), owned_(false)
    {
        if (!borrowed) throw Error(UWIP_ERR_INVALID, "null context");
    }
    ~Context() { if (owned_) uwip_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    uwip_ctx *get() const { return ctx_; }
    void check(int rc) const { if (rc != UWIP_OK) throw Error(rc, uwip_last_error(ctx_)); }
    static int deviceCount() { int n = 0; uwip_device_count(&n); return n; }   // cuda::getCudaEnabledDeviceCount
private:
    uwip_ctx *ctx_ = nullptr;
    bool owned_ = true;
};

// The rank's copy engine (uwip_copier): upload / download of frame batches between page-locked host buffers and HBM on
// two lanes of their own, hand-overs by ticket (GpuMat::upload / download with a cuda::Stream around the timed region,
// histretch.cpp:165-216, for a stream of batches).  `after`: the copy starts once everything queued on that context's
// stream so far has finished.
class Copier {
public:
    explicit Copier(int device = 0)
    {
        int rc = uwip_copier_create(device, &c_);
        if (rc != UWIP_OK) throw Error(rc, "uwip_copier_create failed: no HIP device (there is no CPU fallback)");
    }
    ~Copier() { uwip_copier_destroy(c_); }
    Copier(const Copier &) = delete;
    Copier &operator=(const Copier &) = delete;
    uint64_t upload(void *d_dst, const void *h_src, size_t bytes, Context *after = nullptr)
    {
        uint64_t t = 0;
        check(uwip_copier_upload(c_, after ? after->get() : nullptr, d_dst, h_src, bytes, &t));
        return t;
    }
    uint64_t download(void *h_dst, const void *d_src, size_t bytes, Context *after = nullptr)
    {
        uint64_t t = 0;
        check(uwip_copier_download(c_, after ? after->get() : nullptr, h_dst, d_src, bytes, &t));
        return t;
    }
    void wait(uint64_t ticket) { check(uwip_copier_wait(c_, ticket)); }
    bool done(uint64_t ticket) { int d = 0; check(uwip_copier_query(c_, ticket, &d)); return d != 0; }
private:
    void check(int rc) const { if (rc != UWIP_OK) throw Error(rc, uwip_copier_last_error(c_)); }
    uwip_copier *c_ = nullptr;
};

// device copy of a host Mat (the role cv::cuda::GpuMat plays in the reference's CUDA branches)
class DeviceMat {
public:
    DeviceMat(Context &c, const Mat &m) : c_(c)
    {
        b_.rows = m.rows; b_.cols = m.cols; b_.channels = m.chans; b_.frames = 1;
        b_.step = (size_t)m.cols * m.chans;                      // packed on the device
        b_.frame_stride = b_.step * m.rows;
        c_.check(uwip_malloc(c_.get(), b_.frame_stride, &b_.data));
        upload(m);
    }
    DeviceMat(Context &c, int rows, int cols, int chans) : c_(c)
    {
        b_.rows = rows; b_.cols = cols; b_.channels = chans; b_.frames = 1;
        b_.step = (size_t)cols * chans; b_.frame_stride = b_.step * rows;
        c_.check(uwip_malloc(c_.get(), b_.frame_stride, &b_.data));
    }
    ~DeviceMat() { uwip_free(c_.get(), b_.data); }
    DeviceMat(const DeviceMat &) = delete;
    DeviceMat &operator=(const DeviceMat &) = delete;
    void upload(const Mat &m)                                     // GpuMat::upload
    {
        if (m.step == b_.step) c_.check(uwip_memcpy_h2d(c_.get(), b_.data, m.data, b_.frame_stride));
        else for (int y = 0; y < m.rows; ++y)
            c_.check(uwip_memcpy_h2d(c_.get(), (uint8_t *)b_.data + (size_t)y * b_.step, m.data + (size_t)y * m.step, b_.step));
    }
    void download(Mat &m) const                                   // GpuMat::download
    {
        if (m.step == b_.step) c_.check(uwip_memcpy_d2h(c_.get(), m.data, b_.data, b_.frame_stride));
        else for (int y = 0; y < m.rows; ++y)
            c_.check(uwip_memcpy_d2h(c_.get(), m.data + (size_t)y * m.step, (const uint8_t *)b_.data + (size_t)y * b_.step, b_.step));
    }
    const uwip_batch_u8 *batch() const { return &b_; }
private:
    Context &c_;
    uwip_batch_u8 b_{};
};

// ---- modules/common/preprocessing.h ---------------------------------------------------------
inline int numChannel(char c) { return uwip_numChannel(c); }
inline int numSpace(char c) { return uwip_numSpace(c); }

// void getHistogram(cv::Mat*, cv::Mat*): 256 float counts of an 8UC1 plane
inline void getHistogram(Context &c, const Mat &img, float hist[256])
{
    DeviceMat d(c, img);
    void *dh = nullptr;
    c.check(uwip_malloc(c.get(), sizeof(uint32_t) * 256 * img.chans, &dh));
    c.check(uwip_getHistogram(c.get(), d.batch(), (uint32_t *)dh));
    std::vector<uint32_t> h(256 * (size_t)img.chans);
    c.check(uwip_memcpy_d2h(c.get(), h.data(), dh, h.size() * 4));
    uwip_free(c.get(), dh);
    for (int i = 0; i < 256; ++i) hist[i] = (float)h[i];
}

// void imgChannelStretch(cv::Mat imgOriginal, cv::Mat imgStretched, int lo = 0, int hi = 100): in place
// (both Mats share pixels at every reference call site); `channel` picks the lane of a packed image.
inline void imgChannelStretch(Context &c, Mat imgOriginal, Mat imgStretched, int lowerPercentile = 0, int higherPercentile = 100,
                              int channel = 0)
{
    if (imgOriginal.data != imgStretched.data) throw Error(UWIP_ERR_INVALID, "imgStretched must share pixels with imgOriginal");
    DeviceMat d(c, imgOriginal);
    c.check(uwip_imgChannelStretch(c.get(), d.batch(), channel, lowerPercentile, higherPercentile));
    d.download(imgStretched);
}

// the per-letter loop of histretch.cpp:217-254 on a BGR image, in place
inline void histretch(Context &c, Mat src, const std::string &cChannel, int min_percent = 2, int max_percent = 98, bool fixed_order = false,
                      bool opencv32 = false)
{
    DeviceMat d(c, src);
    c.check(uwip_histretch_ex(c.get(), d.batch(), cChannel.c_str(), min_percent, max_percent,
                              (fixed_order ? UWIP_HISTRETCH_FIXED_ORDER : 0u) | (opencv32 ? UWIP_HISTRETCH_OPENCV32 : 0u)));
    d.download(src);
}

// ---- modules/videostrip/include/videostrip.hpp -------------------------------------------------
struct keyframe {                 // videostrip.hpp:62-68 (keypoints/descriptors live in a device feature slot)
    bool new_img = true;
    Mat img;                      // reference frame (full resolution; the 640-wide resize happens inside)
    uwip_features *feats = nullptr;
};

class Videostrip {
public:
    int videoWidth = 0, videoHeight = 0;          // the reference's globals (main.cpp:45-46)
    unsigned match_flags = 0;                     // 0 = the reference's ">= 4 good matches" rule (videostrip.cpp:252-272); UWIP_OVERLAP_MIN6 = >= 6 inliers
    unsigned detect_flags = 0;                    // 0 = fixed detector threshold (SURF::create(400) is fixed, videostrip.cpp:206); UWIP_OVERLAP_RELATIVE_THRESHOLD
    explicit Videostrip(Context &c) : c_(c)
    {
        c_.check(uwip_features_create(c_.get(), 1, &obj_));
        c_.check(uwip_malloc(c_.get(), 128, &scratch_));
    }
    ~Videostrip() { uwip_features_destroy(obj_); uwip_free(c_.get(), scratch_); }
    void initKeyframe(keyframe &k) { if (!k.feats) c_.check(uwip_features_create(c_.get(), 1, &k.feats)); }
    static void releaseKeyframe(keyframe &k) { uwip_features_destroy(k.feats); k.feats = nullptr; }

    // float calcOverlap(keyframe* kframe, Mat img_object): -1 on empty input, -2.0 when no homography
    float calcOverlap(keyframe *kframe, const Mat &img_object, uint32_t seed = 1)
    {
        if (img_object.empty() || kframe->img.empty()) { std::printf(" --(!) Error reading images \n"); return -1.f; }
        initKeyframe(*kframe);
        if (kframe->new_img) {
            DeviceMat k(c_, kframe->img);
            c_.check(uwip_overlap_detect_ex(c_.get(), k.batch(), kframe->feats, 0, detect_flags));
            kframe->new_img = false;
        }
        DeviceMat o(c_, img_object);
        c_.check(uwip_overlap_detect_ex(c_.get(), o.batch(), obj_, 0, detect_flags));
        int32_t q = 0, t = 0;
        c_.check(uwip_overlap_match_ex(c_.get(), obj_, kframe->feats, &q, &t, 1, videoWidth, videoHeight, seed, match_flags,
                                       (float *)scratch_, nullptr, nullptr, nullptr, nullptr));
        float r = 0.f;
        c_.check(uwip_memcpy_d2h(c_.get(), &r, scratch_, 4));
        if (r == -2.0f) std::printf("[WARN] Not enough good matches!\n");
        return r;
    }
    // cv::resize(frame, res_frame, cv::Size(), hResizeFactor, hResizeFactor), main.cpp:242,287,311: `res` receives the
    // 640-wide BGR frame (its buffer is (re)allocated into `store`)
    void resize(const Mat &frame, Mat &res, std::vector<uint8_t> &store)
    {
        int oh = 0, ow = 0;
        c_.check(uwip_overlap_working_size(frame.rows, frame.cols, &oh, &ow));
        store.resize((size_t)oh * ow * 3);
        res.data = store.data(); res.rows = oh; res.cols = ow; res.chans = 3; res.step = (size_t)ow * 3;
        DeviceMat s(c_, frame), d(c_, oh, ow, 3);
        c_.check(uwip_resize_bgr(c_.get(), s.batch(), d.batch()));
        d.download(res);
    }
    // float calcBlur(Mat frame): frame = the resized BGR frame (main.cpp:338,355)
    float calcBlur(const Mat &frame)
    {
        DeviceMat d(c_, frame);
        c_.check(uwip_calcBlur(c_.get(), d.batch(), (float *)scratch_));
        float r = 0.f;
        c_.check(uwip_memcpy_d2h(c_.get(), &r, scratch_, 4));
        return r;
    }
    // float overlapArea(Mat H): H row-major 3x3 doubles
    float overlapArea(const double H[9])
    {
        double *dH = (double *)((uint8_t *)scratch_ + 16);
        c_.check(uwip_memcpy_h2d(c_.get(), dH, H, sizeof(double) * 9));
        c_.check(uwip_overlapArea(c_.get(), dH, 1, videoWidth, videoHeight, (float *)scratch_, nullptr));
        float r = 0.f;
        c_.check(uwip_memcpy_d2h(c_.get(), &r, scratch_, 4));
        return r;
    }
private:
    Context &c_;
    uwip_features *obj_ = nullptr;
    void *scratch_ = nullptr;
};

// ---- the strip mosaic of the key frames (uwip_strip, include/uwip.h) ---------------------------------------------------
// add() takes each key frame where main.cpp:294,377 writes it; layout() chains the homographies of videostrip.cpp:270 and
// returns the segments; render() gives one segment's canvas (`store` receives its pixels, as Videostrip::resize's does).
class Strip {
public:
    // rows x cols: the full-resolution key frames; match_flags / detect_flags as Videostrip's
    Strip(Context &c, int rows, int cols, int max_frames = 1024, unsigned detect_flags = 0, unsigned match_flags = 0) : c_(c)
    {
        uwip_strip_config cfg;
        c_.check(uwip_strip_config_default(&cfg, rows, cols));
        cfg.batch = 1; cfg.max_frames = max_frames; cfg.detect_flags = detect_flags; cfg.match_flags = match_flags;
        c_.check(uwip_strip_create(c_.get(), &cfg, &s_));
    }
    ~Strip() { uwip_strip_destroy(s_); }
    Strip(const Strip &) = delete;
    Strip &operator=(const Strip &) = delete;
    uwip_strip *get() const { return s_; }
    int count() const { int n = 0; check(uwip_strip_count(s_, &n)); return n; }
    void add(const Mat &frame)
    {
        DeviceMat d(c_, frame);
        check(uwip_strip_add(s_, d.batch(), nullptr, nullptr));
        c_.check(uwip_sync(c_.get()));                            // the device copy of the frame goes with this scope
    }
    std::vector<uwip_strip_segment> layout()
    {
        std::vector<uwip_strip_segment> segs, part(64);
        for (int n = 64; n == 64;) {
            check(uwip_strip_layout(s_, part.data(), 64, &n));
            segs.insert(segs.end(), part.begin(), part.begin() + n);
        }
        segs_ = segs;
        return segs;
    }
    // after layout(): one gain per frame and channel from the overlaps of consecutive frames (cfg: null = the defaults);
    // an add or a new layout drops them
    void gains(const uwip_strip_gain_config *cfg = nullptr) { check(uwip_strip_gains(s_, cfg)); }
    // the gains in 1/4096 [count][3]; g (the solution before it is quantised) and stats [count][7] when asked for
    std::vector<int32_t> gain_values(std::vector<double> *g = nullptr, std::vector<uint64_t> *stats = nullptr)
    {
        const size_t n = (size_t)count();
        std::vector<int32_t> gq(3 * n);
        if (g) g->resize(3 * n);
        if (stats) stats->resize(7 * n);
        check(uwip_strip_gain_values(s_, gq.data(), g ? g->data() : nullptr, stats ? stats->data() : nullptr));
        return gq;
    }
    void set_gains(const std::vector<int32_t> &gq)
    {
        if (gq.size() != 3 * (size_t)count()) throw Error(UWIP_ERR_INVALID, "Strip::set_gains: [count][3] gains");
        check(uwip_strip_set_gains(s_, gq.data()));
    }
    // the stacks of every frame added so far, for UWIP_STRIP_MULTIBAND (cfg: null = 4 levels, ramps 1, 2, 4, 8); an add drops them
    void bands(const uwip_strip_bands_config *cfg = nullptr) { check(uwip_strip_bands(s_, cfg)); }
    // after layout() (and gains(), when the costs are to use them): the seam of every frame against the one before it, for
    // UWIP_STRIP_SEAM (cfg: null = prior 1024); an add, a new layout and new gains drop them
    void seams(const uwip_strip_seam_config *cfg = nullptr) { check(uwip_strip_seams(s_, cfg)); }
    // level 1..levels of a frame's stack: rows x cols x 3 bytes of the stored geometry (the caller sizes `out`)
    void band_level(int frame, int level, uint8_t *out) { check(uwip_strip_band_level(s_, frame, level, out)); }
    // one segment of the last layout(); mode = UWIP_STRIP_FEATHER / FIRST / LAST, MULTIBAND after bands() or SEAM after seams(),
    // | UWIP_STRIP_GAIN after gains() / set_gains()
    void render(int segment, int mode, Mat &out, std::vector<uint8_t> &store)
    {
        if (segment < 0 || segment >= (int)segs_.size()) throw Error(UWIP_ERR_INVALID, "Strip::render: no such segment (layout() first)");
        const uwip_strip_segment &g = segs_[segment];
        store.resize((size_t)g.rows * g.cols * 3);
        out.data = store.data(); out.rows = g.rows; out.cols = g.cols; out.chans = 3; out.step = (size_t)g.cols * 3;
        DeviceMat d(c_, g.rows, g.cols, 3);
        check(uwip_strip_render(s_, segment, mode, nullptr, d.batch(), nullptr));
        d.download(out);
    }
private:
    void check(int rc) const { if (rc != UWIP_OK) throw Error(rc, uwip_strip_last_error(s_)); }
    Context &c_;
    uwip_strip *s_ = nullptr;
    std::vector<uwip_strip_segment> segs_;
};

// ---- cv::imwrite(".jpg") / cv::imencode(".jpg") on the device ------------------------------------------------------
// One baseline JPEG stream per frame of a device batch (uwip_jpeg_encode_host), byte for byte what the CLIs' host codec
// writes.  The slot is the frame's raw size and grows to uwip_jpeg_bound for the rare batch with a frame that outgrows it.
inline std::vector<std::vector<uint8_t>> imencode_jpeg(Context &c, const uwip_batch_u8 &frames, int quality = 95)
{
    const size_t F = (size_t)(frames.frames > 0 ? frames.frames : 0);
    std::vector<std::vector<uint8_t>> out(F);
    if (!F) return out;
    size_t slot = (size_t)frames.rows * frames.cols * frames.channels + 1024;
    std::vector<uint8_t> buf;
    std::vector<int64_t> sizes(F);
    for (int attempt = 0; attempt < 2; ++attempt) {
        buf.resize(F * slot);
        c.check(uwip_jpeg_encode_host(c.get(), &frames, quality, buf.data(), slot, sizes.data()));
        bool fits = true;
        for (int64_t s : sizes) fits = fits && s >= 0;
        if (fits) break;
        if (attempt) throw Error(UWIP_ERR_INVALID, "uwip_jpeg_encode_host: a stream exceeds uwip_jpeg_bound");
        slot = uwip_jpeg_bound(frames.rows, frames.cols, frames.channels);
    }
    for (size_t f = 0; f < F; ++f) out[f].assign(buf.begin() + f * slot, buf.begin() + f * slot + (size_t)sizes[f]);
    return out;
}
inline std::vector<std::vector<uint8_t>> imencode_jpeg(Context &c, const DeviceMat &m, int quality = 95)
{
    return imencode_jpeg(c, *m.batch(), quality);
}

// ---- cv::imwrite(".png") / cv::imencode(".png") on the device ------------------------------------------------------
// One PNG stream per frame of a device batch (uwip_png_encode_host): lossless, filter -1 = the adaptive choice per row.  The
// slot is the frame's raw size and grows to uwip_png_bound for the rare batch with a frame that outgrows it (noise).
inline std::vector<std::vector<uint8_t>> imencode_png(Context &c, const uwip_batch_u8 &frames, int filter = -1)
{
    const size_t F = (size_t)(frames.frames > 0 ? frames.frames : 0);
    std::vector<std::vector<uint8_t>> out(F);
    if (F == 0) return out;
    size_t slot = (size_t)frames.rows * frames.cols * frames.channels + 1024;
    std::vector<uint8_t> buf;
    std::vector<int64_t> sizes(F);
    for (int attempt = 0; attempt < 2; ++attempt) {
        buf.resize(F * slot);
        c.check(uwip_png_encode_host(c.get(), &frames, filter, buf.data(), slot, sizes.data()));
        bool fits = true;
        for (int64_t s : sizes) fits = fits && s >= 0;
        if (fits) break;
        if (attempt) throw Error(UWIP_ERR_INVALID, "uwip_png_encode_host: a stream exceeds uwip_png_bound");
        slot = uwip_png_bound(frames.rows, frames.cols, frames.channels);
    }
    for (size_t f = 0; f < F; ++f) out[f].assign(buf.begin() + f * slot, buf.begin() + f * slot + (size_t)sizes[f]);
    return out;
}
inline std::vector<std::vector<uint8_t>> imencode_png(Context &c, const DeviceMat &m, int filter = -1)
{
    return imencode_png(c, *m.batch(), filter);
}

// ---- cv::imdecode of JPEG streams on the device -------------------------------------------------------------------------
// One frame of the device batch `out` per baseline JPEG / Motion-JPEG stream (uwip_jpeg_decode_host): where the returned
// status is 0, the pixels of the CLIs' host decoder byte for byte; a negative status (UWIP_JPEG_BAD_STREAM / _SIZE_MISMATCH /
// _HOST_ONLY) leaves the other frames complete -- decode such a frame on the host and upload it into its slot.
inline std::vector<int32_t> imdecode_jpeg(Context &c, const std::vector<const uint8_t *> &streams, const std::vector<size_t> &sizes,
                                          const uwip_batch_u8 &out, int sync_rounds = -1)
{
    if (streams.size() != sizes.size()) throw Error(UWIP_ERR_INVALID, "imdecode_jpeg: one size per stream");
    std::vector<int32_t> status(streams.size(), 0);
    if (streams.empty()) return status;
    uwip_jpeg_decode_opts opts{};
    opts.sync_rounds = sync_rounds;
    c.check(uwip_jpeg_decode_host(c.get(), streams.data(), sizes.data(), (int)streams.size(), &out, &opts, status.data()));
    return status;
}
inline std::vector<int32_t> imdecode_jpeg(Context &c, const std::vector<std::vector<uint8_t>> &streams, const uwip_batch_u8 &out,
                                          int sync_rounds = -1)
{
    std::vector<const uint8_t *> p;
    std::vector<size_t> n;
    for (const auto &s : streams) { p.push_back(s.data()); n.push_back(s.size()); }
    return imdecode_jpeg(c, p, n, out, sync_rounds);
}

// ---- the reference's own signatures, on a process-wide default context -------------------------------------
// A call site of the reference switches by name alone (the `...GPU` twins of preprocessing.h:96 /
// videostrip.hpp:84-118 are the precedent): same names, same argument order and defaults, the same globals
// (videoWidth / videoHeight / hResizeFactor, main.cpp:45-49), cv::Mat replaced by the field-compatible uw::Mat.
// Single-threaded, device 0, like the reference.
namespace ref {
inline Context &defaultContext() { static Context c(0); return c; }
inline Videostrip &defaultVideostrip() { static Videostrip v(defaultContext()); return v; }
inline int videoWidth = 0, videoHeight = 0;
inline float hResizeFactor = 1.f;

inline int numChannel(char c) { return uwip_numChannel(c); }                         // preprocessing.h:112
inline int numSpace(char c) { return uwip_numSpace(c); }                             // preprocessing.h:115
// void getHistogram(cv::Mat *imgOriginal, cv::Mat *histogram): the 256 x 1 CV_32F histogram as float[256]
inline void getHistogram(Mat *imgOriginal, float histogram[256]) { uw::getHistogram(defaultContext(), *imgOriginal, histogram); }
// void imgChannelStretch(cv::Mat imgOriginal, cv::Mat imgStretched, int lowerPercentile = 0, int higherPercentile = 100)
inline void imgChannelStretch(Mat imgOriginal, Mat imgStretched, int lowerPercentile = 0, int higherPercentile = 100)
{
    uw::imgChannelStretch(defaultContext(), imgOriginal, imgStretched, lowerPercentile, higherPercentile, 0);
}
inline void imgChannelStretchGPU(Mat imgOriginal, Mat imgStretched, int lowerPercentile = 0, int higherPercentile = 100)
{
    imgChannelStretch(imgOriginal, imgStretched, lowerPercentile, higherPercentile);
}
// float calcOverlap(keyframe *kframe, cv::Mat img_object) / float calcBlur(cv::Mat frame) / float overlapArea(cv::Mat H)
inline float calcOverlap(keyframe *kframe, Mat img_object)
{
    Videostrip &v = defaultVideostrip();
    v.videoWidth = videoWidth; v.videoHeight = videoHeight;
    return v.calcOverlap(kframe, img_object);
}
inline float calcOverlapGPU(keyframe *kframe, Mat img_object) { return calcOverlap(kframe, img_object); }
inline float calcBlur(Mat frame) { return defaultVideostrip().calcBlur(frame); }
inline float calcBlurGPU(Mat frame) { return calcBlur(frame); }
inline float overlapArea(const double H[9])
{
    Videostrip &v = defaultVideostrip();
    v.videoWidth = videoWidth; v.videoHeight = videoHeight;
    return v.overlapArea(H);
}
}  // namespace ref

}  // namespace uw
