// uwip_pipe: the per-frame chain  bgdehaze -> histretch -> aclahe -> videostrip-overlap  as one object over the C ABI
// (include/uwip.h, "the whole per-frame chain").  The reference runs the four tools back to back over files:
// modules/bgdehaze/main.py:14-20, modules/histretch/src/histretch.cpp:217-254, modules/aclahe/src/aclahe.cpp:152-218 with
// python/ACLAHE.py:9-129 + python/main.py:19-20, modules/videostrip/src/main.cpp:300-394.  Everything here is host code that
// calls the library's own entry points; what it adds is the state the chain carries between steps (rounds 1-4 kept that in
// Python, uwimageproc_amd/pipeline.py): the feature-slot carry, the throttle, the double-buffered host front end.
#include "uwip_internal.hpp"
#include "pipe_streams.hpp"
#include <cstring>
#include <deque>

struct uwip_pipe {
    uwip_ctx *ctx = nullptr;
    uwip_pipe_config cfg{};
    std::string err;
    size_t frame_bytes = 0, plane_bytes = 0;
    uint8_t *v = nullptr, *v_out = nullptr;            // [F][H][W]: V of the stretched frames, and its CLAHE
    uwip_features *feats = nullptr;                    // slot 0 = the previous batch's last frame, 1..F = this batch
    bool have_prev = false;
    std::vector<int32_t> pair_q, pair_t;
    // resident form: events of the steps still queued
    std::deque<hipEvent_t> inflight;
    std::vector<hipEvent_t> ev_pool;
    // host-buffer form
    uwip_copier *copier = nullptr;
    bool own_copier = false;
    uint8_t *staging = nullptr;
    bool own_staging = false;
    uint8_t *src[2] = {nullptr, nullptr}, *work[2] = {nullptr, nullptr};
    float *ratio[2] = {nullptr, nullptr};
    int32_t *info[2] = {nullptr, nullptr};
    uint64_t t_up[2] = {0, 0}, t_dn[2] = {0, 0}, t_rt[2] = {0, 0};
    uint64_t k = 0;
    const void *pending = nullptr;                     // host buffer whose upload into src[k % 2] has been requested
    // most recent step's results (uwip_pipe_device_results)
    const uint8_t *last_frames = nullptr;
    const float *last_ratio = nullptr;
    const int32_t *last_info = nullptr;
    int eos_valid = -1;                                // uwip_pipe_end_of_stream: the next step is the last, with this many frames
    // key-frame mode (uwip_pipe_keyframe_chain; kf_chain.hpp): one device block holds everything the chain carries
    struct Keyframe {
        bool on = false;
        uwip_keyframe_config kc{};
        int R = 0, P0 = 0, oh = 0, ow = 0;
        bool started = false;                          // the stream's frame 0 has been seen (host's view)
        int32_t base = 0;                              // stream index of the next step's frame 0
        uint32_t consumed = 0;                         // rows handed out by uwip_pipe_keyframes
        uint8_t *block = nullptr;
        uwip_kf::State *state = nullptr;
        int32_t *fb_key = nullptr, *fb_start = nullptr, *fb_list = nullptr, *fb_n = nullptr, *r0 = nullptr;
        float *out_ratio = nullptr, *blur = nullptr;
        int32_t *out_info = nullptr, *midx = nullptr, *mdist = nullptr;
        uwip_keyframe_row *ring = nullptr;
        uint8_t *res = nullptr;                        // the batch at the working size (calcBlur's input, main.cpp:311)
    } kf;
    // compressed frames in, compressed (key) frames out (uwip_pipe_streams; pipe_streams.hip)
    struct Streams {
        bool on = false;
        uwip_pipe_streams_config sc{};
        size_t slot_bytes = 0, one_frame = 0, table_bytes = 0;
        int32_t base = 0;                              // predecessor mode: stream index of the next step's frame 0
        uint64_t k = 0;                                // steps taken; ticket = step number, 1-based
        uint8_t *block = nullptr;                      // one device allocation for everything below
        uint8_t *src = nullptr, *work = nullptr;       // [F] decoded / enhanced frames
        uint8_t *carried = nullptr, *compact = nullptr;// one frame; [F + 1] frames
        uint8_t *slots = nullptr;                      // [F + 1][slot_bytes]
        int64_t *sizes = nullptr;                      // [F + 1]
        int32_t *status = nullptr, *sel_n = nullptr;
        uint32_t *emitted = nullptr;                   // rows of the walker's ring already handed out
        float *ratio = nullptr;
        uwip_ps::Sel *sel = nullptr;
        std::vector<uint8_t *> table, blob;            // [depth] device
        std::vector<uint8_t *> h_table;                // [depth] page-locked host
        std::vector<uint64_t> t_table, ticket;         // [depth] the table's download; the step whose result the slot holds (0: free)
        std::vector<std::vector<int32_t>> h_par;       // [depth] the step's (BS, CL) where the host made the choice (else empty)
    } st;

    int fail(int code, const char *what)
    {
        err = what;
        return code;
    }
    int from_ctx(int rc)
    {
        if (rc) err = ctx->err;
        return rc;
    }
};

namespace {

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool cfg_ok(const uwip_pipe_config &c)
{
    return c.frames >= 1 && c.rows >= 1 && c.cols >= 1 && c.max_in_flight >= 1 && c.videoWidth >= 0 && c.videoHeight >= 0 &&
           std::memchr(c.letters, 0, sizeof c.letters) != nullptr && (uint64_t)c.rows * (uint64_t)c.cols < (1ull << 31);
}

uwip_batch_u8 batch_of(void *data, const uwip_pipe_config &c, int channels, int frames = -1)
{
    uwip_batch_u8 b;
    b.data = data;
    b.step = (size_t)c.cols * channels;
    b.frame_stride = b.step * c.rows;
    b.rows = c.rows; b.cols = c.cols; b.channels = channels;
    b.frames = frames < 0 ? c.frames : frames;
    return b;
}

int check_io(uwip_pipe *p, const uwip_batch_u8 *b, const char *what)
{
    if (!b || b->rows != p->cfg.rows || b->cols != p->cfg.cols || b->frames != p->cfg.frames || b->channels != 3 || !b->data)
        return p->fail(UWIP_ERR_INVALID, what);
    return UWIP_OK;
}

int run_keyframe(uwip_pipe *p, const uwip_batch_u8 *out, float *d_ratio, int32_t *d_info);

// the chain itself (pipeline stage definitions: uwip.h)
int run_stages(uwip_pipe *p, unsigned stages, const uwip_batch_u8 *in, const uwip_batch_u8 *out, float *d_ratio, int32_t *d_info)
{
    uwip_ctx *ctx = p->ctx;
    const uwip_pipe_config &c = p->cfg;
    int rc = UWIP_OK;
    if ((stages & UWIP_PIPE_DEHAZE) && (stages & UWIP_PIPE_HISTRETCH))
        // chained: the kernel that writes the dehazed bytes hands the stretch its histogram
        rc = uwip_dehaze_histretch(ctx, in, out, c.w, (int)c.dehaze_flags, c.letters, c.lo, c.hi, c.histretch_flags);
    else if (stages & UWIP_PIPE_DEHAZE)
        rc = uwip_dehaze(ctx, in, out, c.w, (int)c.dehaze_flags, nullptr, nullptr, nullptr);
    else if (stages & UWIP_PIPE_HISTRETCH)
        rc = uwip_histretch_ex(ctx, out, c.letters, c.lo, c.hi, c.histretch_flags);
    if (rc) return p->from_ctx(rc);
    if (stages & UWIP_PIPE_ACLAHE) {
        const uwip_batch_u8 vb = batch_of(p->v, c, 1), ob = batch_of(p->v_out, c, 1);
        // V of HSV (aclahe.cpp:152-154) -> sweep, parameter choice, final CLAHE (ACLAHE.py:9-129, python/main.py:19-20) ->
        // back to BGR (the stub of aclahe.cpp:216)
        if ((rc = uwip_bgr_to_v(ctx, out, &vb))) return p->from_ctx(rc);
        if ((rc = uwip_aclahe_auto_ex(ctx, &vb, &ob, c.residual_rule, c.aclahe_flags, nullptr, nullptr))) return p->from_ctx(rc);
        if ((rc = uwip_hsv_replace_v(ctx, out, &ob, out))) return p->from_ctx(rc);
    }
    if (stages & UWIP_PIPE_OVERLAP) {
        if (!d_ratio) return p->fail(UWIP_ERR_INVALID, "the overlap stage needs d_ratio");
        if (p->kf.on) return run_keyframe(p, out, d_ratio, d_info);
        if (!p->have_prev) {
            // first batch: frame 0 is its own key frame (main.cpp:284-297 takes the first frame as key frame)
            uwip_batch_u8 first = *out;
            first.frames = 1;
            if ((rc = uwip_overlap_detect_ex(ctx, &first, p->feats, 0, c.detect_flags))) return p->from_ctx(rc);
            p->have_prev = true;
        } else {
            // the previous batch's last frame becomes the key frame of this batch's first frame (kframe's cached
            // keypoints / descriptors, videostrip.hpp:62-68)
            if ((rc = uwip_features_copy(ctx, p->feats, c.frames, p->feats, 0))) return p->from_ctx(rc);
        }
        if ((rc = uwip_overlap_detect_ex(ctx, out, p->feats, 1, c.detect_flags))) return p->from_ctx(rc);
        rc = uwip_overlap_match_ex(ctx, p->feats, p->feats, p->pair_q.data(), p->pair_t.data(), c.frames,
                                   c.videoWidth ? c.videoWidth : c.cols, c.videoHeight ? c.videoHeight : c.rows, c.seed, c.match_flags,
                                   d_ratio, d_info, nullptr, nullptr, nullptr);
        if (rc) return p->from_ctx(rc);
        if (p->eos_valid >= 0) { p->have_prev = false; p->eos_valid = -1; }
    }
    return UWIP_OK;
}

// The overlap stage in key-frame mode (kf_chain.hpp): detect into slots 1..F, blur, round 0's fixed pair list, then R
// rounds of (walker, matcher on the list the walker wrote), the last walker call, and the carry of the key / window
// candidate into slots 0 / F + 1.  Every count and slot index past round 0 is read on the device: nothing here waits.
int run_keyframe(uwip_pipe *p, const uwip_batch_u8 *out, float *d_ratio, int32_t *d_info)
{
    uwip_ctx *ctx = p->ctx;
    const uwip_pipe_config &c = p->cfg;
    uwip_pipe::Keyframe &k = p->kf;
    const int F = c.frames;
    const int vw = c.videoWidth ? c.videoWidth : c.cols, vh = c.videoHeight ? c.videoHeight : c.rows;
    int rc;
    if ((rc = uwip_overlap_detect_ex(ctx, out, p->feats, 1, c.detect_flags))) return p->from_ctx(rc);
    // the stream's frame 0 is the first key frame (main.cpp:284-297): slot 0 holds the key at the start of a step
    if (!k.started && (rc = uwip_features_copy(ctx, p->feats, 1, p->feats, 0))) return p->from_ctx(rc);
    // calcBlur(res_frame), main.cpp:311,338,355
    uwip_batch_u8 rb;
    rb.data = k.res; rb.step = (size_t)k.ow * 3; rb.frame_stride = rb.step * k.oh;
    rb.rows = k.oh; rb.cols = k.ow; rb.channels = 3; rb.frames = F;
    if ((rc = uwip_resize_bgr(ctx, out, &rb)) || (rc = uwip_calcBlur(ctx, &rb, k.blur))) return p->from_ctx(rc);
    if ((rc = uwip_overlap_match_dev(ctx, p->feats, k.r0, k.r0 + k.P0, nullptr, k.P0, vw, vh, c.seed, c.match_flags, k.out_ratio,
                                     k.out_info, k.midx, k.mdist)))
        return p->from_ctx(rc);
    const bool last = p->eos_valid >= 0;
    uwip_kf::Batch b;
    b.F = F; b.D = k.kc.lookback; b.kWindow = k.kc.kWindow; b.valid = last ? p->eos_valid : F; b.base = k.base;
    b.rounds = k.R; b.max_rows = k.kc.max_rows; b.minOverlap = k.kc.minOverlap; b.first = k.started ? 0 : 1; b.last = last ? 1 : 0;
    uwip_kf::Bufs u;
    u.out_ratio = k.out_ratio; u.out_info = k.out_info; u.blur = k.blur; u.ratio = d_ratio; u.info = d_info; u.ring = k.ring;
    u.fb_key = k.fb_key; u.fb_start = k.fb_start; u.fb_q = k.fb_list; u.fb_t = k.fb_list + F; u.fb_n = k.fb_n;
    if ((rc = uwip_kf_walk(ctx, b, k.state, u, 0))) return p->from_ctx(rc);
    for (int r = 1; r <= k.R; ++r) {
        const size_t at = (size_t)k.P0 + (size_t)(r - 1) * F;
        if ((rc = uwip_overlap_match_dev(ctx, p->feats, u.fb_q, u.fb_t, k.fb_n, F, vw, vh, c.seed, c.match_flags, k.out_ratio + at,
                                         k.out_info + 8 * at, k.midx, k.mdist)))
            return p->from_ctx(rc);
        if ((rc = uwip_kf_walk(ctx, b, k.state, u, r))) return p->from_ctx(rc);
    }
    if ((rc = uwip_features_copy_dev(ctx, p->feats, &k.state->carry_key, 0, F + 1))) return p->from_ctx(rc);
    k.started = true;
    k.base += F;
    if (last) { k.started = false; k.base = 0; p->eos_valid = -1; }
    return UWIP_OK;
}

void kf_free(uwip_pipe *p)
{
    uwip_free(p->ctx, p->kf.block);
    p->kf = uwip_pipe::Keyframe();
}

void st_free(uwip_pipe *p)
{
    uwip_free(p->ctx, p->st.block);
    for (uint8_t *h : p->st.h_table) uwip_host_free(p->ctx, h);
    p->st = uwip_pipe::Streams();
}

int ensure_copier(uwip_pipe *p)
{
    if (p->copier) return UWIP_OK;
    int rc = uwip_copier_create(p->ctx->device, &p->copier);
    if (rc) return p->fail(rc, "uwip_copier_create failed");
    p->own_copier = true;
    return UWIP_OK;
}

// Nothing in a step waits on the host, so a caller that loops would queue steps without bound and end up spinning inside
// the runtime once its hardware queue is full: the wait for the oldest queued step polls its event and sleeps in between.
int throttle_wait(uwip_pipe *p)
{
    while ((int)p->inflight.size() >= p->cfg.max_in_flight) {
        hipEvent_t e = p->inflight.front();
        const hipError_t he = uwip_event_wait(e, 1000);
        if (he != hipSuccess) return p->fail(UWIP_ERR_HIP, hipGetErrorString(he));
        p->inflight.pop_front();
        p->ev_pool.push_back(e);
    }
    return UWIP_OK;
}

int throttle_record(uwip_pipe *p)
{
    hipEvent_t e = nullptr;
    if (!p->ev_pool.empty()) { e = p->ev_pool.back(); p->ev_pool.pop_back(); }
    else if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return p->fail(UWIP_ERR_HIP, "hipEventCreate");
    if (hipEventRecord(e, p->ctx->stream) != hipSuccess) { p->ev_pool.push_back(e); return p->fail(UWIP_ERR_HIP, "hipEventRecord"); }
    p->inflight.push_back(e);
    return UWIP_OK;
}

int ensure_host_state(uwip_pipe *p)
{
    const uwip_pipe_config &c = p->cfg;
    if (int rc = ensure_copier(p)) return rc;
    if (!p->src[0]) {
        uint8_t *base = (uint8_t *)c.d_staging;
        if (!base) {
            void *d = nullptr;
            int rc = uwip_malloc(p->ctx, uwip_pipe_staging_bytes(&c), &d);
            if (rc) return p->from_ctx(rc);
            p->staging = base = (uint8_t *)d;
            p->own_staging = true;
        }
        const size_t fb = p->frame_bytes;
        p->src[0] = base; p->src[1] = base + fb; p->work[0] = base + 2 * fb; p->work[1] = base + 3 * fb;
        uint8_t *r = base + align256(4 * fb);
        p->ratio[0] = (float *)r; p->ratio[1] = (float *)r + c.frames;
        uint8_t *i = r + align256(2 * sizeof(float) * (size_t)c.frames);
        p->info[0] = (int32_t *)i; p->info[1] = (int32_t *)i + 8 * (size_t)c.frames;
    }
    return UWIP_OK;
}

int copier_rc(uwip_pipe *p, int rc)
{
    if (rc) p->err = std::string("copier: ") + uwip_copier_last_error(p->copier);
    return rc;
}

}  // namespace

UWIP_API int uwip_pipe_config_default(uwip_pipe_config *cfg, int frames, int rows, int cols)
{
    if (!cfg) return UWIP_ERR_INVALID;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->frames = frames; cfg->rows = rows; cfg->cols = cols;
    std::strcpy(cfg->letters, "RGB");                   // histretch -c=RGB (histretch.cpp:154)
    cfg->lo = 2; cfg->hi = 98;                          // histretch.cpp:154,236,247
    cfg->w = 15;                                        // main.py:28-29
    cfg->dehaze_flags = UWIP_DEHAZE_FULL;               // adaptiveExp_map as written: S unguarded (BGDehaze.py:83)
    cfg->histretch_flags = 0;
    cfg->residual_rule = 0;                             // OpenCV 3.4.x (INSTALL.md:47-63)
    cfg->aclahe_flags = UWIP_ACLAHE_PREFILTER | UWIP_ACLAHE_ASYNC;     // ParametrosACLAHE (ACLAHE.py:15), no host wait
    cfg->detect_flags = 0;
    cfg->match_flags = 0;                               // >= 4 good matches (videostrip.cpp:252-272)
    cfg->videoWidth = 0; cfg->videoHeight = 0;          // = cols, rows (main.cpp:238-239)
    cfg->seed = 1;
    cfg->max_in_flight = 2;
    cfg->d_staging = nullptr;
    return UWIP_OK;
}

UWIP_API size_t uwip_pipe_staging_bytes(const uwip_pipe_config *cfg)
{
    if (!cfg || !cfg_ok(*cfg)) return 0;
    const size_t fb = (size_t)cfg->frames * cfg->rows * cfg->cols * 3;
    return align256(4 * fb) + align256(2 * sizeof(float) * (size_t)cfg->frames) + align256(2 * 8 * sizeof(int32_t) * (size_t)cfg->frames);
}

UWIP_API int uwip_pipe_create(uwip_ctx *ctx, const uwip_pipe_config *cfg, uwip_copier *copier, uwip_pipe **out)
{
    if (!out) return UWIP_ERR_INVALID;
    *out = nullptr;
    if (int rc_e = uwip_enter(ctx)) return rc_e;
    UWIP_REQUIRE(ctx, cfg && cfg_ok(*cfg), "bad pipe configuration");
    UWIP_REQUIRE(ctx, (cfg->aclahe_flags & ~(unsigned)(UWIP_ACLAHE_PREFILTER | UWIP_ACLAHE_HOST_SELECT | UWIP_ACLAHE_ASYNC)) == 0 &&
                          (cfg->dehaze_flags & ~(unsigned)(UWIP_DEHAZE_FULL | UWIP_DEHAZE_GUARD_S)) == 0, "unknown stage flag");
    uwip_pipe *p = new (std::nothrow) uwip_pipe;
    if (!p) return ctx->fail(UWIP_ERR_NOMEM, "uwip_pipe");
    p->ctx = ctx;
    p->cfg = *cfg;
    p->copier = copier;
    p->plane_bytes = (size_t)cfg->frames * cfg->rows * cfg->cols;
    p->frame_bytes = p->plane_bytes * 3;
    void *d = nullptr;
    int rc = uwip_malloc(ctx, 2 * p->plane_bytes, &d);
    if (!rc) {
        p->v = (uint8_t *)d;
        p->v_out = p->v + p->plane_bytes;
        rc = uwip_features_create(ctx, cfg->frames + 1, &p->feats);
    }
    if (rc) {
        uwip_free(ctx, p->v);
        delete p;
        return rc;
    }
    p->pair_q.resize(cfg->frames);
    p->pair_t.resize(cfg->frames);
    for (int i = 0; i < cfg->frames; ++i) { p->pair_q[i] = i + 1; p->pair_t[i] = i; }
    *out = p;
    return UWIP_OK;
}

UWIP_API int uwip_pipe_sync(uwip_pipe *p)
{
    if (!p) return UWIP_ERR_INVALID;
    int rc = uwip_sync(p->ctx);
    if (rc) return p->from_ctx(rc);
    for (hipEvent_t e : p->inflight) p->ev_pool.push_back(e);
    p->inflight.clear();
    if (p->copier)
        for (int s = 0; s < 2; ++s) {
            const uint64_t t[3] = {p->t_up[s], p->t_dn[s], p->t_rt[s]};
            for (uint64_t x : t)
                if (x && (rc = uwip_copier_wait(p->copier, x))) return copier_rc(p, rc);
        }
    if (p->copier)
        for (uint64_t x : p->st.t_table)
            if (x && (rc = uwip_copier_wait(p->copier, x))) return copier_rc(p, rc);
    return UWIP_OK;
}

UWIP_API int uwip_pipe_destroy(uwip_pipe *p)
{
    if (!p) return UWIP_OK;
    (void)uwip_pipe_sync(p);
    (void)hipSetDevice(p->ctx->device);
    for (hipEvent_t e : p->ev_pool) (void)hipEventDestroy(e);
    if (p->own_copier) uwip_copier_destroy(p->copier);
    if (p->own_staging) uwip_free(p->ctx, p->staging);
    uwip_features_destroy(p->feats);
    kf_free(p);
    st_free(p);
    uwip_free(p->ctx, p->v);
    delete p;
    return UWIP_OK;
}

UWIP_API const char *uwip_pipe_last_error(const uwip_pipe *p) { return p ? p->err.c_str() : "null pipe"; }

UWIP_API int uwip_pipe_stages(uwip_pipe *p, unsigned stages, const uwip_batch_u8 *in, const uwip_batch_u8 *out, float *d_ratio,
                              int32_t *d_info)
{
    if (!p) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
    if (stages & ~UWIP_PIPE_ALL) return p->fail(UWIP_ERR_INVALID, "unknown stage");
    if (int rc = check_io(p, out, "`out` is not a 3-channel batch of the configured geometry")) return rc;
    if (stages & UWIP_PIPE_DEHAZE) {
        if (int rc = check_io(p, in, "`in` is not a 3-channel batch of the configured geometry")) return rc;
        if (in->data == out->data) return p->fail(UWIP_ERR_INVALID, "the dehaze stage is not in place: `in` and `out` must be distinct buffers");
    }
    const int rc = run_stages(p, stages, in, out, d_ratio, d_info);
    if (!rc) { p->last_frames = (const uint8_t *)out->data; p->last_ratio = d_ratio; p->last_info = d_info; }
    return rc;
}

UWIP_API int uwip_pipe_step(uwip_pipe *p, const uwip_batch_u8 *in, const uwip_batch_u8 *out, float *d_ratio, int32_t *d_info)
{
    if (!p) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
    int rc = throttle_wait(p);
    if (rc) return rc;
    if ((rc = uwip_pipe_stages(p, UWIP_PIPE_ALL, in, out, d_ratio, d_info))) return rc;
    return throttle_record(p);
}

UWIP_API int uwip_pipe_step_host(uwip_pipe *p, const void *h_in, void *h_out, float *h_ratio, const void *h_prefetch, uint64_t tickets[3])
{
    if (!p) return UWIP_ERR_INVALID;
    if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
    if (!h_in || !h_out) return p->fail(UWIP_ERR_INVALID, "null host buffer");
    int rc = ensure_host_state(p);
    if (rc) return rc;
    // Two source and two result buffers in device memory, so that batch k + 1 arrives and batch k leaves while the kernels of
    // batch k / k + 1 run.  Every hand-over is a ticket waited for on the host: no stream ever waits for another one on the
    // device (a barrier packet behind a DMA copy stalls whatever shares its hardware queue; DESIGN.md, host-buffer mode).
    const uint64_t k = p->k;
    const int slot = (int)(k & 1);
    const size_t fb = p->frame_bytes;
    if (p->pending != h_in) {
        // nobody prefetched this batch.  src[slot] was last read by batch k - 2's dehaze, which precedes everything queued now
        rc = uwip_copier_upload(p->copier, k >= 2 ? p->ctx : nullptr, p->src[slot], h_in, fb, &p->t_up[slot]);
        if (rc) return copier_rc(p, rc);
    }
    p->pending = nullptr;
    const uint64_t t_in = p->t_up[slot];
    if (h_prefetch) {
        // src[1 - slot] was last read by batch k - 1's dehaze: the upload starts when the stream has finished batch k - 1
        rc = uwip_copier_upload(p->copier, k >= 1 ? p->ctx : nullptr, p->src[1 - slot], h_prefetch, fb, &p->t_up[1 - slot]);
        if (rc) return copier_rc(p, rc);
        p->pending = h_prefetch;
    }
    if ((rc = uwip_copier_wait(p->copier, t_in))) return copier_rc(p, rc);                 // batch k is in device memory
    if ((rc = uwip_copier_wait(p->copier, p->t_dn[slot]))) return copier_rc(p, rc);        // batch k - 2's frames have left work[slot]
    if ((rc = uwip_copier_wait(p->copier, p->t_rt[slot]))) return copier_rc(p, rc);        // ... and its ratios
    const uwip_batch_u8 in = batch_of(p->src[slot], p->cfg, 3), out = batch_of(p->work[slot], p->cfg, 3);
    if ((rc = run_stages(p, UWIP_PIPE_DEHAZE | UWIP_PIPE_HISTRETCH | UWIP_PIPE_ACLAHE, &in, &out, nullptr, nullptr))) return rc;
    // the enhanced frames are final here (the overlap stage only reads them): they leave under its kernels
    if ((rc = uwip_copier_download(p->copier, p->ctx, h_out, p->work[slot], fb, &p->t_dn[slot]))) return copier_rc(p, rc);
    if ((rc = run_stages(p, UWIP_PIPE_OVERLAP, nullptr, &out, p->ratio[slot], p->info[slot]))) return rc;
    p->t_rt[slot] = 0;
    if (h_ratio && (rc = uwip_copier_download(p->copier, p->ctx, h_ratio, p->ratio[slot], sizeof(float) * (size_t)p->cfg.frames, &p->t_rt[slot])))
        return copier_rc(p, rc);
    p->last_frames = p->work[slot]; p->last_ratio = p->ratio[slot]; p->last_info = p->info[slot];
    if (tickets) { tickets[0] = t_in; tickets[1] = p->t_dn[slot]; tickets[2] = p->t_rt[slot]; }
    p->k = k + 1;
    return UWIP_OK;
}

UWIP_API int uwip_pipe_wait(uwip_pipe *p, uint64_t ticket)
{
    if (!p) return UWIP_ERR_INVALID;
    if (!ticket) return UWIP_OK;
    if (!p->copier) return p->fail(UWIP_ERR_INVALID, "no copy has been requested on this pipe");
    return copier_rc(p, uwip_copier_wait(p->copier, ticket));
}

UWIP_API int uwip_pipe_reset(uwip_pipe *p)
{
    if (!p) return UWIP_ERR_INVALID;
    p->have_prev = false;
    p->eos_valid = -1;
    p->kf.started = false;
    p->kf.base = 0;
    p->st.base = 0;
    return UWIP_OK;
}

UWIP_API int uwip_pipe_last_params(uwip_pipe *p, int32_t *h_bs, int32_t *h_cl)
{
    if (!p) return UWIP_ERR_INVALID;
    return p->from_ctx(uwip_aclahe_last_params(p->ctx, h_bs, h_cl, p->cfg.frames));
}

UWIP_API int uwip_pipe_device_results(uwip_pipe *p, const uint8_t **d_v, const uint8_t **d_frames, const float **d_ratio,
                                      const int32_t **d_info)
{
    if (!p) return UWIP_ERR_INVALID;
    if (d_v) *d_v = p->v;
    if (d_frames) *d_frames = p->last_frames;
    if (d_ratio) *d_ratio = p->last_ratio;
    if (d_info) *d_info = p->last_info;
    return UWIP_OK;
}

// ---- key-frame mode ----------------------------------------------------------------------------------------------

UWIP_API int uwip_keyframe_config_default(uwip_keyframe_config *kc)
{
    if (!kc) return UWIP_ERR_INVALID;
    std::memset(kc, 0, sizeof *kc);
    kc->minOverlap = uwip_kf::OVERLAP_MIN;      // videostrip.hpp:50
    kc->kWindow = 11;                           // videostrip.hpp:51
    kc->lookback = 8;                           // the cheapest D measured (tools/keyframe_cost.py)
    kc->max_rows = 4096;
    return UWIP_OK;
}

UWIP_API int uwip_keyframe_max_rounds(const uwip_keyframe_config *kc, int frames)
{
    if (!kc || !uwip_kf::config_ok(*kc) || frames < 1) return -1;
    return uwip_kf::max_rounds(frames, kc->lookback, kc->kWindow);
}

UWIP_API int uwip_pipe_keyframe_chain(uwip_pipe *p, const uwip_keyframe_config *kc)
{
    if (!p) return UWIP_ERR_INVALID;
    if (!kc || !uwip_kf::config_ok(*kc)) return p->fail(UWIP_ERR_INVALID, "bad key-frame configuration");
    if (p->have_prev || p->kf.started || p->eos_valid >= 0)
        return p->fail(UWIP_ERR_INVALID, "uwip_pipe_keyframe_chain: before the first step or right after uwip_pipe_reset");
    if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
    const int F = p->cfg.frames;
    const int P0 = uwip_kf::round0_pairs(F, kc->lookback), R = uwip_kf::max_rounds(F, kc->lookback, kc->kWindow);
    if (P0 > 65535 || F + 2 > 4096) return p->fail(UWIP_ERR_INVALID, "batch too large for key-frame mode (pair list > 65535)");
    int rc = uwip_pipe_sync(p);                 // the feature slots and the chain's buffers are re-made
    if (rc) return rc;
    kf_free(p);
    uwip_features_destroy(p->feats);
    p->feats = nullptr;
    if ((rc = uwip_features_create(p->ctx, F + 2, &p->feats))) return p->from_ctx(rc);
    uwip_pipe::Keyframe &k = p->kf;
    k.kc = *kc; k.R = R; k.P0 = P0;
    if ((rc = uwip_overlap_working_size(p->cfg.rows, p->cfg.cols, &k.oh, &k.ow))) return p->fail(rc, "uwip_overlap_working_size");
    const size_t npo = (size_t)P0 + (size_t)R * F, scratch = uwip_overlap_match_scratch_bytes(std::max(P0, F));
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
    const size_t o_state = take(sizeof(uwip_kf::State)), o_fbk = take(4 * (size_t)(R + 1)), o_fbs = take(4 * (size_t)(R + 1)),
                 o_fbl = take(4 * 2 * (size_t)F), o_fbn = take(4), o_r0 = take(4 * 2 * (size_t)P0), o_ratio = take(4 * npo),
                 o_info = take(32 * npo), o_midx = take(scratch), o_mdist = take(scratch), o_blur = take(4 * (size_t)F),
                 o_ring = take(sizeof(uwip_keyframe_row) * (size_t)kc->max_rows),
                 o_res = take((size_t)F * k.oh * k.ow * 3);
    void *d = nullptr;
    if ((rc = uwip_malloc(p->ctx, off, &d))) return p->from_ctx(rc);
    uint8_t *base = (uint8_t *)d;
    k.block = base;
    k.state = (uwip_kf::State *)(base + o_state);
    k.fb_key = (int32_t *)(base + o_fbk); k.fb_start = (int32_t *)(base + o_fbs);
    k.fb_list = (int32_t *)(base + o_fbl); k.fb_n = (int32_t *)(base + o_fbn); k.r0 = (int32_t *)(base + o_r0);
    k.out_ratio = (float *)(base + o_ratio); k.out_info = (int32_t *)(base + o_info);
    k.midx = (int32_t *)(base + o_midx); k.mdist = (int32_t *)(base + o_mdist);
    k.blur = (float *)(base + o_blur); k.ring = (uwip_keyframe_row *)(base + o_ring); k.res = base + o_res;
    // round 0's fixed list (kf_chain.hpp round0_index): (i, slot 0) for every frame, then (i, i - d) for d = 1..D
    std::vector<int32_t> r0(2 * (size_t)P0);
    uwip_kf::round0_list(F, kc->lookback, r0.data(), r0.data() + P0);
    uwip_kf::State st{};
    st.carry_key = st.carry_best = -1;
    if ((rc = uwip_memcpy_h2d(p->ctx, k.r0, r0.data(), sizeof(int32_t) * r0.size())) ||
        (rc = uwip_memcpy_h2d(p->ctx, k.state, &st, sizeof st))) {
        kf_free(p);
        return p->from_ctx(rc);
    }
    k.on = true;
    // a streams configuration made earlier counts the rows of the new ring (State::total starts at 0 again)
    if (p->st.on && hipMemsetAsync(p->st.emitted, 0, sizeof(uint32_t), p->ctx->stream) != hipSuccess) return p->fail(UWIP_ERR_HIP, "hipMemsetAsync");
    return UWIP_OK;
}

UWIP_API int uwip_pipe_end_of_stream(uwip_pipe *p, int valid)
{
    if (!p) return UWIP_ERR_INVALID;
    if (valid < 1 || valid > p->cfg.frames) return p->fail(UWIP_ERR_INVALID, "valid must be in [1, frames]");
    p->eos_valid = valid;
    return UWIP_OK;
}

UWIP_API int uwip_pipe_keyframes(uwip_pipe *p, uwip_keyframe_row *h_rows, int cap, int *n)
{
    if (!p) return UWIP_ERR_INVALID;
    if (!n || cap < 0 || (cap > 0 && !h_rows)) return p->fail(UWIP_ERR_INVALID, "null buffer or negative capacity");
    *n = 0;
    if (!p->kf.on) return p->fail(UWIP_ERR_INVALID, "the pipe is not in key-frame mode (uwip_pipe_keyframe_chain)");
    if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
    uwip_pipe::Keyframe &k = p->kf;
    const hipError_t he = uwip_stream_wait(p->ctx);
    if (he != hipSuccess) return p->fail(UWIP_ERR_HIP, hipGetErrorString(he));
    uwip_kf::State st;
    if (hipMemcpy(&st, k.state, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return p->fail(UWIP_ERR_HIP, "hipMemcpy");
    if (st.err) {
        // reported once; the chain stays stopped until the next stream (uwip_pipe_reset / uwip_pipe_end_of_stream)
        const int32_t zero = 0;
        if (hipMemcpy(&k.state->err, &zero, sizeof zero, hipMemcpyHostToDevice) != hipSuccess) return p->fail(UWIP_ERR_HIP, "hipMemcpy");
        return p->fail(UWIP_ERR_INVALID, "key-frame chain: a batch was not resolved within the round bound; the stream's chain stopped there");
    }
    const uint32_t M = (uint32_t)k.kc.max_rows;
    if (st.total - k.consumed > M) {
        const uint32_t lost = st.total - k.consumed - M;
        k.consumed = st.total - M;
        return p->fail(UWIP_ERR_INVALID, (std::string("uwip_pipe_keyframes: the caller fell behind the row ring: ") +
                                          std::to_string(lost) + " rows were overwritten").c_str());
    }
    const uint32_t m = std::min<uint32_t>(st.total - k.consumed, (uint32_t)cap);
    for (uint32_t done = 0; done < m;) {
        const uint32_t at = (k.consumed + done) % M, run = std::min(m - done, M - at);
        if (hipMemcpy(h_rows + done, k.ring + at, sizeof(uwip_keyframe_row) * run, hipMemcpyDeviceToHost) != hipSuccess)
            return p->fail(UWIP_ERR_HIP, "hipMemcpy");
        done += run;
    }
    k.consumed += m;
    *n = (int)m;
    return UWIP_OK;
}

// ---- compressed frames in, compressed (key) frames out ----------------------------------------------------------------

UWIP_API int uwip_pipe_streams_config_default(uwip_pipe_streams_config *cfg)
{
    if (!cfg) return UWIP_ERR_INVALID;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->format = UWIP_STREAM_JPEG;
    cfg->quality = 95;                          // cv::imwrite's default
    cfg->png_filter = -1;
    cfg->emit = UWIP_EMIT_ALL;
    cfg->slot_bytes = 0;                        // the raw frame size
    cfg->depth = 2;
    return UWIP_OK;
}

UWIP_API int uwip_pipe_streams(uwip_pipe *p, const uwip_pipe_streams_config *cfg)
{
    if (!p) return UWIP_ERR_INVALID;
    if (!cfg) return p->fail(UWIP_ERR_INVALID, "null streams configuration");
    if (cfg->format != UWIP_STREAM_JPEG && cfg->format != UWIP_STREAM_PNG) return p->fail(UWIP_ERR_INVALID, "format must be UWIP_STREAM_JPEG or UWIP_STREAM_PNG");
    if (cfg->emit != UWIP_EMIT_ALL && cfg->emit != UWIP_EMIT_KEYFRAMES) return p->fail(UWIP_ERR_INVALID, "emit must be UWIP_EMIT_ALL or UWIP_EMIT_KEYFRAMES");
    if (cfg->png_filter < -1 || cfg->png_filter > 4) return p->fail(UWIP_ERR_INVALID, "png_filter must be -1 (adaptive) or 0..4");
    if (cfg->depth < 2 || cfg->depth > 64) return p->fail(UWIP_ERR_INVALID, "depth must be 2..64");
    if (cfg->emit == UWIP_EMIT_KEYFRAMES && !p->kf.on)
        return p->fail(UWIP_ERR_INVALID, "UWIP_EMIT_KEYFRAMES needs key-frame mode (uwip_pipe_keyframe_chain first)");
    if (p->have_prev || p->kf.started || p->eos_valid >= 0 || p->st.base != 0)
        return p->fail(UWIP_ERR_INVALID, "uwip_pipe_streams: before the first step or right after uwip_pipe_reset");
    if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
    int rc = ensure_copier(p);
    if (rc) return rc;
    if ((rc = uwip_pipe_sync(p))) return rc;    // the buffers are re-made; results not collected are dropped
    st_free(p);
    uwip_pipe::Streams &s = p->st;
    const int F = p->cfg.frames, depth = cfg->depth;
    s.sc = *cfg;
    if (s.sc.quality == 0) s.sc.quality = 95;
    s.one_frame = (size_t)p->cfg.rows * p->cfg.cols * 3;
    s.slot_bytes = cfg->slot_bytes ? cfg->slot_bytes : s.one_frame;
    s.table_bytes = uwip_ps::table_bytes(F);
    const size_t blob_cap = (size_t)(F + 1) * s.slot_bytes;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
    const size_t o_src = take(s.one_frame * F), o_work = take(s.one_frame * F), o_carried = take(s.one_frame),
                 o_compact = take(s.one_frame * (F + 1)), o_slots = take(blob_cap + 16), o_sizes = take(8 * (size_t)(F + 1)),
                 o_status = take(4 * (size_t)F), o_seln = take(4), o_emitted = take(4), o_ratio = take(4 * (size_t)F),
                 o_sel = take(sizeof(uwip_ps::Sel) * (size_t)(F + 1));
    std::vector<size_t> o_table(depth), o_blob(depth);
    for (int d = 0; d < depth; ++d) { o_table[d] = take(s.table_bytes); o_blob[d] = take(blob_cap + 16); }
    void *dv = nullptr;
    if ((rc = uwip_malloc(p->ctx, off, &dv))) return p->from_ctx(rc);
    uint8_t *b = (uint8_t *)dv;
    s.block = b;
    s.src = b + o_src; s.work = b + o_work; s.carried = b + o_carried; s.compact = b + o_compact; s.slots = b + o_slots;
    s.sizes = (int64_t *)(b + o_sizes); s.status = (int32_t *)(b + o_status); s.sel_n = (int32_t *)(b + o_seln);
    s.emitted = (uint32_t *)(b + o_emitted); s.ratio = (float *)(b + o_ratio); s.sel = (uwip_ps::Sel *)(b + o_sel);
    for (int d = 0; d < depth; ++d) {
        s.table.push_back(b + o_table[d]);
        s.blob.push_back(b + o_blob[d]);
        void *h = nullptr;
        if ((rc = uwip_host_alloc(p->ctx, s.table_bytes, &h))) { st_free(p); return p->from_ctx(rc); }
        s.h_table.push_back((uint8_t *)h);
    }
    s.t_table.assign(depth, 0);
    s.ticket.assign(depth, 0);
    s.h_par.assign(depth, std::vector<int32_t>());
    // the carried frame is read only by a row that names it, which a carry precedes; zeroed all the same.  The rows the ring
    // holds by now (none on a new pipe) are not this configuration's to emit.
    hipError_t he = hipMemsetAsync(s.carried, 0, s.one_frame, p->ctx->stream);
    if (he == hipSuccess) he = hipMemsetAsync(s.emitted, 0, sizeof(uint32_t), p->ctx->stream);
    if (he == hipSuccess && p->kf.on)
        he = hipMemcpyAsync(s.emitted, &p->kf.state->total, sizeof(uint32_t), hipMemcpyDeviceToDevice, p->ctx->stream);
    if (he != hipSuccess) { st_free(p); return p->fail(UWIP_ERR_HIP, hipGetErrorString(he)); }
    s.on = true;
    return UWIP_OK;
}

UWIP_API int uwip_pipe_step_streams(uwip_pipe *p, const uint8_t *const *h_streams, const size_t *h_sizes, int n, uint64_t *ticket)
{
    if (!p) return UWIP_ERR_INVALID;
    if (!h_streams || !h_sizes || !ticket) return p->fail(UWIP_ERR_INVALID, "null argument");
    *ticket = 0;
    if (n != p->cfg.frames) return p->fail(UWIP_ERR_INVALID, "n must be the pipe's `frames`");
    for (int j = 0; j < n; ++j)
        if (!h_streams[j] && h_sizes[j]) return p->fail(UWIP_ERR_INVALID, "null stream");
    if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
    uwip_pipe::Streams &s = p->st;
    if (!s.on) return p->fail(UWIP_ERR_INVALID, "the pipe has no streams configuration (uwip_pipe_streams)");
    const int F = n, slot = (int)(s.k % (uint64_t)s.sc.depth);
    if (s.ticket[slot]) return p->fail(UWIP_ERR_INVALID, "the result this step would overwrite has not been collected (uwip_pipe_collect)");
    uwip_ctx *ctx = p->ctx;
    int rc = throttle_wait(p);
    if (rc) return rc;
    // decode: a step of one kind is one call, a mixed step one call per run of one kind, each into its slots of the batch
    static const uint8_t png_sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    auto is_png = [&](int j) { return h_sizes[j] >= 8 && !std::memcmp(h_streams[j], png_sig, 8); };
    const uwip_batch_u8 in = batch_of(s.src, p->cfg, 3), out = batch_of(s.work, p->cfg, 3);
    for (int j0 = 0; j0 < F;) {
        int j1 = j0 + 1;
        while (j1 < F && is_png(j1) == is_png(j0)) ++j1;
        const uwip_batch_u8 bq = batch_of(s.src + s.one_frame * j0, p->cfg, 3, j1 - j0);
        rc = is_png(j0) ? uwip_png_decode(ctx, h_streams + j0, h_sizes + j0, j1 - j0, &bq, nullptr, s.status + j0)
                        : uwip_jpeg_decode(ctx, h_streams + j0, h_sizes + j0, j1 - j0, &bq, nullptr, s.status + j0);
        if (rc) return p->from_ctx(rc);
        j0 = j1;
    }
    if ((rc = uwip_ps_blank(ctx, s.src, F, s.one_frame, s.status))) return p->from_ctx(rc);
    // what the selection needs to know of this step, before the overlap stage consumes the end-of-stream mark
    const bool keyframes = s.sc.emit == UWIP_EMIT_KEYFRAMES;
    uwip_ps::Step u{};
    u.emit_all = keyframes ? 0 : 1; u.F = F; u.valid = p->eos_valid >= 0 ? p->eos_valid : F;
    u.base = p->kf.on ? p->kf.base : s.base;
    u.max_rows = keyframes ? p->kf.kc.max_rows : 1;
    u.frame_bytes = s.one_frame; u.status = s.status;
    u.ring = keyframes ? p->kf.ring : nullptr;
    u.total = keyframes ? &p->kf.state->total : nullptr;
    u.carry_best = keyframes ? &p->kf.state->carry_best : nullptr;
    u.emitted = s.emitted; u.work = s.work; u.carried = s.carried; u.compact = s.compact; u.sel = s.sel; u.sel_n = s.sel_n;
    const bool last = p->eos_valid >= 0;
    if ((rc = run_stages(p, UWIP_PIPE_ALL, &in, &out, s.ratio, nullptr))) return rc;
    p->last_frames = s.work; p->last_ratio = s.ratio; p->last_info = nullptr;
    s.base = last ? 0 : s.base + F;
    if ((rc = uwip_ps_select_gather(ctx, u))) return p->from_ctx(rc);
    const uwip_batch_u8 cb = batch_of(s.compact, p->cfg, 3, F + 1);
    rc = s.sc.format == UWIP_STREAM_PNG ? uwip_png_encode_dev(ctx, &cb, s.sc.png_filter, s.slots, s.slot_bytes, s.sizes, s.sel_n)
                                        : uwip_jpeg_encode_dev(ctx, &cb, s.sc.quality, s.slots, s.slot_bytes, s.sizes, s.sel_n);
    if (rc) return p->from_ctx(rc);
    // the aclahe stage's parameters go with the result: from the device record where the choice was made there, else from the host's
    const int32_t *d_par = nullptr;
    s.h_par[slot].clear();
    if (ctx->aclahe_last_n == F && ctx->aclahe_last_on_device) {
        d_par = (const int32_t *)uwip_ws(ctx, "auto.par", sizeof(int32_t) * 4 * (size_t)F);
        if (!d_par) return p->from_ctx(UWIP_ERR_NOMEM);
    } else if (ctx->aclahe_last_n == F && ctx->aclahe_last_host.size() == 4 * (size_t)F) {
        for (int f = 0; f < F; ++f) { s.h_par[slot].push_back(ctx->aclahe_last_host[4 * f]); s.h_par[slot].push_back(ctx->aclahe_last_host[4 * f + 1]); }
    }
    if ((rc = uwip_ps_pack(ctx, u, s.sizes, s.ratio, d_par, s.slots, s.slot_bytes, s.table[slot], s.blob[slot]))) return p->from_ctx(rc);
    // the one small copy of a result, requested now: it leaves when the stream has finished this step
    if ((rc = uwip_copier_download(p->copier, ctx, s.h_table[slot], s.table[slot], s.table_bytes, &s.t_table[slot]))) return copier_rc(p, rc);
    s.k += 1;
    s.ticket[slot] = s.k;
    *ticket = s.k;
    return throttle_record(p);
}

UWIP_API int uwip_pipe_collect(uwip_pipe *p, uint64_t ticket, int32_t *h_status, float *h_ratio, uwip_stream_out *h_outs, int cap,
                               int *n_outs, uint8_t *h_blob, size_t blob_cap, size_t *blob_bytes)
{
    if (!p) return UWIP_ERR_INVALID;
    if (!h_status || !n_outs || !blob_bytes || cap < 0 || (cap > 0 && !h_outs) || (blob_cap > 0 && !h_blob))
        return p->fail(UWIP_ERR_INVALID, "null buffer or negative capacity");
    *n_outs = 0;
    *blob_bytes = 0;
    uwip_pipe::Streams &s = p->st;
    if (!s.on) return p->fail(UWIP_ERR_INVALID, "the pipe has no streams configuration (uwip_pipe_streams)");
    if (!ticket || ticket > s.k) return p->fail(UWIP_ERR_INVALID, "no such ticket");
    const int slot = (int)((ticket - 1) % (uint64_t)s.sc.depth), F = p->cfg.frames;
    if (s.ticket[slot] != ticket) return p->fail(UWIP_ERR_INVALID, "this result has been collected already");
    if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
    int rc = uwip_copier_wait(p->copier, s.t_table[slot]);          // the step is done when its table has arrived
    if (rc) return copier_rc(p, rc);
    const uint8_t *t = s.h_table[slot];
    uwip_ps::TableHdr hdr;
    std::memcpy(&hdr, t, sizeof hdr);
    *n_outs = hdr.n_outs;
    *blob_bytes = (size_t)hdr.blob_bytes;
    if (hdr.n_outs > cap) return p->fail(UWIP_ERR_INVALID, "h_outs is too small (*n_outs entries are needed); the result stays collectable");
    if (hdr.blob_bytes > blob_cap) return p->fail(UWIP_ERR_INVALID, "h_blob is too small (*blob_bytes are needed); the result stays collectable");
    if (hdr.blob_bytes) {
        uint64_t tb = 0;
        if ((rc = uwip_copier_download(p->copier, nullptr, h_blob, s.blob[slot], (size_t)hdr.blob_bytes, &tb)) ||
            (rc = uwip_copier_wait(p->copier, tb)))
            return copier_rc(p, rc);
    }
    std::memcpy(h_outs, t + uwip_ps::outs_offset(), sizeof(uwip_stream_out) * (size_t)hdr.n_outs);
    std::memcpy(h_status, t + uwip_ps::status_offset(F), sizeof(int32_t) * (size_t)F);
    if (h_ratio) std::memcpy(h_ratio, t + uwip_ps::ratio_offset(F), sizeof(float) * (size_t)F);
    s.ticket[slot] = 0;
    s.t_table[slot] = 0;
    return UWIP_OK;
}

UWIP_API int uwip_pipe_result_params(uwip_pipe *p, uint64_t ticket, int32_t *h_bs, int32_t *h_cl)
{
    if (!p) return UWIP_ERR_INVALID;
    if (!h_bs || !h_cl) return p->fail(UWIP_ERR_INVALID, "null output");
    uwip_pipe::Streams &s = p->st;
    if (!s.on) return p->fail(UWIP_ERR_INVALID, "the pipe has no streams configuration (uwip_pipe_streams)");
    if (!ticket || ticket > s.k) return p->fail(UWIP_ERR_INVALID, "no such ticket");
    const int slot = (int)((ticket - 1) % (uint64_t)s.sc.depth), F = p->cfg.frames;
    if (s.ticket[slot] != ticket) return p->fail(UWIP_ERR_INVALID, "this result has been collected already");
    const int32_t *par = s.h_par[slot].data();
    if (s.h_par[slot].empty()) {
        if (int rc_e = uwip_enter(p->ctx)) return p->from_ctx(rc_e);
        const int rc = uwip_copier_wait(p->copier, s.t_table[slot]);
        if (rc) return copier_rc(p, rc);
        par = (const int32_t *)(s.h_table[slot] + uwip_ps::par_offset(F));
    }
    for (int f = 0; f < F; ++f) { h_bs[f] = par[2 * f]; h_cl[f] = par[2 * f + 1]; }
    return UWIP_OK;
}
