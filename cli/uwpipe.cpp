// uwpipe -- the reference's four tools run back to back as ONE program over the C ABI's whole-chain entry (uwip_pipe_*):
//   bgdehaze (modules/bgdehaze/main.py:14-20) -> histretch -c=RGB (modules/histretch/src/histretch.cpp:217-254) ->
//   aclahe (modules/aclahe/src/aclahe.cpp:152-218 + python/ACLAHE.py:9-129, python/main.py:19-20) ->
//   calcOverlap of every frame against its predecessor (modules/videostrip/src/videostrip.cpp:192-289)
// on the frames of a Motion-JPEG .avi or of a frame list, in batches through page-locked host buffers
// (uwip_pipe_step_host: batch k + 1 is uploaded and batch k - 1 leaves while batch k's kernels run).
//   uwpipe [-b N] [-c LETTERS] [-w N] [--guard-s] [--min6] [--relative-threshold] [--png] [--device-jpeg] [--device-png] [--device-decode]
//          [--streams] [--keyframes [-k N] [-p X] [--lookback D]] <video.avi | frame_list.txt> <output_prefix>
// writes <prefix>NNNN.jpg (the enhanced frames) and <prefix>uwpipe_report.txt (TSV: ID, Filename, Overlap, BS, CL).
// --keyframes: the overlap stage runs videostrip's key-frame selector (main.cpp:284-394) on the enhanced frames, on the
// device (uwip_pipe_keyframe_chain); <prefix>videostrip_report.txt gets its rows with the reference's columns (ID, Frame,
// Filename, Overlap, Blur), Filename = the enhanced frame that is the key frame.  Overlap in uwpipe_report.txt is then the
// overlap against the current key frame (nan: not compared).
// --keyframes --strip [--strip-mode feather|first|last|multiband|seam]: the enhanced key frames are also chained by their homographies and
// blended into one image per segment, <prefix>strip_NNN.<ext>, with a "Strip:" line per segment after the table of
// videostrip_report.txt (cli/stripout.hpp).  Refused with --streams, where the frames never reach the host.  --strip-gain: with
// gain compensation from the overlaps of consecutive key frames (uwip_strip_gains); refused without --strip.
// --device-jpeg: the enhanced frames of a step are encoded on the device (uwip_jpeg_encode_host on the pipe's context, from
// the step's frames in the staging area) and the files are written from the returned streams: the same bytes as without it.
// --device-png: the files are .png, encoded on the device in the same way (uwip_png_encode_host): the pixels of --png, other bytes.
// --device-decode (.avi, or a list of .jpg / .png files): the compressed frames of a step are decoded on the pipe's context
// into a device batch -- the frames that start with the PNG signature by uwip_png_decode_host, the others by
// uwip_jpeg_decode_host, a mixed step run by run --, uwip_pipe_step runs on the resident frames, and the results leave as streams
// (--device-jpeg) or by a plain download; a frame with a negative status is decoded on the host and copied into its slot.
// The files and both reports are the same bytes as without the flag.  The steps run one after another here (decode, step,
// wait, results): the overlap of upload, kernels and download that uwip_pipe_step_host gives the raw-frame path is not used.
// --streams (implies --device-decode and device output: .png with --png / --device-png, else .jpg): the compressed frames of a step
// go to uwip_pipe_step_streams, which returns when the step is queued; the loop queues step k, then collects step k - 1
// (uwip_pipe_collect) and writes its files while the device works on step k.  Only compressed bytes cross the link.  With
// --keyframes only the key frames are encoded and written -- what the reference's videostrip writes (main.cpp:368-381) --, named as
// videostrip_report.txt names them.  The files written and both reports are the same bytes as without the flag.  There is no host
// fallback here: a frame the device decoder leaves, or a stream that outgrows the raw frame size, ends the run with a message.
// Defaults are the reference's rules (uwip_pipe_config_default); the three switches are the library's opt-in deviations.
#include <algorithm>
#include <cstring>
#include <fstream>
#include "avi.hpp"
#include "stripout.hpp"
#include <deque>
#include "cliutil.hpp"

int main(int argc, char **argv)
{
    const Args a = parse_args(argc, argv, {"b", "batch", "c", "w", "window", "k", "p", "lookback", "strip-mode", "strip-max", "strip-levels", "strip-seam-prior"});
    if (a.pos.size() < 2 || a.has("h") || a.has("help")) {
        std::printf("uwpipe - bgdehaze -> histretch -> aclahe -> overlap of every frame against its predecessor\n"
                    "usage: uwpipe [-b N] [-c LETTERS] [-w N] [--guard-s] [--min6] [--relative-threshold] [--png] [--device-jpeg]\n"
                    "              [--device-png] [--device-decode] [--streams] [--keyframes [-k N] [-p X] [--lookback D] [--strip [--strip-gain]]] <video.avi (Motion-JPEG) | frame_list.txt> <output_prefix>\n"
                    "  -b N      frames per step (default 8)\n"
                    "  -c L      histretch letters (default RGB)\n"
                    "  -w N      bgdehaze window (default 15)\n"
                    "  --guard-s / --min6 / --relative-threshold   the library's opt-in deviations from the reference's rules (uwip.h)\n"
                    "  --device-jpeg   encode the .jpg files on the device (same bytes; ignored with --png)\n"
                    "  --device-png    write .png files encoded on the device (the pixels of --png; the bytes differ)\n"
                    "  --device-decode decode the input JPEG and PNG frames on the device (same files; a frame the device decoder leaves is decoded on the host)\n"
                    "  --streams       compressed frames in, compressed frames out, queued without a host wait (with --keyframes only the key frames are written)\n"
                    "  --keyframes   select key frames as videostrip does (report: <prefix>videostrip_report.txt)\n"
                    "  -k N          frames of the refinement window (default 11)\n"
                    "  -p X          minOverlap (default 0.4)\n"
                    "  --lookback D  frames matched ahead per frame (a speed knob; the results do not depend on it)\n"
                    "  --strip       with --keyframes: also blend the enhanced key frames into <prefix>strip_NNN.<ext>, one image per chained\n"
                    "                segment (--strip-mode feather|first|last|multiband|seam, --strip-levels N for multiband, --strip-seam-prior N for seam; --strip-max N key frames, default 1024: the strip keeps them\n"
                    "                at 640 wide in device memory, about 0.7 MB each, allocated at the first one; key frame N + 1 ends the\n"
                    "                program with an error).  Not with --streams: the frames never reach the host there\n"
                    "  --strip-gain  with --strip: one gain per key frame and colour channel from the overlaps of consecutive key frames\n");
        return 0;
    }
    const std::string InputFile = a.pos[0], OutputFile = a.pos[1];
    const char *ext = a.has("png") || a.has("device-png") ? "png" : "jpg";
    std::vector<std::string> frames;
    avi::Reader video;
    const bool is_avi = imgio::ends_with(InputFile, ".avi");
    if (is_avi) {
        if (!video.open(InputFile)) { std::printf("Unable to open: %s\n", InputFile.c_str()); return EXIT_FAILURE; }
        frames.resize(video.count());
    } else {
        std::ifstream f(InputFile); std::string l; while (std::getline(f, l)) if (!l.empty()) frames.push_back(l);
    }
    if (frames.empty()) { std::printf("Unable to open frame list: %s\n", InputFile.c_str()); return EXIT_FAILURE; }
    auto read_at = [&](size_t i, imgio::Image &im) { return is_avi ? video.read(i, im) : imgio::imread(frames[i], im, true); };
    imgio::Image first;
    if (!read_at(0, first)) { std::printf("Unable to read first frame\n"); return EXIT_FAILURE; }
    const int rows = first.rows, cols = first.cols;
    const size_t n = frames.size();
    const int B = (int)std::min<size_t>(n, (size_t)std::max(1, std::atoi(a.get("b", a.get("batch", "8")).c_str())));
    const size_t fbytes = (size_t)rows * cols * 3;

    uwip_ctx *ctx = nullptr;
    uwip_pipe *pipe = nullptr;
    void *h_in[2] = {nullptr, nullptr}, *h_out = nullptr, *h_ratio = nullptr;
    void *d_in = nullptr, *d_out = nullptr, *d_ratio = nullptr;
    int rc = 0;
    const char *what = "";
#define CK(expr, msg) do { rc = (expr); if (rc) { what = msg; goto fail; } } while (0)
    {
        CK(uwip_ctx_create(0, nullptr, &ctx), "uwip_ctx_create (no HIP device? there is no CPU fallback)");
        uwip_pipe_config cfg;
        uwip_pipe_config_default(&cfg, B, rows, cols);
        std::snprintf(cfg.letters, sizeof cfg.letters, "%s", a.get("c", "RGB").c_str());
        cfg.w = std::atoi(a.get("w", a.get("window", "15")).c_str());
        if (a.has("guard-s")) cfg.dehaze_flags |= UWIP_DEHAZE_GUARD_S;
        if (a.has("min6")) cfg.match_flags |= UWIP_OVERLAP_MIN6;
        if (a.has("relative-threshold")) cfg.detect_flags |= UWIP_OVERLAP_RELATIVE_THRESHOLD;
        CK(uwip_pipe_create(ctx, &cfg, nullptr, &pipe), "uwip_pipe_create");
        const bool kf = a.has("keyframes");
        uwip_keyframe_config kc;
        uwip_keyframe_config_default(&kc);
        if (a.has("k")) kc.kWindow = std::atoi(a.get("k", "11").c_str());
        if (a.has("p")) kc.minOverlap = (float)std::atof(a.get("p", "0.4").c_str());
        if (a.has("lookback")) kc.lookback = std::atoi(a.get("lookback", "8").c_str());
        if (kf) CK(uwip_pipe_keyframe_chain(pipe, &kc), "uwip_pipe_keyframe_chain");
        // --strip: the enhanced key frames go into a strip as their rows arrive (cli/stripout.hpp).  The rows are then read after
        // every batch, and the enhanced frames of the last kWindow + 2 B + 2 stream positions are kept on the host: a row names a
        // frame at most a window and a batch back
        uw::Context strip_ctx(ctx);                        // a view: the context stays this program's
        StripOut strip;
        if (!strip.configure(a)) { std::printf("--strip-mode: feather, first, last or multiband (--strip-levels 1..4), or seam (--strip-seam-prior 0..4096)\n"); rc = UWIP_ERR_INVALID; what = "--strip-mode"; goto fail; }
        if (strip.gain_without_strip()) { std::printf("--strip-gain is refused without --strip: there is no strip to compensate\n"); rc = UWIP_ERR_INVALID; what = "--strip-gain"; goto fail; }
        strip.detect_flags = cfg.detect_flags; strip.match_flags = cfg.match_flags;
        if (strip.on && !kf) { std::printf("--strip needs --keyframes: the strip is made of the key frames\n"); rc = UWIP_ERR_INVALID; what = "--strip"; goto fail; }
        if (strip.on && a.has("streams")) {
            std::printf("--strip is refused with --streams: the enhanced frames never reach the host there; run without --streams\n");
            rc = UWIP_ERR_UNSUPPORTED; what = "--strip"; goto fail;
        }
        std::deque<std::pair<size_t, std::vector<uint8_t>>> recent;
        const size_t keep = (size_t)std::max(0, kc.kWindow) + 2 * (size_t)B + 2;
        auto strip_add = [&](int index, const char *file) -> bool {
            try {
                imgio::Image im;
                for (auto &r : recent) if (r.first == (size_t)index) { im.rows = rows; im.cols = cols; im.channels = 3; im.data = r.second; }
                if (im.empty() && !imgio::imread(file, im, true)) { std::printf("cannot read back %s\n", file); return false; }
                strip.add(strip_ctx, im);
                return true;
            } catch (const uw::Error &e) { std::printf("error: strip: %s\n", e.what()); return false; }
        };
        std::ofstream kreport;
        std::vector<uwip_keyframe_row> krows(256);
        const size_t kread = (size_t)std::max(1, kc.max_rows / (2 * (B + 1)));
        if (kf) {
            kreport.open(OutputFile + "videostrip_report.txt");
            kreport << "Input:\t" << InputFile << "\n";
            kreport << "Video metadata:\n\tSize:\t" << cols << " x " << rows << "\n\tFrames:\t" << n << "\n\thResize:\t"
                    << (float)640 / (float)cols << "\nTarget minOverlap:\t" << kc.minOverlap << "\nWindow size:\t" << kc.kWindow << "\n";
            kreport << "***************************************\nID\tFrame\tFilename\tOverlap\tBlur\n";
        }
        // --device-decode: the compressed frames of a step, the device batches it runs on; no raw frames are uploaded
        const bool streams = a.has("streams");
        const bool device_decode = a.has("device-decode") || streams;
        for (int s = 0; s < 2 && !device_decode; ++s) CK(uwip_host_alloc(ctx, fbytes * B, &h_in[s]), "uwip_host_alloc");
        CK(uwip_host_alloc(ctx, fbytes * B, &h_out), "uwip_host_alloc");
        CK(uwip_host_alloc(ctx, sizeof(float) * B, &h_ratio), "uwip_host_alloc");

        std::ofstream report(OutputFile + "uwpipe_report.txt");
        report << "Input:\t" << InputFile << "\nSize:\t" << cols << " x " << rows << "\nFrames:\t" << n << "\nBatch:\t" << B
               << "\n***************************************\nID\tFilename\tOverlap\tBS\tCL\n";
        // a batch = B consecutive frames; the last one is padded by repeating the final frame (its outputs are dropped)
        auto fill = [&](size_t k, void *dst) -> bool {
            imgio::Image im;
            for (int j = 0; j < B; ++j) {
                const size_t i = std::min(k * B + j, n - 1);
                if (!read_at(i, im) || im.rows != rows || im.cols != cols || im.channels != 3) {
                    std::printf("cannot read frame %zu (or its size differs from the first frame's)\n", i);
                    return false;
                }
                std::memcpy((uint8_t *)dst + fbytes * j, im.data.data(), fbytes);
            }
            return true;
        };
        const size_t nb = (n + B - 1) / B;
        std::vector<int32_t> bs(B), cl(B);
        // device_jpeg: the files come from device streams, JPEG or (device_png) PNG
        const bool device_png = a.has("device-png");
        const bool device_jpeg = device_png || (a.has("device-jpeg") && !a.has("png"));
        std::vector<uint8_t> jstreams(device_jpeg ? fbytes * B : 0);      // slot = the raw frame size
        std::vector<int64_t> jsizes(B, -1);
        uint64_t prev_up = 0;                    // upload ticket of the step that last read h_in[(k + 1) & 1]
        std::vector<std::vector<uint8_t>> jfiles(device_decode && !is_avi ? B : 0);
        std::vector<const uint8_t *> jptr(B);
        std::vector<size_t> jlen(B);
        std::vector<int32_t> jstatus(B);
        uwip_batch_u8 bin{}, bout{};
        if (device_decode && !streams) {
            CK(uwip_malloc(ctx, fbytes * B, &d_in), "uwip_malloc");
            CK(uwip_malloc(ctx, fbytes * B, &d_out), "uwip_malloc");
            CK(uwip_malloc(ctx, sizeof(float) * B, &d_ratio), "uwip_malloc");
            bin.rows = rows; bin.cols = cols; bin.channels = 3; bin.frames = B; bin.step = (size_t)cols * 3; bin.frame_stride = fbytes;
            bout = bin;
            bin.data = d_in; bout.data = d_out;
        }
        // decodes step k's frames into d_in: on the device, and on the host what the device decoder leaves
        auto decode_step = [&](size_t k) -> bool {
            for (int j = 0; j < B; ++j) {
                const size_t i = std::min(k * B + j, n - 1);
                if (is_avi) { jptr[j] = &video.buf[video.frames[i].first]; jlen[j] = video.frames[i].second; }
                else {
                    if (!imgio::read_file(frames[i], jfiles[j])) { std::printf("cannot read frame %zu\n", i); return false; }
                    jptr[j] = jfiles[j].data(); jlen[j] = jfiles[j].size();
                }
            }
            // a step of one kind is one call; a mixed step is split into its runs of one kind, each decoded into its slots
            static const uint8_t png_sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
            auto is_png = [&](int j) { return jlen[j] >= 8 && !std::memcmp(jptr[j], png_sig, 8); };
            for (int j0 = 0; j0 < B;) {
                int j1 = j0 + 1;
                while (j1 < B && is_png(j1) == is_png(j0)) ++j1;
                uwip_batch_u8 bq = bin;
                bq.frames = j1 - j0;
                bq.data = (uint8_t *)d_in + fbytes * j0;
                const bool png = is_png(j0);
                const int rcq = png ? uwip_png_decode_host(ctx, jptr.data() + j0, jlen.data() + j0, j1 - j0, &bq, nullptr, jstatus.data() + j0)
                                    : uwip_jpeg_decode_host(ctx, jptr.data() + j0, jlen.data() + j0, j1 - j0, &bq, nullptr, jstatus.data() + j0);
                if (rcq) {
                    std::printf("%s: %s\n", png ? "uwip_png_decode_host" : "uwip_jpeg_decode_host", uwip_last_error(ctx));
                    return false;
                }
                j0 = j1;
            }
            for (int j = 0; j < B; ++j) {
                if (jstatus[j] == 0) continue;
                const size_t i = std::min(k * B + j, n - 1);
                imgio::Image im;
                if (!read_at(i, im) || im.rows != rows || im.cols != cols || im.channels != 3) {
                    std::printf("cannot read frame %zu (or its size differs from the first frame's)\n", i);
                    return false;
                }
                if (k * B + j < n) std::printf("\nframe %zu: device decoder status %d, decoded on the host\n", i, jstatus[j]);
                if (uwip_memcpy_h2d(ctx, (uint8_t *)d_in + fbytes * j, im.data.data(), fbytes)) return false;
            }
            return true;
        };
        if (streams) {
            uwip_pipe_streams_config sc;
            uwip_pipe_streams_config_default(&sc);
            sc.format = std::strcmp(ext, "png") == 0 ? UWIP_STREAM_PNG : UWIP_STREAM_JPEG;
            sc.emit = kf ? UWIP_EMIT_KEYFRAMES : UWIP_EMIT_ALL;
            CK(uwip_pipe_streams(pipe, &sc), "uwip_pipe_streams");
            std::vector<uwip_stream_out> outs(B + 1);
            std::vector<uint8_t> blob(fbytes * (B + 1));
            std::vector<float> ratio(B);
            // queue step k: its compressed frames are copied inside the call, so one set of buffers serves every step
            auto submit = [&](size_t k, uint64_t *ticket) -> int {
                for (int j = 0; j < B; ++j) {
                    const size_t i = std::min(k * B + j, n - 1);
                    if (is_avi) { jptr[j] = &video.buf[video.frames[i].first]; jlen[j] = video.frames[i].second; }
                    else {
                        if (!imgio::read_file(frames[i], jfiles[j])) { std::printf("cannot read frame %zu\n", i); return UWIP_ERR_INVALID; }
                        jptr[j] = jfiles[j].data(); jlen[j] = jfiles[j].size();
                    }
                }
                if (k + 1 == nb) {                      // the padding of the last batch is no frame of the stream
                    const int rce = uwip_pipe_end_of_stream(pipe, (int)(n - k * B));
                    if (rce) return rce;
                }
                return uwip_pipe_step_streams(pipe, jptr.data(), jlen.data(), B, ticket);
            };
            // collect step k (the only wait, and for that step alone) and write its files and report rows
            auto drain = [&](size_t k, uint64_t ticket) -> int {
                int nouts = 0;
                size_t nblob = 0;
                int rcd = uwip_pipe_result_params(pipe, ticket, bs.data(), cl.data());
                if (!rcd) rcd = uwip_pipe_collect(pipe, ticket, jstatus.data(), ratio.data(), outs.data(), B + 1, &nouts, blob.data(), blob.size(), &nblob);
                if (rcd) return rcd;
                for (int j = 0; j < B && k * B + j < n; ++j)
                    if (jstatus[j] != 0) {
                        std::printf("\nframe %zu: device decoder status %d; --streams has no host fallback, run without it\n", k * B + j, jstatus[j]);
                        return UWIP_ERR_UNSUPPORTED;
                    }
                for (int e = 0; e < nouts; ++e) {
                    char name[512];
                    std::snprintf(name, sizeof name, "%s%04d.%s", OutputFile.c_str(), outs[e].index, ext);
                    if (outs[e].size < 0) {
                        std::printf("\nframe %d: its stream (%lld bytes) exceeds the slot; run without --streams\n", outs[e].index, (long long)-outs[e].size);
                        return UWIP_ERR_UNSUPPORTED;
                    }
                    FILE *jf = std::fopen(name, "wb");
                    const bool written = jf && std::fwrite(blob.data() + outs[e].offset, 1, (size_t)outs[e].size, jf) == (size_t)outs[e].size;
                    if (jf) std::fclose(jf);
                    if (!written) { std::printf("cannot write %s\n", name); return UWIP_ERR_INVALID; }
                }
                for (int j = 0; j < B && k * B + j < n; ++j) {
                    const size_t i = k * B + j;
                    char name[512];
                    std::snprintf(name, sizeof name, "%s%04zu.%s", OutputFile.c_str(), i, ext);
                    report << i << "\t" << name << "\t" << ratio[j] << "\t" << bs[j] << "\t" << cl[j] << "\n";
                }
                return UWIP_OK;
            };
            uint64_t tk[2] = {0, 0};
            for (size_t k = 0; k < nb; ++k) {
                CK(submit(k, &tk[k & 1]), "uwip_pipe_step_streams");
                if (k) CK(drain(k - 1, tk[(k - 1) & 1]), "uwip_pipe_collect");
                const bool more = k + 1 < nb;
                if (!more) CK(drain(k, tk[k & 1]), "uwip_pipe_collect");
                // the rows of the report: read as rarely as the ring allows (each read drains the stream), and after the last step
                const bool read_rows = kf && ((k + 1) % kread == 0 || !more);
                for (int got = (int)krows.size(); read_rows && got == (int)krows.size();) {
                    CK(uwip_pipe_keyframes(pipe, krows.data(), (int)krows.size(), &got), "uwip_pipe_keyframes");
                    for (int r = 0; r < got; ++r) {
                        const uwip_keyframe_row &w = krows[r];
                        char name[512];
                        std::snprintf(name, sizeof name, "%s%04d.%s", OutputFile.c_str(), w.index, ext);
                        if (w.id == 0) kreport << "0\t0\t" << name << "\t0.0\t0.0\n";              // main.cpp:297
                        else kreport << w.id << "\t" << w.frame << "\t" << name << "\t" << w.overlap << "\t" << w.blur << "\n";   // :381
                    }
                }
                std::printf("\rbatch %zu / %zu", k + 1, nb);
                std::fflush(stdout);
            }
            std::printf("\nEnd of input.\n");
            goto fail;                                  // rc == 0: the common clean-up
        }
        if (!device_decode && !fill(0, h_in[0])) { rc = UWIP_ERR_INVALID; what = "reading the input"; goto fail; }
        for (size_t k = 0; k < nb; ++k) {
            const bool more = k + 1 < nb;
            if (more && !device_decode) {
                CK(uwip_pipe_wait(pipe, prev_up), "uwip_pipe_wait");           // h_in[(k + 1) & 1] has left for the device
                if (!fill(k + 1, h_in[(k + 1) & 1])) { rc = UWIP_ERR_INVALID; what = "reading the input"; goto fail; }
            }
            if (kf && !more) CK(uwip_pipe_end_of_stream(pipe, (int)(n - k * B)), "uwip_pipe_end_of_stream");   // the padding stays out
            bool have_out = true;                 // the enhanced frames are in h_out
            if (device_decode) {
                if (!decode_step(k)) { rc = UWIP_ERR_INVALID; what = "reading the input"; goto fail; }
                CK(uwip_pipe_step(pipe, &bin, &bout, (float *)d_ratio, nullptr), "uwip_pipe_step");
                CK(uwip_pipe_last_params(pipe, bs.data(), cl.data()), "uwip_pipe_last_params");
                CK(uwip_pipe_sync(pipe), "uwip_pipe_sync");
                CK(uwip_memcpy_d2h(ctx, h_ratio, d_ratio, sizeof(float) * B), "uwip_memcpy_d2h");
                have_out = !device_jpeg;          // with --device-jpeg only streams leave (raw frames on demand, below)
                if (have_out) CK(uwip_memcpy_d2h(ctx, h_out, d_out, fbytes * B), "uwip_memcpy_d2h");
            } else {
                uint64_t t[3];
                CK(uwip_pipe_step_host(pipe, h_in[k & 1], h_out, (float *)h_ratio, more ? h_in[(k + 1) & 1] : nullptr, t), "uwip_pipe_step_host");
                prev_up = t[0];
                CK(uwip_pipe_last_params(pipe, bs.data(), cl.data()), "uwip_pipe_last_params");
                CK(uwip_pipe_wait(pipe, t[1]), "uwip_pipe_wait");
                CK(uwip_pipe_wait(pipe, t[2]), "uwip_pipe_wait");
            }
            if (device_jpeg) {
                const uint8_t *d_frames = (const uint8_t *)d_out;
                if (!device_decode) CK(uwip_pipe_device_results(pipe, nullptr, &d_frames, nullptr, nullptr), "uwip_pipe_device_results");
                uwip_batch_u8 bt{};
                bt.data = (void *)d_frames; bt.rows = rows; bt.cols = cols; bt.channels = 3; bt.frames = B;
                bt.step = (size_t)cols * 3; bt.frame_stride = fbytes;
                if (device_png) CK(uwip_png_encode_host(ctx, &bt, -1, jstreams.data(), fbytes, jsizes.data()), "uwip_png_encode_host");
                else CK(uwip_jpeg_encode_host(ctx, &bt, 95, jstreams.data(), fbytes, jsizes.data()), "uwip_jpeg_encode_host");
            }
            for (int j = 0; j < B && k * B + j < n; ++j) {
                const size_t i = k * B + j;
                char name[512];
                std::snprintf(name, sizeof name, "%s%04zu.%s", OutputFile.c_str(), i, ext);
                bool written = false;
                if (device_jpeg && jsizes[j] > 0) {
                    FILE *jf = std::fopen(name, "wb");
                    written = jf && std::fwrite(jstreams.data() + fbytes * j, 1, (size_t)jsizes[j], jf) == (size_t)jsizes[j];
                    if (jf) std::fclose(jf);
                    if (!written) { std::printf("cannot write %s\n", name); rc = UWIP_ERR_INVALID; what = "writing"; goto fail; }
                } else if (device_jpeg) {
                    std::printf("\nframe %zu: its stream (%lld bytes) exceeds the slot, encoded on the host\n", i, (long long)-jsizes[j]);
                }
                imgio::Image out;
                if (!written) {
                    if (!have_out) { CK(uwip_memcpy_d2h(ctx, h_out, d_out, fbytes * B), "uwip_memcpy_d2h"); have_out = true; }
                    out.rows = rows; out.cols = cols; out.channels = 3;
                    out.data.assign((uint8_t *)h_out + fbytes * j, (uint8_t *)h_out + fbytes * (j + 1));
                }
                if (!written && !imgio::imwrite(name, out)) { std::printf("cannot write %s\n", name); rc = UWIP_ERR_INVALID; what = "writing"; goto fail; }
                if (strip.on) {
                    if (!have_out) { CK(uwip_memcpy_d2h(ctx, h_out, d_out, fbytes * B), "uwip_memcpy_d2h"); have_out = true; }
                    recent.emplace_back(i, std::vector<uint8_t>((uint8_t *)h_out + fbytes * j, (uint8_t *)h_out + fbytes * (j + 1)));
                    while (recent.size() > keep) recent.pop_front();
                }
                // frame 0 is its own key frame (main.cpp:284-297): its row carries the self-overlap
                report << i << "\t" << name << "\t" << ((float *)h_ratio)[j] << "\t" << bs[j] << "\t" << cl[j] << "\n";
            }
            // the rows are read every `kread` batches and after the last one (each read drains the stream): at most B + 1 rows
            // close per batch, so the ring (max_rows) never holds more than half of its capacity unread
            const bool read_rows = kf && (strip.on || (k + 1) % kread == 0 || !more);
            for (int got = (int)krows.size(); read_rows && got == (int)krows.size();) {
                CK(uwip_pipe_keyframes(pipe, krows.data(), (int)krows.size(), &got), "uwip_pipe_keyframes");
                for (int r = 0; r < got; ++r) {
                    const uwip_keyframe_row &w = krows[r];
                    char name[512];
                    std::snprintf(name, sizeof name, "%s%04d.%s", OutputFile.c_str(), w.index, ext);
                    if (w.id == 0) kreport << "0\t0\t" << name << "\t0.0\t0.0\n";              // main.cpp:297
                    else kreport << w.id << "\t" << w.frame << "\t" << name << "\t" << w.overlap << "\t" << w.blur << "\n";   // :381
                    if (strip.on && !strip_add(w.index, name)) { rc = UWIP_ERR_INVALID; what = "--strip"; goto fail; }
                }
            }
            std::printf("\rbatch %zu / %zu", k + 1, nb);
            std::fflush(stdout);
        }
        std::printf("\nEnd of input.\n");
        try { strip.finish(OutputFile, ext, kreport); }
        catch (const uw::Error &e) { std::printf("error: strip: %s\n", e.what()); rc = UWIP_ERR_INVALID; what = "--strip"; goto fail; }
    }
fail:
    if (rc) std::printf("error: %s: %s\n", what, pipe ? uwip_pipe_last_error(pipe) : (ctx ? uwip_last_error(ctx) : "no context"));
    uwip_pipe_destroy(pipe);
    if (ctx) {
        for (int s = 0; s < 2; ++s) uwip_host_free(ctx, h_in[s]);
        uwip_host_free(ctx, h_out);
        uwip_host_free(ctx, h_ratio);
        uwip_free(ctx, d_in); uwip_free(ctx, d_out); uwip_free(ctx, d_ratio);
        uwip_ctx_destroy(ctx);
    }
    return rc ? EXIT_FAILURE : 0;
}
