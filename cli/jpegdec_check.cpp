// jpegdec_check -- the device JPEG decoder (uwip_jpeg_decode_host) against the host codec the CLIs read their files with
// (jpeg::decode, cli/jpeg.hpp): the two decodes of every frame must be the same bytes.
//   jpegdec_check <file.jpg | file.avi> [grey] [--rounds N] [--frames B] [--out=FILE] [--host-out=FILE] [--time N]
// prints "identical <frames>", or the first difference and exits non-zero.  A frame the host decoder rejects must have the
// status UWIP_JPEG_BAD_STREAM; a frame with UWIP_JPEG_HOST_ONLY is reported and counts as a difference.  grey: a 1-channel
// batch.  --rounds N: uwip_jpeg_decode_opts::sync_rounds (default -1, the library's choice).  --out / --host-out keep the
// raw pixels of frame 0 (the host ones are written before the device is touched).  --frames B: a .jpg file B times, as a
// batch of B frames.
// --time N: the batch N times after a warm-up: the median wall milliseconds of uwip_jpeg_decode_host (parse, upload, kernels,
// wait), then N profiled calls: the median of the sum of the kernels' HIP-event times (uwip_prof_*) and that call's split, the subsequences still unsettled
// after the sync rounds, and jpeg::decode of the same batch on 1 and on 16 host threads.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <utility>
#include <thread>
#include "cliutil.hpp"
#include "avi.hpp"

static bool dump(const std::string &path, const uint8_t *p, size_t n)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, n, f) == n;
    std::fclose(f);
    return ok;
}


int main(int argc, char **argv)
{
    const Args a = parse_args(argc, argv, {"time", "rounds", "frames"});
    if (a.pos.empty()) { std::printf("usage: jpegdec_check <file.jpg | file.avi> [grey] [--rounds N] [--frames B] [--out=FILE] [--host-out=FILE] [--time N]\n"); return 2; }
    const bool grey = a.pos.size() > 1 && a.pos[1] == "grey";
    const int channels = grey ? 1 : 3;
    const std::string &path = a.pos[0];
    const bool is_avi = path.size() > 4 && (path.substr(path.size() - 4) == ".avi" || path.substr(path.size() - 4) == ".AVI");
    std::vector<uint8_t> file;
    std::vector<const uint8_t *> ptr;
    std::vector<size_t> len;
    avi::Reader rd;
    if (is_avi) {
        if (!rd.open(path)) { std::printf("cannot read %s\n", path.c_str()); return 1; }
        for (auto &fr : rd.frames) { ptr.push_back(&rd.buf[fr.first]); len.push_back(fr.second); }
    } else {
        if (!imgio::read_file(path, file)) { std::printf("cannot read %s\n", path.c_str()); return 1; }
        const int B = std::max(1, std::atoi(a.get("frames", "1").c_str()));
        for (int f = 0; f < B; ++f) { ptr.push_back(file.data()); len.push_back(file.size()); }
    }
    const int n = (int)ptr.size();
    // the host side: every frame, and the size of the batch from the first frame the host decodes
    std::vector<std::vector<uint8_t>> host(n);
    std::vector<char> host_ok(n, 0);
    int rows = 0, cols = 0;
    for (int f = 0; f < n; ++f) {
        int r = 0, c = 0, ch = 0;
        if (f > 0 && ptr[f] == ptr[0]) { host[f] = host[0]; host_ok[f] = host_ok[0]; continue; }
        host_ok[f] = jpeg::decode(ptr[f], len[f], r, c, ch, host[f], !grey);
        if (host_ok[f] && grey && ch != 1) { std::printf("frame %d: a colour stream, and a 1-channel batch was asked for\n", f); return 1; }
        if (host_ok[f] && rows == 0) { rows = r; cols = c; }
    }
    if (rows == 0) { rows = cols = 8; }
    if (a.has("host-out") && host_ok[0] && !dump(a.get("host-out", ""), host[0].data(), host[0].size())) { std::printf("cannot write --host-out\n"); return 1; }
    const size_t fbytes = (size_t)rows * cols * channels;
    try {
        uw::Context ctx(0);
        void *d = nullptr, *d_uns = nullptr;
        ctx.check(uwip_malloc(ctx.get(), fbytes * n, &d));
        ctx.check(uwip_malloc(ctx.get(), 16, &d_uns));
        uwip_batch_u8 bt{};
        bt.data = d; bt.rows = rows; bt.cols = cols; bt.channels = channels; bt.frames = n;
        bt.step = (size_t)cols * channels; bt.frame_stride = fbytes;
        uwip_jpeg_decode_opts opts{};
        opts.sync_rounds = std::atoi(a.get("rounds", "-1").c_str());
        opts.d_unsettled = (uint64_t *)d_uns;
        std::vector<int32_t> status = uw::imdecode_jpeg(ctx, ptr, len, bt, opts.sync_rounds);
        std::vector<uint8_t> dev(fbytes * n);
        ctx.check(uwip_memcpy_d2h(ctx.get(), dev.data(), d, fbytes * n));
        if (a.has("out") && !dump(a.get("out", ""), dev.data(), fbytes)) { std::printf("cannot write --out\n"); return 1; }
        for (int f = 0; f < n; ++f) {
            if (!host_ok[f]) {
                if (status[f] != UWIP_JPEG_BAD_STREAM) { std::printf("frame %d: the host decoder rejects it, device status %d\n", f, status[f]); return 1; }
                continue;
            }
            if (status[f] != 0) { std::printf("frame %d: device status %d, the host decoder reads it\n", f, status[f]); return 1; }
            if (host[f].size() != fbytes) { std::printf("frame %d: differs in size from the batch\n", f); return 1; }
            const uint8_t *s = dev.data() + fbytes * f;
            for (size_t i = 0; i < fbytes; ++i)
                if (s[i] != host[f][i]) {
                    std::printf("frame %d: differs at byte %zu (row %zu, column %zu): device %d, host %d\n", f, i, i / bt.step, (i % bt.step) / channels,
                                s[i], host[f][i]);
                    return 1;
                }
        }
        std::printf("identical %d\n", n);
        if (a.has("time")) {
            const int N = std::max(1, std::atoi(a.get("time", "1").c_str()));
            auto host_batch = [&](int threads) {
                Stopwatch w;
                std::vector<std::thread> th;
                for (int t = 0; t < threads; ++t)
                    th.emplace_back([&, t] {
                        std::vector<uint8_t> pix;
                        int r, c, ch;
                        for (int f = t; f < n; f += threads) jpeg::decode(ptr[f], len[f], r, c, ch, pix, !grey);
                    });
                for (auto &t : th) t.join();
                return w.ms();
            };
            const double h1 = host_batch(1), h16 = host_batch(16);
            std::vector<double> wall;
            for (int rep = 0; rep < N + 2; ++rep) {
                Stopwatch w;
                ctx.check(uwip_jpeg_decode_host(ctx.get(), ptr.data(), len.data(), n, &bt, &opts, status.data()));
                if (rep >= 2) wall.push_back(w.ms());
            }
            std::sort(wall.begin(), wall.end());
            uint64_t uns[2] = {0, 0};
            ctx.check(uwip_memcpy_d2h(ctx.get(), uns, d_uns, 16));
            std::printf("frames %d  rounds %d  host_1thread_ms %.3f  host_16threads_ms %.3f  device_wall_ms_median %.3f\n", n, opts.sync_rounds, h1, h16,
                        wall[wall.size() / 2]);
            std::printf("unsettled %llu of %llu subsequences\n", (unsigned long long)uns[0], (unsigned long long)uns[1]);
            // the kernels' HIP-event times: the median over N profiled calls of their sum, and the split of the median call
            ctx.check(uwip_prof_enable(ctx.get(), 1));
            std::vector<std::pair<double, std::string>> runs;
            for (int rep = 0; rep < N; ++rep) {
                ctx.check(uwip_prof_reset(ctx.get()));
                ctx.check(uwip_jpeg_decode_host(ctx.get(), ptr.data(), len.data(), n, &bt, &opts, status.data()));
                int np = 0;
                double sum = 0;
                std::string split;
                ctx.check(uwip_prof_count(ctx.get(), &np));
                for (int i = 0; i < np; ++i) {
                    char name[128], line[256];
                    double ms = 0;
                    uint64_t launches = 0;
                    ctx.check(uwip_prof_get(ctx.get(), i, name, sizeof name, &ms, &launches));
                    std::snprintf(line, sizeof line, "kernel %s ms %.4f launches %llu\n", name, ms, (unsigned long long)launches);
                    split += line;
                    sum += ms;
                }
                runs.emplace_back(sum, split);
            }
            std::sort(runs.begin(), runs.end());
            std::printf("%sdevice_kernels_ms_median %.4f (of %d: min %.4f max %.4f)\n", runs[runs.size() / 2].second.c_str(), runs[runs.size() / 2].first, N,
                        runs.front().first, runs.back().first);
        }
        uwip_free(ctx.get(), d);
        uwip_free(ctx.get(), d_uns);
    } catch (const uw::Error &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
