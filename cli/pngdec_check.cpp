// pngdec_check -- the device PNG decoder (uwip_png_decode_host) against the host reader the CLIs read their files with
// (imgio::read_png, cli/imgio.hpp): the two decodes of every frame must be the same bytes.
//   pngdec_check <file.png | list.txt> [grey] [--segmented N [--chunk-bytes C]] [--frames B] [--time N]
// prints "identical <frames>", or the first difference and exits non-zero.  A frame the host reader rejects must have the
// status UWIP_PNG_BAD_STREAM, a frame whose IHDR has another size than the first readable one UWIP_PNG_SIZE_MISMATCH.  grey: a 1-channel
// batch.  --segmented N: uwip_png_decode_opts::segmented (default -1, the library's choice); --chunk-bytes C: its chunk_bytes, with
// --segmented 2.  list.txt: one file per line.
// --frames B: a .png file B times, as a batch of B frames.
// --time N: the batch N times after a warm-up: the median wall milliseconds of uwip_png_decode_host (parse, upload, kernels,
// wait), the counts of the two inflate passes, then N profiled calls: the median of the sum of the kernels' HIP-event times
// (uwip_prof_*) and that call's split, and imgio::read_png of the same batch on 1 and on 16 host threads.
#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <string>
#include <utility>
#include <thread>
#include "cliutil.hpp"

int main(int argc, char **argv)
{
    const Args a = parse_args(argc, argv, {"time", "segmented", "frames", "chunk-bytes"});
    if (a.pos.empty()) { std::printf("usage: pngdec_check <file.png | list.txt> [grey] [--segmented N [--chunk-bytes C]] [--frames B] [--time N]\n"); return 2; }
    const bool grey = a.pos.size() > 1 && a.pos[1] == "grey";
    const int channels = grey ? 1 : 3;
    const std::string &path = a.pos[0];
    std::vector<std::vector<uint8_t>> files;
    std::vector<const uint8_t *> ptr;
    std::vector<size_t> len;
    if (imgio::ends_with(path, ".txt")) {
        std::ifstream f(path);
        std::string l;
        while (std::getline(f, l)) {
            if (l.empty()) continue;
            files.emplace_back();
            if (!imgio::read_file(l, files.back())) { std::printf("cannot read %s\n", l.c_str()); return 1; }
        }
        for (auto &v : files) { ptr.push_back(v.data()); len.push_back(v.size()); }
    } else {
        files.emplace_back();
        if (!imgio::read_file(path, files[0])) { std::printf("cannot read %s\n", path.c_str()); return 1; }
        const int B = std::max(1, std::atoi(a.get("frames", "1").c_str()));
        for (int f = 0; f < B; ++f) { ptr.push_back(files[0].data()); len.push_back(files[0].size()); }
    }
    const int n = (int)ptr.size();
    if (n == 0) { std::printf("no frames\n"); return 1; }
    // the host side: every frame, and the size of the batch from the first frame the host reads
    std::vector<imgio::Image> host(n);
    std::vector<char> host_ok(n, 0);
    int rows = 0, cols = 0;
    for (int f = 0; f < n; ++f) {
        if (f > 0 && ptr[f] == ptr[0]) { host[f] = host[0]; host_ok[f] = host_ok[0]; continue; }
        host_ok[f] = imgio::read_png(files[f], host[f], !grey);
        if (host_ok[f] && host[f].channels != channels) { std::printf("frame %d: a colour stream, and a 1-channel batch was asked for\n", f); return 1; }
        if (host_ok[f] && rows == 0) { rows = host[f].rows; cols = host[f].cols; }
    }
    if (rows == 0) { rows = cols = 8; }
    const size_t fbytes = (size_t)rows * cols * channels;
    try {
        uw::Context ctx(0);
        void *d = nullptr, *d_uns = nullptr;
        ctx.check(uwip_malloc(ctx.get(), fbytes * n, &d));
        ctx.check(uwip_malloc(ctx.get(), 24, &d_uns));
        uwip_batch_u8 bt{};
        bt.data = d; bt.rows = rows; bt.cols = cols; bt.channels = channels; bt.frames = n;
        bt.step = (size_t)cols * channels; bt.frame_stride = fbytes;
        uwip_png_decode_opts opts{};
        opts.segmented = std::atoi(a.get("segmented", "-1").c_str());
        opts.chunk_bytes = std::atoi(a.get("chunk-bytes", "0").c_str());
        opts.d_counts = (uint64_t *)d_uns;
        std::vector<int32_t> status(n, 0);
        ctx.check(uwip_png_decode_host(ctx.get(), ptr.data(), len.data(), n, &bt, &opts, status.data()));
        std::vector<uint8_t> dev(fbytes * n);
        ctx.check(uwip_memcpy_d2h(ctx.get(), dev.data(), d, fbytes * n));
        for (int f = 0; f < n; ++f) {
            if (!host_ok[f]) {
                // an IHDR of another size than the batch's is not inflated on the device: a size mismatch whatever the stream holds
                int32_t ir = 0, ic = 0, ich = 0;
                const bool other = uwip_png_info(ptr[f], len[f], &ir, &ic, &ich) == UWIP_OK && (ir != rows || ic != cols);
                if (status[f] != (other ? UWIP_PNG_SIZE_MISMATCH : UWIP_PNG_BAD_STREAM)) {
                    std::printf("frame %d: the host reader rejects it, device status %d\n", f, status[f]);
                    return 1;
                }
                continue;
            }
            if (host[f].rows != rows || host[f].cols != cols) {
                if (status[f] != UWIP_PNG_SIZE_MISMATCH) { std::printf("frame %d: differs in size from the batch, device status %d\n", f, status[f]); return 1; }
                continue;
            }
            if (status[f] != 0) { std::printf("frame %d: device status %d, the host reader reads it\n", f, status[f]); return 1; }
            const uint8_t *s = dev.data() + fbytes * f;
            for (size_t i = 0; i < fbytes; ++i)
                if (s[i] != host[f].data[i]) {
                    std::printf("frame %d: differs at byte %zu (row %zu, column %zu): device %d, host %d\n", f, i, i / bt.step, (i % bt.step) / channels,
                                s[i], host[f].data[i]);
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
                        imgio::Image im;
                        for (int f = t; f < n; f += threads) imgio::read_png(files[ptr[f] == ptr[0] ? 0 : f], im, !grey);
                    });
                for (auto &t : th) t.join();
                return w.ms();
            };
            const double h1 = host_batch(1), h16 = host_batch(16);
            std::vector<double> wall;
            for (int rep = 0; rep < N + 2; ++rep) {
                Stopwatch w;
                ctx.check(uwip_png_decode_host(ctx.get(), ptr.data(), len.data(), n, &bt, &opts, status.data()));
                if (rep >= 2) wall.push_back(w.ms());
            }
            std::sort(wall.begin(), wall.end());
            uint64_t uns[3] = {0, 0, 0};
            ctx.check(uwip_memcpy_d2h(ctx.get(), uns, d_uns, 24));
            std::printf("frames %d  segmented %d  host_1thread_ms %.3f  host_16threads_ms %.3f  device_wall_ms_median %.3f\n", n, opts.segmented, h1, h16,
                        wall[wall.size() / 2]);
            std::printf("units_accepted %llu  serial_frames %llu  frames %llu\n", (unsigned long long)uns[0], (unsigned long long)uns[1],
                        (unsigned long long)uns[2]);
            // the kernels' HIP-event times: the median over N profiled calls of their sum, and the split of the median call
            ctx.check(uwip_prof_enable(ctx.get(), 1));
            std::vector<std::pair<double, std::string>> runs;
            for (int rep = 0; rep < N; ++rep) {
                ctx.check(uwip_prof_reset(ctx.get()));
                ctx.check(uwip_png_decode_host(ctx.get(), ptr.data(), len.data(), n, &bt, &opts, status.data()));
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
