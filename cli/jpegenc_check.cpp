// jpegenc_check -- the device JPEG encoder (uwip_jpeg_encode_host) against the host codec the CLIs write their files with
// (jpeg::encode, cli/jpeg.hpp): the two streams of an image must be the same bytes.
//   jpegenc_check <image> <quality> [grey] [--out=FILE] [--host-out=FILE] [--time N]
// prints "identical <bytes>", or the first differing offset and exits non-zero.  --out / --host-out keep the two streams (the
// host one is written before the device is touched).
// --time N: both encoders on N copies of the image (the frames already in device memory for the device one, the host one on
// one thread), milliseconds for each, then the device kernels' split from uwip_prof_* (ms per N frames per kernel).
// The two share their tables, header writer and DCT pass (csrc/jpeg_tables.hpp, jpeg_core.hpp); everything else is compared here.
#include <cstdlib>
#include "cliutil.hpp"

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
    const Args a = parse_args(argc, argv, {"time"});
    if (a.pos.size() < 2) { std::printf("usage: jpegenc_check <image> <quality> [grey] [--out=FILE] [--host-out=FILE] [--time N]\n"); return 2; }
    const bool grey = a.pos.size() > 2 && a.pos[2] == "grey";
    const int quality = std::atoi(a.pos[1].c_str());
    imgio::Image im;
    if (!imgio::imread(a.pos[0], im, !grey)) { std::printf("cannot read %s\n", a.pos[0].c_str()); return 1; }
    if (grey && im.channels == 3) {                       // cvtColor(BGR2GRAY)'s weights, 14-bit fixed point
        std::vector<uint8_t> g((size_t)im.rows * im.cols);
        for (size_t i = 0; i < g.size(); ++i)
            g[i] = (uint8_t)((im.data[3 * i] * 1868 + im.data[3 * i + 1] * 9617 + im.data[3 * i + 2] * 4899 + 8192) >> 14);
        im.data.swap(g);
        im.channels = 1;
    }
    const int N = std::max(1, std::atoi(a.get("time", "1").c_str()));
    const size_t fbytes = (size_t)im.rows * im.cols * im.channels;
    std::vector<uint8_t> host;
    if (!jpeg::encode(im.data.data(), im.rows, im.cols, im.channels, quality, host)) { std::printf("host encoder failed\n"); return 1; }
    if (a.has("host-out") && !dump(a.get("host-out", ""), host.data(), host.size())) { std::printf("cannot write --host-out\n"); return 1; }
    try {
        uw::Context ctx(0);
        void *d = nullptr;
        ctx.check(uwip_malloc(ctx.get(), fbytes * N, &d));
        for (int f = 0; f < N; ++f) ctx.check(uwip_memcpy_h2d(ctx.get(), (uint8_t *)d + fbytes * f, im.data.data(), fbytes));
        uwip_batch_u8 bt{};
        bt.data = d; bt.rows = im.rows; bt.cols = im.cols; bt.channels = im.channels; bt.frames = N;
        bt.step = (size_t)im.cols * im.channels; bt.frame_stride = fbytes;
        const size_t slot = uwip_jpeg_bound(im.rows, im.cols, im.channels);
        std::vector<uint8_t> dev(slot * N);
        std::vector<int64_t> sizes(N);
        ctx.check(uwip_jpeg_encode_host(ctx.get(), &bt, quality, dev.data(), slot, sizes.data()));
        if (a.has("out") && sizes[0] > 0 && !dump(a.get("out", ""), dev.data(), (size_t)sizes[0])) { std::printf("cannot write --out\n"); return 1; }
        for (int f = 0; f < N; ++f) {
            const uint8_t *s = dev.data() + slot * f;
            if (sizes[f] < 0) { std::printf("frame %d: does not fit uwip_jpeg_bound: needs %lld bytes\n", f, (long long)-sizes[f]); return 1; }
            const size_t n = std::min((size_t)sizes[f], host.size());
            for (size_t i = 0; i < n; ++i)
                if (s[i] != host[i]) {
                    std::printf("frame %d: differs at offset %zu: device %02x, host %02x (lengths %lld, %zu)\n", f, i, s[i], host[i],
                                (long long)sizes[f], host.size());
                    return 1;
                }
            if ((size_t)sizes[f] != host.size()) {
                std::printf("frame %d: differs at offset %zu: lengths %lld (device), %zu (host)\n", f, n, (long long)sizes[f], host.size());
                return 1;
            }
        }
        std::printf("identical %zu\n", host.size());
        if (a.has("time")) {
            std::vector<uint8_t> tmp;
            Stopwatch hw;
            for (int f = 0; f < N; ++f) jpeg::encode(im.data.data(), im.rows, im.cols, im.channels, quality, tmp);
            const double host_ms = hw.ms();
            const size_t tslot = fbytes;                              // the slot uwpipe uses
            double dev_ms = 0;
            for (int rep = 0; rep < 3; ++rep) {                       // the last of three (the first ones warm up and allocate)
                Stopwatch dw;
                ctx.check(uwip_jpeg_encode_host(ctx.get(), &bt, quality, dev.data(), tslot, sizes.data()));
                dev_ms = dw.ms();
            }
            std::printf("frames %d  host_1thread_ms %.3f  device_ms %.3f\n", N, host_ms, dev_ms);
            ctx.check(uwip_prof_enable(ctx.get(), 1));
            ctx.check(uwip_prof_reset(ctx.get()));
            ctx.check(uwip_jpeg_encode_host(ctx.get(), &bt, quality, dev.data(), tslot, sizes.data()));
            int np = 0;
            ctx.check(uwip_prof_count(ctx.get(), &np));
            for (int i = 0; i < np; ++i) {
                char name[128];
                double ms = 0;
                uint64_t launches = 0;
                ctx.check(uwip_prof_get(ctx.get(), i, name, sizeof name, &ms, &launches));
                std::printf("kernel %s ms %.4f\n", name, ms);
            }
        }
        uwip_free(ctx.get(), d);
    } catch (const uw::Error &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
