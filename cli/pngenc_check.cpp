// pngenc_check -- the device PNG encoder (uwip_png_encode_host) read back with the host PNG reader (imgio::read_png): the pixels
// must be the image's, and the stream must be the serial reference encoder's (csrc/png_reference.hpp) byte for byte.
//   pngenc_check <image> [grey] [--filter N] [--out=FILE] [--ref-out=FILE] [--time N]
// prints "lossless <device bytes> host_writer <bytes> ratio <device / host writer>", or what differs and exits non-zero.
// --out keeps the device stream, --ref-out the reference encoder's (written before the device is touched).
// --time N: the encoder on N copies of the image already in device memory (ms per batch, then the kernels' split from
// uwip_prof_*), against imgio::imwrite's PNG path (filter 0, compress2 level 3) on one thread, and that time divided by 16.
#include <cstdlib>
#include <zlib.h>
#include "cliutil.hpp"
#include "png_reference.hpp"

static bool dump(const std::string &path, const uint8_t *p, size_t n)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, n, f) == n;
    std::fclose(f);
    return ok;
}

// the bytes imgio::imwrite's PNG path puts into its IDAT, and the file size that follows from them
static size_t host_writer_bytes(const imgio::Image &im)
{
    const size_t rb = (size_t)im.cols * im.channels;
    std::vector<uint8_t> raw((rb + 1) * im.rows);
    for (int y = 0; y < im.rows; ++y) {
        uint8_t *r = &raw[(size_t)y * (rb + 1)];
        r[0] = 0;
        for (int x = 0; x < im.cols; ++x) {
            const uint8_t *p = &im.data[((size_t)y * im.cols + x) * im.channels];
            if (im.channels == 1) r[1 + x] = p[0];
            else { r[1 + 3 * x] = p[2]; r[2 + 3 * x] = p[1]; r[3 + 3 * x] = p[0]; }
        }
    }
    uLongf zl = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(zl);
    if (compress2(z.data(), &zl, raw.data(), (uLong)raw.size(), 3) != Z_OK) return 0;
    return 8 + 25 + 12 + (size_t)zl + 12;
}

int main(int argc, char **argv)
{
    const Args a = parse_args(argc, argv, {"time", "filter"});
    if (a.pos.empty()) { std::printf("usage: pngenc_check <image> [grey] [--filter N] [--out=FILE] [--ref-out=FILE] [--time N]\n"); return 2; }
    const bool grey = a.pos.size() > 1 && a.pos[1] == "grey";
    const int filter = std::atoi(a.get("filter", "-1").c_str());
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
    std::vector<uint8_t> ref;
    uwip_png::encode_host_reference(im.data.data(), im.rows, im.cols, im.channels, (size_t)im.cols * im.channels, filter, ref);
    if (a.has("ref-out") && !dump(a.get("ref-out", ""), ref.data(), ref.size())) { std::printf("cannot write --ref-out\n"); return 1; }
    const size_t hw = host_writer_bytes(im);
    try {
        uw::Context ctx(0);
        void *d = nullptr;
        ctx.check(uwip_malloc(ctx.get(), fbytes * N, &d));
        for (int f = 0; f < N; ++f) ctx.check(uwip_memcpy_h2d(ctx.get(), (uint8_t *)d + fbytes * f, im.data.data(), fbytes));
        uwip_batch_u8 bt{};
        bt.data = d; bt.rows = im.rows; bt.cols = im.cols; bt.channels = im.channels; bt.frames = N;
        bt.step = (size_t)im.cols * im.channels; bt.frame_stride = fbytes;
        const size_t slot = uwip_png_bound(im.rows, im.cols, im.channels);
        std::vector<uint8_t> dev(slot * N);
        std::vector<int64_t> sizes(N);
        ctx.check(uwip_png_encode_host(ctx.get(), &bt, filter, dev.data(), slot, sizes.data()));
        if (a.has("out") && sizes[0] > 0 && !dump(a.get("out", ""), dev.data(), (size_t)sizes[0])) { std::printf("cannot write --out\n"); return 1; }
        for (int f = 0; f < N; ++f) {
            if (sizes[f] < 0) { std::printf("frame %d: does not fit uwip_png_bound: needs %lld bytes\n", f, (long long)-sizes[f]); return 1; }
            const std::vector<uint8_t> s(dev.begin() + slot * f, dev.begin() + slot * f + (size_t)sizes[f]);
            imgio::Image back;
            if (!imgio::read_png(s, back, !grey && im.channels == 3) || back.rows != im.rows || back.cols != im.cols ||
                back.channels != im.channels || back.data != im.data) {
                std::printf("frame %d: the stream does not decode to the image's pixels\n", f);
                return 1;
            }
            if (s != ref) { std::printf("frame %d: differs from the reference encoder's stream (lengths %zu, %zu)\n", f, s.size(), ref.size()); return 1; }
        }
        std::printf("lossless %lld host_writer %zu ratio %.4f\n", (long long)sizes[0], hw, (double)sizes[0] / (double)hw);
        if (a.has("time")) {
            Stopwatch hwatch;
            size_t sink = 0;
            for (int f = 0; f < N; ++f) sink += host_writer_bytes(im);
            const double host_ms = hwatch.ms();
            const size_t tslot = fbytes + 1024;                       // the slot uwpipe uses
            double dev_ms = 0;
            for (int rep = 0; rep < 3; ++rep) {                       // the last of three (the first ones warm up and allocate)
                Stopwatch dw;
                ctx.check(uwip_png_encode_host(ctx.get(), &bt, filter, dev.data(), tslot, sizes.data()));
                dev_ms = dw.ms();
            }
            std::printf("frames %d  host_1thread_ms %.3f  host_over_16_ms %.3f  device_ms %.3f  (%zu)\n", N, host_ms, host_ms / 16, dev_ms, sink);
            ctx.check(uwip_prof_enable(ctx.get(), 1));
            ctx.check(uwip_prof_reset(ctx.get()));
            ctx.check(uwip_png_encode_host(ctx.get(), &bt, filter, dev.data(), tslot, sizes.data()));
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
