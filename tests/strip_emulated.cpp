// The kernels of uwimageproc_amd/csrc/strip.hip executed on the host, thread for thread: one std::thread per GPU thread, a
// barrier for __syncthreads, workgroups one after another.  tests/test_strip_emulated.py cuts the kernels out of the .hip file
// into kernels.inc (everything inside its anonymous namespace), builds this file with the host compiler under
// -fsanitize=address,undefined -ffp-contract=off, writes a case into a file, runs this program on it and compares what it
// writes with the numpy mirror (tests/_strip_mirror.py).  It checks the kernels' logic where there is no device; the GPU
// tests check the compiled kernels.
//   usage: strip_emulated <case.in> <case.out> <all|rotate>
//   in :  int32 n, h, w, max_rows, max_cols; float32 max_scale; f64 H[n][9]; f32 ratio[n]; u8 frames[n][h][w][3]
//   out:  int32 nseg; int32 segs[nseg][8]; f64 G[n][9], Ginv[n][9]; int32 seg[n], box[n][4];
//         per segment, per mode 0..2: u8 canvas[rows][cols][3], u8 cover[rows][cols]
// Every render goes into a canary-filled buffer in one of three placements (16-byte aligned, 4-byte aligned, odd), which
// select the three write-out bodies; "all" renders each (segment, mode) in all three and wants them equal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include "uwip.h"
#include "strip_core.hpp"
#include "hip_on_host.hpp"
#include "kernels.inc"

static int g_bad = 0;
static void expect(bool ok, const char *what) { if (!ok) { ++g_bad; std::printf("FAIL: %s\n", what); } }

template <class T> static void rd(FILE *f, T *p, size_t n) { if (std::fread(p, sizeof(T), n, f) != n) { std::printf("short read\n"); std::exit(2); } }
template <class T> static void wr(FILE *f, const T *p, size_t n) { if (std::fwrite(p, sizeof(T), n, f) != n) { std::printf("short write\n"); std::exit(2); } }

struct Placed { std::vector<uint8_t> buf; uint8_t *data; size_t step; int32_t vec; };
static const uint8_t kCanary = 0xA5;
static const size_t kGuard = 512;

// placement 0: base and step multiples of 16; 1: of 4 only; 2: odd base, odd step
static Placed place(int rows, int rowbytes, int placement)
{
    Placed p;
    const size_t r16 = ((size_t)rowbytes + 15) / 16 * 16;
    const size_t res = placement == 0 ? 0 : (placement == 1 ? 4 : 5);
    p.step = placement == 0 ? r16 + 16 : (placement == 1 ? r16 + 4 : (size_t)rowbytes + ((rowbytes + 13) % 2 ? 13 : 14));
    p.vec = placement == 0 ? 16 : (placement == 1 ? 4 : 1);
    p.buf.assign(kGuard + 32 + p.step * rows + kGuard, kCanary);
    uintptr_t a = (uintptr_t)p.buf.data() + kGuard;
    a = (a + 15) / 16 * 16 + res;
    p.data = (uint8_t *)a;
    return p;
}
static void check_canary(const Placed &p, int rows, int rowbytes)
{
    const size_t off = p.data - p.buf.data();
    size_t bad = 0;
    for (size_t i = 0; i < p.buf.size(); ++i) {
        bool inside = false;
        if (i >= off) { const size_t r = (i - off) / p.step, x = (i - off) % p.step; inside = r < (size_t)rows && x < (size_t)rowbytes; }
        if (!inside && p.buf[i] != kCanary) ++bad;
    }
    expect(bad == 0, "bytes outside the canvas rows were written");
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const bool all = std::string(argv[3]) == "all";
    FILE *fi = std::fopen(argv[1], "rb"), *fo = std::fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t hd[5]; float max_scale;
    rd(fi, hd, 5); rd(fi, &max_scale, 1);
    const int32_t n = hd[0], h = hd[1], w = hd[2];
    std::vector<double> H(9 * (size_t)n), G(9 * (size_t)n, NAN), Ginv(9 * (size_t)n, NAN), fb(4 * (size_t)n);
    std::vector<float> ratio(n);
    std::vector<uint8_t> given((size_t)n * h * w * 3), store(given.size(), 0);
    std::vector<int32_t> seg(n, -1), box(4 * (size_t)n, -1);
    std::vector<uwip_strip_segment> segs(n);
    int32_t nseg = -1;
    rd(fi, H.data(), H.size()); rd(fi, ratio.data(), ratio.size()); rd(fi, given.data(), given.size());
    std::fclose(fi);

    // k_strip_store: the frames as given (here: rows 7 bytes apart more than they need) into the packed store
    {
        const int32_t rowbytes = w * 3;
        const size_t step = (size_t)rowbytes + 7, fs = step * h + 3;
        std::vector<uint8_t> src(fs * n + 16, kCanary);
        for (int f = 0; f < n; ++f) for (int y = 0; y < h; ++y) std::memcpy(&src[f * fs + y * step], &given[((size_t)f * h + y) * rowbytes], rowbytes);
        const uint8_t *s = src.data(); uint8_t *d = store.data();
        for (int f = 0; f < n; ++f) {
            blockIdx.z = (unsigned)f;
            launch(uwip_cdiv((size_t)rowbytes, 256), (unsigned)h, 256, false, [=] { k_strip_store(s, step, fs, h, rowbytes, d); });
        }
        blockIdx.z = 0;
        expect(store == given, "k_strip_store did not reproduce the frames");
    }

    uwip_sm::ChainParams P;
    P.w = w; P.h = h; P.max_rows = hd[3]; P.max_cols = hd[4]; P.max_scale = (double)max_scale;
    uwip_sm::ChainOut o;
    o.G = G.data(); o.Ginv = Ginv.data(); o.seg = seg.data(); o.box = box.data(); o.segs = segs.data(); o.nseg = &nseg;
    {
        const double *pH = H.data(); const float *pr = ratio.data(); double *pfb = fb.data();
        launch(1, 1, 64, false, [=] { k_strip_chain(P, pH, pr, n, o, pfb); });
    }
    expect(nseg >= (n > 0) && nseg <= n, "segment count");
    wr(fo, &nseg, 1); wr(fo, segs.data(), (size_t)nseg);
    wr(fo, G.data(), G.size()); wr(fo, Ginv.data(), Ginv.size()); wr(fo, seg.data(), seg.size()); wr(fo, box.data(), box.size());

    const uint8_t fill[3] = {7, 99, 200};
    for (int32_t si = 0; si < nseg; ++si) {
        const uwip_strip_segment &g = segs[si];
        for (int mode = 0; mode < 3; ++mode) {
            std::vector<uint8_t> first_canvas, first_cover;
            for (int pl = 0; pl < 3; ++pl) {
                if (!all && pl != (si + mode) % 3) continue;
                Placed c = place(g.rows, g.cols * 3, pl), cv = place(g.rows, g.cols, 2);
                cv.step = (size_t)g.cols;                       // the cover plane is packed
                StripRender a;
                a.store = store.data(); a.fstride = (size_t)w * h * 3; a.w = w; a.h = h;
                a.Ginv = Ginv.data(); a.box = box.data(); a.first = g.first; a.count = g.count;
                a.x0 = g.x0; a.y0 = g.y0; a.rows = g.rows; a.cols = g.cols;
                a.canvas = c.data; a.step = c.step; a.cover = cv.data; a.vec = c.vec;
                for (int k = 0; k < 3; ++k) a.fill[k] = fill[k];
                a.fill[3] = 0;
                const unsigned gx = uwip_cdiv((size_t)g.cols, kTileW), gy = uwip_cdiv((size_t)g.rows, kTileH);
                if (mode == UWIP_STRIP_FEATHER) launch(gx, gy, kRenderThreads, true, [=] { k_strip_render<UWIP_STRIP_FEATHER>(a); });
                else if (mode == UWIP_STRIP_FIRST) launch(gx, gy, kRenderThreads, true, [=] { k_strip_render<UWIP_STRIP_FIRST>(a); });
                else launch(gx, gy, kRenderThreads, true, [=] { k_strip_render<UWIP_STRIP_LAST>(a); });
                check_canary(c, g.rows, g.cols * 3);
                check_canary(cv, g.rows, g.cols);
                std::vector<uint8_t> canvas((size_t)g.rows * g.cols * 3), cover((size_t)g.rows * g.cols);
                for (int y = 0; y < g.rows; ++y) {
                    std::memcpy(&canvas[(size_t)y * g.cols * 3], c.data + (size_t)y * c.step, (size_t)g.cols * 3);
                    std::memcpy(&cover[(size_t)y * g.cols], cv.data + (size_t)y * cv.step, (size_t)g.cols);
                }
                if (first_canvas.empty()) { first_canvas = canvas; first_cover = cover; }
                else expect(first_canvas == canvas && first_cover == cover, "the write-out bodies disagree");
            }
            wr(fo, first_canvas.data(), first_canvas.size()); wr(fo, first_cover.data(), first_cover.size());
        }
    }
    std::fclose(fo);
    std::printf("strip emulation: %d segments, %d mismatches\n", nseg, g_bad);
    return g_bad ? 1 : 0;
}
