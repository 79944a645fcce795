// The multi-band kernels of uwimageproc_amd/csrc/strip.hip executed on the host, thread for thread, as tests/strip_emulated.cpp
// runs the strip's other kernels: k_strip_chain, then k_strip_stack once per level over every (tile, frame), then
// k_strip_render_bands<false> and <true> over every segment.  tests/test_strip_band_emulated.py cuts the kernels into
// kernels.inc, builds this file under -fsanitize=address,undefined -ffp-contract=off, runs it on a case and compares what it
// writes with the numpy mirror (tests/_strip_band_mirror.py).  Every array is a heap block of its exact size, so the address
// sanitizer sees an index one past any of them.
//   usage: strip_band_emulated <case.in> <case.out>
//   in :  int32 n, h, w, max_rows, max_cols; float32 max_scale; int32 levels, ramp[4]; f64 H[n][9]; f32 ratio[n];
//         int32 gq[n][3]; u8 frames[n][h][w][3]
//   out:  int32 nseg; int32 segs[nseg][8]; u8 stack[levels][n][h][w][3];
//         per segment, ungained then gained: u8 canvas[rows][cols][3], u8 cover[rows][cols]
// Every render goes into a canary-filled buffer; the placement (16-byte aligned, 4-byte aligned, odd) rotates with the segment
// and the instantiation.
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
    if (argc < 3) return 2;
    FILE *fi = std::fopen(argv[1], "rb"), *fo = std::fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t hd[5], bp[5]; float fl[1];
    rd(fi, hd, 5); rd(fi, fl, 1); rd(fi, bp, 5);
    const int32_t n = hd[0], h = hd[1], w = hd[2], levels = bp[0];
    const size_t fstride = (size_t)w * h * 3;
    std::vector<double> H(9 * (size_t)n), G(9 * (size_t)n, NAN), Ginv(9 * (size_t)n, NAN), fb(4 * (size_t)n);
    std::vector<float> ratio(n);
    std::vector<int32_t> seg(n, -1), box(4 * (size_t)n, -1), gq(3 * (size_t)n);
    std::vector<uwip_strip_segment> segs(n);
    int32_t nseg = -1;
    // the frames and the stacks are heap blocks of their exact sizes (operator new: aligned to 16 bytes, as the device's are)
    std::vector<uint8_t> store(fstride * n), bands(fstride * n * levels, 0xDD);
    rd(fi, H.data(), H.size()); rd(fi, ratio.data(), ratio.size()); rd(fi, gq.data(), gq.size()); rd(fi, store.data(), store.size());
    std::fclose(fi);

    uwip_sm::ChainParams P;
    P.w = w; P.h = h; P.max_rows = hd[3]; P.max_cols = hd[4]; P.max_scale = (double)fl[0];
    uwip_sm::ChainOut o;
    o.G = G.data(); o.Ginv = Ginv.data(); o.seg = seg.data(); o.box = box.data(); o.segs = segs.data(); o.nseg = &nseg;
    {
        const double *pH = H.data(); const float *pr = ratio.data(); double *pfb = fb.data();
        launch(1, 1, 64, false, [=] { k_strip_chain(P, pH, pr, n, o, pfb); });
    }
    expect(nseg >= (n > 0) && nseg <= n, "segment count");
    wr(fo, &nseg, 1); wr(fo, segs.data(), (size_t)nseg);

    // the stacks: one launch per level over (tiles, frames), as uwip_strip_bands queues them
    for (int l = 0; l < levels; ++l) {
        StripStack a;
        a.in = l == 0 ? store.data() : bands.data() + (size_t)(l - 1) * fstride * n;
        a.out = bands.data() + (size_t)l * fstride * n;
        a.fstride = fstride; a.w = w; a.h = h; a.s = 1 << l;
        a.tiles_x = (int32_t)uwip_cdiv((size_t)w, kTileW);
        a.vec = (w * 3) % 4 == 0 ? 4 : 1;
        launch((unsigned)a.tiles_x * uwip_cdiv((size_t)h, kTileH), (unsigned)n, kRenderThreads, true, [=] { k_strip_stack(a); });
    }
    wr(fo, bands.data(), bands.size());

    const uint8_t fill[3] = {7, 99, 200};
    for (int32_t si = 0; si < nseg; ++si) {
        const uwip_strip_segment &sg = segs[si];
        for (int gain = 0; gain < 2; ++gain) {
            Placed c = place(sg.rows, sg.cols * 3, (si + gain) % 3), cv = place(sg.rows, sg.cols, 2);
            cv.step = (size_t)sg.cols;                       // the cover plane is packed
            StripBands b;
            StripRender &a = b.r;
            a.store = store.data(); a.fstride = fstride; a.w = w; a.h = h;
            a.Ginv = Ginv.data(); a.box = box.data(); a.first = sg.first; a.count = sg.count;
            a.x0 = sg.x0; a.y0 = sg.y0; a.rows = sg.rows; a.cols = sg.cols;
            a.canvas = c.data; a.step = c.step; a.cover = cv.data; a.vec = c.vec;
            a.gq = gain ? gq.data() : nullptr;
            for (int k = 0; k < 3; ++k) a.fill[k] = fill[k];
            a.fill[3] = 0;
            b.bands = bands.data(); b.lstride = fstride * n;
            b.P.levels = levels;
            for (int l = 0; l < 4; ++l) b.P.ramp[l] = bp[1 + l];
            const unsigned gx = uwip_cdiv((size_t)sg.cols, kTileW), gy = uwip_cdiv((size_t)sg.rows, kBandTileH);
            if (gain) launch(gx, gy, kRenderThreads, true, [=] { k_strip_render_bands<true>(b); });
            else launch(gx, gy, kRenderThreads, true, [=] { k_strip_render_bands<false>(b); });
            check_canary(c, sg.rows, sg.cols * 3);
            check_canary(cv, sg.rows, sg.cols);
            std::vector<uint8_t> canvas((size_t)sg.rows * sg.cols * 3), cover((size_t)sg.rows * sg.cols);
            for (int y = 0; y < sg.rows; ++y) {
                std::memcpy(&canvas[(size_t)y * sg.cols * 3], c.data + (size_t)y * c.step, (size_t)sg.cols * 3);
                std::memcpy(&cover[(size_t)y * sg.cols], cv.data + (size_t)y * cv.step, (size_t)sg.cols);
            }
            wr(fo, canvas.data(), canvas.size()); wr(fo, cover.data(), cover.size());
        }
    }
    std::fclose(fo);
    std::printf("strip band emulation: %d segments, %d mismatches\n", nseg, g_bad);
    return g_bad ? 1 : 0;
}
