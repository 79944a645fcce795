// The seam kernels of uwimageproc_amd/csrc/strip.hip executed on the host, thread for thread, as tests/strip_emulated.cpp runs
// the strip's other kernels: k_strip_chain, then per round of pairs k_strip_seam_cost over every (tile, pair) and
// k_strip_seam_path over every pair -- with its back pointers in LDS where they fit, and again with them in global scratch:
// both must agree -- then k_strip_render<UWIP_STRIP_SEAM> (gained or not, as the case says) over every segment.
// tests/test_strip_seam_emulated.py cuts the kernels into kernels.inc, builds this file under -fsanitize=address,undefined
// -ffp-contract=off, runs it on a case and compares what it writes with the numpy mirror (tests/_strip_seam_mirror.py).  Every
// array is a heap block of its exact size, so the address sanitizer sees an index one past any of them.
//   usage: strip_seam_emulated <case.in> <case.out>
//   in :  int32 n, h, w, max_rows, max_cols; float32 max_scale; int32 prior, round, gained; f64 H[n][9]; f32 ratio[n];
//         int32 gq[n][3]; u8 frames[n][h][w][3]
//   out:  int32 nseg; int32 segs[nseg][8]; int32 orient[n]; int32 seam[n][max(w, h)]; u64 total[n];
//         per segment: u8 canvas[rows][cols][3], u8 cover[rows][cols]
// Every render goes into a canary-filled buffer; the placement (16-byte aligned, 4-byte aligned, odd) rotates with the segment.
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
    int32_t hd[5], sp[3]; float fl[1];
    rd(fi, hd, 5); rd(fi, fl, 1); rd(fi, sp, 3);
    const int32_t n = hd[0], h = hd[1], w = hd[2], round = sp[1], L = std::max(w, h);
    const bool gained = sp[2] != 0;
    const size_t fstride = (size_t)w * h * 3, wh = (size_t)w * h;
    std::vector<double> H(9 * (size_t)n), G(9 * (size_t)n, NAN), Ginv(9 * (size_t)n, NAN), fb(4 * (size_t)n);
    std::vector<float> ratio(n);
    std::vector<int32_t> seg(n, -1), box(4 * (size_t)n, -1), gq(3 * (size_t)n);
    std::vector<uwip_strip_segment> segs(n);
    int32_t nseg = -1;
    std::vector<uint8_t> store(fstride * n);
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

    // the seams, as uwip_strip_seams queues them: rounds of `round` pairs over one scratch
    const size_t back_words = std::max((size_t)uwip_cdiv((size_t)w, 16) * h, (size_t)uwip_cdiv((size_t)h, 16) * w);
    const bool lds_fits = back_words <= (size_t)kSeamBackLdsWords;
    std::vector<uint32_t> cost(wh * round, 0xDDDDDDDDu), back(back_words * round, 0xDDDDDDDDu);
    std::vector<int32_t> orient(n, -9), seam((size_t)n * L, -9), seam2((size_t)n * L, -9);
    std::vector<unsigned long long> total(n, 99), total2(n, 99);
    StripSeam a;
    a.store = store.data(); a.fstride = fstride; a.w = w; a.h = h;
    a.G = G.data(); a.Ginv = Ginv.data(); a.seg = seg.data(); a.gq = gained ? gq.data() : nullptr;
    a.P.prior = sp[0];
    a.tiles_x = (int32_t)uwip_cdiv((size_t)w, kTileW);
    a.cost = cost.data(); a.back = back.data(); a.back_stride = back_words;
    a.orient = orient.data(); a.L = L;
    for (int32_t k0 = 0; k0 < n; k0 += round) {
        const unsigned nr = (unsigned)std::min(round, n - k0);
        a.k0 = k0;
        a.seam = seam.data(); a.total = total.data();
        launch((unsigned)a.tiles_x * uwip_cdiv((size_t)h, kTileH), nr, kRenderThreads, true, [=] { k_strip_seam_cost(a); });
        launch(nr, 1, kRenderThreads, true, [=] { k_strip_seam_path<false>(a); });
        if (lds_fits) {
            StripSeam b = a;
            b.back = nullptr; b.seam = seam2.data(); b.total = total2.data();
            launch(nr, 1, kRenderThreads, true, [=] { k_strip_seam_path<true>(b); });
        }
    }
    if (lds_fits) expect(seam == seam2 && total == total2, "back pointers in LDS and in global scratch give different seams");
    wr(fo, orient.data(), orient.size()); wr(fo, seam.data(), seam.size()); wr(fo, total.data(), total.size());

    const uint8_t fill[3] = {7, 99, 200};
    for (int32_t si = 0; si < nseg; ++si) {
        const uwip_strip_segment &sg = segs[si];
        Placed c = place(sg.rows, sg.cols * 3, si % 3), cv = place(sg.rows, sg.cols, 2);
        cv.step = (size_t)sg.cols;                       // the cover plane is packed
        StripRender r;
        r.store = store.data(); r.fstride = fstride; r.w = w; r.h = h;
        r.Ginv = Ginv.data(); r.box = box.data(); r.first = sg.first; r.count = sg.count;
        r.x0 = sg.x0; r.y0 = sg.y0; r.rows = sg.rows; r.cols = sg.cols;
        r.canvas = c.data; r.step = c.step; r.cover = cv.data; r.vec = c.vec;
        r.gq = gained ? gq.data() : nullptr;
        StripSeams q;
        q.seam = seam.data(); q.orient = orient.data(); q.L = L;
        for (int k = 0; k < 3; ++k) r.fill[k] = fill[k];
        r.fill[3] = 0;
        const unsigned gx = uwip_cdiv((size_t)sg.cols, kTileW), gy = uwip_cdiv((size_t)sg.rows, kTileH);
        if (gained) launch(gx, gy, kRenderThreads, true, [=] { k_strip_render<UWIP_STRIP_SEAM, true>(r, q); });
        else launch(gx, gy, kRenderThreads, true, [=] { k_strip_render<UWIP_STRIP_SEAM>(r, q); });
        check_canary(c, sg.rows, sg.cols * 3);
        check_canary(cv, sg.rows, sg.cols);
        std::vector<uint8_t> canvas((size_t)sg.rows * sg.cols * 3), cover((size_t)sg.rows * sg.cols);
        for (int y = 0; y < sg.rows; ++y) {
            std::memcpy(&canvas[(size_t)y * sg.cols * 3], c.data + (size_t)y * c.step, (size_t)sg.cols * 3);
            std::memcpy(&cover[(size_t)y * sg.cols], cv.data + (size_t)y * cv.step, (size_t)sg.cols);
        }
        wr(fo, canvas.data(), canvas.size()); wr(fo, cover.data(), cover.size());
    }
    std::fclose(fo);
    std::printf("strip seam emulation: %d segments, %d mismatches\n", nseg, g_bad);
    return g_bad ? 1 : 0;
}
