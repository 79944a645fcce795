// The kernels of uwimageproc_amd/csrc/jpeg_encode.hip executed on the host, thread for thread: one std::thread per GPU thread, a
// barrier for __syncthreads, workgroups one after another, against jpeg::encode (cli/jpeg.hpp) on strided, misaligned batches,
// with slots that fit, are one byte short, or are far too small.  It checks the kernels' logic where there is no device; the
// GPU tests check the compiled kernels.  tests/test_jpeg_encode_emulated.py cuts the kernels out of the .hip file into
// kernels.inc (everything inside its anonymous namespace) and builds this file with the host compiler; hip_on_host.hpp is the
// device language on host threads.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include "uwip.h"
#include "jpeg.hpp"
#include "jpeg_tables.hpp"
#include "hip_on_host.hpp"
#include "kernels.inc"
static int encode(const uint8_t *img, int F, int rows, int cols, int nc, size_t step, size_t fs, int quality, uint8_t *d_streams, size_t slot_bytes, int64_t *d_sizes)
{
    quality = clamp_quality(quality);
    Geo g; g.rows = rows; g.cols = cols; g.nc = nc; g.step = step; g.fs = fs; g.nblk = blocks_of(rows, cols, nc, &g.mcux);
    static JpegHuff H; std::memset(&H, 0, sizeof H);
    { using namespace uwip_jpeg; uint32_t t[256];
      build_codes(DC_LUM_BITS, DC_VALS, t); std::memcpy(H.dc[0], t, sizeof H.dc[0]);
      build_codes(DC_CHR_BITS, DC_VALS, t); std::memcpy(H.dc[1], t, sizeof H.dc[1]);
      build_codes(AC_LUM_BITS, AC_LUM_VALS, H.ac[0]); build_codes(AC_CHR_BITS, AC_CHR_VALS, H.ac[1]); }
    static JpegConst Cn; std::memset(&Cn, 0, sizeof Cn); build_const(rows, cols, nc, quality, Cn);
    const JpegHuff *huff = &H; const JpegConst *cst = &Cn;
    const int nwg_bits = (int)uwip_cdiv((size_t)g.nblk, kBitsWG), nwg_emit = (int)uwip_cdiv((size_t)g.nblk, kEmitWG);
    const size_t ubound = ((size_t)g.nblk * kMaxBlockBits + 7) / 8;
    const size_t ucap = slot_bytes < ubound ? slot_bytes : ubound;
    const size_t ustride = ((ucap + 15) / 16) * 4 + 8;
    const int nchunk = ucap ? (int)uwip_cdiv(ucap, kChunk) : 1;
    std::vector<int16_t> coefv((size_t)F * g.nblk * 64 + 8);
    int16_t *coef = (int16_t *)(((uintptr_t)coefv.data() + 15) & ~(uintptr_t)15);
    std::vector<uint32_t> ubufv((size_t)F * ustride + 4, 0xDEADBEEFu);      // garbage: only the shared words get zeroed
    uint32_t *ubuf = (uint32_t *)(((uintptr_t)ubufv.data() + 15) & ~(uintptr_t)15);
    std::vector<uint32_t> blkoffv((size_t)F * g.nblk); uint32_t *blkoff = blkoffv.data();
    const size_t n64 = (size_t)F * nwg_bits + F + (size_t)F * nchunk + F;
    const size_t n32 = (size_t)F * nwg_bits + (size_t)F * nchunk + F + (size_t)F * (nwg_emit + 1);
    std::vector<uint64_t> metav(n64 + n32 / 2 + 2, 0x5555555555555555ull); uint64_t *meta = metav.data();
    uint64_t *wgbase = meta, *totbits = wgbase + (size_t)F * nwg_bits, *chunkbase = totbits + F;
    int64_t *needed = reinterpret_cast<int64_t *>(chunkbase + (size_t)F * nchunk);
    uint32_t *wgsum = reinterpret_cast<uint32_t *>(needed + F), *chunkcnt = wgsum + (size_t)F * nwg_bits;
    uint32_t *ffemit = chunkcnt + (size_t)F * nchunk, *notff = ffemit + F;
    std::memset(ffemit, 0, ((size_t)F + (size_t)F * (nwg_emit + 1)) * sizeof(uint32_t));
    const Offs o{blkoff, wgbase, totbits, nwg_bits};
    launch(nwg_bits, F, 256, true, [=] { k_jpeg_transform(img, g, cst, coef); });
    launch(nwg_bits, F, kBitsWG, true, [=] { k_jpeg_bits(coef, g, huff, blkoff, wgsum, nwg_bits); });
    launch(F, 1, 256, true, [=] { k_jpeg_scan_bits(wgsum, wgbase, totbits, nwg_bits); });
    launch(uwip_cdiv((size_t)nwg_emit, 256), F, 256, true, [=] { k_jpeg_zero_shared(g, o, cst, slot_bytes, ubuf, ustride, nwg_emit); });
    launch(nwg_emit, F, kEmitWG, true, [=] { k_jpeg_emit(coef, g, huff, o, cst, slot_bytes, ubuf, ustride, ffemit, notff, nwg_emit); });
    launch(nchunk, F, 256, true, [=] { k_jpeg_ffcount(ubuf, ustride, totbits, cst, slot_bytes, chunkcnt, nchunk); });
    launch(F, 1, 256, true, [=] { k_jpeg_finish(chunkcnt, chunkbase, nchunk, g, o, cst, ffemit, notff, nwg_emit, needed); });
    launch(nchunk, F, 256, true, [=] { k_jpeg_assemble(ubuf, ustride, totbits, chunkbase, nchunk, cst, needed, d_streams, slot_bytes, d_sizes); });
    return 0;
}
int main()
{
    std::mt19937 rng(7);
    int bad = 0, ncase = 0;
    struct Case { int rows, cols, nc, q, kind; };
    std::vector<Case> cases;
    for (int nc : {3, 1}) for (int q : {1, 50, 95, 100}) for (int kind : {0, 1, 2}) {
        cases.push_back({1, 1, nc, q, kind}); cases.push_back({7, 5, nc, q, kind}); cases.push_back({17, 33, nc, q, kind});
        cases.push_back({nc == 3 ? 150 : 90, nc == 3 ? 170 : 100, nc, q, kind});
    }
    cases.push_back({280, 300, 3, 100, 1}); cases.push_back({200, 200, 1, 100, 1});
    for (const Case &c : cases) {
        const int F = 2;
        const size_t step = (size_t)c.cols * c.nc + 5, fs = step * c.rows + 77;
        std::vector<uint8_t> buf(fs * F + 3);
        uint8_t *img = buf.data() + 3;
        std::vector<std::vector<uint8_t>> packed(F, std::vector<uint8_t>((size_t)c.rows * c.cols * c.nc));
        for (int f = 0; f < F; ++f) for (int y = 0; y < c.rows; ++y) for (int x = 0; x < c.cols * c.nc; ++x) {
            uint8_t v = c.kind == 0 ? (uint8_t)(200 - 60 * f) : c.kind == 1 ? (uint8_t)rng() : (uint8_t)(128 + 100 * std::sin(0.07 * x + 0.11 * y + f) + (rng() & 7));
            img[f * fs + y * step + x] = v; packed[f][(size_t)y * c.cols * c.nc + x] = v;
        }
        std::vector<std::vector<uint8_t>> host(F);
        for (int f = 0; f < F; ++f) jpeg::encode(packed[f].data(), c.rows, c.cols, c.nc, c.q, host[f]);
        for (int mode = 0; mode < 3; ++mode) {
            // 0: generous slot; 1: frame 0 one byte short; 2: frame 0 far too small (its unstuffed stream does not fit either)
            size_t slot = mode == 0 ? std::max(host[0].size(), host[1].size()) + 9 : mode == 1 ? host[0].size() - 1 : host[0].size() / 2;
            std::vector<uint8_t> out(slot * F + 8, 0xEE);
            int64_t sizes[2] = {0, 0};
            encode(img, F, c.rows, c.cols, c.nc, step, fs, c.q, out.data(), slot, sizes);
            ++ncase;
            for (int f = 0; f < F; ++f) {
                const bool fit = host[f].size() <= slot;
                const int64_t want = fit ? (int64_t)host[f].size() : -(int64_t)host[f].size();
                bool ok = sizes[f] == want;
                if (ok && fit) ok = !std::memcmp(out.data() + f * slot, host[f].data(), host[f].size());
                if (ok && !fit) for (size_t i = 0; i < slot; ++i) ok = ok && out[f * slot + i] == 0xEE;
                if (!ok) { ++bad; std::printf("MISMATCH %dx%dx%d q%d kind %d mode %d frame %d: size %lld want %lld\n", c.rows, c.cols, c.nc, c.q, c.kind, mode, f, (long long)sizes[f], (long long)want); }
            }
            for (size_t i = slot * F; i < out.size(); ++i) if (out[i] != 0xEE) { ++bad; std::printf("wrote past the end\n"); break; }
        }
    }
    std::printf("%d cases, %d mismatches\n", ncase, bad);
    return bad != 0;
}
