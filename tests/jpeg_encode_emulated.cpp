// uwimageproc_amd/csrc/jpeg_encode.hip executed on the host: the unit's own host sequence (encode_sequence) on the host-thread
// back end of hip_on_host.hpp, so every kernel runs thread for thread -- one std::thread per GPU thread, a barrier for
// __syncthreads, workgroups one after another -- against jpeg::encode (cli/jpeg.hpp) on strided, misaligned batches, with slots
// that fit, are one byte short, or are far too small, and once with a frame count below the batch.  It checks the kernels' logic
// and the host sequence where there is no device; the GPU tests check the compiled kernels.
// tests/test_jpeg_encode_emulated.py cuts the unit's first anonymous namespace into kernels.inc and builds this file with the
// host compiler.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include "uwip.h"
#include "jpeg.hpp"
#include "jpeg_tables.hpp"
#include "hip_on_host.hpp"
#include "kernels.inc"
// uwip_jpeg_encode_dev on host threads: its tables as host structs, then the unit's own encode_sequence.  count: null, or the
// frame count that the kernels read
static void encode(const uint8_t *img, int F, int rows, int cols, int nc, size_t step, size_t fs, int quality, uint8_t *d_streams, size_t slot_bytes,
                   int64_t *d_sizes, const int32_t *count = nullptr)
{
    Geo g; g.rows = rows; g.cols = cols; g.nc = nc; g.step = step; g.fs = fs; g.nblk = blocks_of(rows, cols, nc, &g.mcux);
    static JpegHuff H; build_huff(H);
    static JpegConst Cn; std::memset(&Cn, 0, sizeof Cn); build_const(rows, cols, nc, clamp_quality(quality), Cn);
    HostThreads be;
    be.barrier_free = {"k_jpeg_zero_shared"};
    encode_sequence(be, img, g, F, &H, &Cn, d_streams, slot_bytes, d_sizes, count);
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
        if (c.rows == 7 && c.nc == 3 && c.q == 50 && c.kind == 2) {
            // a device count below the batch: frame 0 as ever, frame 1 reports size 0, its slot and all behind it stay untouched
            const size_t slot = std::max(host[0].size(), host[1].size()) + 9;
            std::vector<uint8_t> out(slot * F + 8, 0xEE);
            int64_t sizes[2] = {-77, -77};
            const int32_t count = 1;
            encode(img, F, c.rows, c.cols, c.nc, step, fs, c.q, out.data(), slot, sizes, &count);
            ++ncase;
            bool ok = sizes[0] == (int64_t)host[0].size() && sizes[1] == 0 && !std::memcmp(out.data(), host[0].data(), host[0].size());
            for (size_t i = slot; i < out.size(); ++i) ok = ok && out[i] == 0xEE;
            if (!ok) { ++bad; std::printf("MISMATCH count 1 of 2: sizes %lld %lld want %zu 0\n", (long long)sizes[0], (long long)sizes[1], host[0].size()); }
            else std::printf("count 1 of 2 ok\n");
        }
    }
    std::printf("%d cases, %d mismatches\n", ncase, bad);
    return bad != 0;
}
