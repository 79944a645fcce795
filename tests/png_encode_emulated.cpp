// uwimageproc_amd/csrc/png_encode.hip executed on the host: the unit's own host sequence (encode_sequence) on the host-thread
// back end of hip_on_host.hpp, so every kernel runs thread for thread -- one std::thread per GPU thread, a barrier for
// __syncthreads, workgroups one after another -- against the serial reference encoder (csrc/png_reference.hpp) on strided,
// misaligned batches, every filter choice, with slots that fit, are one byte short, or are far too small, and once with a frame
// count below the batch.  It checks the kernels' parallel structure and the host sequence where there is no device; the GPU
// tests check the compiled kernels.  tests/test_png_encode_emulated.py cuts the unit's first anonymous namespace into
// kernels.inc, builds this file with the host compiler and the address and undefined-behaviour sanitizers, and then checks the
// streams this program leaves in the directory argv[1] with Pillow, zlib and numpy: <case>.png, <case>.raw (the packed input)
// and manifest.txt (case rows cols channels filter).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include "hip_on_host.hpp"
#include "deflate_core.hpp"
#include "png_reference.hpp"
#include "kernels.inc"

// uwip_png_encode_dev on host threads: the head bytes in host memory, then the unit's own encode_sequence.  count: null, or the
// frame count that the kernels read
static void encode(const uint8_t *img, int F, int rows, int cols, int nc, size_t step, size_t fs, int filter, uint8_t *streams, size_t slot_bytes,
                   int64_t *sizes, const int32_t *count = nullptr)
{
    const PGeo g = geometry_of(rows, cols, nc, step, fs);
    uint8_t head[kHeadBytes];
    write_head(rows, cols, nc, head);
    HostThreads be;
    encode_sequence(be, img, g, F, filter, head, streams, slot_bytes, sizes, count);
}

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
    if (argc < 2) { std::printf("usage: emu <output directory>\n"); return 2; }
    const std::string dir = argv[1];
    std::mt19937 rng(7);
    int bad = 0, ncase = 0;
    // kinds: 0 noise (stored), 1 constant (runs longer than 258 and across chunks), 2 horizontal ramp, 3 two-level checkerboard
    // (no run of 3), 4 Fibonacci byte counts (a Huffman tree deeper than 15), 5 smooth with a little noise
    struct Case { int rows, cols, nc, F, kinds[3]; };
    const std::vector<Case> cases = {
        {1, 1, 1, 2, {0, 1, 0}}, {1, 1, 3, 2, {0, 1, 0}}, {1, 300, 1, 3, {0, 1, 2}}, {300, 1, 1, 2, {5, 1, 0}},
        {5, 7, 3, 3, {0, 3, 5}}, {97, 113, 3, 3, {1, 5, 2}}, {97, 113, 3, 2, {0, 3, 0}}, {200, 333, 1, 3, {4, 1, 5}},
    };
    std::string manifest;
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        const Case &c = cases[ci];
        const int F = c.F;
        const size_t rb = (size_t)c.cols * c.nc, step = rb + 5, fs = step * c.rows + 77;      // padded rows, odd frame stride
        std::vector<uint8_t> buf(fs * F + 3);
        uint8_t *img = buf.data() + 3;                                                         // a base pointer off by 3
        std::vector<std::vector<uint8_t>> packed(F, std::vector<uint8_t>(rb * c.rows));
        for (int f = 0; f < F; ++f) {
            const int kind = c.kinds[f];
            std::vector<uint8_t> fib;
            if (kind == 4) {
                uint32_t a = 1, b = 1;
                for (int s = 0; fib.size() < packed[f].size(); ++s) {
                    for (uint32_t k = 0; k < a && fib.size() < packed[f].size(); ++k) fib.push_back((uint8_t)(s * 7 + 3));
                    const uint32_t t = a + b; a = b; b = t;
                }
                std::shuffle(fib.begin(), fib.end(), rng);
            }
            for (int y = 0; y < c.rows; ++y) for (size_t x = 0; x < rb; ++x) {
                const size_t px = x / c.nc;
                uint8_t v;
                switch (kind) {
                    case 0: v = (uint8_t)rng(); break;
                    case 1: v = (uint8_t)(77 + 50 * f); break;
                    case 2: v = (uint8_t)px; break;
                    case 3: v = ((px + y) & 1) ? 220 : 20; break;
                    case 4: v = fib[(size_t)y * rb + x]; break;
                    default: v = (uint8_t)(128 + 100 * std::sin(0.05 * px + 0.08 * y + f) + (rng() & 3)); break;
                }
                img[f * fs + y * step + x] = v;
                packed[f][(size_t)y * rb + x] = v;
            }
        }
        for (int filter = -1; filter <= 4; ++filter) {
            std::vector<std::vector<uint8_t>> ref(F);
            size_t longest = 0;
            for (int f = 0; f < F; ++f) {
                uwip_png::encode_host_reference(packed[f].data(), c.rows, c.cols, c.nc, rb, filter, ref[f]);
                longest = std::max(longest, ref[f].size());
            }
            for (int mode = 0; mode < 3; ++mode) {
                // 0: generous slot; 1: frame 0 one byte short; 2: frame 0 far too small
                const size_t slot = mode == 0 ? longest + 9 : mode == 1 ? ref[0].size() - 1 : ref[0].size() / 2;
                std::vector<uint8_t> out(slot * F + 8, 0xEE);
                std::vector<int64_t> sizes(F, 0);
                encode(img, F, c.rows, c.cols, c.nc, step, fs, filter, out.data(), slot, sizes.data());
                ++ncase;
                for (int f = 0; f < F; ++f) {
                    const bool fit = ref[f].size() <= slot;
                    const int64_t want = fit ? (int64_t)ref[f].size() : -(int64_t)ref[f].size();
                    bool ok = sizes[f] == want;
                    if (ok && fit) ok = !std::memcmp(out.data() + f * slot, ref[f].data(), ref[f].size());
                    if (ok && fit) for (size_t i = ref[f].size(); i < slot; ++i) ok = ok && out[f * slot + i] == 0xEE;
                    if (ok && !fit) for (size_t i = 0; i < slot; ++i) ok = ok && out[f * slot + i] == 0xEE;
                    if (!ok) {
                        ++bad;
                        std::printf("MISMATCH case %zu (%dx%dx%d) filter %d mode %d frame %d: size %lld want %lld\n", ci, c.rows, c.cols, c.nc,
                                    filter, mode, f, (long long)sizes[f], (long long)want);
                    }
                    if (mode == 0 && sizes[f] > 0) {
                        const std::string name = "c" + std::to_string(ci) + "_k" + std::to_string(filter + 1) + "_f" + std::to_string(f);
                        if (!dump(dir + "/" + name + ".png", out.data() + f * slot, (size_t)sizes[f]) ||
                            (filter == -1 && !dump(dir + "/c" + std::to_string(ci) + "_f" + std::to_string(f) + ".raw", packed[f].data(), packed[f].size()))) {
                            std::printf("cannot write into %s\n", dir.c_str());
                            return 2;
                        }
                        manifest += name + " c" + std::to_string(ci) + "_f" + std::to_string(f) + " " + std::to_string(c.rows) + " " +
                                    std::to_string(c.cols) + " " + std::to_string(c.nc) + " " + std::to_string(filter) + "\n";
                    }
                }
                for (size_t i = slot * F; i < out.size(); ++i) if (out[i] != 0xEE) { ++bad; std::printf("wrote past the end\n"); break; }
            }
            if (c.rows == 5 && c.nc == 3 && filter == -1) {
                // two frames and a device count of 1: frame 0 as ever, frame 1 reports size 0, its slot and all behind it stay untouched
                const size_t slot = longest + 9;
                std::vector<uint8_t> out(slot * 2 + 8, 0xEE);
                int64_t sizes[2] = {-77, -77};
                const int32_t count = 1;
                encode(img, 2, c.rows, c.cols, c.nc, step, fs, filter, out.data(), slot, sizes, &count);
                ++ncase;
                bool ok = sizes[0] == (int64_t)ref[0].size() && sizes[1] == 0 && !std::memcmp(out.data(), ref[0].data(), ref[0].size());
                for (size_t i = ref[0].size(); i < out.size(); ++i) ok = ok && out[i] == 0xEE;
                if (!ok) { ++bad; std::printf("MISMATCH count 1 of 2: sizes %lld %lld want %zu 0\n", (long long)sizes[0], (long long)sizes[1], ref[0].size()); }
                else std::printf("count 1 of 2 ok\n");
            }
        }
    }
    if (!dump(dir + "/manifest.txt", (const uint8_t *)manifest.data(), manifest.size())) return 2;
    std::printf("%d cases, %d mismatches\n", ncase, bad);
    return bad != 0;
}
