// The kernels of uwimageproc_amd/csrc/png_decode.hip executed on the host, thread for thread: one std::thread per GPU thread
// and a barrier for __syncthreads, workgroups one after another, against imgio::read_png (cli/imgio.hpp, zlib's inflate) into a
// strided, misaligned batch.  It checks the kernels' logic (and, under the sanitizers, every index they form) where there is
// no device; the GPU tests check the compiled kernels.  tests/test_png_decode_emulated.py cuts the kernels out of the .hip file
// into kernels_pngd.inc (everything inside its anonymous namespace), builds this file with the host compiler and gives it the
// streams:
//   emu <list file>      one line per case: <path> <segmented> <channels of the batch>
// and prints per case: <path> <segmented> status <s> host <0|1> equal <0|1> clean <0|1> accepted <a> serial <r> maxdist <d>
//   emu --encode <raw file> <rows> <cols> <channels> <filter> <out.png>      the library's own encoder (its serial host form)
// The kernels use no wave primitive beyond what hip_on_host.hpp restates: the lanes meet in LDS and at the barrier.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include "uwip.h"
#include "imgio.hpp"
#include "png_parse.hpp"
#include "png_reference.hpp"
#include "hip_on_host.hpp"
#include "kernels_pngd.inc"

// uwip_png_decode's host side for one frame, the kernels on host threads
static void decode(const std::vector<uint8_t> &stream, int segmented, uint8_t *out, size_t step, size_t fs, int rows, int cols, int channels,
                   int32_t *status, unsigned long long *counts, uint32_t *maxdist)
{
    const int n = 1;
    uwip_pngd::Parsed p;
    PFrame fr;
    std::memset(&fr, 0, sizeof fr);
    std::vector<PSeg> segs;
    PPlan pl;
    fr.status = uwip_pngd::parse(stream.data(), stream.size(), p);
    if (fr.status == 0 && ((int64_t)p.H != rows || (int64_t)p.W != cols || (p.spp >= 3 && channels == 1))) fr.status = UWIP_PNG_SIZE_MISMATCH;
    fr.spp = fr.status == 0 ? p.spp : 1;
    if (fr.status == 0) plan_frame(fr, p, rows, cols, segmented, segs, 0, pl);
    // exact sizes, so that the address sanitizer sees an index one past any of them
    const size_t wsb = ws_bytes(rows, cols), nsegtot = segs.size();
    const uint32_t npieces = (uint32_t)((wsb + kChunk - 1) / kChunk);
    std::vector<uint8_t> src(pl.src_bytes + 16, 0), ws(n * wsb + 16, 0xEE);
    if (fr.status == 0) uwip_pngd::gather(stream.data(), p, src.data() + fr.zoff);
    std::vector<PRes> res(nsegtot + n, PRes{7u, 7u, 7u, 7u});
    std::vector<uint32_t> asum((size_t)n * npieces * 2, 0x55555555u);
    counts[0] = counts[1] = counts[2] = 0;
    PBufs B;
    B.fr = &fr; B.seg = segs.data(); B.src = src.data(); B.ws = ws.data(); B.res = res.data(); B.asum = asum.data();
    B.status = status; B.counts = counts; B.nsegtot = (uint32_t)nsegtot; B.nframes = n;
    PGeoD g;
    g.rows = rows; g.cols = cols; g.ws_stride = (uint32_t)wsb; g.npieces = npieces;
    if (nsegtot) launch((unsigned)nsegtot, 1, 64, true, [=] { k_pngd_inflate(B, g, 0); });
    launch(n, 1, 64, true, [=] { k_pngd_inflate(B, g, 1); });
    launch(npieces, n, 256, true, [=] { k_pngd_adler(B, g); });
    launch(n, 1, 64, true, [=] { k_pngd_unfilter(B, g); });
    launch(uwip_cdiv((size_t)rows * cols, 256), n, 256, false, [=] { k_pngd_color(B, g, out, step, fs, channels); });
    *maxdist = 0;
    for (const PRes &r : res) if (r.maxdist != 7u || r.ok != 7u) *maxdist = std::max(*maxdist, r.maxdist);
}

static int encode_own(char **a)
{
    const int rows = std::atoi(a[1]), cols = std::atoi(a[2]), nc = std::atoi(a[3]), filter = std::atoi(a[4]);
    std::vector<uint8_t> raw, out;
    if (!imgio::read_file(a[0], raw) || raw.size() != (size_t)rows * cols * nc) return 2;
    uwip_png::encode_host_reference(raw.data(), rows, cols, nc, (size_t)cols * nc, filter, out);
    FILE *f = std::fopen(a[5], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc == 8 && !std::strcmp(argv[1], "--encode")) return encode_own(argv + 2);
    if (argc < 2) return 2;
    std::ifstream list(argv[1]);
    std::string line;
    while (std::getline(list, line)) {
        std::istringstream is(line);
        std::string path; int segmented = -1, channels = 3;
        if (!(is >> path >> segmented >> channels)) continue;
        std::vector<uint8_t> s;
        imgio::read_file(path, s);
        imgio::Image host;
        const bool host_ok = imgio::read_png(s, host, channels == 3) && host.channels == channels;
        int rows = host_ok ? host.rows : 8, cols = host_ok ? host.cols : 8;
        int32_t ir = 0, ic = 0, ich = 0;
        if (!host_ok && uwip_pngd::info(s.data(), s.size(), &ir, &ic, &ich) == 0 && (int64_t)ir * ic < (1 << 22)) { rows = ir; cols = ic; }
        const size_t step = (size_t)cols * channels + 5, fs = step * rows + 77;
        std::vector<uint8_t> buf(fs + 3, 0xA5);
        uint8_t *out = buf.data() + 3;
        int32_t status = 99;
        unsigned long long counts[3];
        uint32_t maxdist = 0;
        decode(s, segmented, out, step, fs, rows, cols, channels, &status, counts, &maxdist);
        bool equal = host_ok && status == 0, clean = true;
        for (int y = 0; y < rows && equal; ++y) equal = !std::memcmp(out + y * step, host.data.data() + (size_t)y * cols * channels, (size_t)cols * channels);
        for (size_t i = 0; i < buf.size(); ++i) {
            const size_t o = i < 3 ? SIZE_MAX : i - 3;
            const bool inside = o != SIZE_MAX && o / step < (size_t)rows && o % step < (size_t)cols * channels;
            if (!inside && buf[i] != 0xA5) clean = false;
        }
        std::printf("%s %d status %d host %d equal %d clean %d accepted %llu serial %llu maxdist %u\n", path.c_str(), segmented, status, (int)host_ok,
                    (int)equal, (int)clean, counts[0], counts[1], maxdist);
    }
    return 0;
}
