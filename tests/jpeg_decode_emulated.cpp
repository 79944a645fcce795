// The kernels of uwimageproc_amd/csrc/jpeg_decode.hip executed on the host, thread for thread: one std::thread per GPU thread
// and a barrier for __syncthreads in the kernels that synchronise, a plain loop over the threads in those that do not,
// workgroups one after another, against jpeg::decode (cli/jpeg.hpp) into a strided, misaligned batch.  It checks the kernels'
// logic (and, under the sanitizers, every index they form) where there is no device; the GPU tests check the compiled kernels.
// tests/test_jpeg_decode_emulated.py cuts the kernels out of the .hip file into kernels_dec.inc (everything inside its
// anonymous namespace), builds this file with the host compiler and gives it the streams:
//   emu <list file>      one line per case: <path> <sync_rounds> <channels of the batch> [<file for the host decoder's pixels>]
// and prints per case: <path> <sync_rounds> status <s> host <0|1> equal <0|1> clean <0|1> unsettled <u> of <n>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include "uwip.h"
#include "jpeg.hpp"
#include "jpeg_parse.hpp"
#include "hip_on_host.hpp"
#include "kernels_dec.inc"
// uwip_jpeg_decode's host side for one frame, the kernels on host threads
static int decode(const std::vector<uint8_t> &stream, int sync_rounds, uint8_t *out, size_t step, size_t fs, int rows, int cols, int channels,
                  int32_t *status, unsigned long long *stats)
{
    const int n = 1, rounds = rounds_of(sync_rounds);
    std::vector<DecFrame> fr(n);
    size_t seg = 0;
    std::memset(&fr[0], 0, sizeof(DecFrame));
    int r = 0, c = 0, ch = 0;
    fr[0].status = uwip_jpeg::parse(stream.data(), stream.size(), &r, &c, &ch, &fr[0], &seg);
    if (fr[0].status == 0 && (r != rows || c != cols || (ch == 3 && channels == 1))) fr[0].status = UWIP_JPEG_SIZE_MISMATCH;
    if (fr[0].status == 0) fr[0].seg_len = (uint32_t)(stream.size() - seg);
    DecPlan pl;
    plan_layout(fr.data(), n, pl);
    // exact sizes, so that the address sanitizer sees an index one past any of them
    std::vector<uint8_t> src(pl.src_bytes, 0xEE), ubuf(pl.ubuf_bytes + 16, 0xEE), planes(pl.plane_bytes + 16, 0xEE);
    if (fr[0].status == 0 && fr[0].seg_len) std::memcpy(src.data() + fr[0].seg_off, stream.data() + seg, fr[0].seg_len);
    const size_t ni = pl.nintv + 1, ns = pl.nsub + 1;
    std::vector<uint64_t> e0(ns, 0x5555), e1(ns, 0x5555), en(ns, 0x5555);
    std::vector<uint32_t> cnt(ns, 77), sblk(ns, 77), sint(ns, 77), istart(ni, 77), isub(ni, 77), ifirst(ni, 0xFFFFFFFFu);
    std::vector<int16_t> coef((pl.nblk + 1) * 64, 0);
    int32_t err = 0;
    stats[0] = stats[1] = 0;
    DecBufs B;
    B.fr = fr.data(); B.src = src.data(); B.ubuf = ubuf.data();
    B.exit0 = e0.data(); B.exit1 = e1.data(); B.entry = en.data(); B.stats = stats;
    B.cnt = cnt.data(); B.sblk = sblk.data(); B.sint = sint.data(); B.istart = istart.data(); B.isub = isub.data(); B.ifirst = ifirst.data();
    B.coef = coef.data(); B.planes = planes.data(); B.status = status; B.err = &err;
    const unsigned gsub = uwip_cdiv(pl.max_sub ? pl.max_sub : 1, 256), gint = uwip_cdiv(pl.max_int ? pl.max_int : 1, 64);
    const unsigned gblk = uwip_cdiv(pl.max_blk ? pl.max_blk : 1, 64), gpix = uwip_cdiv((size_t)rows * cols, 256);
    launch(n, 1, 256, true, [=] { k_jpd_unstuff(B); });
    for (int rr = 0; rr <= rounds; ++rr) launch(gsub, n, 256, true, [=] { k_jpd_round(B, rr); });
    launch(gsub, n, 256, true, [=] { k_jpd_check(B, rounds); });
    launch(gint, n, 64, true, [=] { k_jpd_cleanup(B, rounds); });
    launch(n, 1, 256, true, [=] { k_jpd_blkscan(B); });
    launch(gsub, n, 256, true, [=] { k_jpd_write(B, rounds); });
    launch(3, n, 256, true, [=] { k_jpd_dc(B); });
    launch(gblk, n, 64, false, [=] { k_jpd_idct(B); });
    launch(gpix, n, 256, false, [=] { k_jpd_color(B, out, step, fs, rows, cols, channels); });
    return 0;
}
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream list(argv[1]);
    std::string line;
    while (std::getline(list, line)) {
        std::istringstream is(line);
        std::string path, dump; int rounds = -1, channels = 3;
        if (!(is >> path >> rounds >> channels)) continue;
        is >> dump;
        std::ifstream f(path, std::ios::binary);
        std::vector<uint8_t> s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        int rows = 0, cols = 0, ch = 0;
        std::vector<uint8_t> host;
        const bool host_ok = jpeg::decode(s.data(), s.size(), rows, cols, ch, host, channels == 3);
        if (host_ok && !dump.empty()) std::ofstream(dump, std::ios::binary).write((const char *)host.data(), (std::streamsize)host.size());
        int32_t ir = 0, ic = 0, ich = 0;
        const int info = uwip_jpeg::parse(s.data(), s.size(), &ir, &ic, &ich, nullptr, nullptr);
        if (!host_ok) { rows = info == 0 ? ir : 8; cols = info == 0 ? ic : 8; }
        const size_t step = (size_t)cols * channels + 5, fs = step * rows + 77;
        std::vector<uint8_t> buf(fs + 3, 0xA5);
        uint8_t *out = buf.data() + 3;
        int32_t status = 99;
        unsigned long long stats[2];
        decode(s, rounds, out, step, fs, rows, cols, channels, &status, stats);
        bool equal = host_ok && status == 0, clean = true;
        for (int y = 0; y < rows && equal; ++y) equal = !std::memcmp(out + y * step, host.data() + (size_t)y * cols * channels, (size_t)cols * channels);
        for (size_t i = 0; i < buf.size(); ++i) {
            const size_t o = i < 3 ? SIZE_MAX : i - 3;
            const bool inside = o != SIZE_MAX && o / step < (size_t)rows && o % step < (size_t)cols * channels;
            if (!inside && buf[i] != 0xA5) clean = false;
        }
        std::printf("%s %d status %d host %d equal %d clean %d unsettled %llu of %llu\n", path.c_str(), rounds, status, (int)host_ok, (int)equal, (int)clean, stats[0], stats[1]);
    }
    return 0;
}
