// uwimageproc_amd/csrc/jpeg_decode.hip executed on the host: the unit's own parse, plan and host sequence (decode_sequence) on
// the host-thread back end of hip_on_host.hpp, so every kernel runs thread for thread -- one std::thread per GPU thread and a
// barrier for __syncthreads in the kernels that synchronise, a plain loop over the threads in those that do not, workgroups
// one after another -- against jpeg::decode (cli/jpeg.hpp) into a strided, misaligned batch.  It checks the kernels' logic and
// the host sequence (under the sanitizers every index they form, every array size and grid) where there is no device; the GPU
// tests check the compiled kernels.  tests/test_jpeg_decode_emulated.py cuts the unit's first anonymous namespace into
// kernels_dec.inc, builds this file with the host compiler and gives it the streams:
//   emu <list file>      one line per case: <path> <sync_rounds> <channels of the batch> [<file for the host decoder's pixels>]
//                        or: batch <sync_rounds> <channels> <rows> <cols> <path>...     (all the streams in one call)
// and prints per case: <path> <sync_rounds> status <s> host <0|1> equal <0|1> clean <0|1> unsettled <u> of <n>
// per frame of a batch: batch <sync_rounds> frame <f> status <s> single <status alone> same <0|1> clean <0|1>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include "uwip.h"
#include "jpeg.hpp"
#include "jpeg_parse.hpp"
#include "guarded_batch.hpp"
#include "hip_on_host.hpp"
#include "kernels_dec.inc"
// uwip_jpeg_decode on host threads: its parse and plan, then the unit's own decode_sequence.  stats: unsettled lanes, lanes
static void decode(const std::vector<std::vector<uint8_t>> &streams, int sync_rounds, const uwip_batch_u8 &out, int32_t *status,
                   unsigned long long *stats)
{
    const int n = (int)streams.size();
    std::vector<DecFrame> fr(n);
    std::vector<size_t> seg(n, 0);
    for (int f = 0; f < n; ++f) {
        DecFrame &d = fr[f];
        std::memset(&d, 0, sizeof d);
        int r = 0, c = 0, ch = 0;
        d.status = uwip_jpeg::parse(streams[f].data(), streams[f].size(), &r, &c, &ch, &d, &seg[f]);
        if (d.status == 0 && (r != out.rows || c != out.cols || (ch == 3 && out.channels == 1))) d.status = UWIP_JPEG_SIZE_MISMATCH;
        if (d.status == 0) d.seg_len = (uint32_t)(streams[f].size() - seg[f]);
    }
    DecPlan pl;
    plan_layout(fr.data(), n, pl);
    std::vector<uint8_t> src(pl.src_bytes, 0xEE);              // its exact size, as the back end's arrays have theirs
    for (int f = 0; f < n; ++f)
        if (fr[f].status == 0 && fr[f].seg_len) std::memcpy(src.data() + fr[f].seg_off, streams[f].data() + seg[f], fr[f].seg_len);
    HostThreads be;
    be.barrier_free = {"k_jpd_idct", "k_jpd_color"};
    decode_sequence(be, fr.data(), src.data(), pl, n, rounds_of(sync_rounds), out, status, stats);
}

static std::vector<uint8_t> read_file(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// batch <sync_rounds> <channels> <rows> <cols> <path>...: the streams in one call, and each alone into a batch of the same shape
static void batch_case(std::istringstream &is)
{
    int rounds = -1, channels = 3, rows = 0, cols = 0;
    is >> rounds >> channels >> rows >> cols;
    std::vector<std::vector<uint8_t>> streams;
    for (std::string path; is >> path;) streams.push_back(read_file(path));
    const int n = (int)streams.size();
    Batch all(n, rows, cols, channels);
    std::vector<int32_t> status(n, 99);
    unsigned long long stats[2];
    decode(streams, rounds, all.b, status.data(), stats);
    for (int f = 0; f < n; ++f) {
        Batch one(1, rows, cols, channels);
        int32_t st1 = 99;
        decode({streams[f]}, rounds, one.b, &st1, stats);
        bool same = true;
        for (int y = 0; y < rows; ++y) same = same && !std::memcmp(all.row(f, y), one.row(0, y), (size_t)cols * channels);
        std::printf("batch %d frame %d status %d single %d same %d clean %d\n", rounds, f, status[f], st1, (int)same, (int)(all.clean() && one.clean()));
    }
}
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream list(argv[1]);
    std::string line;
    while (std::getline(list, line)) {
        std::istringstream is(line);
        std::string path, dump; int rounds = -1, channels = 3;
        if (!(is >> path)) continue;
        if (path == "batch") { batch_case(is); continue; }
        if (!(is >> rounds >> channels)) continue;
        is >> dump;
        const std::vector<uint8_t> s = read_file(path);
        int rows = 0, cols = 0, ch = 0;
        std::vector<uint8_t> host;
        const bool host_ok = jpeg::decode(s.data(), s.size(), rows, cols, ch, host, channels == 3);
        if (host_ok && !dump.empty()) std::ofstream(dump, std::ios::binary).write((const char *)host.data(), (std::streamsize)host.size());
        int32_t ir = 0, ic = 0, ich = 0;
        const int info = uwip_jpeg::parse(s.data(), s.size(), &ir, &ic, &ich, nullptr, nullptr);
        if (!host_ok) { rows = info == 0 ? ir : 8; cols = info == 0 ? ic : 8; }
        Batch bt(1, rows, cols, channels);
        int32_t status = 99;
        unsigned long long stats[2];
        decode({s}, rounds, bt.b, &status, stats);
        bool equal = host_ok && status == 0;
        for (int y = 0; y < rows && equal; ++y) equal = !std::memcmp(bt.row(0, y), host.data() + (size_t)y * cols * channels, (size_t)cols * channels);
        const bool clean = bt.clean();
        std::printf("%s %d status %d host %d equal %d clean %d unsettled %llu of %llu\n", path.c_str(), rounds, status, (int)host_ok, (int)equal, (int)clean, stats[0], stats[1]);
    }
    return 0;
}
