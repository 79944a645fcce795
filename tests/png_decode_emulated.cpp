// uwimageproc_amd/csrc/png_decode.hip executed on the host in every mode (segmented 0, 1 and 2, the found block starts): the
// unit's own parse, plan and host sequence (decode_sequence) on the host-thread back end of hip_on_host.hpp, so every kernel
// runs thread for thread -- one std::thread per GPU thread and a barrier for __syncthreads, workgroups one after another --
// against imgio::read_png (cli/imgio.hpp, zlib's inflate) into a strided, misaligned batch.  It checks the kernels' logic and
// the host sequence (under the sanitizers every index they form: the arrays have their exact sizes) where there is no device;
// the GPU tests check the compiled kernels.  The inflate machinery is csrc/png_inflate.hpp, included as it stands;
// tests/_png_emu.py cuts the unit's first anonymous namespace into kernels_pngd.inc, builds this file with the host compiler
// and gives it the streams:
//   emu <list file>      one line per case: <path> <segmented> <channels of the batch> <chunk_bytes>
//                        or: batch <segmented> <channels> <chunk_bytes> <rows> <cols> <path>...     (all the streams in one call),
//                        answered per frame: batch <segmented> <chunk_bytes> frame <f> status <s> single <status alone> same <0|1>
//                        clean <0|1> accepted <a> serial <r>
// and reads per case:
//   <path> <segmented> <chunk_bytes> status <s> host <0|1> equal <0|1> clean <0|1> accepted <a> serial <r> maxdist <d>
//   starts <n> <bit>... tried <t> valid <v>
// maxdist: the largest match distance of k_pngd_inflate's runs; starts: the start bits (behind the zlib header) of the chunks
// accepted from found block starts, in chain order; tried: the candidates that passed the screen and got the full decode, over
// all searching chunks; valid: the chunks that kept one.
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
#include "guarded_batch.hpp"
#include "hip_on_host.hpp"
#include "png_inflate.hpp"
#include "kernels_pngd.inc"

struct Seen {                   // what a case reports beside its pixels and status
    unsigned long long counts[3] = {0, 0, 0};
    uint32_t maxdist = 0;
    std::vector<uint32_t> starts;
    unsigned tried = 0, valid = 0;
};

// uwip_png_decode on host threads: its parse and plan, then the unit's own decode_sequence.  seen: the taps, those on the found
// block starts for frame 0
static void decode(const std::vector<std::vector<uint8_t>> &streams, int segmented, int asked, const uwip_batch_u8 &out, int32_t *status, Seen &seen)
{
    const int n = (int)streams.size();
    std::vector<uwip_pngd::Parsed> parsed(n);
    std::vector<PFrame> fr(n);
    std::vector<PSeg> segs;
    PPlan pl;
    size_t nslots = 0;
    uint32_t maxslots = 0;
    const uint32_t chunk_bytes = spec_chunk_bytes(asked);
    for (int f = 0; f < n; ++f) {
        PFrame &d = fr[f];
        std::memset(&d, 0, sizeof d);
        const uwip_pngd::Parsed &p = parsed[f];
        d.status = uwip_pngd::parse(streams[f].data(), streams[f].size(), parsed[f]);
        if (d.status == 0 && ((int64_t)p.H != out.rows || (int64_t)p.W != out.cols || (p.spp >= 3 && out.channels == 1))) d.status = UWIP_PNG_SIZE_MISMATCH;
        d.spp = d.status == 0 ? p.spp : 1;
        if (d.status == 0) {
            plan_frame(d, p, out.rows, out.cols, segmented, segs, f, pl);
            if (segmented == 2) spec_plan_frame(d, chunk_bytes, nslots, maxslots);
        }
    }
    std::vector<uint8_t> src(pl.src_bytes + 16, 0);            // its exact size, as the back end's arrays have theirs
    for (int f = 0; f < n; ++f)
        if (fr[f].status == 0) uwip_pngd::gather(streams[f].data(), parsed[f], src.data() + fr[f].zoff);
    HostThreads be;
    be.barrier_free = {"k_pngs_begin", "k_pngs_verify", "k_pngd_color"};
    bool took_path = false, begun = false;
    be.before_launch = [&](const std::string &name, dim3 &grid) {
        if (name == "k_pngs_measure" && !begun) { begun = true; took_path = be.get<PSpecFrame>("pngdec.chunks")[0].open != 0u; }
        // the library launches maxslots workgroups per frame; those at and behind nacc return at once, and a host thread each
        // is what this harness spends its time on, so they are left out here (one stays, to return at once)
        if (name == "k_pngs_write" || name == "k_pngs_resolve") {
            const PSpecFrame *sp = be.get<PSpecFrame>("pngdec.chunks");          // the buffer's first records (SpecLayout)
            unsigned nacc = 0;
            for (int f = 0; f < n; ++f) nacc = std::max<unsigned>(nacc, sp[f].ok ? sp[f].nacc : 0u);
            grid.x = std::min(grid.x, nacc + 1u);
        }
    };
    decode_sequence(be, fr.data(), segs.data(), src.data(), segs.size(), nslots, maxslots, chunk_bytes, n, out, status, seen.counts);
    if (nslots) {
        PBufs T;                                               // the unit's own binding of the records, for the taps
        spec_bind(T, const_cast<uint8_t *>(be.get<uint8_t>("pngdec.chunks")), nullptr, n, nslots, chunk_bytes);
        const PSpecFrame *sp = T.spec;
        const PChunk *chunk = T.chunk;
        const uint32_t *order = T.order;
        for (uint32_t c = 1; took_path && c < fr[0].nchunks; ++c) {
            seen.tried += chunk[fr[0].chunk0 + c].tries;
            seen.valid += chunk[fr[0].chunk0 + c].flags & kChunkValid;
        }
        if (sp[0].ok)
            for (uint32_t i = 0; i < sp[0].nacc; ++i) seen.starts.push_back(chunk[fr[0].chunk0 + order[fr[0].chunk0 + i]].start);
    }
    const PRes *res = be.get<PRes>("pngdec.res");
    for (size_t i = 0; i < segs.size() + n; ++i)
        if (res[i].maxdist != 0xDDDDDDDDu || res[i].ok != 0xDDDDDDDDu) seen.maxdist = std::max(seen.maxdist, res[i].maxdist);
}

// batch <segmented> <channels> <chunk_bytes> <rows> <cols> <path>...: the streams in one call, and each alone into a batch of the
// same shape
static void batch_case(std::istringstream &is)
{
    int segmented = -1, channels = 3, asked = 0, rows = 0, cols = 0;
    is >> segmented >> channels >> asked >> rows >> cols;
    std::vector<std::vector<uint8_t>> streams;
    for (std::string path; is >> path;) { streams.emplace_back(); imgio::read_file(path, streams.back()); }
    const int n = (int)streams.size();
    Batch all(n, rows, cols, channels);
    std::vector<int32_t> status(n, 99);
    Seen seen;
    decode(streams, segmented, asked, all.b, status.data(), seen);
    for (int f = 0; f < n; ++f) {
        Batch one(1, rows, cols, channels);
        int32_t st1 = 99;
        Seen alone;
        decode({streams[f]}, segmented, asked, one.b, &st1, alone);
        bool same = true;
        for (int y = 0; y < rows; ++y) same = same && !std::memcmp(all.row(f, y), one.row(0, y), (size_t)cols * channels);
        std::printf("batch %d %d frame %d status %d single %d same %d clean %d accepted %llu serial %llu\n", segmented, asked, f, status[f], st1, (int)same,
                    (int)(all.clean() && one.clean()), seen.counts[0], seen.counts[1]);
    }
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
        std::string path; int segmented = -1, channels = 3, asked = 0;
        if (!(is >> path)) continue;
        if (path == "batch") { batch_case(is); std::fflush(stdout); continue; }
        if (!(is >> segmented >> channels >> asked)) continue;
        std::vector<uint8_t> s;
        imgio::read_file(path, s);
        imgio::Image host;
        const bool host_ok = imgio::read_png(s, host, channels == 3) && host.channels == channels;
        int rows = host_ok ? host.rows : 8, cols = host_ok ? host.cols : 8;
        int32_t ir = 0, ic = 0, ich = 0;
        if (!host_ok && uwip_pngd::info(s.data(), s.size(), &ir, &ic, &ich) == 0 && (int64_t)ir * ic < (1 << 22)) { rows = ir; cols = ic; }
        Batch bt(1, rows, cols, channels);
        int32_t status = 99;
        Seen seen;
        decode({s}, segmented, asked, bt.b, &status, seen);
        bool equal = host_ok && status == 0;
        for (int y = 0; y < rows && equal; ++y) equal = !std::memcmp(bt.row(0, y), host.data.data() + (size_t)y * cols * channels, (size_t)cols * channels);
        const bool clean = bt.clean();
        std::printf("%s %d %d status %d host %d equal %d clean %d accepted %llu serial %llu maxdist %u starts %zu", path.c_str(), segmented, asked,
                    status, (int)host_ok, (int)equal, (int)clean, seen.counts[0], seen.counts[1], seen.maxdist, seen.starts.size());
        for (uint32_t b : seen.starts) std::printf(" %u", b);
        std::printf(" tried %u valid %u\n", seen.tried, seen.valid);
        std::fflush(stdout);
    }
    return 0;
}
