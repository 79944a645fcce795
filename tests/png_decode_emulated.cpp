// The kernels of uwimageproc_amd/csrc/png_decode.hip executed on the host, thread for thread, in every mode (segmented 0, 1 and
// 2, the found block starts): one std::thread per GPU thread and a barrier for __syncthreads, workgroups one after another,
// against imgio::read_png (cli/imgio.hpp, zlib's inflate) into a strided, misaligned frame.  It checks the kernels' logic (and,
// under the sanitizers, every index they form: the workspaces have their exact sizes) where there is no device; the GPU tests
// check the compiled kernels.  The inflate machinery is csrc/png_inflate.hpp, included as it stands; tests/_png_emu.py cuts
// the kernels and the host planning (the .hip file's anonymous namespace) into kernels_pngd.inc, builds this file with the
// host compiler and gives it the streams:
//   emu <list file>      one line per case: <path> <segmented> <channels of the batch> <chunk_bytes>
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
#include "hip_on_host.hpp"
#include "png_inflate.hpp"
#include "kernels_pngd.inc"

struct Seen {                   // what a case reports beside its pixels and status
    unsigned long long counts[3] = {0, 0, 0};
    uint32_t maxdist = 0;
    std::vector<uint32_t> starts;
    unsigned tried = 0, valid = 0;
};

// uwip_png_decode's host side for one frame, the kernels on host threads
static void decode(const std::vector<uint8_t> &stream, int segmented, int asked, uint8_t *out, size_t step, size_t fs, int rows, int cols,
                   int channels, int32_t *status, Seen &seen)
{
    const int n = 1;
    uwip_pngd::Parsed p;
    PFrame fr;
    std::memset(&fr, 0, sizeof fr);
    std::vector<PSeg> segs;
    PPlan pl;
    size_t nslots = 0;
    uint32_t maxslots = 0;
    const uint32_t chunk_bytes = spec_chunk_bytes(asked);
    fr.status = uwip_pngd::parse(stream.data(), stream.size(), p);
    if (fr.status == 0 && ((int64_t)p.H != rows || (int64_t)p.W != cols || (p.spp >= 3 && channels == 1))) fr.status = UWIP_PNG_SIZE_MISMATCH;
    fr.spp = fr.status == 0 ? p.spp : 1;
    if (fr.status == 0) {
        plan_frame(fr, p, rows, cols, segmented, segs, 0, pl);
        if (segmented == 2) spec_plan_frame(fr, chunk_bytes, nslots, maxslots);
    }
    // exact sizes, so that the address sanitizer sees an index one past any of them
    const size_t wsb = ws_bytes(rows, cols), nsegtot = segs.size();
    const uint32_t npieces = (uint32_t)((wsb + kChunk - 1) / kChunk);
    std::vector<uint8_t> src(pl.src_bytes + 16, 0), ws(n * wsb + 16, 0xEE);
    if (fr.status == 0) uwip_pngd::gather(stream.data(), p, src.data() + fr.zoff);
    std::vector<PRes> res(nsegtot + n, PRes{7u, 7u, 7u, 7u});
    std::vector<uint32_t> asum((size_t)n * npieces * 2, 0x55555555u);
    std::vector<uint8_t> meta(nslots ? spec_meta_bytes(n, nslots) - 16 : 0, 0xDD);      // exact: no slack behind the records
    std::vector<uint16_t> sym(nslots ? n * wsb : 0, 0xDDDD);
    PBufs B;
    B.fr = &fr; B.seg = segs.data(); B.src = src.data(); B.ws = ws.data(); B.res = res.data(); B.asum = asum.data();
    B.status = status; B.counts = seen.counts; B.nsegtot = (uint32_t)nsegtot; B.nframes = n;
    PGeoD g;
    g.rows = rows; g.cols = cols; g.ws_stride = (uint32_t)wsb; g.npieces = npieces;
    if (nsegtot) launch((unsigned)nsegtot, 1, 64, true, [=] { k_pngd_inflate(B, g, 0); });
    if (nslots) {
        spec_bind(B, meta.data(), sym.data(), n, nslots, chunk_bytes);
        launch(1, 1, 64, false, [=] { k_pngs_begin(B); });
        const bool took_path = B.spec[0].open != 0u;
        launch(maxslots - kRepairs, n, 64, true, [=] { k_pngs_measure(B, g, 0); });
        launch(1, 1, 64, false, [=] { k_pngs_verify(B, g); });
        for (int r = 0; r < kRepairs; ++r) {
            launch(1, n, 64, true, [=] { k_pngs_measure(B, g, 1); });
            launch(1, 1, 64, false, [=] { k_pngs_verify(B, g); });
        }
        // the library launches maxslots workgroups per frame; those at and behind nacc return at once, and a host thread each
        // is what this harness spends its time on, so they are left out here (one stays, to return at once)
        const unsigned nacc1 = std::min<unsigned>(maxslots, (B.spec[0].ok ? B.spec[0].nacc : 0u) + 1u);
        launch(nacc1, n, 64, true, [=] { k_pngs_write(B, g); });
        launch(n, 1, 256, true, [=] { k_pngs_window(B, g); });
        launch(nacc1, n, 256, true, [=] { k_pngs_resolve(B, g); });
        for (uint32_t c = 1; took_path && c < fr.nchunks; ++c) {
            seen.tried += B.chunk[fr.chunk0 + c].tries;
            seen.valid += B.chunk[fr.chunk0 + c].flags & kChunkValid;
        }
        if (B.spec[0].ok)
            for (uint32_t i = 0; i < B.spec[0].nacc; ++i) seen.starts.push_back(B.chunk[fr.chunk0 + B.order[fr.chunk0 + i]].start);
    }
    launch(n, 1, 64, true, [=] { k_pngd_inflate(B, g, 1); });
    launch(npieces, n, 256, true, [=] { k_pngd_adler(B, g); });
    launch(n, 1, 64, true, [=] { k_pngd_unfilter(B, g); });
    launch(uwip_cdiv((size_t)rows * cols, 256), n, 256, false, [=] { k_pngd_color(B, g, out, step, fs, channels); });
    for (const PRes &r : res) if (r.maxdist != 7u || r.ok != 7u) seen.maxdist = std::max(seen.maxdist, r.maxdist);
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
        if (!(is >> path >> segmented >> channels >> asked)) continue;
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
        Seen seen;
        decode(s, segmented, asked, out, step, fs, rows, cols, channels, &status, seen);
        bool equal = host_ok && status == 0, clean = true;
        for (int y = 0; y < rows && equal; ++y) equal = !std::memcmp(out + y * step, host.data.data() + (size_t)y * cols * channels, (size_t)cols * channels);
        for (size_t i = 0; i < buf.size(); ++i) {
            const size_t o = i < 3 ? SIZE_MAX : i - 3;
            const bool inside = o != SIZE_MAX && o / step < (size_t)rows && o % step < (size_t)cols * channels;
            if (!inside && buf[i] != 0xA5) clean = false;
        }
        std::printf("%s %d %d status %d host %d equal %d clean %d accepted %llu serial %llu maxdist %u starts %zu", path.c_str(), segmented, asked,
                    status, (int)host_ok, (int)equal, (int)clean, seen.counts[0], seen.counts[1], seen.maxdist, seen.starts.size());
        for (uint32_t b : seen.starts) std::printf(" %u", b);
        std::printf(" tried %u valid %u\n", seen.tried, seen.valid);
        std::fflush(stdout);
    }
    return 0;
}
