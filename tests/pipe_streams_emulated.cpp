// The kernels of uwimageproc_amd/csrc/pipe_streams.hip (blank, select, gather, carry, table, pack) executed on the host, thread
// for thread, against a serial restatement written here: random ring contents and sizes, zero rows, F + 1 rows, a row on the
// carried frame, a negative size in the middle of the list (the later offsets skip it), misaligned sizes and bases (the 16-byte
// and the byte paths of the copies both run), guard bytes behind every buffer.  tests/test_pipe_streams_emulated.py cuts the
// kernels out of the .hip file into kernels.inc (everything inside its first anonymous namespace) and builds this file with the
// host compiler under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <random>
#include "hip_on_host.hpp"
static thread_local d3 gridDim;
#include "pipe_streams.hpp"
#include "kernels.inc"

// a grid of gx x gy workgroups of bs threads; the threads of a workgroup run at the same time
template <class Fn> static void run(unsigned gx, unsigned gy, unsigned bs, Fn f)
{
    for (unsigned by = 0; by < gy; ++by) for (unsigned bx = 0; bx < gx; ++bx) {
        std::barrier<> bar(bs);
        std::vector<std::thread> th;
        for (unsigned t = 0; t < bs; ++t)
            th.emplace_back([=, &bar] {
                g_bar = &bar; threadIdx.x = t; blockDim.x = bs; blockIdx.x = bx; blockIdx.y = by; gridDim.x = gx; gridDim.y = gy;
                f();
            });
        for (auto &t : th) t.join();
    }
}

// the copy kernels stride by blockDim and gridDim: fewer threads per workgroup than the device's 256 walk the same paths
constexpr unsigned kCopyThreads = 24;
static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

constexpr uint8_t GUARD = 0xEE;
// a buffer of n bytes at an offset `mis` from a 16-byte boundary, with 64 guard bytes on both sides
struct Guarded {
    std::vector<uint8_t> raw;
    size_t n, lead;
    Guarded(size_t n_, size_t mis, uint8_t fill) : raw(n_ + 160, GUARD), n(n_)
    {
        lead = 64 + ((16 - ((uintptr_t)raw.data() + 64) % 16) % 16) + mis;
        std::memset(p(), fill, n);
    }
    uint8_t *p() { return raw.data() + lead; }
    bool guards_ok() const
    {
        for (size_t i = 0; i < lead; ++i) if (raw[i] != GUARD) return false;
        for (size_t i = lead + n; i < raw.size(); ++i) if (raw[i] != GUARD) return false;
        return true;
    }
};

int main()
{
    std::mt19937 rng(11);
    int ncase = 0;
    // ---- blank: frames with a negative status are zeroed, the others untouched; odd frame sizes and bases
    for (size_t fb : {1u, 15u, 16u, 17u, 777u, 4096u + 5u}) for (size_t mis : {0u, 3u}) {
        const int F = 5;
        Guarded g(fb * F, mis, 0);
        std::vector<uint8_t> want(fb * F);
        for (auto &v : want) v = (uint8_t)(1 + rng() % 255);
        std::memcpy(g.p(), want.data(), want.size());
        const int32_t status[F] = {0, -1, 0, -3, -2};
        for (int f = 0; f < F; ++f) if (status[f] < 0) std::memset(want.data() + f * fb, 0, fb);
        uint8_t *frames = g.p();
        run(2, F, kCopyThreads, [=] { k_ps_blank(frames, fb, status); });
        ++ncase;
        CHECK(!std::memcmp(g.p(), want.data(), want.size()) && g.guards_ok(), "blank fb %zu mis %zu", fb, mis);
    }
    // ---- select, gather, carry, table, pack: random steps
    for (int it = 0; it < 40; ++it) {
        const int F = it % 3 == 0 ? 4 : 1 + (int)(rng() % 6);
        const int emit_all = it % 4 == 3;
        static const size_t kFrameBytes[4] = {36, 47, 64, 333};
        const size_t fb = kFrameBytes[rng() % 4];       // bytes per "frame": multiples of 16 and not
        const size_t mis = rng() % 2 ? 0 : 1 + rng() % 15;
        const int max_rows = 3 + (int)(rng() % 6) + F;
        const int base = (int)(rng() % 3) * F;
        const int valid = emit_all && it % 8 == 7 ? 1 + (int)(rng() % F) : F;
        // rows this step closed: 0, F + 1, or something between; some on the carried frame (an index below base)
        int nrows = it % 5 == 0 ? 0 : it % 5 == 1 ? F + 1 : (int)(rng() % (F + 2));
        const uint32_t emitted0 = (uint32_t)(rng() % 1000);                 // rows handed out before this step: any place in the ring
        const uint32_t total = emitted0 + (uint32_t)nrows;
        std::vector<uwip_keyframe_row> ring(max_rows);
        for (auto &r : ring) { r.id = -77; r.frame = -77; r.index = 1 << 20; r.overlap = r.blur = 0; }
        std::vector<uwip_ps::Sel> want_sel;
        std::vector<int32_t> status(F);
        for (auto &s : status) s = rng() % 4 == 0 ? -1 - (int)(rng() % 3) : 0;
        if (emit_all) {
            for (int f = 0; f < valid; ++f) if (status[f] >= 0) want_sel.push_back({f, base + f, -1, 0});
        } else {
            for (int r = 0; r < nrows; ++r) {
                uwip_keyframe_row &row = ring[(emitted0 + (uint32_t)r) % (uint32_t)max_rows];
                const bool carried = (r == 0 && base > 0 && rng() % 2) || (it % 5 == 1 && r == 0 && base > 0);
                row.index = carried ? base - 1 - (int)(rng() % base) : base + (int)(rng() % F);
                row.id = 100 + r; row.frame = row.index + (int)(rng() % 2);
                want_sel.push_back({carried ? F : row.index - base, row.index, row.id, 0});
            }
        }
        const int n = (int)want_sel.size();
        Guarded work(fb * F, mis, 0), carried(fb, (mis + 5) % 16, 0), compact(fb * (F + 1), (mis + 9) % 16, 0xCC);
        for (size_t i = 0; i < work.n; ++i) work.p()[i] = (uint8_t)rng();
        for (size_t i = 0; i < carried.n; ++i) carried.p()[i] = (uint8_t)rng();
        std::vector<uint8_t> want_compact(compact.n, 0xCC), carried0(carried.p(), carried.p() + fb);
        for (int e = 0; e < n; ++e)
            std::memcpy(want_compact.data() + e * fb, want_sel[e].src < F ? work.p() + want_sel[e].src * fb : carried0.data(), fb);
        std::vector<uwip_ps::Sel> sel(F + 2, uwip_ps::Sel{-9, -9, -9, -9});
        int32_t sel_n = -5;
        uint32_t emitted = emitted0;
        {
            const int32_t *st = status.data();
            const uwip_keyframe_row *rg = ring.data();
            uwip_ps::Sel *sl = sel.data();
            int32_t *sn = &sel_n;
            uint32_t *em = &emitted;
            const uint32_t *tot = &total;
            run(1, 1, 64, [=] { k_ps_select(emit_all, F, valid, base, st, rg, max_rows, tot, em, sl, sn); });
            const uint8_t *w = work.p(), *c = carried.p();
            uint8_t *cp = compact.p();
            run(2, F + 1, kCopyThreads, [=] { k_ps_gather(w, c, F, fb, sl, sn, cp); });
        }
        ++ncase;
        CHECK(sel_n == n, "select count %d want %d (it %d)", sel_n, n, it);
        for (int e = 0; e < n && sel_n == n; ++e)
            CHECK(sel[e].src == want_sel[e].src && sel[e].index == want_sel[e].index && sel[e].row_id == want_sel[e].row_id, "select entry %d (it %d)", e, it);
        CHECK(sel[F + 1].src == -9, "select wrote past its list (it %d)", it);
        CHECK(emit_all ? emitted == emitted0 : emitted == total, "emitted counter (it %d)", it);
        CHECK(!std::memcmp(compact.p(), want_compact.data(), compact.n) && compact.guards_ok(), "gather (it %d)", it);
        // carry: slot 1 + frame, -1 none; the work frames stay as they are
        const int32_t carry_best = it % 3 == 1 ? -1 : 1 + (int)(rng() % F);
        {
            const uint8_t *w = work.p();
            uint8_t *c = carried.p();
            const int32_t *cb = &carry_best;
            run(3, 1, kCopyThreads, [=] { k_ps_carry(w, F, fb, cb, c); });
        }
        const uint8_t *want_carried = carry_best < 1 ? carried0.data() : work.p() + (carry_best - 1) * fb;
        CHECK(!std::memcmp(carried.p(), want_carried, fb) && carried.guards_ok() && work.guards_ok(), "carry (it %d)", it);
        // table + pack: sizes of every alignment, a negative one in the middle, a zero
        const size_t slot = 200 + rng() % 60;
        std::vector<int64_t> sizes(F + 1, 0);
        for (int e = 0; e < n; ++e) sizes[e] = 1 + (int64_t)(rng() % slot);
        if (n >= 3) sizes[n / 2] = -(int64_t)(slot + 1 + rng() % 1000);
        if (n >= 2 && it % 2) sizes[0] = 0;
        Guarded slots(slot * (F + 1), (mis + 2) % 16, 0), blob(slot * (F + 1), (mis + 7) % 16, 0xDD);
        for (size_t i = 0; i < slots.n; ++i) slots.p()[i] = (uint8_t)rng();
        std::vector<uint8_t> want_blob(blob.n, 0xDD);
        std::vector<uwip_stream_out> want_outs(n);
        uint64_t off = 0;
        for (int e = 0; e < n; ++e) {
            want_outs[e] = {want_sel[e].index, want_sel[e].row_id, sizes[e], (int64_t)off};
            if (sizes[e] > 0) { std::memcpy(want_blob.data() + off, slots.p() + e * slot, (size_t)sizes[e]); off += (uint64_t)sizes[e]; }
        }
        std::vector<float> ratio(F);
        for (auto &r : ratio) r = (float)(rng() % 1000) / 1000.0f;
        Guarded table(uwip_ps::table_bytes(F), 0, 0x55);
        {
            uwip_ps::TableHdr *hdr = (uwip_ps::TableHdr *)table.p();
            uwip_stream_out *outs = (uwip_stream_out *)(table.p() + uwip_ps::outs_offset());
            int32_t *ts = (int32_t *)(table.p() + uwip_ps::status_offset(F));
            float *tr = (float *)(table.p() + uwip_ps::ratio_offset(F));
            int32_t *tp = (int32_t *)(table.p() + uwip_ps::par_offset(F));
            std::vector<int32_t> par4(4 * F), want_par(2 * F, 0);
            for (auto &v : par4) v = (int32_t)(rng() % 64);
            const bool have_par = it % 3 != 2;                              // null: the host made the choice, zeros in the table
            for (int f = 0; f < F && have_par; ++f) { want_par[2 * f] = par4[4 * f]; want_par[2 * f + 1] = par4[4 * f + 1]; }
            const int32_t *pr = have_par ? par4.data() : nullptr;
            const uwip_ps::Sel *sl = sel.data();
            const int32_t *sn = &sel_n, *st = status.data();
            const int64_t *sz = sizes.data();
            const float *rt = ratio.data();
            run(1, 1, 256, [=] { k_ps_table(F, sl, sn, sz, st, rt, pr, hdr, outs, ts, tr, tp); });
            CHECK(!std::memcmp(tp, want_par.data(), 8 * F), "table parameters (it %d)", it);
            const uint8_t *sp = slots.p();
            uint8_t *bp = blob.p();
            run(2, F + 1, kCopyThreads, [=] { k_ps_pack(sp, slot, hdr, outs, bp); });
            CHECK(hdr->n_outs == n && hdr->blob_bytes == off, "table header (it %d): %d %llu want %d %llu", it, hdr->n_outs,
                  (unsigned long long)hdr->blob_bytes, n, (unsigned long long)off);
            for (int e = 0; e < n; ++e)
                CHECK(outs[e].index == want_outs[e].index && outs[e].row_id == want_outs[e].row_id && outs[e].size == want_outs[e].size &&
                          outs[e].offset == want_outs[e].offset, "table out %d (it %d)", e, it);
            CHECK(!std::memcmp(ts, status.data(), 4 * F) && !std::memcmp(tr, ratio.data(), 4 * F), "table status / ratio (it %d)", it);
        }
        CHECK(table.guards_ok(), "table guards (it %d)", it);
        CHECK(!std::memcmp(blob.p(), want_blob.data(), blob.n) && blob.guards_ok() && slots.guards_ok(), "pack (it %d)", it);
    }
    // ---- table: more entries than threads (every thread scans a share of several)
    {
        const int F = 700, n = F + 1;
        std::vector<uwip_ps::Sel> sel(n);
        std::vector<int64_t> sizes(n);
        std::vector<int32_t> status(F, 0);
        std::vector<float> ratio(F, 0.5f);
        for (int e = 0; e < n; ++e) { sel[e] = {e % F, e, e, 0}; sizes[e] = e % 7 == 3 ? -(int64_t)(rng() % 99 + 1) : (int64_t)(rng() % 0x7fffffffu); }
        std::vector<uint8_t> table(uwip_ps::table_bytes(F));
        uwip_ps::TableHdr *hdr = (uwip_ps::TableHdr *)table.data();
        uwip_stream_out *outs = (uwip_stream_out *)(table.data() + uwip_ps::outs_offset());
        int32_t *ts = (int32_t *)(table.data() + uwip_ps::status_offset(F));
        float *tr = (float *)(table.data() + uwip_ps::ratio_offset(F));
        int32_t *tp = (int32_t *)(table.data() + uwip_ps::par_offset(F));
        const uwip_ps::Sel *sl = sel.data();
        const int32_t sel_n = n, *sn = &sel_n, *st = status.data();
        const int64_t *sz = sizes.data();
        const float *rt = ratio.data();
        run(1, 1, 256, [=] { k_ps_table(F, sl, sn, sz, st, rt, nullptr, hdr, outs, ts, tr, tp); });
        uint64_t off = 0;
        ++ncase;
        for (int e = 0; e < n; ++e) {
            CHECK(outs[e].offset == (int64_t)off && outs[e].size == sizes[e], "large table entry %d", e);
            if (sizes[e] > 0) off += (uint64_t)sizes[e];
        }
        CHECK(off > (1ull << 32) && hdr->blob_bytes == off && hdr->n_outs == n, "large table total");
    }
    std::printf("%d cases, %d mismatches\n", ncase, bad);
    return bad != 0;
}
