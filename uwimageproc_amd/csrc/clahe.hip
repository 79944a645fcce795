// The CLAHE core of the aclahe hot path for gfx950.
//
// cv::CLAHE::apply as driven by modules/aclahe/src/aclahe.cpp:175-187 becomes
//   k_clahe_tilehist  per-tile 256-bin histograms (per-wave LDS copies,
//                     BORDER_REFLECT_101 padding folded into the indexing)
//   k_clahe_lut       clip / redistribute / cumulative LUT, one block per
//                     (tile, clip limit, frame)
//   k_clahe_band      the two fused for small or padded tiles, one block per row of tiles
//   k_clahe_apply     bilinear blend of the 4 neighbouring tile LUTs; a block
//                     owns a strip of rows that share (ty1, ty2), stages the
//                     (gx+1) column cells' four LUTs packed as one uint32 per
//                     grey level in LDS, so each pixel costs one ds_read_b32
// The 5 x 51 sweep lives in aclahe_sweep.hip, the stage driver in aclahe_auto.hip; clahe_internal.hpp holds what they share
// with this unit.  All float32 arithmetic keeps OpenCV's operation order (file is compiled with -ffp-contract=off).
#include "clahe_internal.hpp"
#include <cstring>

namespace {

// ---- C1a: tile histograms ---------------------------------------------------
// One WAVE per (tile, row part); a block is four independent waves, no workgroup barrier.  The wave reads its rows as
// ALIGNED dwords (4 pixels per lane and load); a tile narrower than 64 dwords is covered several rows at a time (lane ->
// (row, dword) of a patch), so a 61-pixel tile of the 32 x 32 grid still keeps 51 of the 64 lanes busy.  Bytes of an
// edge dword that lie outside the tile's columns are masked by a per-lane byte mask computed once.  Same-bin atomics of
// one LDS instruction serialise (tools/ubench/lds_rand.hip: 1.7 ns with distinct banks, 53 ns with one word), and
// neighbouring pixels of a smooth underwater frame fall into few bins: the wave's counters are replicated TH_REP times,
// keyed by the lane index modulo TH_REP, with a replica stride of 256 + 8 words (equal bins of different replicas sit in
// different banks).  The reflect-101 padding of a grid that does not divide the image (columns >= cols) is a per-pixel
// loop over the few padded columns; padded rows are index math.
constexpr int TH_REP = 4;
constexpr int TH_RSTRIDE = 256 + 8;
// BP (tiles of >= TH_BP_MIN pixels whose rows are 16-byte aligned runs: the 2x2 ... 8x8 grids of a 1080p or 4K frame): a
// slot-keyed layout -- TH_BP_SLOTS slots per PAIR of bins, two 16-bit counters per word, lane l counts in slot l mod 16 (a
// slot sees the pixels of four lanes: < 65536 for any part below 1 M pixels), 8 KB per wave -- read with 16 pixels per
// lane and load, four row patches in flight.  Measured per 64 frames (tools/tilehist_only.py): replica form 56-62 us;
// 32 slots (one lane pair per bank, 16 KB per wave, 8 waves per CU) 51 us; 16 slots 40 us; 8 slots 59 us; 4 slots 74 us;
// 2 / 4 / 8 row patches in flight 42-45 / 40 / 40 us.  The flush adds the slots of a bin with a lane-rotated slot index.
constexpr int TH_BP_MIN = 8192;
constexpr int TH_BP_SLOTS = 16;
constexpr int TH_BP_WORDS = 128 * TH_BP_SLOTS;
// FORM 2 (round 4): the slot-keyed layout for ANY tile -- the padded 121 x 68 / 61 x 34 tiles of the 16 x 16 / 32 x 32 grids of a
// 1080p frame, unaligned or strided images.  A tile row is read as 16-byte units starting at the tile's own first column
// (unaligned global_load_dwordx4: the hardware splits what crosses a line); the last unit of a row that is not a multiple of
// 16 is loaded ENDING at the tile's last in-image column and its leading bytes -- pixels of the previous unit -- add zero
// (a per-lane mask bit shifted into the increment: no per-pixel branch); reflect-101 padding columns and rows as in the
// replica form.  The replica form spent 90 / 112 us per 64 frames on those grids (4 pixels per load, 16 lanes per replica),
// against 40 us of the slot-keyed form on the aligned grids.
// Measured per 64 frames of 1080p (tools/tilehist_only.py, replica form -> FORM 2): 16 x 16 grid (121 x 68 tiles) 86 -> 67 us;
// 32 x 32 grid (61 x 34 tiles = 2074 pixels: 33 pixels per lane against an 8 KB zero + 2048-slot flush per wave, three row
// passes of 16 rows for 34 rows) 107 -> 157 us: those stay with the replica form.
constexpr int TH_G_MIN = 4096;            // pixels per tile from which the 8 KB zero + flush of the slot-keyed layout pays
template <int FORM>
__global__ __launch_bounds__(256) void k_clahe_tilehist(const uint8_t *__restrict__ src,
                                                        size_t step, size_t fstride, int rows,
                                                        int cols, int gx, int tw, int th, int split,
                                                        int rows_per_part,
                                                        const int *__restrict__ frame_map,
                                                        uint32_t *__restrict__ hists, int tiles,
                                                        const int *__restrict__ nf_dev /*optional: frames that take part*/)
{
    if (nf_dev && (int)blockIdx.y >= *nf_dev) return;
    constexpr bool BP = FORM != 0;
    constexpr int HWORDS = BP ? TH_BP_WORDS : TH_REP * TH_RSTRIDE;
    __shared__ __attribute__((aligned(16))) uint32_t sh[4][HWORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wave;
    if (item >= tiles * split) return;
    uint32_t *H = sh[wave];
    if (BP) for (int i = lane; i < HWORDS / 4; i += 64) reinterpret_cast<uint4 *>(H)[i] = make_uint4(0, 0, 0, 0);
    else for (int i = lane; i < HWORDS; i += 64) H[i] = 0;
    const int t = item / split, part = item - t * split;
    const int ty = t / gx, tx = t - ty * gx;
    const int f = blockIdx.y;
    const int fr = frame_map ? frame_map[f] : f;
    const uint8_t *base = src + (size_t)fr * fstride;
    const int j0 = part * rows_per_part, j1 = min(th, j0 + rows_per_part);
    uint32_t *my = BP ? H + (lane & (TH_BP_SLOTS - 1)) : H + (lane % TH_REP) * TH_RSTRIDE;
    // count one pixel of value v
    auto add = [&](uint32_t v) {
        if (BP) atomicAdd(&my[(v >> 1) * TH_BP_SLOTS], (v & 1u) ? 65536u : 1u);
        else atomicAdd(&my[v], 1u);
    };
    const int xs = tx * tw, xe = max(xs, min(xs + tw, cols));   // in-image columns [xs, xe); [xe, xs + tw) is reflected padding
    const bool vec = ((reinterpret_cast<uintptr_t>(base) | step) & 3u) == 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if constexpr (FORM == 2) {
        struct __attribute__((packed, aligned(1))) U16 { uint32_t x, y, z, w; };      // 16 bytes at any address
        const int n_in = xe - xs;
        if (n_in > 0) {
            const int nu = (n_in + 15) >> 4, CW = min(nu, 64), RW = 64 / CW;
            const int r = lane / CW, c = lane - r * CW;
            if (r < RW) {
                for (int cb = c; cb < nu; cb += 64) {
                    const int x0 = xs + cb * 16;
                    int xl = x0;
                    uint32_t vm = 0xffffu;                 // bit k: byte k of the unit is a pixel of this unit
                    if (x0 + 16 > xe) { xl = xe - 16; vm = (0xffffu << (x0 - xl)) & 0xffffu; }     // host: cols >= 16
                    const uint8_t *colp = base + xl;
                    constexpr int U = 4;
                    for (int j = j0 + r; j < j1; j += RW * U) {
                        U16 w[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int jj = min(j + u * RW, j1 - 1);           // clamped: a duplicate row is loaded, not counted
                            w[u] = *reinterpret_cast<const U16 *>(colp + (size_t)reflect101(ty * th + jj, rows) * step);
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            if (j + u * RW >= j1) break;
                            const uint32_t q[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
                            for (int k = 0; k < 4; ++k)
#pragma unroll
                                for (int b = 0; b < 4; ++b) {
                                    const uint32_t v = (q[k] >> (8 * b)) & 255u;
                                    atomicAdd(&my[(v >> 1) * TH_BP_SLOTS], ((vm >> (4 * k + b)) & 1u) << ((v & 1u) << 4));
                                }
                        }
                    }
                }
            }
        }
    } else if constexpr (FORM == 1) {
        // fast path (host guarantees: rows 16-byte aligned, tw a multiple of 16, no padded columns): 16 pixels per lane
        // and load, the wave covers RW rows x CW 16-byte units, four such patches in flight (4 KB per wave: at 8 waves
        // per CU that is what the HBM latency needs)
        const int n16 = tw >> 4, CW = min(n16, 64), RW = 64 / CW;
        const int r = lane / CW, c = lane - r * CW;
        if (r < RW) {
            for (int cb = c; cb < n16; cb += 64) {
                const uint8_t *colp = base + xs + cb * 16;
                constexpr int U = 4;
                for (int j = j0 + r; j < j1; j += RW * U) {
                    uint4 w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int jj = min(j + u * RW, j1 - 1);           // clamped: a duplicate row is loaded, not counted
                        w[u] = *reinterpret_cast<const uint4 *>(colp + (size_t)reflect101(ty * th + jj, rows) * step);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (j + u * RW >= j1) break;
                        const uint32_t q[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) { add(q[k] & 255u); add((q[k] >> 8) & 255u); add((q[k] >> 16) & 255u); add(q[k] >> 24); }
                    }
                }
            }
        }
    } else if (xe > xs) {
        // units along a row: aligned dwords (vec) or single pixels; the wave covers a patch of RW rows x CW units
        const int u0 = vec ? (xs >> 2) : xs, nu = vec ? ((xe + 3) >> 2) - u0 : xe - xs;
        const int CW = min(nu, 64), RW = 64 / CW;
        const int r = lane / CW, c = lane - r * CW;
        if (r < RW) {
            for (int cb = c; cb < nu; cb += 64) {
                const int u = u0 + cb;
                uint32_t bmask = 0xfu;          // which bytes of the dword are columns of this tile
                bool whole = true;              // the dword may be loaded as one (it ends inside the image row)
                if (vec) {
                    bmask = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) bmask |= (4 * u + k >= xs && 4 * u + k < xe) ? (1u << k) : 0u;
                    whole = 4 * u + 4 <= cols;
                }
                for (int j = j0 + r; j < j1; j += RW) {
                    const int y = reflect101(ty * th + j, rows);
                    const uint8_t *row = base + (size_t)y * step;
                    if (!vec) { add(row[u]); continue; }
                    if (bmask == 0xfu) {
                        const uint32_t w = reinterpret_cast<const uint32_t *>(row)[u];
                        add(w & 255u); add((w >> 8) & 255u); add((w >> 16) & 255u); add(w >> 24);
                    } else {
                        uint32_t w = 0;
                        if (whole) w = reinterpret_cast<const uint32_t *>(row)[u];
                        else {
#pragma unroll
                            for (int k = 0; k < 4; ++k) if (bmask & (1u << k)) w |= (uint32_t)row[4 * u + k] << (8 * k);
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k) if (bmask & (1u << k)) add((w >> (8 * k)) & 255u);
                    }
                }
            }
        }
    }
    // reflected padding columns [xe, xs + tw): a handful per row
    const int npad = FORM == 1 ? 0 : xs + tw - xe;
    if (npad > 0) {
        for (int i = lane; i < npad * (j1 - j0); i += 64) {
            const int jr = i / npad, x = xe + (i - jr * npad);
            const int y = reflect101(ty * th + j0 + jr, rows);
            add(base[(size_t)y * step + reflect101(x, cols)]);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint32_t *out = hists + ((size_t)f * tiles + t) * 256;
    if (BP) {
        for (int bp = lane; bp < 128; bp += 64) {
            uint32_t lo = 0, hi = 0;
#pragma unroll 8
            for (int q = 0; q < TH_BP_SLOTS; ++q) {
                const uint32_t w = H[bp * TH_BP_SLOTS + ((q + lane) & (TH_BP_SLOTS - 1))];      // lane-rotated slot: spreads the banks
                lo += w & 0xffffu; hi += w >> 16;
            }
            if (split == 1) { out[2 * bp] = lo; out[2 * bp + 1] = hi; }
            else { if (lo) atomicAdd(&out[2 * bp], lo); if (hi) atomicAdd(&out[2 * bp + 1], hi); }
        }
        return;
    }
    for (int bn = lane; bn < 256; bn += 64) {
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < TH_REP; ++q) sum += H[q * TH_RSTRIDE + bn];
        if (split == 1) out[bn] = sum;                  // the only writer: no memset, no atomic
        else if (sum) atomicAdd(&out[bn], sum);
    }
}

// Histograms of a g x g grid from those of the 2g x 2g grid when neither is padded (a tile is then exactly four
// tiles of the finer grid): no second pass over the image.
__global__ __launch_bounds__(256) void k_clahe_tilehist_merge(const uint32_t *__restrict__ child, int gx, int tiles,
                                                              uint32_t *__restrict__ hists)
{
    const int t = blockIdx.x, f = blockIdx.y, v = threadIdx.x;
    const int ty = t / gx, tx = t - ty * gx, gx2 = 2 * gx;
    const uint32_t *c = child + (size_t)f * tiles * 4 * 256;
    const size_t c00 = (size_t)(2 * ty) * gx2 + 2 * tx;
    hists[((size_t)f * tiles + t) * 256 + v] = c[c00 * 256 + v] + c[(c00 + 1) * 256 + v] + c[(c00 + gx2) * 256 + v] + c[(c00 + gx2 + 1) * 256 + v];
}

__global__ __launch_bounds__(256) void k_clahe_lut(const uint32_t *__restrict__ hists, int tiles, int nf,
                                                   float lutScale, ClipList cl,
                                                   const int *__restrict__ frame_clip, int rule,
                                                   uint8_t *__restrict__ luts, uint32_t *__restrict__ tile_max /*optional*/,
                                                   const int *__restrict__ nf_dev /*optional*/)
{
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= (long long)tiles * nf) return;
    const int f = (int)(wv / tiles), t = (int)(wv - (long long)f * tiles);
    if (nf_dev && f >= *nf_dev) return;
    const uint4 hv = *reinterpret_cast<const uint4 *>(hists + ((size_t)f * tiles + t) * 256 + lane * 4);
    const int h0[4] = {(int)hv.x, (int)hv.y, (int)hv.z, (int)hv.w};
    // [frame][tile][clip limit][256]: the wave's rows are one contiguous run (ncl = 1: the plain [frame][tile][256] table)
    clahe_lut_rows(h0, lane, lutScale, cl, frame_clip ? frame_clip[f] : -1, rule, luts + (((size_t)f * tiles + t) * cl.n) * 256,
                   tile_max ? tile_max + (size_t)f * tiles + t : nullptr);
}

// ---- C1a + C1b fused for small or padded tiles: one block per ROW OF TILES (round 4) -------------------------------------------
// The 61 x 34 tiles of the 32 x 32 grid of a 1080p frame (and the 121 x 68 ones of 16 x 16) are too small for a per-wave
// histogram image (8 KB of zeroing and flushing per 2074 pixels) and not aligned to anything, which left the replica form
// at 107 us per 64 frames against 40 us on the big aligned tiles.  Here a 512-thread block owns one row of tiles of one
// frame: gx histograms in LDS -- two 16-bit counters per word, BAND_SLOTS lane-keyed slots per pair of bins, tiles skewed by
// four banks -- filled from WHOLE IMAGE ROWS read as 16-byte units (a unit straddles at most two tiles: the counter base of
// each of its 16 pixels is precomputed per lane, the units a lane owns sit in the same columns of every row), the
// reflect-101 padding columns on a per-pixel path, padding rows by index; then the block's waves turn the histograms into
// LUT rows themselves (clahe_lut_rows) -- the 1 KB per tile of histogram never travels to HBM and back, and there is no
// second launch.
constexpr int BAND_SLOTS = 4;
constexpr int BAND_TSTRIDE = 128 * BAND_SLOTS + 4;          // words per tile: + 4 = the bank skew between neighbouring tiles
constexpr int BAND_THREADS = 512;
// A block may own a PART of the row of tiles (tpb tiles: the 32 tiles of a 32 x 32 grid as two blocks of 16, 33 KB of LDS
// each, four blocks per CU like the 16 x 16 grid instead of two at 66 KB): units at a part's edge straddle a neighbouring
// part's tile, whose pixels add zero here.  (Measured and dropped: the same image as 32-bit counters with two slots per bin --
// 3 instead of 7 vector instructions per pixel, twice the lanes per slot: 16 x 16 grid 48 -> 65 us, 32 x 32 64 -> 62: the
// kernel is bound by LDS collisions, not by its instruction count.)
template <int CHUNKS>       // 64-unit chunks per part of an image row (1, 2, 4, 8); BAND_THREADS / 64 / CHUNKS waves share a chunk
__global__ __launch_bounds__(BAND_THREADS) void k_clahe_band(const uint8_t *__restrict__ src, size_t step, size_t fstride, int rows, int cols,
                                                             int gx, int tw, uint32_t tw_magic, int th, int tpb, int nparts,
                                                             const int *__restrict__ frame_map, float lutScale,
                                                             ClipList cl, const int *__restrict__ frame_clip, int rule,
                                                             uint8_t *__restrict__ luts, uint32_t *__restrict__ tile_max, int tiles,
                                                             const int *__restrict__ nf_dev /*optional*/)
{
    if (nf_dev && (int)blockIdx.y >= *nf_dev) return;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_band[];      // [tpb][BAND_TSTRIDE]
    struct __attribute__((packed, aligned(1))) U16 { uint32_t x, y, z, w; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = (int)blockIdx.x / nparts, part = (int)blockIdx.x - ty * nparts, f = blockIdx.y;
    const int tx0 = part * tpb, ntx = min(tpb, gx - tx0);
    const int xA = tx0 * tw, xB = min((tx0 + ntx) * tw, cols);          // this part's in-image columns [xA, xB)
    const int fr = frame_map ? frame_map[f] : f;
    const uint8_t *base = src + (size_t)fr * fstride;
    for (int i = tid; i < ntx * BAND_TSTRIDE; i += BAND_THREADS) s_band[i] = 0;
    __syncthreads();
    constexpr int WPC = BAND_THREADS / 64 / CHUNKS;          // waves per chunk
    const int chunk = wave / WPC, wrow = wave - chunk * WPC;
    const int ua = xA >> 4, ub = (xB + 15) >> 4;             // the 16-byte units (counted from the row start) that touch [xA, xB)
    const int u = ua + chunk * 64 + lane;
    if (u < ub && xB > xA) {
        // this lane's unit: pixels [x0, x0 + 16) of every row -- the last unit of a row whose width is not a multiple of 16
        // is loaded ENDING at the last column and its leading bytes, pixels of the previous unit, add zero
        const int x0 = u * 16;
        int xl = x0;
        uint32_t vm = 0xffffu;
        if (x0 + 16 > cols) { xl = cols - 16; vm = (0xffffu << (x0 - xl)) & 0xffffu; }
        // LDS byte address of the counter image of the tile each of the 16 loaded pixels falls in (+ this lane's slot);
        // pixels left or right of this part's columns belong to another block: their mask bit goes
        uint32_t cbase[16];
        const uint32_t slot = (uint32_t)(lane & (BAND_SLOTS - 1)) * 4u;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int x = xl + k;
            const int tx = (int)__umulhi((unsigned)x, tw_magic);       // x / tw: tw_magic = floor(2^32 / tw) + 1, exact while x * tw < 2^32
            const bool mine = x >= xA && x < xB;
            if (!mine) vm &= ~(1u << k);
            cbase[k] = (uint32_t)(mine ? tx - tx0 : 0) * (BAND_TSTRIDE * 4u) + slot;
        }
        const uint8_t *colp = base + xl;
        constexpr int U = 4;
        for (int j = wrow; j < th; j += WPC * U) {
            U16 w[U];
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int jj = min(j + q * WPC, th - 1);           // clamped: a duplicate row is loaded, not counted
                w[q] = *reinterpret_cast<const U16 *>(colp + (size_t)reflect101(ty * th + jj, rows) * step);
            }
#pragma unroll
            for (int q = 0; q < U; ++q) {
                if (j + q * WPC >= th) break;
                const uint32_t d[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const uint32_t v = (d[k >> 2] >> (8 * (k & 3))) & 255u;
                    const uint32_t inc = ((vm >> k) & 1u) << ((v & 1u) << 4);
                    atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(s_band) + cbase[k] + (v >> 1) * (BAND_SLOTS * 4u)), inc);
                }
            }
        }
    }
    // reflected padding columns [cols, gx * tw): every part counts those that fall into ITS tiles (with a grid that is not a
    // power of two the padding can cover more tiles than the last part owns: cols = 1915, gx = 49 -> tw = 40, padding over
    // tiles 47 and 48, the last part holding tile 48 alone)
    {
        const int pa = max(cols, tx0 * tw), pb = (tx0 + ntx) * tw;
        const int npad = pb - pa;
        for (int i = tid; i < npad * th; i += BAND_THREADS) {
            const int jr = i / npad, x = pa + (i - jr * npad);
            const uint32_t v = base[(size_t)reflect101(ty * th + jr, rows) * step + reflect101(x, cols)];
            const int tx = x / tw - tx0;
            atomicAdd(&s_band[tx * BAND_TSTRIDE + (v >> 1) * BAND_SLOTS + (tid & (BAND_SLOTS - 1))], (v & 1u) ? 65536u : 1u);
        }
    }
    __syncthreads();
    // histograms -> LUT rows: a wave per tile, lane l owns bins 4l .. 4l+3 = pairs 2l, 2l + 1
    for (int tl = wave; tl < ntx; tl += BAND_THREADS / 64) {
        const uint4 a = *reinterpret_cast<const uint4 *>(&s_band[tl * BAND_TSTRIDE + (2 * lane) * BAND_SLOTS]);
        const uint4 b = *reinterpret_cast<const uint4 *>(&s_band[tl * BAND_TSTRIDE + (2 * lane + 1) * BAND_SLOTS]);
        static_assert(BAND_SLOTS == 4, "one 16-byte read per pair of bins");
        // a tile holds < 65536 pixels (host: checked), so the packed halves can be added as whole words
        const uint32_t sa = a.x + a.y + a.z + a.w, sb = b.x + b.y + b.z + b.w;
        const int h0[4] = {(int)(sa & 0xffffu), (int)(sa >> 16), (int)(sb & 0xffffu), (int)(sb >> 16)};
        const int t = ty * gx + tx0 + tl;
        clahe_lut_rows(h0, lane, lutScale, cl, frame_clip ? frame_clip[f] : -1, rule, luts + (((size_t)f * tiles + t) * cl.n) * 256,
                       tile_max ? tile_max + (size_t)f * tiles + t : nullptr);
    }
}

// ---- C1c: bilinear LUT interpolation, strip per block (ApplyFrame: clahe_internal.hpp) ---------
template <bool VEC>
__global__ __launch_bounds__(256) void k_clahe_apply(const uint8_t *__restrict__ src, size_t sstep,
                                                     size_t sfs, uint8_t *__restrict__ dst,
                                                     size_t dstep, size_t dfs, int cols, int gx,
                                                     int gy, float inv_tw, float inv_th,
                                                     const uint8_t *__restrict__ luts,
                                                     size_t lut_fs, const int4 *__restrict__ strips,
                                                     const int *__restrict__ frame_map, int TX, int xs,
                                                     const ApplyFrame *__restrict__ desc)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_pack[];   // [cells of this block's columns][256]
    const int tid = threadIdx.x;
    const int f = blockIdx.y;
    int fr = frame_map ? frame_map[f] : f;
    const uint8_t *lbase = luts + (size_t)f * lut_fs;
    int nstrips = (int)gridDim.x / max(xs, 1);
    if (desc) {                                     // block-uniform
        const ApplyFrame d = desc[f];
        strips = d.strips; lbase = d.luts; fr = d.fr; gx = d.gx; gy = d.gy; TX = d.TX; xs = d.xs; inv_tw = d.inv_tw; inv_th = d.inv_th;
        nstrips = d.nstrips;
    }
    // A block = one strip of rows that share (ty1, ty2) x one of xs column parts: the LUT row it stages (1 KB per
    // interpolation cell) shrinks with the part, and tall strips amortise it over more rows (at 32 x 32 tiles and 16-row
    // strips the LUT row was as many bytes as the pixels).
    const int strip = (int)blockIdx.x / xs, part = (int)blockIdx.x - strip * xs;
    if (strip >= nstrips) return;
    const int4 sd = strips[strip];
    const int cy = sd.x, r0 = sd.y, r1 = sd.z;
    const int groups = (cols + 7) / 8;
    const int g_lo = (int)(((long long)groups * part) / xs), g_hi = (int)(((long long)groups * (part + 1)) / xs);
    if (g_lo >= g_hi) return;
    // cells touched by columns [8 g_lo, 8 g_hi): cell(x) = floor(x * inv_tw - 0.5) + 1, non-decreasing in x
    const int c_lo = (int)floorf((float)(g_lo * 8) * inv_tw - 0.5f) + 1;
    const int c_hi = (int)floorf((float)(min(g_hi * 8, cols) - 1) * inv_tw - 0.5f) + 1;
    // the packed LUT row of this strip's cells, built while it is staged: entry v of interpolation cell c holds the four
    // neighbour tiles' LUT bytes TL | TR << 8 | BL << 16 | BR << 24.  A thread takes four grey levels of a cell: one dword
    // from each of the four tile LUTs (L2 hits: a tile serves four cells and every strip of its cell rows), byte-
    // transposed by v_perm, one 16-byte LDS store.  (Round 2 packed the rows in a kernel of its own and staged copies.)
    {
        const uint32_t *L4 = reinterpret_cast<const uint32_t *>(lbase);
        const int ty1 = max(cy - 1, 0), ty2 = min(cy, gy - 1);
        for (int idx = tid; idx < (c_hi - c_lo + 1) * 64; idx += 256) {
            const int c = c_lo + (idx >> 6), v4 = idx & 63;
            const int tx1 = max(c - 1, 0), tx2 = min(c, gx - 1);
            const uint32_t a = L4[((size_t)ty1 * gx + tx1) * 64 + v4], b = L4[((size_t)ty1 * gx + tx2) * 64 + v4];
            const uint32_t cc = L4[((size_t)ty2 * gx + tx1) * 64 + v4], d = L4[((size_t)ty2 * gx + tx2) * 64 + v4];
            const uint32_t t0 = __builtin_amdgcn_perm(b, a, 0x05010400u), t1 = __builtin_amdgcn_perm(b, a, 0x07030602u);
            const uint32_t u0 = __builtin_amdgcn_perm(d, cc, 0x05010400u), u1 = __builtin_amdgcn_perm(d, cc, 0x07030602u);
            reinterpret_cast<uint4 *>(s_pack)[idx] =
                make_uint4(__builtin_amdgcn_perm(u0, t0, 0x05040100u), __builtin_amdgcn_perm(u0, t0, 0x07060302u),
                           __builtin_amdgcn_perm(u1, t1, 0x05040100u), __builtin_amdgcn_perm(u1, t1, 0x07060302u));
        }
    }
    __syncthreads();
    const uint8_t *sb = src + (size_t)fr * sfs;
    uint8_t *db = dst + (size_t)fr * dfs;
    const int tx = tid % TX, ty = tid / TX, TY = 256 / TX;
    for (int g = g_lo + tx; g < g_hi; g += TX) {
        const int x0 = g * 8;
        uint32_t base[8];
        float xa[8], xa1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float txf = (float)(x0 + i) * inv_tw - 0.5f;
            const float fl = floorf(txf);
            xa[i] = txf - fl;
            xa1[i] = 1.0f - xa[i];
            base[i] = (uint32_t)(((int)fl + 1 - c_lo) << 8);
        }
        const bool full = VEC && (x0 + 8 <= cols);
        constexpr int RU = 4;                       // rows in flight per thread (memory-level parallelism)
        for (int yb = r0 + ty; yb < r1; yb += TY * RU) {
            uint32_t w[RU][2];
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int y = yb + u * TY;
                w[u][0] = w[u][1] = 0;
                if (y < r1) {
                    const uint8_t *sp = sb + (size_t)y * sstep + x0;
                    if (full) {
                        const uint2 q = *reinterpret_cast<const uint2 *>(sp);
                        w[u][0] = q.x; w[u][1] = q.y;
                    } else {
                        for (int i = 0; i < min(8, cols - x0); ++i) w[u][i >> 2] |= (uint32_t)sp[i] << ((i & 3) * 8);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int y = yb + u * TY;
                if (y >= r1) break;
                const float tyf = (float)y * inv_th - 0.5f;
                const float ya = tyf - floorf(tyf), ya1 = 1.0f - ya;
                uint8_t *dp = db + (size_t)y * dstep + x0;
                uint32_t o[2] = {0, 0};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t v = (w[u][i >> 2] >> ((i & 3) * 8)) & 255u;
                    const uint32_t p = s_pack[base[i] + v];
                    const float res = clahe_blend(p & 255u, (p >> 8) & 255u, (p >> 16) & 255u, p >> 24, xa1[i], xa[i], ya1, ya);
                    // v_cvt_pk_u8_f32: round-to-nearest-even + clamp + byte insert in one instruction
                    o[i >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(res, i & 3, o[i >> 2]);
                }
                if (full) {
                    *reinterpret_cast<uint2 *>(dp) = make_uint2(o[0], o[1]);
                } else {
                    for (int i = 0; i < min(8, cols - x0); ++i) dp[i] = (uint8_t)(o[i >> 2] >> ((i & 3) * 8));
                }
            }
        }
    }
}

// -----------------------------------------------------------------------------
// the kernels' clip list from the launchers' (clip, ncl) (null: zeros -- the launch reads per-frame clips instead)
ClipList make_clip_list(const int *clip, int ncl)
{
    ClipList cl{};
    cl.n = ncl;
    if (clip) memcpy(cl.clip, clip, sizeof(int) * (size_t)ncl);
    return cl;
}

// the big-tile (slot-keyed, FORM 1) tile histogram applies: tiles of >= TH_BP_MIN pixels whose rows are 16-byte aligned runs
bool big_tile_ok(const uwip_batch_u8 *src, const ClaheGeom &g)
{
    return (long long)g.tw * g.th >= TH_BP_MIN && (g.tw & 15) == 0 && g.tw * g.gx == g.cols && g.tw < (1 << 17) &&
           ((reinterpret_cast<uintptr_t>(src->data) | src->step | src->frame_stride) & 15u) == 0;
}

}  // namespace

int uwip_clahe_launch_tilehist(uwip_ctx *ctx, const uwip_batch_u8 *src, const ClaheGeom &g, const int *d_frame_map, int nf,
                               uint32_t *d_hists, const int *d_nf)
{
    const int tiles = g.gx * g.gy;
    // one wave per (tile, row part).  Large aligned tiles take the slot-keyed form: parts of >= TH_BP_MIN pixels, enough of
    // them for ~4096 waves; small or unaligned tiles the replica form: enough parts for >= 16384 waves, at
    // least 8 rows each.
    // The slot-keyed form counts in 16-bit halves: a slot is shared by the lanes l = s mod 16 of a wave, at most 4 of at
    // least 33 active ones, so it sees at most 1/8 of its part's pixels -- a part must stay below 2^19 pixels or a constant
    // (saturated / black) tile carries the even bin's counter into the odd bin's.  TH_BP_PART_MAX keeps a margin for
    // the rounding of rows_per_part (one more row of < 2^17 columns); wider tiles take the 32-bit replica form.
    constexpr long long TH_BP_PART_MAX = 3ll << 17;                   // 393 216 pixels
    const bool bp = big_tile_ok(src, g);
    // FORM 2: any other tile of >= TH_G_MIN pixels in an image at least 16 columns wide (the tail unit of a row is loaded
    // ending at the tile's last in-image column)
    const bool bpg = !bp && (long long)g.tw * g.th >= TH_G_MIN && g.cols >= 16 && g.tw >= 16 && g.tw < (1 << 17);
    int split;
    if (bp || bpg) {
        split = (int)(((bp ? 4096 : 16384) + (size_t)tiles * nf - 1) / ((size_t)tiles * nf));
        split = std::max(1, std::min(split, (int)(((long long)g.tw * g.th) / (bp ? TH_BP_MIN : TH_G_MIN))));
        split = std::max(split, (int)(((long long)g.tw * g.th + TH_BP_PART_MAX - 1) / TH_BP_PART_MAX));
        split = std::min(split, g.th);
    } else {
        split = (int)((16384 + (size_t)tiles * nf - 1) / ((size_t)tiles * nf));
        split = std::max(1, std::min(split, std::max(1, g.th / 8)));
    }
    const int rpp = (g.th + split - 1) / split;
    split = (g.th + rpp - 1) / rpp;                       // no empty parts
    if (split > 1) UWIP_HIP(ctx, hipMemsetAsync(d_hists, 0, sizeof(uint32_t) * 256 * (size_t)tiles * nf, ctx->stream));
    dim3 grid((unsigned)((tiles * split + 3) / 4), (unsigned)nf);
    uwip_kscope ks(ctx, "k_clahe_tilehist");
    if (bp)
        k_clahe_tilehist<1><<<grid, 256, 0, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, g.rows, g.cols,
                                                           g.gx, g.tw, g.th, split, rpp, d_frame_map, d_hists, tiles, d_nf);
    else if (bpg)
        k_clahe_tilehist<2><<<grid, 256, 0, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, g.rows, g.cols,
                                                           g.gx, g.tw, g.th, split, rpp, d_frame_map, d_hists, tiles, d_nf);
    else
        k_clahe_tilehist<0><<<grid, 256, 0, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, g.rows, g.cols,
                                                           g.gx, g.tw, g.th, split, rpp, d_frame_map, d_hists, tiles, d_nf);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

int uwip_clahe_launch_tilehist_merge(uwip_ctx *ctx, const uint32_t *d_child, const ClaheGeom &g, int nf, uint32_t *d_hists)
{
    uwip_kscope ks(ctx, "k_clahe_tilehist");
    k_clahe_tilehist_merge<<<dim3((unsigned)(g.gx * g.gy), (unsigned)nf), 256, 0, ctx->stream>>>(d_child, g.gx, g.gx * g.gy, d_hists);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

int uwip_clahe_launch_lut(uwip_ctx *ctx, const ClaheGeom &g, const uint32_t *d_hists, const int *clip, int ncl, const int *d_frame_clip,
                          int nf, int rule, uint8_t *d_luts, uint32_t *d_tile_max, const int *d_nf)
{
    const int tiles = g.gx * g.gy;
    const ClipList cl = make_clip_list(clip, ncl);
    uwip_kscope ks(ctx, "k_clahe_lut");
    k_clahe_lut<<<uwip_cdiv((size_t)tiles * nf, 4), 256, 0, ctx->stream>>>(d_hists, tiles, nf, g.lutScale, cl, d_frame_clip, rule, d_luts, d_tile_max, d_nf);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

// tile histograms + LUT rows in one launch (k_clahe_band) where the geometry allows and the big-tile form does not apply
bool uwip_clahe_band_ok(const uwip_batch_u8 *src, const ClaheGeom &g)
{
    // tw >= 2: the column -> tile division is a multiply-high by floor(2^32 / tw) + 1, which does not exist for tw = 1
    return !big_tile_ok(src, g) && g.tw >= 2 && g.cols >= 16 && g.cols <= 8192 && (long long)g.tw * g.th < 65536 && g.gy <= 4096;
}

int uwip_clahe_launch_band(uwip_ctx *ctx, const uwip_batch_u8 *src, const ClaheGeom &g, const int *d_frame_map, int nf, const int *clip,
                           int ncl, const int *d_frame_clip, int rule, uint8_t *d_luts, uint32_t *d_tile_max, const int *d_nf)
{
    const ClipList cl = make_clip_list(clip, ncl);
    // tiles per block: as many as fill one 64-unit chunk (1024 columns: every lane of the block's eight waves busy), at most
    // 16 (33 KB of LDS: four blocks per CU).  Measured per 64 frames of 1080p (tools/tilehist_only.py): 16 x 16
    // grid (121-pixel tiles) 8 tiles per block 43.9 us, 16 (the whole row) 48.5; 32 x 32 grid (61-pixel tiles) 16 per block
    // 63.1, 32 (the whole row, 66 KB) 66.5, 8 (half the lanes idle) 99.5.
    const int tpb = std::min(g.gx, std::min(16, std::max(1, 1024 / g.tw)));
    const int nparts = (g.gx + tpb - 1) / tpb;
    const int part_cols = std::min(tpb * g.tw, g.cols);
    const int nu = (part_cols + 15) / 16 + 1;                          // a part's columns need not start on a unit boundary
    const int chunks = nu <= 64 ? 1 : (nu <= 128 ? 2 : (nu <= 256 ? 4 : 8));
    const size_t lds = (size_t)tpb * BAND_TSTRIDE * 4;
    const uint32_t magic = (uint32_t)(4294967296ull / (uint64_t)g.tw) + 1u;
    const int tiles = g.gx * g.gy;
    dim3 grid((unsigned)(g.gy * nparts), (unsigned)nf);
    uwip_kscope ks(ctx, "k_clahe_band");
#define UWIP_BAND(C)                                                                                                                   \
    do {                                                                                                                               \
        int rc_l = uwip_lds_optin(ctx, "k_clahe_band" #C, (const void *)k_clahe_band<C>, lds);                                          \
        if (rc_l) return rc_l;                                                                                                         \
        k_clahe_band<C><<<grid, BAND_THREADS, lds, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride, g.rows, g.cols, \
                                                               g.gx, g.tw, magic, g.th, tpb, nparts, d_frame_map, g.lutScale, cl, d_frame_clip, rule, \
                                                               d_luts, d_tile_max, tiles, d_nf);                                        \
    } while (0)
    switch (chunks) {
    case 1: UWIP_BAND(1); break;
    case 2: UWIP_BAND(2); break;
    case 4: UWIP_BAND(4); break;
    default: UWIP_BAND(8); break;
    }
#undef UWIP_BAND
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

int uwip_clahe_build_strips(uwip_ctx *ctx, const ClaheGeom &g, int max_rows, const int4 **d_strips, int *nstrips)
{
    char key[96];
    snprintf(key, sizeof key, "strips:%d:%d:%d:%d", g.rows, g.gy, g.th, max_rows);
    size_t bytes = 0;
    const void *d = uwip_table_find(ctx, key, &bytes);
    if (!d) {
        std::vector<int> ys;
        cell_starts(g.rows, g.gy, g.inv_th, ys);
        std::vector<int4> strips;
        for (int cy = 0; cy <= g.gy; ++cy) {
            const int L = ys[cy + 1] - ys[cy];
            if (L <= 0) continue;
            const int nch = (L + max_rows - 1) / max_rows, rows = (L + nch - 1) / nch;     // balanced chunks
            for (int r = ys[cy]; r < ys[cy + 1]; r += rows)
                strips.push_back(make_int4(cy, r, std::min(r + rows, ys[cy + 1]), 0));
        }
        bytes = strips.size() * sizeof(int4);
        d = uwip_table_put(ctx, key, strips.data(), bytes);
        if (!d) return UWIP_ERR_NOMEM;
    }
    *d_strips = (const int4 *)d;
    *nstrips = (int)(bytes / sizeof(int4));
    return UWIP_OK;
}

ApplyShape uwip_clahe_apply_shape(const ClaheGeom &g)
{
    ApplyShape a;
    const int groups = (g.cols + 7) / 8;
    a.xs = groups >= 128 ? 4 : (groups >= 32 ? 2 : 1);
    const int pg = (groups + a.xs - 1) / a.xs;          // groups per part
    a.TX = 256;
    while (a.TX > 32 && a.TX / 2 >= pg) a.TX /= 2;
    // strips as tall as a cell row (capped): the staged LUT bytes per pixel fall with the strip height
    a.max_rows = std::min(std::max(g.th, 16), 64);
    // a part of pg groups spans at most (8 pg) / tw + 2 cells
    a.lds_cells = std::min(g.gx + 1, (8 * pg + g.tw - 1) / g.tw + 2);
    return a;
}

namespace {

int launch_apply(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, const ClaheGeom &g,
                 const uint8_t *d_luts, size_t lut_fs, const int *d_frame_map, int nf)
{
    const ApplyShape sh = uwip_clahe_apply_shape(g);
    const int4 *d_strips = nullptr;
    int nstrips = 0;
    int rc = uwip_clahe_build_strips(ctx, g, sh.max_rows, &d_strips, &nstrips);
    if (rc) return rc;
    if (nstrips == 0) return UWIP_OK;
    const size_t lds = (size_t)sh.lds_cells * 256 * sizeof(uint32_t);
    const bool vec = uwip_aligned_for(src, 8) && uwip_aligned_for(dst, 8);
    dim3 grid((unsigned)(nstrips * sh.xs), (unsigned)nf);
    uwip_kscope ks(ctx, "k_clahe_apply");
    if (vec)
        k_clahe_apply<true><<<grid, 256, lds, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride,
                                                             (uint8_t *)dst->data, dst->step, dst->frame_stride, g.cols,
                                                             g.gx, g.gy, g.inv_tw, g.inv_th, d_luts, lut_fs, d_strips,
                                                             d_frame_map, sh.TX, sh.xs, nullptr);
    else
        k_clahe_apply<false><<<grid, 256, lds, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride,
                                                              (uint8_t *)dst->data, dst->step, dst->frame_stride, g.cols,
                                                              g.gx, g.gy, g.inv_tw, g.inv_th, d_luts, lut_fs, d_strips,
                                                              d_frame_map, sh.TX, sh.xs, nullptr);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

}  // namespace

int uwip_clahe_launch_apply_mixed(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, const void *d_desc_v, int nf,
                                  int max_blocks, int max_cells)
{
    const ApplyFrame *d_desc = (const ApplyFrame *)d_desc_v;
    if (max_blocks == 0 || nf == 0) return UWIP_OK;
    const size_t lds = (size_t)max_cells * 256 * sizeof(uint32_t);
    const bool vec = uwip_aligned_for(src, 8) && uwip_aligned_for(dst, 8);
    dim3 grid((unsigned)max_blocks, (unsigned)nf);
    uwip_kscope ks(ctx, "k_clahe_apply");
    if (vec)
        k_clahe_apply<true><<<grid, 256, lds, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride,
                                                             (uint8_t *)dst->data, dst->step, dst->frame_stride, src->cols, 0, 0,
                                                             0.f, 0.f, nullptr, 0, nullptr, nullptr, 0, 1, d_desc);
    else
        k_clahe_apply<false><<<grid, 256, lds, ctx->stream>>>((const uint8_t *)src->data, src->step, src->frame_stride,
                                                              (uint8_t *)dst->data, dst->step, dst->frame_stride, src->cols, 0, 0,
                                                              0.f, 0.f, nullptr, 0, nullptr, nullptr, 0, 1, d_desc);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

// ---- exported entry points --------------------------------------------------

UWIP_API int uwip_clahe_luts(uwip_ctx *ctx, const uwip_batch_u8 *src, double clipLimit, int gx, int gy,
                             int residual_rule, uint8_t *d_luts)
{
    int rc = uwip_check_batch(ctx, src, 1);
    if (rc) return rc;
    rc = check_grid(ctx, gx, gy);
    if (rc) return rc;
    if (uwip_batch_empty(src)) return UWIP_OK;
    UWIP_REQUIRE(ctx, d_luts != nullptr, "null LUT buffer");
    const ClaheGeom g = make_geom(src->rows, src->cols, gx, gy);
    const int tiles = gx * gy;
    const int clip = clip_from_limit(clipLimit, g.area);
    if (uwip_clahe_band_ok(src, g)) return uwip_clahe_launch_band(ctx, src, g, nullptr, src->frames, &clip, 1, nullptr, residual_rule, d_luts, nullptr);
    uint32_t *d_hists = (uint32_t *)uwip_ws(ctx, "clahe.tilehist", sizeof(uint32_t) * 256 * (size_t)tiles * src->frames);
    if (!d_hists) return UWIP_ERR_NOMEM;
    rc = uwip_clahe_launch_tilehist(ctx, src, g, nullptr, src->frames, d_hists);
    if (rc) return rc;
    return uwip_clahe_launch_lut(ctx, g, d_hists, &clip, 1, nullptr, src->frames, residual_rule, d_luts);
}

UWIP_API int uwip_clahe(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst, double clipLimit,
                        int gx, int gy, int residual_rule)
{
    int rc = uwip_check_pair(ctx, src, dst);
    if (rc) return rc;
    rc = check_grid(ctx, gx, gy);
    if (rc) return rc;
    if (uwip_batch_empty(src)) return UWIP_OK;
    const ClaheGeom g = make_geom(src->rows, src->cols, gx, gy);
    const int tiles = gx * gy;
    uint8_t *d_luts = (uint8_t *)uwip_ws(ctx, "clahe.luts", (size_t)256 * tiles * src->frames);
    if (!d_luts) return UWIP_ERR_NOMEM;
    rc = uwip_clahe_luts(ctx, src, clipLimit, gx, gy, residual_rule, d_luts);
    if (rc) return rc;
    return launch_apply(ctx, src, dst, g, d_luts, (size_t)tiles * 256, nullptr, src->frames);
}

UWIP_API int uwip_clahe_per_frame(uwip_ctx *ctx, const uwip_batch_u8 *src, const uwip_batch_u8 *dst,
                                  const double *h_clipLimit, const int32_t *h_grid, int residual_rule)
{
    int rc = uwip_check_pair(ctx, src, dst);
    if (rc) return rc;
    if (uwip_batch_empty(src)) return UWIP_OK;
    UWIP_REQUIRE(ctx, h_clipLimit && h_grid, "null parameter arrays");
    const int F = src->frames;
    for (int f = 0; f < F; ++f) {
        rc = check_grid(ctx, h_grid[f], h_grid[f]);
        if (rc) return rc;
    }
    // group frames by grid size; one (tilehist, lut, apply) triple per group
    std::vector<int> order(F);
    for (int f = 0; f < F; ++f) order[f] = f;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h_grid[a] < h_grid[b]; });
    int *h_map = (int *)uwip_host_ws(ctx, "clahe.pf.map", sizeof(int) * 2 * (size_t)F);
    int *d_map = (int *)uwip_ws(ctx, "clahe.pf.map", sizeof(int) * 2 * (size_t)F);
    ApplyFrame *h_desc = (ApplyFrame *)uwip_host_ws(ctx, "clahe.pf.desc", sizeof(ApplyFrame) * (size_t)F);
    ApplyFrame *d_desc = (ApplyFrame *)uwip_ws(ctx, "clahe.pf.desc", sizeof(ApplyFrame) * (size_t)F);
    if (!h_map || !d_map || !h_desc || !d_desc) return UWIP_ERR_NOMEM;
    UWIP_HIP(ctx, uwip_stream_wait(ctx));
    int *h_clip = h_map + F, *d_clip = d_map + F;
    for (int i = 0; i < F; ++i) {
        const int f = order[i];
        h_map[i] = f;
        const ClaheGeom g = make_geom(src->rows, src->cols, h_grid[f], h_grid[f]);
        h_clip[i] = clip_from_limit(h_clipLimit[f], g.area);
    }
    UWIP_HIP(ctx, hipMemcpyAsync(d_map, h_map, sizeof(int) * 2 * (size_t)F, hipMemcpyHostToDevice, ctx->stream));
    size_t max_tiles = 0;
    for (int f = 0; f < F; ++f) max_tiles = std::max(max_tiles, (size_t)h_grid[f] * h_grid[f]);
    uint32_t *d_hists = (uint32_t *)uwip_ws(ctx, "clahe.tilehist", sizeof(uint32_t) * 256 * max_tiles * F);
    uint8_t *d_luts = (uint8_t *)uwip_ws(ctx, "clahe.luts", (size_t)256 * max_tiles * F);
    if (!d_hists || !d_luts) return UWIP_ERR_NOMEM;
    // per group of equal grid size: tile histograms and LUTs (small launches; every group keeps its own LUT range, the
    // interpolation reads them all); the interpolation itself
    // then runs ONCE over all frames with a per-frame descriptor (a launch per group would be too short to reach the
    // HBM rate: at 4K 16 frames split three ways ran at 29 % of peak, the single launch at 41 %)
    int i = 0, max_blocks = 0, max_cells = 0;
    size_t loff = 0;
    while (i < F) {
        int j = i;
        const int gsz = h_grid[order[i]];
        while (j < F && h_grid[order[j]] == gsz) ++j;
        const int nf = j - i;
        const ClaheGeom g = make_geom(src->rows, src->cols, gsz, gsz);
        const int tiles = gsz * gsz;
        if (uwip_clahe_band_ok(src, g)) {
            rc = uwip_clahe_launch_band(ctx, src, g, d_map + i, nf, nullptr, 1, d_clip + i, residual_rule, d_luts + loff, nullptr);
            if (rc) return rc;
        } else {
            rc = uwip_clahe_launch_tilehist(ctx, src, g, d_map + i, nf, d_hists);
            if (rc) return rc;
            rc = uwip_clahe_launch_lut(ctx, g, d_hists, nullptr, 1, d_clip + i, nf, residual_rule, d_luts + loff);
            if (rc) return rc;
        }
        // d_hists is reused by the next group: stream order keeps that safe
        const ApplyShape sh = uwip_clahe_apply_shape(g);
        const int4 *d_strips = nullptr;
        int nstrips = 0;
        rc = uwip_clahe_build_strips(ctx, g, sh.max_rows, &d_strips, &nstrips);
        if (rc) return rc;
        for (int k = 0; k < nf; ++k) {
            ApplyFrame &a = h_desc[i + k];
            a.strips = d_strips; a.luts = d_luts + loff + (size_t)k * tiles * 256; a.fr = order[i + k];
            a.nstrips = nstrips; a.gx = g.gx; a.gy = g.gy; a.TX = sh.TX; a.xs = sh.xs; a.inv_tw = g.inv_tw; a.inv_th = g.inv_th;
        }
        max_blocks = std::max(max_blocks, nstrips * sh.xs);
        max_cells = std::max(max_cells, sh.lds_cells);
        loff += (size_t)tiles * 256 * nf;
        i = j;
    }
    UWIP_HIP(ctx, hipMemcpyAsync(d_desc, h_desc, sizeof(ApplyFrame) * (size_t)F, hipMemcpyHostToDevice, ctx->stream));
    return uwip_clahe_launch_apply_mixed(ctx, src, dst, d_desc, F, max_blocks, max_cells);
}
