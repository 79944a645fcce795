// videostrip overlap path, matching: brute-force Hamming kNN(2) of binary descriptors as a dense distance matrix on MFMA.
#include "overlap_internal.hpp"

namespace {

// ---- brute-force Hamming kNN(2): dense q x t dot products on i8 MFMA -------------------------------------
// popcount(a xor b) = |a| + |b| - 2 a.b with a, b in {0,1}^512 held as bytes; QT query tiles of 16 per wave, so every
// train fragment read from LDS feeds QT MFMAs.
typedef int v4i __attribute__((ext_vector_type(4)));
// Row stride of a staged train tile: 512 + 32 bytes.  A ds_read_b128 is served in four groups of 16 lanes --
// {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32 (MI355X_MICROARCH.md, LDS) -- i.e. rows of two neighbouring
// 16-byte columns kb, kb + 1 in one group; with a stride of 8 dwords mod 64 the 16-byte slot of (row, kb) is (2 row + kb) mod 16:
// the even kb of a group takes the even slots, the odd one the odd slots -- conflict-free.  (Rounds 1-3 used 512 + 16:
// slot (row + kb) mod 16, where row 11 of column kb + 1 meets row 12 of column kb -- SQ_LDS_BANK_CONFLICT was 42 % of
// SQ_LDS_IDX_ACTIVE, profiles/r04_matcher_counters.txt before the change.)
constexpr int MT_ROW = DESC_K + 32;

// Top-2 of (distance, index) pairs under the order "smaller distance, then lower index" (BFMatcher::knnMatch k = 2 with
// ties to the lower train index) on PACKED keys: key = distance << 11 | index (distance <= 512, index < 2048), so
// the lexicographic order is the integer order and one candidate costs a max and two mins instead of two
// compares and four selects per slot.  b0 <= b1 always; empty slots hold MT_EMPTY.
constexpr uint32_t MT_EMPTY = 0xffffffffu;
__device__ __forceinline__ void top2_push(uint32_t &b0, uint32_t &b1, uint32_t k)
{
    b1 = min(b1, max(b0, k));     // the second smallest of three (b0 <= b1)
    b0 = min(b0, k);
}

// Software-pipelined (round 4).  What the ISA of the plain form of rounds 2-3 showed (llvm-objdump): (i) the four
// `tpop` loads of a tile sit behind four lane-mask branches, each followed by `s_waitcnt vmcnt(0)` -- four serialised
// global-memory round trips per 64 MFMAs; (ii) the whole top-2 epilogue of a tile (112 vector instructions) runs AFTER its
// 64 MFMAs, right before the barrier, so all eight waves of the block alternate between a matrix phase and a vector
// phase in step; (iii) the B fragments are read two at a time and waited for at once.  Here:
//   * the train keys ((|b| + 512) << 11 | t, or the dead-column key) travel with the tile: fetched by 64 threads a
//     tile ahead, parked in LDS beside the descriptors, read back with one ds_read_b32 per 16 columns;
//   * the B fragments of column group tt + 1 are requested before the MFMAs of group tt (two register sets);
//   * the epilogue of group tt - 1 (the last group's: of the previous tile) is issued between the MFMAs of group tt
//     -- an MFMA holds the SIMD's vector issue for 8 of its 16 cycles, two vector instructions fit in the rest
//     (MI355X_MICROARCH.md, "vector-instruction ISSUE cost") -- pinned with sched_group_barrier.
// Same results bit for bit (packed-key top-2 is order-independent).
template <int QT, int NW, int TG>      // TG: column groups of 16 per staged train tile: one barrier per TG * 16 columns
__global__ __launch_bounds__(64 * NW) void k_ov_match_sp(const int8_t *__restrict__ qbits, const int32_t *__restrict__ qpop,
                                                    const int32_t *__restrict__ qn, const int8_t *__restrict__ tbits,
                                                    const int32_t *__restrict__ tpop, const int32_t *__restrict__ tn,
                                                    const int32_t *__restrict__ pair_q, const int32_t *__restrict__ pair_t,
                                                    int32_t *__restrict__ out_idx /*[P][MAXKP][2]*/, int32_t *__restrict__ out_dist,
                                                    const int32_t *__restrict__ d_npairs /*null: every launched pair*/)
{
    extern __shared__ __attribute__((aligned(16))) int8_t s_t[];      // 2 x [64][MT_ROW] descriptors, then 2 x [64] keys
    const int p = blockIdx.y;
    if (d_npairs && p >= *d_npairs) return;
    const int fq = pair_q[p], ft = pair_t[p];
    const int nq = qn[fq], nt = tn[ft];
    const int q0 = blockIdx.x * (16 * NW * QT);
    if (q0 >= nq) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = lane & 15, kb = lane >> 4;
    const int8_t *Q = qbits + (size_t)fq * MAXKP * DESC_K;
    const int8_t *T = tbits + (size_t)ft * MAXKP * DESC_K;
    const int32_t *TP = tpop + (size_t)ft * MAXKP;
    v4i a[QT][8];
    int cq[QT][4];
    uint32_t b0[QT][4], b1[QT][4];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
        const int qrow = q0 + (wave * QT + u) * 16 + row;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            a[u][ks] = *reinterpret_cast<const v4i *>(Q + (size_t)qrow * DESC_K + ks * 64 + kb * 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            cq[u][r] = qpop[(size_t)fq * MAXKP + q0 + (wave * QT + u) * 16 + kb * 4 + r];
            b0[u][r] = b1[u][r] = MT_EMPTY;
        }
    }
    constexpr int TC = TG * 16;               // train columns per tile
    constexpr int NP = TC * 32 / (64 * NW);   // 16-byte pieces per thread
    constexpr int NK = (TC + 63) / 64;        // keys per lane
    constexpr uint32_t DEAD = 0x7ff00000u;
    v4i stage[NP];
    uint32_t stage_key[NK];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = threadIdx.x + 64 * NW * j, tr = i >> 5, piece = i & 31;
            stage[j] = *reinterpret_cast<const v4i *>(T + (size_t)(t0 + tr) * DESC_K + piece * 16);
        }
        // the tile's 64 train keys (rows up to MAXKP exist; dead ones get the dead key): every wave loads and parks the
        // same 64 values -- no branch, so the loop body stays ONE basic block and the scheduler may interleave it
#pragma unroll
        for (int j = 0; j < NK; ++j) {
        const int t = t0 + lane + 64 * j;
        const uint32_t pc = (uint32_t)TP[min(t, MAXKP - 1)];
        // live keys are < 0x200800; a dead column ORs the dead key in (any key >= DEAD is dead).  Written as an OR, not
        // as a select between the two keys: a select whose one arm comes from a load is turned into a branch around the
        // load, with a vmcnt(0) wait inside it
        stage_key[j] = (((pc + 512u) << 11) | (uint32_t)t) | (t < nt ? 0u : DEAD);
        }
    };
    int8_t *const bufA = s_t, *const bufB = s_t + (size_t)TC * MT_ROW;
    uint32_t *const keyA = reinterpret_cast<uint32_t *>(s_t + (size_t)2 * TC * MT_ROW), *const keyB = keyA + TC;
    auto park = [&](int8_t *buf, uint32_t *kbuf) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = threadIdx.x + 64 * NW * j, tr = i >> 5, piece = i & 31;
            *reinterpret_cast<v4i *>(buf + (size_t)tr * MT_ROW + piece * 16) = stage[j];
        }
#pragma unroll
        for (int j = 0; j < NK; ++j) if (lane + 64 * j < TC) kbuf[lane + 64 * j] = stage_key[j];
    };
    if (nt > 0) {
        fetch(0);
        park(bufA, keyA);
        fetch(TC);                            // MAXKP >= 2 TC: the rows exist; keys past nt are dead
    }
    __syncthreads();
    // Two accumulator sets: group tt multiplies into acc[tt & 1] while the results of group tt - 1 in acc[(tt + 1) & 1] (for
    // tt = 0: the previous tile's last group) go through the top-2 insertion.  An even number of groups per tile, so the parity carries
    // over the tile loop without a register copy.
    v4i acc[2][QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) acc[1][u] = v4i{0, 0, 0, 0};
    uint32_t tb_last = DEAD;                  // key of the pending group of the previous tile (none yet: dead)
    auto epilogue_one = [&](const v4i (&ac)[QT], uint32_t tbk, int idx) {
        const int u = idx >> 2, r = idx & 3;
        const int mf = tbk >= DEAD ? 0 : -4096;
        top2_push(b0[u][r], b1[u][r], (uint32_t)(__mul24(ac[u][r], mf) + (int)tbk));
    };
    static_assert(TG % 2 == 0 && TC * 32 % (64 * NW) == 0, "tile shape");
    for (int t0 = 0, it = 0; t0 < nt; t0 += TC, ++it) {
        const int8_t *cur = (it & 1) ? bufB : bufA;
        const uint32_t *kcur = (it & 1) ? keyB : keyA;
        uint32_t tb[TG];
#pragma unroll
        for (int tt = 0; tt < TG; ++tt) tb[tt] = kcur[tt * 16 + row];
        v4i bf[2][8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            bf[0][ks] = *reinterpret_cast<const v4i *>(cur + (size_t)row * MT_ROW + ks * 64 + kb * 16);
#pragma unroll
        for (int tt = 0; tt < TG; ++tt) {
            if (tt < TG - 1) {
#pragma unroll
                for (int ks = 0; ks < 8; ++ks)
                    bf[(tt + 1) & 1][ks] = *reinterpret_cast<const v4i *>(cur + (size_t)((tt + 1) * 16 + row) * MT_ROW + ks * 64 + kb * 16);
            }
            const uint32_t tbk = tt == 0 ? tb_last : tb[(tt + TG - 1) % TG];
#pragma unroll
            for (int u = 0; u < QT; ++u) acc[tt & 1][u] = v4i{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
                for (int u = 0; u < QT; ++u)
                    acc[tt & 1][u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[u][ks], bf[tt & 1][ks], acc[tt & 1][u], 0, 0, 0);
                // QT * 4 pending results over the 8 steps
                if (QT * 4 >= 8) {
#pragma unroll
                    for (int e = 0; e < QT * 4 / 8; ++e) epilogue_one(acc[(tt + 1) & 1], tbk, ks * (QT * 4 / 8) + e);
                } else if ((ks & 1) == 0) {
                    epilogue_one(acc[(tt + 1) & 1], tbk, ks >> 1);
                }
            }
        }
        tb_last = tb[TG - 1];
        // unconditional (clamped) staging of the next tiles: a branch here would split the body and let the compiler sink
        // the epilogue behind it; the last two tiles park / fetch rows nobody reads
        park((it & 1) ? bufA : bufB, (it & 1) ? keyA : keyB);
        fetch(min(t0 + 2 * TC, MAXKP - TC));
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < QT * 4; ++i) epilogue_one(acc[1], tb_last, i);
#pragma unroll
    for (int u = 0; u < QT; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const uint32_t o0 = (uint32_t)__shfl_xor((int)b0[u][r], d, 64), o1 = (uint32_t)__shfl_xor((int)b1[u][r], d, 64);
                top2_push(b0[u][r], b1[u][r], o0);
                top2_push(b0[u][r], b1[u][r], o1);
            }
            const int q = q0 + (wave * QT + u) * 16 + kb * 4 + r;
            if (row == 0 && q < nq) {
                const size_t o = ((size_t)p * MAXKP + q) * 2;
                const bool h0 = b0[u][r] < DEAD, h1 = b1[u][r] < DEAD;
                out_idx[o] = h0 ? (int)(b0[u][r] & 2047u) : -1; out_idx[o + 1] = h1 ? (int)(b1[u][r] & 2047u) : -1;
                out_dist[o] = h0 ? (int)(b0[u][r] >> 11) - 512 + cq[u][r] : -1;
                out_dist[o + 1] = h1 ? (int)(b1[u][r] >> 11) - 512 + cq[u][r] : -1;
            }
        }
}

// ---- the same matcher on the FP4 form of the f8f6f4 MFMA (round 5) ---------------------------------------------------------
// v_mfma_scale_f32_16x16x128_f8f6f4 with both operands E2M1: a descriptor bit travels as a NIBBLE (0x0 = 0.0, 0x2 = 1.0), 256
// bytes per 512-bit descriptor instead of the 512 of the i8 form -- half the global and LDS bytes per MAC -- and one
// instruction covers K = 128: four MFMAs per 16 x 16 x 512 tile instead of eight, at the cycles of the i8 instruction (twice
// its MAC rate; MI355X_MICROARCH.md, Matrix cores).  Block scales are E8M0 bytes of 127 = 2^0.  The products are 0 or 1 and a
// sum is at most 512: exact in the float32 accumulator.  The packed key (distance, train index) is formed and compared as
// FLOAT -- (|t| + 512 - 2 a.b) * 2048 + t < 2^22 is exact in float32, one v_fma_f32 from the accumulator, v_min / v_max_f32
// for the top-2 insertion: the same four vector instructions per result as the integer form -- and converted once at the end.
// Both operands' lanes read their 32 nibbles of a K = 128 step from the same byte offsets of a descriptor, so whatever k
// order the hardware assigns inside a lane, the two sides agree: the sum is the dot product.
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int F4_DESC = DESC_NIBW * 4;                 // 256 bytes per descriptor
constexpr int F4_ROW = F4_DESC + 32;                   // LDS row stride (the i8 form's argument: 2 row + kb mod 16 slots)
constexpr float F4_DEAD = 8388608.0f;                  // any key >= 2^23 is dead (live keys are < 2^22)
constexpr float F4_EMPTY = 3.0e9f;
// b0 <= b1 always, so the new second-best min(b1, max(b0, k)) is the MEDIAN of (b0, b1, k): one v_med3_f32 instead of a
// max and a min -- three vector instructions per result (fma, med3, min) where the integer form has four
__device__ __forceinline__ void top2_push_f(float &b0, float &b1, float k)
{
    b1 = __builtin_amdgcn_fmed3f(b0, b1, k);
    b0 = fminf(b0, k);
}
__device__ __forceinline__ v4f mfma_f4(const v4i &a, const v4i &b, const v4f &c)
{
    const v8i A = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, B = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
    // cbsz = blgp = 4: FP4 E2M1 on both sides; scale operands: four E8M0 bytes of 127 (x 1.0), byte 0 selected
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, B, c, 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}
template <int QT, int NW, int TG>
__global__ __launch_bounds__(64 * NW) void k_ov_match_f4(const uint32_t *__restrict__ qnib, const int32_t *__restrict__ qpop,
                                                    const int32_t *__restrict__ qn, const uint32_t *__restrict__ tnib,
                                                    const int32_t *__restrict__ tpop, const int32_t *__restrict__ tn,
                                                    const int32_t *__restrict__ pair_q, const int32_t *__restrict__ pair_t,
                                                    int32_t *__restrict__ out_idx /*[P][MAXKP][2]*/, int32_t *__restrict__ out_dist,
                                                    const int32_t *__restrict__ d_npairs /*null: every launched pair*/)
{
    extern __shared__ __attribute__((aligned(16))) int8_t s_t[];      // 2 x [TC][F4_ROW] descriptors, then 2 x [TC] keys
    const int p = blockIdx.y;
    if (d_npairs && p >= *d_npairs) return;
    const int fq = pair_q[p], ft = pair_t[p];
    const int nq = qn[fq], nt = tn[ft];
    const int q0 = blockIdx.x * (16 * NW * QT);
    if (q0 >= nq) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = lane & 15, kb = lane >> 4;
    const int8_t *Q = reinterpret_cast<const int8_t *>(qnib) + (size_t)fq * MAXKP * F4_DESC;
    const int8_t *T = reinterpret_cast<const int8_t *>(tnib) + (size_t)ft * MAXKP * F4_DESC;
    const int32_t *TP = tpop + (size_t)ft * MAXKP;
    v4i a[QT][4];
    int cq[QT][4];
    float b0[QT][4], b1[QT][4];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
        const int qrow = q0 + (wave * QT + u) * 16 + row;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            a[u][ks] = *reinterpret_cast<const v4i *>(Q + (size_t)qrow * F4_DESC + ks * 64 + kb * 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            cq[u][r] = qpop[(size_t)fq * MAXKP + q0 + (wave * QT + u) * 16 + kb * 4 + r];
            b0[u][r] = b1[u][r] = F4_EMPTY;
        }
    }
    constexpr int TC = TG * 16;               // train columns per tile
    constexpr int NP = TC * 16 / (64 * NW);   // 16-byte pieces per thread
    constexpr int NK = (TC + 63) / 64;        // keys per lane
    static_assert(TG % 2 == 0 && TC * 16 % (64 * NW) == 0 && NP >= 1, "tile shape");
    v4i stage[NP];
    float stage_key[NK];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = threadIdx.x + 64 * NW * j, tr = i >> 4, piece = i & 15;
            stage[j] = *reinterpret_cast<const v4i *>(T + (size_t)(t0 + tr) * F4_DESC + piece * 16);
        }
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const int t = t0 + lane + 64 * j;
            const int pc = TP[min(t, MAXKP - 1)];
            // live: (|t| + 512) * 2048 + t, exact in float32; a dead column adds 2^23 (no select on a loaded value: see the i8 form)
            stage_key[j] = (float)(((pc + 512) << 11) | t) + (t < nt ? 0.0f : F4_DEAD);
        }
    };
    int8_t *const bufA = s_t, *const bufB = s_t + (size_t)TC * F4_ROW;
    float *const keyA = reinterpret_cast<float *>(s_t + (size_t)2 * TC * F4_ROW), *const keyB = keyA + TC;
    auto park = [&](int8_t *buf, float *kbuf) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = threadIdx.x + 64 * NW * j, tr = i >> 4, piece = i & 15;
            *reinterpret_cast<v4i *>(buf + (size_t)tr * F4_ROW + piece * 16) = stage[j];
        }
#pragma unroll
        for (int j = 0; j < NK; ++j) if (lane + 64 * j < TC) kbuf[lane + 64 * j] = stage_key[j];
    };
    if (nt > 0) {
        fetch(0);
        park(bufA, keyA);
        fetch(TC);
    }
    __syncthreads();
    v4f acc[2][QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) acc[1][u] = v4f{0.f, 0.f, 0.f, 0.f};
    float tb_last = F4_DEAD;
    auto epilogue_one = [&](const v4f (&ac)[QT], float tbk, int idx) {
        const int u = idx >> 2, r = idx & 3;
        const float mf = tbk >= F4_DEAD ? 0.0f : -4096.0f;
        top2_push_f(b0[u][r], b1[u][r], fmaf(ac[u][r], mf, tbk));
    };
    for (int t0 = 0, it = 0; t0 < nt; t0 += TC, ++it) {
        const int8_t *cur = (it & 1) ? bufB : bufA;
        const float *kcur = (it & 1) ? keyB : keyA;
        float tb[TG];
#pragma unroll
        for (int tt = 0; tt < TG; ++tt) tb[tt] = kcur[tt * 16 + row];
        v4i bf[2][4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            bf[0][ks] = *reinterpret_cast<const v4i *>(cur + (size_t)row * F4_ROW + ks * 64 + kb * 16);
#pragma unroll
        for (int tt = 0; tt < TG; ++tt) {
            if (tt < TG - 1) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    bf[(tt + 1) & 1][ks] = *reinterpret_cast<const v4i *>(cur + (size_t)((tt + 1) * 16 + row) * F4_ROW + ks * 64 + kb * 16);
            }
            const float tbk = tt == 0 ? tb_last : tb[(tt + TG - 1) % TG];
#pragma unroll
            for (int u = 0; u < QT; ++u) acc[tt & 1][u] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
                for (int u = 0; u < QT; ++u) acc[tt & 1][u] = mfma_f4(a[u][ks], bf[tt & 1][ks], acc[tt & 1][u]);
                // the QT * 4 pending results of the previous group over the 4 steps of this one
#pragma unroll
                for (int e = 0; e < QT; ++e) epilogue_one(acc[(tt + 1) & 1], tbk, ks * QT + e);
            }
        }
        tb_last = tb[TG - 1];
        park((it & 1) ? bufA : bufB, (it & 1) ? keyA : keyB);
        fetch(min(t0 + 2 * TC, MAXKP - TC));
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < QT * 4; ++i) epilogue_one(acc[1], tb_last, i);
#pragma unroll
    for (int u = 0; u < QT; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const float o0 = __shfl_xor(b0[u][r], d, 64), o1 = __shfl_xor(b1[u][r], d, 64);
                top2_push_f(b0[u][r], b1[u][r], o0);
                top2_push_f(b0[u][r], b1[u][r], o1);
            }
            const int q = q0 + (wave * QT + u) * 16 + kb * 4 + r;
            if (row == 0 && q < nq) {
                const size_t o = ((size_t)p * MAXKP + q) * 2;
                const bool h0 = b0[u][r] < F4_DEAD, h1 = b1[u][r] < F4_DEAD;
                const int k0 = h0 ? (int)b0[u][r] : 0, k1 = h1 ? (int)b1[u][r] : 0;
                out_idx[o] = h0 ? (k0 & 2047) : -1; out_idx[o + 1] = h1 ? (k1 & 2047) : -1;
                out_dist[o] = h0 ? (k0 >> 11) - 512 + cq[u][r] : -1;
                out_dist[o + 1] = h1 ? (k1 >> 11) - 512 + cq[u][r] : -1;
            }
        }
}

}  // namespace

int uwip_overlap_knn(uwip_ctx *ctx, const uwip_features *fq, const uwip_features *ft, const int32_t *d_pq, const int32_t *d_pt,
                     const int32_t *d_npairs, int npairs, int32_t *m_idx, int32_t *m_dist)
{
    uwip_kscope ks(ctx, "k_ov_match");
    constexpr int QT = 2;            // 2 query tiles of 16 per wave
    // UWIP_MATCH_FORM: 4 (default) FP4 operands; 3 the i8 form of round 4; 5 / 6 experimental FP4 shapes
    auto read_form = [] { const char *e = std::getenv("UWIP_MATCH_FORM"); return e && *e ? std::atoi(e) : 4; };
    static const int form_once = read_form();
    const int form = uwip_test_hooks() ? read_form() : form_once;      // tests switch forms inside one process
    // one form: `kernel` with nw waves per block and `lds` bytes of dynamic LDS on the operands qd / td (0/1 bytes or FP4 nibbles)
    auto launch = [&](const char *name, auto kernel, int nw, size_t lds, auto *qd, auto *td) -> int {
        if (int rc = uwip_lds_optin(ctx, name, (const void *)kernel, lds)) return rc;
        kernel<<<dim3(MAXKP / (16 * nw * QT), npairs), 64 * nw, lds, ctx->stream>>>(qd, fq->d_pop, fq->d_n, td, ft->d_pop, ft->d_n, d_pq,
                                                                                   d_pt, m_idx, m_dist, d_npairs);
        UWIP_HIP(ctx, hipGetLastError());
        return UWIP_OK;
    };
    const size_t ldsi8 = (size_t)2 * 64 * MT_ROW + 2 * 64 * sizeof(uint32_t);
    const size_t ldsf4 = (size_t)2 * 64 * F4_ROW + 2 * 64 * sizeof(float), ldsf8 = (size_t)2 * 128 * F4_ROW + 2 * 128 * sizeof(float);
    switch (form) {                  // unknown values run the default
    case 3: return launch("k_ov_match_sp<2,8,4>", k_ov_match_sp<QT, 8, 4>, 8, ldsi8, fq->d_bits, ft->d_bits);   // round 4's i8 form
    case 5: return launch("k_ov_match_f4<2,8,8>", k_ov_match_f4<QT, 8, 8>, 8, ldsf8, fq->d_nib, ft->d_nib);     // FP4, 128 train columns per barrier
    case 6: return launch("k_ov_match_f4<2,4,4>", k_ov_match_f4<QT, 4, 4>, 4, ldsf4, fq->d_nib, ft->d_nib);     // FP4, 4-wave blocks
    default: return launch("k_ov_match_f4<2,8,4>", k_ov_match_f4<QT, 8, 4>, 8, ldsf4, fq->d_nib, ft->d_nib);    // FP4 operands (round 5)
    }
}
