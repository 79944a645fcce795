// uwip_keyframe_chain_host: the key-frame chain of a pipe (kf_chain.hpp) run on the host, batch by batch and round by
// round as the device runs it, with the matcher replaced by a callback.  What the device's walker reads, this one reads
// from the same places (round 0's fixed list, the fallback lists the walker writes, the slot carry), so a test of this
// function against the reference loop is a test of the device chain's logic.
#include "uwip_internal.hpp"
#include <algorithm>
#include <vector>

UWIP_API int uwip_keyframe_chain_host(const uwip_keyframe_config *kc, int n_frames, int batch, uwip_kf_overlap_fn overlap,
                                      uwip_kf_blur_fn blur, void *user, uwip_keyframe_row *rows, int cap, int *n_rows, int32_t *rounds)
{
    if (!kc || !uwip_kf::config_ok(*kc) || n_frames < 0 || batch < 1 || batch + 2 > 4096 || !overlap || !blur || !n_rows || cap < 0 ||
        (cap > 0 && !rows))
        return UWIP_ERR_INVALID;
    *n_rows = 0;
    if (n_frames == 0) return UWIP_OK;
    const int F = batch, P0 = uwip_kf::round0_pairs(F, kc->lookback), R = uwip_kf::max_rounds(F, kc->lookback, kc->kWindow);
    const size_t npo = (size_t)P0 + (size_t)R * F;
    std::vector<int32_t> r0(2 * (size_t)P0), out_info(8 * npo), info(8 * (size_t)F), fb_key(R + 1), fb_start(R + 1), fb_list(2 * (size_t)F);
    std::vector<float> out_ratio(npo), blurv(F), ratio(F);
    std::vector<uwip_keyframe_row> ring((size_t)n_frames + 1);     // a row closes at most once per frame: nothing wraps
    std::vector<int32_t> slot_index(F + 2, -1);                    // stream index of the frame each feature slot holds
    int32_t fb_n = 0;
    uwip_kf::round0_list(F, kc->lookback, r0.data(), r0.data() + P0);
    uwip_kf::State st{};
    st.carry_key = st.carry_best = -1;
    uwip_kf::Bufs u;
    u.out_ratio = out_ratio.data(); u.out_info = out_info.data(); u.blur = blurv.data(); u.ratio = ratio.data(); u.info = info.data();
    u.ring = ring.data(); u.fb_key = fb_key.data(); u.fb_start = fb_start.data(); u.fb_q = fb_list.data(); u.fb_t = fb_list.data() + F;
    u.fb_n = &fb_n;
    const int nb = (n_frames + F - 1) / F;
    for (int kb = 0; kb < nb; ++kb) {
        uwip_kf::Batch b;
        b.F = F; b.D = kc->lookback; b.kWindow = kc->kWindow; b.base = kb * F; b.valid = std::min(F, n_frames - b.base);
        b.rounds = R; b.max_rows = (int32_t)ring.size(); b.minOverlap = kc->minOverlap; b.first = kb == 0; b.last = kb == nb - 1;
        // detect: slots 1..F; the last batch is padded with the final frame (what uwpipe does)
        for (int i = 0; i < F; ++i) slot_index[1 + i] = std::min(b.base + i, n_frames - 1);
        if (b.first) slot_index[0] = slot_index[1];
        for (int i = 0; i < F; ++i) blurv[i] = blur(user, slot_index[1 + i]);
        for (int p = 0; p < P0; ++p) out_ratio[p] = overlap(user, slot_index[r0[P0 + p]], slot_index[r0[p]]);
        uwip_kf::walk(b, st, u, 0);
        for (int r = 1; r <= R; ++r) {
            const size_t at = (size_t)P0 + (size_t)(r - 1) * F;
            for (int j = 0; j < fb_n; ++j) out_ratio[at + j] = overlap(user, slot_index[u.fb_t[j]], slot_index[u.fb_q[j]]);
            uwip_kf::walk(b, st, u, r);
        }
        if (rounds) rounds[kb] = st.nfb;
        // the carry kernel
        if (st.carry_key >= 0) slot_index[0] = slot_index[st.carry_key];
        if (st.carry_best >= 0) slot_index[F + 1] = slot_index[st.carry_best];
    }
    if (st.err) return UWIP_ERR_INVALID;
    *n_rows = (int)st.total;
    std::copy(ring.begin(), ring.begin() + std::min<size_t>(st.total, (size_t)cap), rows);
    return UWIP_OK;
}
